"""Opt-in FAR-FIELD attention reuse across sampler steps of the three DiTs: the keys inside the frame window fresh on every step,
the keys outside it from the last step that computed them, merged by their log-sum-exps -- an extension, the reference has none.

`attn_window` alone drops every key outside the window (wrong for a head that spreads its softmax mass), `attn_reuse` replays the
whole attention output (the near field is as stale as the far field).  Two partial attentions over DISJOINT key sets, each with the
log2-domain log-sum-exp of the keys it visited, combine into the exact attention over the union, so a layer's keys are split into
the window (near) and its complement (far):

    refresh forward    per layer: the NEAR launch (the grid-aligned window table; O into the attention-output buffer, LSE into an
                       fp32 scratch), the FAR launches (the complement table; one per sample, O and LSE straight into that
                       sample's cache entry [layer] -- no staging, no copy), the MERGE (alg_attn_merge_lse, in place, per sample).
                       The result is the exact softmax over all keys formed from two bf16-rounded partials: not bit-identical to
                       the dense entry (docs/numerics.md)
    reusing forward    per layer: the near launch, then the merge against the cached entry.  Everything in front of the attention
                       (norm, Q|K, V^T, RoPE) runs, unlike with attn_reuse.  The merge weights come from THIS step's near LSE, so
                       a head whose near mass grows leans on its fresh part

The rule and the keys are attn_reuse.AttnReuse's (this module subclasses it for the buffers): entries keyed by the role of the
pass, reuse iff t_lo < t < t_hi and every key holds an entry of age 1 .. N - 1, one decision per forward from the SCHEDULE -- no
host round trip, forwards can be captured once the tables exist.  Steps outside (t_lo, t_hi) are refresh steps: exact attention,
not window-only.  A dense step (attn_window_dense_steps) launches the dense entry and leaves the entries invalid; where the window
covers the video (frame_window_ranges gives None) the layer launches dense and nothing is cached.

The tables: a partition is exact only if no key is visited twice, and the kernels round a range's begin down to the 64-key grid,
so the near table is attn_window.grid_aligned(window table) and the far one attn_window.complement_ranges(near).

Memory: layers x keys x (rows x D x 2 + heads x rows x 4) bytes, plus one fp32 [samples][heads][rows] scratch.
"""
from __future__ import annotations

import torch

from . import _lib
from .attn_reuse import T_HI, T_LO, AttnReuse, StepKeys, parse_timesteps, step_keys   # noqa: F401  (the keys are shared)
from .attn_window import SelfAttnOperands, complement_ranges, grid_aligned

BF = torch.bfloat16


def check_switches(every, t_lo=T_LO, t_hi=T_HI):
    """(every, t_lo, t_hi) as ints; every: 0 = off, 1 is refused (every step would refresh), N >= 2; t_lo < t_hi."""
    if isinstance(every, bool) or int(every) != every:
        raise ValueError("attn_far_reuse=%r: an int -- 0 = off, N >= 2 refreshes the far field on every N-th step" % (every,))
    every, t_lo, t_hi = int(every), int(t_lo), int(t_hi)
    if every < 0 or every == 1:
        raise ValueError("attn_far_reuse=%d: 0 = off, N >= 2 refreshes the far field on every N-th step (1 would reuse nothing)" % every)
    if t_lo >= t_hi:
        raise ValueError("attn_far_reuse_t_lo=%d >= attn_far_reuse_t_hi=%d: a step reuses only while t_lo < t < t_hi" % (t_lo, t_hi))
    return every, t_lo, t_hi


def switches_from(kw):
    """from_pretrained's three keywords taken out of its trailing keywords `kw`: a dict with the defaults filled in, validated."""
    every, t_lo, t_hi = check_switches(kw.pop("attn_far_reuse", 0), kw.pop("attn_far_reuse_t_lo", T_LO),
                                       kw.pop("attn_far_reuse_t_hi", T_HI))
    return dict(attn_far_reuse=every, attn_far_reuse_t_lo=t_lo, attn_far_reuse_t_hi=t_hi)


def pipeline_switches(kw, others=(), **named):
    """A pipeline's from_pretrained: switches_from(kw), and -- before anything is loaded -- the refusals of check_composition and
    of a missing window against the loader's other keywords (`named`: attn_window, attn_window_recall, ...; `others`: the dict
    of the attn_reuse / cfg_reuse switches)."""
    from types import SimpleNamespace
    far = switches_from(kw)
    if far["attn_far_reuse"]:
        check_composition(SimpleNamespace(**dict(dict(others), **named, **far)))
        if not int(named.get("attn_window", 0) or 0) > 0:
            raise ValueError("attn_far_reuse=%d with attn_window=0: the far field is what lies outside the frame window; set "
                             "attn_window > 0 (or attn_far_reuse = 0)" % far["attn_far_reuse"])
    return far


def apply_switches(transformer, switches):
    """Set a freshly loaded transformer's three attributes (a transformer instance that was passed in is left alone, like fp8=)."""
    for name, value in switches.items():
        setattr(transformer, name, value)


def check_composition(transformer, cfg_split=None):
    """ValueError, naming both switches, for everything the far-field reuse does not compose with.  attn_window == 0 is looked at
    by the forward (a sampler's dense step runs with the window switched off)."""
    n = transformer.attn_far_reuse
    for name, off in (("attn_window_recall", 0.0), ("attn_window_balance", False), ("attn_window_widths", None), ("attn_band", 0),
                      ("fp8_attention", False), ("step_cache", 0.0), ("attn_reuse", 0), ("cfg_reuse", 0)):
        value = getattr(transformer, name, off)
        if value is not None and value:
            raise ValueError("attn_far_reuse=%d with %s=%r: the far-field reuse runs the shared frame window of every head in bf16 "
                             "and keys its entries by the passes of every forward; run one of the two" % (n, name, value))
    if cfg_split is not None:   # refused, not dropped: the two ranks of a CFG pair would each hold a part of the keys
        raise ValueError("attn_far_reuse=%d with cfg_split: the cache is keyed by the passes of ONE rank's forward; run one of the two" % n)


class AttnFar(AttnReuse):
    """The far-field cache of ONE transformer: AttnReuse's rule and record; an entry is the far partial of every layer, output and
    LSE, and the near LSE of the running forward has one scratch."""

    def __init__(self):
        super().__init__()
        self.lse_near = None             # fp32 [samples * heads * rows], allocated once (grows)
        self.tables = {}                 # id(window table) -> (window table, near, far)

    @property
    def bytes(self):
        """Device bytes of the cache entries: layers x keys x (rows x D x 2 + heads x rows x 4)."""
        return sum(t.numel() * t.element_size() for e in self.entries.values() for t in e)

    def buffers(self, keys, layers, rows, D, heads, samples, device):
        """The entries (o [layers, rows, D] bf16, lse [layers, heads, rows] fp32) of `keys`, allocated on first use; another shape
        drops everything cached."""
        if self._shape != (layers, rows, D, heads):
            self._shape = (layers, rows, D, heads)
            self.entries, self._age = {}, {}
        for k in keys:
            if k not in self.entries:
                need = layers * (rows * D * 2 + heads * rows * 4)
                try:
                    self.entries[k] = (torch.empty(layers, rows, D, dtype=BF, device=device),
                                       torch.empty(layers, heads, rows, dtype=torch.float32, device=device))
                except torch.cuda.OutOfMemoryError:
                    raise _lib.AlgHipError("attn_far_reuse: the cache entry of key %r needs %d bytes (layers %d x (rows %d x D %d x 2 "
                                           "+ heads %d x rows %d x 4)) next to the %d bytes of the %d entries held, and the device "
                                           "has no room for it" % (k, need, layers, rows, D, heads, rows, self.bytes,
                                                                   len(self.entries))) from None
        n = samples * heads * rows
        if self.lse_near is None or self.lse_near.numel() < n or self.lse_near.device != torch.device(device):
            self.lse_near = torch.empty(n, dtype=torch.float32, device=device)
        return [self.entries[k] for k in keys]

    def invalidate(self, keys):
        for k in keys:
            self._age.pop(k, None)

    def near_far(self, window_table, device):
        """(near, far) of a window table -- grid_aligned and its complement_ranges, device-resident, built once per table (before
        any capture that replays them)."""
        hit = self.tables.get(id(window_table))
        if hit is None or hit[0] is not window_table:
            near = grid_aligned(window_table)
            far = complement_ranges(near)
            near.on(device)
            far.on(device)
            hit = self.tables[id(window_table)] = (window_table, near, far)
        return hit[1], hit[2]


class AttnFarPass:
    """One active forward: what the rule decided, the tables of every launch group and the launches of a layer."""

    def __init__(self, state, keys, reuse, entries, tables):
        self.state, self.keys, self.reuse, self.entries, self.tables = state, keys, reuse, entries, tables

    def attention(self, timed, name, ops, layer, group=0, sample0=0):
        """The self-attention of `ops` (a SelfAttnOperands; its samples are sample0 .. sample0 + ops.batch - 1 of the forward) for
        layer `layer` into ops.o: the near launch under `name`, on a refresh forward the far launches under "attn_far", the
        merges under "attn_merge"."""
        near, far = self.tables[group]
        st, hd, heads, Sq = self.state, ops.head_dim, ops.heads, ops.Sq
        row = heads * hd
        entry = getattr(_lib, "flash_attn_d%d_ranges_heads" % hd)
        a, offs = ops.args()
        timed(name, entry, *a, near, lse=st.lse_near, **offs, lse_off=sample0 * heads * Sq)
        for n in range(ops.batch):
            e_o, e_lse = self.entries[sample0 + n]
            if not self.reuse:   # sample n alone, its output rows and LSE straight into its entry
                one = dict(o=e_o[layer], batch=1, o_bs=Sq * row, o_rs=row, o_off=0, q_off=ops.q_off + n * ops.q_bs,
                           k_off=ops.k_off + n * ops.k_bs)
                if hd == 64:     # (the d = 64 wrappers take no vt_off)
                    one["vt"] = ops.vt.view(-1)[n * ops.vt_bs:]
                else:
                    one["vt_off"] = ops.vt_off + n * ops.vt_bs
                fa, foffs = SelfAttnOperands(*ops._replace(**one)).args()
                timed("attn_far", entry, *fa, far, lse=e_lse, **foffs, lse_off=layer * heads * Sq)
            timed("attn_merge", _lib.attn_merge_lse, ops.o, st.lse_near, e_o, e_lse, 1, heads, hd, Sq, ops.o_bs, ops.o_rs, Sq * row, row,
                  o_off=ops.o_off + n * ops.o_bs, lse_off=(sample0 + n) * heads * Sq, far_off=layer * Sq * row,
                  lse_far_off=layer * heads * Sq)
        return ops.o

    def finish(self):
        """End of the forward: a refresh forward puts its keys back into use."""
        if not self.reuse:
            self.state.mark_written(self.keys)


class AttnFarHost:
    """What a transformer with the far-field reuse carries: the switches, the record, the reset.  `attn_far_reuse` = 0 is off:
    such a forward runs the launches of a model without this class, allocates nothing and records nothing."""

    attn_far_reuse = 0                # N: the far field is refreshed on every N-th step inside the range; 0 = off, 1 is refused
    attn_far_reuse_t_lo = T_LO        # a step reuses only while t_lo < t < t_hi (plain ints: bench.py --set coerces them)
    attn_far_reuse_t_hi = T_HI
    _attn_far_obj = None
    _attn_dense_step = False          # set around one forward by attn_window.call_transformer(dense=True)

    def _attn_far_state(self):
        if self._attn_far_obj is None:
            self._attn_far_obj = AttnFar()
        return self._attn_far_obj

    @property
    def attn_far_reuse_stats(self):
        """One record per active forward since the last reset: {"keys", "t", "reused", "forced"}."""
        return self._attn_far_state().stats

    @property
    def attn_far_reuse_bytes(self):
        """Device bytes the cache holds: layers x keys x (rows x D x 2 + heads x rows x 4) (0 before the first active forward)."""
        return 0 if self._attn_far_obj is None else self._attn_far_obj.bytes

    def reset_attn_far_reuse(self):
        """Invalidate every key (a new video); the buffers are kept."""
        self._attn_far_state().reset()

    def attn_far_reuse_advance(self):
        """One sampler step has passed (the pipelines call it once per step, in front of the step's forward)."""
        self._attn_far_state().advance()

    def _attn_far_begin(self, cache_keys, cache_force, windows, samples, layers, heads, head_dim, rows):
        """The AttnFarPass of this forward -- or None: off, a forward that names no keys, a dense step, a window that covers the
        video (then the launches are what they are without the switch).  windows: the attn_window table of every launch group."""
        if not self.attn_far_reuse:
            return None
        every, t_lo, t_hi = check_switches(self.attn_far_reuse, self.attn_far_reuse_t_lo, self.attn_far_reuse_t_hi)
        check_composition(self)
        dense = bool(self._attn_dense_step)
        if not dense and not int(getattr(self, "attn_window", 0)) > 0:
            raise ValueError("attn_far_reuse=%d with attn_window=0: the far field is what lies outside the frame window; set "
                             "attn_window > 0 (or attn_far_reuse = 0)" % every)
        if cache_keys is None:
            return None
        keys = list(cache_keys)
        t = getattr(cache_keys, "timestep", None)
        if t is None:
            raise ValueError("attn_far_reuse: cache_keys must carry the sampler step's timestep as a host number -- pass "
                             "attn_far.step_keys(n_pass, batch, timestep) or attn_far.StepKeys(keys, timestep)")
        if len(keys) != samples or len(set(keys)) != len(keys):
            raise ValueError("attn_far_reuse: cache_keys must name each of the %d samples once, got %r" % (samples, keys))
        st = self._attn_far_state()
        st.every, st.t_lo, st.t_hi = every, t_lo, t_hi
        if dense or any(w is None for w in windows):   # dense launches: nothing is cached, what was cached is a step behind
            st.invalidate(keys)
            return None
        tables = [st.near_far(w, self.device) for w in windows]
        entries = st.buffers(keys, layers, rows, heads * head_dim, heads, samples, self.device)   # (another shape invalidates)
        reuse = st.decide(keys, t, bool(cache_force))
        return AttnFarPass(st, keys, reuse, entries, tables)


def active(transformer):
    """True when the pipeline has to drive the far-field reuse of this transformer (stand-ins without the attribute: never)."""
    n = getattr(transformer, "attn_far_reuse", 0)
    return isinstance(n, int) and not isinstance(n, bool) and n != 0


def begin_video(transformer, cfg_split=None):
    """What a pipeline does at the start of a video: False when the switch is off, else the refusals, the reset, True."""
    if not active(transformer):
        return False
    check_switches(transformer.attn_far_reuse, transformer.attn_far_reuse_t_lo, transformer.attn_far_reuse_t_hi)
    check_composition(transformer, cfg_split)
    if not int(getattr(transformer, "attn_window", 0)) > 0:
        raise ValueError("attn_far_reuse=%d with attn_window=0: the far field is what lies outside the frame window; set "
                         "attn_window > 0 (or attn_far_reuse = 0)" % transformer.attn_far_reuse)
    transformer.reset_attn_far_reuse()
    return True
