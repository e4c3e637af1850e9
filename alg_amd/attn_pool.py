"""Opt-in POOLED far-field attention of the three DiTs: the keys inside the frame window at full resolution, the keys outside it on
every step at 1 / G of their resolution, merged by their log-sum-exps -- an extension, the reference has none.

`attn_window` alone drops every key outside the window (wrong for a head that spreads its softmax mass); `attn_far_reuse` brings
them back stale and from a cache.  This module looks at the far field on EVERY step through pooled keys: every group of G
consecutive far keys (aligned to G on the absolute key index) becomes one key k_g = bf16(mean k) with the value v_g = bf16(mean v)
and a score bias of log2 G, so that it weighs as G keys -- the compressed-token branch of Native Sparse Attention, restricted to
the complement of the frame window.  For a block of queries with the near keys N and the far groups g (scores in the log2 domain):

    o = (sum_{j in N} 2^s_j v_j + sum_g G 2^(q . k_g) v_g) / (sum_{j in N} 2^s_j + sum_g G 2^(q . k_g))

    per layer   POOL    alg_attn_pool_k, alg_attn_pool_vt (attn_pool.hip): this layer's K rows and V^T at 1 / G, under "attn_pool"
                NEAR    alg_flash_attn_d{64,128}_ranges_heads on the near table: O into the attention-output buffer, LSE into a scratch
                FAR     the same entry on the POOLED operands and the pooled table, O and LSE into scratches, under "attn_far"
                MERGE   alg_attn_merge_lse_shift with the far LSE shifted by log2 G, in place, under "attn_merge"

No state crosses a step: no cache, no schedule, no staleness, so the switch composes with everything the shared `attn_window`
composes with (fp8 / fp4 linears, packed weights, LoRA, step_cache, cfg_split, attn_reuse, cfg_reuse).  It is an APPROXIMATION of
the dense attention (docs/numerics.md), off by default; its visual quality on a trained checkpoint is unmeasured (README).

The tables: a pooled key whose originals are also visited at full resolution would be counted twice, so every near / far cut lies
on the 64 G key grid: near = attn_window.grid_aligned(window table, grid=64 G) (ranges widened outward; the keys behind the last
multiple of 64 G, CogVideoX's prompt prefix and HunyuanVideo's prompt tail stay near), far = complement_ranges(near), and the far
launch runs pooled_ranges(far, G), which lies on the kernels' 64-key grid.  A block that sees every key at full resolution
(CogVideoX's block with the prompt rows, HunyuanVideo's prompt rows) has no far range: the far launch writes zeros and an LSE of
-inf there and the merge leaves the near bits.  A dense step (attn_window_dense_steps) and a window that covers the video launch
the dense entry and allocate nothing.

Memory, ONE workspace for all layers (attn_far_pool_bytes), with P = keys // G rounded up to 64, D = heads x head_dim:
    pooled K      samples x P x D x 2            (head_dim 64: x the Q|K buffer's row stride instead of D -- its K shares Q's strides)
    pooled V^T    samples x D x P x 2            (head_dim 64: x the V^T pitch instead of P -- the entry wants it to cover its one S)
    far output    samples x rows x D x 2
    two LSEs      2 x samples x heads x rows x 4
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .attn_window import KV_ALIGN, SelfAttnOperands, _block_ranges, complement_ranges, grid_aligned, pooled_ranges

BF = torch.bfloat16
GROUPS = (2, 4, 8)      # powers of two: the mean is an exact scaling, log2 G an integer


def check_switch(group):
    """attn_far_pool as an int: 0 = off, else G in {2, 4, 8}."""
    if isinstance(group, bool) or not isinstance(group, (int, float)) or int(group) != group:
        raise ValueError("attn_far_pool=%r: an int -- 0 = off, G in %r pools every G far keys into one" % (group, GROUPS))
    group = int(group)
    if group and group not in GROUPS:
        raise ValueError("attn_far_pool=%d: 0 = off, G in %r pools every G far keys into one (powers of two: the mean is an exact "
                         "scaling)" % (group, GROUPS))
    return group


def switches_from(kw):
    """from_pretrained's keyword taken out of its trailing keywords `kw`: a dict with the default filled in, validated."""
    return dict(attn_far_pool=check_switch(kw.pop("attn_far_pool", 0)))


def _no_window(group):
    return ValueError("attn_far_pool=%d with attn_window=0: the far field is what lies outside the frame window; set attn_window > 0 "
                      "(or attn_far_pool = 0)" % group)


def check_composition(transformer):
    """ValueError, naming both switches, for everything the pooled far field does not compose with.  attn_window == 0 is looked at
    by the callers (a sampler's dense step runs with the window switched off)."""
    g = transformer.attn_far_pool
    for name, off in (("attn_far_reuse", 0), ("attn_window_recall", 0.0), ("attn_window_balance", False), ("attn_window_widths", None),
                      ("attn_band", 0), ("fp8_attention", False)):
        value = getattr(transformer, name, off)
        if value is not None and value:
            raise ValueError("attn_far_pool=%d with %s=%r: the pooled far field runs the shared frame window of every head in bf16 "
                             "next to ONE pooled launch; run one of the two" % (g, name, value))


def pipeline_switches(kw, others=(), **named):
    """A pipeline's from_pretrained: switches_from(kw), and -- before anything is loaded -- the refusals of check_composition and
    of a missing window against the loader's other keywords (`named`: attn_window, attn_window_recall, ...; `others`: the dict
    of the switches taken from the trailing keywords so far)."""
    from types import SimpleNamespace
    pool = switches_from(kw)
    if pool["attn_far_pool"]:
        check_composition(SimpleNamespace(**dict(dict(others), **named, **pool)))
        if not int(named.get("attn_window", 0) or 0) > 0:
            raise _no_window(pool["attn_far_pool"])
    return pool


def apply_switches(transformer, switches):
    """Set a freshly loaded transformer's attribute (a transformer instance that was passed in is left alone, like fp8=)."""
    for name, value in switches.items():
        setattr(transformer, name, value)


def near_far_pooled(window_table, group, pooled_skv=None):
    """(near, far, pooled) of a window table: grid_aligned(table, grid=64 G), its complement_ranges, and the far table in pooled
    keys.  near and the expansion of pooled by G visit every key of every block exactly once."""
    near = grid_aligned(window_table, grid=KV_ALIGN * group)
    far = complement_ranges(near)
    return near, far, pooled_ranges(far, group, Skv=pooled_skv)


class AttnPool:
    """The workspace and the tables of ONE transformer."""

    def __init__(self):
        self.k = self.vt = self.o_far = self.lse_near = self.lse_far = None
        self.shape = None
        self.tables = {}                 # (id(window table), G, head_dim) -> (window table, near, pooled or None)

    @property
    def bytes(self):
        return sum(t.numel() * t.element_size() for t in (self.k, self.vt, self.o_far, self.lse_near, self.lse_far) if t is not None)

    def workspace(self, shape, device):
        """Five flat buffers that hold `shape`, allocated on the first active forward and GROW-ONLY: a forward with fewer samples
        or a larger G (cfg_reuse and cfg_split alternate between one and two samples) lays its operands out in what is there, and a
        buffer an earlier capture points to is never freed by a smaller shape.  A buffer that has to grow is never grown inside a
        stream capture."""
        samples, rows, heads, hd, P, k_rs, vt_rs = shape
        D = heads * hd
        need = (("k", samples * P * k_rs, BF), ("vt", samples * D * vt_rs, BF), ("o_far", samples * rows * D, BF),
                ("lse_near", samples * heads * rows, torch.float32), ("lse_far", samples * heads * rows, torch.float32))
        self.shape = shape
        short = [(name, n, dt) for name, n, dt in need
                 if getattr(self, name) is None or getattr(self, name).numel() < n or getattr(self, name).device != device]
        if not short:
            return
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AlgHipError("attn_far_pool: the workspace is allocated on the first active forward; run one eager forward "
                                   "of this shape before capturing")
        for name, n, dt in short:     # (zeros: the rows between a sample's pooled keys and P are never written and never read)
            setattr(self, name, torch.zeros(n, dtype=dt, device=device))

    def near_pooled(self, window_table, group, head_dim, device):
        """(near, pooled) of a window table, device-resident, built once per table (before any capture that replays them);
        pooled is None when no block has a far key."""
        key = (id(window_table), group, head_dim)
        hit = self.tables.get(key)
        if hit is None or hit[0] is not window_table:
            # the d = 64 entries have one S for queries and keys: their pooled table states Sq
            near, far, pooled = near_far_pooled(window_table, group, window_table.Sq if head_dim == 64 else None)
            near.on(device)
            if any(_block_ranges(far)):
                pooled.on(device)
            else:
                pooled = None
            hit = self.tables[key] = (window_table, near, pooled)
        return hit[1], hit[2]


class AttnPoolPass:
    """One active forward: the tables of every launch group and the launches of a layer."""

    def __init__(self, state, group, tables, samples, rows, P):
        self.state, self.group, self.tables = state, group, tables
        self.samples, self.rows, self.P = samples, rows, P      # of the whole forward; P: pooled keys, rounded up to 64

    def attention(self, timed, name, ops, layer, group=0, sample0=0):
        """The self-attention of `ops` (a SelfAttnOperands; its samples are sample0 .. sample0 + ops.batch - 1 of the forward) into
        ops.o: the poolings under "attn_pool", the near launch under `name`, the far launch(es) under "attn_far", the merge under
        "attn_merge".  Nothing depends on `layer`: the workspace is shared by all layers."""
        near, pooled = self.tables[group]
        st, G, hd, heads, Sq, n = self.state, self.group, ops.head_dim, ops.heads, ops.Sq, ops.batch
        row = heads * hd
        entry = getattr(_lib, "flash_attn_d%d_ranges_heads" % hd)
        a, offs = ops.args()
        if pooled is None:    # every block sees every key at full resolution: the near table alone
            timed(name, entry, *a, near, **offs)
            return ops.o
        # the d = 64 entries apply Q's row stride to K and want a V^T pitch that covers their one S: the pooled operands have both
        P = self.P
        k_rs, vt_rs = (ops.q_rs, ops.vt_rs) if hd == 64 else (row, P)
        st.workspace((self.samples, self.rows, heads, hd, P, k_rs, vt_rs), ops.o.device)
        k_bs, vt_bs = P * k_rs, row * vt_rs
        timed("attn_pool", _lib.attn_pool_k, ops.k, st.k, n, heads, hd, ops.Skv, G, ops.k_bs, ops.k_rs, k_bs, k_rs, src_off=ops.k_off,
              dst_off=sample0 * k_bs)
        timed("attn_pool", _lib.attn_pool_vt, ops.vt, st.vt, n, heads, hd, ops.Skv, G, ops.vt_bs, ops.vt_rs, vt_bs, vt_rs,
              src_off=ops.vt_off, dst_off=sample0 * vt_bs)
        lse_off = sample0 * heads * Sq
        timed(name, entry, *a, near, lse=st.lse_near, **offs, lse_off=lse_off)
        far = dict(k=st.k, vt=st.vt, o=st.o_far, Skv=pooled.Skv, k_bs=k_bs, k_rs=k_rs, vt_bs=vt_bs, vt_rs=vt_rs, o_bs=Sq * row, o_rs=row)
        if hd == 64:          # K shares Q's strides and the wrappers take no vt_off / o_off: one launch per sample, on views
            for i in range(n):
                s = sample0 + i
                one = dict(far, batch=1, q_off=ops.q_off + i * ops.q_bs, k_off=s * k_bs, vt=st.vt[s * vt_bs:], o=st.o_far[s * Sq * row:],
                           Skv=Sq, k_bs=ops.q_bs)
                fa, foffs = SelfAttnOperands(*ops._replace(**one)).args()
                timed("attn_far", entry, *fa, pooled, lse=st.lse_far, **foffs, lse_off=s * heads * Sq)
        else:
            fa, foffs = SelfAttnOperands(*ops._replace(**dict(far, k_off=sample0 * k_bs, vt_off=sample0 * vt_bs,
                                                              o_off=sample0 * Sq * row))).args()
            timed("attn_far", entry, *fa, pooled, lse=st.lse_far, **foffs, lse_off=lse_off)
        timed("attn_merge", _lib.attn_merge_lse_shift, ops.o, st.lse_near, st.o_far, st.lse_far, n, heads, hd, Sq, ops.o_bs, ops.o_rs,
              Sq * row, row, float(int(math.log2(G))), o_off=ops.o_off, lse_off=lse_off, far_off=sample0 * Sq * row, lse_far_off=lse_off)
        return ops.o

    def finish(self):
        """End of the forward: nothing is kept."""


class AttnPoolHost:
    """What a transformer with the pooled far field carries: the switch and the workspace.  `attn_far_pool` = 0 is off: such a
    forward runs the launches of a model without this class and allocates nothing."""

    attn_far_pool = 0                 # G: every G far keys are pooled into one; 0 = off (a plain int: bench.py --set coerces it)
    _attn_pool_obj = None

    @property
    def attn_far_pool_bytes(self):
        """Device bytes of the workspace (the module's docstring states the formula; 0 before the first active forward)."""
        return 0 if self._attn_pool_obj is None else self._attn_pool_obj.bytes

    def _attn_pool_begin(self, windows, samples, heads, head_dim, rows):
        """The AttnPoolPass of this forward -- or None: off, a dense step, a window that covers the video (then the launches are
        what they are without the switch).  windows: the attn_window table of every launch group; rows: the query rows of a
        sample, which bound its keys.  The workspace is allocated by the first layer's launches."""
        if not self.attn_far_pool:
            return None
        G = check_switch(self.attn_far_pool)
        check_composition(self)
        dense = bool(getattr(self, "_attn_dense_step", False))
        if not dense and not int(getattr(self, "attn_window", 0)) > 0:
            raise _no_window(G)
        if dense or any(w is None for w in windows):
            return None
        if self._attn_pool_obj is None:
            self._attn_pool_obj = AttnPool()
        st = self._attn_pool_obj
        tables = [st.near_pooled(w, G, head_dim, self.device) for w in windows]
        return AttnPoolPass(st, G, tables, samples, rows, -(-(rows // G) // KV_ALIGN) * KV_ALIGN)


def active(transformer):
    """True when this transformer runs the pooled far field (stand-ins without the attribute: never)."""
    g = getattr(transformer, "attn_far_pool", 0)
    return isinstance(g, int) and not isinstance(g, bool) and g != 0


def begin_video(transformer):
    """What a pipeline does at the start of a video: False when the switch is off, else the refusals, True.  (There is no state
    to reset.)"""
    if not active(transformer):
        return False
    check_switch(transformer.attn_far_pool)
    check_composition(transformer)
    if not int(getattr(transformer, "attn_window", 0)) > 0:
        raise _no_window(transformer.attn_far_pool)
    return True
