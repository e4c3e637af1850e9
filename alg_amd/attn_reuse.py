"""Opt-in attention reuse across sampler steps (Pyramid Attention Broadcast with one N for every layer) of the three DiTs -- an
extension, the reference has none.

In the middle of the schedule a layer's self-attention output moves little from step to step, so a layer computes it on every
N-th step and reads it back on the steps between.  The decision comes from the SCHEDULE, not from the data: no calibration, no
host round trip, and a computed step is bit for bit the step of a model without the switch.

    computed forward   every block runs as ever; behind its self-attention the output rows of each sample are COPIED into that
                       sample's cache entry [layer]  (one read and one write of rows * D bf16 per layer and sample; the attention
                       does not write the cache itself, so that no launch of a computed forward differs from today's)
    reusing forward    a block skips everything whose only consumer is the self-attention (the norm in front of it, Q|K, V^T, the
                       head norms / RoPE, the attention), copies the cached rows into the attention-output buffer and goes on with
                       the output projection -- this step's gate and residual -- and the rest of the block.  to_out is linear and
                       fixed, so to_out(cached attention) is PAB's cached module output, and no GEMM epilogue changes

A sample's entry is keyed by the ROLE of its pass, exactly step_cache.pass_keys ("uncond_init" / "uncond" / "cond", with the
video's index when a call carries several): the ALG loop runs 3 passes per step early and 2 later, and "uncond" / "cond" carry
over.  One decision per forward, over all its rows.

`AttnReuse.decide` / `advance` and the bookkeeping around them are plain host code (tests/test_attn_reuse_cpu.py); everything
that touches the GPU is a copy or a launch of libalg_hip.so (the drift diagnostic: alg_attn_drift).
"""
from __future__ import annotations

import torch

from . import _lib
from .step_cache import pass_keys

BF = torch.bfloat16
T_LO, T_HI = 100, 800       # diffusers' PAB defaults for the spatial attention: reuse only while t_lo < t < t_hi


class StepKeys(list):
    """The cache keys of one forward (a list: the step cache reads it as one) that also carry the sampler step's timestep as a
    HOST number -- the rule needs it, and the transformer's own `timestep` argument lives on the device."""

    def __init__(self, keys, timestep):
        super().__init__(keys)
        self.timestep = float(timestep)


def step_keys(n_pass, batch, timestep):
    """pass_keys(n_pass, batch) of a CFG batch at the sampler step whose timestep is `timestep`."""
    return StepKeys(pass_keys(n_pass, batch), timestep)


def check_switches(every, t_lo=T_LO, t_hi=T_HI):
    """(every, t_lo, t_hi) as ints; every: 0 = off, 1 is refused (it would reuse nothing), N >= 2; t_lo < t_hi."""
    if isinstance(every, bool) or int(every) != every:
        raise ValueError("attn_reuse=%r: an int -- 0 = off, N >= 2 computes the attention on every N-th step" % (every,))
    every, t_lo, t_hi = int(every), int(t_lo), int(t_hi)
    if every < 0 or every == 1:
        raise ValueError("attn_reuse=%d: 0 = off, N >= 2 computes the attention on every N-th step (1 would reuse nothing)" % every)
    if t_lo >= t_hi:
        raise ValueError("attn_reuse_t_lo=%d >= attn_reuse_t_hi=%d: a step reuses only while t_lo < t < t_hi" % (t_lo, t_hi))
    return every, t_lo, t_hi


def switches_from(kw):
    """from_pretrained's three keywords taken out of its trailing keywords `kw` (the named ones are pinned): a dict with the
    defaults filled in, validated."""
    every, t_lo, t_hi = check_switches(kw.pop("attn_reuse", 0), kw.pop("attn_reuse_t_lo", T_LO), kw.pop("attn_reuse_t_hi", T_HI))
    return dict(attn_reuse=every, attn_reuse_t_lo=t_lo, attn_reuse_t_hi=t_hi)


def apply_switches(transformer, switches):
    """Set a freshly loaded transformer's three attributes (a transformer instance that was passed in is left alone, like fp8=)."""
    for name, value in switches.items():
        setattr(transformer, name, value)


def parse_timesteps(text):
    """run.py's --attn_reuse_timesteps LO,HI -> (lo, hi)."""
    try:
        lo, hi = (int(v) for v in str(text).split(","))
    except ValueError:
        raise ValueError("two integers LO,HI such as 100,800, got %r" % (text,))
    return lo, hi


class AttnReuse:
    """The attention cache of ONE transformer: the rule, its record, and (from the first active forward on) the buffers."""

    def __init__(self, every=0, t_lo=T_LO, t_hi=T_HI):
        self.every, self.t_lo, self.t_hi = check_switches(every, t_lo, t_hi)
        self.stats = []                  # one record per active forward
        self._age = {}                   # key -> sampler steps since its entry was written; present = valid
        # device state: nothing is allocated before the first active forward
        self._shape = None               # (layers, rows, D)
        self.entries = {}                # key -> [layers, rows, D] bf16
        self._drift = self._drift_host = self._work = None

    # ---- the rule (no GPU) -------------------------------------------------------------------------------------------
    def reset(self):
        """Forget every key (the buffers stay): the next forward is computed."""
        self._age.clear()
        del self.stats[:]

    def advance(self):
        """One sampler step has passed: every valid entry is a step older."""
        for k in self._age:
            self._age[k] += 1

    def valid(self, keys):
        return all(k in self._age for k in keys)

    def decide(self, keys, t, force=False):
        """One decision for a forward whose samples carry `keys` at timestep `t`.  Reuse iff every >= 2, `force` is false,
        t_lo < t < t_hi (both exclusive) and every key holds a valid entry of age 1 .. every - 1.  Otherwise the forward computes:
        its keys' entries are about to be rewritten and stay out of use until `mark_written` (the forward has finished) puts them
        back with age 0.  A key that is not named is left alone.  Appends the record to `stats`."""
        keys = list(keys)
        reuse = (self.every >= 2 and bool(keys) and not force and self.t_lo < t < self.t_hi
                 and all(1 <= self._age.get(k, 0) <= self.every - 1 for k in keys))
        if not reuse:
            for k in keys:
                self._age.pop(k, None)
        self.stats.append({"keys": keys, "t": t, "reused": reuse, "forced": bool(force)})
        return reuse

    def mark_written(self, keys):
        """After a computed forward: the entries of these keys are current."""
        for k in keys:
            self._age[k] = 0

    # ---- the buffers -------------------------------------------------------------------------------------------------
    @property
    def bytes(self):
        """Device bytes of the cache entries: layers x keys x rows x D x 2."""
        return sum(t.numel() * t.element_size() for t in self.entries.values())

    def buffers(self, keys, layers, rows, D, device):
        """The entries of `keys`, allocated on first use; another shape drops everything cached."""
        if self._shape != (layers, rows, D):
            self._shape = (layers, rows, D)
            self.entries, self._age, self._drift = {}, {}, None
        for k in keys:
            if k not in self.entries:
                need = layers * rows * D * 2
                try:
                    self.entries[k] = torch.empty(layers, rows, D, dtype=BF, device=device)
                except torch.cuda.OutOfMemoryError:
                    raise _lib.AlgHipError("attn_reuse: the cache entry of key %r needs %d bytes (layers %d x rows %d x D %d x 2) "
                                           "next to the %d bytes of the %d entries held, and the device has no room for it"
                                           % (k, need, layers, rows, D, self.bytes, len(self.entries))) from None
        return [self.entries[k] for k in keys]

    def drift_buffers(self, n_keys, layers, rows, D, device):
        """[keys][layers][2] device doubles (and their pinned host copy) for one forward's alg_attn_drift launches."""
        if self._drift is None or self._drift.shape[0] < n_keys:
            self._drift = torch.zeros(n_keys, layers, 2, dtype=torch.float64, device=device)
            self._drift_host = torch.zeros(n_keys, layers, 2, dtype=torch.float64).pin_memory()
            self._work = torch.empty(_lib.attn_drift_workspace_bytes(rows, D), dtype=torch.uint8, device=device)
        return self._drift


class AttnReusePass:
    """One active forward: what the rule decided, and the copies between the blocks' attention output and the cache."""

    def __init__(self, state, keys, reuse, entries, drift):
        self.state, self.keys, self.reuse, self.entries, self.drift = state, keys, reuse, entries, drift

    def load(self, layer, outs):
        """A reusing forward: outs[n] ([rows, D] view of the block's attention-output buffer) <- sample n's cached rows."""
        for o, e in zip(outs, self.entries):
            o.copy_(e[layer])

    def store(self, layer, outs):
        """A computed forward, behind the block's self-attention: sample n's cached rows <- outs[n]; with the drift diagnostic
        sum |new - cached| and sum |cached| are taken first."""
        for n, (o, e) in enumerate(zip(outs, self.entries)):
            if self.drift is not None:
                _lib.attn_drift(o, e[layer], self.state._work, self.drift[n, layer])
            e[layer].copy_(o)

    def finish(self):
        """End of the forward: a computed one puts its keys back into use; with the drift diagnostic the sums come to the host
        (one copy, one stream synchronisation) and the ratios join the forward's record."""
        if self.reuse:
            return
        st = self.state
        st.mark_written(self.keys)
        if self.drift is not None:
            n = len(self.keys)
            st._drift_host[:n].copy_(self.drift[:n], non_blocking=True)
            torch.cuda.current_stream(self.drift.device).synchronize()
            st.stats[-1]["drift"] = [[(a / b if b > 0.0 else float("inf") if a == a else float("nan")) for a, b in per_key]
                                     for per_key in st._drift_host[:n].tolist()]


class AttnReuseHost:
    """What a transformer with attention reuse carries: the switches, the record, the reset.  `attn_reuse` = 0 is off: such a
    forward runs the launches of a model without this class, allocates nothing and records nothing."""

    attn_reuse = 0                    # N: the attention is computed on every N-th step inside the range; 0 = off, 1 is refused
    attn_reuse_t_lo = T_LO            # a step reuses only while t_lo < t < t_hi (plain ints: bench.py --set coerces them)
    attn_reuse_t_hi = T_HI
    attn_reuse_drift = False          # the diagnostic: every computed forward over valid entries records sum |new - cached| / sum |cached|
    _attn_reuse_obj = None

    def _attn_reuse_state(self):
        if self._attn_reuse_obj is None:
            self._attn_reuse_obj = AttnReuse()
        return self._attn_reuse_obj

    @property
    def attn_reuse_stats(self):
        """One record per active forward since the last reset: {"keys", "t", "reused", "forced"} (+ "drift": [[per layer] per key])."""
        return self._attn_reuse_state().stats

    @property
    def attn_reuse_bytes(self):
        """Device bytes the cache holds: layers x keys x rows x D x 2 (0 before the first active forward)."""
        return 0 if self._attn_reuse_obj is None else self._attn_reuse_obj.bytes

    def reset_attn_reuse(self):
        """Invalidate every key (a new video); the buffers are kept."""
        self._attn_reuse_state().reset()

    def attn_reuse_advance(self):
        """One sampler step has passed (the pipelines call it once per step, in front of the step's forward)."""
        self._attn_reuse_state().advance()

    def _attn_reuse_begin(self, cache_keys, cache_force, samples, layers, rows, D):
        """The AttnReusePass of this forward -- or None (off, or a forward that names no keys: nothing happens)."""
        if not self.attn_reuse:
            if self.attn_reuse_drift:
                raise ValueError("attn_reuse_drift needs attn_reuse >= 2: it measures the entries the reuse would read")
            return None
        every, t_lo, t_hi = check_switches(self.attn_reuse, self.attn_reuse_t_lo, self.attn_reuse_t_hi)
        if getattr(self, "step_cache", 0.0) > 0.0:     # refused, not dropped: a skipped tail would leave its layers' entries stale
            raise ValueError("attn_reuse=%d with step_cache=%r: the two caches do not compose; run one of the two"
                             % (every, self.step_cache))
        if cache_keys is None:
            return None
        keys = list(cache_keys)
        t = getattr(cache_keys, "timestep", None)
        if t is None:
            raise ValueError("attn_reuse: cache_keys must carry the sampler step's timestep as a host number -- pass "
                             "attn_reuse.step_keys(n_pass, batch, timestep) or attn_reuse.StepKeys(keys, timestep)")
        if len(keys) != samples or len(set(keys)) != len(keys):
            raise ValueError("attn_reuse: cache_keys must name each of the %d samples once, got %r" % (samples, keys))
        st = self._attn_reuse_state()
        st.every, st.t_lo, st.t_hi = every, t_lo, t_hi
        force = bool(cache_force) or bool(getattr(self, "_attn_calibrate", False))
        measure = bool(self.attn_reuse_drift)
        if measure and _lib._capturing():
            raise _lib.AlgHipError("attn_reuse_drift: a forward that measures the drift cannot be captured into a graph -- its sums "
                                   "are read on the host at the end of the forward; set attn_reuse_drift = False under capture")
        entries = st.buffers(keys, layers, rows, D, self.device)     # (another shape invalidates: before the rule looks)
        had = st.valid(keys)
        reuse = st.decide(keys, t, force)
        drift = st.drift_buffers(len(keys), layers, rows, D, self.device) if measure and had and not reuse else None
        return AttnReusePass(st, keys, reuse, entries, drift)


def active(transformer):
    """True when the pipeline has to drive the attention reuse of this transformer (stand-ins without the attribute: never)."""
    n = getattr(transformer, "attn_reuse", 0)
    return isinstance(n, int) and not isinstance(n, bool) and n != 0


def begin_video(transformer, cfg_split=None):
    """What a pipeline does at the start of a video: False when the switch is off, else the refusals, the reset, True."""
    if not active(transformer):
        return False
    check_switches(transformer.attn_reuse, transformer.attn_reuse_t_lo, transformer.attn_reuse_t_hi)
    if cfg_split is not None:   # refused, not dropped: the two ranks of a CFG pair would each hold a part of the keys
        raise ValueError("attn_reuse=%d with cfg_split: the cache is keyed by the passes of ONE rank's forward; run one of the two"
                         % transformer.attn_reuse)
    if getattr(transformer, "step_cache", 0.0) > 0.0:
        raise ValueError("attn_reuse=%d with step_cache=%r: the two caches do not compose; run one of the two"
                         % (transformer.attn_reuse, transformer.step_cache))
    transformer.reset_attn_reuse()
    return True
