"""Opt-in CFG residual reuse across sampler steps (the "CFG-Cache" half of FasterCache, Lv et al., ICLR 2025, with one N and no
frequency split) for the three ALG samplers -- an extension, the reference has none.

In the middle of the schedule the difference of the two predictions of a two-pass CFG step, delta = cond - uncond, moves little
from step to step, so the unconditional pass is computed on every N-th step and rebuilt from the cached delta on the steps
between.  The decision comes from the SCHEDULE, not from the data: no calibration, no host round trip, and a computed step is
bit for bit the step of a sampler without the switch.

    computed two-pass step   the forward runs both passes; the loop's combine runs in its STORE form, which leaves the bits of
                             the plain combine and writes delta next to them (alg_cfg_ddim_step_delta / alg_cfg_combine_delta)
    reused step              the forward runs the conditional pass ALONE (one sample in place of two); the combine runs in its
                             REUSE form: uncond' = cond - delta, then the plain arithmetic on (uncond', cond) with THIS step's
                             guidance scale

One decision per sampler step, over all videos of a call; the delta is [B, ...] in the dtype the loop combines in.  A step with
any other pass count invalidates the delta: in a three-pass ALG step "uncond" and "cond" see the low-passed condition, which is
another regime, and a one-pass step has no CFG.

`CfgReuse.decide` / `advance` and the bookkeeping around them are plain host code (tests/test_cfg_reuse_cpu.py); everything that
touches the GPU is a launch of libalg_hip.so.  The samplers drive it through alg_amd/sampler_ext.py.

Not built: FasterCache's frequency-split weighting of the delta (low and high frequencies scaled apart), and a data-dependent
decision (the drift below is a diagnostic, the rule does not read it).
"""
from __future__ import annotations

import torch

from . import _lib
from .attn_reuse import parse_timesteps  # noqa: F401  (run.py's --cfg_reuse_timesteps LO,HI reads like --attn_reuse_timesteps)

T_LO, T_HI = 100, 800       # attn_reuse's defaults, this build's choice: reuse only while t_lo < t < t_hi
STORE, REUSE = _lib.CFG_DELTA_STORE, _lib.CFG_DELTA_REUSE


def check_switches(every, t_lo=T_LO, t_hi=T_HI):
    """(every, t_lo, t_hi) as ints; every: 0 = off, 1 is refused (it would reuse nothing), N >= 2; t_lo < t_hi."""
    if isinstance(every, bool) or not isinstance(every, (int, float)) or int(every) != every:
        raise ValueError("cfg_reuse=%r: an int -- 0 = off, N >= 2 computes the unconditional pass on every N-th step" % (every,))
    every, t_lo, t_hi = int(every), int(t_lo), int(t_hi)
    if every < 0 or every == 1:
        raise ValueError("cfg_reuse=%d: 0 = off, N >= 2 computes the unconditional pass on every N-th step (1 would reuse nothing)"
                         % every)
    if t_lo >= t_hi:
        raise ValueError("cfg_reuse_t_lo=%d >= cfg_reuse_t_hi=%d: a step reuses only while t_lo < t < t_hi" % (t_lo, t_hi))
    return every, t_lo, t_hi


def switches_from(kw):
    """from_pretrained's three keywords taken out of its trailing keywords `kw` (the named ones are pinned): a dict with the
    defaults filled in, validated."""
    every, t_lo, t_hi = check_switches(kw.pop("cfg_reuse", 0), kw.pop("cfg_reuse_t_lo", T_LO), kw.pop("cfg_reuse_t_hi", T_HI))
    return dict(cfg_reuse=every, cfg_reuse_t_lo=t_lo, cfg_reuse_t_hi=t_hi)


def apply_switches(transformer, switches):
    """Set a freshly loaded transformer's three attributes (a transformer instance that was passed in is left alone, like fp8=)."""
    for name, value in switches.items():
        setattr(transformer, name, value)


class CfgReuse:
    """The CFG delta of ONE video: the rule, its record, and (from the first armed two-pass step on) the buffers."""

    def __init__(self, every=0, t_lo=T_LO, t_hi=T_HI):
        self.every, self.t_lo, self.t_hi = check_switches(every, t_lo, t_hi)
        self.stats = []                  # one record per armed step
        self._age = None                 # sampler steps since the delta was written; None = no valid delta
        self._step = -1                  # sampler steps since the last reset, minus one
        # device state: nothing is allocated before the first armed two-pass step
        self._shape = None               # (shape, dtype) of the delta
        self._bufs = []                  # one delta, two with the drift diagnostic (written in turn)
        self._cur = 0                    # the buffer that holds the valid delta
        self._drift = self._drift_host = self._work = None

    # ---- the rule (no GPU) -------------------------------------------------------------------------------------------
    def reset(self):
        """A new video: no valid delta, an empty record (the buffers stay)."""
        self._age, self._step = None, -1
        del self.stats[:]

    def advance(self):
        """One sampler step has passed: a valid delta is a step older."""
        self._step += 1
        if self._age is not None:
            self._age += 1

    @property
    def valid(self):
        return self._age is not None

    def invalidate(self):
        """The delta no longer describes the next step (a callback replaced the latents or a prompt embedding)."""
        self._age = None

    def decide(self, n_pass, t, force=False, step=None):
        """One decision for the sampler step whose forward would run `n_pass` passes at timestep `t`.  Reuse iff every >= 2,
        n_pass == 2, `force` is false, t_lo < t < t_hi (both exclusive) and the delta is valid with age 1 .. every - 1.
        Otherwise the step computes: a two-pass step is about to rewrite the delta, which stays out of use until `mark_written`
        puts it back with age 0; any other pass count invalidates it.  Appends the record to `stats`."""
        reuse = (self.every >= 2 and n_pass == 2 and not force and self.t_lo < t < self.t_hi
                 and self._age is not None and 1 <= self._age <= self.every - 1)
        if not reuse:
            self._age = None
        self.stats.append({"step": self._step if step is None else step, "t": t, "n_pass": n_pass, "reused": reuse,
                           "forced": bool(force)})
        return reuse

    def mark_written(self):
        """After a computed two-pass step: the delta is current."""
        self._age = 0

    # ---- the buffers -------------------------------------------------------------------------------------------------
    @property
    def bytes(self):
        """Device bytes of the delta (and, with the diagnostic, of its second copy)."""
        return sum(t.numel() * t.element_size() for t in self._bufs)

    def buffers(self, shape, dtype, device, copies):
        """`copies` delta buffers of this shape and dtype, allocated on first use; another shape or dtype drops what is cached."""
        key = (tuple(shape), dtype)
        if self._shape != key:
            self._shape, self._bufs, self._cur, self._age = key, [], 0, None
        while len(self._bufs) < copies:
            try:
                self._bufs.append(torch.empty(key[0], dtype=dtype, device=device))
            except torch.cuda.OutOfMemoryError:
                raise _lib.AlgHipError("cfg_reuse: the delta of shape %r needs %d bytes and the device has no room for it"
                                       % (key[0], torch.empty(key[0], dtype=dtype, device="meta").nbytes)) from None
        return self._bufs

    def drift_buffers(self, numel, device):
        """Two device doubles (and their pinned host copy) and the workspace of one alg_cfg_delta_drift launch."""
        need = _lib.cfg_delta_drift_workspace_bytes(numel)
        if self._drift is None or self._work.numel() < need:
            self._drift = torch.zeros(2, dtype=torch.float64, device=device)
            self._drift_host = torch.zeros(2, dtype=torch.float64).pin_memory()
            self._work = torch.empty(need, dtype=torch.uint8, device=device)
        return self._drift


class CfgPlan:
    """What the loop does with one step's CFG: `reuse` -- drop the unconditional pass; `mode` -- None (the plain combine), STORE
    or REUSE (the combine's delta form, with `delta(...)` as its buffer); `finish()` behind the combine."""

    reuse, mode = False, None

    def __init__(self, state=None, mode=None, measure=False):
        self.state, self.mode, self.measure = state, mode, measure
        self.reuse = mode == REUSE
        self._new = None

    def delta(self, shape, dtype, device):
        """The delta buffer this step's combine writes (STORE) or reads (REUSE)."""
        st = self.state
        had = st._shape == (tuple(shape), dtype) and len(st._bufs) > 0
        if self.mode == REUSE and not had:
            raise _lib.AlgHipError("cfg_reuse: the step reuses a delta of shape %r, and the one held has %r"
                                   % (tuple(shape), st._shape))
        bufs = st.buffers(shape, dtype, device, 2 if self.measure or len(st._bufs) == 2 else 1)
        if self.mode == REUSE:
            return bufs[st._cur]
        self.measure = self.measure and had
        self._new = (st._cur + 1) % len(bufs) if self.measure else st._cur   # with the diagnostic the cached copy is kept for the sums
        return bufs[self._new]

    def finish(self):
        """Behind the combine.  A STORE step puts the delta back into use with age 0; with the drift diagnostic over a valid
        delta, sum |new - cached| / sum |cached| comes to the host first (one launch pair, one copy, one stream synchronisation)
        and joins the step's record."""
        if self.mode != STORE:
            return
        st = self.state
        if self._new is None:
            raise _lib.AlgHipError("cfg_reuse: a computed two-pass step of an armed video must run the combine's STORE form")
        if self.measure:
            new, old = st._bufs[self._new], st._bufs[st._cur]
            sums = st.drift_buffers(new.numel(), new.device)
            _lib.cfg_delta_drift(new, old, st._work, sums)
            st._drift_host.copy_(sums, non_blocking=True)
            torch.cuda.current_stream(new.device).synchronize()
            a, b = st._drift_host.tolist()
            st.stats[-1]["drift"] = a / b if b > 0.0 else float("inf") if a == a else float("nan")
        st._cur = self._new
        st.mark_written()


PLAIN = CfgPlan()        # the step of a sampler without the switch (and every step that is no two-pass step): nothing differs


class CfgReuseHost:
    """What a transformer carries for the samplers' CFG reuse: the switches (attributes, so that `--set cfg_reuse=2` reaches
    them), the record, the reset.  The transformer's forward never reads them -- the loop drops a pass and changes its combine.
    `cfg_reuse` = 0 is off: such a sampler allocates nothing, records nothing and launches what it launched without this class."""

    cfg_reuse = 0                     # N: the unconditional pass is computed on every N-th step inside the range; 0 = off, 1 is refused
    cfg_reuse_t_lo = T_LO             # a step reuses only while t_lo < t < t_hi (plain ints: bench.py --set coerces them)
    cfg_reuse_t_hi = T_HI
    cfg_reuse_drift = False           # the diagnostic: a computed two-pass step over a valid delta records sum |new - cached| / sum |cached|
    _cfg_reuse_obj = None

    def _cfg_reuse_state(self):
        if self._cfg_reuse_obj is None:
            self._cfg_reuse_obj = CfgReuse()
        return self._cfg_reuse_obj

    @property
    def cfg_reuse_stats(self):
        """One record per armed step since the last reset: {"step", "t", "n_pass", "reused", "forced"} (+ "drift")."""
        return self._cfg_reuse_state().stats

    @property
    def cfg_reuse_bytes(self):
        """Device bytes the delta holds (0 before the first armed two-pass step)."""
        return 0 if self._cfg_reuse_obj is None else self._cfg_reuse_obj.bytes

    def reset_cfg_reuse(self):
        """Invalidate the delta and empty the record (a new video); the buffers are kept."""
        self._cfg_reuse_state().reset()


def active(transformer):
    """True when the sampler has to drive the CFG reuse for this transformer (stand-ins without the attribute: never)."""
    n = getattr(transformer, "cfg_reuse", 0)
    return not (isinstance(n, int) and not isinstance(n, bool) and n == 0)


def begin_video(transformer, cfg_split=None, do_cfg=True):
    """What a sampler does at the start of a video: None when the switch is off, else the refusals, the reset, the video's
    CfgReuse with the switches of this moment."""
    if not active(transformer):
        if getattr(transformer, "cfg_reuse_drift", False):
            raise ValueError("cfg_reuse_drift needs cfg_reuse >= 2: it measures the delta the reuse would read")
        return None
    every, t_lo, t_hi = check_switches(transformer.cfg_reuse, getattr(transformer, "cfg_reuse_t_lo", T_LO),
                                       getattr(transformer, "cfg_reuse_t_hi", T_HI))
    if cfg_split is not None:   # refused, not dropped: the two ranks of a CFG pair would each hold half of the delta
        raise ValueError("cfg_reuse=%d with cfg_split: a reused step has one pass and nothing to split; run one of the two" % every)
    if getattr(transformer, "step_cache", 0.0) > 0.0:
        raise ValueError("cfg_reuse=%d with step_cache=%r: the step cache keys its residuals by the passes of every forward; "
                         "run one of the two" % (every, transformer.step_cache))
    if not do_cfg:
        raise ValueError("cfg_reuse=%d in a call without classifier-free guidance (guidance_scale <= 1; HunyuanVideo: "
                         "true_cfg_scale <= 1): the switch could never act" % every)
    state = transformer._cfg_reuse_state() if hasattr(transformer, "_cfg_reuse_state") else CfgReuse()
    state.every, state.t_lo, state.t_hi = every, t_lo, t_hi
    state.reset()
    return state
