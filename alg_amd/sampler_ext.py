"""The samplers' side of the transformers' opt-in extensions -- frame window, per-head windows by recall (balance, widths, band),
step cache, attention reuse, far-field reuse, pooled far field, CFG reuse -- written once for the three ALG loops.  Plain host code: nothing here launches anything.

    from_pretrained   `window_switches` validates the keywords before anything is loaded, `apply_switches` sets what was given
    start of a video  `SamplerExtensions(transformer, n_steps, ...)` refuses what does not compose and empties the caches
    every step        `ext.cfg_plan(i, t, n_pass)` says whether the step drops its unconditional pass and which form its combine
                      takes (alg_amd/cfg_reuse.py); `ext.step(i, t, n_pass, batch)` is the callable the loop uses for the
                      step's forwards, with the passes that are actually run

What is refused with what, and which forwards are forced: DESIGN.md ("Sampler extensions")."""
from __future__ import annotations

import functools
from types import SimpleNamespace

from . import _lib, attn_far, attn_pool, attn_reuse, cfg_reuse
from . import step_cache as _step_cache
from .attn_window import HeadWindowHost, _balance_policy, _widths_tuple, calibration_step, call_transformer


def window_switches(attn_window, attn_window_recall, attn_window_balance, attn_window_widths, attn_band=0, fp8_attention=False,
                    *, step_cache=0.0, widths_built=True, recall_needs_window=False):
    """from_pretrained's window keywords (and `step_cache`, which has no rule of its own) -> {attribute: value} of those that
    were given, widths as a tuple; ValueError where two do not compose.  widths_built=False, recall_needs_window=True: CogVideoX."""
    if attn_window_widths is not None and not widths_built:
        raise ValueError("attn_window_widths=%r: the per-head window width (one-pass calibration) is not built for head_dim 64"
                         % (attn_window_widths,))
    if recall_needs_window and attn_window_recall and not int(attn_window) > 0:
        raise ValueError("attn_window_recall=%r needs attn_window > 0: the recall is that of a frame window" % (attn_window_recall,))
    _balance_policy(attn_window_balance)
    if attn_window_balance and not attn_window_recall:
        raise ValueError("attn_window_balance=%r needs attn_window_recall > 0: it orders the launches of layers with dense and "
                         "windowed heads" % (attn_window_balance,))
    if attn_window_widths is not None:
        attn_window_widths = _widths_tuple(attn_window_widths, "attn_window_widths")
        if attn_window_widths[-1] != int(attn_window):
            raise ValueError("attn_window_widths %r: the last (largest) width must equal attn_window = %d"
                             % (attn_window_widths, int(attn_window)))
        if not float(attn_window_recall) > 0.0:
            raise ValueError("attn_window_widths=%r needs attn_window_recall > 0: the width of a head is the narrowest that "
                             "reaches the recall" % (attn_window_widths,))
    if attn_band:   # (the transformer's own check, before anything is loaded)
        HeadWindowHost._head_window_band(SimpleNamespace(attn_band=attn_band, attn_window=attn_window,
                                                         attn_window_recall=attn_window_recall,
                                                         attn_window_widths=attn_window_widths))
        if fp8_attention:
            raise ValueError("attn_band=%d does not compose with fp8_attention: the e4m3 attention kernel takes no key ranges"
                             % attn_band)
    given = {}
    for name, value, cast in (("attn_band", attn_band, int), ("step_cache", step_cache, float), ("attn_window", attn_window, int),
                              ("attn_window_recall", attn_window_recall, float), ("attn_window_balance", attn_window_balance, None)):
        if value:
            given[name] = value if cast is None else cast(value)
    if attn_window_widths is not None:
        given["attn_window_widths"] = attn_window_widths
    return given


def apply_switches(transformer, switches):
    """Set what `window_switches` returned -- also on a transformer instance that was passed in; with every switch off nothing is
    touched (a stand-in need not take attributes)."""
    for name, value in switches.items():
        setattr(transformer, name, value)


class SamplerExtensions:
    """One video's drive of a transformer's step cache, attention reuse, CFG reuse and per-head windows.  A transformer without
    the attributes (the loops' stand-ins) arms nothing and is called as ever."""

    def __init__(self, transformer, n_steps, dense_steps=0, cfg_split=None, forward=None, host_timestep=float, do_cfg=True):
        """forward: a bound method of the transformer to call in its place (CogVideoX: forward_assembled); host_timestep: the
        step's timestep as a host number, taken only while a reuse is on (a device tensor costs a round trip); do_cfg: whether
        the call runs classifier-free guidance at all (the CFG reuse refuses a call that does not)."""
        self.transformer, self.last, self.dense_steps = transformer, n_steps - 1, dense_steps
        self.forward, self.host_timestep = forward, host_timestep
        # step cache (alg_amd/step_cache.py): a new video starts from an empty cache, the last step is always computed
        self.cache = _step_cache.active(transformer)
        if self.cache:
            if cfg_split is not None:
                raise _lib.AlgHipError("step_cache > 0 with cfg_split: the two ranks of a CFG pair would each decide on their own "
                                       "passes and leave the single-GPU result; run one of the two")
            transformer.reset_step_cache()
        # attention reuse (alg_amd/attn_reuse.py): an empty cache too, the first and the last step are always computed
        self.reuse = attn_reuse.begin_video(transformer, cfg_split)
        # far-field reuse (alg_amd/attn_far.py): the same drive -- refusals, an empty cache, the first and the last step refresh
        self.far = attn_far.begin_video(transformer, cfg_split)
        # pooled far field (alg_amd/attn_pool.py): the refusals only -- no state crosses a step, nothing to drive
        attn_pool.begin_video(transformer)
        # CFG reuse (alg_amd/cfg_reuse.py): the video's CfgReuse -- no valid delta, an empty record -- or None: off
        self.cfg = cfg_reuse.begin_video(transformer, cfg_split, do_cfg)
        # per-head windows chosen by recall: every video is calibrated anew, on its last dense step
        self.recall = bool(getattr(transformer, "attn_window", 0)) and getattr(transformer, "attn_window_recall", 0.0) > 0.0
        if self.recall:
            if cfg_split is not None:
                raise _lib.AlgHipError("attn_window_recall > 0 with cfg_split: the two ranks of a CFG pair would decide the windowed "
                                       "heads on different passes; run one of the two")
            transformer.reset_attn_window_heads()

    def cfg_plan(self, i, t, n_pass, force=False):
        """The CfgPlan of step `i` (timestep `t`), whose forward would run `n_pass` passes, asked for in front of the forward.
        plan.reuse: run the conditional pass alone; plan.mode: None -- the plain combine --, cfg_reuse.STORE or cfg_reuse.REUSE
        with plan.delta(shape, dtype, device) as the delta buffer; plan.finish() behind the combine.  Forced (computed whatever
        the schedule says): the last step, the calibration forward of attn_window_recall (its per-sample recall rule needs
        every pass), and what the caller passes as `force`.  With the switch off: cfg_reuse.PLAIN, and nothing else happens."""
        if self.cfg is None:
            return cfg_reuse.PLAIN
        st = self.cfg
        st.advance()
        force = bool(force) or i == self.last or (self.recall and i == calibration_step(self.dense_steps))
        had = st.valid
        if st.decide(n_pass, self.host_timestep(t), force, step=i):
            return cfg_reuse.CfgPlan(st, cfg_reuse.REUSE)
        if n_pass != 2:
            return cfg_reuse.PLAIN
        measure = bool(getattr(self.transformer, "cfg_reuse_drift", False)) and had
        if measure and _lib._capturing():
            raise _lib.AlgHipError("cfg_reuse_drift: a step that measures the drift cannot be captured into a graph -- its sums are "
                                   "read on the host at the end of the step; set cfg_reuse_drift = False under capture")
        return cfg_reuse.CfgPlan(st, cfg_reuse.STORE, measure)

    def cfg_invalidate(self):
        """A callback replaced the latents or a prompt embedding: the delta no longer describes the next step."""
        if self.cfg is not None:
            self.cfg.invalidate()

    def step(self, i, t, n_pass, batch):
        """The callable for the forwards of step `i` (timestep `t`, a CFG batch of n_pass x batch samples): call_transformer with
        the step's dense / calibrate flags and, while a cache is on, the roles of the passes and whether the step is forced."""
        kw = {}
        if self.cache:
            kw = dict(cache_keys=_step_cache.pass_keys(n_pass, batch), cache_force=i == self.last)
        if self.reuse:
            self.transformer.attn_reuse_advance()
            kw = dict(cache_keys=attn_reuse.step_keys(n_pass, batch, self.host_timestep(t)),
                      cache_force=i == self.last or not self.transformer.attn_reuse_stats)
        if self.far:
            self.transformer.attn_far_reuse_advance()
            kw = dict(cache_keys=attn_far.step_keys(n_pass, batch, self.host_timestep(t)),
                      cache_force=i == self.last or not self.transformer.attn_far_reuse_stats)
        return functools.partial(call_transformer, self.transformer, i < self.dense_steps, forward=self.forward,
                                 calibrate=self.recall and i == calibration_step(self.dense_steps), **kw)
