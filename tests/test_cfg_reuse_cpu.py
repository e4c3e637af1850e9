"""CFG residual reuse across steps, host side: the rule of alg_amd.cfg_reuse.CfgReuse as a truth table, the refusals (through
check_switches, through SamplerExtensions on stand-ins, through run.py's argument handling), the switches on the three model
classes, from_pretrained's keywords, run.py's two flags, and the C ABI of the three entries (names, argument refusals before any
launch).  No GPU.

The expected `reused` columns are written out by hand.  Pass pattern 3 3 2 2 2 2 2 2, timesteps 900, 800, ..., 200, a range
(350, 750) that holds steps 2 .. 5 (t = 700 .. 400) only:

    N = 2   steps 0, 1: three passes -- no CFG pair in this regime, the delta is invalid                          F F
            step 2: the first two-pass step, nothing to reuse: computes and writes the delta (age 0)              F
            step 3: age 1 <= N - 1: reuses                                                                        T
            step 4: age 2 > N - 1: computes, age 0                                                                F
            step 5: age 1: reuses                                                                                 T
            step 6: t = 300 is outside the range: computes                                                        F
            step 7: outside the range (and the last step, forced)                                                 F
    N = 3   as above up to step 3 (age 1, T); step 4: age 2 <= N - 1: T; step 5: age 3: computes                  F F F T T F F F
"""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest

import alg_amd
from alg_amd import _lib, cfg_reuse, sampler_ext
from alg_amd.cfg_reuse import CfgReuse, CfgReuseHost
from alg_amd.sampler_ext import SamplerExtensions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alg_cfg_ddim_step_delta", "alg_cfg_combine_delta", "alg_cfg_delta_drift", "alg_cfg_delta_drift_workspace_bytes")
F, T = False, True
PASSES = [3, 3, 2, 2, 2, 2, 2, 2]
TS = [900, 800, 700, 600, 500, 400, 300, 200]
LO, HI = 350, 750


def run_steps(rule, steps):
    """steps: (n_pass, t, force) per sampler step -> the `reused` column (a computed two-pass step writes the delta)"""
    out = []
    for n_pass, t, force in steps:
        rule.advance()
        hit = rule.decide(n_pass, t, force)
        if not hit and n_pass == 2:
            rule.mark_written()
        out.append(hit)
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_the_hand_written_columns_for_n_2_and_n_3():
    steps = [(n, t, i == 7) for i, (n, t) in enumerate(zip(PASSES, TS))]
    r = CfgReuse(2, LO, HI)
    assert run_steps(r, steps) == [F, F, F, T, F, T, F, F]
    assert [s["step"] for s in r.stats] == list(range(8)) and [s["n_pass"] for s in r.stats] == PASSES
    assert r.stats[3] == {"step": 3, "t": 600, "n_pass": 2, "reused": True, "forced": False}
    assert run_steps(CfgReuse(3, LO, HI), steps) == [F, F, F, T, T, F, F, F]
    assert run_steps(CfgReuse(0, LO, HI), steps) == [F] * 8                       # off: never


def test_both_range_edges_are_exclusive():
    for t, want in ((100, F), (101, T), (799, T), (800, F), (99, F), (801, F)):
        assert run_steps(CfgReuse(2, 100, 800), [(2, 500, F), (2, t, F)]) == [F, want], t
    assert run_steps(CfgReuse(2, 0, 1000), [(2, 999.5, F), (2, 0.5, F)]) == [F, T]  # flow timesteps are floats


def test_a_three_pass_step_in_the_middle_invalidates_the_delta():
    # 2 2 3 2 2: step 1 reuses; the three-pass step 2 drops the delta, so step 3 computes although the schedule would reuse
    assert run_steps(CfgReuse(3), [(2, 500, F), (2, 500, F), (3, 500, F), (2, 500, F), (2, 500, F)]) == [F, T, F, F, T]
    # a one-pass step (no CFG) does the same
    assert run_steps(CfgReuse(3), [(2, 500, F), (1, 500, F), (2, 500, F), (2, 500, F)]) == [F, F, F, T]


def test_a_forced_step_computes_and_rewrites():
    r = CfgReuse(2)
    assert run_steps(r, [(2, 500, F), (2, 500, T), (2, 500, F), (2, 500, F)]) == [F, F, T, F]
    assert [s["forced"] for s in r.stats] == [F, T, F, F]


def test_invalidate_after_a_callback_and_the_ages_after_mark_written():
    r = CfgReuse(3)
    assert r._age is None and not r.valid
    r.advance()
    assert r.decide(2, 500) is False and not r.valid          # out of use until the combine has written it
    r.mark_written()
    assert r._age == 0 and r.valid
    r.advance()
    assert r._age == 1 and r.decide(2, 500) is True and r._age == 1            # a reused step leaves the delta and its age
    r.advance()
    assert r._age == 2
    r.invalidate()                                                              # a callback replaced the latents
    assert r._age is None and r.decide(2, 500) is False
    r.mark_written()
    r.advance()
    r.advance()
    r.advance()
    assert r._age == 3 and r.decide(2, 500) is False and r._age is None         # age N: computes
    r.reset()
    assert r.stats == [] and r._age is None and r._step == -1


# ---- refusals: check_switches, SamplerExtensions on stand-ins ------------------------------------------------------------------
def test_check_switches_refusals():
    for bad in (1, -1, 2.5, True, "2", None):
        with pytest.raises(ValueError, match="cfg_reuse"):
            cfg_reuse.check_switches(bad)
    for lo, hi in ((800, 800), (801, 800)):
        with pytest.raises(ValueError, match="cfg_reuse_t_lo"):
            cfg_reuse.check_switches(2, lo, hi)
    assert cfg_reuse.check_switches(0) == (0, 100, 800) and cfg_reuse.check_switches(3, 50, 900) == (3, 50, 900)
    assert (CfgReuse(2).t_lo, CfgReuse(2).t_hi) == (100, 800)


class Dit(CfgReuseHost):
    """A stand-in with the switch attributes and a forward that records the keywords it was handed."""

    def __init__(self, **switches):
        self.step_cache, self.attn_reuse, self.attn_window, self.attn_window_recall = 0.0, 0, 0, 0.0
        self._attn_calibrate = self.attn_window_calibrated = False
        self.calls = []
        vars(self).update(switches)

    def reset_attn_window_heads(self):
        self.attn_window_calibrated = False

    def reset_step_cache(self):
        pass

    def __call__(self, *args, **kw):
        self.calls.append(kw)
        if self._attn_calibrate:
            self.attn_window_calibrated = True
        return "prediction"


def test_sampler_extensions_refuse_what_does_not_compose():
    for bad in (1, 2.5, True):
        with pytest.raises(ValueError, match="cfg_reuse"):
            SamplerExtensions(Dit(cfg_reuse=bad), 4)
    with pytest.raises(ValueError, match="cfg_reuse_t_lo"):
        SamplerExtensions(Dit(cfg_reuse=2, cfg_reuse_t_lo=800, cfg_reuse_t_hi=100), 4)
    with pytest.raises(ValueError, match="cfg_reuse=2 with cfg_split"):
        SamplerExtensions(Dit(cfg_reuse=2), 4, cfg_split=object())
    with pytest.raises(ValueError, match="cfg_reuse=2 with step_cache=0.1"):
        SamplerExtensions(Dit(cfg_reuse=2, step_cache=0.1), 4)
    with pytest.raises(ValueError, match="cfg_reuse=2 in a call without classifier-free guidance"):
        SamplerExtensions(Dit(cfg_reuse=2), 4, do_cfg=False)
    with pytest.raises(ValueError, match="cfg_reuse_drift needs cfg_reuse >= 2"):
        SamplerExtensions(Dit(cfg_reuse_drift=True), 4)
    SamplerExtensions(Dit(), 4, cfg_split=object(), do_cfg=False)               # off: nothing to refuse
    SamplerExtensions(Dit(cfg_reuse=2, attn_reuse=0, attn_window=2), 4)         # composes with a window


def drive(dit, passes, timesteps, dense_steps=0, force=()):
    ext = SamplerExtensions(dit, len(passes), dense_steps)
    plans, run = [], []
    for i, (n, t) in enumerate(zip(passes, timesteps)):
        plan = ext.cfg_plan(i, t, n, force=i in force)
        plans.append(plan)
        n_run = 1 if plan.reuse else n
        run.append(n_run)
        assert ext.step(i, t, n_run, 1)("x") == "prediction"
        if plan.mode == cfg_reuse.STORE:          # (what plan.finish() does behind the combine, without the GPU)
            plan.state.mark_written()
    return ext, plans, run


def test_sampler_extensions_plan_the_steps_and_record_them():
    dit = Dit(cfg_reuse=2, cfg_reuse_t_lo=LO, cfg_reuse_t_hi=HI)
    dit._cfg_reuse_state().stats.append("stale")
    ext, plans, run = drive(dit, PASSES, TS)
    assert ext.cfg is dit._cfg_reuse_obj and (ext.cfg.every, ext.cfg.t_lo, ext.cfg.t_hi) == (2, LO, HI)
    assert [p.reuse for p in plans] == [F, F, F, T, F, T, F, F] and run == [3, 3, 2, 1, 2, 1, 2, 2]
    S, R = cfg_reuse.STORE, cfg_reuse.REUSE
    assert [p.mode for p in plans] == [None, None, S, R, S, R, S, S]            # a three-pass step runs the plain combine
    st = dit.cfg_reuse_stats
    assert [r["reused"] for r in st] == [F, F, F, T, F, T, F, F] and [r["step"] for r in st] == list(range(8))
    assert [r["t"] for r in st] == [float(t) for t in TS] and [r["n_pass"] for r in st] == PASSES
    assert [r["forced"] for r in st] == [F] * 7 + [T]                           # the last step of the schedule
    assert all(sorted(kw) == [] for kw in dit.calls)                            # no cache keyword: the forward is the plain one
    dit.reset_cfg_reuse()
    assert dit.cfg_reuse_stats == []
    # what the caller forces, and the calibration forward of attn_window_recall (step max(dense_steps, 1) - 1 = 3 here)
    dit = Dit(cfg_reuse=2, attn_window=1, attn_window_recall=0.5)
    _, plans, _ = drive(dit, [2] * 8, [500] * 8, dense_steps=4, force=(5,))
    st = dit.cfg_reuse_stats
    assert [r["forced"] for r in st] == [F, F, F, T, F, T, F, T]
    assert [r["reused"] for r in st] == [F, T, F, F, T, F, T, F]


def test_switch_off_and_bare_stand_ins_arm_nothing():
    dit = Dit()
    ext, plans, run = drive(dit, PASSES, TS)
    assert ext.cfg is None and all(p is cfg_reuse.PLAIN for p in plans) and run == PASSES
    assert dit._cfg_reuse_obj is None                                           # nothing allocated, nothing recorded
    assert cfg_reuse.PLAIN.mode is None and cfg_reuse.PLAIN.reuse is False and cfg_reuse.PLAIN.finish() is None
    fn = lambda x: "p"
    ext = SamplerExtensions(fn, 2, do_cfg=False)
    assert ext.cfg_plan(0, 5, 2) is cfg_reuse.PLAIN and ext.cfg_invalidate() is None and vars(fn) == {}
    assert cfg_reuse.active(SimpleNamespace()) is False
    assert list(inspect.signature(SamplerExtensions.step).parameters) == ["self", "i", "t", "n_pass", "batch"]


def test_a_callback_invalidates_through_the_driver():
    dit = Dit(cfg_reuse=3)
    ext = SamplerExtensions(dit, 6)
    for i in range(2):
        plan = ext.cfg_plan(i, 500, 2)
        if plan.mode == cfg_reuse.STORE:
            plan.state.mark_written()
    assert dit.cfg_reuse_stats[1]["reused"] is True
    ext.cfg_invalidate()
    assert ext.cfg_plan(2, 500, 2).reuse is False


# ---- the model classes ---------------------------------------------------------------------------------------------------------
def model_classes():
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    return CogVideoXTransformer3DModel, WanTransformer3DModel, HunyuanVideoTransformer3DModel


def pipelines():
    from alg_amd import CogVideoXImageToVideoPipeline, HunyuanVideoImageToVideoPipeline, WanImageToVideoPipeline
    return CogVideoXImageToVideoPipeline, WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline


def test_the_three_models_carry_the_switches_off():
    for cls in model_classes():
        assert issubclass(cls, CfgReuseHost)
        m = object.__new__(cls)
        assert m.cfg_reuse == 0 and type(m.cfg_reuse) is int
        assert (m.cfg_reuse_t_lo, m.cfg_reuse_t_hi) == (100, 800) and type(m.cfg_reuse_t_lo) is int and type(m.cfg_reuse_t_hi) is int
        assert m.cfg_reuse_drift is False and m.cfg_reuse_bytes == 0 and m._cfg_reuse_obj is None
        assert cfg_reuse.active(m) is False and cfg_reuse.begin_video(m, cfg_split=object(), do_cfg=False) is None
        assert m.cfg_reuse_stats == []
        m.cfg_reuse = 2
        assert cfg_reuse.active(m) is True
        m._cfg_reuse_state().stats.append("stale")
        assert cfg_reuse.begin_video(m) is m._cfg_reuse_obj and m.cfg_reuse_stats == []      # a new video: reset
        with pytest.raises(ValueError, match="cfg_split"):
            cfg_reuse.begin_video(m, cfg_split=object())
        m.step_cache = 0.1
        with pytest.raises(ValueError, match="step_cache"):
            cfg_reuse.begin_video(m)


def test_call_signatures_are_unchanged():
    for pipe in pipelines():
        p = inspect.signature(pipe.__call__).parameters
        assert list(p)[-1] == "attn_window_dense_steps" and not any(n.startswith("cfg_reuse") for n in p)


def test_from_pretrained_keywords_reach_the_transformer_loader_with_their_defaults(monkeypatch, tmp_path):
    for pipe, cls in zip(pipelines(), model_classes()):
        seen = {}

        class Loaded(SimpleNamespace):
            pass

        def loader(path, *a, _seen=seen, **kw):
            _seen.update(kw)
            return Loaded()

        monkeypatch.setattr(cls, "from_pretrained", loader)
        pipe.from_pretrained(str(tmp_path), cfg_reuse=3, cfg_reuse_t_lo=50, cfg_reuse_t_hi=900, scheduler=object(), device="cpu")
        assert (seen["cfg_reuse"], seen["cfg_reuse_t_lo"], seen["cfg_reuse_t_hi"]) == (3, 50, 900), pipe
        seen.clear()
        pipe.from_pretrained(str(tmp_path), scheduler=object(), device="cpu")
        assert (seen["cfg_reuse"], seen["cfg_reuse_t_lo"], seen["cfg_reuse_t_hi"]) == (0, 100, 800), pipe
        given = Loaded()                                                          # like attn_reuse=: no effect on an instance passed in
        pipe.from_pretrained(str(tmp_path), transformer=given, cfg_reuse=2, scheduler=object(), device="cpu")
        assert not hasattr(given, "cfg_reuse")
        with pytest.raises(ValueError, match="cfg_reuse=1"):
            pipe.from_pretrained(str(tmp_path), cfg_reuse=1, device="cpu")
        with pytest.raises(ValueError, match="cfg_reuse_t_lo"):
            pipe.from_pretrained(str(tmp_path), cfg_reuse=2, cfg_reuse_t_lo=800, cfg_reuse_t_hi=100, device="cpu")
    assert cfg_reuse.switches_from({}) == dict(cfg_reuse=0, cfg_reuse_t_lo=100, cfg_reuse_t_hi=800)


def test_transformer_loaders_set_the_switches_on_a_freshly_loaded_model(monkeypatch, tmp_path):
    from alg_amd import lora
    for cls in model_classes():
        assert "cfg_reuse.switches_from(_)" in inspect.getsource(cls.from_pretrained)
        with pytest.raises(ValueError, match="cfg_reuse=1"):                      # refused before the disk is read
            cls.from_pretrained(str(tmp_path / "nowhere"), cfg_reuse=1)
        with pytest.raises(ValueError, match="cfg_reuse_t_lo"):
            cls.from_pretrained(str(tmp_path / "nowhere"), cfg_reuse=2, cfg_reuse_t_lo=5, cfg_reuse_t_hi=5)
    m = SimpleNamespace()
    cfg_reuse.apply_switches(m, cfg_reuse.switches_from(dict(cfg_reuse=2, cfg_reuse_t_hi=700)))
    assert (m.cfg_reuse, m.cfg_reuse_t_lo, m.cfg_reuse_t_hi) == (2, 100, 700)


# ---- run.py --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["cogvideox_alg.yaml", "wan_alg.yaml", "hunyuan_video_alg.yaml"])
def test_run_py_flags_parse_arrive_and_refuse(config, monkeypatch):
    import yaml

    import run
    off = run.make_parser().parse_args([])
    assert off.cfg_reuse == 0 and off.cfg_reuse_timesteps is None
    args = run.make_parser().parse_args(["--config", os.path.join(ROOT, "configs", config), "--synthetic", "--cfg_reuse", "3",
                                         "--cfg_reuse_timesteps", "50,900"])
    assert args.cfg_reuse == 3 and args.cfg_reuse_timesteps == "50,900"
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["synthetic_config"] = {"num_layers": 1}                          # (no VAE is built)
    hy = "hunyuan" in config
    if hy:                                                                        # the shipped config is the distilled one: no true CFG
        assert cfg["generation"]["true_cfg_scale"] == 1.0
        with pytest.raises(SystemExit, match="--cfg_reuse.*true_cfg_scale"):
            run.build_pipeline(cfg, args, "cpu")
        cfg["generation"]["true_cfg_scale"] = 6.0
    made = []

    def stand_in(*a, **kw):
        made.append(SimpleNamespace(config=SimpleNamespace(), dtype=None))
        return made[-1]

    monkeypatch.setattr(run, "_synthetic_transformer", stand_in)
    for name in ("CogVideoXImageToVideoPipeline", "WanImageToVideoPipeline", "HunyuanVideoImageToVideoPipeline"):
        monkeypatch.setattr(run, name, lambda transformer=None, **kw: SimpleNamespace(transformer=transformer, to=lambda d, _t=transformer: SimpleNamespace(transformer=_t)))
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert t is made[0] and (t.cfg_reuse, t.cfg_reuse_t_lo, t.cfg_reuse_t_hi) == (3, 50, 900)
    args.cfg_reuse_timesteps = None
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert (t.cfg_reuse, t.cfg_reuse_t_lo, t.cfg_reuse_t_hi) == (3, 100, 800)
    args.attn_reuse = 2                                                           # the two reuses compose
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert (t.cfg_reuse, t.attn_reuse) == (3, 2)
    args.attn_reuse, args.cfg_reuse = 0, 0
    assert not hasattr(run.build_pipeline(cfg, args, "cpu").transformer, "cfg_reuse")        # off: the attribute is left alone
    hand = SimpleNamespace(**{k: v for k, v in vars(args).items() if not k.startswith("cfg_reuse")})
    assert not hasattr(run.build_pipeline(cfg, hand, "cpu").transformer, "cfg_reuse")        # a namespace built by hand, without the flags
    scale = "true_cfg_scale" if hy else "guidance_scale"
    for bad, flag in ((dict(cfg_reuse=1), "--cfg_reuse"), (dict(cfg_reuse=2, cfg_reuse_timesteps="800,100"), "--cfg_reuse"),
                      (dict(cfg_reuse=2, cfg_reuse_timesteps="abc"), "--cfg_reuse_timesteps"),
                      (dict(cfg_reuse=2, step_cache=0.1), "--step_cache"),
                      (dict(cfg_reuse=0, cfg_reuse_timesteps="50,900", step_cache=0.1), "--step_cache")):
        ns = run.make_parser().parse_args(["--config", args.config, "--synthetic"])
        for k, v in bad.items():
            setattr(ns, k, v)
        with pytest.raises(SystemExit, match=flag):
            run.build_pipeline(cfg, ns, "cpu")
    ns = run.make_parser().parse_args(["--config", args.config, "--synthetic", "--cfg_reuse", "2"])
    cfg["generation"][scale] = 1.0
    with pytest.raises(SystemExit, match="--cfg_reuse.*" + scale):
        run.build_pipeline(cfg, ns, "cpu")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_exported_and_wrapped():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    lib = alg_amd.load_library()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define ALG_CFG_DELTA_STORE 0\b", header) and re.search(r"#define ALG_CFG_DELTA_REUSE 1\b", header)
    assert (_lib.CFG_DELTA_STORE, _lib.CFG_DELTA_REUSE) == (0, 1) == (cfg_reuse.STORE, cfg_reuse.REUSE)
    assert list(inspect.signature(_lib.cfg_ddim_step_delta_).parameters) == [
        "pred", "latents", "delta", "mode", "guidance_scale", "sqrt_alpha_t", "sqrt_beta_t", "coef_a", "coef_b"]
    assert list(inspect.signature(_lib.cfg_combine_delta).parameters) == ["pred", "delta", "mode", "guidance_scale"]
    assert list(inspect.signature(_lib.cfg_delta_drift).parameters) == ["a", "b", "workspace", "out"]
    from alg_amd.schedulers import CogVideoXDDIMScheduler
    assert list(inspect.signature(CogVideoXDDIMScheduler.fused_cfg_step_delta_).parameters) == [
        "self", "noise_pred", "latents", "delta", "mode", "guidance_scale", "timestep"]


def test_drift_workspace_bytes():
    lib, pair = alg_amd.load_library(), 16
    T_, B_ = _lib.CFG_DRIFT_THREADS, _lib.CFG_DRIFT_MAX_BLOCKS
    for numel, blocks in ((0, 1), (1, 1), (105, 1), (8 * T_, 1), (8 * T_ + 1, 2), (105 * 8 * T_, 105), (1123200, B_),
                          (8 * T_ * B_, B_), (8 * T_ * B_ + 1, B_), (1 << 33, B_)):
        assert lib.alg_cfg_delta_drift_workspace_bytes(numel) == blocks * pair == _lib.cfg_delta_drift_workspace_bytes(numel), numel
    assert lib.alg_cfg_delta_drift_workspace_bytes(-1) == -1 and b"alg_cfg_delta_drift_workspace_bytes" in lib.alg_last_error()


def test_argument_refusals_come_before_any_launch():
    """Host memory stands in for the operands: every call below must return before a kernel is launched."""
    lib = alg_amd.load_library()
    buf = (ctypes.c_char * 256)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = lambda off=0: ctypes.c_void_p(base + off)
    ddim = lambda pred=p(), pd=0, delta=p(64), lat=p(128), ld=0, mode=0, numel=8: lib.alg_cfg_ddim_step_delta(
        pred, pd, delta, lat, ld, mode, numel, 6.0, 0.9, 0.4, 1.0, 0.1, None)
    comb = lambda pred=p(), delta=p(64), out=p(128), dt=0, mode=0, numel=8: lib.alg_cfg_combine_delta(
        pred, delta, out, dt, mode, numel, 6.0, None)
    drift = lambda a=p(), b=p(64), dt=0, numel=8, work=p(128), out=p(192): lib.alg_cfg_delta_drift(a, b, dt, numel, work, out, None)
    for name, call in (("alg_cfg_ddim_step_delta", ddim), ("alg_cfg_combine_delta", comb)):
        for kw in (dict(mode=2), dict(mode=-1), dict(numel=-1), dict(pred=None), dict(delta=None)):
            assert call(**kw) == -1 and name.encode() in lib.alg_last_error(), (name, kw)
        assert call(numel=0, pred=None, delta=None) == 0                       # nothing to do: ALG_OK without a launch
    for kw in (dict(pd=2), dict(ld=7), dict(lat=None), dict(pred=p(2)), dict(pd=1, pred=p(1)), dict(delta=p(66)), dict(ld=1, lat=p(129))):
        assert ddim(**kw) == -1 and b"alg_cfg_ddim_step_delta" in lib.alg_last_error(), kw
    for kw in (dict(dt=2), dict(out=None), dict(pred=p(2)), dict(dt=1, delta=p(65)), dict(out=p(130))):
        assert comb(**kw) == -1 and b"alg_cfg_combine_delta" in lib.alg_last_error(), kw
    for kw in (dict(dt=2), dict(numel=-1), dict(a=None), dict(b=None), dict(work=None), dict(out=None), dict(a=p(8)), dict(b=p(68)),
               dict(work=p(132)), dict(out=p(196))):
        assert drift(**kw) == -1 and b"alg_cfg_delta_drift" in lib.alg_last_error(), kw
    assert drift(numel=0, a=None, b=None, work=None, out=None) == 0
