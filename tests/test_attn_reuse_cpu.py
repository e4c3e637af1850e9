"""Attention reuse across steps, host side: the rule of alg_amd.attn_reuse.AttnReuse as a truth table, the switches on the three
model classes, from_pretrained's keywords, the unchanged __call__ signatures, run.py's two flags, and the C ABI of the drift
kernel (names, argument refusals before any launch).  No GPU."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest

import alg_amd
from alg_amd import attn_reuse
from alg_amd.attn_reuse import AttnReuse, AttnReuseHost, StepKeys, step_keys
from alg_amd.step_cache import pass_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alg_attn_drift", "alg_attn_drift_workspace_bytes")


def run_steps(rule, steps):
    """steps: (keys, t, force) per sampler step, one forward each -> the `reused` column"""
    out = []
    for keys, t, force in steps:
        rule.advance()
        hit = rule.decide(keys, t, force)
        if not hit:
            rule.mark_written(keys)
        out.append(hit)
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_every_second_and_every_third_step():
    k = ["cond"]
    assert run_steps(AttnReuse(2), [(k, 500, False)] * 7) == [False, True, False, True, False, True, False]
    assert run_steps(AttnReuse(3), [(k, 500, False)] * 7) == [False, True, True, False, True, True, False]
    assert run_steps(AttnReuse(0), [(k, 500, False)] * 3) == [False] * 3           # off: never


def test_both_range_edges_are_exclusive():
    k = ["cond"]
    for t, want in ((100, False), (101, True), (799, True), (800, False), (99, False), (801, False)):
        assert run_steps(AttnReuse(2, 100, 800), [(k, 500, False), (k, t, False)]) == [False, want], t
    assert run_steps(AttnReuse(2, 0, 1000), [(k, 999.5, False), (k, 0.5, False)]) == [False, True]    # flow timesteps are floats


def test_force_computes_and_rewrites():
    k = ["cond"]
    r = AttnReuse(2)
    assert run_steps(r, [(k, 500, False), (k, 500, True), (k, 500, False), (k, 500, False)]) == [False, False, True, False]
    assert [s["forced"] for s in r.stats] == [False, True, False, False]
    assert r.stats[2] == {"keys": k, "t": 500, "reused": True, "forced": False}


def test_a_new_key_computes_and_an_absent_key_is_left_alone():
    r = AttnReuse(3)
    assert run_steps(r, [(["uncond", "cond"], 500, False)]) == [False]
    # a forward that brings a key without an entry computes, all of it
    assert run_steps(r, [(["uncond_init", "uncond", "cond"], 500, False)]) == [False]
    # "uncond_init" is absent from now on: its entry ages but nothing invalidates it, and the two others go on
    assert run_steps(r, [(["uncond", "cond"], 500, False)] * 3) == [True, True, False]
    assert "uncond_init" in r._age and r._age["uncond_init"] == 3


def test_three_to_two_pass_hand_over():
    r = AttnReuse(2)
    three, two = pass_keys(3, 1), pass_keys(2, 1)
    assert run_steps(r, [(three, 500, True), (three, 500, False), (two, 500, False), (two, 500, False)]) == [False, True, False, True]
    # several videos per call: the key carries the video's index
    r = AttnReuse(2)
    assert run_steps(r, [(pass_keys(3, 2), 500, False), (pass_keys(2, 2), 500, False)]) == [False, True]


def test_reset_forgets_every_key_and_the_record():
    r = AttnReuse(2)
    run_steps(r, [(["cond"], 500, False)])
    r.reset()
    assert r.stats == []
    assert run_steps(r, [(["cond"], 500, False)]) == [False]


def test_a_computed_forward_is_out_of_use_until_it_is_written():
    r = AttnReuse(2)
    run_steps(r, [(["cond"], 500, False)])
    r.advance()
    assert r.decide(["cond"], 900, False) is False and not r.valid(["cond"])     # (the forward died before mark_written)
    r.advance()
    assert r.decide(["cond"], 500, False) is False


def test_refusals_of_the_switches():
    for bad in (1, -1, 2.5, True):
        with pytest.raises(ValueError, match="attn_reuse"):
            AttnReuse(bad)
    for lo, hi in ((800, 800), (801, 800)):
        with pytest.raises(ValueError, match="attn_reuse_t_lo"):
            AttnReuse(2, lo, hi)
    assert (AttnReuse(2).t_lo, AttnReuse(2).t_hi) == (100, 800)                   # diffusers' PAB defaults, spatial attention


def test_step_keys_are_pass_keys_with_the_timestep():
    k = step_keys(3, 1, 981)
    assert isinstance(k, list) and list(k) == pass_keys(3, 1) and k.timestep == 981.0
    assert list(step_keys(2, 2, 0.5)) == pass_keys(2, 2)
    assert StepKeys(["a"], 3).timestep == 3.0


# ---- the model classes -----------------------------------------------------------------------------------------------------
def model_classes():
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    return CogVideoXTransformer3DModel, WanTransformer3DModel, HunyuanVideoTransformer3DModel


def test_the_three_models_carry_the_switches_off():
    for cls in model_classes():
        assert issubclass(cls, AttnReuseHost)
        m = object.__new__(cls)
        assert m.attn_reuse == 0 and isinstance(m.attn_reuse, int)
        assert (m.attn_reuse_t_lo, m.attn_reuse_t_hi) == (100, 800) and type(m.attn_reuse_t_lo) is int
        assert m.attn_reuse_drift is False and m.attn_reuse_bytes == 0 and m.attn_reuse_stats == []
        assert attn_reuse.active(m) is False
        assert m._attn_reuse_begin(["cond"], False, 1, 2, 8, 64) is None          # off: nothing happens, nothing is allocated
        assert m._attn_reuse_obj is None or m._attn_reuse_obj.entries == {}
        m.attn_reuse = 2
        assert attn_reuse.active(m) is True
        assert m._attn_reuse_begin(None, False, 1, 2, 8, 64) is None              # a forward that names no keys is the plain one
        with pytest.raises(ValueError, match="timestep"):
            m._attn_reuse_begin(["cond"], False, 1, 2, 8, 64)                     # plain keys carry no timestep
        with pytest.raises(ValueError, match="each of the 2 samples"):
            m._attn_reuse_begin(StepKeys(["cond"], 500), False, 2, 2, 8, 64)
        m.attn_reuse = 1
        with pytest.raises(ValueError, match="attn_reuse=1"):
            m._attn_reuse_begin(StepKeys(["cond"], 500), False, 1, 2, 8, 64)
        m.attn_reuse, m.attn_reuse_t_lo = 2, 800
        with pytest.raises(ValueError, match="attn_reuse_t_lo"):
            m._attn_reuse_begin(StepKeys(["cond"], 500), False, 1, 2, 8, 64)
        m.attn_reuse, m.attn_reuse_t_lo, m.attn_reuse_drift = 0, 100, True
        with pytest.raises(ValueError, match="attn_reuse_drift"):
            m._attn_reuse_begin(StepKeys(["cond"], 500), False, 1, 2, 8, 64)
    assert attn_reuse.active(SimpleNamespace()) is False                          # the loops' stand-in transformers are left alone


def test_step_cache_and_cfg_split_are_refused_not_dropped():
    cog, wan, hy = model_classes()
    for cls in (cog, wan):
        m = object.__new__(cls)
        m.attn_reuse, m.step_cache = 2, 0.1
        with pytest.raises(ValueError, match="step_cache"):
            m._attn_reuse_begin(StepKeys(["cond"], 500), False, 1, 2, 8, 64)
        with pytest.raises(ValueError, match="step_cache"):
            attn_reuse.begin_video(m)
    for cls in (cog, wan, hy):
        m = object.__new__(cls)
        assert attn_reuse.begin_video(m, cfg_split=object()) is False             # off: nothing to refuse
        m.attn_reuse = 2
        with pytest.raises(ValueError, match="cfg_split"):
            attn_reuse.begin_video(m, cfg_split=object())
        m._attn_reuse_state().stats.append("stale")
        assert attn_reuse.begin_video(m) is True and m.attn_reuse_stats == []     # a new video: reset


def test_transformer_forwards_take_cache_keys():
    cog, wan, hy = model_classes()
    for fn in (cog.__call__, cog.forward_assembled, wan.__call__, hy.__call__):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["cache_keys", "cache_force"] and p["cache_keys"].default is None and p["cache_force"].default is False


# ---- pipelines ---------------------------------------------------------------------------------------------------------------
def pipelines():
    from alg_amd import CogVideoXImageToVideoPipeline, HunyuanVideoImageToVideoPipeline, WanImageToVideoPipeline
    return CogVideoXImageToVideoPipeline, WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline


def test_call_signatures_are_unchanged():
    for pipe in pipelines():
        p = inspect.signature(pipe.__call__).parameters
        assert list(p)[-1] == "attn_window_dense_steps" and not any(n.startswith("attn_reuse") for n in p)


def test_from_pretrained_keywords_reach_the_transformer_loader_with_their_defaults(monkeypatch, tmp_path):
    for pipe, cls in zip(pipelines(), model_classes()):
        seen = {}

        class Loaded(SimpleNamespace):
            pass

        def loader(path, *a, _seen=seen, **kw):
            _seen.update(kw)
            return Loaded()

        monkeypatch.setattr(cls, "from_pretrained", loader)
        pipe.from_pretrained(str(tmp_path), attn_reuse=3, attn_reuse_t_lo=50, attn_reuse_t_hi=900, scheduler=object(), device="cpu")
        assert (seen["attn_reuse"], seen["attn_reuse_t_lo"], seen["attn_reuse_t_hi"]) == (3, 50, 900), pipe
        seen.clear()
        pipe.from_pretrained(str(tmp_path), scheduler=object(), device="cpu")
        assert (seen["attn_reuse"], seen["attn_reuse_t_lo"], seen["attn_reuse_t_hi"]) == (0, 100, 800), pipe
        given = Loaded()                                                          # like fp8=: no effect on an instance passed in
        pipe.from_pretrained(str(tmp_path), transformer=given, attn_reuse=2, scheduler=object(), device="cpu")
        assert not hasattr(given, "attn_reuse")
        with pytest.raises(ValueError, match="attn_reuse=1"):
            pipe.from_pretrained(str(tmp_path), attn_reuse=1, device="cpu")
        with pytest.raises(ValueError, match="attn_reuse_t_lo"):
            pipe.from_pretrained(str(tmp_path), attn_reuse=2, attn_reuse_t_lo=800, attn_reuse_t_hi=100, device="cpu")
    assert attn_reuse.switches_from({}) == dict(attn_reuse=0, attn_reuse_t_lo=100, attn_reuse_t_hi=800)
    m = SimpleNamespace()
    attn_reuse.apply_switches(m, attn_reuse.switches_from(dict(attn_reuse=2)))
    assert (m.attn_reuse, m.attn_reuse_t_lo, m.attn_reuse_t_hi) == (2, 100, 800)


def test_transformer_loaders_take_the_switches_from_their_trailing_keywords(tmp_path):
    for cls in model_classes():
        p = inspect.signature(cls.from_pretrained).parameters
        assert list(p)[-2:] == ["lora", "_"]                                      # the named keywords are pinned
        assert "switches_from(_)" in inspect.getsource(cls.from_pretrained) and "apply_switches(model" in inspect.getsource(cls.from_pretrained)
        with pytest.raises(ValueError, match="attn_reuse=1"):                     # refused before the disk is read
            cls.from_pretrained(str(tmp_path / "nowhere"), attn_reuse=1)
        with pytest.raises(ValueError, match="attn_reuse_t_lo"):
            cls.from_pretrained(str(tmp_path / "nowhere"), attn_reuse=2, attn_reuse_t_lo=5, attn_reuse_t_hi=5)


# ---- run.py --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["cogvideox_alg.yaml", "wan_alg.yaml", "hunyuan_video_alg.yaml"])
def test_run_py_flags_parse_and_arrive(config, monkeypatch):
    import yaml

    import run
    off = run.make_parser().parse_args([])
    assert off.attn_reuse == 0 and off.attn_reuse_timesteps is None
    args = run.make_parser().parse_args(["--config", os.path.join(ROOT, "configs", config), "--synthetic", "--attn_reuse", "3",
                                         "--attn_reuse_timesteps", "50,900"])
    assert args.attn_reuse == 3 and args.attn_reuse_timesteps == "50,900"
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["synthetic_config"] = {"num_layers": 1}                          # (no VAE is built)
    made = []

    def stand_in(*a, **kw):
        made.append(SimpleNamespace(config=SimpleNamespace(), dtype=None))
        return made[-1]

    monkeypatch.setattr(run, "_synthetic_transformer", stand_in)
    for name in ("CogVideoXImageToVideoPipeline", "WanImageToVideoPipeline", "HunyuanVideoImageToVideoPipeline"):
        monkeypatch.setattr(run, name, lambda transformer=None, **kw: SimpleNamespace(transformer=transformer, to=lambda d, _t=transformer: SimpleNamespace(transformer=_t)))
    pipe = run.build_pipeline(cfg, args, "cpu")
    t = pipe.transformer
    assert t is made[0] and (t.attn_reuse, t.attn_reuse_t_lo, t.attn_reuse_t_hi) == (3, 50, 900)
    args.attn_reuse_timesteps = None
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert (t.attn_reuse, t.attn_reuse_t_lo, t.attn_reuse_t_hi) == (3, 100, 800)
    args.attn_reuse = 0
    assert not hasattr(run.build_pipeline(cfg, args, "cpu").transformer, "attn_reuse")       # off: the attribute is left alone
    for bad, flag in ((dict(attn_reuse=1), "--attn_reuse"), (dict(attn_reuse=2, attn_reuse_timesteps="800,100"), "--attn_reuse"),
                      (dict(attn_reuse=2, attn_reuse_timesteps="abc"), "--attn_reuse_timesteps"),
                      (dict(attn_reuse=2, step_cache=0.1), "--step_cache"),
                      (dict(attn_reuse=0, attn_reuse_timesteps="50,900", step_cache=0.1), "--step_cache")):
        ns = run.make_parser().parse_args(["--config", args.config, "--synthetic"])
        for k, v in bad.items():
            setattr(ns, k, v)
        with pytest.raises(SystemExit, match=flag):
            run.build_pipeline(cfg, ns, "cpu")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_exports_binding_and_library_agree_on_the_two_names():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    lib = alg_amd.load_library()
    for name in NAMES:
        assert name in declared and name in alg_amd._lib.EXPORTS and hasattr(lib, name), name
    assert callable(alg_amd._lib.attn_drift) and callable(alg_amd._lib.attn_drift_workspace_bytes)
    assert list(inspect.signature(alg_amd._lib.attn_drift).parameters) == ["a", "b", "workspace", "out"]


def test_workspace_query_is_a_host_function_and_exposes_the_grid_cap():
    lib, L = alg_amd.load_library(), alg_amd._lib
    pair = 2 * 8
    assert lib.alg_attn_drift_workspace_bytes(1, 8) == pair                       # one vector: one block
    assert lib.alg_attn_drift_workspace_bytes(257, 192) == -(-257 * 24 // L.ATTN_DRIFT_THREADS) * pair
    assert lib.alg_attn_drift_workspace_bytes(4096, 512) == L.ATTN_DRIFT_MAX_BLOCKS * pair       # capped
    assert lib.alg_attn_drift_workspace_bytes(75600, 5120) == L.ATTN_DRIFT_MAX_BLOCKS * pair
    assert L.attn_drift_workspace_bytes(3, 64) == lib.alg_attn_drift_workspace_bytes(3, 64) == pair
    assert lib.alg_attn_drift_workspace_bytes(0, 64) == pair                      # rows == 0 is fine
    for rows, cols in ((4, 60), (4, 0), (-1, 64)):
        assert lib.alg_attn_drift_workspace_bytes(rows, cols) == -1
        assert b"alg_attn_drift_workspace_bytes" in lib.alg_last_error()


def test_drift_argument_errors_come_before_any_launch():
    lib = alg_amd.load_library()
    bufs = [(ctypes.c_char * 4096)() for _ in range(4)]
    a, b, work, out = (ctypes.c_void_p((ctypes.addressof(x) + 63) // 64 * 64) for x in bufs)

    def call(a=a, b=b, rows=4, cols=64, sa=64, sb=64, work=work, out=out):
        rc = lib.alg_attn_drift(a, b, rows, cols, sa, sb, work, out, None)
        return rc, lib.alg_last_error()

    for null in ("a", "b", "work", "out"):
        rc, msg = call(**{null: None})
        assert rc == -1 and b"alg_attn_drift" in msg and b"null" in msg, null
    for kw in (dict(cols=60), dict(cols=0), dict(rows=-1)):
        rc, msg = call(**kw)
        assert rc == -1 and b"alg_attn_drift" in msg and b"multiple of 8" in msg, kw
    for kw in (dict(sa=56), dict(sb=56), dict(sa=68), dict(sb=-64), dict(sa=2 ** 40 + 4)):
        rc, msg = call(**kw)
        assert rc == -1 and b"alg_attn_drift" in msg and b"row strides" in msg, kw
    for off in ("a", "b"):
        rc, msg = call(**{off: ctypes.c_void_p(locals()[off].value + 2)})
        assert rc == -1 and b"alg_attn_drift" in msg and b"aligned" in msg, off
    rc, msg = call(out=ctypes.c_void_p(out.value + 4))
    assert rc == -1 and b"aligned" in msg


def test_an_entry_that_does_not_fit_raises_with_its_byte_count(monkeypatch):
    import torch

    r = AttnReuse(2)
    got = r.buffers(["cond"], 2, 8, 64, "cpu")                                   # (the bookkeeping does not care where the tensors live)
    assert [tuple(t.shape) for t in got] == [(2, 8, 64)] and r.bytes == 2 * 1 * 8 * 64 * 2

    def no_room(*a, **kw):
        raise torch.cuda.OutOfMemoryError("out of memory")

    monkeypatch.setattr(torch, "empty", no_room)
    with pytest.raises(alg_amd._lib.AlgHipError, match=r"needs 2048 bytes .*next to the 2048 bytes of the 1 entries held"):
        r.buffers(["cond", "uncond"], 2, 8, 64, "cpu")
    monkeypatch.undo()
    assert r.buffers(["cond"], 3, 8, 64, "cpu")[0].shape == (3, 8, 64) and r.bytes == 3 * 8 * 64 * 2      # another shape drops what was held
