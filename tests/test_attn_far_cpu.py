"""Far-field attention reuse, host side (alg_amd/attn_far.py): the near / far tables of alg_amd/attn_window.py as an exact partition,
the rule (attn_reuse.AttnReuse's, reused) and the refusals on stand-in transformers, from_pretrained's keywords, run.py's two flags,
the C ABI of alg_attn_merge_lse (names, argument refusals before any launch) and the float64 reference of the merge.  No GPU."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import alg_amd
from alg_amd import attn_far, attn_reuse, sampler_ext
from alg_amd.attn_far import AttnFar, AttnFarHost, StepKeys
from alg_amd.attn_window import (KV_ALIGN, MAX_RANGES, KvRanges, _block_ranges, call_transformer, complement_ranges,
                                 frame_window_ranges, grid_aligned, ranges_to_mask)
from helpers.attn_far_ref import merge_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (frame_window_ranges keywords, far ranges of the widest block, blocks without a far key)
SHAPES = {
    "cog_9x384_prefix32_w1": (dict(frames=9, tokens_per_frame=384, window=1, prefix=32), 2, 1),
    "cog_c2_13x1350_prefix226_w2": (dict(frames=13, tokens_per_frame=1350, window=2, prefix=226), 2, 1),
    "wan_7x160_w1": (dict(frames=7, tokens_per_frame=160, window=1), 2, 0),
    "plain_9x100_w1": (dict(frames=9, tokens_per_frame=100, window=1), 1, 0),
    "hy_9x96_tail50_w1": (dict(frames=9, tokens_per_frame=96, window=1, tail=(864, 914), rows=924), 1, 1),
    "hy_21x240_tail200_w3": (dict(frames=21, tokens_per_frame=240, window=3, tail=(5040, 5240), rows=5296), 2, 2),
}


# ---- the tables --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_near_and_far_visit_every_key_exactly_once(name):
    kw, far_ranges, empty = SHAPES[name]
    window = frame_window_ranges(**kw)
    near = grid_aligned(window)
    far = complement_ranges(near)
    a, b, w = ranges_to_mask(near), ranges_to_mask(far), ranges_to_mask(window)
    assert bool((a | b).all()) and not bool((a & b).any())                       # a partition of every block's keys
    assert bool((w <= a).all())                                                  # the near table is a superset of the window
    assert near.max_ranges <= MAX_RANGES and far.max_ranges <= MAX_RANGES
    per_block = _block_ranges(far)
    assert max(len(r) for r in per_block) == far_ranges and sum(not r for r in per_block) == empty, (name, per_block)
    for blk in _block_ranges(near):
        assert all(b_ % KV_ALIGN == 0 and (e % KV_ALIGN == 0 or e == near.Skv) for b_, e in blk)
    assert all(b_ % KV_ALIGN == 0 for blk in per_block for b_, _ in blk)         # a far range begins where a near one ends
    assert abs(near.coverage + far.coverage - 1.0) < 1e-12
    assert (near.Sq, near.Skv, far.Sq, far.Skv) == (window.Sq, window.Skv) * 2


def test_grid_aligned_merges_ranges_that_come_to_touch():
    t = torch.tensor([[[0, 70], [128, 200], [256, 300]]], dtype=torch.int32)
    near = grid_aligned(KvRanges(t, 300, 10))
    assert _block_ranges(near) == [[(0, 300)]]                                   # 70 -> 128 touches, 200 -> 256 touches
    assert _block_ranges(complement_ranges(near)) == [[]]
    t = torch.tensor([[[64, 70], [256, 290]]], dtype=torch.int32)
    near = grid_aligned(KvRanges(t, 300, 10))
    assert _block_ranges(near) == [[(64, 128), (256, 300)]]
    assert _block_ranges(complement_ranges(near)) == [[(0, 64), (128, 256)]]


def test_complement_refuses_a_table_that_is_not_grid_aligned_and_too_many_gaps():
    t = torch.tensor([[[0, 70], [128, 200]]], dtype=torch.int32)
    with pytest.raises(ValueError, match="grid-aligned"):
        complement_ranges(KvRanges(t, 300, 10))
    t = torch.tensor([[[64, 128], [192, 256], [320, 384], [448, 512]]], dtype=torch.int32)
    with pytest.raises(ValueError, match="5 key ranges"):
        complement_ranges(KvRanges(t, 600, 10))                                  # 5 gaps, the kernels take 4
    with pytest.raises(ValueError, match="KvRanges"):
        grid_aligned(None)


def test_empty_ok_is_opt_in():
    t = torch.zeros(2, 1, 2, dtype=torch.int32)
    t[0, 0, 1] = 64
    with pytest.raises(ValueError, match="block 1: no key"):
        KvRanges(t, 64, 300)                                                     # today's rule is unchanged
    r = KvRanges(t, 64, 300, empty_ok=True)
    assert not r.absent and r.coverage == 256 * 64 / (300 * 64)
    assert list(inspect.signature(KvRanges.__init__).parameters)[-2:] == ["absent_ok", "empty_ok"]
    assert inspect.signature(KvRanges.__init__).parameters["empty_ok"].default is False


# ---- the rule and the buffers ------------------------------------------------------------------------------------------------
def test_the_rule_is_attn_reuse_s_own_class():
    assert issubclass(AttnFar, attn_reuse.AttnReuse)
    assert AttnFar.decide is attn_reuse.AttnReuse.decide and AttnFar.advance is attn_reuse.AttnReuse.advance
    assert attn_far.step_keys is attn_reuse.step_keys and StepKeys is attn_reuse.StepKeys
    r = AttnFar()
    r.every = 2
    out = []
    for t in (500, 500, 500, 900, 500, 500):
        r.advance()
        hit = r.decide(["cond"], t, False)
        if not hit:
            r.mark_written(["cond"])
        out.append(hit)
    assert out == [False, True, False, False, True, False]
    assert r.stats[1] == {"keys": ["cond"], "t": 500, "reused": True, "forced": False}


def test_entries_hold_output_and_lse_and_the_bytes_are_the_documented_product(monkeypatch):
    r = AttnFar()
    layers, rows, heads, hd = 3, 40, 2, 64
    D = heads * hd
    got = r.buffers(["uncond", "cond"], layers, rows, D, heads, 2, "cpu")
    assert [tuple(t.shape) for t in got[0]] == [(layers, rows, D), (layers, heads, rows)]
    assert got[0][0].dtype == torch.bfloat16 and got[0][1].dtype == torch.float32
    assert r.bytes == layers * 2 * (rows * D * 2 + heads * rows * 4)
    assert r.lse_near.numel() == 2 * heads * rows and r.lse_near.dtype == torch.float32
    r.mark_written(["uncond", "cond"])
    r.buffers(["cond"], layers, rows + 1, D, heads, 1, "cpu")                    # another shape drops what was held
    assert not r.valid(["uncond"]) and sorted(r.entries) == ["cond"]

    def no_room(*a, **kw):
        raise torch.cuda.OutOfMemoryError("out of memory")

    monkeypatch.setattr(torch, "empty", no_room)
    need = layers * ((rows + 1) * D * 2 + heads * (rows + 1) * 4)
    with pytest.raises(alg_amd._lib.AlgHipError, match=r"attn_far_reuse: .*needs %d bytes .*next to the %d bytes of the 1 entries" % (need, need)):
        r.buffers(["cond", "uncond"], layers, rows + 1, D, heads, 2, "cpu")


# ---- the model classes -------------------------------------------------------------------------------------------------------
def model_classes():
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    return CogVideoXTransformer3DModel, WanTransformer3DModel, HunyuanVideoTransformer3DModel


KEYS = StepKeys(["cond"], 500)
BEGIN = (KEYS, False, [None], 1, 2, 2, 64, 8)          # cache_keys, cache_force, windows, samples, layers, heads, head_dim, rows


def test_the_three_models_carry_the_switches_off():
    for cls in model_classes():
        assert issubclass(cls, AttnFarHost)
        m = object.__new__(cls)
        assert m.attn_far_reuse == 0 and type(m.attn_far_reuse) is int
        assert (m.attn_far_reuse_t_lo, m.attn_far_reuse_t_hi) == (100, 800) and type(m.attn_far_reuse_t_lo) is int
        assert m.attn_far_reuse_bytes == 0 and m._attn_far_obj is None and attn_far.active(m) is False
        assert m._attn_far_begin(*BEGIN) is None and m._attn_far_obj is None      # off: nothing happens, nothing is made
        assert m.attn_far_reuse_stats == []
    assert attn_far.active(SimpleNamespace()) is False                            # the loops' stand-in transformers are left alone


def test_a_forward_refuses_what_does_not_compose_and_names_both_switches():
    for cls in model_classes():
        m = object.__new__(cls)
        m.attn_far_reuse = 2
        with pytest.raises(ValueError, match=r"attn_far_reuse=2 with attn_window=0"):
            m._attn_far_begin(*BEGIN)
        m.attn_window = 1
        assert m._attn_far_begin(None, *BEGIN[1:]) is None                         # a forward that names no keys
        with pytest.raises(ValueError, match="timestep"):
            m._attn_far_begin(["cond"], *BEGIN[1:])
        with pytest.raises(ValueError, match="each of the 2 samples"):
            m._attn_far_begin(KEYS, False, [None], 2, 2, 2, 64, 8)
        for name, value in (("attn_window_recall", 0.9), ("attn_window_balance", "lanes"), ("fp8_attention", True), ("step_cache", 0.1),
                            ("attn_reuse", 2), ("cfg_reuse", 2), ("attn_band", 3)):
            setattr(m, name, value)
            with pytest.raises(ValueError, match=r"attn_far_reuse=2 with %s=" % name):
                m._attn_far_begin(*BEGIN)
            with pytest.raises(ValueError, match=r"attn_far_reuse=2 with %s=" % name):
                attn_far.begin_video(m)
            setattr(m, name, type(value)())
        m.attn_far_reuse = 1
        with pytest.raises(ValueError, match="attn_far_reuse=1"):
            m._attn_far_begin(*BEGIN)
        m.attn_far_reuse, m.attn_far_reuse_t_lo = 2, 800
        with pytest.raises(ValueError, match="attn_far_reuse_t_lo=800 >= attn_far_reuse_t_hi=800"):
            m._attn_far_begin(*BEGIN)
        m.attn_far_reuse_t_lo = 100
        with pytest.raises(ValueError, match=r"attn_far_reuse=2 with cfg_split"):
            attn_far.begin_video(m, cfg_split=object())
        m._attn_far_state().stats.append("stale")
        assert attn_far.begin_video(m) is True and m.attn_far_reuse_stats == []    # a new video: reset
        m.attn_window = 0
        with pytest.raises(ValueError, match=r"attn_far_reuse=2 with attn_window=0"):
            attn_far.begin_video(m)
    from alg_amd.transformer_wan import WanTransformer3DModel
    m = object.__new__(WanTransformer3DModel)
    m.attn_far_reuse, m.attn_window, m.attn_window_widths = 2, 2, (1, 2)
    with pytest.raises(ValueError, match=r"attn_far_reuse=2 with attn_window_widths="):
        m._attn_far_begin(*BEGIN)


def test_a_dense_step_and_a_covering_window_cache_nothing_and_leave_the_entries_invalid():
    cog = model_classes()[0]
    m = object.__new__(cog)
    m.attn_far_reuse, m.attn_window = 2, 1
    st = m._attn_far_state()
    st.mark_written(["cond"])
    assert m._attn_far_begin(*BEGIN) is None and not st.valid(["cond"])           # the window covers the video (table None)
    assert st.stats == [] and st.entries == {} and m.attn_far_reuse_bytes == 0
    st.mark_written(["cond"])
    seen = []

    def forward(**kw):
        seen.append((m.attn_window, m._attn_dense_step))
        return m._attn_far_begin(*BEGIN)

    assert call_transformer(m, True, forward=forward) is None                     # a sampler's dense step: no refusal
    assert seen == [(0, True)] and m.attn_window == 1 and m._attn_dense_step is False and not st.valid(["cond"])
    plain = SimpleNamespace(attn_window=1)                                         # without the switch nothing is marked
    call_transformer(plain, True, forward=lambda: None)
    assert not hasattr(plain, "_attn_dense_step")


def test_sampler_extensions_drive_it_like_the_attention_reuse():
    cog = model_classes()[0]
    m = object.__new__(cog)
    m.attn_far_reuse, m.attn_window, m.attn_window_recall = 2, 1, 0.0
    ext = sampler_ext.SamplerExtensions(m, 4)
    assert ext.far is True and ext.reuse is False
    calls = []
    for i, t in enumerate((900.0, 600.0, 400.0, 50.0)):
        fn = ext.step(i, t, 2, 1)
        assert fn.func is call_transformer
        kw = fn.keywords
        calls.append((list(kw["cache_keys"]), kw["cache_keys"].timestep, kw["cache_force"]))
        m._attn_far_state().stats.append({"t": t})                                 # (what a forward would record)
    assert calls == [(["uncond", "cond"], 900.0, True), (["uncond", "cond"], 600.0, False), (["uncond", "cond"], 400.0, False),
                     (["uncond", "cond"], 50.0, True)]                             # the first forward of a video, the last step
    off = sampler_ext.SamplerExtensions(object.__new__(cog), 4)
    assert off.far is False and "cache_keys" not in off.step(0, 900.0, 2, 1).keywords


# ---- pipelines and loaders ---------------------------------------------------------------------------------------------------
def pipelines():
    from alg_amd import CogVideoXImageToVideoPipeline, HunyuanVideoImageToVideoPipeline, WanImageToVideoPipeline
    return CogVideoXImageToVideoPipeline, WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline


def test_from_pretrained_keywords_reach_the_transformer_loader_with_their_defaults(monkeypatch, tmp_path):
    for pipe, cls in zip(pipelines(), model_classes()):
        seen = {}

        def loader(path, *a, _seen=seen, **kw):
            _seen.update(kw)
            return SimpleNamespace()

        monkeypatch.setattr(cls, "from_pretrained", loader)
        pipe.from_pretrained(str(tmp_path), attn_window=2, attn_far_reuse=3, attn_far_reuse_t_lo=50, attn_far_reuse_t_hi=900,
                             scheduler=object(), device="cpu")
        assert (seen["attn_far_reuse"], seen["attn_far_reuse_t_lo"], seen["attn_far_reuse_t_hi"]) == (3, 50, 900), pipe
        seen.clear()
        pipe.from_pretrained(str(tmp_path), scheduler=object(), device="cpu")
        assert (seen["attn_far_reuse"], seen["attn_far_reuse_t_lo"], seen["attn_far_reuse_t_hi"]) == (0, 100, 800), pipe
        given = SimpleNamespace()                                                  # like fp8=: no effect on an instance passed in
        pipe.from_pretrained(str(tmp_path), transformer=given, attn_window=2, attn_far_reuse=2, scheduler=object(), device="cpu")
        assert not hasattr(given, "attn_far_reuse") and given.attn_window == 2
        assert list(inspect.signature(pipe.from_pretrained).parameters)[-1] == "_"  # the named keywords are as they were
        for bad, match in ((dict(attn_far_reuse=1, attn_window=2), "attn_far_reuse=1"),
                           (dict(attn_far_reuse=2, attn_window=2, attn_far_reuse_t_lo=800, attn_far_reuse_t_hi=100), "attn_far_reuse_t_lo"),
                           (dict(attn_far_reuse=2), "attn_far_reuse=2 with attn_window=0"),
                           (dict(attn_far_reuse=2, attn_window=2, attn_reuse=2), "attn_far_reuse=2 with attn_reuse=2"),
                           (dict(attn_far_reuse=2, attn_window=2, cfg_reuse=2), "attn_far_reuse=2 with cfg_reuse=2"),
                           (dict(attn_far_reuse=2, attn_window=2, attn_window_recall=0.9), "attn_far_reuse=2 with attn_window_recall")):
            with pytest.raises(ValueError, match=match):
                pipe.from_pretrained(str(tmp_path), device="cpu", **bad)
    assert attn_far.switches_from({}) == dict(attn_far_reuse=0, attn_far_reuse_t_lo=100, attn_far_reuse_t_hi=800)


def test_transformer_loaders_take_the_switches_from_their_trailing_keywords(tmp_path):
    for cls in model_classes():
        assert list(inspect.signature(cls.from_pretrained).parameters)[-2:] == ["lora", "_"]
        with pytest.raises(ValueError, match="attn_far_reuse=1"):                  # refused before the disk is read
            cls.from_pretrained(str(tmp_path / "nowhere"), attn_far_reuse=1)
        with pytest.raises(ValueError, match="attn_far_reuse_t_lo"):
            cls.from_pretrained(str(tmp_path / "nowhere"), attn_far_reuse=2, attn_far_reuse_t_lo=5, attn_far_reuse_t_hi=5)


def test_call_signatures_are_unchanged():
    for pipe in pipelines():
        p = inspect.signature(pipe.__call__).parameters
        assert list(p)[-1] == "attn_window_dense_steps" and not any(n.startswith("attn_far") for n in p)


# ---- run.py --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["wan_alg.yaml", "hunyuan_video_alg.yaml", "cogvideox_alg.yaml"])
def test_run_py_flags_parse_and_arrive(config, monkeypatch):
    import yaml

    import run
    off = run.make_parser().parse_args([])
    assert off.attn_far_reuse == 0 and off.attn_far_reuse_timesteps is None
    base = ["--config", os.path.join(ROOT, "configs", config), "--synthetic"]
    args = run.make_parser().parse_args(base + ["--attn_window", "2", "--attn_far_reuse", "3", "--attn_far_reuse_timesteps", "50,900"])
    assert args.attn_far_reuse == 3 and args.attn_far_reuse_timesteps == "50,900"
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
    if "cogvideox" in config:      # a CogVideoX config refuses --attn_window, so the switch is reached through from_pretrained
        with pytest.raises(SystemExit, match="--attn_window"):
            run.build_pipeline(cfg, args, "cpu")
        args.attn_window = 0
        with pytest.raises(SystemExit, match="--attn_far_reuse: needs --attn_window > 0"):
            run.build_pipeline(cfg, args, "cpu")
        return
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert t is made[0] and (t.attn_far_reuse, t.attn_far_reuse_t_lo, t.attn_far_reuse_t_hi, t.attn_window) == (3, 50, 900, 2)
    args.attn_far_reuse_timesteps = None
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert (t.attn_far_reuse, t.attn_far_reuse_t_lo, t.attn_far_reuse_t_hi) == (3, 100, 800)
    args.attn_far_reuse = 0
    assert not hasattr(run.build_pipeline(cfg, args, "cpu").transformer, "attn_far_reuse")    # off: the attribute is left alone
    for bad, flag in ((dict(attn_far_reuse=1), "--attn_far_reuse"), (dict(attn_far_reuse=2, attn_far_reuse_timesteps="800,100"), "--attn_far_reuse"),
                      (dict(attn_far_reuse=2, attn_far_reuse_timesteps="abc"), "--attn_far_reuse_timesteps"),
                      (dict(attn_far_reuse=2, attn_window=0), "needs --attn_window > 0"),
                      (dict(attn_far_reuse=2, attn_window_recall=0.9), "--attn_far_reuse with --attn_window_recall"),
                      (dict(attn_far_reuse=2, attn_reuse=2), "--attn_far_reuse with --attn_reuse"),
                      # (the HunyuanVideo config runs without CFG: --cfg_reuse is refused for that before anything else)
                      (dict(attn_far_reuse=2, cfg_reuse=2), "--attn_far_reuse with --cfg_reuse" if "wan" in config else "--cfg_reuse")):
        ns = run.make_parser().parse_args(base + ["--attn_window", "2"])
        for k, v in bad.items():
            setattr(ns, k, v)
        with pytest.raises(SystemExit, match=flag):
            run.build_pipeline(cfg, ns, "cpu")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_exports_binding_and_library_agree_on_the_name():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    lib = alg_amd.load_library()
    assert "alg_attn_merge_lse" in declared and "alg_attn_merge_lse" in alg_amd._lib.EXPORTS and hasattr(lib, "alg_attn_merge_lse")
    assert list(inspect.signature(alg_amd._lib.attn_merge_lse).parameters)[:13] == [
        "o", "lse", "o_far", "lse_far", "batch", "heads", "head_dim", "Sq", "o_bs", "o_rs", "far_bs", "far_rs", "lse_out"]


def test_merge_argument_errors_come_before_any_launch():
    lib = alg_amd.load_library()
    bufs = [(ctypes.c_char * 4096)() for _ in range(5)]
    o, lse, far, lse_far, out = (ctypes.c_void_p((ctypes.addressof(x) + 63) // 64 * 64) for x in bufs)

    def call(o=o, lse=lse, far=far, lse_far=lse_far, batch=1, heads=2, hd=64, Sq=4, obs=512, ors=128, fbs=512, frs=128, out=out):
        rc = lib.alg_attn_merge_lse(o, lse, far, lse_far, batch, heads, hd, Sq, obs, ors, fbs, frs, out, None)
        return rc, lib.alg_last_error()

    for null in ("o", "lse", "far", "lse_far"):
        rc, msg = call(**{null: None})
        assert rc == -1 and b"alg_attn_merge_lse" in msg and b"null" in msg, null
    for name in ("o", "far"):
        rc, msg = call(**{name: ctypes.c_void_p(locals()[name].value + 8)})
        assert rc == -1 and b"alg_attn_merge_lse" in msg and b"aligned" in msg, name
    rc, msg = call(lse=ctypes.c_void_p(lse.value + 2))
    assert rc == -1 and b"alg_attn_merge_lse" in msg and b"aligned" in msg
    for hd in (32, 96, 0, 256):
        rc, msg = call(hd=hd)
        assert rc == -1 and b"alg_attn_merge_lse" in msg and b"head_dim" in msg, hd
    for kw in (dict(ors=120), dict(frs=64), dict(ors=132), dict(frs=-128), dict(ors=2 ** 40 + 4)):
        rc, msg = call(**kw)
        assert rc == -1 and b"alg_attn_merge_lse" in msg and b"row strides" in msg, kw
    for kw in (dict(batch=2, obs=500), dict(batch=2, fbs=128), dict(obs=4)):
        rc, msg = call(**kw)
        assert rc == -1 and b"alg_attn_merge_lse" in msg and b"batch strides" in msg, kw
    for kw in (dict(batch=0), dict(heads=0), dict(Sq=-1)):
        rc, msg = call(**kw)
        assert rc == -1 and b"alg_attn_merge_lse" in msg and b"positive" in msg, kw


def test_the_binding_checks_dtypes_shapes_and_strides_before_the_library_sees_them():
    L = alg_amd._lib
    o = torch.zeros(2, 5, 128, dtype=torch.bfloat16)
    with pytest.raises(L.AlgHipError, match="device tensor"):
        L.attn_merge_lse(o, torch.zeros(20), o, torch.zeros(20), 2, 2, 64, 5, 640, 128, 640, 128)
    with pytest.raises(L.AlgHipError, match="head_dim=96"):
        L.attn_merge_lse(o, None, o, None, 2, 2, 96, 5, 640, 128, 640, 128)


# ---- the reference of the merge ------------------------------------------------------------------------------------------------
def test_the_reference_merge_of_two_partials_is_the_softmax_over_the_union():
    g = torch.Generator().manual_seed(5)
    B, H, hd, Sq, Sk = 2, 3, 16, 7, 40
    q, k, v = (torch.randn(B, H, n, hd, generator=g, dtype=torch.float64) for n in (Sq, Sk, Sk))
    s = q @ k.transpose(-1, -2)                                                    # scores in log2 units
    full = torch.softmax(s * 0.6931471805599453, dim=-1) @ v
    near = torch.zeros(Sq, Sk, dtype=torch.bool)
    near[:, 8:24] = True
    near[3] = True                                                                 # a row whose near part holds every key
    near[5] = False                                                                # a row without a near key

    def partial(mask):
        sm = s.masked_fill(~mask, float("-inf"))
        lse = torch.logsumexp(sm * 0.6931471805599453, dim=-1) / 0.6931471805599453
        p = torch.exp2(sm - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse).unsqueeze(-1))
        return (p @ v).transpose(1, 2).reshape(B, Sq, H * hd), lse

    (o_n, l_n), (o_f, l_f) = partial(near), partial(~near)
    assert bool(torch.isinf(l_f[:, :, 3]).all()) and bool(torch.isinf(l_n[:, :, 5]).all())
    merged, lse = merge_ref(o_n, l_n, o_f, l_f, H, hd)
    want = full.transpose(1, 2).reshape(B, Sq, H * hd)
    assert (merged - want).abs().max().item() < 1e-12
    assert (lse - torch.logsumexp(s * 0.6931471805599453, dim=-1) / 0.6931471805599453).abs().max().item() < 1e-12
    assert torch.equal(merged[:, 3], o_n[:, 3]) and torch.equal(merged[:, 5], o_f[:, 5])
    dead = torch.full_like(l_n, float("-inf"))
    m2, l2 = merge_ref(o_n, dead, o_f, dead, H, hd)
    assert torch.equal(m2, o_n) and bool((l2 == float("-inf")).all())
