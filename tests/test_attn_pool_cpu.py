"""The pooled far field (alg_amd/attn_pool.py) on the CPU: the exact partition on the 64 G grid, the switch and its refusals, the
loaders' keywords, the C ABI's names and argument errors, and the float64 reference of the operator against its formula."""
import ctypes
import inspect
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import alg_amd
from alg_amd import attn_far, attn_pool, attn_reuse, sampler_ext
from alg_amd.attn_pool import AttnPoolHost
from alg_amd.attn_window import (KV_ALIGN, KvRanges, _block_ranges, call_transformer, complement_ranges, frame_window_ranges,
                                 grid_aligned, pooled_ranges, ranges_to_mask)
from helpers import attn_pool_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN = ([None], 2, 2, 64, 8)


def model_classes():
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    return CogVideoXTransformer3DModel, WanTransformer3DModel, HunyuanVideoTransformer3DModel


# ---- the tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("layout,hw", [("prefix", 384), ("prefix", 380), ("tail", 384), ("tail", 380), ("plain", 384), ("plain", 380)])
def test_near_and_the_expanded_far_groups_visit_every_key_exactly_once(layout, hw, G):
    window, near, far, pooled = R.tables(layout, hw, G)
    Skv = window.Skv
    wm, nm, fm, pm = (ranges_to_mask(t) for t in (window, near, far, pooled))
    assert pm.shape == (window.Sq, Skv // G)
    expanded = pm.repeat_interleave(G, dim=1)                                    # pooled key p stands for the keys [p G, (p + 1) G)
    expanded = torch.cat([expanded, torch.zeros(window.Sq, Skv - expanded.shape[1], dtype=torch.bool)], dim=1)
    count = nm.to(torch.int32) + expanded.to(torch.int32)
    assert bool((count == 1).all())                                              # every key of every block exactly once
    assert torch.equal(expanded, fm)                                             # the pooled table IS the far table, divided
    assert bool((nm | ~wm).all())                                                # near only widens the window
    # every cut on the 64 G grid, the pooled ranges on the kernels' grid, the keys behind the last multiple of 64 G near
    for blk in _block_ranges(far):
        assert all(b % (KV_ALIGN * G) == 0 and e % (KV_ALIGN * G) == 0 for b, e in blk)
    for blk in _block_ranges(pooled):
        assert all(b % KV_ALIGN == 0 and e % KV_ALIGN == 0 for b, e in blk)
    assert bool(nm[:, Skv - Skv % (KV_ALIGN * G):].all())
    if layout == "prefix":
        assert bool(nm[:, :R.PREFIX].all()) and bool(nm[:256].all()) and not _block_ranges(far)[0]     # the block with the prompt rows
    if layout == "tail":
        S = R.FRAMES * hw
        assert bool(nm[:, S:].all()) and bool(nm[-1].all()) and not _block_ranges(far)[-1]             # the prompt rows see everything
    assert any(_block_ranges(far))                                               # and some block has a far key


def test_grid_aligned_keeps_its_one_argument_behaviour():
    for layout, hw in (("prefix", 384), ("tail", 380), ("plain", 380)):
        t = R.window_table(layout, hw)
        assert torch.equal(grid_aligned(t).table, grid_aligned(t, grid=64).table)
        assert torch.equal(grid_aligned(t).table, grid_aligned(t, KV_ALIGN).table)
    assert inspect.signature(grid_aligned).parameters["grid"].default == 64
    t = R.window_table("plain", 380)
    assert not any(e == t.Skv and b == t.Skv - t.Skv % 64 for blk in _block_ranges(grid_aligned(t))[:2] for b, e in blk)
    for bad in (0, 32, 96, -64):
        with pytest.raises(ValueError, match="multiple of 64"):
            grid_aligned(t, grid=bad)


def test_pooled_ranges_refuses_a_far_table_off_the_group_grid():
    t = R.window_table("plain", 384)
    far64 = complement_ranges(grid_aligned(t))                                   # on the 64 grid only: 1152 = 4.5 x 256
    with pytest.raises(ValueError, match="256-key grid"):
        pooled_ranges(far64, 4)
    far = complement_ranges(grid_aligned(t, grid=256))
    p = pooled_ranges(far, 4)
    assert p.Skv == t.Skv // 4 and p.Sq == t.Sq
    assert pooled_ranges(far, 4, Skv=t.Sq).Skv == t.Sq                           # the d = 64 entries state one S
    assert _block_ranges(p) == [[(b // 4, e // 4) for b, e in blk] for blk in _block_ranges(far)]


# ---- the switch ----------------------------------------------------------------------------------------------------------------
def test_switch_helpers():
    assert attn_pool.switches_from({}) == dict(attn_far_pool=0)
    kw = dict(attn_far_pool=4, other=1)
    assert attn_pool.switches_from(kw) == dict(attn_far_pool=4) and kw == dict(other=1)
    assert "attn_far_pool" not in attn_reuse.switches_from({})                    # (that dict is pinned: this module has its own)
    assert attn_far.switches_from({}) == dict(attn_far_reuse=0, attn_far_reuse_t_lo=100, attn_far_reuse_t_hi=800)
    for bad in (1, 3, 6, 16, -2, 2.5, True, "4", None):
        with pytest.raises(ValueError, match="attn_far_pool="):
            attn_pool.check_switch(bad)
    assert [attn_pool.check_switch(g) for g in (0, 2, 4, 8, 4.0)] == [0, 2, 4, 8, 4]
    t = SimpleNamespace()
    attn_pool.apply_switches(t, dict(attn_far_pool=2))
    assert t.attn_far_pool == 2 and attn_pool.active(t) and not attn_pool.active(SimpleNamespace())


def test_the_three_models_carry_the_switch_off():
    for cls in model_classes():
        assert issubclass(cls, AttnPoolHost)
        m = object.__new__(cls)
        assert m.attn_far_pool == 0 and type(m.attn_far_pool) is int
        assert m.attn_far_pool_bytes == 0 and m._attn_pool_obj is None and attn_pool.active(m) is False
        assert m._attn_pool_begin(*BEGIN) is None and m._attn_pool_obj is None    # off: nothing happens, nothing is made
        assert attn_pool.begin_video(m) is False


def test_a_forward_refuses_what_does_not_compose_and_names_both_switches():
    for cls in model_classes():
        m = object.__new__(cls)
        m.attn_far_pool = 4
        with pytest.raises(ValueError, match=r"attn_far_pool=4 with attn_window=0"):
            m._attn_pool_begin(*BEGIN)
        with pytest.raises(ValueError, match=r"attn_far_pool=4 with attn_window=0"):
            attn_pool.begin_video(m)
        m.attn_window = 1
        assert m._attn_pool_begin(*BEGIN) is None and m.attn_far_pool_bytes == 0   # the window covers the video: dense, nothing made
        assert attn_pool.begin_video(m) is True
        for name, value in (("attn_far_reuse", 2), ("attn_window_recall", 0.9), ("attn_window_balance", "lanes"), ("fp8_attention", True),
                            ("attn_band", 3), ("attn_window_widths", (1, 2))):
            if name == "attn_window_widths" and cls is model_classes()[0]:
                continue                                                           # (CogVideoX refuses the widths by itself)
            setattr(m, name, value)
            with pytest.raises(ValueError, match=r"attn_far_pool=4 with %s=" % name):
                m._attn_pool_begin(*BEGIN)
            with pytest.raises(ValueError, match=r"attn_far_pool=4 with %s=" % name):
                attn_pool.begin_video(m)
            setattr(m, name, None if name == "attn_window_widths" else type(value)())
        for name, value in (("step_cache", 0.1), ("attn_reuse", 2), ("cfg_reuse", 2)):    # these compose: no state across steps
            setattr(m, name, value)
            assert m._attn_pool_begin(*BEGIN) is None and attn_pool.begin_video(m) is True
        for bad in (3, 16, 1):
            m.attn_far_pool = bad
            with pytest.raises(ValueError, match="attn_far_pool=%d" % bad):
                m._attn_pool_begin(*BEGIN)
            with pytest.raises(ValueError, match="attn_far_pool=%d" % bad):
                attn_pool.begin_video(m)


def test_a_dense_step_is_not_a_missing_window():
    m = object.__new__(model_classes()[0])
    m.attn_far_pool, m.attn_window = 2, 1
    seen = []

    def forward(**kw):
        seen.append((m.attn_window, m._attn_dense_step))
        return m._attn_pool_begin(*BEGIN)

    assert call_transformer(m, True, forward=forward) is None                     # a sampler's dense step: no refusal, dense launches
    assert seen == [(0, True)] and m.attn_window == 1 and m._attn_dense_step is False and m.attn_far_pool_bytes == 0


def test_an_active_forward_builds_the_tables_and_sizes_one_workspace(monkeypatch):
    made = []
    monkeypatch.setattr(KvRanges, "on", lambda self, device: made.append(self) or self.table)
    m = object.__new__(model_classes()[1])
    m.attn_far_pool, m.attn_window, m.device = 4, 1, "cpu"
    w = R.window_table("plain", 384)
    p = m._attn_pool_begin([w], 2, 3, 128, w.Sq)
    assert isinstance(p, attn_pool.AttnPoolPass) and p.group == 4 and (p.samples, p.rows, p.P) == (2, 3456, 896)
    near, pooled = p.tables[0]
    assert len(made) == 2 and pooled.Skv == 3456 // 4 and m.attn_far_pool_bytes == 0       # the workspace: the first layer's launch
    assert m._attn_pool_begin([w], 2, 3, 128, w.Sq).tables[0][0] is near and len(made) == 2   # built once per table
    # the documented formula, head_dim 128: samples x (P D 2 + D P 2 + rows D 2 + 2 heads rows 4)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    st = m._attn_pool_obj
    st.workspace((2, 3456, 3, 128, 896, 384, 896), torch.device("cpu"))
    assert m.attn_far_pool_bytes == 2 * (896 * 384 * 2 + 384 * 896 * 2 + 3456 * 384 * 2 + 2 * 3 * 3456 * 4)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    held = (st.k.data_ptr(), st.vt.data_ptr(), st.o_far.data_ptr(), st.lse_near.data_ptr(), st.lse_far.data_ptr(), st.bytes)
    st.workspace((2, 3456, 3, 128, 896, 384, 896), torch.device("cpu"))                    # the same shape: nothing is allocated
    # grow-only: one sample (cfg_reuse, cfg_split) and a larger G live in what is there -- also inside a capture
    st.workspace((1, 3456, 3, 128, 896, 384, 896), torch.device("cpu"))
    st.workspace((2, 3456, 3, 128, 448, 384, 448), torch.device("cpu"))
    assert held == (st.k.data_ptr(), st.vt.data_ptr(), st.o_far.data_ptr(), st.lse_near.data_ptr(), st.lse_far.data_ptr(), st.bytes)
    assert st.shape == (2, 3456, 3, 128, 448, 384, 448)                                    # (the strides of the running forward)
    with pytest.raises(alg_amd._lib.AlgHipError, match="before capturing"):
        st.workspace((3, 3456, 3, 128, 896, 384, 896), torch.device("cpu"))                # a larger one has to grow: not in a capture
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    st.workspace((3, 3456, 3, 128, 896, 384, 896), torch.device("cpu"))
    assert st.bytes == held[5] // 2 * 3


def test_sampler_extensions_check_it_and_drive_nothing():
    cog = model_classes()[0]
    m = object.__new__(cog)
    m.attn_far_pool, m.attn_window, m.attn_window_recall, m.attn_reuse = 2, 1, 0.0, 2
    ext = sampler_ext.SamplerExtensions(m, 4)
    assert ext.far is False and ext.reuse is True                                 # attn_reuse next to it: its own drive, unchanged
    m.attn_far_reuse = 2
    m.attn_reuse = 0
    with pytest.raises(ValueError, match="attn_far_pool=2 with attn_far_reuse=2"):
        sampler_ext.SamplerExtensions(m, 4)


# ---- pipelines and loaders -----------------------------------------------------------------------------------------------------
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
        pipe.from_pretrained(str(tmp_path), attn_window=2, attn_far_pool=4, scheduler=object(), device="cpu")
        assert seen["attn_far_pool"] == 4, pipe
        seen.clear()
        pipe.from_pretrained(str(tmp_path), scheduler=object(), device="cpu")
        assert seen["attn_far_pool"] == 0, pipe
        given = SimpleNamespace()                                                  # like fp8=: no effect on an instance passed in
        pipe.from_pretrained(str(tmp_path), transformer=given, attn_window=2, attn_far_pool=2, scheduler=object(), device="cpu")
        assert not hasattr(given, "attn_far_pool") and given.attn_window == 2
        assert list(inspect.signature(pipe.from_pretrained).parameters)[-1] == "_"  # the named keywords are as they were
        assert "attn_far_pool" not in inspect.signature(pipe.from_pretrained).parameters
        for bad, match in ((dict(attn_far_pool=3, attn_window=2), "attn_far_pool=3"),
                           (dict(attn_far_pool=2), "attn_far_pool=2 with attn_window=0"),
                           (dict(attn_far_pool=2, attn_window=2, attn_far_reuse=2), "attn_far_pool=2 with attn_far_reuse=2"),
                           (dict(attn_far_pool=2, attn_window=2, attn_window_recall=0.9), "attn_far_pool=2 with attn_window_recall")):
            with pytest.raises(ValueError, match=match):
                pipe.from_pretrained(str(tmp_path), device="cpu", **bad)
    for pipe in pipelines()[1:]:
        with pytest.raises(ValueError, match="attn_far_pool=2 with fp8_attention"):
            pipe.from_pretrained(str(tmp_path), device="cpu", attn_far_pool=2, attn_window=2, fp8_attention=True)


def test_transformer_loaders_take_the_switch_from_their_trailing_keywords(tmp_path):
    for cls in model_classes():
        assert list(inspect.signature(cls.from_pretrained).parameters)[-2:] == ["lora", "_"]
        with pytest.raises(ValueError, match="attn_far_pool=5"):                   # refused before the disk is read
            cls.from_pretrained(str(tmp_path / "nowhere"), attn_far_pool=5)


def test_call_signatures_are_unchanged():
    for pipe in pipelines():
        p = inspect.signature(pipe.__call__).parameters
        assert list(p)[-1] == "attn_window_dense_steps" and not any(n.startswith("attn_far") for n in p)


@pytest.mark.parametrize("config", ["wan_alg.yaml", "hunyuan_video_alg.yaml", "cogvideox_alg.yaml"])
def test_run_py_flag_parses_and_arrives(config, monkeypatch):
    import yaml

    import run
    assert run.make_parser().parse_args([]).attn_far_pool == 0
    base = ["--config", os.path.join(ROOT, "configs", config), "--synthetic"]
    args = run.make_parser().parse_args(base + ["--attn_window", "2", "--attn_far_pool", "4"])
    assert args.attn_far_pool == 4
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["synthetic_config"] = {"num_layers": 1}                          # (no VAE is built)
    made = []

    def stand_in(*a, **kw):
        made.append(SimpleNamespace(config=SimpleNamespace(), dtype=None))
        return made[-1]

    monkeypatch.setattr(run, "_synthetic_transformer", stand_in)
    for name in ("CogVideoXImageToVideoPipeline", "WanImageToVideoPipeline", "HunyuanVideoImageToVideoPipeline"):
        monkeypatch.setattr(run, name, lambda transformer=None, **kw: SimpleNamespace(
            transformer=transformer, to=lambda d, _t=transformer: SimpleNamespace(transformer=_t)))
    if "cogvideox" in config:      # a CogVideoX config refuses --attn_window, so the switch is reached through from_pretrained
        with pytest.raises(SystemExit, match="--attn_window"):
            run.build_pipeline(cfg, args, "cpu")
        args.attn_window = 0
        with pytest.raises(SystemExit, match="--attn_far_pool: needs --attn_window > 0"):
            run.build_pipeline(cfg, args, "cpu")
        return
    t = run.build_pipeline(cfg, args, "cpu").transformer
    assert t is made[0] and (t.attn_far_pool, t.attn_window) == (4, 2)
    args.attn_far_pool = 0
    assert not hasattr(run.build_pipeline(cfg, args, "cpu").transformer, "attn_far_pool")     # off: the attribute is left alone
    for bad, flag in ((dict(attn_far_pool=3), "--attn_far_pool"), (dict(attn_far_pool=2, attn_window=0), "needs --attn_window > 0"),
                      (dict(attn_far_pool=2, attn_far_reuse=2), "--attn_far_pool with --attn_far_reuse"),
                      (dict(attn_far_pool=2, attn_window_recall=0.9), "--attn_far_pool with --attn_window_recall"),
                      # (--attn_window itself refuses --fp8_attention before anything else)
                      (dict(attn_far_pool=2, fp8_attention=True), "with --fp8_attention")):
        ns = run.make_parser().parse_args(base + ["--attn_window", "2"])
        for k, v in bad.items():
            setattr(ns, k, v)
        with pytest.raises(SystemExit, match=flag):
            run.build_pipeline(cfg, ns, "cpu")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
NEW = ("alg_attn_pool_k", "alg_attn_pool_vt", "alg_attn_merge_lse_shift")


def test_header_exports_binding_and_library_agree_on_the_names():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    lib = alg_amd.load_library()
    for name in NEW:
        assert name in declared and name in alg_amd._lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    L = alg_amd._lib
    assert list(inspect.signature(L.attn_merge_lse_shift).parameters)[:14] == [
        "o", "lse", "o_far", "lse_far", "batch", "heads", "head_dim", "Sq", "o_bs", "o_rs", "far_bs", "far_rs", "far_lse_shift", "lse_out"]
    assert list(inspect.signature(L.attn_merge_lse).parameters)[:13] == [
        "o", "lse", "o_far", "lse_far", "batch", "heads", "head_dim", "Sq", "o_bs", "o_rs", "far_bs", "far_rs", "lse_out"]
    for fn in (L.attn_pool_k, L.attn_pool_vt):
        assert list(inspect.signature(fn).parameters) == ["src", "dst", "batch", "heads", "head_dim", "S", "group", "src_bs", "src_rs",
                                                          "dst_bs", "dst_rs", "src_off", "dst_off"]
    # the declared parameter counts are the bound ones
    for name in NEW:
        params = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(params.split(",")) == len(getattr(lib, name).argtypes), name


def test_argument_errors_come_before_any_launch():
    lib = alg_amd.load_library()
    bufs = [(ctypes.c_char * 4096)() for _ in range(5)]
    src, dst, lse, lse_far, out = (ctypes.c_void_p((ctypes.addressof(x) + 63) // 64 * 64) for x in bufs)
    for name, least in (("alg_attn_pool_k", 128), ("alg_attn_pool_vt", 64)):
        fn = getattr(lib, name)

        def call(src=src, dst=dst, sbs=0, srs=128, dbs=0, drs=128, batch=1, heads=2, hd=64, S=16, G=2):
            rc = fn(src, sbs, srs, dst, dbs, drs, batch, heads, hd, S, G, None)
            return rc, lib.alg_last_error()

        for kw in (dict(src=None), dict(dst=None), dict(src=ctypes.c_void_p(src.value + 8)), dict(dst=ctypes.c_void_p(dst.value + 2))):
            rc, msg = call(**kw)
            assert rc == -1 and name.encode() in msg and b"aligned" in msg, kw
        for kw in (dict(G=1), dict(G=3), dict(G=16), dict(G=0), dict(hd=96), dict(batch=0), dict(heads=0), dict(S=1), dict(S=0),
                   dict(S=7, G=8)):
            rc, msg = call(**kw)
            assert rc == -1 and name.encode() in msg and b"bad argument" in msg, kw
        for kw in (dict(srs=least - 8), dict(drs=least - 8), dict(srs=132), dict(drs=132), dict(sbs=4), dict(dbs=-8),
                   dict(batch=2, sbs=8), dict(batch=2, sbs=1 << 20, dbs=8)):
            rc, msg = call(**kw)
            assert rc == -1 and name.encode() in msg and b"bad strides" in msg, (name, kw)

    def merge(shift=1.0, hd=64, o=src):
        rc = lib.alg_attn_merge_lse_shift(o, lse, dst, lse_far, 1, 2, hd, 4, 512, 128, 512, 128, shift, out, None)
        return rc, lib.alg_last_error()

    for shift in (float("inf"), float("-inf"), float("nan")):
        rc, msg = merge(shift=shift)
        assert rc == -1 and b"alg_attn_merge_lse_shift" in msg and b"finite" in msg, shift
    rc, msg = merge(hd=96)
    assert rc == -1 and b"alg_attn_merge_lse_shift" in msg and b"head_dim" in msg
    rc, msg = merge(o=None)
    assert rc == -1 and b"alg_attn_merge_lse_shift: null" in msg
    rc = lib.alg_attn_merge_lse(None, lse, dst, lse_far, 1, 2, 64, 4, 512, 128, 512, 128, out, None)
    assert rc == -1 and b"alg_attn_merge_lse: null" in lib.alg_last_error()       # the existing entry keeps its own name


def test_the_binding_checks_dtypes_shapes_and_strides_before_the_library_sees_them():
    L = alg_amd._lib
    x = torch.zeros(1, 128, 128, dtype=torch.bfloat16)
    for fn in (L.attn_pool_k, L.attn_pool_vt):
        with pytest.raises(L.AlgHipError, match="device tensor"):
            fn(x, x, 1, 2, 64, 128, 2, 0, 128, 0, 128)
        with pytest.raises(L.AlgHipError, match="group=3"):
            fn(x, x, 1, 2, 64, 128, 3, 0, 128, 0, 128)
        with pytest.raises(L.AlgHipError, match="head_dim=96"):
            fn(x, x, 1, 2, 96, 128, 2, 0, 128, 0, 128)
    with pytest.raises(L.AlgHipError, match="finite"):
        L.attn_merge_lse_shift(x, None, x, None, 1, 2, 64, 128, 0, 128, 0, 128, float("nan"))


# ---- the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4])
def test_the_reference_by_partials_is_the_formula(G):
    """operator_ref evaluates the formula as ONE softmax over [near keys; pooled keys biased by log2 G]; partials_ref takes the
    kernels' route (two partials, the far LSE shifted, the merge).  Float64: they agree to rounding."""
    g = torch.Generator().manual_seed(5)
    hw = 192
    q, k, v = (torch.randn(1, 2, R.PREFIX + R.FRAMES * hw, 16, generator=g).to(torch.bfloat16) for _ in range(3))
    window, near, far, pooled = R.tables("prefix", hw, G)
    nm, pm = ranges_to_mask(near), ranges_to_mask(pooled)
    assert any(_block_ranges(far)) and not _block_ranges(far)[0]
    unit = R.LOG2E / 4.0
    a, b = R.operator_ref(q, k, v, nm, pm, G, unit), R.partials_ref(q, k, v, nm, pm, G, unit)
    assert (a - b).abs().max().item() < 1e-12
    # a row without a far key is the exact attention over its near keys; with G = 1 groups (no pooling) the operator is dense
    dense = R.windowed_ref(q, k, v, torch.ones_like(nm), unit)
    assert (a[:, :, :256] - dense[:, :, :256]).abs().max().item() < 1e-12
    assert (a[:, :, 256:] - dense[:, :, 256:]).abs().max().item() > 1e-4
    # the literal formula on one row, by hand
    row = 300
    s = (q[0, 0, row].double() @ k[0, 0].double().T) * unit
    kp, vp = R.pool_ref(k, G, 2)[0, 0].double(), R.pool_ref(v, G, 2)[0, 0].double()
    sp = (q[0, 0, row].double() @ kp.T) * unit
    wn = torch.where(nm[row], torch.exp2(s - s.max()), torch.zeros_like(s))
    wp = torch.where(pm[row, :kp.shape[0]], G * torch.exp2(sp - s.max()), torch.zeros_like(sp))
    want = (wn @ v[0, 0].double() + wp @ vp) / (wn.sum() + wp.sum())
    assert (a[0, 0, row] - want).abs().max().item() < 1e-12


def test_pool_ref_is_the_mean_rounded_once():
    x = torch.arange(24, dtype=torch.float32).reshape(1, 12, 2).to(torch.bfloat16)
    assert torch.equal(R.pool_ref(x, 4, 1).float(), x.float().reshape(1, 3, 4, 2).mean(dim=2))
    assert R.pool_ref(x[:, :11], 4, 1).shape == (1, 2, 2)                         # a last partial group is left out


@pytest.mark.parametrize("G", [2, 4])
def test_on_trained_like_operands_the_pooled_far_field_beats_the_window_alone_in_float64(G):
    """The inequality tests/test_gpu_attn_pool.py asserts on the kernels' output, established first without them: block 0 of the
    small trained-like CogVideoX oracle, 9 x 384 + 10 tokens, window 1, latent rows, relative L2 against dense.  Measured:
    window only 0.1163, pooled G = 2 0.0657, G = 4 0.0907."""
    e_window, e_pool = R.window_vs_pool_errors(G)
    print("trained-like, float64: window only %.4f, pooled G = %d %.4f" % (e_window, G, e_pool))
    assert e_pool < e_window
