"""Per-head frame windows chosen by recall, the host side (alg_amd/attn_window.py): per-head tables and their validation, the
decision rule, the C ABI of the two new entries against the binding, and run.py's flag with its refusals.  No GPU."""
import argparse
import inspect
import os
import re

import pytest
import torch

import alg_amd
from alg_amd.attn_window import (KvRanges, KvRangesHeads, calibration_step, decide_heads, frame_window_ranges, full_ranges,
                                 head_window_ranges, ranges_to_mask)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_head_window_ranges_gives_windowed_heads_the_base_rows_and_the_others_the_full_range():
    base = frame_window_ranges(8, 256, 1)                      # 8 blocks, up to two ranges
    assert base.max_ranges == 2 and base.coverage < 1
    assert head_window_ranges(base, [True, True, True]) is base
    assert head_window_ranges(base, [False, False]) is None
    r = head_window_ranges(base, [True, False, True])
    assert isinstance(r, KvRangesHeads) and (r.heads, r.q_blocks, r.max_ranges, r.Sq, r.Skv) == (3, 8, 2, 2048, 2048)
    assert r.table.dtype == torch.int32 and tuple(r.table.shape) == (3, 8, 2, 2)
    assert torch.equal(r.table[0], base.table) and torch.equal(r.table[2], base.table)
    want_full = torch.zeros(8, 2, 2, dtype=torch.int32)
    want_full[:, 0, 1] = 2048
    assert torch.equal(r.table[1], want_full)                  # [(0, Skv)], zero-padded to max_ranges
    assert r.per_head[1].is_full and not r.per_head[0].is_full
    assert abs(r.coverage - (2 * base.coverage + 1.0) / 3) < 1e-12
    m = ranges_to_mask(r)
    assert tuple(m.shape) == (3, 2048, 2048) and m.dtype == torch.bool
    assert torch.equal(m[0], ranges_to_mask(base)) and bool(m[1].all()) and torch.equal(m[2], m[0])
    assert tuple(ranges_to_mask(base).shape) == (2048, 2048)   # a shared table keeps its two dimensions
    with pytest.raises(ValueError):
        head_window_ranges(base, [])
    with pytest.raises(ValueError):
        head_window_ranges(base.table, [True, False])


def test_per_head_tables_are_validated_head_by_head():
    good = full_ranges(300, 512).table                         # [2, 1, 2]
    KvRangesHeads(torch.stack([good, good]), 512, 300)
    bad = good.clone()
    bad[1, 0, 0] = 32                                          # begin not on the tile grid, in head 1 only
    with pytest.raises(ValueError, match=r"head 1: block 1: begin 32"):
        KvRangesHeads(torch.stack([good, bad]), 512, 300)
    empty = good.clone()
    empty[0] = 0
    with pytest.raises(ValueError, match=r"head 0: block 0: no key"):
        KvRangesHeads(torch.stack([empty, good]), 512, 300)
    with pytest.raises(ValueError, match="beyond Skv"):
        KvRangesHeads(torch.stack([good, good]), 500, 300)
    with pytest.raises(ValueError):
        KvRangesHeads(good, 512, 300)                          # no head dimension
    with pytest.raises(ValueError):
        KvRangesHeads(torch.stack([good, good]).long(), 512, 300)
    with pytest.raises(ValueError):
        KvRangesHeads(torch.zeros(0, 2, 1, 2, dtype=torch.int32), 512, 300)


def test_decide_heads_takes_the_minimum_over_the_samples_and_never_windows_a_nan():
    assert decide_heads([[0.95, 0.5, 0.9]], 0.9) == [True, False, True]             # >= : the threshold itself passes
    assert decide_heads([[0.95, 0.95], [0.89, 0.91]], 0.9) == [False, True]         # min over the samples
    assert decide_heads([[NAN, 1.0], [1.0, 1.0]], 0.5) == [False, True]
    assert decide_heads([[1.0, 1.0], [NAN, 1.0]], 0.5) == [False, True]
    assert decide_heads([[NAN]], 0.0) == [False]                                     # NaN is not windowed at any threshold
    assert decide_heads([[0.3, 1.0]], 2.0) == [False, False]                         # unreachable
    assert decide_heads([[0.3, 1e-6]], 1e-9) == [True, True]
    assert all(type(x) is bool for x in decide_heads([[0.3, 0.95]], 0.9))
    for bad in ([], [[]], [[0.5, 0.5], [0.5]]):
        with pytest.raises(ValueError):
            decide_heads(bad, 0.5)


def test_the_calibration_step_is_the_last_dense_one():
    assert [calibration_step(n) for n in (0, 1, 2, 5)] == [0, 0, 1, 4]


def _prototype(name, text):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_exports_and_wrapper_agree_on_the_two_new_entries():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "attention128_q64.hip")).read()
    lib_src = open(os.path.join(ROOT, "alg_amd", "_lib.py")).read()
    for name, n_args, wrapper in (("alg_flash_attn_d128_ranges_heads", 22, "flash_attn_d128_ranges_heads"),
                                  ("alg_attn_lse_recall", 8, "attn_lse_recall")):
        assert name in alg_amd._lib.EXPORTS and callable(getattr(alg_amd._lib, wrapper))
        declared, defined = _prototype(name, header), _prototype(name, src[src.index('extern "C" int ' + name + "("):])
        assert len(declared) == n_args
        strip = lambda a: a.rsplit(" ", 1)[0]                   # the type of an argument
        assert [strip(a) for a in declared] == [strip(a) for a in defined], name
        m = re.search(r"lib\.%s\.argtypes = (.*?)\n    lib\." % name, lib_src, re.S)
        ns = {k: getattr(alg_amd._lib, k) for k in ("c_void_p", "c_int", "c_int64", "c_float")}
        assert len(eval(m.group(1), ns)) == n_args, name
    tail = _prototype("alg_flash_attn_d128_ranges_heads", header)[-5:]
    assert tail == ["const int32_t* kv_ranges", "int max_ranges", "int table_heads", "float* lse", "void* stream"]
    assert _prototype("alg_attn_lse_recall", header) == ["const float* lse_part", "const float* lse_full", "double* out", "int panels",
                                                         "int Sq", "int row0", "int rows", "void* stream"]
    # the existing entries keep their prototypes
    assert re.search(r"alg_flash_attn_d128_ranges\([^;]*const int32_t\* kv_ranges,\s*int max_ranges, void\* stream\);", header)
    sig = inspect.signature(alg_amd._lib.flash_attn_d128_ranges_heads).parameters
    assert sig["lse"].default is None and sig["k_off"].default == 0 and sig["vt_off"].default == 0
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "alg_flash_attn_d128_ranges_heads" in text and "alg_attn_lse_recall" in text


def test_the_wrapper_takes_only_validated_tables_of_the_calls_shape():
    L = alg_amd._lib
    args = (None, None, None, None, 1, 2, 300, 512, 0, 0, 0, 0, 0, 0, 0, 0, 1.0)
    with pytest.raises(L.AlgHipError, match="KvRanges"):
        L.flash_attn_d128_ranges_heads(*args, full_ranges(300, 512).table)
    with pytest.raises(L.AlgHipError, match="Sq=256"):
        L.flash_attn_d128_ranges_heads(*args, full_ranges(256, 512))
    with pytest.raises(L.AlgHipError, match="3 heads"):
        L.flash_attn_d128_ranges_heads(*args, KvRangesHeads(torch.stack([full_ranges(300, 512).table] * 3), 512, 300))


def test_the_models_and_pipelines_carry_the_switch():
    from alg_amd.attn_window import HeadWindowHost
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    for model in (WanTransformer3DModel, HunyuanVideoTransformer3DModel):
        assert issubclass(model, HeadWindowHost) and callable(model.reset_attn_window_heads)
    for pipe in (WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline):
        assert inspect.signature(pipe.from_pretrained).parameters["attn_window_recall"].default == 0.0
        assert list(inspect.signature(pipe.__call__).parameters)[-1] == "attn_window_dense_steps"     # __call__ is unchanged
    host = HeadWindowHost()
    host._head_window_init()
    assert host.attn_window_recall == 0.0 and host.attn_window_stats == [] and not host.attn_window_calibrated
    assert host._head_window_mode(("k",), 2, 1, 4, 256, (1, 256, 512)) is None and host._attn_cal is None      # off: nothing happens
    host.attn_window_recall = 0.9
    assert host._head_window_mode(("k",), 2, 1, 4, 256, (1, 256, 512)) == "dense" and host._attn_cal is None   # not asked to calibrate
    host._attn_decided = ((("k",), 0.9), [(True, False)] * 2)
    assert host._head_window_mode(("k",), 2, 1, 4, 256, (1, 256, 512)) == "tables"
    assert host._head_window_mode(("other",), 2, 1, 4, 256, (1, 256, 512)) == "dense" and not host.attn_window_calibrated   # dropped


WAN = {"model": {"path": "Wan-AI/Wan2.1-I2V-14B-480P-Diffusers", "dtype": "bfloat16"}, "generation": {"height": 480}}
HY = {"model": {"path": "hunyuanvideo-community/HunyuanVideo-I2V", "dtype": "bfloat16"}, "generation": {}}
COG = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}


def _ns(**kw):
    base = dict(fp8=False, fp8_attention=False, attn_window=0, attn_window_recall=0.0, step_cache=0.0, synthetic=True,
                model_cache_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_run_py_parses_the_flag():
    import run
    assert run.make_parser().parse_args([]).attn_window_recall == 0.0
    ns = run.make_parser().parse_args(["--attn_window", "4", "--attn_window_recall", "0.9"])
    assert ns.attn_window == 4 and ns.attn_window_recall == 0.9


@pytest.mark.parametrize("config,kw", [
    (WAN, dict(attn_window_recall=0.9)),                             # without --attn_window
    (HY, dict(attn_window_recall=0.9)),
    (COG, dict(attn_window_recall=0.9)),                             # no d = 64 per-head entry
    (COG, dict(attn_window=4, attn_window_recall=0.9)),
    (WAN, dict(attn_window=4, attn_window_recall=1.5)),              # out of range
    (WAN, dict(attn_window=4, attn_window_recall=-0.1)),
    (HY, dict(attn_window=4, attn_window_recall=NAN)),
])
def test_run_py_refusals_name_the_flag(config, kw):
    import run
    with pytest.raises(SystemExit, match="--attn_window_recall"):
        run.build_pipeline(config, _ns(**kw), "cuda")
