"""Per-head frame windows for head_dim 64 (CogVideoX), the host side: the C ABI of alg_flash_attn_d64_ranges_heads against its
binding, the wrapper's refusals, and the switch on the model and the pipeline.  No GPU."""
import inspect
import os
import re

import pytest
import torch

import alg_amd
from alg_amd.attn_window import KvRangesHeads, frame_window_ranges, full_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "alg_flash_attn_d64_ranges_heads"


def _prototype(name, text):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_export_source_and_wrapper_agree_on_the_entry():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "attention.hip")).read()
    lib_src = open(os.path.join(ROOT, "alg_amd", "_lib.py")).read()
    assert _prototype(NAME, header) == [
        "const void* q", "const void* k", "const void* vt", "void* o", "int batch", "int heads", "int S", "int64_t q_bstride",
        "int64_t q_rstride", "int64_t vt_bstride", "int64_t vt_rstride", "int64_t o_bstride", "int64_t o_rstride",
        "const int32_t* kv_ranges", "int max_ranges", "int table_heads", "float* lse", "void* stream"]
    assert NAME in alg_amd._lib.EXPORTS
    assert re.search(r'extern "C" int %s\(' % NAME, src)
    defined = _prototype(NAME, src[src.index('extern "C" int ' + NAME + "("):])
    strip = lambda a: a.rsplit(" ", 1)[0]                       # the type of an argument
    assert [strip(a) for a in _prototype(NAME, header)] == [strip(a) for a in defined]
    m = re.search(r"lib\.%s\.argtypes = (.*?)\n    lib\." % NAME, lib_src, re.S)
    ns = {k: getattr(alg_amd._lib, k) for k in ("c_void_p", "c_int", "c_int64", "c_float")}
    assert len(eval(m.group(1), ns)) == 18
    # the existing entries keep their prototypes
    assert re.search(r"alg_flash_attn_d64_ranges\([^;]*const int32_t\* kv_ranges,\s*int max_ranges, void\* stream\);", header)
    assert list(inspect.signature(alg_amd._lib.flash_attn_d64_ranges).parameters)[-3:] == ["kv_ranges", "q_off", "k_off"]
    sig = inspect.signature(alg_amd._lib.flash_attn_d64_ranges_heads).parameters
    assert list(sig)[13:] == ["kv_ranges", "lse", "q_off", "k_off", "lse_off"]
    assert sig["lse"].default is None and sig["q_off"].default == 0 and sig["k_off"].default == 0 and sig["lse_off"].default == 0
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_wrapper_takes_only_validated_tables_of_the_calls_shape(monkeypatch):
    L = alg_amd._lib

    def touched(*a, **kw):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load_library", touched)            # refused before the library or a device is touched
    args = (None, None, None, None, 1, 2, 300, 0, 0, 0, 0, 0, 0)
    with pytest.raises(L.AlgHipError, match="KvRanges"):
        L.flash_attn_d64_ranges_heads(*args, full_ranges(300, 300).table)
    with pytest.raises(L.AlgHipError, match="Sq=256"):
        L.flash_attn_d64_ranges_heads(*args, full_ranges(256, 256))
    with pytest.raises(L.AlgHipError, match="Sq=300 Skv=512"):
        L.flash_attn_d64_ranges_heads(*args, full_ranges(300, 512))         # Sq != Skv: the entry has one S
    with pytest.raises(L.AlgHipError, match="3 heads"):
        L.flash_attn_d64_ranges_heads(*args, KvRangesHeads(torch.stack([full_ranges(300, 300).table] * 3), 300, 300))
    with pytest.raises(L.AlgHipError, match="built for"):
        L.flash_attn_d64_ranges_heads(*args, frame_window_ranges(6, 160, 1, prefix=70))


def test_the_model_and_the_pipeline_carry_the_switch():
    from alg_amd.attn_window import HeadWindowHost
    from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    assert issubclass(CogVideoXTransformer3DModel, HeadWindowHost) and callable(CogVideoXTransformer3DModel.reset_attn_window_heads)
    assert isinstance(CogVideoXTransformer3DModel.attn_window_calibrated, property)
    assert "CogVideoXTransformer3DModel" in HeadWindowHost.__doc__
    pipe = CogVideoXImageToVideoPipeline
    params = inspect.signature(pipe.from_pretrained).parameters
    assert params["attn_window_recall"].default == 0.0
    assert list(params).index("attn_window_recall") == list(params).index("attn_window") + 1      # behind attn_window
    assert list(inspect.signature(pipe.__call__).parameters)[-1] == "attn_window_dense_steps"     # __call__ is unchanged
    with pytest.raises(ValueError, match="attn_window"):
        pipe.from_pretrained("/nonexistent", transformer=object(), attn_window_recall=0.9)         # needs attn_window > 0
