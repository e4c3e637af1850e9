"""Host side of the HunyuanVideo `fp8` path, without a GPU: the two new C entry points are declared, exported and refuse bad
calls before any launch; run.py still has --fp8 and hands it to both HunyuanVideo constructions; a width the e4m3 path cannot take
is refused by the constructor before it touches the device."""
import argparse
import ctypes
import os
import re
import types

import pytest
import torch

import alg_amd
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alg_layernorm_modulate_seg_fp8", "alg_quantize_fp8_rows_batched")


def test_header_and_exports_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in alg_amd._lib.EXPORTS, name
    assert declared == set(alg_amd._lib.EXPORTS)
    lib = alg_amd.load_library()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.alg_version() == 110
    assert callable(alg_amd._lib.layernorm_modulate_seg_fp8) and callable(alg_amd._lib.quantize_fp8_rows_batched)


def _host_buffer(nbytes, fill):
    """a 64-byte aligned host buffer: argument checks come before any launch, so no call below ever dereferences it"""
    raw = (ctypes.c_uint8 * (nbytes + 64))()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    ctypes.memset(base, fill, nbytes)
    return raw, base


def test_layernorm_modulate_seg_fp8_argument_errors_without_gpu():
    lib = alg_amd.load_library()
    keep_x, x = _host_buffer(4096, 0)
    keep_q, q = _host_buffer(4096, 0xA5)
    keep_s, s = _host_buffer(64, 0x5A)
    keep_m, m = _host_buffer(8192, 0)
    P = ctypes.c_void_p

    def call(x_=x, q_=q, s_=s, scale=m, shift=m + 1024, mod_bs=2048, seg_stride=1024, batch=1, rows=2, D=512, x_bs=1024):
        return lib.alg_layernorm_modulate_seg_fp8(P(x_), P(q_), P(s_), None, None, P(scale) if scale else None,
                                                  P(shift) if shift else None, mod_bs, seg_stride, batch, rows, D, x_bs, 1, 1e-6,
                                                  None)

    for kw, msg in ((dict(x_=0), b"bad argument"), (dict(q_=0), b"bad argument"), (dict(s_=0), b"bad argument"),
                    (dict(x_=x + 2), b"aligned"), (dict(q_=q + 4), b"aligned"), (dict(scale=m + 2), b"aligned"),
                    (dict(D=768), b"multiple of 512"), (dict(D=8704), b"multiple of 512"), (dict(D=500), b"multiple of 512"),
                    (dict(shift=0), b"together"), (dict(scale=0), b"together"),
                    (dict(batch=-1), b"bad argument"), (dict(rows=0), b"bad argument"), (dict(seg_stride=1028), b"bad argument"),
                    (dict(mod_bs=2052), b"aligned"), (dict(x_bs=1028), b"aligned")):
        assert call(**kw) == -1, kw
        err = lib.alg_last_error()
        assert b"alg_layernorm_modulate_fp8" in err and msg in err, (kw, err)
    assert bytes(keep_q).count(b"\xa5") == 4096 and bytes(keep_s).count(b"\x5a") == 64      # nothing was written


def test_quantize_fp8_rows_batched_argument_errors_without_gpu():
    lib = alg_amd.load_library()
    keep_x, x = _host_buffer(4096, 0)
    keep_q, q = _host_buffer(4096, 0xA5)
    keep_s, s = _host_buffer(64, 0x5A)
    P = ctypes.c_void_p

    def call(x_=x, q_=q, s_=s, x_bs=1024, x_rs=512, batch=1, rows=2, K=256):
        return lib.alg_quantize_fp8_rows_batched(P(x_), x_bs, x_rs, P(q_), P(s_), batch, rows, K, None)

    for kw, msg in ((dict(x_=0), b"null or misaligned"), (dict(q_=0), b"null or misaligned"), (dict(s_=0), b"null or misaligned"),
                    (dict(x_=x + 8), b"null or misaligned"), (dict(q_=q + 4), b"null or misaligned"),
                    (dict(s_=s + 2), b"null or misaligned"),
                    (dict(K=12), b"K % 8"), (dict(K=0), b"K % 8"), (dict(K=-8), b"K % 8"), (dict(batch=-1), b"bad shape"),
                    (dict(rows=-3), b"bad shape"), (dict(x_rs=516), b"bad shape"), (dict(x_bs=1028), b"bad shape")):
        assert call(**kw) == -1, kw
        err = lib.alg_last_error()
        assert b"alg_quantize_fp8_rows_batched" in err and msg in err, (kw, err)
    assert call(batch=0) == 0 and call(rows=0) == 0                                            # nothing to do is not an error
    assert bytes(keep_q).count(b"\xa5") == 4096 and bytes(keep_s).count(b"\x5a") == 64        # nothing was written


def test_constructor_refuses_a_width_the_e4m3_path_cannot_take_before_it_touches_the_device():
    with pytest.raises(ValueError, match="D % 512"):          # 3 heads: dim 384
        HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(num_attention_heads=3, rope_axes_dim=(16, 56, 56)), {},
                                       fp8=True)
    with pytest.raises(ValueError, match="K % 128"):          # dim 512, MLP width 64
        HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(num_attention_heads=4, mlp_ratio=0.125), {}, fp8=True)


def test_run_py_keeps_the_flag_and_hands_it_to_both_hunyuan_constructions(monkeypatch):
    import run
    from alg_amd import transformer_hunyuan_video as thv
    assert run.make_parser().parse_args([]).fp8 is False
    assert run.make_parser().parse_args(["--fp8"]).fp8 is True
    help_text = run.make_parser().format_help()
    assert "HunyuanVideo" in help_text and "ignores it" not in help_text
    seen = []

    class FakeTransformer:
        dtype = torch.bfloat16
        config = HunyuanVideoTransformerConfig()

        def __init__(self, cfg, sd, device="cuda", **kw):
            seen.append(("synthetic", kw))

        def to(self, *a, **k):
            return self

    monkeypatch.setattr(run, "HunyuanVideoTransformer3DModel", FakeTransformer)
    monkeypatch.setattr(thv, "synthetic_state_dict", lambda cfg, seed=0, device="cpu": {})
    config = {"model": {"path": "hunyuanvideo-community/HunyuanVideo-I2V", "dtype": "bfloat16",
                        "synthetic_config": {"num_layers": 1, "num_single_layers": 1}}, "generation": {}}
    for fp8, f8a in ((True, False), (False, True), (True, True)):
        ns = argparse.Namespace(fp8=fp8, fp8_attention=f8a, synthetic=True, model_cache_dir=None)
        pipe = run.build_pipeline(config, ns, "cpu")
        assert isinstance(pipe.transformer, FakeTransformer)
        assert seen[-1] == ("synthetic", dict(fp8=fp8, fp8_attention=f8a))

    def from_pretrained(model_path, **kw):
        seen.append(("checkpoint", kw))
        from alg_amd.schedulers import FlowMatchEulerDiscreteScheduler
        sched = FlowMatchEulerDiscreteScheduler(shift=7.0)
        return types.SimpleNamespace(scheduler=sched, to=lambda dev: "the pipeline")

    monkeypatch.setattr(run.HunyuanVideoImageToVideoPipeline, "from_pretrained", staticmethod(from_pretrained))
    ns = argparse.Namespace(fp8=True, fp8_attention=False, synthetic=False, model_cache_dir=None)
    assert run.build_pipeline(config, ns, "cpu") == "the pipeline"
    assert seen[-1][0] == "checkpoint" and seen[-1][1]["fp8"] is True and seen[-1][1]["fp8_attention"] is False


def test_pipeline_loader_hands_fp8_to_the_transformer(monkeypatch):
    from alg_amd import transformer_hunyuan_video as thv
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    seen = {}

    def from_pretrained(path, **kw):
        seen.update(kw)
        raise RuntimeError("stop here")

    monkeypatch.setattr(thv.HunyuanVideoTransformer3DModel, "from_pretrained", staticmethod(from_pretrained))
    with pytest.raises(RuntimeError, match="stop here"):
        HunyuanVideoImageToVideoPipeline.from_pretrained("/nonexistent", device="cpu", fp8=True)
    assert seen["fp8"] is True and seen["fp8_attention"] is False
