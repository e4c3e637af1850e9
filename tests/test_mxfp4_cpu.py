"""OCP MXFP4 feed-forward linears (fp4), the parts that need no GPU: the host emulation of the format against a brute-force
nearest-grid search, the C ABI surface and its refusals (all before any launch), and the flag through run.py / from_pretrained."""
import argparse
import ctypes
import inspect
import os
import re

import pytest
import torch

import alg_amd
from _mxfp4 import GRID, dequantize, fake_quant, mxfp4_linears, pack, quantize, special_blocks, unpack
from alg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alg_gemm_fp4", "alg_quantize_mxfp4_rows")
def brute_force(x, exps):
    """Nearest grid value of x / 2^e by exhaustive search, ties to the even code, float64."""
    grid = torch.tensor(GRID, dtype=torch.float64)
    out = torch.empty(x.shape, dtype=torch.long)
    for r in range(x.shape[0]):
        for c in range(x.shape[1]):
            v = abs(float(x[r, c])) / 2.0 ** exps[r]
            d = (grid - v).abs()
            best = [i for i in range(8) if d[i] == d.min()]
            code = best[0] if len(best) == 1 else [i for i in best if i % 2 == 0][0]
            out[r, c] = code + (8 if torch.signbit(x[r, c]) else 0)
    return out


def test_emulation_quantiser_is_nearest_even_on_the_special_blocks():
    x, exps = special_blocks()
    codes, scales = quantize(x)
    assert scales.shape == (x.shape[0], 1)
    assert scales[:, 0].tolist() == [e + 127 for e in exps]
    assert torch.equal(codes.long(), brute_force(x, exps))
    # spot checks, by hand: ties go to the even code, (6, 8) saturates, small negatives keep their sign on a zero
    s0 = codes[0].tolist()
    assert s0[:7] == [0, 2, 2, 4, 4, 6, 6] and s0[7:14] == [8, 10, 10, 12, 12, 14, 14] and s0[14] == 7
    assert codes[2, :5].tolist() == [7, 7, 7, 15, 15]
    assert codes[2, 7:11].tolist() == [0, 8, 8, 8]
    assert codes[-2].tolist() == [8] * 16 + [0] * 16 and codes[-3].tolist() == [0] * 32
    assert float(dequantize(codes, scales)[-1, 0]) == 1.0 and codes[-1, 0] == 6           # 1.0 = 4 * 2^-2
    assert 255 not in scales.tolist()


def test_emulation_round_trip_packing_and_range():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(7, 256, generator=g) * torch.logspace(-30, 30, 7, base=2.0)[:, None]).bfloat16()
    codes, scales = quantize(x)
    assert torch.equal(unpack(pack(codes)), codes)
    assert pack(codes).shape == (7, 128) and int(pack(codes)[0, 0]) == int(codes[0, 0]) | (int(codes[0, 1]) << 4)
    dq = dequantize(codes, scales)
    # idempotent, and within half a grid step of the input: steps are <= 2 * 2^(e - 127) (1 below 4, then 2 up to 6, saturation
    # reaches 2 below 8) and amax >= 4 * 2^(e - 127)
    assert torch.equal(fake_quant(dq), dq)
    amax = x.double().reshape(7, 8, 32).abs().amax(-1, keepdim=True)
    err = (dq - x.double()).reshape(7, 8, 32).abs()
    assert bool((err <= amax / 4 + 1e-300).all())
    # the extreme exponents clamp: a subnormal-range block writes byte 0, the largest finite bf16 byte 252
    tiny = torch.full((1, 32), 2.0 ** -130).bfloat16()
    big = torch.full((1, 32), 3.0e38).bfloat16()
    assert quantize(tiny)[1].item() == 0 and quantize(big)[1].item() == 252


def test_mxfp4_linears_routes_only_the_two_feed_forward_linears():
    import torch.nn.functional as F
    w = {"transformer_blocks.0.ff.net.0.proj.weight": torch.randn(64, 32), "transformer_blocks.0.ff.net.2.weight": torch.randn(32, 64),
         "transformer_blocks.0.attn1.to_q.weight": torch.randn(32, 32), "proj_out.weight": torch.randn(8, 32)}
    x = torch.randn(5, 32).bfloat16()
    original = F.linear
    with mxfp4_linears(w) as stats:
        a = F.linear(x, w["transformer_blocks.0.ff.net.0.proj.weight"].bfloat16())          # a copy: another pointer, untouched
        b = F.linear(x.float(), w["transformer_blocks.0.ff.net.0.proj.weight"])
        c = F.linear(x.float(), w["transformer_blocks.0.attn1.to_q.weight"])
    assert F.linear is original and stats == {"routed": 1, "other": 2, "weights": 2}
    assert torch.equal(c, original(x.float(), w["transformer_blocks.0.attn1.to_q.weight"]))
    assert a.dtype == torch.bfloat16 and not torch.equal(b, original(x.float(), w["transformer_blocks.0.ff.net.0.proj.weight"]))
    ref = (fake_quant(x) @ fake_quant(w["transformer_blocks.0.ff.net.0.proj.weight"]).t()).float()
    assert torch.allclose(b, ref, rtol=1e-5, atol=1e-5)


# ---- 2. ABI surface -----------------------------------------------------------------------------------------------------
def test_header_and_library_carry_both_entries():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    lib = alg_amd.load_library()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert declared == set(_lib.EXPORTS)
    assert callable(_lib.gemm_fp4) and callable(_lib.quantize_mxfp4_rows)
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "gemm_fp4.hip")).read()
    assert "__builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4" in src


def _args(**kw):
    """A well-formed alg_gemm_fp4 call on made-up (aligned, never dereferenced) addresses; kw overrides fields."""
    a = _lib.GemmArgs()
    a.A, a.B, a.C, a.a_scale, a.b_scale = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.M, a.N, a.K, a.batch = 64, 64, 256, 1
    a.lda = a.ldb = 256
    a.ldc = 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("what,kw", [
    ("packed B", dict(flags=_lib.GEMM_B_PACKED11)),
    ("per-row bias", dict(flags=_lib.GEMM_BIAS_PER_ROW, bias=0x60000)),
    ("permuted columns", dict(flags=_lib.GEMM_PERMUTE_COLS)),
    ("convolution addressing", dict(conv_wp=5, conv_hpwp=25, conv_kw=3, conv_cin_log2=6)),
    ("K % 256", dict(K=128, lda=128, ldb=128)),
    ("no scales", dict(a_scale=None)),
    ("misaligned scales", dict(b_scale=0x50004)),
    ("lda not a multiple of 16 bytes", dict(lda=264)),
    ("activation with residual", dict(R=0x70000, ldr=64, act=_lib.ACT_GELU_TANH)),
    ("gate without residual", dict(gate=0x80000)),
])
def test_gemm_fp4_refusals_name_the_entry_before_any_launch(what, kw):
    lib = alg_amd.load_library()
    a = _args(**kw)
    rc = lib.alg_gemm_fp4(ctypes.byref(a), None)
    assert rc == -1, what
    assert "alg_gemm_fp4" in lib.alg_last_error().decode(), what
    assert lib.alg_gemm_fp4(None, None) == -1


@pytest.mark.parametrize("what,call", [
    ("K % 32", (0x10000, 48, 0x20000, 0x30000, 4, 48)),
    ("K <= 0", (0x10000, 0, 0x20000, 0x30000, 4, 0)),
    ("negative rows", (0x10000, 64, 0x20000, 0x30000, -1, 64)),
    ("row stride % 8", (0x10000, 68, 0x20000, 0x30000, 4, 64)),
    ("row stride below K", (0x10000, 32, 0x20000, 0x30000, 4, 64)),
    ("null x", (None, 64, 0x20000, 0x30000, 4, 64)),
    ("null scales", (0x10000, 64, 0x20000, None, 4, 64)),
    ("misaligned x", (0x10008, 64, 0x20000, 0x30000, 4, 64)),
    ("misaligned q", (0x10000, 64, 0x20002, 0x30000, 4, 64)),
])
def test_quantize_mxfp4_rows_refusals_name_the_entry_before_any_launch(what, call):
    lib = alg_amd.load_library()
    x, rs, q, sc, rows, K = call
    assert lib.alg_quantize_mxfp4_rows(x, rs, q, sc, rows, K, None) == -1, what
    assert "alg_quantize_mxfp4_rows" in lib.alg_last_error().decode(), what


def test_python_wrappers_validate_before_the_library_is_asked():
    u8 = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(_lib.AlgHipError, match="device tensor"):
        _lib.quantize_mxfp4_rows(torch.zeros(2, 32, dtype=torch.bfloat16), u8, u8, 2, 32)
    with pytest.raises(_lib.AlgHipError, match="a_scale and b_scale"):
        _lib.gemm_fp4(u8, u8, u8, 1, 1, 256, 256, 256, 1)
    with pytest.raises(_lib.AlgHipError, match="device tensor"):
        _lib.gemm_fp4(u8, u8, u8, 1, 1, 256, 256, 256, 1, a_scale=u8, b_scale=u8)


# ---- 3. flag and switches -----------------------------------------------------------------------------------------------
def test_run_py_parses_fp4_and_the_other_families_refuse_it():
    import run
    assert run.make_parser().parse_args([]).fp4 is False
    assert run.make_parser().parse_args(["--fp4"]).fp4 is True
    for path in ("Wan-AI/Wan2.1-I2V-14B-720P-Diffusers", "hunyuanvideo-community/HunyuanVideo-I2V"):
        config = {"model": {"path": path, "dtype": "bfloat16"}, "generation": {"height": 720}}
        ns = argparse.Namespace(fp8=False, fp4=True, synthetic=True, model_cache_dir=None)
        with pytest.raises(SystemExit, match="--fp4"):
            run.build_pipeline(config, ns, "cuda")


def test_from_pretrained_carries_fp4_off_and_call_signatures_are_unchanged():
    from alg_amd import CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel
    for fn in (CogVideoXImageToVideoPipeline.from_pretrained, CogVideoXTransformer3DModel.from_pretrained,
               CogVideoXTransformer3DModel.from_synthetic, CogVideoXTransformer3DModel.__init__):
        p = inspect.signature(fn).parameters
        assert p["fp4"].default is False and p["fp8"].default is False, fn
    assert "fp4" not in inspect.signature(CogVideoXImageToVideoPipeline.__call__).parameters
    assert list(inspect.signature(CogVideoXTransformer3DModel.__call__).parameters) == [
        "self", "hidden_states", "encoder_hidden_states", "timestep", "timestep_cond", "ofs", "image_rotary_emb", "attention_kwargs",
        "return_dict", "cache_keys", "cache_force"]
    assert list(inspect.signature(CogVideoXTransformer3DModel.forward_assembled).parameters) == [
        "self", "latents", "conds", "encoder_hidden_states", "timestep", "image_rotary_emb", "ofs", "cache_keys", "cache_force"]
