"""MXFP4 operands written where they are computed (alg_layernorm_modulate_mxfp4, alg_gemm_fp4_q4out), the parts that need no GPU:
the C ABI surface, the refusals of both entries (every one before any launch, on made-up addresses that are never dereferenced)
and the switch the model hangs them on."""
import ctypes
import os
import re

import pytest
import torch

import alg_amd
from alg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alg_gemm_fp4_q4out", "alg_layernorm_modulate_mxfp4")
EINVAL = -1


# ---- 1. ABI surface -----------------------------------------------------------------------------------------------------
def test_header_and_library_carry_both_entries():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    lib = alg_amd.load_library()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert len(lib.alg_gemm_fp4_q4out.argtypes) == 4 and len(lib.alg_layernorm_modulate_mxfp4.argtypes) == 15
    assert len(lib.alg_layernorm_modulate_mxfp4.argtypes) == len(lib.alg_layernorm_modulate_fp8.argtypes)
    assert callable(_lib.layernorm_modulate_mxfp4) and callable(_lib.gemm_fp4)


def test_gemm_args_keeps_its_size():
    """The output scales are a parameter of alg_gemm_fp4_q4out: the struct every GEMM entry takes did not grow."""
    assert ctypes.sizeof(_lib.GemmArgs) == 216               # tests/test_host_logic.py spells the sum out
    assert [n for n, _ in _lib.GemmArgs._fields_][-4:] == ["conv_wp", "conv_hpwp", "conv_kw", "reserved1"]


def test_the_block_quantiser_is_defined_once():
    """The compare chain of the e2m1 rounding stands in row_ops.h and nowhere else; both producers and the row quantiser call it."""
    csrc = os.path.join(ROOT, "alg_amd", "csrc")
    chain = re.compile(r">=\s*0\.75f")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc")) and chain.search(open(os.path.join(csrc, f)).read())]
    assert holders == ["row_ops.h"]
    assert "mxfp4_quantize8" in open(os.path.join(csrc, "norm.hip")).read()
    gemm = open(os.path.join(csrc, "gemm_fp4.hip")).read()
    assert "mxfp4_quantize8" in gemm and "e2m1_pack" in gemm and "mxfp4_scale_byte" in gemm


# ---- 2. alg_gemm_fp4_q4out refuses ----------------------------------------------------------------------------------------
SCALES = 0x60000


def _args(**kw):
    """A well-formed alg_gemm_fp4_q4out call on made-up (aligned, never dereferenced) addresses; kw overrides fields."""
    a = _lib.GemmArgs()
    a.A, a.B, a.C, a.a_scale, a.b_scale = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.M, a.N, a.K, a.batch = 64, 64, 256, 1
    a.lda = a.ldb = 256
    a.ldc = 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("what,kw,scales,bstride", [
    ("N % 32", dict(N=48), SCALES, 0),
    ("N % 32, a multiple of 4", dict(N=36), SCALES, 0),
    ("residual", dict(R=0x70000, ldr=64), SCALES, 0),
    ("gate", dict(gate=0x80000), SCALES, 0),
    ("residual and gate", dict(R=0x70000, ldr=64, gate=0x80000), SCALES, 0),
    ("null out_scales", dict(), None, 0),
    ("misaligned out_scales", dict(), SCALES + 4, 0),
    ("out_scales batch stride % 8", dict(batch=2, strideA=64 * 256, strideC=64 * 64), SCALES, 132),
    ("K % 256", dict(K=128, lda=128, ldb=128), SCALES, 0),
    ("ldc % 32", dict(ldc=80), SCALES, 0),
    ("ldc below N", dict(ldc=32), SCALES, 0),
    ("misaligned C", dict(C=0x30008), SCALES, 0),
    ("C == A", dict(C=0x10000), SCALES, 0),
    ("C inside A", dict(C=0x10000 + 63 * 128), SCALES, 0),
    ("A inside C", dict(A=0x30000 + 63 * 32 + 16), SCALES, 0),
    ("out_scales == a_scale", dict(), 0x40000, 0),
    ("SiLU", dict(act=_lib.ACT_SILU), SCALES, 0),
    ("packed B", dict(flags=_lib.GEMM_B_PACKED11), SCALES, 0),
    ("per-row bias", dict(flags=_lib.GEMM_BIAS_PER_ROW, bias=0x60000), SCALES, 0),
    ("no A scales", dict(a_scale=None), SCALES, 0),
    ("lda not a multiple of 16 bytes", dict(lda=264), SCALES, 0),
    ("misaligned bias", dict(bias=0x90004), SCALES, 0),
])
def test_gemm_fp4_q4out_refusals_name_the_entry_before_any_launch(what, kw, scales, bstride):
    lib = alg_amd.load_library()
    a = _args(**kw)
    assert lib.alg_gemm_fp4_q4out(ctypes.byref(a), scales, bstride, None) == EINVAL, what
    assert "alg_gemm_fp4_q4out" in lib.alg_last_error().decode(), what
    assert lib.alg_gemm_fp4_q4out(None, SCALES, 0, None) == EINVAL


def test_gemm_fp4_keeps_its_refusals_and_its_name():
    lib = alg_amd.load_library()
    a = _args(K=128, lda=128, ldb=128)
    assert lib.alg_gemm_fp4(ctypes.byref(a), None) == EINVAL
    msg = lib.alg_last_error().decode()
    assert msg.startswith("alg_gemm_fp4: ") and "q4out" not in msg


# ---- 3. alg_layernorm_modulate_mxfp4 refuses ------------------------------------------------------------------------------
def _ln(x=0x10000, q4=0x20000, q4s=0x30000, w=0x40000, b=0x50000, sc=0x60000, sh=0x70000, mod_bs=4096, batch=2, rows=8, D=512,
        x_bs=8 * 512, seg_split=3):
    return (x, q4, q4s, w, b, sc, sh, mod_bs, batch, rows, D, x_bs, seg_split, 1e-5, None)


@pytest.mark.parametrize("what,call", [
    ("D % 512", _ln(D=768, x_bs=8 * 768)),
    ("D > 8192", _ln(D=8704, x_bs=8 * 8704)),
    ("D <= 0", _ln(D=0)),
    ("misaligned x", _ln(x=0x10008)),
    ("misaligned q4", _ln(q4=0x20002)),
    ("null x", _ln(x=None)),
    ("null q4", _ln(q4=None)),
    ("null q4_scales", _ln(q4s=None)),
    ("scale without shift", _ln(sh=None)),
    ("misaligned weight", _ln(w=0x40008)),
    ("x batch stride % 8", _ln(x_bs=8 * 512 + 4)),
    ("no rows", _ln(rows=0)),
])
def test_layernorm_modulate_mxfp4_refusals_name_the_entry_before_any_launch(what, call):
    lib = alg_amd.load_library()
    assert lib.alg_layernorm_modulate_mxfp4(*call) == EINVAL, what
    assert "alg_layernorm_modulate_mxfp4" in lib.alg_last_error().decode(), what


def test_python_wrappers_validate_before_the_library_is_asked():
    u8 = torch.zeros(4096, dtype=torch.uint8)
    bf = torch.zeros(2, 512, dtype=torch.bfloat16)
    with pytest.raises(_lib.AlgHipError, match="device tensor"):
        _lib.layernorm_modulate_mxfp4(bf, u8, u8, None, None, None, None, 0, 1, 2, 512, 0, 1e-5)
    with pytest.raises(_lib.AlgHipError, match="device tensor"):
        _lib.gemm_fp4(u8, u8, u8, 1, 32, 256, 256, 256, 32, a_scale=u8, b_scale=u8, q_out_scales=u8)


# ---- 4. the switch --------------------------------------------------------------------------------------------------------
def test_fuse_quant_is_still_an_attribute_that_defaults_to_true():
    import inspect
    from alg_amd import CogVideoXTransformer3DModel
    src = inspect.getsource(CogVideoXTransformer3DModel.__init__)
    assert re.search(r"^\s*self\.fuse_quant = True$", src, re.M)
    for fn in (CogVideoXTransformer3DModel.__init__, CogVideoXTransformer3DModel.from_synthetic, CogVideoXTransformer3DModel.from_pretrained):
        assert "fuse_quant" not in inspect.signature(fn).parameters
    ff = inspect.getsource(CogVideoXTransformer3DModel._ff_fp4)
    assert "self.fuse_quant" in ff and "layernorm_modulate_mxfp4" in ff and "q_out_scales" in ff
    assert ff.count('TM("quant4"') == 2                      # the unfused path is still there, launch for launch
