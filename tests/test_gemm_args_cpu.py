"""The GEMM entries' host path on a machine WITHOUT a GPU: every refusal of the argument check with its exact text, the order of
the checks, and the route a valid call is planned onto.

No operand is ever dereferenced: a refused call returns before any HIP call, and a valid call fails cleanly at its launcher's
first HIP call -- the opt-in to more than 64 KiB of dynamic LDS -- with ALG_ELAUNCH and a message that names the C entry and
the LDS bytes of the kernels it would have launched: alg_gemm_bf16 / 131072 is the 8-wave schedule 6 (bf16 or e4m3),
alg_gemm_bf16 / 163840 an asm-loop schedule (9, 10, 11, 9 e4m3), alg_conv_cl_bf16 / 131072 the convolution form, and
alg_gemm_bf16_pair / alg_gemm_bf16_pair_qk the two-problem launches.  The expected values were recorded from the library
before check, plan and launch were separated (gemm.hip); the file passes unchanged against that library.

With a GPU the file is skipped: a check lost by mistake would launch a kernel on host pointers."""
import ctypes

import pytest
import torch

import alg_amd
from alg_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")

EINVAL, ELAUNCH, ELIMIT = -1, -2, -3
_BUF = ctypes.create_string_buffer(1024)
P = (ctypes.addressof(_BUF) + 255) & ~255          # a 256-byte aligned host address; P + 16 k are "other" operands
A, B, C, BIAS, R, GATE, SA, SB = (P + 64 * i for i in range(8))

SHAPE = "alg_gemm_bf16: bad shape M=%d N=%d K=%d batch=%d"
ALIGN_AB = "alg_gemm: A/B must be 16-byte aligned with lda/ldb/strides multiples of 16 bytes"
ALIGN_C = "alg_gemm_bf16: C/bias/R/gate must be 8-byte aligned with ldc/ldr/strides multiples of 4 elements"
SCALES = "alg_gemm_fp8: a_scale / b_scale are required (b_scale 16-byte aligned)"
PERM = "alg_gemm_bf16: PERMUTE_COLS cannot be combined with residual/gate"
ACT_RES = "alg_gemm_bf16: an activation cannot be combined with the residual epilogue"
CONV = "alg_gemm_bf16: bad convolution addressing (cin_log2=%d K=%d lda=%d wp=%d hpwp=%d)"
PACKED_FP8 = ("alg_gemm_fp8: a packed B (ALG_GEMM_B_PACKED11) holds bf16 fragments for schedule 11; the e4m3 GEMM reads a "
              "row-major B")
PACKED_CONV = "alg_gemm_bf16: convolution addressing cannot be combined with a packed B (ALG_GEMM_B_PACKED11)"
PACKED = ("alg_gemm_bf16: a packed B (ALG_GEMM_B_PACKED11) needs K >= 128, 32-bit byte offsets inside a 256-row A panel, a B "
          "shared by the batch (strideB = 0) and a plain column layout (no per-row bias / column permutation)")
LIMIT = "alg_gemm_bf16: M*ldc must stay below 2^31 (32-bit epilogue offsets)"
GRID = "alg_gemm_bf16: grid too large"
QK_ARGS = "alg_gemm_bf16_pair_qk: bad LayerNorm / rotary arguments"
QK_ALIGN = "alg_gemm_bf16_pair_qk: pointers must be 16-byte aligned"
QK_PLAIN = ("alg_gemm_bf16_pair_qk: qk must be a plain GEMM onto the contiguous [batch][S][2][heads][64] tensor "
            "(N=%d heads=%d ldc=%d)")
CONV_SHAPE = ("alg_conv_cl_bf16: bad shape frames=%d Hp=%d Wp=%d Cin=%d Cout=%d kt=%d (Cin a power of two >= 64, "
              "Cout %% 4 == 0)")


@pytest.fixture(scope="module")
def lib():
    return alg_amd.load_library()


def g(M=300, N=520, K=128, batch=1, **kw):
    """a valid plain call (contiguous operands) with the fields of kw on top"""
    a = _lib.GemmArgs()
    a.A, a.B, a.C = A, B, C
    a.M, a.N, a.K, a.batch = M, N, K, batch
    a.lda, a.ldb, a.ldc, a.ldr = K, K, N, N
    a.strideA, a.strideB, a.strideC, a.strideR = M * K, 0, M * N, M * N
    a.seg_split = M
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def f8(**kw):
    return g(**{**dict(a_scale=SA, b_scale=SB), **kw})


def conv_args(**kw):
    """the GEMM alg_conv_cl_bf16 builds for frames=2, Hp=8, Wp=8, Cin=64, Cout=64, kt=1, plain mode"""
    return g(**{**dict(M=64, N=64, K=576, batch=2, lda=64, ldb=576, ldc=64, ldr=64, strideA=4096, strideC=4096, strideR=4096,
                       conv_cin_log2=6, conv_wp=8, conv_hpwp=64, conv_kw=3), **kw})


def qk(heads=4, **kw):
    e = _lib.QkNormRopeArgs()
    e.wq, e.bq, e.wk, e.bk = P + 512, P + 528, P + 544, P + 560
    e.heads, e.text_len, e.eps, e.q_scale = heads, 0, 1e-6, 0.125
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def qk_a(heads=4, **kw):
    """the Q|K projection onto the contiguous [1][300][2][heads][64] tensor"""
    return g(**{**dict(N=2 * heads * 64), **kw})


def call(lib, entry, *a):
    fn = getattr(lib, entry)
    rc = fn(*[ctypes.byref(x) if isinstance(x, ctypes.Structure) else x for x in a], None)
    return rc, lib.alg_last_error().decode()


PACKED11, PER_ROW, PERMUTE, GATE_F32 = _lib.GEMM_B_PACKED11, _lib.GEMM_BIAS_PER_ROW, _lib.GEMM_PERMUTE_COLS, _lib.GEMM_GATE_F32
SEG_STRIDE = _lib.GEMM_GATE_SEG_STRIDE
# the tall call of tests/test_gpu_gemm_packed_entries.py (TALL): two slabs at ldc = 16384
TALL = dict(M=140_000, N=512, K=128, ldc=16384, strideC=0)

REFUSALS = [
    # ---- one case per refusal of the check, in the order the check runs them
    ("null struct", "alg_gemm_bf16", (None,), EINVAL, "alg_gemm_bf16: null argument"),
    ("null A", "alg_gemm_bf16", (g(A=None),), EINVAL, "alg_gemm_bf16: null argument"),
    ("null C fp8", "alg_gemm_fp8", (f8(C=None),), EINVAL, "alg_gemm_bf16: null argument"),
    ("M = 0", "alg_gemm_bf16", (g(M=0),), EINVAL, SHAPE % (0, 520, 128, 1)),
    ("batch < 0", "alg_gemm_bf16", (g(batch=-2),), EINVAL, SHAPE % (300, 520, 128, -2)),
    ("K = 96", "alg_gemm_bf16", (g(K=96),), EINVAL, "alg_gemm_bf16: K=96 must be a multiple of 64"),
    ("fp8 K = 192", "alg_gemm_fp8", (f8(K=192),), EINVAL, "alg_gemm_fp8: K=192 must be a multiple of 128"),
    ("lda % 8", "alg_gemm_bf16", (g(lda=132),), EINVAL, ALIGN_AB),
    ("B misaligned", "alg_gemm_bf16", (g(B=B + 8),), EINVAL, ALIGN_AB),
    ("fp8 lda % 16", "alg_gemm_fp8", (f8(lda=136),), EINVAL, ALIGN_AB),
    ("fp8 no a_scale", "alg_gemm_fp8", (f8(a_scale=None),), EINVAL, SCALES),
    ("fp8 b_scale misaligned", "alg_gemm_fp8", (f8(b_scale=SB + 4),), EINVAL, SCALES),
    ("act = 3", "alg_gemm_bf16", (g(act=3),), EINVAL, "alg_gemm_bf16: unknown activation 3"),
    ("act = -1", "alg_gemm_bf16", (g(act=-1),), EINVAL, "alg_gemm_bf16: unknown activation -1"),
    ("permute + residual", "alg_gemm_bf16", (g(R=R, flags=PERMUTE),), EINVAL, PERM),
    ("activation + residual", "alg_gemm_bf16", (g(R=R, act=_lib.ACT_SILU),), EINVAL, ACT_RES),
    ("gate without residual", "alg_gemm_bf16", (g(gate=GATE),), EINVAL, "alg_gemm_bf16: gate needs a residual"),
    ("ldc % 4", "alg_gemm_bf16", (g(ldc=522),), EINVAL, ALIGN_C),
    ("column bias misaligned", "alg_gemm_bf16", (g(bias=BIAS + 4),), EINVAL, ALIGN_C),
    ("fp32 gate 8-byte aligned", "alg_gemm_bf16", (g(R=R, gate=GATE + 8, flags=GATE_F32),), EINVAL, ALIGN_C),
    # the second gate segment is read with 8- and 16-byte loads at gate + gate_seg_stride + n: the segment stride is a pitch
    ("gate_seg_stride % 4", "alg_gemm_bf16", (g(R=R, gate=GATE, flags=SEG_STRIDE, gate_seg_stride=522),), EINVAL, ALIGN_C),
    ("gate_seg_stride odd, fp32 gate, fp8", "alg_gemm_fp8", (f8(R=R, gate=GATE, flags=SEG_STRIDE | GATE_F32, gate_seg_stride=521),),
     EINVAL, ALIGN_C),
    ("gate_seg_stride % 4, packed", "alg_gemm_bf16", (g(R=R, gate=GATE, flags=SEG_STRIDE | PACKED11, gate_seg_stride=6),), EINVAL,
     ALIGN_C),
    ("conv kw = 5", "alg_gemm_bf16", (conv_args(conv_kw=5),), EINVAL, CONV % (6, 576, 64, 8, 64)),
    ("conv + fp8", "alg_gemm_fp8", (conv_args(K=1152, lda=128, ldb=1152, a_scale=SA, b_scale=SB),), EINVAL,
     CONV % (6, 1152, 128, 8, 64)),
    ("fp8 + packed", "alg_gemm_fp8", (f8(flags=PACKED11),), EINVAL, PACKED_FP8),
    ("conv + packed", "alg_gemm_bf16", (conv_args(flags=PACKED11),), EINVAL, PACKED_CONV),
    ("packed K = 64", "alg_gemm_bf16", (g(K=64, flags=PACKED11),), EINVAL, PACKED),
    ("packed, B per batch item", "alg_gemm_bf16", (g(batch=2, strideB=520 * 128, flags=PACKED11),), EINVAL, PACKED),
    ("packed, A panel past 32 bits", "alg_gemm_bf16", (g(lda=1 << 23, flags=PACKED11),), EINVAL, PACKED),
    ("packed + column permutation", "alg_gemm_bf16", (g(flags=PACKED11 | PERMUTE),), EINVAL, PACKED),
    ("tall packed + per-row bias", "alg_gemm_bf16", (g(bias=BIAS, flags=PACKED11 | PER_ROW, **TALL),), EINVAL, PACKED),
    # ---- the limits behind the check
    ("ldc = 2^31", "alg_gemm_bf16", (g(M=1, ldc=1 << 31, strideC=0),), ELIMIT, LIMIT),
    ("conv taller than 2^31 / ldc", "alg_gemm_bf16", (conv_args(M=1 << 20, ldc=1 << 12),), ELIMIT, LIMIT),
    ("grid", "alg_gemm_bf16", (g(M=257, N=8, ldc=8, batch=(1 << 30) + 1, strideA=0, strideC=0),), ELIMIT, GRID),
    # ---- two faults: the earlier check speaks
    ("null + shape", "alg_gemm_bf16", (g(B=None, M=0),), EINVAL, "alg_gemm_bf16: null argument"),
    ("shape + K", "alg_gemm_bf16", (g(N=0, K=96),), EINVAL, SHAPE % (300, 0, 96, 1)),
    ("K + act", "alg_gemm_bf16", (g(K=96, act=9),), EINVAL, "alg_gemm_bf16: K=96 must be a multiple of 64"),
    ("alignment + act", "alg_gemm_bf16", (g(A=A + 2, act=9),), EINVAL, ALIGN_AB),
    ("fp8 scales + packed", "alg_gemm_fp8", (f8(b_scale=None, flags=PACKED11),), EINVAL, SCALES),
    ("act + permute", "alg_gemm_bf16", (g(act=9, R=R, flags=PERMUTE),), EINVAL, "alg_gemm_bf16: unknown activation 9"),
    ("permute + activation, both with a residual", "alg_gemm_bf16", (g(R=R, act=_lib.ACT_SILU, flags=PERMUTE),), EINVAL, PERM),
    ("gate + C alignment", "alg_gemm_bf16", (g(gate=GATE, C=C + 4),), EINVAL, "alg_gemm_bf16: gate needs a residual"),
    ("C alignment + packed", "alg_gemm_bf16", (g(C=C + 4, K=64, flags=PACKED11),), EINVAL, ALIGN_C),
    ("conv + packed, bad conv", "alg_gemm_bf16", (conv_args(conv_wp=2, flags=PACKED11),), EINVAL, CONV % (6, 576, 64, 2, 64)),
    ("packed + ldc = 2^31", "alg_gemm_bf16", (g(M=1, K=64, ldc=1 << 31, strideC=0, flags=PACKED11),), EINVAL, PACKED),
    # ---- pairs: both problems are checked before anything runs; a's text comes first
    ("pair, b bad", "alg_gemm_bf16_pair", (g(), g(K=96)), EINVAL, "alg_gemm_bf16: K=96 must be a multiple of 64"),
    ("pair, b null", "alg_gemm_bf16_pair", (g(), None), EINVAL, "alg_gemm_bf16: null argument"),
    ("pair, b bad packed", "alg_gemm_bf16_pair", (g(), g(K=64, flags=PACKED11)), EINVAL, PACKED),
    ("pair, both bad", "alg_gemm_bf16_pair", (g(act=7), g(K=96)), EINVAL, "alg_gemm_bf16: unknown activation 7"),
    ("pair, a over the limit, b bad", "alg_gemm_bf16_pair", (g(M=1, ldc=1 << 31, strideC=0), g(K=96)), EINVAL,
     "alg_gemm_bf16: K=96 must be a multiple of 64"),
    ("pair_qk, b bad", "alg_gemm_bf16_pair_qk", (qk_a(), g(M=0), qk(heads=0)), EINVAL, SHAPE % (0, 520, 128, 1)),
    ("pair_qk, no arguments", "alg_gemm_bf16_pair_qk", (qk_a(), g(), None), EINVAL, QK_ARGS),
    ("pair_qk, heads = 0", "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk(heads=0)), EINVAL, QK_ARGS),
    ("pair_qk, cos without sin", "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk(cos_tab=P + 576)), EINVAL, QK_ARGS),
    ("pair_qk, wk misaligned", "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk(wk=P + 548)), EINVAL, QK_ALIGN),
    ("pair_qk, C 8-byte aligned", "alg_gemm_bf16_pair_qk", (qk_a(C=C + 8), g(), qk()), EINVAL, QK_ALIGN),
    ("pair_qk, N != 2 heads 64", "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk(heads=3)), EINVAL, QK_PLAIN % (512, 3, 512)),
    ("pair_qk, ldc != N", "alg_gemm_bf16_pair_qk", (qk_a(ldc=1024), g(), qk()), EINVAL, QK_PLAIN % (512, 4, 1024)),
    ("pair_qk, residual", "alg_gemm_bf16_pair_qk", (qk_a(R=R), g(), qk()), EINVAL, QK_PLAIN % (512, 4, 512)),
    ("pair_qk, misaligned + not plain", "alg_gemm_bf16_pair_qk", (qk_a(ldc=1024), g(), qk(bq=P + 520)), EINVAL, QK_ALIGN),
]


@pytest.mark.parametrize("name,entry,args,rc,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(lib, name, entry, args, rc, text):
    assert call(lib, entry, *args) == (rc, text)


def test_conv_entry_refuses_its_own_shape_errors(lib):
    conv = lambda *geom: (lib.alg_conv_cl_bf16(A, B, None, None, C, *geom, None), lib.alg_last_error().decode())
    assert conv(2, 8, 8, 96, 64, 1, 0) == (EINVAL, CONV_SHAPE % (2, 8, 8, 96, 64, 1))      # Cin no power of two
    assert conv(2, 8, 8, 64, 256, 3, 1) == (EINVAL, CONV_SHAPE % (2, 8, 8, 64, 256, 3))    # two voxels per row: Cout <= 128
    assert conv(2, 8, 8, 64, 64, 3, 2) == (EINVAL, CONV_SHAPE % (2, 8, 8, 64, 64, 3))      # stride 2 is a 2-d convolution


ASM, PP = 163840, 131072      # dynamic LDS of the asm-loop schedules (9, 10, 11, 9 e4m3) and of the 8-wave schedule 6
ROUTES = [
    # (id, ALG_GEMM_PIPE, entry, arguments, entry named by the message, its LDS bytes)
    ("plain", None, "alg_gemm_bf16", (g(),), "alg_gemm_bf16", ASM),
    ("K = 64", None, "alg_gemm_bf16", (g(K=64),), "alg_gemm_bf16", PP),
    ("A panel past 32 bits", None, "alg_gemm_bf16", (g(lda=1 << 23),), "alg_gemm_bf16", PP),
    ("residual + gate", None, "alg_gemm_bf16", (g(R=R, gate=GATE),), "alg_gemm_bf16", ASM),
    ("gelu", None, "alg_gemm_bf16", (g(act=_lib.ACT_GELU_TANH),), "alg_gemm_bf16", ASM),
    ("gate_seg_stride = 0", None, "alg_gemm_bf16", (g(R=R, gate=GATE, flags=SEG_STRIDE, gate_seg_stride=0),), "alg_gemm_bf16", ASM),
    ("gate_seg_stride = N + 4", None, "alg_gemm_bf16", (g(R=R, gate=GATE, flags=SEG_STRIDE, gate_seg_stride=524),), "alg_gemm_bf16", ASM),
    ("gate_seg_stride unused without the flag", None, "alg_gemm_bf16", (g(R=R, gate=GATE, gate_seg_stride=522),), "alg_gemm_bf16", ASM),
    ("gate_seg_stride odd, N % 4 != 0", None, "alg_gemm_bf16", (g(N=250, ldc=250, ldr=250, strideC=75000, strideR=75000, R=R, gate=GATE,
                                                                 flags=SEG_STRIDE, gate_seg_stride=251),), "alg_gemm_bf16", ASM),
    ("packed", None, "alg_gemm_bf16", (g(flags=PACKED11),), "alg_gemm_bf16", ASM),
    ("tall: first slab", None, "alg_gemm_bf16", (g(**TALL),), "alg_gemm_bf16", ASM),
    ("fp8 K = 128", None, "alg_gemm_fp8", (f8(),), "alg_gemm_bf16", PP),
    ("fp8 K = 256", None, "alg_gemm_fp8", (f8(K=256),), "alg_gemm_bf16", ASM),
    ("conv through alg_gemm_bf16", None, "alg_gemm_bf16", (conv_args(),), "alg_conv_cl_bf16", PP),
    ("pair", None, "alg_gemm_bf16_pair", (g(), g(N=264)), "alg_gemm_bf16_pair", ASM),
    ("pair, one residual", None, "alg_gemm_bf16_pair", (g(), g(R=R)), "alg_gemm_bf16", ASM),
    ("pair, a K = 64", None, "alg_gemm_bf16_pair", (g(K=64), g()), "alg_gemm_bf16", PP),
    ("pair, b packed", None, "alg_gemm_bf16_pair", (g(), g(flags=PACKED11)), "alg_gemm_bf16", ASM),
    ("pair_qk fused", None, "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk()), "alg_gemm_bf16_pair_qk", ASM),
    ("pair_qk, heads % 4", None, "alg_gemm_bf16_pair_qk", (qk_a(heads=3), g(), qk(heads=3)), "alg_gemm_bf16_pair", ASM),
    ("pair_qk, per-row bias", None, "alg_gemm_bf16_pair_qk", (qk_a(bias=BIAS, flags=PER_ROW), g(), qk()), "alg_gemm_bf16_pair", ASM),
    ("pair_qk, b packed", None, "alg_gemm_bf16_pair_qk", (qk_a(), g(flags=PACKED11), qk()), "alg_gemm_bf16", ASM),
    ("plain, pipe 9", "9", "alg_gemm_bf16", (g(),), "alg_gemm_bf16", ASM),
    ("pair, pipe 9", "9", "alg_gemm_bf16_pair", (g(), g(N=264)), "alg_gemm_bf16_pair", ASM),
    ("pair one residual, pipe 9", "9", "alg_gemm_bf16_pair", (g(), g(R=R)), "alg_gemm_bf16", ASM),
    ("pair_qk, pipe 9", "9", "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk()), "alg_gemm_bf16_pair_qk", ASM),
    ("plain, pipe 6", "6", "alg_gemm_bf16", (g(),), "alg_gemm_bf16", PP),
    ("packed, pipe 6", "6", "alg_gemm_bf16", (g(flags=PACKED11),), "alg_gemm_bf16", ASM),
    ("fp8 K = 256, pipe 6", "6", "alg_gemm_fp8", (f8(K=256),), "alg_gemm_bf16", PP),
    ("pair, pipe 6", "6", "alg_gemm_bf16_pair", (g(), g(N=264)), "alg_gemm_bf16", PP),
    ("pair one residual, pipe 6", "6", "alg_gemm_bf16_pair", (g(), g(R=R)), "alg_gemm_bf16", PP),
    ("pair_qk, pipe 6", "6", "alg_gemm_bf16_pair_qk", (qk_a(), g(), qk()), "alg_gemm_bf16", PP),
]


@pytest.mark.parametrize("name,pipe,entry,args,named,lds", ROUTES, ids=[r[0] for r in ROUTES])
def test_route(lib, monkeypatch, name, pipe, entry, args, named, lds):
    """a valid call gets as far as its launcher, which names the entry and the LDS bytes of the route"""
    monkeypatch.setenv("ALG_GEMM_PIPE", pipe or "10")   # (conftest: the library re-reads its options, now and when this is undone)
    rc, text = call(lib, entry, *args)
    assert rc == ELAUNCH and text.startswith("%s: hipFuncSetAttribute(%d B LDS): " % (named, lds)), (rc, text)


@pytest.mark.parametrize("mode,lds", [(_lib.CONV_PLAIN, PP), (_lib.CONV_PAIR, PP), (_lib.CONV_STRIDE2, PP)])
def test_conv_entry_route(lib, mode, lds):
    rc = lib.alg_conv_cl_bf16(A, B, BIAS, None, C, 2, 8, 8, 64, 64, 1, mode, None)
    text = lib.alg_last_error().decode()
    assert rc == ELAUNCH and text.startswith("alg_conv_cl_bf16: hipFuncSetAttribute(%d B LDS): " % lds), (rc, text)
