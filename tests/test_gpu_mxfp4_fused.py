"""MXFP4 operands written where they are computed: alg_layernorm_modulate_mxfp4 (norm2 -> q4), alg_gemm_fp4_q4out (ff1's epilogue ->
q4h) and the three-launch feed-forward of CogVideoXTransformer3DModel(fp4=True) under fuse_quant.

The contract of both entries is "the bits of the unfused pair", so every comparison is torch.equal on the packed bytes and on the
scale bytes, against (a) the unfused HIP pair and (b) the host emulation (tests/_mxfp4.py) applied to the bf16 tensor the unfused
first launch wrote -- (b) keeps the test from comparing the code with itself.  Output buffers carry guard rows / pad columns
filled with a pattern: nothing outside the result may be written."""
import pytest
import torch

from _mxfp4 import pack, quantize, special_blocks
from alg_amd import CogVideoXTransformer3DModel, CogVideoXTransformerConfig, _lib
from oracle import dit_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U8 = torch.uint8
EPS = 1e-5
FILL_Q, FILL_S = 0xA5, 0xFF

SMALL = dict(num_attention_heads=8, attention_head_dim=64, in_channels=16, out_channels=8, num_layers=2,
             time_embed_dim=64, text_embed_dim=128, max_text_seq_length=10, sample_width=12, sample_height=8,
             sample_frames=9, patch_size=2)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _hip_quantize(x, rows, K):
    q = torch.full((rows, K // 2), FILL_Q, dtype=U8, device=DEV)
    s = torch.full((rows, K // 32), FILL_S, dtype=U8, device=DEV)
    _lib.quantize_mxfp4_rows(x, q, s, rows, K)
    return q, s


def _same_bits(q, s, y, rows, K):
    """q / s (device) against (a) the HIP quantiser and (b) the emulation, both on the bf16 tensor y [rows, K] (device)."""
    q_hip, s_hip = _hip_quantize(y, rows, K)
    assert torch.equal(s, s_hip) and torch.equal(q, q_hip)
    codes, scales = quantize(y.cpu())
    assert torch.equal(s.cpu(), scales) and torch.equal(q.cpu(), pack(codes))
    assert not bool((s == 0xFF).any())


# ---- 1. norm2 -> q4 ---------------------------------------------------------------------------------------------------------
def _norm_pair(D, batch, rows, seg_split, affine, modulated, seed, pad=3, zero_span=None):
    """One call of the bf16 norm and one of the MXFP4 twin on the same operands: x rows inside a longer batch item (x_bstride >
    rows * D), two modulation vectors per sample behind 8 unused columns.  Returns (y, q4, q4s, guard rows)."""
    n = batch * rows
    x = (_rand((batch, rows + pad, D), seed, 2.0).float() + _rand((batch, rows + pad, 1), seed + 1, 0.5).float()).to(BF).to(DEV)
    w, b = (1.0 + _rand((D,), seed + 2, 0.3).float()).to(BF), _rand((D,), seed + 3, 0.2)
    mod_cols = 8 + 4 * D                                    # per sample: 8 unused | shift[2][D] | scale[2][D]
    mod = _rand((batch, mod_cols), seed + 4, 0.5)
    if zero_span is not None:
        c0, c1 = zero_span
        w[c0:c1] = 0
        b[c0:c1] = 0
        mod.view(batch, -1)[:, 8 + c0:8 + c1] = 0
        mod.view(batch, -1)[:, 8 + D + c0:8 + D + c1] = 0
    w, b = (w.to(DEV), b.to(DEV)) if affine else (None, None)
    sc = mod.to(DEV) if modulated else None
    kw = dict(x_bstride=(rows + pad) * D, scale_off=8 + 2 * D, shift_off=8)
    y = torch.full((n, D), float("nan"), dtype=BF, device=DEV)
    _lib.layernorm_modulate(x, y, w, b, sc, sc, mod_cols, batch, rows, D, seg_split, EPS, **kw)
    q4 = torch.full((n + 1, D // 2), FILL_Q, dtype=U8, device=DEV)
    q4s = torch.full((n + 1, D // 32), FILL_S, dtype=U8, device=DEV)
    _lib.layernorm_modulate_mxfp4(x, q4, q4s, w, b, sc, sc, mod_cols, batch, rows, D, seg_split, EPS, **kw)
    assert bool((q4[n] == FILL_Q).all()) and bool((q4s[n] == FILL_S).all())       # nothing behind the last row
    assert bool(torch.isfinite(y.float()).all())
    return y, q4[:n], q4s[:n]


@pytest.mark.parametrize("affine,modulated", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("D", [512, 1536, 3072, 8192])
def test_norm_writes_the_bits_of_norm_then_quantiser(D, affine, modulated):
    """batch 2 x 37 rows (no multiple of the four rows of a workgroup), the segment boundary at row 10."""
    y, q4, q4s = _norm_pair(D, 2, 37, 10, affine, modulated, 1000 + D)
    _same_bits(q4, q4s, y, 2 * 37, D)


def test_norm_against_the_many_rows_kernel():
    """2 x 2,050 rows at D = 512 with all four parameter rows: the bf16 side runs ln_mod_rows_kernel (from 4,096 rows), the
    MXFP4 twin its one row per wave."""
    y, q4, q4s = _norm_pair(512, 2, 2050, 226, True, True, 77)
    _same_bits(q4, q4s, y, 2 * 2050, 512)


def test_norm_all_zero_blocks_write_scale_127():
    """Zero weight, bias and shift over channels 96 .. 159: the blocks 3 and 4 of every row are all zero (of either sign)."""
    D = 512
    y, q4, q4s = _norm_pair(D, 2, 37, 10, True, True, 5, zero_span=(96, 160))
    assert bool((y[:, 96:160].float() == 0).all()) and bool((y[:, :96].float() != 0).any())
    _same_bits(q4, q4s, y, 2 * 37, D)
    assert bool((q4s[:, 3:5] == 127).all()) and bool(((q4[:, 48:80] & 0x77) == 0).all())
    assert bool((q4s[:, :3] != 127).any())


# ---- 2. ff1's epilogue -> q4h -----------------------------------------------------------------------------------------------
def _operands(rows_a, N, K, seed):
    a, w = _rand((rows_a, K), seed, 2.0), _rand((N, K), seed + 1, 0.05)
    qa, sa = _hip_quantize(a.to(DEV), rows_a, K)
    qw, sw = _hip_quantize(w.to(DEV), N, K)
    return qa, sa, qw, sw


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("act", [_lib.ACT_NONE, _lib.ACT_GELU_TANH])
@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("N", [32, 288])
def test_gemm_q4out_writes_the_bits_of_gemm_then_quantiser(N, K, act, with_bias):
    """M = 300: three row tiles, the last with 44 rows.  N = 288: three column tiles, the last with one valid block; N = 32: one."""
    M = 300
    qa, sa, qw, sw = _operands(M, N, K, 200 + N + K)
    bias = _rand((N,), 9, 0.5).to(DEV) if with_bias else None
    c = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    _lib.gemm_fp4(qa, qw, c, M, N, K, K, K, N, a_scale=sa, b_scale=sw, bias=bias, act=act)
    cq = torch.full((M + 1, N // 2), FILL_Q, dtype=U8, device=DEV)
    cs = torch.full((M + 1, N // 32), FILL_S, dtype=U8, device=DEV)
    _lib.gemm_fp4(qa, qw, cq, M, N, K, K, K, N, a_scale=sa, b_scale=sw, bias=bias, act=act, q_out_scales=cs)
    assert bool((cq[M] == FILL_Q).all()) and bool((cs[M] == FILL_S).all())         # edge rows are guarded
    assert bool(torch.isfinite(c.float()).all()) and float(c.float().abs().max()) > 0.5
    _same_bits(cq[:M], cs[:M], c, M, N)


@pytest.mark.parametrize("act", [_lib.ACT_NONE, _lib.ACT_GELU_TANH])
def test_gemm_q4out_batched_with_padded_strides(act):
    """batch 2: A rows at lda > K inside longer items, C rows at ldc > N inside longer items, the scales of an item behind a
    padded batch stride.  Pad columns, pad rows and pad scale bytes keep their fill."""
    B, M, N, K = 2, 300, 288, 256
    lda, ldc, Ma, Mc = K + 64, N + 64, M + 3, M + 2
    s_bs = M * (N // 32) + 4                                # 2,704 bytes: a multiple of 8 above the 2,700 an item needs
    qa, sa, qw, sw = _operands(B * Ma, N, K, 300)
    qa_p = torch.zeros(B, Ma, lda // 2, dtype=U8, device=DEV)
    qa_p[:, :, :K // 2] = qa.view(B, Ma, K // 2)
    bias = _rand((N,), 10, 0.5).to(DEV)
    kw = dict(a_scale=sa, b_scale=sw, bias=bias, act=act, batch=B, strideA=Ma * lda, strideAScale=Ma * (K // 32))
    c = torch.full((B, M, N), float("nan"), dtype=BF, device=DEV)
    _lib.gemm_fp4(qa_p, qw, c, M, N, K, lda, K, N, strideC=M * N, **kw)
    cq = torch.full((B, Mc, ldc // 2), FILL_Q, dtype=U8, device=DEV)
    cs = torch.full((B, s_bs), FILL_S, dtype=U8, device=DEV)
    _lib.gemm_fp4(qa_p, qw, cq, M, N, K, lda, K, ldc, strideC=Mc * ldc, q_out_scales=cs, strideOutScales=s_bs, **kw)
    assert bool((cq[:, M:] == FILL_Q).all()) and bool((cq[:, :, N // 2:] == FILL_Q).all()) and bool((cs[:, M * (N // 32):] == FILL_S).all())
    q = cq[:, :M, :N // 2].reshape(B * M, N // 2)
    s = cs[:, :M * (N // 32)].reshape(B * M, N // 32)
    _same_bits(q, s, c.view(B * M, N), B * M, N)


def test_gemm_q4out_special_blocks_reach_the_epilogue_quantiser_exactly():
    """tests/_mxfp4.special_blocks() as GEMM OUTPUTS: ties at every boundary (both signs), saturation, a zero block, negative
    zeros, a power-of-two amax.  Every special value is an integer < 256 times a power of two 2^e of its row, so A carries its
    eight bits in eight K blocks (block j: +-1 or 0 at scale 2^(e + 7 - j)) and the weight adds them up unchanged: B[n, 32 j + n]
    = 1.  A ninth block makes the negative zeros, which no sum that starts at +0 yields: -2^-128 in A times 2^-20 in B is
    -2^-148, which the bf16 rounding of the epilogue turns into -0.  All sums are exact in fp32."""
    sp, _ = special_blocks()
    R, N, K = sp.shape[0], 32, 512
    ca = torch.zeros(R, K, dtype=U8)
    sa = torch.full((R, K // 32), 127, dtype=U8)
    for r in range(R):
        amax = float(sp[r].abs().max())
        e = (torch.frexp(torch.tensor(amax))[1].item() - 1 - 7) if amax > 0 else 0
        ints = sp[r].double() * 2.0 ** -e
        assert torch.equal(ints, ints.round()) and float(ints.abs().max()) < 256
        mag, neg = ints.abs().long(), torch.signbit(sp[r])
        for j in range(8):
            bit = (mag >> (7 - j)) & 1
            ca[r, 32 * j:32 * j + 32] = (2 * bit + 8 * (neg & (bit == 1)).long()).to(U8)       # code 2 = 1.0, bit 3 = sign
            sa[r, j] = 127 + e + 7 - j
        zneg = neg & (mag == 0)
        if bool(zneg.any()):
            ca[r, 256:288] = (9 * zneg.long()).to(U8)                                           # code 9 = -0.5
            sa[r, 8] = 0                                                                        # 2^-127
    cb = torch.zeros(N, K, dtype=U8)
    sb = torch.full((N, K // 32), 127, dtype=U8)
    for j in range(9):
        cb[torch.arange(N), 32 * j + torch.arange(N)] = 2
    sb[:, 8] = 127 - 20
    A, SA, B_, SB = pack(ca).to(DEV), sa.to(DEV), pack(cb).to(DEV), sb.to(DEV)
    c = torch.full((R, N), float("nan"), dtype=BF, device=DEV)
    _lib.gemm_fp4(A, B_, c, R, N, K, K, K, N, a_scale=SA, b_scale=SB)
    assert torch.equal(c.cpu().view(torch.int16), sp.to(BF).view(torch.int16))                 # the blocks arrived, -0 included
    cq = torch.full((R + 1, N // 2), FILL_Q, dtype=U8, device=DEV)
    cs = torch.full((R + 1, N // 32), FILL_S, dtype=U8, device=DEV)
    _lib.gemm_fp4(A, B_, cq, R, N, K, K, K, N, a_scale=SA, b_scale=SB, q_out_scales=cs)
    assert bool((cq[R] == FILL_Q).all()) and bool((cs[R] == FILL_S).all())
    _same_bits(cq[:R], cs[:R], c, R, N)
    codes, scales = quantize(sp.to(BF))
    assert torch.equal(cq[:R].cpu(), pack(codes)) and torch.equal(cs[:R].cpu(), scales)


# ---- 3. the model ------------------------------------------------------------------------------------------------------------
_CASE = {}


def _case():
    if not _CASE:
        ocfg = dit_oracle.DiTConfig(**SMALL)
        w32 = dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)
        g = torch.Generator().manual_seed(1)
        hs = torch.randn(3, 3, 16, 8, 12, generator=g).to(BF)
        ehs = torch.randn(3, 10, 128, generator=g).to(BF)
        _CASE.update(wbf={k: v.to(BF) for k, v in w32.items()},
                     inputs=(hs, ehs, torch.tensor([999] * 3), dit_oracle.rope_tables(ocfg, 64, 96, 3)))
    return _CASE["wbf"], _CASE["inputs"]


def _model(wbf, **kw):
    return CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**SMALL), wbf, device=DEV, **kw)


def _run(model, hs, ehs, ts, rope):
    return model(hs.to(DEV), ehs.to(DEV), ts, image_rotary_emb=rope, return_dict=False)[0]


@pytest.mark.parametrize("fp8", [False, True])
def test_fp4_forward_is_the_same_with_and_without_fusion(fp8):
    wbf, inp = _case()
    model = _model(wbf, fp4=True, fp8=fp8)
    assert model.fuse_quant is True
    fused = _run(model, *inp)
    assert torch.isfinite(fused.float()).all()
    model.fuse_quant = False
    unfused = _run(model, *inp)
    model.fuse_quant = True
    again = _run(model, *inp)
    assert torch.equal(fused, unfused) and torch.equal(fused, again)
    # a bf16 model flipped to fp4 (and fp8) quantises its weights on the first such forward: the same result under fusion
    flip = _model(wbf)
    flip.fp4, flip.fp8 = True, fp8
    assert flip.fuse_quant is True and torch.equal(_run(flip, *inp), fused)


def test_fused_forward_launches_no_quantiser_pass():
    """The timing hook: three feed-forward launches per block with fusion (ln_mod also counts norm1), five without."""
    wbf, inp = _case()
    model = _model(wbf, fp4=True)
    layers = len(model.layers)
    model.profile = {}
    fused = _run(model, *inp)
    on = {k: len(v) for k, v in model.profile.items()}
    model.fuse_quant = False
    model.profile = {}
    unfused = _run(model, *inp)
    off = {k: len(v) for k, v in model.profile.items()}
    model.profile = None
    assert "quant4" not in on and off["quant4"] == 2 * layers
    for name in ("ln_mod", "gemm_ff1", "gemm_ff2"):
        assert on[name] == off[name] and on[name] >= layers, name
    assert on["gemm_ff1"] == layers and on["gemm_ff2"] == layers
    assert torch.equal(fused, unfused)
