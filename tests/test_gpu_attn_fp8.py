"""alg_flash_attn_d128_fp8 and its producers (alg_amd/csrc/attention128_fp8.hip, the *_fp8 norms of wan.hip / hunyuan.hip).

The reference of every attention case is float64 attention on the DE-QUANTISED operands; the floor is the error of the eager
restatement of the scheme (tests/helpers/attn_fp8_ref.py) on the same operands, and the bound is the unchanged factors of
tests/_parity.py against that floor: 1.5 x global, 4 x per token p99.9, 2 x worst element.  No other tolerance.  The producers
are bit-exact against the bf16 kernel followed by a standalone quantiser."""
import math

import pytest
import torch

from _parity import check_floor
from alg_amd import _lib
from helpers import attn_fp8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
SENT = -77.0
SCALE = 1.0 / math.sqrt(128)


def _operands(N, Sq, Skv, H, seed, kind="gauss", far_first_tile=False):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(N, s, H, 128, generator=g) for s in (Sq, Skv, Skv))
    if kind == "trained_like":            # QK gains near 3 and a bias component shared by all tokens of a head
        gq, gk = (3.0 + 0.3 * torch.randn(H, 128, generator=g) for _ in range(2))
        bq, bk = (0.5 * torch.randn(H, 128, generator=g) for _ in range(2))
        q, k = q * gq + bq, k * gk + bk
        v = v * (1.0 + 0.5 * torch.randn(H, 128, generator=g)) + 0.3 * torch.randn(H, 128, generator=g)
    if far_first_tile:                    # the first 64 keys far below what follows: the running offset has to grow afterwards
        k[:, :64] *= 0.02
        k[:, 64:] *= 2.5
    return q.to(BF).to(DEV), k.to(BF).to(DEV), v.to(BF).to(DEV)


def _quantise_on_gpu(q, k, v, src_permuted=False):
    """The standalone quantisers: Q rows of 128 (alg_quantize_fp8_rows), K per (batch, head), V^T per row in the kernel's order."""
    N, Sq, H, _ = q.shape
    Skv = k.shape[1]
    D = H * 128
    q8 = torch.empty(N, Sq, D, dtype=torch.uint8, device=DEV)
    qs = torch.empty(N, Sq, H, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_rows(q.contiguous(), q8, qs, N * Sq * H, 128)
    k8 = torch.empty(N, Skv, D, dtype=torch.uint8, device=DEV)
    ks = torch.empty(N, H, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_khead(k.contiguous(), k8, ks, N, H, Skv, Skv * D, D, Skv * D, D)
    pad = (Skv + 63) // 64 * 64
    vt = torch.full((N, D, pad), float("nan"), dtype=BF, device=DEV)         # padding columns of the SOURCE: never used
    vt[:, :, :Skv] = v.reshape(N, Skv, D).transpose(1, 2)
    if src_permuted:                                                       # what gemm(..., GEMM_PERMUTE_COLS) writes: index bits 2 <-> 3
        idx = torch.arange(pad, device=DEV)
        swapped = (idx & ~12) | ((idx & 4) << 1) | ((idx & 8) >> 1)
        src = torch.empty_like(vt)
        src[:, :, swapped] = vt
        vt = src
    vt8 = torch.full((N, D, pad), 0x7F, dtype=torch.uint8, device=DEV)       # NaN bytes: every column has to be written
    vs = torch.empty(N, D, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_vt(vt, vt8, vs, N, D, Skv, D * pad, pad, D * pad, pad, src_permuted=src_permuted)
    return q8, qs, k8, ks, vt8, vs


def _floor_inputs(q8, qs, k8, ks, vt8, vs, Skv):
    """e4m3 bytes -> the values the restatement and the float64 reference work on ([N, S, H, 128] fp32) and their scales."""
    N, Sq, D = q8.shape
    H = D // 128
    qv = q8.view(F8).float().view(N, Sq, H, 128)
    kv = k8.view(F8).float().view(N, -1, H, 128)
    pos = torch.tensor([R.vt_position(s) for s in range(Skv)], device=vt8.device)
    vv = vt8.view(F8).float()[:, :, pos].transpose(1, 2).reshape(N, Skv, H, 128)
    return qv, qs, kv, ks, vv, vs.view(N, H, 128)


def _check(name, out, q8, qs, k8, ks, vt8, vs, Skv):
    qv, qs_, kv, ks_, vv, vs_ = _floor_inputs(q8, qs, k8, ks, vt8, vs, Skv)
    ref = R.attention_f64(qv * qs_[..., None], kv * ks_[:, None, :, None], vv * vs_[:, None], SCALE)
    stats = {}
    floor = R.attention_fp8(qv, qs_, kv, ks_, vv, vs_, SCALE, stats)
    e_hip, e_floor = check_floor(name, out, ref, floor)
    print("%s: HIP %.3e, restatement %.3e vs float64 on the de-quantised operands; %d of %d (block, tile) steps exact, largest "
          "value converted %.1f" % (name, e_hip, e_floor, stats["exact"], stats["tiles"], stats["p_max"]))
    return stats


@pytest.mark.parametrize("kind", ["gauss", "trained_like"])
@pytest.mark.parametrize("N,Sq,Skv,H", [(1, 256, 256, 2), (2, 300, 1000, 3), (3, 65, 37, 2), (1, 257, 64, 1), (2, 31, 129, 8),
                                        (1, 512, 4160, 2)])
def test_attention_fp8_vs_float64_on_the_restatement_floor(N, Sq, Skv, H, kind):
    """Sq != Skv, ragged Skv (not a multiple of 64; < 64), tile-edge query counts (255 / 256 / 257 around the 256-query workgroup
    via 256, 257, 300; 31, 65 around the 32-query block), N = 1, 2, 3."""
    q, k, v = _operands(N, Sq, Skv, H, 100 * N + Sq + Skv, kind)
    q8, qs, k8, ks, vt8, vs = _quantise_on_gpu(q, k, v)
    D, pad = H * 128, vt8.shape[2]
    out = torch.full((N, Sq, D), SENT, dtype=BF, device=DEV)
    _lib.flash_attn_d128_fp8(q8, qs, k8, ks, vt8, vs, out, N, H, Sq, Skv, Sq * D, D, Skv * D, D, D * pad, pad, Sq * D, D, SCALE)
    _check("attn_fp8_%s_N%d_Sq%d_Skv%d_H%d" % (kind, N, Sq, Skv, H), out.view(N, Sq, H, 128), q8, qs, k8, ks, vt8, vs, Skv)


@pytest.mark.parametrize("kind", ["gauss", "trained_like"])
def test_attention_fp8_first_tile_far_below_the_later_maximum(kind):
    """Tile 0 sets a low offset, the tiles behind it hold scores far above it: without the rescale the probabilities would leave
    the e4m3 range.  The restatement asserts that no value above 448 reaches the conversion and counts the exact steps."""
    N, Sq, Skv, H = 1, 128, 1024, 2
    q, k, v = _operands(N, Sq, Skv, H, 7, kind, far_first_tile=True)
    q8, qs, k8, ks, vt8, vs = _quantise_on_gpu(q, k, v)
    D, pad = H * 128, vt8.shape[2]
    out = torch.empty(N, Sq, D, dtype=BF, device=DEV)
    _lib.flash_attn_d128_fp8(q8, qs, k8, ks, vt8, vs, out, N, H, Sq, Skv, Sq * D, D, Skv * D, D, D * pad, pad, Sq * D, D, SCALE)
    stats = _check("attn_fp8_far_first_tile_" + kind, out.view(N, Sq, H, 128), q8, qs, k8, ks, vt8, vs, Skv)
    blocks = N * H * (Sq // 32)
    assert stats["exact"] > blocks, "the case is meant to take the exact path behind tile 0 too"
    assert stats["p_max"] <= 448.0


def test_attention_fp8_strides_offsets_and_nothing_written_outside():
    """HunyuanVideo's layout: Q | K halves of one [J, 2 D] buffer (byte offsets), the output in the first D columns of rows of D + M
    (`am`), one launch per sample at its own key count; guard bands around and between the rows stay as they were."""
    N, J, H, M = 2, 333, 2, 384
    D = H * 128
    AM = D + M
    q, k, v = _operands(N, J, J, H, 11, "trained_like")
    q8, qs, k8, ks, vt8, vs = _quantise_on_gpu(q, k, v, src_permuted=True)
    pad = vt8.shape[2]
    qk8 = torch.cat([q8, k8], dim=2).contiguous()                          # [N, J, 2 D]
    lead, tail = 96, 160
    buf = torch.full((lead + N * J * AM + tail,), SENT, dtype=BF, device=DEV)
    valid = [J, J - 71]
    for b in range(N):
        _lib.flash_attn_d128_fp8(qk8, qs, qk8, ks, vt8, vs, buf, 1, H, J, valid[b], J * 2 * D, 2 * D, J * 2 * D, 2 * D, D * pad, pad,
                                 J * AM, AM, SCALE, q_off=b * J * 2 * D, qs_off=b * J * H, k_off=b * J * 2 * D + D, ks_off=b * H,
                                 vt_off=b * D * pad, vts_off=b * D, o_off=lead + b * J * AM)
    torch.cuda.synchronize()
    assert bool((buf[:lead] == SENT).all()) and bool((buf[lead + N * J * AM:] == SENT).all())
    am = buf[lead:lead + N * J * AM].view(N, J, AM)
    assert bool((am[:, :, D:] == SENT).all()), "written outside the attention columns of am"
    for b in range(N):
        Skv = valid[b]
        sl = slice(b, b + 1)
        _check("attn_fp8_am_stride_sample%d" % b, am[sl, :, :D].reshape(1, J, H, 128), q8[sl], qs[sl], k8[sl, :Skv], ks[sl],
               vt8[sl], vs[sl], Skv)


def test_attention_fp8_refuses_causal_grouped_and_misaligned_before_any_launch():
    N, S, H = 1, 64, 2
    D = H * 128
    q, k, v = _operands(N, S, S, H, 3)
    q8, qs, k8, ks, vt8, vs = _quantise_on_gpu(q, k, v)
    out = torch.full((N, S, D), SENT, dtype=BF, device=DEV)
    args = (q8, qs, k8, ks, vt8, vs, out, N, H, S, S, S * D, D, S * D, D, D * 64, 64, S * D, D, SCALE)
    with pytest.raises(_lib.AlgHipError, match="causal"):
        _lib.flash_attn_d128_fp8(*args, causal=True)
    with pytest.raises(_lib.AlgHipError, match="kv_group"):
        _lib.flash_attn_d128_fp8(*args, kv_group=2)
    with pytest.raises(_lib.AlgHipError, match="aligned"):
        _lib.flash_attn_d128_fp8(*args, q_off=8)
    with pytest.raises(_lib.AlgHipError, match="e4m3 bytes"):
        _lib.flash_attn_d128_fp8(q, *args[1:])
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- producers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_permuted", [False, True])
@pytest.mark.parametrize("Skv", [1, 37, 64, 200, 4161])
def test_vt_quantiser_order_scales_and_zero_padding(Skv, src_permuted):
    """alg_quantize_fp8_vt against the restatement: scales amax / 448 per row over the keys < Skv, bytes bit for bit at the
    positions the MFMA layout asks for, padding columns zero, nothing written beyond the row's Skv-rounded-up-to-64 window."""
    N, H = 2, 1
    D = H * 128
    pad = (Skv + 63) // 64 * 64
    g = torch.Generator().manual_seed(Skv)
    v = (torch.randn(N, Skv, H, 128, generator=g) * (1.0 + torch.arange(128) / 16.0)).to(BF).to(DEV)
    v[0, :, 0, 5] = 0                                                       # an all-zero row: scale 1
    x_rs, q_rs = pad + 64, pad + 32                                          # both pitches wider than the window
    src = torch.full((N, D, x_rs), float("nan"), dtype=BF, device=DEV)
    idx = torch.arange(Skv, device=DEV)
    col = ((idx & ~12) | ((idx & 4) << 1) | ((idx & 8) >> 1)) if src_permuted else idx
    src[:, :, col] = v.reshape(N, Skv, D).transpose(1, 2)
    q8 = torch.full((N, D, q_rs), 0xA5, dtype=torch.uint8, device=DEV)
    sc = torch.full((N, D), -3.0, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_vt(src, q8, sc, N, D, Skv, D * x_rs, x_rs, D * q_rs, q_rs, src_permuted=src_permuted)
    v8, vs = R.quantize_vt(v)
    assert torch.equal(sc, vs.view(N, D))
    assert sc[0, 5].item() == 1.0
    want = R.pack_vt(v8, pad).to(F8).view(torch.uint8)
    got = q8[:, :, :pad]
    assert torch.equal(got.view(F8).float(), want.view(F8).float())          # (+0 and -0 compare equal)
    assert bool((q8[:, :, pad:] == 0xA5).all())
    pos = torch.tensor([R.vt_position(s) for s in range(Skv)], device=DEV)
    padding = torch.ones(pad, dtype=torch.bool, device=DEV)
    padding[pos] = False
    assert bool((got[:, :, padding] == 0).all())


def test_khead_quantiser_measured_and_given_scale():
    N, S, H = 2, 301, 3
    D = H * 128
    g = torch.Generator().manual_seed(5)
    kbuf = torch.randn(N, S, 2 * D, generator=g).to(BF).to(DEV)               # the K half of a Q | K buffer
    kbuf[1, :, D:D + 128] = 0                                                # head 0 of sample 1 all zero
    k = kbuf[:, :, D:].reshape(N, S, H, 128)
    k8 = torch.full((N, S, D + 16), 0xA5, dtype=torch.uint8, device=DEV)
    ks = torch.full((N, H), -3.0, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_khead(kbuf, k8, ks, N, H, S, S * 2 * D, 2 * D, S * (D + 16), D + 16, x_off=D)
    r8, rs = R.quantize_khead(k)
    assert torch.equal(ks, rs) and ks[1, 0].item() == 1.0
    assert torch.equal(k8[:, :, :D].view(F8).float().view(N, S, H, 128), r8)
    assert bool((k8[:, :, D:] == 0xA5).all())
    given = (rs * 0.5).contiguous()                                          # a bound that is too small: saturates, never NaN
    keep = given.clone()
    _lib.quantize_fp8_khead(kbuf, k8, given, N, H, S, S * 2 * D, 2 * D, S * (D + 16), D + 16, x_off=D, scale_given=True)
    assert torch.equal(given, keep)
    r8, _ = R.quantize_khead(k, given)
    assert torch.equal(k8[:, :, :D].view(F8).float().view(N, S, H, 128), r8)
    assert float(r8.abs().max()) == 448.0


@pytest.mark.parametrize("D", [512, 1536, 5120])
def test_rmsnorm_rope_fp8_is_norm_then_quantiser(D):
    """Wan: alg_rmsnorm_rope_fp8 == alg_rmsnorm_rope in place on bf16 + quantiser, bytes and scales bit for bit, for the Q form
    (a scale per token and head: alg_quantize_fp8_rows on rows of 128) and the K form (given scales per (batch, head):
    alg_quantize_fp8_khead with scale_given), with and without RoPE, on the Q | K buffer of the block."""
    N, S, H, eps = 2, 203, D // 128, 1e-6
    g = torch.Generator().manual_seed(D)
    qk = (torch.randn(N, S, 2 * D, generator=g) * 1.7).to(BF).to(DEV)
    qk[1, 7, :D] = 0                                                         # a zero token
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).to(BF).to(DEV)
    cos, sin = (torch.rand(S, 64, generator=g) * 2 - 1).to(DEV), (torch.rand(S, 64, generator=g) * 2 - 1).to(DEV)
    hs = (0.02 + 0.05 * torch.rand(N, H, generator=g)).to(DEV)
    for rope in (True, False):
        cs = (cos, sin) if rope else (None, None)
        for half, x_off in (("q", 0), ("k", D)):
            normed = qk.clone()
            _lib.rmsnorm_rope_(normed, w, cs[0], cs[1], 2 * D, N, S, D, eps, x_off=x_off)
            y = normed[:, :, x_off:x_off + D].contiguous()
            ref8 = torch.empty(N, S, D, dtype=torch.uint8, device=DEV)
            got8 = torch.full((N, S, 2 * D), 0xA5, dtype=torch.uint8, device=DEV)
            before = qk.clone()
            if half == "q":
                ref_s = torch.empty(N, S, H, dtype=torch.float32, device=DEV)
                _lib.quantize_fp8_rows(y, ref8, ref_s, N * S * H, 128)
                got_s = torch.full((N, S, H), -3.0, dtype=torch.float32, device=DEV)
                _lib.rmsnorm_rope_fp8(qk, w, cs[0], cs[1], 2 * D, N, S, D, eps, got8, 2 * D, scale=got_s, x_off=x_off, q8_off=x_off)
                assert torch.equal(got_s, ref_s), (rope, half)
            else:
                _lib.quantize_fp8_khead(y, ref8, hs, N, H, S, S * D, D, S * D, D, scale_given=True)
                _lib.rmsnorm_rope_fp8(qk, w, cs[0], cs[1], 2 * D, N, S, D, eps, got8, 2 * D, head_scale=hs, x_off=x_off, q8_off=x_off)
            assert torch.equal(qk, before), "x is only read"
            assert torch.equal(got8[:, :, x_off:x_off + D], ref8), (rope, half)
            other = got8[:, :, D:] if half == "q" else got8[:, :, :D]
            assert bool((other == 0xA5).all())


@pytest.mark.parametrize("rope_tokens", [0, 150, 229])
def test_headnorm_rope_fp8_is_norm_then_quantiser(rope_tokens):
    """HunyuanVideo: the same statement for alg_headnorm_rope_fp8 -- per-head RMSNorm, RoPE on the first rope_tokens tokens of a
    sample only (0: the prompt rows' form), batch strides, scales at a batch stride of their own."""
    N, J, H, eps = 2, 229, 3, 1e-6
    D = H * 128
    g = torch.Generator().manual_seed(rope_tokens)
    lead = 3                                                                 # rows in front: the call starts at a row offset
    qk = (torch.randn(N, lead + J, 2 * D, generator=g) * 1.3).to(BF).to(DEV)
    w = (1.0 + 0.3 * torch.randn(128, generator=g)).to(BF).to(DEV)
    cos, sin = (torch.rand(J, 128, generator=g) * 2 - 1).to(DEV), (torch.rand(J, 128, generator=g) * 2 - 1).to(DEV)
    hs = (0.02 + 0.05 * torch.rand(N, H, generator=g)).to(DEV)
    bs = (lead + J) * 2 * D
    for half, col in (("q", 0), ("k", D)):
        x_off = lead * 2 * D + col
        normed = qk.clone()
        _lib.headnorm_rope_(normed, w, cos, sin, 2 * D, bs, N, J, H, rope_tokens, eps, x_off=x_off)
        y = normed[:, lead:, col:col + D].contiguous()
        ref8 = torch.empty(N, J, D, dtype=torch.uint8, device=DEV)
        got8 = torch.full((N, lead + J, 2 * D), 0xA5, dtype=torch.uint8, device=DEV)
        before = qk.clone()
        if half == "q":
            ref_s = torch.empty(N, J, H, dtype=torch.float32, device=DEV)
            _lib.quantize_fp8_rows(y, ref8, ref_s, N * J * H, 128)
            got_s = torch.full((N, lead + J, H), -3.0, dtype=torch.float32, device=DEV)
            _lib.headnorm_rope_fp8(qk, w, cos, sin, 2 * D, bs, N, J, H, rope_tokens, eps, got8, 2 * D, bs, scale=got_s,
                                   scale_bstride=(lead + J) * H, x_off=x_off, q8_off=x_off, scale_off=lead * H)
            assert torch.equal(got_s[:, lead:], ref_s) and bool((got_s[:, :lead] == -3.0).all())
        else:
            _lib.quantize_fp8_khead(y, ref8, hs, N, H, J, J * D, D, J * D, D, scale_given=True)
            _lib.headnorm_rope_fp8(qk, w, cos, sin, 2 * D, bs, N, J, H, rope_tokens, eps, got8, 2 * D, bs, head_scale=hs,
                                   x_off=x_off, q8_off=x_off)
        assert torch.equal(qk, before), "x is only read"
        assert torch.equal(got8[:, lead:, col:col + D], ref8), half
        got8[:, lead:, col:col + D] = 0xA5
        assert bool((got8 == 0xA5).all())
