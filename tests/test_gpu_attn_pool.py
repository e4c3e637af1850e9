"""The pooled far field on the GPU (attn_pool.hip, alg_amd/attn_pool.py).

  pool kernels      exact small-integer data (every mean is a bf16 number): bit-exact against torch, head_dim 64 and 128, G = 2, 4
                    and 8, the permuted V^T layout, strided and offset operands inside poisoned guards, zero padding up to the next
                    multiple of 64, keys behind the last whole group left out, argument errors before any launch
  merge             shift 0 is alg_attn_merge_lse's bits; shift log2 G within ONE bf16 step of bf16(float64 merge), lse_out inside
                    LSE_FACTOR x torch fp32's own error (the existing merge test's bounds); a far LSE of -inf keeps the near bits
  composite         pool + near + pooled far + merge through AttnPoolPass against the float64 reference OF THE SAME OPERATOR
                    (helpers/attn_pool_ref.py), held to the project's bound for multi-range tables: max < 3e-2, mean < 2e-3
                    (docs/numerics.md).  9 frames x 384 tokens (and x 380: a latent length that is no multiple of 64 G), window 1,
                    10 prompt tokens in front for d = 64, 13 prompt keys and 20 prompt rows behind for d = 128: every shape has a
                    block with far keys and a block without, and both are asserted
  against dense     on the trained-like operands of helpers/attn_pool_ref.py the error against the dense float64 attention is
                    strictly below the window-only launch's (tests/test_attn_pool_cpu.py establishes it in float64 first)
  graph capture     a capture made after one eager forward replays the eager bits"""
import math

import pytest
import torch

import test_gpu_attn_ranges as R128
import test_gpu_attn_ranges_d64 as R64
from alg_amd import _lib
from alg_amd.attn_pool import AttnPool, AttnPoolPass
from alg_amd.attn_window import KV_ALIGN, SelfAttnOperands, _block_ranges
from helpers import attn_pool_ref as R
from helpers.attn_far_ref import merge_ref
from test_gpu_attn_ranges_heads_d64 import LSE_FACTOR
from test_gpu_lora_merge import one_bf16_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 7.0
NINF = float("-inf")


def bits(t):
    return t.view(torch.int16)


# ---- the pool kernels ------------------------------------------------------------------------------------------------------------
B, H, S = 2, 3, 333            # G = 2: 166 pooled keys (192 padded), one key left over; G = 8: 41 (64 padded), 5 left over


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(BF)      # a sum of 8 stays below 2^7 steps of 1 / 8: every mean is exact


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_pool_k_is_bit_exact_on_strided_offset_operands_and_leaves_the_guards(hd, G):
    row = H * hd
    P, P_pad = S // G, -(-(S // G) // 64) * 64
    k = _ints((B, S, row), 100 + hd + G)
    k[:, 8 * G:9 * G, ::3] = -0.0                                             # a group of -0.0 pools to -0.0 (the sum starts from its first key)
    # the K half of a Q|K buffer: row stride 2 row + 16, offset row + 24 (a multiple of 8), a padded batch stride
    s_rs, s_off = 2 * row + 16, row + 24
    s_bs = S * s_rs + 40
    src = torch.full((s_off + B * s_bs + 64,), float("nan"), dtype=BF, device=DEV)
    torch.as_strided(src, (B, S, row), (s_bs, s_rs, 1), s_off).copy_(k)
    d_rs, d_off = row + 8, 16
    d_bs = P_pad * d_rs + 24
    dst = torch.full((d_off + B * d_bs + 64,), GUARD, dtype=BF, device=DEV)
    src0 = src.clone()
    _lib.attn_pool_k(src, dst, B, H, hd, S, G, s_bs, s_rs, d_bs, d_rs, src_off=s_off, dst_off=d_off)
    want = torch.zeros(B, P_pad, row, dtype=BF)
    want[:, :P] = R.pool_ref(k, G, 1)
    assert torch.equal(want[:, :P].float(), k[:, :P * G].float().reshape(B, P, G, row).mean(dim=2))      # (exact data: torch's own mean)
    got = torch.as_strided(dst, (B, P_pad, row), (d_bs, d_rs, 1), d_off)
    assert torch.equal(bits(got.cpu()), bits(want))
    inside = torch.zeros_like(dst, dtype=torch.bool)
    torch.as_strided(inside, (B, P_pad, row), (d_bs, d_rs, 1), d_off).fill_(True)
    assert bool((dst[~inside] == GUARD).all()) and torch.equal(bits(src), bits(src0))


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_pool_vt_is_bit_exact_in_the_permuted_layout_and_leaves_the_guards(hd, G):
    row = H * hd
    P, P_pad, S_pad = S // G, -(-(S // G) // 64) * 64, -(-S // 64) * 64
    v = _ints((B, S, row), 200 + hd + G)
    v[:, 8 * G:9 * G, ::3] = -0.0                                             # a group of -0.0 pools to -0.0, as in K and in torch
    assert bool((bits(R.pool_ref(v, G, 1))[:, 8, ::3] == -32768).all())
    vt = R128.make_vt(v.to(DEV), S_pad)                                       # [B, row, S_pad], index bits 2 and 3 swapped
    vt[:, :, R128._perm(S_pad)[S:]] = float("nan")                            # the source's padding keys: read, never used
    s_rs, s_off = S_pad + 24, 8
    s_bs = row * s_rs + 16
    src = torch.full((s_off + B * s_bs + 64,), float("nan"), dtype=BF, device=DEV)
    torch.as_strided(src, (B, row, S_pad), (s_bs, s_rs, 1), s_off).copy_(vt)
    d_rs, d_off = P_pad + 40, 24
    d_bs = row * d_rs + 8
    dst = torch.full((d_off + B * d_bs + 64,), GUARD, dtype=BF, device=DEV)
    src0 = src.clone()
    _lib.attn_pool_vt(src, dst, B, H, hd, S, G, s_bs, s_rs, d_bs, d_rs, src_off=s_off, dst_off=d_off)
    want = R128.make_vt(R.pool_ref(v, G, 1).to(DEV), P_pad)                   # zero padded, permuted
    got = torch.as_strided(dst, (B, row, P_pad), (d_bs, d_rs, 1), d_off)
    assert torch.equal(bits(got), bits(want))
    inside = torch.zeros_like(dst, dtype=torch.bool)
    torch.as_strided(inside, (B, row, P_pad), (d_bs, d_rs, 1), d_off).fill_(True)
    assert bool((dst[~inside] == GUARD).all()) and torch.equal(bits(src), bits(src0))


def test_pool_on_random_data_is_the_fp32_mean_rounded_once_and_run_to_run_identical():
    g = torch.Generator().manual_seed(9)
    hd, G, S_ = 128, 4, 4 * 64 * 5 + 3
    row = 2 * hd
    k = (torch.randn(1, S_, row, generator=g) * 3.0).to(BF)
    P_pad = -(-(S_ // G) // 64) * 64
    outs = []
    for _ in range(2):
        dst = torch.full((1, P_pad, row), GUARD, dtype=BF, device=DEV)
        _lib.attn_pool_k(k.to(DEV), dst, 1, 2, hd, S_, G, S_ * row, row, P_pad * row, row)
        outs.append(dst)
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    assert torch.equal(bits(outs[0][:, :S_ // G].cpu()), bits(R.pool_ref(k, G, 1))) and bool((outs[0][:, S_ // G:] == 0).all())
    s_pad = -(-S_ // 64) * 64
    vt = R128.make_vt(k.to(DEV), s_pad)
    dst = torch.full((1, row, P_pad), GUARD, dtype=BF, device=DEV)
    _lib.attn_pool_vt(vt, dst, 1, 2, hd, S_, G, row * s_pad, s_pad, row * P_pad, P_pad)
    assert torch.equal(bits(dst), bits(R128.make_vt(R.pool_ref(k, G, 1).to(DEV), P_pad)))


def test_the_pool_wrappers_refuse_what_the_kernels_would_touch_out_of_bounds():
    hd, G = 64, 2
    row, P_pad, S_pad = H * hd, 192, 384
    k = torch.zeros(B * S * row, dtype=BF, device=DEV)
    kp = torch.zeros(B * P_pad * row, dtype=BF, device=DEV)
    ok = dict(batch=B, heads=H, head_dim=hd, S=S, group=G, src_bs=S * row, src_rs=row, dst_bs=P_pad * row, dst_rs=row)
    _lib.attn_pool_k(k, kp, **ok)
    for bad, match in ((dict(src_rs=row + 8), "does not hold"), (dict(dst_off=8), "does not hold"), (dict(dst_rs=row - 8), "row stride"),
                       (dict(src_rs=row + 4), "multiples of 8"), (dict(group=3), "group=3"), (dict(head_dim=96), "head_dim=96"),
                       (dict(S=1), "at least one group"), (dict(batch=0), "positive")):
        with pytest.raises(_lib.AlgHipError, match=match):
            _lib.attn_pool_k(k, kp, **dict(ok, **bad))
    with pytest.raises(_lib.AlgHipError, match="bfloat16"):
        _lib.attn_pool_k(k.float(), kp, **ok)
    vt = torch.zeros(B * row * S_pad, dtype=BF, device=DEV)
    vp = torch.zeros(B * row * P_pad, dtype=BF, device=DEV)
    ok = dict(batch=B, heads=H, head_dim=hd, S=S, group=G, src_bs=row * S_pad, src_rs=S_pad, dst_bs=row * P_pad, dst_rs=P_pad)
    _lib.attn_pool_vt(vt, vp, **ok)
    for bad, match in ((dict(src_rs=S_pad - 64), "row stride"), (dict(dst_rs=P_pad - 64), "row stride"), (dict(dst_rs=P_pad + 8), "does not hold"),
                       (dict(src_off=8), "does not hold")):
        with pytest.raises(_lib.AlgHipError, match=match):
            _lib.attn_pool_vt(vt, vp, **dict(ok, **bad))
    torch.cuda.synchronize()


# ---- the merge with a shift --------------------------------------------------------------------------------------------------------
MB, MH, MSQ = 2, 3, 300


def _merge_case(hd, seed=1):
    g = torch.Generator().manual_seed(seed)
    row = MH * hd
    x, y = (torch.randn(MB, MSQ, row, generator=g).to(BF) for _ in range(2))
    a, f = (torch.randn(MB, MH, MSQ, generator=g) * 3.0 + 7.0 for _ in range(2))
    return x, y, a, f


def _merge(hd, x, y, a, f, shift):
    """shift None: alg_attn_merge_lse; -> (o, lse_out)"""
    row = MH * hd
    o, far, lse_out = x.to(DEV).clone(), y.to(DEV), torch.full((MB, MH, MSQ), float("nan"), device=DEV)
    args = (o, a.to(DEV).contiguous(), far, f.to(DEV).contiguous(), MB, MH, hd, MSQ, MSQ * row, row, MSQ * row, row)
    if shift is None:
        _lib.attn_merge_lse(*args, lse_out=lse_out)
    else:
        _lib.attn_merge_lse_shift(*args, shift, lse_out=lse_out)
    return o, lse_out


@pytest.mark.parametrize("hd", [64, 128])
def test_merge_shift_zero_is_the_existing_entry_and_a_dead_far_side_keeps_the_near_bits(hd):
    x, y, a, f = _merge_case(hd)
    f = f.clone()
    f[:, :, ::7] = NINF
    o0, l0 = _merge(hd, x, y, a, f, None)
    o1, l1 = _merge(hd, x, y, a, f, 0.0)
    assert torch.equal(bits(o0), bits(o1)) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    # a far LSE of -inf stays -inf under any shift: the near bits, and lse_out = the near LSE
    dead = torch.full_like(f, NINF)
    for shift in (1.0, 3.0):
        o, l = _merge(hd, x, y, a, dead, shift)
        assert torch.equal(bits(o.cpu()), bits(x)) and torch.equal(l.cpu(), a)
    o, l = _merge(hd, x, y, a, f, 2.0)
    rows = torch.isinf(f).transpose(1, 2).unsqueeze(-1).expand(MB, MSQ, MH, hd).reshape(MB, MSQ, MH * hd)
    assert torch.equal(o.cpu()[rows], x[rows]) and not torch.equal(o.cpu()[~rows], x[~rows])
    assert bool(torch.isfinite(o.float()).all())


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_merge_shift_log2_g_within_one_bf16_step_of_float64(hd, G):
    x, y, a, f = _merge_case(hd, seed=G)
    shift = math.log2(G)
    o, lse = _merge(hd, x, y, a, f, shift)
    want64, lse64 = merge_ref(x, a, y, f.double() + shift, MH, hd)            # the formula: a far key weighs as G keys
    want, got = want64.to(BF), o.cpu()
    diff = (got.double() - want.double()).abs()
    worst = (diff / one_bf16_step(torch.maximum(got.double().abs(), want.double().abs()))).max().item()
    print("merge shift d%d G=%d: %d of %d elements differ from bf16(ref64), worst %.3f bf16 steps" % (hd, G, int((diff > 0).sum()),
                                                                                                    diff.numel(), worst))
    assert worst <= 1.0, worst
    fs = f + shift
    m = torch.maximum(a, fs)
    f32 = m + torch.log2(torch.exp2(a - m) + torch.exp2(fs - m))
    e_hip, e_torch = (lse.cpu().double() - lse64).abs().max().item(), (f32.double() - lse64).abs().max().item()
    print("merge shift d%d G=%d: max |lse_out - float64| kernel %.3e, torch fp32 %.3e (bound factor %.1f)" % (hd, G, e_hip, e_torch,
                                                                                                          LSE_FACTOR))
    assert e_torch > 0 and e_hip <= LSE_FACTOR * e_torch, (e_hip, e_torch)
    # without the shift the result differs: the shift is applied
    assert not torch.equal(bits(_merge(hd, x, y, a, f, 0.0)[0]), bits(o))


# ---- the composite -----------------------------------------------------------------------------------------------------------------
def _pass(window, G, hd, samples, rows):
    st = AttnPool()
    tables = [st.near_pooled(window, G, hd, DEV)]
    return AttnPoolPass(st, G, tables, samples, rows, -(-(rows // G) // KV_ALIGN) * KV_ALIGN), st


def _direct(name, fn, *a, **k):
    return fn(*a, **k)


def _far_blocks(window, G, hd):
    """(blocks with far keys, blocks without) -- the shape rule: both exist"""
    _, _, far, _ = R.tables(*window, G)
    per_block = _block_ranges(far)
    with_far, without = [j for j, r in enumerate(per_block) if r], [j for j, r in enumerate(per_block) if not r]
    assert with_far and without, (with_far, without)
    return with_far, without


def _block_rows(blocks, Sq):
    rows = torch.zeros(Sq, dtype=torch.bool)
    for j in blocks:
        rows[j * 256:(j + 1) * 256] = True
    return rows


def _check(got, ref, what):
    err = (got.double() - ref).abs()
    print("%s: against the float64 reference of the operator max %.3e mean %.3e" % (what, err.max().item(), err.mean().item()))
    assert bool(torch.isfinite(got.float()).all())
    assert err.max().item() < 3e-2
    assert err.mean().item() < 2e-3


_D64 = {}


def d64_case(hw):
    """operands and the near-only / dense launches of the d = 64 shape, shared by the G cases"""
    if hw not in _D64:
        Hn, S_ = 2, R.PREFIX + R.FRAMES * hw
        q, k, v, vt, s_pad = R64.operands(1, Hn, S_)
        _D64[hw] = (Hn, S_, q, k, v, vt, s_pad)
    return _D64[hw]


def run_d64(q, k, vt, s_pad, Hn, S_, window, G):
    D = Hn * 64
    o = torch.full((1, S_, D), GUARD, dtype=BF, device=DEV)
    ops = SelfAttnOperands(64, q, k, vt, o, 1, Hn, S_, S_, S_ * D, D, S_ * D, D, D * s_pad, s_pad, S_ * D, D, 1.0, q_prescaled=True)
    p, st = _pass(window, G, 64, 1, S_)
    p.attention(_direct, "attn", ops, 0)
    return o, p, st, ops


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("hw", [384, 380])
def test_composite_d64_is_the_operator(hw, G):
    Hn, S_, q, k, v, vt, s_pad = d64_case(hw)
    window, near, far, pooled = R.tables("prefix", hw, G)
    with_far, without = _far_blocks(("prefix", hw), G, 64)
    assert without == [0]                                                        # the block with the prompt rows
    o, p, st, _ = run_d64(q, k, vt, s_pad, Hn, S_, window, G)
    to = lambda m: R.ranges_to_mask(m).to(DEV)
    ref = R.rows_first(R.operator_ref(*(R.heads_first(t, Hn) for t in (q, k, v)), to(near), to(pooled), G, 1.0))
    _check(o, ref, "composite d64 hw=%d G=%d" % (hw, G))
    # the block without a far key: zeros and -inf from the far launch, the near launch's bits after the merge
    none = _block_rows(without, S_)
    assert bool((st.lse_far.view(1, Hn, S_)[:, :, none] == NINF).all()) and bool((st.o_far.view(1, S_, -1)[:, none] == 0).all())
    assert bool(torch.isfinite(st.lse_far.view(1, Hn, S_)[:, :, ~none]).all())
    o_near = torch.full_like(o, GUARD)
    _lib.flash_attn_d64_ranges_heads(q, k, vt, o_near, 1, Hn, S_, S_ * Hn * 64, Hn * 64, Hn * 64 * s_pad, s_pad, S_ * Hn * 64, Hn * 64, near)
    assert torch.equal(bits(o[:, none]), bits(o_near[:, none])) and not torch.equal(bits(o[:, ~none]), bits(o_near[:, ~none]))
    assert st.bytes == st.k.numel() * 2 + st.vt.numel() * 2 + S_ * Hn * 64 * 2 + 2 * Hn * S_ * 4
    assert st.k.numel() == p.P * Hn * 64 and st.vt.numel() == Hn * 64 * s_pad   # (K shares Q's row stride, V^T the pitch of S)


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("hw", [384, 380])
def test_composite_d128_per_sample_layout_is_the_operator(hw, G):
    Hn = 2
    S_ = R.FRAMES * hw
    Skv, Sq = S_ + R.TAIL, S_ + R.TAIL_ROWS
    D = Hn * 128
    q, k, v, vt, s_pad = R128.operands(1, Hn, Sq, Skv)
    window, near, far, pooled = R.tables("tail", hw, G)
    with_far, without = _far_blocks(("tail", hw), G, 128)
    assert without[-1] == (Sq - 1) // 256                                        # the prompt rows
    o = torch.full((1, Sq, D), GUARD, dtype=BF, device=DEV)
    ops = SelfAttnOperands(128, q, k, vt, o, 1, Hn, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, R128.SCALE)
    p, st = _pass(window, G, 128, 1, Sq)
    p.attention(_direct, "attn", ops, 0)
    to = lambda m: R.ranges_to_mask(m).to(DEV)
    ref = R.rows_first(R.operator_ref(*(R.heads_first(t, Hn) for t in (q, k, v)), to(near), to(pooled), G, R128.SCALE * R.LOG2E))
    _check(o, ref, "composite d128 hw=%d G=%d" % (hw, G))
    none = _block_rows(without, Sq)
    assert bool((st.lse_far.view(1, Hn, Sq)[:, :, none] == NINF).all()) and bool((st.o_far.view(1, Sq, -1)[:, none] == 0).all())
    o_near = torch.full_like(o, GUARD)
    _lib.flash_attn_d128_ranges_heads(q, k, vt, o_near, 1, Hn, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, R128.SCALE, near)
    assert torch.equal(bits(o[:, none]), bits(o_near[:, none])) and not torch.equal(bits(o[:, ~none]), bits(o_near[:, ~none]))
    P = -(-(Sq // G) // 64) * 64
    assert st.bytes == P * D * 2 + D * P * 2 + Sq * D * 2 + 2 * Hn * Sq * 4     # the documented formula, one sample


def test_composite_d128_batched_launch_group_with_a_sample_offset():
    """Wan's layout: one launch group for the whole batch, and (HunyuanVideo) a group that is sample 1 of a two-sample workspace.
    5 frames x 380 tokens: the window of the block in the middle reaches both ends on the 64 G grid, so it has no far key."""
    Hn, hw, G, frames = 2, 380, 4, 5
    S_ = frames * hw
    D = Hn * 128
    q, k, v, vt, s_pad = R128.operands(2, Hn, S_, S_)
    window = R.frame_window_ranges(frames, hw, R.WINDOW)
    near, far, pooled = R.near_far_pooled(window, G)
    per_block = _block_ranges(far)
    without = [j for j, r in enumerate(per_block) if not r]
    assert without and any(per_block), per_block                                 # the shape rule: a block without far keys, blocks with
    o = torch.full((2, S_, D), GUARD, dtype=BF, device=DEV)
    ops = SelfAttnOperands(128, q, k, vt, o, 2, Hn, S_, S_, S_ * D, D, S_ * D, D, D * s_pad, s_pad, S_ * D, D, R128.SCALE)
    p, st = _pass(window, G, 128, 2, S_)
    p.attention(_direct, "attn", ops, 0)
    to = lambda m: R.ranges_to_mask(m).to(DEV)
    ref = R.rows_first(R.operator_ref(*(R.heads_first(t, Hn) for t in (q, k, v)), to(near), to(pooled), G, R128.SCALE * R.LOG2E))
    _check(o, ref, "composite d128 batched hw=%d G=%d" % (hw, G))
    none = _block_rows(without, S_)
    assert bool((st.lse_far.view(2, Hn, S_)[:, :, none] == NINF).all()) and bool(torch.isfinite(st.lse_far.view(2, Hn, S_)[:, :, ~none]).all())
    # sample 1 alone, as group 0 at sample0 = 1 of the same workspace: the same bits
    o1 = torch.full((2, S_, D), GUARD, dtype=BF, device=DEV)
    one = SelfAttnOperands(*ops._replace(o=o1, batch=1, q_off=S_ * D, k_off=S_ * D, vt_off=D * s_pad, o_off=S_ * D))
    p.attention(_direct, "attn", one, 0, group=0, sample0=1)
    assert torch.equal(bits(o1[1]), bits(o[1])) and bool((o1[0] == GUARD).all())


# ---- against dense, trained-like operands ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4])
def test_on_trained_like_operands_the_pooled_far_field_beats_the_window_alone(G):
    """Latent rows, relative L2 against the dense float64 attention; no margin.  Float64 says window only 0.1163, G = 2 0.0657,
    G = 4 0.0907 (tests/test_attn_pool_cpu.py)."""
    qh, kh, vh = (t.to(DEV) for t in R.trained_like_qkv())
    Hn, S_ = qh.shape[1], qh.shape[2]
    q, k, v = (R.rows_first(t).contiguous() for t in (qh, kh, vh))
    s_pad = -(-S_ // 64) * 64
    vt = R64.make_vt(v, s_pad)
    window = R.window_table("prefix", 384)
    _far_blocks(("prefix", 384), G, 64)
    o_pool = run_d64(q, k, vt, s_pad, Hn, S_, window, G)[0]
    o_win = R64.ranged(q, k, vt, s_pad, 1, Hn, S_, window)
    dense = R.rows_first(R.windowed_ref(qh, kh, vh, torch.ones(S_, S_, dtype=torch.bool, device=DEV), 1.0))[:, 256:]
    e_win, e_pool = R.rel_l2(o_win[:, 256:], dense), R.rel_l2(o_pool[:, 256:], dense)
    print("trained-like, kernels: window only %.4f, pooled G = %d %.4f" % (e_win, G, e_pool))
    assert e_pool < e_win, (e_pool, e_win)


# ---- graph capture -----------------------------------------------------------------------------------------------------------------
def test_a_capture_after_one_eager_forward_replays_the_eager_bits():
    Hn, S_, q, k, v, vt, s_pad = d64_case(380)
    window = R.window_table("prefix", 380)
    o, p, st, ops = run_d64(q, k, vt, s_pad, Hn, S_, window, 2)                 # eager: the tables and the workspace exist
    eager = o.clone()
    held = (st.k.data_ptr(), st.o_far.data_ptr())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        p.attention(_direct, "attn", ops, 1)
    o.fill_(GUARD)
    st.o_far.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(o), bits(eager)) and held == (st.k.data_ptr(), st.o_far.data_ptr())
