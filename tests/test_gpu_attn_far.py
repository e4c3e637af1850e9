"""alg_attn_merge_lse (attn_far.hip): the merge of two partial attentions over disjoint key sets by their log2-domain log-sum-exps.

  random data       batch 2, heads 3, head_dim 64 and 128, Sq = 300 (ragged against the 256-thread block and the 8-element vector),
                    padded row and batch strides, guard elements around every output: every element within ONE bf16 step of
                    bf16(float64 merge) -- the standard of a once-rounded bf16 result (test_gpu_lora_merge.py) --, lse_out within
                    the LSE tests' LSE_FACTOR x torch fp32's own error on the same operands
  exact cases       torch.equal: a side without mass (lse -inf, or 200 log2 units below the other) leaves the other side's bits
  partition         near launch + far launch + merge over the tables of alg_amd/attn_window.py (grid_aligned, complement_ranges)
                    against fp32 SDPA over all keys, held to the bounds the multi-range tests of the two kernels state
                    (test_gpu_attn_ranges_d64.py: FACTOR x the dense entry's error; test_gpu_attn_ranges.py: max 3e-2, mean 2e-3)"""
import math

import pytest
import torch

import test_gpu_attn_ranges as R128
import test_gpu_attn_ranges_d64 as R64
from _parity import FACTOR, rel
from alg_amd import _lib
from alg_amd.attn_window import _block_ranges, complement_ranges, frame_window_ranges, full_ranges, grid_aligned
from helpers.attn_far_ref import merge_ref
from test_gpu_attn_ranges_heads_d64 import BF16_SUM_TERM, LSE_FACTOR
from test_gpu_lora_merge import one_bf16_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
B, H, SQ = 2, 3, 300
GUARD = 7.0
NINF = float("-inf")


class Case:
    """Operands of one merge on padded strides inside guarded buffers.  o / far: [B][SQ][H * hd] views of flat bf16 buffers whose
    every other element is GUARD; lse, lse_far, lse_out: [B][H][SQ] at offset 5 of flat fp32 buffers."""

    def __init__(self, hd, seed=1):
        self.hd, self.row = hd, H * hd
        self.o_rs, self.far_rs = self.row + 16, self.row + 40
        self.o_bs, self.far_bs = SQ * self.o_rs + 24, SQ * self.far_rs + 8
        self.o_off, self.far_off, self.l_off = 64, 8, 5
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(B, SQ, self.row, generator=g).to(BF)
        self.y = torch.randn(B, SQ, self.row, generator=g).to(BF)
        self.a = torch.randn(B, H, SQ, generator=g) * 3.0 + 7.0
        self.f = torch.randn(B, H, SQ, generator=g) * 3.0 + 7.0

    def view(self, buf, off, bs, rs):
        return torch.as_strided(buf, (B, SQ, self.row), (bs, rs, 1), off)

    def run(self, x=None, y=None, a=None, f=None, with_lse=True):
        """-> (o buffer, its [B][SQ][row] view, lse_out [B][H][SQ] or None): one launch on fresh guarded buffers"""
        x, y = (self.x if x is None else x), (self.y if y is None else y)
        a, f = (self.a if a is None else a), (self.f if f is None else f)
        ob = torch.full((self.o_off + B * self.o_bs + 64,), GUARD, dtype=BF, device=DEV)
        fb = torch.full((self.far_off + B * self.far_bs + 64,), GUARD, dtype=BF, device=DEV)
        self.view(ob, self.o_off, self.o_bs, self.o_rs).copy_(x)
        self.view(fb, self.far_off, self.far_bs, self.far_rs).copy_(y)
        n = B * H * SQ
        lb = [torch.full((n + 2 * self.l_off,), GUARD, device=DEV) for _ in range(3)]
        lb[0][self.l_off:self.l_off + n] = a.flatten().to(DEV)
        lb[1][self.l_off:self.l_off + n] = f.flatten().to(DEV)
        fb0, l0, l1 = fb.clone(), lb[0].clone(), lb[1].clone()
        _lib.attn_merge_lse(ob, lb[0], fb, lb[1], B, H, self.hd, SQ, self.o_bs, self.o_rs, self.far_bs, self.far_rs,
                            lse_out=lb[2] if with_lse else None, o_off=self.o_off, lse_off=self.l_off, far_off=self.far_off,
                            lse_far_off=self.l_off, lse_out_off=self.l_off)
        bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)                 # (a NaN is not equal to itself)
        assert all(torch.equal(bits(p), bits(q)) for p, q in ((fb, fb0), (lb[0], l0), (lb[1], l1)))     # the inputs are read only
        # guards: everything of the o buffer outside the [B][SQ][row] view, and around lse_out
        inside = torch.zeros_like(ob, dtype=torch.bool)
        self.view(inside, self.o_off, self.o_bs, self.o_rs).fill_(True)
        assert bool((ob[~inside] == GUARD).all())
        assert bool((lb[2][:self.l_off] == GUARD).all()) and bool((lb[2][self.l_off + n:] == GUARD).all())
        if not with_lse:
            assert bool((lb[2] == GUARD).all())
        out = self.view(ob, self.o_off, self.o_bs, self.o_rs)
        return ob, out, (lb[2][self.l_off:self.l_off + n].view(B, H, SQ) if with_lse else None)


_CASES = {}


def case(hd):
    if hd not in _CASES:
        _CASES[hd] = Case(hd)
    return _CASES[hd]


@pytest.mark.parametrize("hd", [64, 128])
def test_random_rows_within_one_bf16_step_of_float64_and_lse_out_within_the_fp32_tolerance(hd):
    c = case(hd)
    _, out, lse = c.run()
    want64, lse64 = merge_ref(c.x, c.a, c.y, c.f, H, hd)
    want = want64.to(BF)
    got = out.cpu()
    diff = (got.double() - want.double()).abs()
    step = one_bf16_step(torch.maximum(got.double().abs(), want.double().abs()))
    share, worst = (diff > 0).double().mean().item(), (diff / step).max().item()
    print("merge d%d: %d of %d elements differ from bf16(ref64) (share %.3e), worst %.3f bf16 steps"
          % (hd, int((diff > 0).sum()), diff.numel(), share, worst))
    assert worst <= 1.0, worst
    # lse_out: the LSE tests' yardstick -- the kernel's error against float64 within LSE_FACTOR x torch fp32's on the same operands
    m = torch.maximum(c.a, c.f)
    f32 = m + torch.log2(torch.exp2(c.a - m) + torch.exp2(c.f - m))
    e_hip, e_torch = (lse.cpu().double() - lse64).abs().max().item(), (f32.double() - lse64).abs().max().item()
    print("merge d%d: max |lse_out - float64| kernel %.3e, torch fp32 %.3e (ratio %.2f, bound %.1f)"
          % (hd, e_hip, e_torch, e_hip / max(e_torch, 1e-30), LSE_FACTOR))
    assert e_torch > 0 and e_hip <= LSE_FACTOR * e_torch, (e_hip, e_torch)
    # two runs bit-identical, with and without lse_out
    _, again, lse2 = c.run()
    _, no_lse, _ = c.run(with_lse=False)
    assert torch.equal(again, out) and torch.equal(lse2, lse) and torch.equal(no_lse, out)


@pytest.mark.parametrize("hd", [64, 128])
def test_a_side_without_mass_leaves_the_other_sides_bits(hd):
    c = case(hd)
    x, y = c.x.to(DEV), c.y.to(DEV)
    dead = torch.full_like(c.a, NINF)
    # lse_far = -inf: o keeps its bits; lse = -inf: the far bits; both: o, and lse_out = -inf
    _, out, lse = c.run(f=dead)
    assert torch.equal(out, x) and torch.equal(lse.cpu(), c.a)
    _, out, lse = c.run(a=dead)
    assert torch.equal(out, y) and torch.equal(lse.cpu(), c.f)
    _, out, lse = c.run(a=dead, f=dead)
    assert torch.equal(out, x) and bool((lse == NINF).all())
    # mixed per (b, h, q): every third row dead on the far side, every fifth on the near side
    a, f = c.a.clone(), c.f.clone()
    f[:, :, ::3] = NINF
    a[:, :, 1::5] = NINF
    _, out, lse = c.run(a=a, f=f)
    want64, lse64 = merge_ref(c.x, a, c.y, f, H, hd)
    far_dead = torch.isinf(f).transpose(1, 2).unsqueeze(-1).expand(B, SQ, H, hd).reshape(B, SQ, c.row)
    near_dead = (torch.isinf(a) & ~torch.isinf(f)).transpose(1, 2).unsqueeze(-1).expand(B, SQ, H, hd).reshape(B, SQ, c.row)
    got = out.cpu()
    assert torch.equal(got[far_dead], c.x[far_dead]) and torch.equal(got[near_dead], c.y[near_dead])
    both = torch.isinf(a) & torch.isinf(f)
    assert bool(both.any()) and bool((lse.cpu()[both] == NINF).all()) and bool(torch.isfinite(lse.cpu()[~both]).all())
    # |a - f| = 200: the smaller weight underflows to 0 (2^-200 is no fp32 number): the dominant side's bits
    _, out, lse = c.run(f=c.a - 200.0)
    assert torch.equal(out, x) and torch.equal(lse.cpu(), c.a)
    _, out, lse = c.run(f=c.a + 200.0)
    assert torch.equal(out, y) and torch.equal(lse.cpu(), c.a + 200.0)
    # equal LSEs, rows of 2 and of 4: 3 exactly, and lse_out = a + 1
    two, four = torch.full_like(c.x, 2.0), torch.full_like(c.x, 4.0)
    _, out, lse = c.run(x=two, y=four, f=c.a)
    assert bool((out == 3.0).all()) and torch.equal(lse.cpu(), c.a + 1.0)
    # specials in a row that is not merged do not travel: NaN in the far row of a far-dead query stays out of o
    y2 = c.y.clone()
    y2[:, ::3] = float("nan")
    f2 = c.f.clone()
    f2[:, :, ::3] = NINF
    _, out, _ = c.run(y=y2, f=f2)
    assert bool(torch.isfinite(out.float()).all())


def test_the_wrapper_refuses_what_the_kernel_would_read_out_of_bounds():
    c = case(64)
    o = torch.zeros(B * SQ * c.row, dtype=BF, device=DEV)
    lse = torch.zeros(B * H * SQ, device=DEV)
    ok = dict(batch=B, heads=H, head_dim=64, Sq=SQ, o_bs=SQ * c.row, o_rs=c.row, far_bs=SQ * c.row, far_rs=c.row)
    _lib.attn_merge_lse(o, lse, o.clone(), lse, **ok)
    for bad, match in ((dict(o_rs=c.row + 8), "does not hold"), (dict(o_off=8), "does not hold"), (dict(far_rs=c.row - 8), "row stride"),
                       (dict(o_rs=c.row + 4), "multiples of 8"), (dict(lse_off=1), "lse must be contiguous fp32"),
                       (dict(head_dim=96), "head_dim=96"), (dict(Sq=0), "positive")):
        with pytest.raises(_lib.AlgHipError, match=match):
            _lib.attn_merge_lse(o, lse, o.clone(), lse, **dict(ok, **bad))
    with pytest.raises(_lib.AlgHipError, match="bfloat16"):
        _lib.attn_merge_lse(o.float(), lse, o, lse, **ok)
    with pytest.raises(_lib.AlgHipError, match="lse_far must be contiguous fp32"):
        _lib.attn_merge_lse(o, lse, o.clone(), lse.double(), **ok)
    torch.cuda.synchronize()


# ---- the partition identity ----------------------------------------------------------------------------------------------------
FRAMES, HW, PREFIX, TAIL = 9, 384, 32, 50
LN2 = 0.6931471805599453


def _tables(window):
    near = grid_aligned(window)
    far = complement_ranges(near)
    per_block = _block_ranges(far)
    assert max(len(r) for r in per_block) == 2 and any(not r for r in per_block)      # a block with two far ranges, one with none
    return near, far, [j for j, r in enumerate(per_block) if not r]


def _lse_bound(lse_m, lse_full, lse_n, lse_f, ref64, f32, term):
    """|merged lse_out - the one-full-range launch's lse| by the triangle inequality over float64: the full launch and the two
    partial launches are each held to (term + LSE_FACTOR x torch fp32's error) by their own tests, a log-sum-exp of two values does
    not amplify their errors, and the merge's own arithmetic is held to LSE_FACTOR x torch fp32's error on the same two inputs."""
    e_torch = (f32 - ref64).abs().max().item()
    a, f = lse_n.double(), lse_f.double()
    m = torch.maximum(a, f)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    m64 = m0 + torch.log2(torch.exp2(a - m0) + torch.exp2(f - m0))
    a32, f32_ = lse_n.float(), lse_f.float()
    mm = torch.maximum(a32, f32_)
    m32 = mm + torch.log2(torch.exp2(a32 - mm) + torch.exp2(f32_ - mm))
    e_merge = (m32.double() - m64).abs().max().item()
    bound = 2.0 * (term + LSE_FACTOR * e_torch) + LSE_FACTOR * max(e_merge, 2.0 ** -20)
    err = (lse_m.double() - lse_full.double()).abs().max().item()
    print("partition: max |merged lse - full-range lse| %.3e; torch fp32 vs float64 %.3e, merge in fp32 vs float64 %.3e, bound %.3e"
          % (err, e_torch, e_merge, bound))
    assert err <= bound, (err, bound)


def _lse_refs(q, k, Bn, Hn, hd, Sq, Skv, unit):
    """(float64 log2-domain lse over all keys, the same by torch in fp32 with TF32 off) [B, H, Sq]"""
    qh = q.view(Bn, Sq, Hn, hd).transpose(1, 2)
    kh = k.view(Bn, Skv, Hn, hd).transpose(1, 2)
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ref = torch.logsumexp(qh.double() @ kh.double().transpose(-1, -2) * unit, dim=-1) / math.log(2.0)
        f32 = (torch.logsumexp(qh.float() @ kh.float().transpose(-1, -2) * unit, dim=-1) / math.log(2.0)).double()
    finally:
        torch.backends.cuda.matmul.allow_tf32 = saved
    return ref, f32


def test_partition_d64_near_far_merge_is_the_attention_over_all_keys():
    Bn, Hn = 1, 2
    S = PREFIX + FRAMES * HW
    D = Hn * 64
    near, far, full_blocks = _tables(frame_window_ranges(FRAMES, HW, 1, prefix=PREFIX))
    assert full_blocks == [0]                                                        # the block with the prompt rows
    q, k, v, vt, s_pad = R64.operands(Bn, Hn, S)

    def launch(table):
        o = torch.full((Bn, S, D), GUARD, dtype=BF, device=DEV)
        lse = torch.full((Bn, Hn, S), float("nan"), device=DEV)
        _lib.flash_attn_d64_ranges_heads(q, k, vt, o, Bn, Hn, S, S * D, D, D * s_pad, s_pad, S * D, D, table, lse=lse)
        return o, lse

    (o_n, lse_n), (o_f, lse_f), (o_full, lse_full) = launch(near), launch(far), launch(full_ranges(S, S))
    assert bool((lse_f[:, :, :256] == NINF).all()) and bool((o_f[:, :256] == 0).all())           # the block without a far key
    assert bool(torch.isfinite(lse_f[:, :, 256:]).all()) and bool(torch.isfinite(lse_n).all())
    merged, lse_m = o_n.clone(), torch.full_like(lse_n, float("nan"))
    _lib.attn_merge_lse(merged, lse_n, o_f, lse_f, Bn, Hn, 64, S, S * D, D, S * D, D, lse_out=lse_m)
    assert torch.equal(merged[:, :256], o_n[:, :256]) and torch.equal(lse_m[:, :, :256], lse_n[:, :, :256])
    assert not torch.equal(merged[:, 256:], o_n[:, 256:])
    ref = R64._sdpa(q, k, v, None, Bn, Hn, S)
    e_merged, e_dense = rel(merged, ref), rel(R64.dense(q, k, vt, s_pad, Bn, Hn, S), ref)
    print("partition d64: near + far + merge vs fp32 SDPA %.4e, the one-full-range launch %.4e, the dense entry %.4e (ratio %.3f, "
          "factor %.1f)" % (e_merged, rel(o_full, ref), e_dense, e_merged / e_dense, FACTOR))
    assert bool(torch.isfinite(merged.float()).all())
    assert e_merged <= FACTOR * e_dense, (e_merged, e_dense)
    _lse_bound(lse_m, lse_full, lse_n, lse_f, *_lse_refs(q, k, Bn, Hn, 64, S, S, LN2), BF16_SUM_TERM)


def test_partition_d128_near_far_merge_is_the_attention_over_all_keys():
    Bn, Hn = 1, 2
    S = FRAMES * HW
    Skv, Sq = S + TAIL, S + TAIL + 10                                                # prompt keys behind the video, prompt queries
    D = Hn * 128
    near, far, full_blocks = _tables(frame_window_ranges(FRAMES, HW, 1, tail=(S, Skv), rows=Sq))
    q, k, v, vt, s_pad = R128.operands(Bn, Hn, Sq, Skv)

    def launch(table):
        o = torch.full((Bn, Sq, D), GUARD, dtype=BF, device=DEV)
        lse = torch.full((Bn, Hn, Sq), float("nan"), device=DEV)
        _lib.flash_attn_d128_ranges_heads(q, k, vt, o, Bn, Hn, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, R128.SCALE,
                                          table, lse=lse)
        return o, lse

    (o_n, lse_n), (o_f, lse_f), (o_full, lse_full) = launch(near), launch(far), launch(full_ranges(Sq, Skv))
    rows = torch.zeros(Sq, dtype=torch.bool)
    for j in full_blocks:
        rows[j * 256:(j + 1) * 256] = True
    assert bool((lse_f[:, :, rows] == NINF).all()) and bool((o_f[:, rows] == 0).all())
    assert bool(torch.isfinite(lse_f[:, :, ~rows]).all()) and bool(torch.isfinite(lse_n).all())
    merged, lse_m = o_n.clone(), torch.full_like(lse_n, float("nan"))
    _lib.attn_merge_lse(merged, lse_n, o_f, lse_f, Bn, Hn, 128, Sq, Sq * D, D, Sq * D, D, lse_out=lse_m)
    assert torch.equal(merged[:, rows], o_n[:, rows]) and torch.equal(merged[:, rows], o_full[:, rows])
    assert not torch.equal(merged[:, ~rows], o_n[:, ~rows])
    ref = R128._masked_sdpa(q, k, v, torch.ones(Sq, Skv, dtype=torch.bool), Bn, Hn, Sq, Skv)
    err = (merged.float() - ref).abs()
    err_full = (o_full.float() - ref).abs()
    print("partition d128: near + far + merge vs fp32 SDPA max %.3e mean %.3e; the one-full-range launch max %.3e mean %.3e"
          % (err.max().item(), err.mean().item(), err_full.max().item(), err_full.mean().item()))
    assert bool(torch.isfinite(merged.float()).all())
    assert err.max().item() < 3e-2
    assert err.mean().item() < 2e-3
    _lse_bound(lse_m, lse_full, lse_n, lse_f, *_lse_refs(q, k, Bn, Hn, 128, Sq, Skv, R128.SCALE), 0.0)
