"""alg_flash_attn_d128_ranges_heads (attention128_q64.hip: a table row per (head, q block) and the log2-domain log-sum-exp of the
visited keys) and alg_attn_lse_recall, on the operands and tables of test_gpu_attn_ranges.py -- half the queries x 6, one
dominating key -- with the statement on (ALG_ATTN128_Q64=2) and with the frame's C++ tile body on its own (=3): a per-head table
IS the shared-table entry head by head, the LSE output leaves O alone, is exact where it can be derived (Q = 0) and is held to a
torch fp32 evaluation elsewhere; the recall reduction against its definition; and a head that is local is told from one that is
not."""
import ctypes
import json
import math
import os

import pytest
import torch

import test_gpu_attn_ranges as R
from alg_amd import _lib
from alg_amd.attn_window import (KvRanges, KvRangesHeads, decide_heads, frame_window_ranges, full_ranges, head_window_ranges,
                                 ranges_to_mask)

pytestmark = pytest.mark.gpu
DEV, BF, SCALE, FLAGS, LISTS, ALG_EINVAL = R.DEV, R.BF, R.SCALE, R.FLAGS, R.LISTS, R.ALG_EINVAL
SQ, SKV = 1300, 2050
LSE_FACTOR = 4.0     # kernel error <= 4 x torch fp32's on the same operands: 1-ulp v_exp / v_log and another fp32 summation order


def rotated(h):
    return LISTS[h % len(LISTS):] + LISTS[:h % len(LISTS)]


def heads_table(H, Sq=SQ, Skv=SKV):
    return KvRangesHeads(torch.stack([R.table_of(rotated(h), Sq, Skv).table for h in range(H)]), Skv, Sq)


def run(q, k, vt, s_pad, B, H, Sq, Skv, kvr, lse=False):
    """The new entry; returns o, or (o, lse) with lse [B, H, Sq] started from NaN (every query must be written)."""
    D = H * 128
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    l = torch.full((B, H, Sq), float("nan"), device=DEV) if lse else None
    _lib.flash_attn_d128_ranges_heads(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE, kvr,
                                      lse=l)
    return (o, l) if lse else o


def visited_keys(lists, Sq):
    """[Sq] number of keys each query visits under the block lists."""
    n = torch.zeros(Sq, dtype=torch.float64)
    for j, r in enumerate(lists):
        n[j * 256:(j + 1) * 256] = sum(e - b for b, e in r)
    return n


_OPERANDS = {}


def operands(B, H):
    """The operands of test_gpu_attn_ranges.py, made once per shape and never written to."""
    if (B, H) not in _OPERANDS:
        _OPERANDS[(B, H)] = R.operands(B, H, SQ, SKV)
    return _OPERANDS[(B, H)]


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("B,H", [(1, 2), (2, 3)])
def test_per_head_table_is_the_shared_table_entry_head_by_head(B, H, flag, monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    q, k, v, vt, s_pad = operands(B, H)
    got = run(q, k, vt, s_pad, B, H, SQ, SKV, heads_table(H))
    for h in range(H):
        want = R.ranged(q, k, vt, s_pad, B, H, SQ, SKV, R.table_of(rotated(h), SQ, SKV))
        assert torch.equal(got[:, :, h * 128:(h + 1) * 128], want[:, :, h * 128:(h + 1) * 128]), h
    shared = R.table_of(LISTS, SQ, SKV)
    assert torch.equal(run(q, k, vt, s_pad, B, H, SQ, SKV, shared), R.ranged(q, k, vt, s_pad, B, H, SQ, SKV, shared))   # table_heads = 1


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("B,H", [(1, 2), (2, 3)])
def test_lse_output_does_not_disturb_o(B, H, flag, monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    q, k, v, vt, s_pad = operands(B, H)
    for kvr in (heads_table(H), R.table_of(LISTS, SQ, SKV)):
        o, lse = run(q, k, vt, s_pad, B, H, SQ, SKV, kvr, lse=True)
        assert torch.equal(o, run(q, k, vt, s_pad, B, H, SQ, SKV, kvr))
        assert bool(torch.isfinite(lse).all())                         # written for every query
        assert torch.equal(run(q, k, vt, s_pad, B, H, SQ, SKV, kvr, lse=True)[1], lse)      # deterministic


@pytest.mark.parametrize("flag", FLAGS)
def test_lse_of_zero_queries_is_log2_of_the_visited_keys_and_an_empty_block_is_minus_inf(flag, monkeypatch):
    """Q = 0: every score is 0, every probability 1, the row sum an integer below 2^24, so lse == log2(visited keys).  abs 1e-5:
    fp32 spacing at 11 is 9.5e-7, which leaves room for a few ulps of the hardware log2."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    B, H = 2, 3
    q, k, v, vt, s_pad = operands(B, H)
    q0 = torch.zeros_like(q)
    o, lse = run(q0, k, vt, s_pad, B, H, SQ, SKV, heads_table(H), lse=True)
    for h in range(H):
        want = torch.log2(visited_keys(rotated(h), SQ)).to(DEV)
        err = (lse[:, h].double() - want).abs().max().item()
        print("Q = 0, head %d: max |lse - log2(n)| = %.3e" % (h, err))
        assert err <= 1e-5, (h, err)
    # a block the table leaves without a key (no validated table has one: raw call): -inf, zero rows
    D = H * 128
    t = R.table_of(LISTS, SQ, SKV).table.clone()
    t[2] = 0
    t[4, 0, 0], t[4, 0, 1] = 128, 64                                       # end <= begin: skipped as well
    td = t.to(DEV)
    o = torch.full((B, SQ, D), 7.0, dtype=BF, device=DEV)
    lse = torch.full((B, H, SQ), float("nan"), device=DEV)
    lib = _lib.load_library()
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib.alg_flash_attn_d128_ranges_heads(P(q0), P(k), P(vt), P(o), B, H, SQ, SKV, SQ * D, D, SKV * D, D, D * s_pad, s_pad,
                                              SQ * D, D, SCALE, P(td), 4, 1, P(lse), _lib._stream())
    assert rc == 0
    for j in (2, 4):
        rows = slice(j * 256, (j + 1) * 256)
        assert bool((lse[:, :, rows] == float("-inf")).all()) and bool((o[:, rows] == 0).all()), j
    rows = slice(0, 512)
    assert (lse[:, :, rows].double() - torch.log2(visited_keys(LISTS, SQ))[rows].to(DEV)).abs().max().item() <= 1e-5


def _report(case, e_hip, e_torch):
    print("%s: max |lse - float64| kernel %.3e, torch fp32 %.3e (ratio %.2f, bound %.1f)"
          % (case, e_hip, e_torch, e_hip / max(e_torch, 1e-30), LSE_FACTOR))
    dest = os.environ.get("ALG_PARITY_REPORT", "")
    if dest.endswith(".jsonl"):
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "a") as f:
            f.write(json.dumps({"case": case, "err_lse_hip_vs_float64": e_hip, "err_lse_torch_fp32_vs_float64": e_torch,
                                "ratio": e_hip / max(e_torch, 1e-30), "factor": LSE_FACTOR,
                                "passed": e_hip <= LSE_FACTOR * e_torch}) + "\n")


_LSE_REF = {}


def lse_references(B, H):
    """(float64 log2-domain log-sum-exp of the bf16 operands under the per-head tables, the same by torch in fp32 with TF32 off)."""
    if (B, H) not in _LSE_REF:
        q, k, v, vt, s_pad = operands(B, H)
        mask = ranges_to_mask(heads_table(H)).to(DEV)                   # [H, Sq, Skv]
        heads = lambda t, n: t.view(B, n, H, 128).transpose(1, 2)
        ref = torch.empty(B, H, SQ, dtype=torch.float64, device=DEV)
        f32 = torch.empty(B, H, SQ, dtype=torch.float64, device=DEV)
        saved = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            for b in range(B):          # per sample: the float64 score matrix of one sample is 21 MB per head
                s64 = (heads(q, SQ)[b].double() @ heads(k, SKV)[b].double().transpose(-1, -2) * SCALE).masked_fill(~mask, -math.inf)
                ref[b] = torch.logsumexp(s64, dim=-1) / math.log(2.0)
                s32 = (heads(q, SQ)[b].float() @ heads(k, SKV)[b].float().transpose(-1, -2) * SCALE).masked_fill(~mask, -math.inf)
                f32[b] = (torch.logsumexp(s32, dim=-1) / math.log(2.0)).double()
        finally:
            torch.backends.cuda.matmul.allow_tf32 = saved
        _LSE_REF[(B, H)] = (ref, f32)
    return _LSE_REF[(B, H)]


@pytest.mark.parametrize("flag", FLAGS)
def test_lse_on_random_operands_is_within_four_times_torch_fp32_of_float64(flag, monkeypatch):
    """Measured on an MI355X (docs/numerics.md): kernel 3.08e-5, torch fp32 4.16e-5 (ratio 0.74), with either flag."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    B, H = 2, 3
    q, k, v, vt, s_pad = operands(B, H)
    ref, f32 = lse_references(B, H)
    o, lse = run(q, k, vt, s_pad, B, H, SQ, SKV, heads_table(H), lse=True)
    e_hip, e_torch = (lse.double() - ref).abs().max().item(), (f32 - ref).abs().max().item()
    _report("lse_d128_ranges_heads_B2_H3_flag" + flag, e_hip, e_torch)
    assert e_torch > 0
    assert e_hip <= LSE_FACTOR * e_torch, (e_hip, e_torch)


def recall(part, full, row0=0, rows=None):
    B, H, Sq = part.shape
    out = torch.full((B * H,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.attn_lse_recall(part, full, out, B * H, Sq, row0=row0, rows=rows)
    return out.view(B, H)


def test_recall_of_zero_queries_is_the_covered_fraction():
    """Q = 0: a query's recall is (visited keys) / Skv, so a panel's is the mean of that over its rows; the full table gives 1."""
    B, H = 2, 3
    q, k, v, vt, s_pad = operands(B, H)
    q0 = torch.zeros_like(q)
    part = run(q0, k, vt, s_pad, B, H, SQ, SKV, heads_table(H), lse=True)[1]
    full = run(q0, k, vt, s_pad, B, H, SQ, SKV, full_ranges(SQ, SKV), lse=True)[1]
    assert torch.equal(recall(full, full), torch.ones(B, H, dtype=torch.float64, device=DEV))
    for row0, rows in ((0, SQ), (256, 512), (100, 1001)):
        got = recall(part, full, row0, rows).cpu()
        for h in range(H):
            want = (visited_keys(rotated(h), SQ)[row0:row0 + rows] / SKV).mean().item()
            err = (got[:, h] - want).abs().max().item() / want
            print("Q = 0, head %d, rows [%d, %d): recall %.9f, covered %.9f (rel %.2e)" % (h, row0, row0 + rows, got[0, h], want, err))
            assert err <= 1e-6, (h, row0, rows, err)
    assert abs(recall(part, full)[0, 0].item() - R.table_of(LISTS, SQ, SKV).coverage) <= 1e-6 * 0.5


def test_recall_against_torch_on_random_operands_and_bit_identical_runs():
    B, H = 2, 3
    q, k, v, vt, s_pad = operands(B, H)
    part = run(q, k, vt, s_pad, B, H, SQ, SKV, heads_table(H), lse=True)[1]
    full = run(q, k, vt, s_pad, B, H, SQ, SKV, full_ranges(SQ, SKV), lse=True)[1]
    for row0, rows in ((0, SQ), (256, 512), (100, 1001), (1299, 1)):
        got = recall(part, full, row0, rows)
        want = torch.exp2((part - full).double())[:, :, row0:row0 + rows].mean(dim=-1)
        err = ((got - want).abs() / want).max().item()
        print("rows [%d, %d): recall %s, max rel err vs torch %.2e" % (row0, row0 + rows, [round(x, 6) for x in got.flatten().tolist()], err))
        assert bool((got > 0).all()) and bool((got <= 1.0 + 1e-6).all())
        assert err <= 1e-6, (row0, rows, err)
        assert torch.equal(recall(part, full, row0, rows), got)
    # a term is 0 where lse_part is -inf
    part2 = part.clone()
    part2[:, :, :650] = float("-inf")
    want = torch.exp2((part - full).double())[:, :, 650:].sum(dim=-1) / SQ
    assert ((recall(part2, full) - want).abs() / want).max().item() <= 1e-6


def test_bad_arguments_are_refused_before_any_launch():
    B, H, Sq, Skv = 1, 2, 256, 513
    q, k, v, vt, s_pad = R.operands(B, H, Sq, Skv)
    D = H * 128
    table = full_ranges(Sq, Skv).device_table
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    lse = torch.full((B * H * Sq + 1,), 7.0, device=DEV)
    lib = _lib.load_library()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(max_ranges, table_heads, lse_p):
        return lib.alg_flash_attn_d128_ranges_heads(P(q), P(k), P(vt), P(o), B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad,
                                                    Sq * D, D, SCALE, P(table), max_ranges, table_heads, lse_p, _lib._stream())

    for args in ((1, 3, P(lse)), (1, 0, P(lse)), (1, 1, P(lse, 2)), (0, 1, P(lse)), (5, 1, P(lse))):
        assert call(*args) == ALG_EINVAL, args[:2]
        assert b"alg_flash_attn_d128_ranges_heads" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((lse == 7.0).all())          # nothing was launched
    assert call(1, 1, P(lse)) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any()) and not bool((lse[:-1] == 7.0).any()) and lse[-1].item() == 7.0
    out = torch.zeros(B * H, dtype=torch.float64, device=DEV)
    for rows0 in ((-1, 4), (0, 0), (200, 57)):
        assert lib.alg_attn_lse_recall(P(lse), P(lse), P(out), B * H, Sq, rows0[0], rows0[1], _lib._stream()) == ALG_EINVAL
        assert b"alg_attn_lse_recall" in lib.alg_last_error()
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):
        _lib.flash_attn_d128_ranges_heads(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE,
                                          table)
    with pytest.raises(_lib.AlgHipError, match="3 heads"):
        _lib.flash_attn_d128_ranges_heads(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE,
                                          KvRangesHeads(torch.stack([full_ranges(Sq, Skv).table] * 3), Skv, Sq))


def test_a_head_that_is_local_is_found(monkeypatch):
    """8 frames x 256 tokens, 2 heads, window 1.  Head 0: K and Q carry 1.5 x a frame-specific +-1 pattern (Walsh functions:
    orthogonal between frames), worth 1.5^2 * 128 / sqrt(128) = 25 nats on the keys of the query's own frame -- its mass stays in
    the frame.  Head 1: Q = 0, uniform attention, so its recall is its coverage."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")
    F, hw, B, H = 8, 256, 1, 2
    S = F * hw
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(B, S, H * 128, generator=g) for _ in range(3))
    d = torch.arange(128)
    walsh = torch.stack([1.0 - 2.0 * (torch.tensor([bin(int(x) & f).count("1") for x in d]) % 2) for f in range(F)])   # [F, 128]
    code = 1.5 * walsh.repeat_interleave(hw, dim=0)
    q[:, :, :128] += code
    k[:, :, :128] += code
    q[:, :, 128:] = 0
    q, k, v = q.to(BF).to(DEV), k.to(BF).to(DEV), v.to(BF).to(DEV)
    vt = R.make_vt(v, S)
    base = frame_window_ranges(F, hw, 1)
    lse_full = run(q, k, vt, S, B, H, S, S, full_ranges(S, S), lse=True)[1]
    lse_part = run(q, k, vt, S, B, H, S, S, base, lse=True)[1]
    rec = recall(lse_part, lse_full).cpu()
    print("recall: local head %.6f, uniform head %.9f (coverage %.9f)" % (rec[0, 0], rec[0, 1], base.coverage))
    assert rec[0, 0].item() > 0.99
    assert abs(rec[0, 1].item() - base.coverage) <= 1e-6 * base.coverage
    windowed = decide_heads(rec.tolist(), 0.9)
    assert windowed == [True, False]
    # ... and the table built from the decision is what each head then runs
    kvr = head_window_ranges(base, windowed)
    o = run(q, k, vt, S, B, H, S, S, kvr)
    assert torch.equal(o[:, :, :128], R.ranged(q, k, vt, S, B, H, S, S, base)[:, :, :128])
    assert torch.equal(o[:, :, 128:], R.dense(q, k, vt, S, B, H, S, S)[:, :, 128:])
