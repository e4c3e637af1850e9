"""alg_flash_attn_d64_ranges_heads (attention.hip: a table row per (head, q block) and the log2-domain log-sum-exp of the visited
keys on the d = 64 frame), the twin of test_gpu_attn_ranges_heads.py, on the operands and tables of test_gpu_attn_ranges_d64.py --
S = 2050, nine query blocks, half the rows x 6 (they keep a non-zero offset), one dominating key -- under ALG_ATTN_PP = 4, 8 and 0:
a per-head table IS the shared-table entry head by head, the LSE output leaves O alone, is exact where it can be derived (Q = 0)
and is held to a float64 evaluation elsewhere; alg_attn_lse_recall on d = 64 LSEs; refusals; capture.  No shape plans a split tail."""
import ctypes
import json
import math
import os

import pytest
import torch

import test_gpu_attn_ranges_d64 as R
from alg_amd import _lib
from alg_amd.attn_window import (KvRanges, KvRangesHeads, decide_heads, frame_window_ranges, full_ranges, head_window_ranges,
                                 ranges_to_mask)

pytestmark = pytest.mark.gpu
DEV, BF, PPS, LISTS, ALG_EINVAL = R.DEV, R.BF, R.PPS, R.LISTS, R.ALG_EINVAL
S = R.S_BIG
SHAPES = [(1, 2), (2, 3)]
LSE_FACTOR = 4.0     # the d = 128 test's yardstick: kernel error <= 4 x torch fp32's on the same operands
# the allowance the entry was specified with for the d = 64 frames' row sum of bf16-rounded probabilities.  (The frame's own sum is
# off by up to 2^-8, one bf16 round-to-nearest, which misses this; the instantiations that write the LSE therefore carry the
# difference to the fp32 sum of the unrounded probabilities, and the term is kept as an allowance they do not need.)
BF16_SUM_TERM = math.log2(1.0 + 2.0 ** -9)


def head_lists(h):
    """Head slices: LISTS, the full range, LISTS reversed."""
    return (LISTS, [[(0, S)]] * len(LISTS), LISTS[::-1])[h % 3]


def padded(lists):
    """A KvRanges of `lists` with four entries per block (unused ones (0, 0)): every head's slice has the same width."""
    t = torch.zeros(len(lists), 4, 2, dtype=torch.int32)
    for j, r in enumerate(lists):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return KvRanges(t, S, S)


def heads_table(H):
    return KvRangesHeads(torch.stack([padded(head_lists(h)).table for h in range(H)]), S, S)


def run(q, k, vt, s_pad, B, H, kvr, lse=False, S_=S):
    """The new entry; returns o, or (o, lse) with lse [B, H, S] started from NaN (every query must be written)."""
    D = H * 64
    o = torch.full((B, S_, D), 7.0, dtype=BF, device=DEV)
    l = torch.full((B, H, S_), float("nan"), device=DEV) if lse else None
    _lib.flash_attn_d64_ranges_heads(q, k, vt, o, B, H, S_, S_ * D, D, D * s_pad, s_pad, S_ * D, D, kvr, lse=l)
    return (o, l) if lse else o


def visited_keys(lists):
    """[S] number of keys each query visits under the block lists."""
    n = torch.zeros(S, dtype=torch.float64)
    for j, r in enumerate(lists):
        n[j * 256:(j + 1) * 256] = sum(e - b for b, e in r)
    return n


@pytest.mark.parametrize("pp", PPS)
@pytest.mark.parametrize("B,H", SHAPES)
def test_per_head_table_is_the_shared_table_entry_head_by_head(B, H, pp, monkeypatch):
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    q, k, v, vt, s_pad = R.operands(B, H, S)
    got = run(q, k, vt, s_pad, B, H, heads_table(H))
    for h in range(H):
        want = R.ranged(q, k, vt, s_pad, B, H, S, padded(head_lists(h)))
        assert torch.equal(got[:, :, h * 64:(h + 1) * 64], want[:, :, h * 64:(h + 1) * 64]), h
        assert not bool((got[:, :, h * 64:(h + 1) * 64] == 7.0).all(dim=-1).any())


@pytest.mark.parametrize("pp", PPS)
@pytest.mark.parametrize("B,H", SHAPES)
def test_shared_table_bits_and_the_lse_output_does_not_disturb_o(B, H, pp, monkeypatch):
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    q, k, v, vt, s_pad = R.operands(B, H, S)
    shared = R.table_of(LISTS, S)
    assert torch.equal(run(q, k, vt, s_pad, B, H, shared), R.ranged(q, k, vt, s_pad, B, H, S, shared))   # table_heads = 1, lse = None
    D = H * 64
    for kvr in (heads_table(H), shared):
        want = run(q, k, vt, s_pad, B, H, kvr)
        o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
        buf = torch.full((B * H * S + 1,), float("nan"), device=DEV)       # one guard element behind [B][H][S]
        buf[-1] = 7.0
        _lib.flash_attn_d64_ranges_heads(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr, lse=buf)
        assert torch.equal(o, want)
        assert bool(torch.isfinite(buf[:-1]).all())                        # written for every query
        assert buf[-1].item() == 7.0
        assert torch.equal(run(q, k, vt, s_pad, B, H, kvr, lse=True)[1].flatten(), buf[:-1])      # deterministic


@pytest.mark.parametrize("pp", PPS)
def test_lse_of_zero_queries_is_log2_of_the_visited_keys_and_an_empty_block_is_minus_inf(pp, monkeypatch):
    """Q = 0: every score is 0, the offset snaps to zero, every probability is 1 (exact in bf16), the row sum an integer below
    2^24, so lse == log2(visited keys).  abs 1e-5: fp32 spacing at 11 is 9.5e-7, which leaves room for a few ulps of the hardware
    log2 (the bound of the d = 128 test for the same exact case)."""
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    B, H = 2, 3
    q, k, v, vt, s_pad = R.operands(B, H, S)
    q0 = torch.zeros_like(q)
    o, lse = run(q0, k, vt, s_pad, B, H, heads_table(H), lse=True)
    for h in range(H):
        want = torch.log2(visited_keys(head_lists(h))).to(DEV)
        err = (lse[:, h].double() - want).abs().max().item()
        print("ALG_ATTN_PP=%s Q = 0, head %d: max |lse - log2(n)| = %.3e" % (pp, h, err))
        assert err <= 1e-5, (h, err)
    # a block the table leaves without a key (no validated table has one: raw call): -inf, zero rows
    D = H * 64
    t = R.table_of(LISTS, S).table.clone()
    t[2] = 0
    t[4, 0, 0], t[4, 0, 1] = 128, 64                                       # end <= begin: skipped as well
    td = t.to(DEV)
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    lse = torch.full((B, H, S), float("nan"), device=DEV)
    lib = _lib.load_library()
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib.alg_flash_attn_d64_ranges_heads(P(q0), P(k), P(vt), P(o), B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, P(td), 4, 1,
                                             P(lse), _lib._stream())
    assert rc == 0
    for j in (2, 4):
        rows = slice(j * 256, (j + 1) * 256)
        assert bool((lse[:, :, rows] == float("-inf")).all()) and bool((o[:, rows] == 0).all()), j
    rows = slice(0, 512)
    assert (lse[:, :, rows].double() - torch.log2(visited_keys(LISTS))[rows].to(DEV)).abs().max().item() <= 1e-5


def _report(case, e_hip, e_torch, bound):
    print("%s: max |lse - float64| kernel %.3e, torch fp32 %.3e, bound log2(1 + 2^-9) + %.1f x torch = %.3e"
          % (case, e_hip, e_torch, LSE_FACTOR, bound))
    dest = os.environ.get("ALG_PARITY_REPORT", "")
    if dest.endswith(".jsonl"):
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "a") as f:
            f.write(json.dumps({"case": case, "err_lse_hip_vs_float64": e_hip, "err_lse_torch_fp32_vs_float64": e_torch,
                                "bf16_sum_term": BF16_SUM_TERM, "factor": LSE_FACTOR, "bound": bound,
                                "passed": e_hip <= bound}) + "\n")


_LSE_REF = {}


def lse_references(B, H):
    """(float64 log2-domain log-sum-exp of the bf16 operands under the per-head tables -- Q is pre-scaled: the scores are q . k --
    and the same by torch in fp32 with TF32 off).  Made once, never written to."""
    if (B, H) not in _LSE_REF:
        q, k, v, vt, s_pad = R.operands(B, H, S)
        mask = ranges_to_mask(heads_table(H)).to(DEV)                   # [H, S, S]
        heads = lambda t: t.view(B, S, H, 64).transpose(1, 2)
        ref = torch.empty(B, H, S, dtype=torch.float64, device=DEV)
        f32 = torch.empty(B, H, S, dtype=torch.float64, device=DEV)
        saved = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            for b in range(B):
                s64 = (heads(q)[b].double() @ heads(k)[b].double().transpose(-1, -2) * R.LN2).masked_fill(~mask, -math.inf)
                ref[b] = torch.logsumexp(s64, dim=-1) / math.log(2.0)
                s32 = (heads(q)[b].float() @ heads(k)[b].float().transpose(-1, -2) * R.LN2).masked_fill(~mask, -math.inf)
                f32[b] = (torch.logsumexp(s32, dim=-1) / math.log(2.0)).double()
        finally:
            torch.backends.cuda.matmul.allow_tf32 = saved
        _LSE_REF[(B, H)] = (ref, f32)
    return _LSE_REF[(B, H)]


@pytest.mark.parametrize("pp", PPS)
def test_lse_on_random_operands_against_float64(pp, monkeypatch):
    """max |lse - float64| <= log2(1 + 2^-9) + LSE_FACTOR x (torch fp32's error against the same float64): the first term is the
    allowance for bf16-rounded probabilities in the row sum, the second the d = 128 test's yardstick.  The rows that snap their
    offset to zero (the second half) and those that carry one (the first half, x 6) are reported separately."""
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    B, H = 2, 3
    q, k, v, vt, s_pad = R.operands(B, H, S)
    ref, f32 = lse_references(B, H)
    o, lse = run(q, k, vt, s_pad, B, H, heads_table(H), lse=True)
    for name, rows in (("offset_rows", slice(0, S // 2)), ("zero_offset_rows", slice(S // 2, S)), ("all_rows", slice(0, S))):
        e_hip = (lse.double() - ref)[:, :, rows].abs().max().item()
        e_torch = (f32 - ref)[:, :, rows].abs().max().item()
        _report("lse_d64_ranges_heads_B2_H3_pp%s_%s" % (pp, name), e_hip, e_torch, BF16_SUM_TERM + LSE_FACTOR * e_torch)
    assert e_torch > 0
    assert e_hip <= BF16_SUM_TERM + LSE_FACTOR * e_torch, (e_hip, e_torch)      # (the last pass of the loop: all rows)


def recall(part, full, row0=0, rows=None):
    B, H, Sq = part.shape
    out = torch.full((B * H,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.attn_lse_recall(part, full, out, B * H, Sq, row0=row0, rows=rows)
    return out.view(B, H)


def test_recall_of_zero_queries_is_the_covered_fraction():
    """Q = 0: a query's recall is (visited keys) / S, so a panel's is the mean of that over its rows; the full table gives 1."""
    B, H = 2, 3
    q, k, v, vt, s_pad = R.operands(B, H, S)
    q0 = torch.zeros_like(q)
    part = run(q0, k, vt, s_pad, B, H, heads_table(H), lse=True)[1]
    full = run(q0, k, vt, s_pad, B, H, full_ranges(S, S), lse=True)[1]
    assert torch.equal(recall(full, full), torch.ones(B, H, dtype=torch.float64, device=DEV))
    for row0, rows in ((0, S), (256, 512), (100, 1001)):
        got = recall(part, full, row0, rows).cpu()
        for h in range(H):
            want = (visited_keys(head_lists(h))[row0:row0 + rows] / S).mean().item()
            err = (got[:, h] - want).abs().max().item() / want
            print("Q = 0, head %d, rows [%d, %d): recall %.9f, covered %.9f (rel %.2e)" % (h, row0, row0 + rows, got[0, h], want, err))
            assert err <= 1e-6, (h, row0, rows, err)


def test_a_head_that_is_local_is_found(monkeypatch):
    """8 frames x 256 tokens, 2 heads, window 1.  Head 0: K and Q carry 0.8 x a frame-specific +-1 pattern (Walsh functions:
    orthogonal between frames) on top of 0.25 x noise, worth 0.64 * 64 = 41 log2 units on the keys of the query's own frame
    against a spread of about 2 elsewhere -- its mass stays in the frame.  Head 1: Q = 0, uniform attention, so its recall is its
    coverage."""
    monkeypatch.setenv("ALG_ATTN_PP", "4")
    F, hw, B, H = 8, 256, 1, 2
    S_ = F * hw
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(B, S_, H * 64, generator=g) for _ in range(3))
    d = torch.arange(64)
    walsh = torch.stack([1.0 - 2.0 * (torch.tensor([bin(int(x) & f).count("1") for x in d]) % 2) for f in range(F)])   # [F, 64]
    code = 0.8 * walsh.repeat_interleave(hw, dim=0)
    q[:, :, :64] = 0.25 * q[:, :, :64] + code
    k[:, :, :64] = 0.25 * k[:, :, :64] + code
    q[:, :, 64:] = 0
    q, k, v = q.to(BF).to(DEV), k.to(BF).to(DEV), v.to(BF).to(DEV)
    vt = R.make_vt(v, S_)
    base = frame_window_ranges(F, hw, 1)
    lse_full = run(q, k, vt, S_, B, H, full_ranges(S_, S_), lse=True, S_=S_)[1]
    lse_part = run(q, k, vt, S_, B, H, base, lse=True, S_=S_)[1]
    rec = recall(lse_part, lse_full).cpu()
    print("recall: local head %.6f, uniform head %.9f (coverage %.9f)" % (rec[0, 0], rec[0, 1], base.coverage))
    assert rec[0, 0].item() > 0.99
    assert abs(rec[0, 1].item() - base.coverage) <= 1e-6 * base.coverage
    windowed = decide_heads(rec.tolist(), 0.9)
    assert windowed == [True, False]
    # ... and the table built from the decision is what each head then runs
    kvr = head_window_ranges(base, windowed)
    o = run(q, k, vt, S_, B, H, kvr, S_=S_)
    assert torch.equal(o[:, :, :64], R.ranged(q, k, vt, S_, B, H, S_, base)[:, :, :64])
    assert torch.equal(o[:, :, 64:], R.ranged(q, k, vt, S_, B, H, S_, full_ranges(S_, S_))[:, :, 64:])


def test_bad_arguments_are_refused_before_any_launch():
    B, H, S_ = 1, 2, 513
    q, k, v, vt, s_pad = R.operands(B, H, S_)
    D = H * 64
    table = full_ranges(S_, S_).device_table
    o = torch.full((B, S_, D), 7.0, dtype=BF, device=DEV)
    lse = torch.full((B * H * S_ + 1,), 7.0, device=DEV)
    lib = _lib.load_library()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(max_ranges, table_heads, lse_p):
        return lib.alg_flash_attn_d64_ranges_heads(P(q), P(k), P(vt), P(o), B, H, S_, S_ * D, D, D * s_pad, s_pad, S_ * D, D,
                                                   P(table), max_ranges, table_heads, lse_p, _lib._stream())

    for args in ((1, 3, P(lse)), (1, 0, P(lse)), (1, 1, P(lse, 2)), (0, 1, P(lse)), (5, 1, P(lse))):
        assert call(*args) == ALG_EINVAL, args[:2]
        assert b"alg_flash_attn_d64_ranges_heads" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((lse == 7.0).all())          # nothing was launched
    assert call(1, 1, P(lse)) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any()) and not bool((lse[:-1] == 7.0).any()) and lse[-1].item() == 7.0
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):
        _lib.flash_attn_d64_ranges_heads(q, k, vt, o, B, H, S_, S_ * D, D, D * s_pad, s_pad, S_ * D, D, table)
    with pytest.raises(_lib.AlgHipError, match="3 heads"):
        _lib.flash_attn_d64_ranges_heads(q, k, vt, o, B, H, S_, S_ * D, D, D * s_pad, s_pad, S_ * D, D,
                                         KvRangesHeads(torch.stack([full_ranges(S_, S_).table] * 3), S_, S_))


def test_graph_capture_replays_the_per_head_launch_with_lse():
    """The table is device-resident before the capture begins, the entry only enqueues: a captured launch replays to the eager bits."""
    B, H = 2, 3
    D = H * 64
    q, k, v, vt, s_pad = R.operands(B, H, S)
    kvr = heads_table(H)
    want_o, want_lse = run(q, k, vt, s_pad, B, H, kvr, lse=True)
    o = torch.zeros(B, S, D, dtype=BF, device=DEV)
    lse = torch.zeros(B, H, S, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.flash_attn_d64_ranges_heads(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr, lse=lse)
    o.zero_()
    lse.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want_o) and torch.equal(lse, want_lse)
