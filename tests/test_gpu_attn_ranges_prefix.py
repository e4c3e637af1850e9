"""alg_flash_attn_d128_ranges_prefix (attention128_q64.hip: the ranged frame over up to 12 segments, with the log-sum-exp of the
keys visited so far written behind every segment) and alg_attn_prefix_mass, on the operands, tables and references of
test_gpu_attn_ranges.py / test_gpu_attn_ranges_heads.py, with the statement on (ALG_ATTN128_Q64=2) and off (=3)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import test_gpu_attn_ranges as R
import test_gpu_attn_ranges_heads as RH
from alg_amd import _lib
from alg_amd.attn_window import (KvRanges, KvRangesHeads, KvSegments, decide_widths, frame_profile_segments, frame_window_ranges,
                                 head_width_ranges, width_segments)

pytestmark = pytest.mark.gpu
DEV, BF, SCALE, FLAGS, LISTS, ALG_EINVAL = R.DEV, R.BF, R.SCALE, R.FLAGS, R.LISTS, R.ALG_EINVAL
SQ, SKV, LSE_FACTOR = RH.SQ, RH.SKV, RH.LSE_FACTOR
GUARD = 64
E = None     # an empty entry

# Partitions of [0, 2050) per block of 256 queries (Sq = 1300: six blocks, the last one partial).  Empty entries first, in the
# middle and last; adjacent segments of one tile (64 keys: too short for the statement), of 2 keys (the ragged last tile on its
# own) and of 9 tiles and more (the statement runs); block 0 has everything in ONE segment.
CUTS9 = [
    [E, E, E, E, (0, 2050), E, E, E, E],
    [(0, 64), (64, 128), (128, 640), (640, 704), (704, 1024), (1024, 1088), (1088, 1600), (1600, 2048), (2048, 2050)],
    [E, (0, 1024), E, (1024, 1088), E, E, (1088, 2050), E, E],
    [(0, 576), E, E, (576, 1216), (1216, 1280), (1280, 1344), E, (1344, 2050), E],
    [E, E, (0, 64), (64, 1984), E, (1984, 2050), E, E, E],
    [(0, 192), (192, 256), E, (256, 896), (896, 960), E, (960, 1600), (1600, 1664), (1664, 2050)],
]
CUTS12 = [
    [(0, 64), (64, 128), (128, 192), (192, 256), (256, 832), (832, 896), (896, 1472), (1472, 1536), (1536, 1600), (1600, 1664),
     (1664, 2048), (2048, 2050)],
    [E, E, E, E, E, E, E, E, E, E, E, (0, 2050)],
    [E, (0, 640), E, (640, 1280), E, (1280, 1920), E, (1920, 1984), E, (1984, 2048), (2048, 2050), E],
    [(0, 1024), E, E, E, E, E, (1024, 2050), E, E, E, E, E],
    [E, E, E, (0, 128), (128, 704), (704, 768), (768, 1408), E, E, (1408, 2050), E, E],
    [(0, 2050), E, E, E, E, E, E, E, E, E, E, E],
]


def segments_of(cuts):
    t = torch.zeros(len(cuts), len(cuts[0]), 2, dtype=torch.int32)
    for j, row in enumerate(cuts):
        for i, be in enumerate(row):
            if be is not None:
                t[j, i, 0], t[j, i, 1] = be
    return KvSegments(t, SKV, SQ)


def run_prefix(q, k, vt, s_pad, B, H, Sq, Skv, table):
    """The new entry: (o, prefix [B, H, segments, Sq]).  The prefix buffer starts from NaN between two guards: every [b, h, i, q]
    must have been written and nothing else."""
    D = H * 128
    n = table.max_ranges
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    buf = torch.full((GUARD + B * H * n * Sq + GUARD,), float("nan"), device=DEV)
    buf[:GUARD] = 7.0
    buf[-GUARD:] = 7.0
    _lib.flash_attn_d128_ranges_prefix(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE, table,
                                       buf, prefix_off=GUARD)
    pre = buf[GUARD:-GUARD].view(B, H, n, Sq)
    assert not bool(torch.isnan(pre).any())                                   # every prefix of every query is written
    assert bool((buf[:GUARD] == 7.0).all()) and bool((buf[-GUARD:] == 7.0).all())         # and nothing around them
    return o, pre


def cut_down(table, n):
    """`table` with only the first n ranges of every row."""
    t = table.table.clone()
    t[..., n:, :] = 0
    return type(table)(t, table.Skv, table.Sq)


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("B,H", [(1, 2), (2, 3)])
def test_o_and_every_prefix_are_the_existing_entrys_bits(B, H, flag, monkeypatch):
    """For tables alg_flash_attn_d128_ranges_heads takes: O is that entry's O, and prefix i is the lse of that entry on the table
    cut down to its first i + 1 ranges.  No tolerance."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    q, k, v, vt, s_pad = RH.operands(B, H)
    for table in (R.table_of(LISTS, SQ, SKV), RH.heads_table(H)):
        o, pre = run_prefix(q, k, vt, s_pad, B, H, SQ, SKV, table)
        want_o, want_lse = RH.run(q, k, vt, s_pad, B, H, SQ, SKV, table, lse=True)
        assert torch.equal(o, want_o)
        assert torch.equal(pre[:, :, -1], want_lse)
        for i in range(table.max_ranges - 1):
            lse_i = RH.run(q, k, vt, s_pad, B, H, SQ, SKV, cut_down(table, i + 1), lse=True)[1]
            assert torch.equal(pre[:, :, i], lse_i), i


_FULL_REF = {}


def full_references(B, H):
    """(fp32 SDPA over all keys, float64 log2-domain LSE over all keys, the same by torch in fp32 with TF32 off), made once."""
    if (B, H) not in _FULL_REF:
        q, k, v, vt, s_pad = RH.operands(B, H)
        heads = lambda t, n: t.view(B, n, H, 128).transpose(1, 2)
        ref = torch.empty(B, H, SQ, dtype=torch.float64, device=DEV)
        f32 = torch.empty(B, H, SQ, dtype=torch.float64, device=DEV)
        saved = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            sdpa = R._masked_sdpa(q, k, v, torch.ones(SQ, SKV, dtype=torch.bool), B, H, SQ, SKV)
            for b in range(B):
                s64 = heads(q, SQ)[b].double() @ heads(k, SKV)[b].double().transpose(-1, -2) * SCALE
                ref[b] = torch.logsumexp(s64, dim=-1) / math.log(2.0)
                s32 = heads(q, SQ)[b].float() @ heads(k, SKV)[b].float().transpose(-1, -2) * SCALE
                f32[b] = (torch.logsumexp(s32, dim=-1) / math.log(2.0)).double()
        finally:
            torch.backends.cuda.matmul.allow_tf32 = saved
        _FULL_REF[(B, H)] = (sdpa, ref, f32)
    return _FULL_REF[(B, H)]


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("name,cuts", [("9", CUTS9), ("12", CUTS12)])
@pytest.mark.parametrize("B,H", [(1, 2), (2, 3)])
def test_partition_tables_are_the_dense_attention(B, H, name, cuts, flag, monkeypatch):
    """A partition of [0, Skv) into 9 / 12 segments: O within the multi-range bound of test_gpu_attn_ranges.py (max 3e-2, mean
    2e-3 against fp32 SDPA), the last prefix within LSE_FACTOR x torch fp32's error against float64.
    Measured on an MI355X (docs/numerics.md), 9 and 12 segments and either flag alike: O max 1.74e-2 / mean 4.8e-4 (B, H = 1, 2) and
    2.14e-2 / 5.0e-4 (2, 3); last prefix 2.81e-5 against torch fp32 3.36e-5 (ratio 0.84) and 3.08e-5 against 4.16e-5 (0.74)."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    q, k, v, vt, s_pad = RH.operands(B, H)
    seg = segments_of(cuts)
    assert seg.segments == len(cuts[0])
    o, pre = run_prefix(q, k, vt, s_pad, B, H, SQ, SKV, seg)
    sdpa, ref, f32 = full_references(B, H)
    err = (o.float() - sdpa).abs()
    print("%s segments vs fp32 SDPA: max %.3e mean %.3e" % (name, err.max().item(), err.mean().item()))
    assert bool(torch.isfinite(o.float()).all())
    assert err.max().item() < 3e-2
    assert err.mean().item() < 2e-3
    e_hip, e_torch = (pre[:, :, -1].double() - ref).abs().max().item(), (f32 - ref).abs().max().item()
    RH._report("lse_d128_ranges_prefix_%sseg_B%d_H%d_flag%s" % (name, B, H, flag), e_hip, e_torch)
    assert e_torch > 0
    assert e_hip <= LSE_FACTOR * e_torch, (e_hip, e_torch)
    # a prefix never shrinks beyond the rounding of m * c + log2(l) on either side (8 fp32 spacings: 1e-6 relative), and a
    # skipped segment repeats its predecessor bit for bit
    assert bool((pre[:, :, 1:] >= pre[:, :, :-1] - 1e-6 * (1.0 + pre[:, :, 1:].abs())).all())
    for j, row in enumerate(cuts):
        rows = slice(j * 256, min((j + 1) * 256, SQ))
        for i, be in enumerate(row):
            if be is None and i > 0:
                assert torch.equal(pre[:, :, i, rows], pre[:, :, i - 1, rows]), (j, i)
    o2, pre2 = run_prefix(q, k, vt, s_pad, B, H, SQ, SKV, seg)
    assert torch.equal(o2, o) and torch.equal(pre2, pre)                      # deterministic


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("cuts", [CUTS9, CUTS12])
def test_prefixes_of_zero_queries_are_log2_of_the_keys_visited_so_far(cuts, flag, monkeypatch):
    """Q = 0: every probability is 1 and the row sum an integer below 2^24, so prefix i == log2(keys of the segments 0 .. i), and
    -inf in front of the first visited segment.  abs 1e-5 as in test_gpu_attn_ranges_heads.py (fp32 spacing at 11 is 9.5e-7)."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    B, H = 2, 3
    q, k, v, vt, s_pad = RH.operands(B, H)
    o, pre = run_prefix(torch.zeros_like(q), k, vt, s_pad, B, H, SQ, SKV, segments_of(cuts))
    for j, row in enumerate(cuts):
        rows = slice(j * 256, min((j + 1) * 256, SQ))
        n = 0
        for i, be in enumerate(row):
            n += 0 if be is None else be[1] - be[0]
            got = pre[:, :, i, rows]
            if n == 0:
                assert bool((got == float("-inf")).all()), (j, i)
            else:
                assert (got.double() - math.log2(n)).abs().max().item() <= 1e-5, (j, i)
        assert n == SKV


def prefix_mass(pre, row0=0, rows=None):
    B, H, n, Sq = pre.shape
    out = torch.full((B * H * n,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.attn_prefix_mass(pre.contiguous(), out, B * H, n, Sq, row0=row0, rows=rows)
    return out.view(B, H, n)


def mass_by_definition(pre, row0, rows):
    """The definition in float64 on the CPU, every (panel, segment) summed exactly (math.fsum) from the kernel's own prefixes."""
    P = pre.double().cpu().numpy()[..., row0:row0 + rows]                     # [B, H, n, rows]
    with np.errstate(invalid="ignore"):
        cum = np.where(np.isneginf(P), 0.0, np.exp2(P - P[:, :, -1:, :]))
    term = np.diff(cum, axis=2, prepend=0.0)
    B, H, n, _ = term.shape
    return torch.tensor([[[math.fsum(term[b, h, i]) / rows for i in range(n)] for h in range(H)] for b in range(B)],
                        dtype=torch.float64)


def test_prefix_mass_is_its_definition_and_bit_identical_from_run_to_run(monkeypatch):
    """Against the definition evaluated in float64 with exact sums.  Bound 32 * 2^-53 absolute on masses <= 1: a term is the
    difference of two exp2 of which each implementation is within 1 ulp of the truth (4 * 2^-53 between the two evaluations), and the
    kernel's sum of `rows` terms goes through at most 2 + 6 + 16 = 24 roundings of partial sums <= rows (per lane, across the
    lanes, across the waves) before the division by rows: 24 * 2^-53.  Measured on an MI355X: at most 1.1e-16."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")
    B, H = 2, 3
    q, k, v, vt, s_pad = RH.operands(B, H)
    for cuts in (CUTS9, CUTS12):
        pre = run_prefix(q, k, vt, s_pad, B, H, SQ, SKV, segments_of(cuts))[1]
        for row0, rows in ((0, SQ), (256, 512), (100, 1001), (1299, 1)):
            got = prefix_mass(pre, row0, rows)
            want = mass_by_definition(pre, row0, rows)
            err = (got.cpu() - want).abs().max().item()
            print("%d segments, rows [%d, %d): max |mass - definition| = %.3e" % (len(cuts[0]), row0, row0 + rows, err))
            assert err <= 32 * 2.0 ** -53, (row0, rows, err)
            assert abs(got.sum(dim=-1).cpu() - 1.0).max().item() <= 32 * 12 * 2.0 ** -53          # the masses of a panel add up to 1
            assert torch.equal(prefix_mass(pre, row0, rows), got)
    # Q = 0: the mass of a segment is its share of the keys
    pre0 = run_prefix(torch.zeros_like(q), k, vt, s_pad, B, H, SQ, SKV, segments_of(CUTS9))[1]
    got = prefix_mass(pre0, 256, 256).cpu()                                  # block 1: nine segments
    want = torch.tensor([(e - b) / SKV for b, e in CUTS9[1]], dtype=torch.float64)
    assert (got - want).abs().max().item() <= 1e-6


_MASS_REF = {}


def mass_references(B, H, cuts):
    """Per (b, h, segment) the mean over all rows of the softmax mass on the segment's keys: (float64 masked softmax of the bf16
    operands, the same through torch fp32 -- fp32 scores, fp32 log-sum-exp of the keys of the segments 0 .. i, then the definition
    of alg_attn_prefix_mass: the route whose error sources are the kernel's, 1-ulp exp / log and the summation order)."""
    key = (B, H, id(cuts))
    if key not in _MASS_REF:
        q, k, v, vt, s_pad = RH.operands(B, H)
        n = len(cuts[0])
        upto = torch.zeros(n, SQ, SKV, dtype=torch.bool)                      # keys of the segments 0 .. i, per query
        for j, row in enumerate(cuts):
            for i, be in enumerate(row):
                if be is not None:
                    upto[i:, j * 256:(j + 1) * 256, be[0]:be[1]] = True
        upto = upto.to(DEV)
        heads = lambda t, m: t.view(B, m, H, 128).transpose(1, 2)
        ref = torch.empty(B, H, n, dtype=torch.float64, device=DEV)
        f32 = torch.empty(B, H, n, dtype=torch.float64, device=DEV)
        saved = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            for b in range(B):
                p64 = torch.softmax(heads(q, SQ)[b].double() @ heads(k, SKV)[b].double().transpose(-1, -2) * SCALE, dim=-1)
                s32 = heads(q, SQ)[b].float() @ heads(k, SKV)[b].float().transpose(-1, -2) * SCALE
                cum64 = torch.stack([(p64 * upto[i]).sum(dim=-1) for i in range(n)], dim=1)                   # [H, n, Sq]
                l32 = torch.stack([torch.logsumexp(s32.masked_fill(~upto[i], -math.inf), dim=-1) for i in range(n)], dim=1)
                l32 = (l32 / math.log(2.0)).double()                                                          # fp32 values
                cum32 = torch.where(torch.isneginf(l32), torch.zeros_like(l32), torch.exp2(l32 - l32[:, -1:]))
                ref[b] = torch.diff(cum64, dim=1, prepend=torch.zeros_like(cum64[:, :1])).mean(dim=-1)
                f32[b] = torch.diff(cum32, dim=1, prepend=torch.zeros_like(cum32[:, :1])).mean(dim=-1)
        finally:
            torch.backends.cuda.matmul.allow_tf32 = saved
        _MASS_REF[key] = (ref, f32)
    return _MASS_REF[key]


@pytest.mark.parametrize("flag", FLAGS)
def test_prefix_mass_on_random_operands_is_within_four_times_torch_fp32_of_float64(flag, monkeypatch):
    """Measured on an MI355X (docs/numerics.md): kernel 2.10e-8 (statement) / 2.02e-8 (C++ tile body), torch fp32 3.20e-8: ratio
    0.66 / 0.63."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    B, H = 2, 3
    q, k, v, vt, s_pad = RH.operands(B, H)
    ref, f32 = mass_references(B, H, CUTS12)
    got = prefix_mass(run_prefix(q, k, vt, s_pad, B, H, SQ, SKV, segments_of(CUTS12))[1])
    e_hip, e_torch = (got - ref).abs().max().item(), (f32 - ref).abs().max().item()
    RH._report("prefix_mass_12seg_B2_H3_flag" + flag, e_hip, e_torch)
    assert e_torch > 0
    assert e_hip <= LSE_FACTOR * e_torch, (e_hip, e_torch)


def test_bad_arguments_are_refused_before_any_launch():
    B, H, Sq, Skv = 1, 2, 256, 513
    q, k, v, vt, s_pad = R.operands(B, H, Sq, Skv)
    D = H * 128
    t = torch.zeros(1, 12, 2, dtype=torch.int32)
    t[0, 3, 1], t[0, 7, 0], t[0, 7, 1] = 256, 256, 513
    seg = KvSegments(t, Skv, Sq)
    table = seg.device_table
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    pre = torch.full((B * H * 12 * Sq + 1,), 7.0, device=DEV)
    lib = _lib.load_library()
    P = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def call(table_p, segments, table_heads, pre_p, q_p=None):
        return lib.alg_flash_attn_d128_ranges_prefix(q_p or P(q), P(k), P(vt), P(o), B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad,
                                                     s_pad, Sq * D, D, SCALE, table_p, segments, table_heads, pre_p, _lib._stream())

    null = ctypes.c_void_p(0)
    for args in ((P(table), 0, 1, P(pre)), (P(table), 13, 1, P(pre)), (P(table), 12, 3, P(pre)), (P(table), 12, 0, P(pre)),
                 (P(table), 12, 1, null), (P(table), 12, 1, P(pre, 2)), (null, 12, 1, P(pre)), (P(table, 2), 12, 1, P(pre)),
                 (P(table), 12, 1, P(pre), P(q, 2))):
        assert call(*args) == ALG_EINVAL, args[1:3]
        assert b"alg_flash_attn_d128_ranges_prefix" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((pre == 7.0).all())              # nothing was launched
    assert call(P(table), 12, 1, P(pre)) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any()) and not bool((pre[:-1] == 7.0).any()) and pre[-1].item() == 7.0
    out = torch.full((B * H * 12 + 1,), 7.0, dtype=torch.float64, device=DEV)
    for a in ((null, P(out), 2, 12, Sq, 0, Sq), (P(pre), null, 2, 12, Sq, 0, Sq), (P(pre, 2), P(out), 2, 12, Sq, 0, Sq),
              (P(pre), P(out, 4), 2, 12, Sq, 0, Sq), (P(pre), P(out), 0, 12, Sq, 0, Sq), (P(pre), P(out), 2, 0, Sq, 0, Sq),
              (P(pre), P(out), 2, 13, Sq, 0, Sq), (P(pre), P(out), 2, 12, Sq, -1, 4), (P(pre), P(out), 2, 12, Sq, 0, 0),
              (P(pre), P(out), 2, 12, Sq, 200, 57)):
        assert lib.alg_attn_prefix_mass(*a, _lib._stream()) == ALG_EINVAL, a[2:]
        assert b"alg_attn_prefix_mass" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    A = (q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE)
    with pytest.raises(_lib.AlgHipError, match="KvSegments"):
        _lib.flash_attn_d128_ranges_prefix(*A, table, pre)
    with pytest.raises(_lib.AlgHipError, match="room for"):
        _lib.flash_attn_d128_ranges_prefix(*A, seg, pre[:100])
    with pytest.raises(_lib.AlgHipError, match="Sq=512"):
        _lib.flash_attn_d128_ranges_prefix(*A, KvSegments(torch.cat([t, t]), Skv, 512), pre)


def test_graph_capture_replays_the_prefix_launch_and_the_reduction():
    B, H = 1, 2
    D = H * 128
    q, k, v, vt, s_pad = RH.operands(B, H)
    seg = segments_of(CUTS9)
    want_o, want_pre = run_prefix(q, k, vt, s_pad, B, H, SQ, SKV, seg)
    want_mass = prefix_mass(want_pre)
    o = torch.zeros(B, SQ, D, dtype=BF, device=DEV)
    pre = torch.zeros(B, H, 9, SQ, device=DEV)
    mass = torch.zeros(B * H * 9, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.flash_attn_d128_ranges_prefix(q, k, vt, o, B, H, SQ, SKV, SQ * D, D, SKV * D, D, D * s_pad, s_pad, SQ * D, D, SCALE, seg,
                                           pre)
        _lib.attn_prefix_mass(pre, mass, B * H, 9, SQ)
    o.zero_(), pre.zero_(), mass.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want_o) and torch.equal(pre, want_pre) and torch.equal(mass.view(B, H, 9), want_mass)


def test_a_local_head_is_found_with_its_width(monkeypatch):
    """8 frames x 256 tokens, 3 heads, widths (1, 2, 4), in the manner of test_a_head_that_is_local_is_found.  Head 0: K and Q carry
    1.5 x the Walsh pattern of their own frame (25 nats on the keys of the query's frame): width 1.  Head 1: Q carries the
    pattern of the frame TWO away (f + 2, or f - 2 at the end of the video): nothing within +-1, everything within +-2.  Head 2:
    Q = 0, uniform attention: its recall at width 4 is the coverage, 55 / 64 -- dense at 0.9."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")
    F, hw, B, H = 8, 256, 1, 3
    S = F * hw
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(B, S, H * 128, generator=g) for _ in range(3))
    d = torch.arange(128)
    walsh = torch.stack([1.0 - 2.0 * (torch.tensor([bin(int(x) & f).count("1") for x in d]) % 2) for f in range(F)])   # [F, 128]
    code = 1.5 * walsh.repeat_interleave(hw, dim=0)
    two_away = 1.5 * torch.stack([walsh[f + 2 if f + 2 < F else f - 2] for f in range(F)]).repeat_interleave(hw, dim=0)
    q[:, :, :128] += code
    k[:, :, :128] += code
    q[:, :, 128:256] += two_away
    k[:, :, 128:256] += code
    q[:, :, 256:] = 0
    q, k, v = q.to(BF).to(DEV), k.to(BF).to(DEV), v.to(BF).to(DEV)
    vt = R.make_vt(v, S)
    widths = (1, 2, 4)
    seg = frame_profile_segments(F, hw, widths)
    assert seg.segments == 9
    D = H * 128
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    pre = torch.full((B, H, 9, S), float("nan"), device=DEV)
    _lib.flash_attn_d128_ranges_prefix(q, k, vt, o, B, H, S, S, S * D, D, S * D, D, D * S, S, S * D, D, SCALE, seg, pre)
    mass = prefix_mass(pre).cpu()
    recall = [[[min(sum(mass[0, h, i].item() for i in idx), 1.0) for idx in width_segments(3)] for h in range(H)]]
    print("recall by width:", [[round(x, 6) for x in h] for h in recall[0]])
    assert recall[0][0][0] > 0.99
    assert recall[0][1][0] < 0.01 and recall[0][1][1] > 0.99
    assert abs(recall[0][2][2] - 55.0 / 64.0) <= 1e-6
    for h in range(H):
        assert recall[0][h][0] <= recall[0][h][1] + 1e-12 and recall[0][h][1] <= recall[0][h][2] + 1e-12
    chosen = decide_widths(recall, widths, 0.9)
    assert chosen == [1, 2, 0]
    # hw % 64 == 0 and no tail: the counted keys ARE the window's, so the recall is the two-launch one up to the fp32 LSEs: a
    # log-sum-exp below 64 has spacing 3.8e-6, each route takes the difference of two of them (rounding + 1-ulp log: 3 spacings,
    # 1.1e-5 in log2, 7.9e-6 relative on a recall <= 1): 2e-5 between the two routes
    full = RH.run(q, k, vt, S, B, H, S, S, KvRanges(torch.tensor([[[0, S]]] * F, dtype=torch.int32), S, S), lse=True)[1]
    for j, w in enumerate(widths):
        part = RH.run(q, k, vt, S, B, H, S, S, frame_window_ranges(F, hw, w), lse=True)[1]
        two = RH.recall(part, full).cpu()
        assert (two[0] - torch.tensor([recall[0][h][j] for h in range(H)], dtype=torch.float64)).abs().max().item() <= 2e-5
    # ... and the table built from the decision is what each head then runs; the calibration launch was the dense attention
    kvr = head_width_ranges({w: frame_window_ranges(F, hw, w) for w in widths}, chosen)
    assert isinstance(kvr, KvRangesHeads)
    got = RH.run(q, k, vt, S, B, H, S, S, kvr)
    assert torch.equal(got[:, :, :128], R.ranged(q, k, vt, S, B, H, S, S, frame_window_ranges(F, hw, 1))[:, :, :128])
    assert torch.equal(got[:, :, 128:256], R.ranged(q, k, vt, S, B, H, S, S, frame_window_ranges(F, hw, 2))[:, :, 128:256])
    dense = R.dense(q, k, vt, S, B, H, S, S)
    assert torch.equal(got[:, :, 256:], dense[:, :, 256:])
    err = (o.float() - dense.float()).abs()
    assert err.max().item() < 3e-2 and err.mean().item() < 2e-3
