"""The position-major band at kernel level: gather (attn_layout.hip) -> alg_flash_attn_d128_ranges with the position_band_ranges
table -> scatter, on the operands of test_gpu_attn_ranges.py -- half the queries x 6, one dominating key -- at S = 960 (F = 6,
HW = 160) and S = 385 (F = 5, HW = 77: nothing is a multiple of anything), band 2.  In frame-major terms the launch is a masked
softmax under M[s_q][s_k] = band_mask[pi(s_q)][pi(s_k)]: held to that file's bound for range lists; keys outside the mask are not
visited; and the band's recall from the two LSEs is the softmax mass torch finds inside the mask."""
import math

import pytest
import torch

import test_gpu_attn_ranges as R
from alg_amd import _lib
from alg_amd.attn_window import HeadList, full_ranges, position_band_ranges, position_major_index, ranges_to_mask

pytestmark = pytest.mark.gpu
DEV, BF, SCALE = R.DEV, R.BF, R.SCALE
B, H, BAND = 2, 3, 2
SHAPES = [(6, 160), (5, 77)]
RECALL_RTOL = 1e-6     # what test_gpu_attn_ranges_heads.py holds the frame window's recall to (relative)


@pytest.fixture(autouse=True)
def _q64_for_every_call(monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")


_CASES = {}


def case(F, HW):
    """Operands, the band table, pi and the frame-major mask of one shape: made once, never written to."""
    if (F, HW) not in _CASES:
        S = F * HW
        q, k, v, vt, s_pad = R.operands(B, H, S, S)
        table = position_band_ranges(F, HW, BAND)
        pi = position_major_index(F, HW)
        mask = ranges_to_mask(table)[pi][:, pi]                            # M[s_q][s_k] = band_mask[pi(s_q)][pi(s_k)]
        _CASES[(F, HW)] = (q, k, v, vt, s_pad, table, pi.to(DEV), mask)
    return _CASES[(F, HW)]


def band_launch(F, HW, q, k, vt, s_pad, table, heads, lse=False):
    """gather -> ranged launch on the compact position-major buffers -> (o_pm, lse_pm); heads: indices into the H heads."""
    S, D, n = F * HW, H * 128, len(heads)
    Dc = n * 128
    hl = HeadList(heads, H)
    e = lambda *s: torch.full(s, 5.0, dtype=BF, device=DEV)
    qp, kp, vtp, op = e(B, S, Dc), e(B, S, Dc), e(B, Dc, s_pad), e(B, S, Dc)
    _lib.attn_rows_position_major(q, qp, hl, 128, B, F, HW, S * D, D, S * Dc, Dc)
    _lib.attn_rows_position_major(k, kp, hl, 128, B, F, HW, S * D, D, S * Dc, Dc)
    _lib.attn_vt_position_major(vt, vtp, hl, 128, B, F, HW, D * s_pad, s_pad, Dc * s_pad, s_pad)
    A = (qp, kp, vtp, op, B, n, S, S, S * Dc, Dc, S * Dc, Dc, Dc * s_pad, s_pad, S * Dc, Dc, SCALE, table)
    if lse:
        l = torch.full((B, n, S), float("nan"), device=DEV)
        _lib.flash_attn_d128_ranges_heads(*A, lse=l)
        return op, l
    _lib.flash_attn_d128_ranges(*A)
    return op, None


def band_forward(F, HW, q, k, vt, s_pad, table, heads):
    """... and the scatter into a frame-major output pre-filled with 7: what the Wan forward does for its band heads."""
    S, D = F * HW, H * 128
    Dc = len(heads) * 128
    op, _ = band_launch(F, HW, q, k, vt, s_pad, table, heads)
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    _lib.attn_rows_position_major(op, o, HeadList(heads, H), 128, B, F, HW, S * Dc, Dc, S * D, D, inverse=True)
    return o


@pytest.mark.parametrize("heads", [[2, 0], [0, 1, 2]], ids=["heads20", "all"])
@pytest.mark.parametrize("F,HW", SHAPES)
def test_band_against_masked_sdpa_in_frame_major_terms(F, HW, heads):
    S = F * HW
    q, k, v, vt, s_pad, table, pi, mask = case(F, HW)
    assert table.max_ranges == 1 and 0 < table.coverage < 1
    o = band_forward(F, HW, q, k, vt, s_pad, table, heads).view(B, S, H, 128)
    ref = R._masked_sdpa(q, k, v, mask, B, H, S, S).view(B, S, H, 128)
    err = (o[:, :, heads].float() - ref[:, :, heads]).abs()
    print("band F=%d HW=%d heads %s vs masked fp32 SDPA: max %.3e mean %.3e" % (F, HW, heads, err.max().item(), err.mean().item()))
    assert bool(torch.isfinite(o.float()).all())
    assert err.max().item() < 3e-2
    assert err.mean().item() < 2e-3
    for h in set(range(H)) - set(heads):
        assert bool((o[:, :, h] == 7.0).all())                            # a head outside the list keeps its bytes
    assert torch.equal(band_forward(F, HW, q, k, vt, s_pad, table, heads).view(B, S, H, 128), o)      # deterministic


@pytest.mark.parametrize("F,HW", SHAPES)
def test_keys_outside_the_band_are_not_visited(F, HW):
    """As test_gpu_attn_ranges.py checks for range lists: a large FINITE value in every K row and V^T column whose position-major
    index lies outside block j's range and shares no 64-key tile with the range's end leaves block j's queries bit for bit."""
    S = F * HW
    q, k, v, vt, s_pad, table, pi, mask = case(F, HW)
    heads = [0, 1, 2]
    o = band_forward(F, HW, q, k, vt, s_pad, table, heads)
    inv = position_major_index(HW, F).to(DEV)                              # position-major row -> frame-major row
    perm = R._perm(s_pad)
    for j in range(table.q_blocks):
        b, e = table.table[j, 0].tolist()
        touched = torch.zeros(S, dtype=torch.bool, device=DEV)
        touched[b:(e + 63) // 64 * 64] = True
        outside = inv[(~touched).nonzero().flatten()]                      # frame-major indices of the untouched keys
        rows = inv[j * 256:min((j + 1) * 256, S)]
        assert outside.numel() > 0, j
        k2, vt2 = k.clone(), vt.clone()
        k2[:, outside] = 3.0e4
        vt2[:, :, perm[outside]] = 3.0e4
        assert torch.equal(band_forward(F, HW, q, k2, vt2, s_pad, table, heads)[:, rows], o[:, rows]), j
        inside = inv[b]                                                    # ... and one key inside the range changes them
        vt3 = vt.clone()
        vt3[:, :, perm[inside]] = 3.0e4
        assert not torch.equal(band_forward(F, HW, q, k, vt3, s_pad, table, heads)[:, rows], o[:, rows]), j


@pytest.mark.parametrize("F,HW", SHAPES)
def test_band_recall_is_the_softmax_mass_inside_the_mask(F, HW):
    """lse_band (position-major launch, rows brought back to frame-major) and lse_full (the frame-major launch over all keys)
    through alg_attn_lse_recall, against the same fraction by torch in double from the fp32 scores.
    Measured on an MI355X: see the printed figures (the run's output)."""
    S, D = F * HW, H * 128
    q, k, v, vt, s_pad, table, pi, mask = case(F, HW)
    _, lse_pm = band_launch(F, HW, q, k, vt, s_pad, table, [0, 1, 2], lse=True)
    lse_band = lse_pm[:, :, pi].contiguous()                               # frame-major row s holds the LSE of row pi(s)
    assert torch.equal(lse_band, lse_pm.view(B, H, HW, F).transpose(-1, -2).reshape(B, H, S))      # the transpose the model uses
    lse_full = torch.full((B, H, S), float("nan"), device=DEV)
    o = torch.empty(B, S, D, dtype=BF, device=DEV)
    _lib.flash_attn_d128_ranges_heads(q, k, vt, o, B, H, S, S, S * D, D, S * D, D, D * s_pad, s_pad, S * D, D, SCALE, full_ranges(S, S),
                                      lse=lse_full)
    got = torch.zeros(B, H, dtype=torch.float64, device=DEV)
    _lib.attn_lse_recall(lse_band, lse_full, got, B * H, S)
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        heads_of = lambda t: t.float().view(B, S, H, 128).transpose(1, 2)
        s32 = heads_of(q) @ heads_of(k).transpose(-1, -2) * SCALE          # the fp32 scores
    finally:
        torch.backends.cuda.matmul.allow_tf32 = saved
    p = torch.softmax(s32.double(), dim=-1)
    want = (p * mask.to(DEV)).sum(dim=-1).mean(dim=-1)                     # [B, H]
    err = ((got - want).abs() / want).max().item()
    print("band recall F=%d HW=%d: %s, torch %s, max rel err %.3e (bound %.1e); coverage %.4f"
          % (F, HW, [round(x, 7) for x in got.flatten().tolist()], [round(x, 7) for x in want.flatten().tolist()], err, RECALL_RTOL,
             table.coverage))
    assert bool((got > 0).all()) and bool((got <= 1.0 + 1e-6).all())
    assert err <= RECALL_RTOL, err


def test_graph_capture_replays_gather_band_scatter():
    F, HW = 6, 160
    S, D = F * HW, H * 128
    q, k, v, vt, s_pad, table, pi, mask = case(F, HW)
    heads = [2, 0]
    want = band_forward(F, HW, q, k, vt, s_pad, table, heads)             # (also uploads the table; HeadLists upload below)
    Dc = len(heads) * 128
    hl = HeadList(heads, H)
    hl.on(DEV)
    e = lambda *s: torch.zeros(s, dtype=BF, device=DEV)
    qp, kp, vtp, op = e(B, S, Dc), e(B, S, Dc), e(B, Dc, s_pad), e(B, S, Dc)
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.attn_rows_position_major(q, qp, hl, 128, B, F, HW, S * D, D, S * Dc, Dc)
        _lib.attn_rows_position_major(k, kp, hl, 128, B, F, HW, S * D, D, S * Dc, Dc)
        _lib.attn_vt_position_major(vt, vtp, hl, 128, B, F, HW, D * s_pad, s_pad, Dc * s_pad, s_pad)
        _lib.flash_attn_d128_ranges(qp, kp, vtp, op, B, len(heads), S, S, S * Dc, Dc, S * Dc, Dc, Dc * s_pad, s_pad, S * Dc, Dc, SCALE, table)
        _lib.attn_rows_position_major(op, o, hl, 128, B, F, HW, S * Dc, Dc, S * D, D, inverse=True)
    o.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want)
