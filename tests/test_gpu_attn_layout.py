"""alg_attn_rows_position_major and alg_attn_vt_position_major (attn_layout.hip) against torch indexing, bit for bit: the gather's
compact output, the scatter that leaves every other byte alone, gather then scatter as the identity, and V^T's permuted key axis
with zero padding -- at shapes with ragged 16-byte tails (S = 385), one frame, one position, both head widths, head lists in any
order, sources inside a wider buffer and destinations pre-filled with a pattern."""
import pytest
import torch

from alg_amd import _lib
from alg_amd.attn_window import HeadList, position_major_index

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
B, HEADS = 2, 4
SHAPES = [(6, 160), (5, 77), (1, 96), (9, 1)]
LISTS = [[0], [3, 0], [0, 1, 2, 3]]
PATTERN = -3.0


def _perm(n):
    return torch.tensor([(i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1) for i in range(n)])


_CACHE = {}


def wide(F, HW, hd):
    """The [Q | K] buffer of a layer, [B][S][2 D] (K at offset D: row stride 2 D), and its guard: a flat tensor with 64 elements
    in front of and behind it.  Computed once per shape and never written."""
    key = ("rows", F, HW, hd)
    if key not in _CACHE:
        S, D = F * HW, HEADS * hd
        g = torch.Generator().manual_seed(F * 1000 + HW + hd)
        _CACHE[key] = torch.randn(64 + B * S * 2 * D + 64, generator=g).to(BF).to(DEV)
    return _CACHE[key]


def vt_src(F, HW, hd):
    """V^T [B][D][S_pad + 64] (a row stride wider than needed) holding key s at column perm(s), and the logical [B][D][S]."""
    key = ("vt", F, HW, hd)
    if key not in _CACHE:
        S, D = F * HW, HEADS * hd
        S_pad = (S + 63) // 64 * 64
        g = torch.Generator().manual_seed(F * 1000 + HW + hd + 7)
        logical = torch.randn(B, D, S, generator=g).to(BF)
        buf = torch.randn(B, D, S_pad + 64, generator=g).to(BF)            # the padding columns hold anything
        buf[:, :, _perm(S_pad)[:S]] = logical
        _CACHE[key] = (buf.to(DEV), logical.to(DEV))
    return _CACHE[key]


@pytest.mark.parametrize("heads", LISTS, ids=lambda l: "heads" + "".join(map(str, l)))
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("F,HW", SHAPES)
def test_rows_gather_scatter_and_round_trip(F, HW, hd, heads):
    S, D, n = F * HW, HEADS * hd, len(heads)
    Dc = n * hd
    pi = position_major_index(F, HW).to(DEV)
    hl = HeadList(heads, HEADS)
    flat = wide(F, HW, hd)
    before = flat.clone()
    qk = flat[64:64 + B * S * 2 * D].view(B, S, 2 * D)
    for off in (0, D):                                                   # Q, and K through the base offset
        want = torch.full((B, S, Dc), PATTERN, dtype=BF, device=DEV)
        sel = qk[:, :, off:off + D].reshape(B, S, HEADS, hd)[:, :, heads].reshape(B, S, Dc)
        want[:, pi] = sel                                                # dst[b][pi(s)][j hd + d] = src[b][s][head_list[j] hd + d]
        guard = torch.full((32 + B * S * Dc + 32,), PATTERN, dtype=BF, device=DEV)
        _lib.attn_rows_position_major(flat, guard, hl, hd, B, F, HW, S * 2 * D, 2 * D, S * Dc, Dc, src_off=64 + off, dst_off=32)
        assert torch.equal(guard[32:-32].view(B, S, Dc), want)
        assert bool((guard[:32] == PATTERN).all()) and bool((guard[-32:] == PATTERN).all())
        assert torch.equal(flat, before)                                 # the source is only read

        # the scatter back into a pre-filled wide tensor [B][S][D]: the selected heads' slices only, nothing outside the tensor
        out = torch.full((32 + B * S * D + 32,), PATTERN, dtype=BF, device=DEV)
        _lib.attn_rows_position_major(guard, out, hl, hd, B, F, HW, S * Dc, Dc, S * D, D, inverse=True, src_off=32, dst_off=32)
        o = out[32:-32].view(B, S, HEADS, hd)
        src = qk[:, :, off:off + D].reshape(B, S, HEADS, hd)
        for h in range(HEADS):
            if h in heads:
                assert torch.equal(o[:, :, h], src[:, :, h]), h          # gather then scatter is the identity
            else:
                assert bool((o[:, :, h] == PATTERN).all()), h
        assert bool((out[:32] == PATTERN).all()) and bool((out[-32:] == PATTERN).all())


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("F,HW", SHAPES)
def test_rows_scatter_against_indexing_into_a_strided_destination(F, HW, hd):
    """inverse = 1 on its own, the destination inside a wider buffer (row stride 2 D, offset D): torch indexing is the reference."""
    S, D, heads = F * HW, HEADS * hd, [3, 0]
    Dc = len(heads) * hd
    pi = position_major_index(F, HW).to(DEV)
    g = torch.Generator().manual_seed(5)
    compact = torch.randn(B, S, Dc, generator=g).to(BF).to(DEV)
    dst = torch.full((B, S, 2 * D), PATTERN, dtype=BF, device=DEV)
    want = dst.clone()
    wv = want[:, :, D:].view(B, S, HEADS, hd)
    for j, h in enumerate(heads):
        wv[:, :, h] = compact[:, pi, j * hd:(j + 1) * hd]                # dst[b][s][head_list[j] hd + d] = src[b][pi(s)][j hd + d]
    _lib.attn_rows_position_major(compact, dst, HeadList(heads, HEADS), hd, B, F, HW, S * Dc, Dc, S * 2 * D, 2 * D, inverse=True, dst_off=D)
    assert torch.equal(dst, want)


@pytest.mark.parametrize("heads", LISTS, ids=lambda l: "heads" + "".join(map(str, l)))
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("F,HW", SHAPES)
def test_vt_keys_move_to_position_major_and_the_padding_is_zero(F, HW, hd, heads):
    S, D, n = F * HW, HEADS * hd, len(heads)
    S_pad = (S + 63) // 64 * 64
    rows = n * hd
    src, logical = vt_src(F, HW, hd)
    before = src.clone()
    pi = position_major_index(F, HW).to(DEV)
    perm = _perm(S_pad).to(DEV)
    want = torch.zeros(B, rows, S_pad, dtype=BF, device=DEV)             # columns S .. S_pad: zero
    sel = logical.view(B, HEADS, hd, S)[:, heads].reshape(B, rows, S)
    want[:, :, perm[pi]] = sel                                           # dst[..][perm(pi(s))] = src[..][perm(s)]
    guard = torch.full((32 + B * rows * S_pad + 32,), PATTERN, dtype=BF, device=DEV)
    _lib.attn_vt_position_major(src, guard, HeadList(heads, HEADS), hd, B, F, HW, D * (S_pad + 64), S_pad + 64, rows * S_pad, S_pad, dst_off=32)
    got = guard[32:-32].view(B, rows, S_pad)
    assert torch.equal(got, want)
    assert bool((got[:, :, perm[S:]] == 0).all()) if S < S_pad else True
    assert bool((guard[:32] == PATTERN).all()) and bool((guard[-32:] == PATTERN).all())
    assert torch.equal(src, before)


def test_vt_more_than_one_tile_per_row():
    """S = 21 x 800 = 16,800 keys: three LDS tiles per row, the last one ragged (S_pad = 16,832), positions that straddle tiles."""
    F, HW, hd, heads = 21, 800, 128, [1]
    S = F * HW
    S_pad = (S + 63) // 64 * 64
    g = torch.Generator().manual_seed(3)
    logical = torch.randn(1, 2 * hd, S, generator=g).to(BF).to(DEV)
    perm, pi = _perm(S_pad).to(DEV), position_major_index(F, HW).to(DEV)
    src = torch.zeros(1, 2 * hd, S_pad, dtype=BF, device=DEV)
    src[:, :, perm[:S]] = logical
    want = torch.zeros(1, hd, S_pad, dtype=BF, device=DEV)
    want[:, :, perm[pi]] = logical[:, hd:]
    got = torch.full((1, hd, S_pad), PATTERN, dtype=BF, device=DEV)
    _lib.attn_vt_position_major(src, got, HeadList(heads, 2), hd, 1, F, HW, 2 * hd * S_pad, S_pad, hd * S_pad, S_pad)
    assert torch.equal(got, want)


def test_graph_capture_replays_the_gather():
    F, HW, hd, heads = 6, 160, 128, [3, 0]
    S, D, Dc = F * HW, HEADS * hd, 2 * hd
    flat = wide(F, HW, hd)
    hl = HeadList(heads, HEADS)
    want = torch.empty(B, S, Dc, dtype=BF, device=DEV)
    _lib.attn_rows_position_major(flat, want, hl, hd, B, F, HW, S * 2 * D, 2 * D, S * Dc, Dc, src_off=64)
    got = torch.zeros_like(want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.attn_rows_position_major(flat, got, hl, hd, B, F, HW, S * 2 * D, 2 * D, S * Dc, Dc, src_off=64)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
