"""alg_flash_attn_d64_ranges (attention.hip: each block of 256 queries attends to a short list of key ranges), the d = 64 twin of
test_gpu_attn_ranges.py, under ALG_ATTN_PP = 4 (the zero-offset statement), 8 (the any-offset one) and 0 (the frame's C++ tile
body on its own): the full range IS the dense entry, one range IS the dense entry on the slice, range lists against masked fp32
SDPA, and keys outside the ranges are not visited.

Operands: Q pre-scaled (log2 units: q . k has a standard deviation of 8), half the query rows x 6 -- their first-tile max leaves
(-64, 64), so they keep a non-zero offset and stay out of the zero-offset statement -- and one dominating key (x 8).  None of the
shapes plans a split-KV tail (fewer than 64 units per XCD), so the dense entry is a single launch too."""
import ctypes
import functools

import pytest
import torch

from _parity import FACTOR, rel
from alg_amd import _lib
from alg_amd.attn_window import KvRanges, full_ranges, ranges_to_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
PPS = ("4", "8", "0")
ALG_EINVAL = -1
LN2 = 0.6931471805599453

# one table row per block of 256 queries (S = 2050: nine blocks, the last one of two rows): segment lengths 1, 2, 63, 64, 65, 66;
# segments under eight tiles, which never enter the statement (200: 4, 448: 7), of eight (512: one group of four) and of nine and
# more with every remainder of the four-tile unroll (2050: 33 tiles, 1410: 23, 1025: 17, 576: 9); the dominating key 683 lies inside
# the ranges of blocks 0, 1, 6, 7 and 8 and outside those of blocks 2 .. 5
S_BIG = 2050
LISTS = [
    [(0, 2050)],
    [(0, 64), (640, 2050)],
    [(0, 1), (64, 127), (1024, 1600)],
    [(0, 200), (256, 321), (960, 1985)],
    [(1984, 2050)],
    [(0, 64), (128, 192), (256, 320), (2048, 2050)],
    [(0, 448), (512, 1024)],
    [(640, 1216)],
    [(0, 2050)],
]


def _perm(n):
    return torch.tensor([(i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1) for i in range(n)], device=DEV)


def make_vt(v, s_pad):
    """v [B, S, H*64] -> V^T [B, H*64, s_pad] with kv index bits 2 and 3 swapped, zero padded."""
    B, S, D = v.shape
    vt = torch.zeros(B, D, s_pad, dtype=BF, device=DEV)
    vt[:, :, _perm(s_pad)[:S]] = v.transpose(1, 2)
    return vt


@functools.lru_cache(maxsize=None)
def operands(B, H, S):
    """(q, k, v, vt, s_pad): shared by the tests and left unchanged (the poison cases work on clones)."""
    D = H * 64
    g = torch.Generator().manual_seed(64 + S)
    q, k, v = (torch.randn(B, S, D, generator=g).to(BF).to(DEV) for _ in range(3))
    q[:, : S // 2] *= 6.0
    k[:, S // 3] *= 8.0
    s_pad = (S + 63) // 64 * 64
    return q, k, v, make_vt(v, s_pad), s_pad


def dense(q, k, vt, s_pad, B, H, S, begin=0, rows=None):
    """The dense entry (pre-scaled form) on the keys [begin, begin + S) of buffers that hold `rows` tokens: queries 0 .. S - 1."""
    D = H * 64
    rows = S if rows is None else rows
    o = torch.full((B, rows, D), 7.0, dtype=BF, device=DEV)
    _lib.flash_attn_d64(q, k, vt[:, :, begin:], o, B, H, S, rows * D, D, D * s_pad, s_pad, rows * D, D, 1.0, k_off=begin * D,
                        q_prescaled=True)
    return o


def ranged(q, k, vt, s_pad, B, H, S, kvr):
    D = H * 64
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    _lib.flash_attn_d64_ranges(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr)
    return o


def table_of(lists, S):
    n = max(len(r) for r in lists)
    t = torch.zeros(len(lists), n, 2, dtype=torch.int32)
    for j, r in enumerate(lists):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return KvRanges(t, S, S)


def test_the_operands_keep_offsets_on_half_the_rows():
    q, k, _, _, _ = operands(1, 2, S_BIG)
    s = torch.einsum("bqhd,bkhd->bhqk", q.float().view(1, S_BIG, 2, 64), k.float().view(1, S_BIG, 2, 64)[:, :64])
    m = s.max(dim=-1).values.abs()                                    # first-tile max per (head, row)
    assert bool((m[..., : S_BIG // 2] >= 64.0).float().mean() > 0.9)  # the x 6 rows keep a non-zero offset
    assert bool((m[..., S_BIG // 2:] < 64.0).all())                   # the others snap to zero


@pytest.mark.parametrize("pp", PPS)
@pytest.mark.parametrize("B,H,S", [(1, 2, S_BIG), (1, 1, 513), (2, 3, 1000)])   # (2, 3): six panels on eight XCD slots
def test_full_range_is_the_dense_entry(B, H, S, pp, monkeypatch):
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    q, k, v, vt, s_pad = operands(B, H, S)
    want = dense(q, k, vt, s_pad, B, H, S)
    got = ranged(q, k, vt, s_pad, B, H, S, full_ranges(S, S))
    assert torch.equal(got, want)


@pytest.mark.parametrize("pp", PPS)
@pytest.mark.parametrize("begin,end", [(64, 577), (128, 1128), (1344, 2050)])
def test_one_range_is_the_dense_entry_on_the_slice(begin, end, pp, monkeypatch):
    """The entry has one S for queries and keys: the dense call on the slice has end - begin queries, the first rows of the same Q.
    The rows compared are those of the waves (32 consecutive queries) that lie wholly inside them: a wave decides as ONE whether a
    tile takes the exact max / rescale path (softmax_tile_zero: __any), which moves the offsets of all its rows, so a row's bits
    depend on the 31 rows it shares a wave with -- and the dense call's last wave holds copies of its last row where the ranged
    call's holds the next rows of Q."""
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    B, H, S = 1, 2, S_BIG
    q, k, v, vt, s_pad = operands(B, H, S)
    n = end - begin
    want = dense(q, k, vt, s_pad, B, H, n, begin=begin, rows=S)
    got = ranged(q, k, vt, s_pad, B, H, S, table_of([[(begin, end)]] * 9, S))
    whole = n // 32 * 32
    assert whole >= 512 and torch.equal(got[:, :whole], want[:, :whole])
    assert bool((want[:, n:] == 7.0).all()) and not bool((want[:, :n] == 7.0).all(dim=-1).any())


def _sdpa(q, k, v, mask, B, H, S):
    """fp32 softmax of the log2-unit scores (masked where `mask` is False) times v"""
    qh, kh, vh = (t.float().view(B, S, H, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * LN2
    if mask is not None:
        s = s.masked_fill(~mask.to(DEV), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, S, H * 64)


@pytest.mark.parametrize("pp", PPS)
@pytest.mark.parametrize("B,H", [(1, 2), (2, 3)])
def test_range_lists_against_masked_sdpa(B, H, pp, monkeypatch):
    """The ranged error may be FACTOR x the dense entry's error against unmasked fp32 SDPA on the same operands (relative L2)."""
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    S = S_BIG
    q, k, v, vt, s_pad = operands(B, H, S)
    kvr = table_of(LISTS, S)
    assert kvr.max_ranges == 4 and kvr.q_blocks == 9
    o = ranged(q, k, vt, s_pad, B, H, S, kvr)
    e_ranged = rel(o, _sdpa(q, k, v, ranges_to_mask(kvr), B, H, S))
    e_dense = rel(dense(q, k, vt, s_pad, B, H, S), _sdpa(q, k, v, None, B, H, S))
    print("ALG_ATTN_PP=%s B=%d H=%d: ranged vs masked fp32 SDPA %.4e, dense vs fp32 SDPA %.4e (ratio %.3f, factor %.1f)"
          % (pp, B, H, e_ranged, e_dense, e_ranged / e_dense, FACTOR))
    assert bool(torch.isfinite(o.float()).all())
    assert torch.equal(ranged(q, k, vt, s_pad, B, H, S, kvr), o)           # deterministic
    assert e_ranged <= FACTOR * e_dense, (e_ranged, e_dense)


@pytest.mark.parametrize("pp", PPS)
def test_keys_outside_the_ranges_are_not_visited(pp, monkeypatch):
    """A large FINITE value in every K row and V^T column that no range of block j touches and that shares no 64-key tile with a
    range end (the padding columns of a ragged tile are multiplied by p = 0, as in the dense contract: NaN would be the wrong
    poison) leaves the rows of block j bit for bit as they were; one key inside a range changes them -- the key that carries the
    largest weight of the block's first row in head 0 (half the rows have softmaxes sharp enough for most single keys to weigh
    nothing in bf16)."""
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    B, H, S = 1, 2, S_BIG
    q, k, v, vt, s_pad = operands(B, H, S)
    kvr = table_of(LISTS, S)
    o = ranged(q, k, vt, s_pad, B, H, S, kvr)
    perm = _perm(s_pad)
    mask = ranges_to_mask(kvr).to(DEV)
    for j, ranges in enumerate(LISTS):
        touched = torch.zeros(S, dtype=torch.bool, device=DEV)
        for b, e in ranges:
            touched[b:(e + 63) // 64 * 64] = True
        outside = (~touched).nonzero().flatten()
        rows = slice(j * 256, min((j + 1) * 256, S))
        if outside.numel():
            k2, vt2 = k.clone(), vt.clone()
            k2[:, outside] = 3.0e4
            vt2[:, :, perm[outside]] = 3.0e4
            assert torch.equal(ranged(q, k2, vt2, s_pad, B, H, S, kvr)[:, rows], o[:, rows]), j
        inside = int((q[0, j * 256, :64].float() @ k[0, :, :64].float().T).masked_fill(~mask[j * 256], float("-inf")).argmax())
        assert any(b <= inside < e for b, e in ranges)
        vt3 = vt.clone()
        vt3[:, :, perm[inside]] = 3.0e4
        assert not torch.equal(ranged(q, k, vt3, s_pad, B, H, S, kvr)[:, rows], o[:, rows]), j


def test_path_counters_count_the_tiles_of_visited_segments(monkeypatch):
    """{statement entries, tiles inside, tiles straight}: inside + straight = the tiles of the table's segments, per wave; with the
    statement off (ALG_ATTN_PP=0) nothing enters."""
    B, H, S = 1, 2, S_BIG
    q, k, v, vt, s_pad = operands(B, H, S)
    kvr = table_of(LISTS, S)
    tiles = sum((e - b + 63) // 64 for r in LISTS for b, e in r) * 8 * B * H        # eight waves per block
    for pp in PPS:
        monkeypatch.setenv("ALG_ATTN_PP", pp)
        cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        _lib.attn_path_tap(cnt)
        try:
            ranged(q, k, vt, s_pad, B, H, S, kvr)
            torch.cuda.synchronize()
        finally:
            _lib.attn_path_tap(None)
        ent, inside, straight = (int(x) for x in cnt.cpu())
        print("ALG_ATTN_PP=%s: entries %d, tiles inside %d, straight %d (segments' tiles %d)" % (pp, ent, inside, straight, tiles))
        assert inside + straight == tiles
        assert (ent == 0 and inside == 0) if pp == "0" else (ent > 0 and inside > 0)


def test_bad_scalar_arguments_are_refused_before_any_launch():
    B, H, S = 1, 1, 513
    q, k, v, vt, s_pad = operands(B, H, S)
    D = H * 64
    kvr = full_ranges(S, S)
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    lib = _lib.load_library()
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(table, max_ranges, S_=S, pitch=s_pad):
        return lib.alg_flash_attn_d64_ranges(P(q), P(k), P(vt), P(o), B, H, S_, S * D, D, D * s_pad, pitch, S * D, D, table,
                                             max_ranges, _lib._stream())

    tab = P(kvr.device_table)
    odd = ctypes.c_void_p(kvr.device_table.data_ptr() + 2)
    for args in ((tab, 0), (tab, 5), (ctypes.c_void_p(0), 1), (odd, 1), (tab, 1, 0), (tab, 1, S, 512)):
        assert call(*args) == ALG_EINVAL, args
        assert b"alg_flash_attn_d64_ranges" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                      # nothing was launched
    assert call(tab, 1) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any())
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):
        _lib.flash_attn_d64_ranges(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr.device_table)
    with pytest.raises(_lib.AlgHipError, match="built for"):
        _lib.flash_attn_d64_ranges(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, full_ranges(S - 1, S - 1))


def test_graph_capture_replays_the_ranged_launch():
    """The table is device-resident before the capture begins, the entry only enqueues: a captured launch replays to the eager bits."""
    B, H, S = 1, 2, S_BIG
    D = H * 64
    q, k, v, vt, s_pad = operands(B, H, S)
    kvr = table_of(LISTS, S)
    want = ranged(q, k, vt, s_pad, B, H, S, kvr)
    o = torch.zeros(B, S, D, dtype=BF, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.flash_attn_d64_ranges(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr)
    o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want)
