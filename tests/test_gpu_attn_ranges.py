"""alg_flash_attn_d128_ranges (attention128_q64.hip: each block of 256 queries attends to a short list of key ranges) on the
operands of test_flash_attn_d128_q64_kernel -- half the queries x 6, one dominating key -- with the statement on
(ALG_ATTN128_Q64=2) and with the frame's C++ tile body on its own (=3): the full range IS the dense kernel, one range IS the dense
kernel on the slice, range lists against masked fp32 SDPA, and keys outside the ranges are not visited."""
import ctypes
import math

import pytest
import torch

from alg_amd import _lib
from alg_amd.attn_window import KvRanges, full_ranges, ranges_to_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SCALE = 1.0 / math.sqrt(128)
FLAGS = ("2", "3")
ALG_EINVAL = -1

# one table row per block of 256 queries (Sq = 1300, Skv = 2050): segment lengths 1, 2, 63, 64, 65, 66; segments under four tiles
# and of nine tiles and more with every remainder of the four-tile unroll (2050: 33 tiles, 1410: 23, 576: 9, 1025: 17 -- and 200:
# 4, 66: 2); the dominating key 683 lies inside the ranges of blocks 0 and 1 and outside those of blocks 2 .. 5
LISTS = [
    [(0, 2050)],
    [(0, 64), (640, 2050)],
    [(0, 1), (64, 127), (1024, 1600)],
    [(0, 200), (256, 321), (960, 1985)],
    [(1984, 2050)],
    [(0, 64), (128, 192), (256, 320), (2048, 2050)],
]


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF).to(DEV)


def _perm(n):
    return torch.tensor([(i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1) for i in range(n)], device=DEV)


def make_vt(v, s_pad):
    """v [B, S, H*128] -> V^T [B, H*128, s_pad] with kv index bits 2 and 3 swapped, zero padded."""
    B, S, D = v.shape
    vt = torch.zeros(B, D, s_pad, dtype=BF, device=DEV)
    vt[:, :, _perm(s_pad)[:S]] = v.transpose(1, 2)
    return vt


def operands(B, H, Sq, Skv):
    D = H * 128
    q, k, v = _rand((B, Sq, D), 11), _rand((B, Skv, D), 12), _rand((B, Skv, D), 13)
    q[:, : Sq // 2] *= 6.0
    k[:, Skv // 3] *= 8.0
    s_pad = (Skv + 63) // 64 * 64
    return q, k, v, make_vt(v, s_pad), s_pad


def dense(q, k, vt, s_pad, B, H, Sq, Skv, begin=0, Skv_rows=None):
    """flash_attn_d128 on the keys [begin, begin + Skv) of the buffers (k / vt hold Skv_rows keys)."""
    D = H * 128
    rows = Skv if Skv_rows is None else Skv_rows
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    _lib.flash_attn_d128(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, rows * D, D, D * s_pad, s_pad, Sq * D, D, SCALE,
                         k_off=begin * D, vt_off=begin)
    return o


def ranged(q, k, vt, s_pad, B, H, Sq, Skv, kvr):
    D = H * 128
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    _lib.flash_attn_d128_ranges(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE, kvr)
    return o


def table_of(lists, Sq, Skv):
    n = max(len(r) for r in lists)
    t = torch.zeros(len(lists), n, 2, dtype=torch.int32)
    for j, r in enumerate(lists):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return KvRanges(t, Skv, Sq)


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("B,H,Sq,Skv", [(1, 2, 700, 1024), (2, 3, 257, 1000), (1, 1, 256, 513), (1, 2, 1300, 2050)])
def test_full_range_is_the_dense_kernel(B, H, Sq, Skv, flag, monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    q, k, v, vt, s_pad = operands(B, H, Sq, Skv)
    want = dense(q, k, vt, s_pad, B, H, Sq, Skv)
    got = ranged(q, k, vt, s_pad, B, H, Sq, Skv, full_ranges(Sq, Skv))
    assert torch.equal(got, want)


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("begin,end", [(64, 577), (128, 1128)])
def test_one_range_is_the_dense_kernel_on_the_slice(begin, end, flag, monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    B, H, Sq, Skv = 1, 2, 1300, 2050
    q, k, v, vt, s_pad = operands(B, H, Sq, Skv)
    want = dense(q, k, vt, s_pad, B, H, Sq, end - begin, begin=begin, Skv_rows=Skv)
    got = ranged(q, k, vt, s_pad, B, H, Sq, Skv, table_of([[(begin, end)]] * 6, Sq, Skv))
    assert torch.equal(got, want)


def _masked_sdpa(q, k, v, mask, B, H, Sq, Skv):
    D = H * 128
    qh = q.float().view(B, Sq, H, 128).transpose(1, 2)
    kh = k.float().view(B, Skv, H, 128).transpose(1, 2)
    vh = v.float().view(B, Skv, H, 128).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2) * SCALE).masked_fill(~mask.to(DEV), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, Sq, D)


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("B,H", [(1, 2), (2, 3)])      # (2, 3): six (batch, head) panels on eight XCD slots, two of them idle
def test_range_lists_against_masked_sdpa_and_outside_keys_are_not_visited(B, H, flag, monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    Sq, Skv = 1300, 2050
    q, k, v, vt, s_pad = operands(B, H, Sq, Skv)
    kvr = table_of(LISTS, Sq, Skv)
    assert kvr.max_ranges == 4 and kvr.q_blocks == 6
    o = ranged(q, k, vt, s_pad, B, H, Sq, Skv, kvr)
    ref = _masked_sdpa(q, k, v, ranges_to_mask(kvr), B, H, Sq, Skv)
    err = (o.float() - ref).abs()
    print("ranges vs masked fp32 SDPA: max %.3e mean %.3e" % (err.max().item(), err.mean().item()))
    assert bool(torch.isfinite(o.float()).all())
    assert err.max().item() < 3e-2
    assert err.mean().item() < 2e-3
    assert torch.equal(ranged(q, k, vt, s_pad, B, H, Sq, Skv, kvr), o)           # deterministic

    # keys outside the ranges are not visited: a large FINITE value in every K row and V^T column that no range of block j
    # touches and that shares no 64-key tile with a range end (the padding columns of a ragged tile are multiplied by p = 0, as
    # in the dense contract: NaN would be the wrong poison) leaves the rows of block j bit for bit as they were ...
    perm = _perm(s_pad)
    for j, ranges in enumerate(LISTS):
        touched = torch.zeros(Skv, dtype=torch.bool, device=DEV)
        for b, e in ranges:
            touched[b:(e + 63) // 64 * 64] = True
        outside = (~touched).nonzero().flatten()
        rows = slice(j * 256, min((j + 1) * 256, Sq))
        if outside.numel():
            k2, vt2 = k.clone(), vt.clone()
            k2[:, outside] = 3.0e4
            vt2[:, :, perm[outside]] = 3.0e4
            assert torch.equal(ranged(q, k2, vt2, s_pad, B, H, Sq, Skv, kvr)[:, rows], o[:, rows]), j
        # ... and one key inside a range changes them
        inside = ranges[-1][0]
        vt3 = vt.clone()
        vt3[:, :, perm[inside]] = 3.0e4
        assert not torch.equal(ranged(q, k, vt3, s_pad, B, H, Sq, Skv, kvr)[:, rows], o[:, rows]), j


def test_bad_scalar_arguments_are_refused_before_any_launch():
    B, H, Sq, Skv = 1, 1, 256, 513
    q, k, v, vt, s_pad = operands(B, H, Sq, Skv)
    D = H * 128
    kvr = full_ranges(Sq, Skv)
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    lib = _lib.load_library()
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(table, max_ranges):
        return lib.alg_flash_attn_d128_ranges(P(q), P(k), P(vt), P(o), B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad,
                                              Sq * D, D, SCALE, table, max_ranges, _lib._stream())

    for table, n in ((P(kvr.device_table), 0), (P(kvr.device_table), 5), (ctypes.c_void_p(0), 1)):
        assert call(table, n) == ALG_EINVAL
        assert b"alg_flash_attn_d128_ranges" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                      # nothing was launched
    assert call(P(kvr.device_table), 1) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any())
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):
        _lib.flash_attn_d128_ranges(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE,
                                    kvr.device_table)


def test_graph_capture_replays_the_ranged_launch():
    """The table is device-resident before the capture begins, the entry only enqueues: a captured launch replays to the eager bits."""
    B, H, Sq, Skv = 1, 2, 1300, 2050
    D = H * 128
    q, k, v, vt, s_pad = operands(B, H, Sq, Skv)
    kvr = table_of(LISTS, Sq, Skv)
    want = ranged(q, k, vt, s_pad, B, H, Sq, Skv, kvr)
    o = torch.zeros(B, Sq, D, dtype=BF, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.flash_attn_d128_ranges(q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE, kvr)
    o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want)
