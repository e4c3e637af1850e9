"""alg_flash_attn_d128_ranges_order (attention128_q64.hip: the ranged kernel with its workgroups in an order the host computed), on
the operands and tables of test_gpu_attn_ranges.py / test_gpu_attn_ranges_heads.py, with the statement on (ALG_ATTN128_Q64=2) and
with the frame's C++ tile body on its own (=3).  Every workgroup computes what it computes in alg_flash_attn_d128_ranges_heads, so
for every valid order -- the kernels' own as a table, its reverse, a random one with exiting workgroups scattered through it, and
the two balancing policies -- O and the LSE are that entry's bit for bit."""
import ctypes

import pytest
import torch

import test_gpu_attn_ranges as R
import test_gpu_attn_ranges_heads as RH
from alg_amd import _lib
from alg_amd.attn_window import LaunchOrder, balanced_order, full_ranges, unit_costs

pytestmark = pytest.mark.gpu
DEV, BF, SCALE, FLAGS, LISTS, ALG_EINVAL = R.DEV, R.BF, R.SCALE, R.FLAGS, R.LISTS, R.ALG_EINVAL
SQ, SKV = RH.SQ, RH.SKV          # 1300 queries: six blocks, the last one of 20 rows
Q_BLOCKS = (SQ + 255) // 256
# (1, 2): fewer units' heads than lanes -- six lanes of the natural order hold padding only; (1, 9): more than eight heads, not a
# multiple of eight
SHAPES = [(1, 2), (2, 3), (1, 9)]
ORDERS = ("natural", "reversed", "random", "lanes", "units")


def make_order(name, kvr, B, H):
    costs = unit_costs(kvr, B, H)
    if name in ("natural", "lanes", "units"):
        return balanced_order(costs, name, heads=H)
    natural = balanced_order(costs, "natural", heads=H).order
    if name == "reversed":
        return LaunchOrder(natural.flip(0), B, H, Q_BLOCKS)
    units = B * H * Q_BLOCKS
    n = 8 * ((B * H + 7) // 8 * Q_BLOCKS + 2)         # 8 x (the longest lane of the natural order + 2)
    g = torch.Generator().manual_seed(1000 * B + H)
    order = torch.full((n,), -1, dtype=torch.int32)
    order[torch.randperm(n, generator=g)[:units]] = torch.randperm(units, generator=g).to(torch.int32)
    return LaunchOrder(order, B, H, Q_BLOCKS)


def run_order(q, k, vt, s_pad, B, H, kvr, order, lse):
    D = H * 128
    o = torch.full((B, SQ, D), 7.0, dtype=BF, device=DEV)
    l = torch.full((B, H, SQ), float("nan"), device=DEV) if lse else None
    _lib.flash_attn_d128_ranges_order(q, k, vt, o, B, H, SQ, SKV, SQ * D, D, SKV * D, D, D * s_pad, s_pad, SQ * D, D, SCALE, kvr,
                                      order, lse=l)
    return o, l


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("table", ["per_head", "shared"])
@pytest.mark.parametrize("B,H", SHAPES)
def test_every_order_gives_the_bits_of_the_heads_entry(B, H, table, flag, monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    q, k, v, vt, s_pad = RH.operands(B, H)
    kvr = RH.heads_table(H) if table == "per_head" else R.table_of(LISTS, SQ, SKV)
    want_o, want_lse = RH.run(q, k, vt, s_pad, B, H, SQ, SKV, kvr, lse=True)
    assert not bool((want_o == 7.0).all())
    for name in ORDERS:
        order = make_order(name, kvr, B, H)
        o, lse = run_order(q, k, vt, s_pad, B, H, kvr, order, True)
        assert torch.equal(o, want_o), name
        assert torch.equal(lse, want_lse), name          # (NaN-prefilled: a query left unwritten fails this)
        o, _ = run_order(q, k, vt, s_pad, B, H, kvr, order, False)
        assert torch.equal(o, want_o), name


def test_graph_capture_replays_the_ordered_launch():
    """The order and the table are device-resident before the capture begins, the entry only enqueues (single stream)."""
    B, H = 2, 3
    D = H * 128
    q, k, v, vt, s_pad = RH.operands(B, H)
    kvr = RH.heads_table(H)
    order = make_order("lanes", kvr, B, H)
    want_o, want_lse = run_order(q, k, vt, s_pad, B, H, kvr, order, True)
    assert torch.equal(want_o, RH.run(q, k, vt, s_pad, B, H, SQ, SKV, kvr))
    o = torch.zeros(B, SQ, D, dtype=BF, device=DEV)
    lse = torch.zeros(B, H, SQ, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.flash_attn_d128_ranges_order(q, k, vt, o, B, H, SQ, SKV, SQ * D, D, SKV * D, D, D * s_pad, s_pad, SQ * D, D, SCALE, kvr,
                                          order, lse=lse)
    o.zero_()
    lse.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want_o) and torch.equal(lse, want_lse)


def test_bad_arguments_are_refused_before_any_launch():
    B, H, Sq, Skv = 1, 2, SQ, SKV
    q, k, v, vt, s_pad = RH.operands(B, H)
    D = H * 128
    kvr = full_ranges(Sq, Skv)
    table = kvr.device_table
    good = balanced_order(unit_costs(kvr, B, H), "natural", heads=H)
    order = torch.cat([good.device_table, torch.full((8,), -1, dtype=torch.int32, device=DEV)])     # 56 entries, 12 units
    o = torch.full((B, Sq, D), 7.0, dtype=BF, device=DEV)
    lib = _lib.load_library()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(order_p, order_len):
        return lib.alg_flash_attn_d128_ranges_order(P(q), P(k), P(vt), P(o), B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad,
                                                    Sq * D, D, SCALE, P(table), 1, 1, None, order_p, order_len, _lib._stream())

    # null order, misaligned order, order_len % 8 != 0, order_len too small (12 units), order_len <= 0
    for args in ((None, 56), (P(order, 2), 48), (P(order), 52), (P(order), 12), (P(order), 8), (P(order), 0), (P(order), -8)):
        assert call(*args) == ALG_EINVAL, args[1]
        assert b"alg_flash_attn_d128_ranges_order" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                       # nothing was launched
    assert call(P(order), 56) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any())
    A = (q, k, vt, o, B, H, Sq, Skv, Sq * D, D, Skv * D, D, D * s_pad, s_pad, Sq * D, D, SCALE, kvr)
    with pytest.raises(_lib.AlgHipError, match="LaunchOrder"):
        _lib.flash_attn_d128_ranges_order(*A, order)
    with pytest.raises(_lib.AlgHipError, match="LaunchOrder"):
        _lib.flash_attn_d128_ranges_order(*A, good.order)
    other = balanced_order(unit_costs(full_ranges(Sq + 256, Skv), B, H), "natural", heads=H)       # two query blocks
    with pytest.raises(_lib.AlgHipError, match="built for"):
        _lib.flash_attn_d128_ranges_order(*A, other)
    with pytest.raises(_lib.AlgHipError, match="built for"):
        _lib.flash_attn_d128_ranges_order(*A, balanced_order(unit_costs(kvr, B, 3), "natural", heads=3))
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):
        _lib.flash_attn_d128_ranges_order(*A[:-1], table, good)
