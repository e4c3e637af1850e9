"""alg_flash_attn_d64_ranges_order (attention.hip: the ranged d = 64 pipelined kernel with its workgroups in an order the host
computed), on the operands and tables of test_gpu_attn_ranges_d64.py / test_gpu_attn_ranges_heads_d64.py under ALG_ATTN_PP = 4, 8
and 0.  Every workgroup computes what it computes in alg_flash_attn_d64_ranges_heads, so for every valid order -- the kernels' own
as a table, its reverse, a random one with exiting workgroups scattered through it, and the two balancing policies -- O and the
LSE are that entry's bit for bit."""
import ctypes

import pytest
import torch

import test_gpu_attn_ranges_d64 as R
import test_gpu_attn_ranges_heads_d64 as RH
from alg_amd import _lib
from alg_amd.attn_window import LaunchOrder, balanced_order, full_ranges, unit_costs

pytestmark = pytest.mark.gpu
DEV, BF, PPS, LISTS, ALG_EINVAL = R.DEV, R.BF, R.PPS, R.LISTS, R.ALG_EINVAL
S = RH.S                          # 2050 rows: nine query blocks, the last one of two rows
Q_BLOCKS = (S + 255) // 256
# (1, 2): six lanes of the natural order hold padding only; (1, 9): more than eight heads, not a multiple of eight
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
    D = H * 64
    o = torch.full((B, S, D), 7.0, dtype=BF, device=DEV)
    l = torch.full((B, H, S), float("nan"), device=DEV) if lse else None
    _lib.flash_attn_d64_ranges_order(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr, order, lse=l)
    return o, l


@pytest.mark.parametrize("pp", PPS)
@pytest.mark.parametrize("table", ["per_head", "shared"])
@pytest.mark.parametrize("B,H", SHAPES)
def test_every_order_gives_the_bits_of_the_heads_entry(B, H, table, pp, monkeypatch):
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    q, k, v, vt, s_pad = R.operands(B, H, S)
    kvr = RH.heads_table(H) if table == "per_head" else R.table_of(LISTS, S)
    want_o, want_lse = RH.run(q, k, vt, s_pad, B, H, kvr, lse=True)
    want_plain = RH.run(q, k, vt, s_pad, B, H, kvr)       # (the launch without lse runs other instantiations)
    assert not bool((want_o == 7.0).all())
    for name in ORDERS:
        order = make_order(name, kvr, B, H)
        o, lse = run_order(q, k, vt, s_pad, B, H, kvr, order, True)
        assert torch.equal(o, want_o), name
        assert torch.equal(lse, want_lse), name          # (NaN-prefilled: a query left unwritten fails this)
        o, _ = run_order(q, k, vt, s_pad, B, H, kvr, order, False)
        assert torch.equal(o, want_plain), name


def test_graph_capture_replays_the_ordered_launch():
    """The order and the table are device-resident before the capture begins, the entry only enqueues (single stream)."""
    B, H = 2, 3
    D = H * 64
    q, k, v, vt, s_pad = R.operands(B, H, S)
    kvr = RH.heads_table(H)
    order = make_order("units", kvr, B, H)
    want_o, want_lse = run_order(q, k, vt, s_pad, B, H, kvr, order, True)
    assert torch.equal(want_o, RH.run(q, k, vt, s_pad, B, H, kvr, lse=True)[0])
    o = torch.zeros(B, S, D, dtype=BF, device=DEV)
    lse = torch.zeros(B, H, S, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.flash_attn_d64_ranges_order(q, k, vt, o, B, H, S, S * D, D, D * s_pad, s_pad, S * D, D, kvr, order, lse=lse)
    o.zero_()
    lse.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want_o) and torch.equal(lse, want_lse)


def test_bad_arguments_are_refused_before_any_launch():
    B, H, S_ = 1, 2, S
    q, k, v, vt, s_pad = R.operands(B, H, S_)
    D = H * 64
    kvr = full_ranges(S_, S_)
    table = kvr.device_table
    good = balanced_order(unit_costs(kvr, B, H), "natural", heads=H)
    order = torch.cat([good.device_table, torch.full((8,), -1, dtype=torch.int32, device=DEV)])     # 80 entries, 18 units
    o = torch.full((B, S_, D), 7.0, dtype=BF, device=DEV)
    lib = _lib.load_library()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(order_p, order_len):
        return lib.alg_flash_attn_d64_ranges_order(P(q), P(k), P(vt), P(o), B, H, S_, S_ * D, D, D * s_pad, s_pad, S_ * D, D,
                                                   P(table), 1, 1, None, order_p, order_len, _lib._stream())

    # null order, misaligned order, order_len % 8 != 0, order_len too small (18 units), order_len <= 0
    for args in ((None, 80), (P(order, 2), 72), (P(order), 76), (P(order), 18), (P(order), 16), (P(order), 0), (P(order), -8)):
        assert call(*args) == ALG_EINVAL, args[1]
        assert b"alg_flash_attn_d64_ranges_order" in lib.alg_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                       # nothing was launched
    assert call(P(order), 80) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).any())
    A = (q, k, vt, o, B, H, S_, S_ * D, D, D * s_pad, s_pad, S_ * D, D, kvr)
    with pytest.raises(_lib.AlgHipError, match="LaunchOrder"):
        _lib.flash_attn_d64_ranges_order(*A, order)
    other = balanced_order(unit_costs(full_ranges(S_ + 256, S_ + 256), B, H), "natural", heads=H)     # two query blocks
    with pytest.raises(_lib.AlgHipError, match="built for"):
        _lib.flash_attn_d64_ranges_order(*A, other)
    with pytest.raises(_lib.AlgHipError, match="built for"):
        _lib.flash_attn_d64_ranges_order(*A, balanced_order(unit_costs(kvr, B, 3), "natural", heads=3))
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):
        _lib.flash_attn_d64_ranges_order(*A[:-1], table, good)
