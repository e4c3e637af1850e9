"""The dense attention entries (alg_flash_attn_d64[_ex], alg_flash_attn_d128[_ex], alg_flash_attn_d128_dual) on strided, offset
and minimally padded operands (tests/helpers/attn_arena.py: the product's packed layout and a loose one, inside guarded arenas,
under a friendly fill of zeros and a hostile one of NaN with finite random V^T padding columns).  Every kernel route, under each
non-compact layout and both fills:

  1. layout independence: the output is BIT FOR BIT the same entry's output on the compact copies -- the plans are functions of the
     shape and the options, and the arithmetic of a (batch, head, query block) does not depend on addresses;
  2. fill independence: the hostile and the friendly outputs are bit-equal and finite (K rows behind Skv, Q rows behind Sq, the
     V^T padding columns "multiplied by p = 0", whatever a prefetch past the panel picks up);
  3. footprint: every element of the o arena outside the B * Sq * H * d the call may write still holds the canary -- rows >= Sq,
     columns outside the head windows, the idle workgroups of the grid rounded up to 8;
  4. reference: float64 SDPA on the compact copies, N(0, 1) inputs and scale d ** -0.5, within the bounds the kernel tests already
     use for that distribution (d = 128: max < 2e-2, mean < 2e-3, test_flash_attn_d128_matches_sdpa; d = 64: max <= 2e-2,
     test_flash_attention_vs_sdpa; the pre-scaled d = 64 call in log2 units as test_pipelined_attention_kernel does it).

tests/test_attn_arena_cpu.py shows on an emulation that these assertions catch the ways such addressing goes wrong."""
import math

import pytest
import torch

from alg_amd import _lib
from helpers import attn_arena as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
LAYOUTS = ["packed", "loose"]
LOG2E = 1.4426950408889634

_BASE = {}     # (route, shape) -> (compact q, k, v, the entry's output on them, the float64 reference): computed once, never written


def call128(ar, o_full, causal=False):
    _lib.flash_attn_d128(ar.q.view, ar.k.view, ar.vt.view, ar.o_view(o_full), ar.B, ar.H, ar.Sq, ar.Skv, ar.q.bs, ar.q.rs, ar.k.bs,
                         ar.k.rs, ar.vt.bs, ar.vt.rs, ar.o.bs, ar.o.rs, 128 ** -0.5, kv_group=ar.kv_group, causal=causal)


def call64(ar, o_full, prescaled):
    _lib.flash_attn_d64(ar.q.view, ar.k.view, ar.vt.view, ar.o_view(o_full), ar.B, ar.H, ar.Sq, ar.q.bs, ar.q.rs, ar.vt.bs, ar.vt.rs,
                        ar.o.bs, ar.o.rs, 0.125, q_prescaled=prescaled)


def drive(key, d, B, H, Sq, Skv, layout, call, group=1, ref_fn=None, make_q=None, bounds=None):
    """Assertions 1 to 4 (4 when ref_fn is given) for one call under one layout and both fills; the compact run and the reference
    are shared by the layouts of a (route, shape)."""
    if key not in _BASE:
        q = make_q() if make_q else None
        base = A.build(d, B, H, Sq, Skv, group, "compact", "friendly", DEV, q=q, seed=Sq + 7 * Skv + H)
        o = base.fresh_o()
        call(base, o)
        A.assert_footprint(base, o)
        _BASE[key] = (base.q_c, base.k_c, base.v_c, base.extract(o), ref_fn(base) if ref_fn else None)
    q, k, v, baseline, ref = _BASE[key]
    runs = []
    for fill in A.FILLS:
        ar = A.build(d, B, H, Sq, Skv, group, layout, fill, DEV, q=q, k=k, v=v, seed=Sq + 7 * Skv + H)
        o = ar.fresh_o()
        call(ar, o)
        runs += [ar, o]
    torch.cuda.synchronize()
    if bounds is None:
        bounds = dict(max_bound=2e-2, mean_bound=2e-3, strict=True) if d == 128 else dict(max_bound=2e-2, strict=False)
    failed = A.failures(*runs, baseline, ref, **bounds)
    assert failed == {}, failed


def ref128(causal=False):
    return lambda base: A.sdpa64(base.q_c, base.k_c, base.v_c, 128 ** -0.5, causal, base.kv_group)


# ---------------------------------------------------------------------------------------------------------------------- d = 128
def _base_route(monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", "0")
    monkeypatch.setenv("ALG_ATTN128_PIPE", "0")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B,H,Sq,Skv", [(2, 3, 257, 65), (1, 1, 31, 64), (1, 2, 300, 270)])
def test_d128_base_kernel(B, H, Sq, Skv, layout, monkeypatch):
    """attention128.hip: more than one query block with a one-key last tile; less than a wave of queries on exactly one tile;
    HunyuanVideo's form, Sq > Skv, where the packed buffer has K rows behind Skv that belong to the fill."""
    _base_route(monkeypatch)
    drive(("base", B, H, Sq, Skv), 128, B, H, Sq, Skv, layout, call128, ref_fn=ref128())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("L,heads,kv_heads", [(333, 4, 2), (64, 8, 2), (300, 4, 1)])
def test_d128_base_kernel_causal_grouped(L, heads, kv_heads, layout, monkeypatch):
    """alg_flash_attn_d128_ex as the Llama tower calls it: causal, kv_group query heads on one K / V head, Q and K out of LLaVA's
    [L][D + KV] buffer under the packed layout."""
    _base_route(monkeypatch)
    drive(("causal", L, heads, kv_heads), 128, 1, heads, L, L, layout, lambda ar, o: call128(ar, o, causal=True),
          group=heads // kv_heads, ref_fn=ref128(causal=True))


# 12, 14, 15 and 18 tiles: 0 to 3 tiles behind the four-tile groups; full, one-key and 63-key tails
PIPE_SHAPES = [(1, 1, 64, 768), (2, 3, 129, 833), (1, 1, 300, 959), (2, 3, 64, 1100), (1, 1, 129, 1100)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B,H,Sq,Skv", PIPE_SHAPES)
def test_d128_pipelined_kernel(B, H, Sq, Skv, layout, monkeypatch):
    """attention128_pipe.hip (from 12 KV tiles on): its statement prefetches K and V^T past the tile it computes."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "0")
    monkeypatch.setenv("ALG_ATTN128_PIPE", "1")
    drive(("pipe", B, H, Sq, Skv), 128, B, H, Sq, Skv, layout, call128, ref_fn=ref128())


# 8 to 11 tiles; tails: full, one key (the second half-tile entirely masked), 63 keys, 60 keys
Q64_SHAPES = [(1, 1, 64, 512), (2, 3, 257, 513), (1, 1, 300, 575), (1, 1, 257, 640), (2, 3, 300, 700)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("flag", ["2", "3"], ids=["statement", "frame"])
@pytest.mark.parametrize("B,H,Sq,Skv", Q64_SHAPES)
def test_d128_q64_kernel(B, H, Sq, Skv, flag, layout, monkeypatch):
    """attention128_q64.hip forced onto every call of >= 8 KV tiles: with its statement (2) and the frame's C++ tile body alone (3)."""
    monkeypatch.setenv("ALG_ATTN128_Q64", flag)
    drive(("q64", flag, B, H, Sq, Skv), 128, B, H, Sq, Skv, layout, call128, ref_fn=ref128())


@pytest.mark.parametrize("layouts", [("packed", "loose"), ("loose", "packed")], ids=["packed+loose", "loose+packed"])
@pytest.mark.parametrize("B,H,Sq,Skv,Skv2", [(2, 3, 300, 257, 70), (1, 1, 31, 64, 1)])
def test_d128_dual(B, H, Sq, Skv, Skv2, layouts):
    """alg_flash_attn_d128_dual with the two key / value sets in different layouts: q and o follow the first set's layout.  The
    reference is bf16(bf16(a) + bf16(b)) of two float64 SDPAs."""
    scale = 128 ** -0.5

    def build(layout1, layout2, fill, q=None, kv=None):
        k, v, k2, v2 = kv if kv else (None,) * 4
        a1 = A.build(128, B, H, Sq, Skv, 1, layout1, fill, DEV, q=q, k=k, v=v, seed=Sq + Skv)
        a2 = A.build(128, B, H, Sq, Skv2, 1, layout2, fill, DEV, q=a1.q_c, k=k2, v=v2, seed=Sq + Skv2 + 1)
        return a1, a2

    def call(a1, a2, o_full):
        _lib.flash_attn_d128_dual(a1.q.view, a1.k.view, a1.vt.view, Skv, a1.k.bs, a1.k.rs, a1.vt.bs, a1.vt.rs, a2.k.view, a2.vt.view,
                                  Skv2, a2.k.bs, a2.k.rs, a2.vt.bs, a2.vt.rs, a1.o_view(o_full), B, H, Sq, a1.q.bs, a1.q.rs, a1.o.bs,
                                  a1.o.rs, scale)

    key = ("dual", B, H, Sq, Skv, Skv2)
    if key not in _BASE:
        a1, a2 = build("compact", "compact", "friendly")
        o = a1.fresh_o()
        call(a1, a2, o)
        A.assert_footprint(a1, o)
        ra, rb = A.sdpa64(a1.q_c, a1.k_c, a1.v_c, scale), A.sdpa64(a1.q_c, a2.k_c, a2.v_c, scale)
        ref = (ra.to(BF).float() + rb.to(BF).float()).to(BF).double()
        _BASE[key] = (a1.q_c, (a1.k_c, a1.v_c, a2.k_c, a2.v_c), a1.extract(o), ref)
    q, kv, baseline, ref = _BASE[key]
    runs = []
    for fill in A.FILLS:
        a1, a2 = build(layouts[0], layouts[1], fill, q, kv)
        o = a1.fresh_o()
        call(a1, a2, o)
        runs += [a1, o]
    torch.cuda.synchronize()
    failed = A.failures(*runs, baseline, ref, max_bound=2e-2, mean_bound=2e-3, strict=True)
    assert failed == {}, failed


# ----------------------------------------------------------------------------------------------------------------------- d = 64
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", ["1", "33"])
@pytest.mark.parametrize("B,S,H", [(1, 17, 1), (1, 65, 3), (2, 273, 9)])
def test_d64_unprescaled(B, S, H, variant, layout, monkeypatch):
    """alg_flash_attn_d64 under both softmax forms (33 = the lazy running max, 1 = the exact one).  At S = 17 the packed layout's
    V^T pitch is 64 where the compact run's is 128."""
    monkeypatch.setenv("ALG_ATTN_VARIANT", variant)
    drive(("d64", variant, B, S, H), 64, B, H, S, S, layout, lambda ar, o: call64(ar, o, False),
          ref_fn=lambda base: A.sdpa64(base.q_c, base.k_c, base.v_c, 0.125))


def _prescaled_q(B, S, H):
    def make():
        g = torch.Generator().manual_seed(S + H)
        return (torch.randn(B, S, H, 64, generator=g).to(BF).float() * (0.125 * LOG2E)).to(BF)   # what alg_qk_norm_rope_scaled leaves
    return make


def _ref_log2(base):
    return A.sdpa64(base.q_c, base.k_c, base.v_c, math.log(2.0))      # the scores are in log2 units


# 9, 11, 13 and 17 KV tiles -- odd counts: a V^T pitch of 64 is not one of 128 -- and S = 1000 (16 tiles, a 40-key tail)
PRESCALED_SHAPES = [(1, 2, 575), (2, 3, 700), (8, 1, 832), (2, 3, 1087), (1, 2, 1000)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pp", ["0", "4", "7", "8"])
@pytest.mark.parametrize("B,H,S", PRESCALED_SHAPES)
def test_d64_prescaled(B, H, S, pp, layout, monkeypatch):
    """alg_flash_attn_d64_ex(ALG_ATTN_Q_PRESCALED) under every main-launch form: the straight loop (0), the zero-offset statement on
    32x32x16 (4) and on 16x16x32 (7), the any-offset statement (8).  The packed layout's V^T pitch is exactly ceil(S / 64) * 64
    with an odd tile count: the last tile of the last row ends where the pitch ends."""
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    drive(("pp", pp, B, H, S), 64, B, H, S, S, layout, lambda ar, o: call64(ar, o, True), ref_fn=_ref_log2, make_q=_prescaled_q(B, S, H))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pp", ["0", "4"])
def test_d64_split_kv_tail(pp, layout, monkeypatch):
    """The smallest shape with a split-KV tail (test_split_kv_tail_at_small_sizes has its reference): the chunk workgroups and the
    merge kernel address the same operands, through the workspace.  Assertions 1 to 3."""
    B, S, H = 1, 4090, 40
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    assert _lib.load_library().alg_flash_attn_d64_workspace_bytes(B, H, S, _lib.ATTN_Q_PRESCALED) > 0
    drive(("tail", pp), 64, B, H, S, S, layout, lambda ar, o: call64(ar, o, True), make_q=_prescaled_q(B, S, H))
