"""tests/helpers/attn_arena.py has teeth: a torch emulation of a strided attention call -- it reads the arenas with as_strided
exactly as include/alg_hip.h describes the operands, applies the bit-2/3 perm on V^T, clamps the K rows of the ragged last tile and
writes the head windows of o -- drives the four assertions of tests/test_gpu_attn_operands.py (layout independence bit for bit,
fill independence, footprint, reference).  The faithful emulation passes every layout and fill; each mutant -- the ways a kernel
addressing such operands goes wrong -- fails the assertion named for it."""
import pytest
import torch

from helpers import attn_arena as A

# (d, B, H, Sq, Skv, kv_group, causal): a ragged last tile everywhere (the mutants of that tile need one), Sq > Skv and Sq < Skv,
# more than one batch item and head, grouped and causal
SHAPES = [(128, 2, 3, 70, 65, 1, False), (128, 1, 2, 40, 130, 1, False), (128, 1, 4, 77, 77, 2, True), (64, 2, 3, 100, 100, 1, False)]
IDS = ["d128", "d128-long-kv", "d128-grouped-causal", "d64"]
NONCOMPACT = [l for l in A.LAYOUTS if l != "compact"]


def emulate(ar, o_full, scale, causal=False, mutant=None):
    """softmax(q k^T * scale) v out of the arenas of `ar` into o_full, float64 inside, one (batch, head) at a time over whole
    64-key tiles: the keys of the last tile behind Skv read the clamped row Skv - 1 and are masked, the V^T padding columns are
    read and multiplied by p = 0."""
    d, Skv, Sq, pad = ar.d, ar.Skv, ar.Sq, A.ceil64(ar.Skv)
    pi = A.perm_index(pad)
    o_rs = ar.H * d if mutant == "o_rs" else ar.o.rs
    vt_off = 0 if mutant == "vt_off" else ar.vt.off
    rows = torch.arange(pad).clamp(max=Skv - 1)
    for b in range(ar.B):
        for h in range(ar.H):
            hk = h // ar.kv_group
            Q = torch.as_strided(ar.q.full, (Sq, d), (ar.q.rs, 1), ar.q.off + b * ar.q.bs + h * d).double()
            K = torch.as_strided(ar.k.full, (Skv, d), (ar.k.rs, 1), ar.k.off + b * ar.k.bs + hk * d).double()[rows]
            VT = torch.as_strided(ar.vt.full, (d, pad), (ar.vt.rs, 1), vt_off + b * ar.vt.bs + hk * d * ar.vt.rs).double()
            sc = Q @ K.T * scale
            masked = torch.arange(pad)[None, :] >= (Skv + 1 if mutant == "key_skv" else Skv)
            if causal:
                masked = masked | (torch.arange(pad)[None, :] > torch.arange(Sq)[:, None])
            p = torch.softmax(sc.masked_fill(masked, -float("inf")), dim=-1)
            out = p @ VT[:, pi].T                     # key s sits at column perm(s); p = 0 on the padding columns
            if mutant == "vt_col_pad" and h == ar.H - 1:    # the tile behind the last one, for the last V^T row of the batch item
                out[:, d - 1] += 0.0 * ar.vt.full[vt_off + b * ar.vt.bs + (hk * d + d - 1) * ar.vt.rs + pad].double()
            n_rows = Sq + 1 if mutant == "row_sq" and (b, h) == (0, 0) else Sq
            n_cols = d + 8 if mutant == "cols_past" and (b, h) == (0, ar.H - 1) else d
            src = torch.zeros(n_rows, n_cols, dtype=torch.float64)
            src[:Sq, :d] = out
            torch.as_strided(o_full, (n_rows, n_cols), (o_rs, 1), ar.o.off + b * ar.o.bs + h * d).copy_(src.to(A.BF))
    return o_full


def run(shape, layout, mutant=None):
    d, B, H, Sq, Skv, group, causal = shape
    scale = d ** -0.5
    base = A.build(d, B, H, Sq, Skv, group, "compact", "friendly", seed=Sq + Skv)
    baseline = base.extract(emulate(base, base.fresh_o(), scale, causal))
    ref = A.sdpa64(base.q_c, base.k_c, base.v_c, scale, causal, group)
    ar_f = A.build(d, B, H, Sq, Skv, group, layout, "friendly", seed=Sq + Skv)
    ar_h = A.build(d, B, H, Sq, Skv, group, layout, "hostile", seed=Sq + Skv)
    o_f = emulate(ar_f, ar_f.fresh_o(), scale, causal, mutant)
    o_h = emulate(ar_h, ar_h.fresh_o(), scale, causal, mutant)
    return A.failures(ar_f, o_f, ar_h, o_h, baseline, ref, 2e-2, 2e-3 if d == 128 else None, strict=d == 128)


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_faithful_emulation_passes_every_layout_and_fill(shape, layout):
    assert run(shape, layout) == {}


# the assertion that has to catch each mutant (others may fail too)
MUTANTS = [("row_sq", "footprint"),        # it writes row Sq of one head
           ("cols_past", "footprint"),     # it writes 8 columns past the head window
           ("key_skv", "fill"),            # it includes key Skv, the clamped row, unmasked in the last tile: V^T's padding shows
           ("vt_col_pad", "fill"),         # it reads V^T column ceil(Skv / 64) * 64 of the last row: NaN x 0
           ("o_rs", "footprint"),          # it treats o_rs as H * d
           ("vt_off", "layout")]           # it ignores vt_off


# (under the causal mask no query sees key Skv = Sq: that mutant has nothing to show there)
@pytest.mark.parametrize("mutant,caught_by", MUTANTS)
@pytest.mark.parametrize("layout", NONCOMPACT)
@pytest.mark.parametrize("shape", [s for s in SHAPES if not s[6]], ids=[i for s, i in zip(SHAPES, IDS) if not s[6]])
def test_every_mutant_fails_the_assertion_named_for_it(shape, layout, mutant, caught_by):
    failed = run(shape, layout, mutant)
    assert caught_by in failed, (mutant, failed)
    if mutant == "o_rs":
        assert "layout" in failed, failed


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("fill", A.FILLS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_mask_marks_exactly_the_output_elements(shape, layout, fill):
    d, B, H, Sq, Skv, group, _ = shape
    ar = A.build(d, B, H, Sq, Skv, group, layout, fill)
    assert int(ar.o_mask.sum()) == B * Sq * H * d
    o = ar.fresh_o()
    ar.o.window(o).fill_(1.0)
    assert bool((o.view(torch.int16)[ar.o_mask] == 0x3F80).all()) and bool((o.view(torch.int16)[~ar.o_mask] == A.CANARY_BITS).all())
    assert ar.extract(o).shape == (B, Sq, H, d)


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_fills_differ_only_outside_the_live_elements(shape, layout):
    d, B, H, Sq, Skv, group, _ = shape
    f, h = (A.build(d, B, H, Sq, Skv, group, layout, fill, seed=3) for fill in A.FILLS)
    for name in ("q", "k", "vt"):
        rf, rh = getattr(f, name), getattr(h, name)
        assert (rf.off, rf.bs, rf.rs) == (rh.off, rh.bs, rh.rs)
        live = torch.zeros(rf.full.numel(), dtype=torch.bool)
        if name == "vt":
            w = torch.as_strided(live, (B, rf.rows, rf.pad), (rf.bs, rf.rs, 1), rf.off)
            w[:, :, A.perm_index(rf.pad)[:Skv]] = True
        else:
            rf.window(live).fill_(True)
            if f.q.full is f.k.full:        # Q and K in one buffer
                f.q.window(live).fill_(True), f.k.window(live).fill_(True)
        bits_f, bits_h = rf.full.view(torch.int16), rh.full.view(torch.int16)
        assert torch.equal(bits_f[live], bits_h[live])
        assert bool((bits_f[~live] == 0).all())
        outside = bits_h[~live]
        if name != "vt":
            assert bool((outside == A.NAN_BITS).all())
        else:       # the padding columns are finite, within [-4, 4], and not all zero; everything else is NaN
            padding = torch.zeros_like(live)
            w = torch.as_strided(padding, (B, rf.rows, rf.pad), (rf.bs, rf.rs, 1), rf.off)
            w[:, :, A.perm_index(rf.pad)[Skv:]] = True
            assert bool((bits_h[~live & ~padding] == A.NAN_BITS).all())
            vals = rh.full[padding].float()
            assert bool(torch.isfinite(vals).all()) and vals.abs().max().item() <= 4.0 and bool((vals != 0).any())
    # the compact copies are the live elements
    assert torch.equal(torch.as_strided(h.k.full, (B, Skv, h.k.width), (h.k.bs, h.k.rs, 1), h.k.off), h.k_c.reshape(B, Skv, -1))
