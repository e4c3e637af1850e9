"""tests/helpers/enc_attn_arena.py has teeth: tests/helpers/enc_attn_emu.py restates attn_bias_kernel's addressing in torch on the
arenas and drives the assertions of tests/test_gpu_enc_attn_operands.py (value, footprint, inputs unchanged, fill independence,
determinism).  The faithful emulation passes every case of the table under every layout and both fills; each mutant -- the ways
such a kernel goes wrong -- fails the value or the footprint assertion on at least one FAMILY A case.  The same file asserts the
conditions the helper's docstring puts on the data, for every case and every row, and that the table meets every boundary."""
import functools

import pytest
import torch

from helpers import enc_attn_arena as E
from helpers import enc_attn_emu as EMU

TABLE = E.table()
IDS = [E.case_id(c) for c in TABLE]


@functools.lru_cache(maxsize=None)
def _data_ref(case):
    data = E.make_data(case)
    return data, E.reference(data)


def _run(call, mutant=None):
    return EMU.emulate(call, call.fresh_out(), mutant)


def _failures(case, layout, mutant=None):
    data, ref = _data_ref(case)
    f, h = E.build(data, layout, "friendly"), E.build(data, layout, "hostile")
    return E.failures(f, _run(f, mutant), h, _run(h, mutant), ref, _run(f, mutant))


@pytest.mark.parametrize("case", TABLE, ids=IDS)
def test_the_faithful_emulation_passes_every_case(case):
    for layout in E.layouts_of(case):
        assert _failures(case, layout) == {}, layout


@pytest.mark.parametrize("mutant", EMU.MUTANTS)
def test_every_mutant_fails_a_family_a_case(mutant):
    caught = []
    for case in TABLE:
        if case.family != "A":
            continue
        for layout in E.layouts_of(case):
            failed = _failures(case, layout, mutant)
            if "value" in failed or "footprint" in failed:
                caught.append((E.case_id(case), layout, sorted(failed)))
                break
        if len(caught) >= 2:
            break
    print("%-24s caught by %s" % (mutant, caught))
    assert caught, mutant


@pytest.mark.parametrize("case", TABLE, ids=IDS)
def test_the_data_keeps_the_scores_exact(case):
    """q . k has integer terms and magnitude <= 256 (family A: a single term, a power of two, 256 at scale 1); the bias holds
    multiples of 1/4; masked k and v stay finite."""
    data, _ = _data_ref(case)
    q, k = (t.double().permute(0, 2, 1, 3) for t in (data.q, data.k))
    assert bool((q == q.round()).all()) and bool((k == k.round()).all())
    if case.family == "A":
        code, hit = (16.0, 256.0) if data.scale == 1.0 else (32.0, 1024.0)
        for t in (q, k):       # one code per row: a dot product has at most one non-zero term, code * code
            assert bool(((t != 0).sum(dim=-1) == 1).all()) and bool(((t == 0) | (t == code)).all())
        dots = q @ k.transpose(-1, -2)
        assert bool(((dots == 0) | (dots == hit)).all()) and (bool((dots == hit).any()) or case.L == 1) and bool((dots == 0).any())
        assert float(torch.tensor(hit).to(E.BF)) == hit and hit * data.scale >= E.GAP
    else:
        assert (q.abs() @ k.abs().transpose(-1, -2)).max().item() <= 256
        assert bool((data.q.float().abs() <= 2).all()) and bool((data.k.float().abs() <= 2).all())
        cols = (data.q.float() != 0).any(dim=0).any(dim=0).any(dim=0).nonzero().reshape(-1).tolist()
        assert 1 < len(cols) <= 4 and (data.d == 64 or max(cols) >= 64), cols
    if data.table is not None:
        t = data.table.double()
        assert bool((t * 4 == (t * 4).round()).all())
        assert all(not torch.equal(t[:, a], t[:, b]) for a in range(E.H) for b in range(a)), "the same bias for two heads"
        if case.family == "B":
            assert t.abs().max().item() <= 4 and bool((t[1:] != t[:-1]).all()), "the same bias in neighbouring buckets"
    assert bool(torch.isfinite(data.k.float()).all()) and bool(torch.isfinite(data.v.float()).all())


@pytest.mark.parametrize("case", [c for c in TABLE if c.family == "A"], ids=[i for i, c in zip(IDS, TABLE) if c.family == "A"])
def test_family_a_rows_are_uniform_over_their_top_level(case):
    """Every row of every case, none left out: the scores below the top level are at least 112 below it, bf16(1 / n) does not
    depend on the device's division, p v is exact in float32, masked keys carry 2^100 and the other v are small integers that
    vary along every index."""
    data, ref = _data_ref(case)
    assert bool((ref.top_gap >= E.GAP).all()), ref.top_gap.min().item()
    n = ref.n[~ref.nokey]
    assert bool(E.n_is_safe(n).all()), sorted(set(n[~E.n_is_safe(n)].tolist()))
    v = data.v.double()
    live = torch.ones(E.B, case.L, dtype=torch.bool) if data.mask is None else data.mask != 0
    assert bool((v[~live] == E.BIG_V).all())
    small = v[live]
    assert bool((small == small.round()).all()) and small.abs().max().item() <= 8
    assert 8 * case.L * 256 <= 2 ** 24              # |sum of v| <= 8 L (13 bits at most) times an 8-bit p: exact in float32
    assert bool(v.diff(dim=3)[live].ne(0).any()) and bool(v.diff(dim=2)[live].ne(0).any())
    pairs, both = live[:, 1:] & live[:, :-1], live[0] & live[1]
    assert not bool(pairs.any()) or bool(v.diff(dim=1)[pairs].ne(0).any())
    assert not bool(both.any()) or bool((v[0][both] != v[1][both]).any())
    # rows without a hit: every surviving key at the top (where a phantom key of [L, Lp) would join)
    if data.table is None:
        keys = ref.n.clone()
        survivors = live.sum(dim=1).reshape(E.B, 1, 1).expand_as(keys)
        if data.causal:
            survivors = torch.stack([live[b].cumsum(0) for b in range(E.B)]).reshape(E.B, 1, case.L).expand_as(keys)
        flat = (ref.n == survivors) & (survivors > 1) if case.L > 1 else (ref.n == survivors)
        assert bool(flat.any()), "no row whose scores are all equal"


@pytest.mark.parametrize("case", [c for c in TABLE if c.family == "B"], ids=[i for i, c in zip(IDS, TABLE) if c.family == "B"])
def test_family_b_softmax_is_not_one_hot_and_the_bound_holds_for_every_correct_kernel(case):
    """The median of max_j p_j over the rows with a key (a stronger statement than over all rows, where a row without a key
    counts 0); and on every element the p flips float32 allows, its arithmetic and the rounding of the result fit the bound."""
    _, ref = _data_ref(case)
    pmax = ref.pmax[~ref.nokey]
    assert pmax.median().item() <= 0.5 and ref.pmax.median().item() <= 0.5, pmax.median().item()
    assert E.room(ref).max().item() <= 1.0, E.room(ref).max().item()


def test_the_table_meets_every_boundary_and_every_mask():
    for mode in E.PRODUCT_MODES:
        d = E.MODES[mode]["d"]
        for family in "AB":
            met = set().union(*(E.classes_of(c.L, d) for c in TABLE if c.mode == mode and c.family == family))
            assert met == {"chunk_edge", "workgroup_tail", "mod4", "limit"}, (mode, family, met)
            lengths = {c.L for c in TABLE if c.mode == mode and c.family == family}
            assert lengths == {L for L in E.L_LIST if L <= E.LIMIT[d] and (family == "A" or L > 1)}, (mode, family)
    for mode in E.CROSS_MODES:       # the contract allows them, the product never issues them: L = 65 only, which is no size limit
        d = E.MODES[mode]["d"]
        assert {c.L for c in TABLE if c.mode == mode} == {65} and {c.family for c in TABLE if c.mode == mode} == {"A", "B"}
        assert E.classes_of(65, d) == {"chunk_edge", "workgroup_tail", "mod4"}
    m = E.MODES
    assert (m["x_causal_mask"]["causal"] and m["x_causal_mask"]["mask"] and m["x_causal_bias"]["causal"] and m["x_causal_bias"]["bias"]
            and m["x_d80_mask_causal"]["d"] == 80 and m["x_d80_mask_causal"]["mask"] and m["x_d80_mask_causal"]["causal"])
    assert {E.mask_kind(c) for c in TABLE} == set(E.MASK_KINDS) | {None}
    assert {layout for c in TABLE for layout in E.layouts_of(c)} == set(E.LAYOUTS)
    for mode in E.MODES:
        assert any("compact" in E.layouts_of(c) for c in TABLE if c.mode == mode) and all("loose" in E.layouts_of(c) for c in TABLE)


@pytest.mark.parametrize("L", [33, 65, 512])
def test_the_masks_are_what_their_names_say(L):
    tails, holes, item, key0 = (E.make_mask(kind, L) for kind in E.MASK_KINDS)
    lengths = tails.sum(dim=1).tolist()
    assert lengths[0] != lengths[1] and all(0 < n < L for n in lengths)
    assert all(bool((tails[b, :lengths[b]] == 1).all()) for b in range(E.B))
    for b in range(E.B):      # a hole: a masked key with live keys on both sides
        z = (holes[b] == 0).nonzero().reshape(-1)
        assert z.numel() > 0 and holes[b, 0] == 1 and holes[b, L - 1] == 1
    assert not torch.equal(holes[0], holes[1])
    assert int(item[1].sum()) == 0 and 0 < int(item[0].sum()) < L
    assert int(key0[0, 0]) == 0 and int(key0[0].sum()) > 0 and int(key0[1, 0]) == 1


def test_rows_without_a_key_are_in_the_table():
    rows = {E.case_id(c): int(_data_ref(c)[1].nokey.sum()) for c in TABLE if E.mask_kind(c) in ("item", "key0")}
    assert rows and all(n > 0 for n in rows.values()), rows
    # a fully masked item: every row of it; key 0 masked under causal: row 0 of item 0, every head
    for c in TABLE:
        nokey = _data_ref(c)[1].nokey
        if E.mask_kind(c) == "item":
            assert bool(nokey[1].all()) and not bool(nokey[0].any())
        if E.mask_kind(c) == "key0":
            assert bool(nokey[0, :, 0].all()) and int(nokey.sum()) == E.H


def test_hostile_arenas_hold_nan_everywhere_outside_the_live_elements():
    data, _ = _data_ref(E.Case("clip_vision", 65, "A"))
    for layout in E.LAYOUTS:
        f, h = E.build(data, layout, "friendly"), E.build(data, layout, "hostile")
        live = torch.zeros(h.qkv.numel(), dtype=torch.bool)
        for off in (h.q_off, h.k_off, h.v_off):
            torch.as_strided(live, (E.B * 65, h.inner), (h.qkv_rs, 1), off).fill_(True)
        assert int(live.sum()) == 3 * E.B * 65 * h.inner
        assert bool((h.qkv.view(torch.int16)[~live] == E.NAN_BITS).all()) and bool((f.qkv.view(torch.int16)[~live] == 0).all())
        assert torch.equal(h.qkv.view(torch.int16)[live], f.qkv.view(torch.int16)[live])
        assert bool((h.fresh_out().view(torch.int16) == E.CANARY_BITS).all())
        assert int(h.o_mask.sum()) == E.B * 65 * h.inner
        if layout == "loose":
            assert h.qkv_rs % 8 == 0 and h.qkv_rs > 3 * h.inner and h.out_rs == h.inner + 20
            offs = [off % h.qkv_rs for off in (h.q_off, h.k_off, h.v_off)]
            assert all(o % 8 == 0 and o > 0 for o in offs) and offs[1] - offs[0] > h.inner and offs[2] - offs[1] > h.inner
