"""tests/helpers/gemm_arena.py has teeth: a torch emulation of a strided GEMM call -- float32 arithmetic, every operand read and C
written through explicit flat indices built from the call's offsets, pitches and batch strides, the activation in the kernel's own
float32 form -- drives the assertions of tests/test_gpu_gemm_operands.py (reference, footprint, inputs unchanged, fill independence,
determinism).  The faithful emulation passes every case of the GPU table; each mutant -- the ways a kernel addressing such operands
goes wrong -- fails the assertion named for it.  The same file asserts the exactness property of the data for every case (the
reference asserts every float32 intermediate) and that the table holds every (route, trigger) pair it has to."""
import pytest
import torch

import _mxfp4
from helpers import gemm_arena as G

TABLE = G.table(cus=8)
IDS = [G.case_id(c) for c in TABLE]


def _problems(case):
    return G.pair_cases(case) if case.route in ("pair", "pair_qk") else (case,)


def act32(x, act):
    """act_apply of csrc/common.h in float32: x * rcp(1 + exp2(...))."""
    if act == G.ACT_GELU:
        k1 = torch.tensor(-2.0 * 1.4426950408889634 * 0.7978845608028654, dtype=torch.float32)
        k2 = torch.tensor(0.044715, dtype=torch.float32) * k1
        return x * (1.0 / (1.0 + torch.exp2(x * (k2 * (x * x) + k1))))
    if act == G.ACT_SILU:
        return x * (1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634, dtype=torch.float32) * x)))
    return x


def emulate(call, c_full, mutant=None):
    """The call on the arenas of `call` into c_full, as a kernel addresses them: element (b, m, k) of A at A.off + b * strideA +
    m * lda + k and so on.  Rows and columns of the edge tiles read the clamped row M - 1 / N - 1 and are not stored."""
    case, f, g, ops = call.case, call.f, call.g, call.ops
    M, N, K, B = case.M, case.N, case.K, case.batch
    ar = torch.arange
    b_, m_, n_ = ar(B).reshape(B, 1, 1), ar(M).reshape(1, M, 1), ar(N).reshape(1, 1, N)

    def rows(op, count, bs, ld, width, unit=1):     # [B, count, width] flat indices of a row-major operand
        return op.off + b_ * (bs // unit) + ar(count).reshape(1, count, 1) * (ld // unit) + ar(width).reshape(1, 1, width)

    if call.kind == "bf16":
        A = ops["A"].full[rows(ops["A"], M, g["strideA"], g["lda"], K)].float()
        Bm = ops["B"].full[rows(ops["B"], N, g["strideB"], g["ldb"], K)].float()
    elif call.kind == "fp8":
        A = ops["A"].full[rows(ops["A"], M, g["strideA"], g["lda"], K)].view(G.F8).float()
        Bm = ops["B"].full[rows(ops["B"], N, g["strideB"], g["ldb"], K)].view(G.F8).float()
    else:
        kb = K // 32
        qa = ops["A"].full[rows(ops["A"], M, g["strideA"], g["lda"], K // 2, unit=2)]
        qb = ops["B"].full[rows(ops["B"], N, g["strideB"], g["ldb"], K // 2, unit=2)]
        sa = ops["a_scale"].full[ops["a_scale"].off + b_ * g["strideAScale"] + ar(M).reshape(1, M, 1) * kb + ar(kb).reshape(1, 1, kb)]
        sb = ops["b_scale"].full[ops["b_scale"].off + b_ * g["strideBScale"] + ar(N).reshape(1, N, 1) * kb + ar(kb).reshape(1, 1, kb)]
        A, Bm = _mxfp4.dequantize(_mxfp4.unpack(qa), sa).float(), _mxfp4.dequantize(_mxfp4.unpack(qb), sb).float()
    acc = A @ Bm.transpose(1, 2)
    if call.kind == "fp8":
        row = m_ + (1 if mutant == "scale_row_plus1" else 0)
        a_sc = ops["a_scale"].full[ops["a_scale"].off + b_ * g["strideAScale"] + row]
        b_sc = ops["b_scale"].full[ops["b_scale"].off + b_ * g["strideBScale"] + n_]
        acc = acc * (a_sc * b_sc)
    by_row = f["bias"] == "row" and mutant != "bias_by_col"
    bias = ops["bias"].full[ops["bias"].off + (m_ if by_row else n_)].float()
    x = (acc + bias).to(G.BF).float()
    if f["act"] != G.ACT_NONE:
        x = act32(x, f["act"]).to(G.BF).float()
    if f["res"]:
        r_full, r_op = (c_full, call.c) if f["res"] == "alias" else (ops["R"].full, ops["R"])
        ldr = g["ldc"] if mutant == "r_at_ldc" else g["ldr"]
        r = r_full[r_op.off + b_ * (0 if mutant == "strideR_ignored" else g["strideR"]) + m_ * ldr + n_].float()
        if f["gate"]:
            gs = N if g["gseg"] is None or mutant == "gseg_as_N" else g["gseg"]
            seg1 = m_ >= g["seg_split"] + (1 if mutant == "seg_split_plus1" else 0)
            gv = ops["gate"].full[ops["gate"].off + b_ * g["strideGate"] + seg1 * gs + n_].float()
            x = r + (gv * x if f["gate"] == "f32" else (gv * x).to(G.BF).float())
        else:
            x = r + x
    y = x.to(G.BF)
    if call.q4:
        q, s = G.quantized(y)
        c_full[0][call.c.off + b_ * (g["strideC"] // 2) + m_ * (g["ldc"] // 2) + ar(N // 2).reshape(1, 1, -1)] = q
        c_full[1][call.out_scales.off + b_ * g["strideOutScales"] + m_ * (N // 32) + ar(N // 32).reshape(1, 1, -1)] = s
        return c_full
    if f["perm"]:
        col = torch.tensor([G.swap23(n) + g["perm_col0"] if mutant == "perm_after_swap" else G.swap23(g["perm_col0"] + n) for n in range(N)])
    else:
        col = ar(N)
    ldc = N if mutant == "ldc_as_N" else g["ldc"]
    base = call.c.off + b_ * (0 if mutant == "strideC_ignored" else g["strideC"])
    c_full[base + m_ * ldc + col.reshape(1, 1, N)] = y
    if mutant == "chunk8":         # the last 8-column chunk of the edge tile goes out whole: columns N .. behind it, every row
        extra = ar(N, G.ceil_to(N, 8)).reshape(1, 1, -1)
        c_full[base + m_ * ldc + extra] = y[:, :, -1:].expand(B, M, extra.numel())
    if mutant == "row_M":          # row M of the last batch item (the clamped row's values): behind the operand under every geometry
        c_full[call.c.off + (B - 1) * g["strideC"] + M * ldc + col] = y[B - 1, M - 1]
    return c_full


def run(case, mutant=None, report=None):
    """{assertion: message} over the problems of a case, under both fills and a second friendly run."""
    failed = {}
    for prob in _problems(case):
        f, h = G.build(prob, "friendly"), G.build(prob, "hostile")
        y = G.reference(f)
        c_f, c_h, c_f2 = emulate(f, f.fresh_c(), mutant), emulate(h, h.fresh_c(), mutant), emulate(f, f.fresh_c(), mutant)
        failed.update(G.failures(f, c_f, h, c_h, y, c_f2, report))
    return failed


@pytest.mark.parametrize("case", TABLE, ids=IDS)
def test_the_faithful_emulation_passes_every_case_and_the_data_is_exact(case):
    """(G.reference asserts that the K-term sum in any order, acc * a_scale * b_scale, + bias, gate * x and r + ... are exact in
    float32, and that an activation sees values on the 1/8 grid inside [-6, 6].)"""
    assert run(case) == {}


def _pick(pred, limit=4):
    """Up to `limit` cases of the table that satisfy pred, from different routes first."""
    hits, seen = [], set()
    for c in TABLE:
        if c.route not in ("pair", "pair_qk") and c.trigger != "second_tile" and c.route not in seen and pred(c):
            hits.append(c), seen.add(c.route)
    return hits[:limit]


_geo = G.geometry
_form = G.form_of
# mutant -> (the assertion that has to catch it -- others may fail too, the cases it is tried on)
MUTANTS = {
    "ldc_as_N": ("footprint", _pick(lambda c: _geo(c)["ldc"] != c.N and not c.route.startswith("fp4_q"))),
    "strideC_ignored": ("reference", _pick(lambda c: c.batch > 1 and not c.route.startswith("fp4_q"))),
    "strideR_ignored": ("reference", _pick(lambda c: _form(c)["res"] == "own")),
    "perm_after_swap": ("reference", _pick(lambda c: c.trigger in ("perm4", "perm180", "perm37"), 9) +
                        [c for c in TABLE if c.route == "p10" and c.trigger in ("perm4", "perm180", "perm37")]),
    "chunk8": ("footprint", _pick(lambda c: c.N % 8 != 0 and not _form(c)["perm"])),
    "row_M": ("footprint", _pick(lambda c: c.trigger == "none" and not c.route.startswith("fp4_q")) + _pick(lambda c: c.trigger == "ldc4")),
    "seg_split_plus1": ("reference", _pick(lambda c: _form(c)["split"] == "mid" and c.trigger != "gseg0")),
    "gseg_as_N": ("reference", [c for c in TABLE if c.route in ("p9", "fp8_p6") and c.trigger in ("gseg0", "gsegN4", "gsegN8")]),
    "bias_by_col": ("reference", _pick(lambda c: _form(c)["bias"] == "row")),
    "scale_row_plus1": ("reference", _pick(lambda c: c.route.startswith("fp8"))),
    "r_at_ldc": ("reference", _pick(lambda c: _form(c)["res"] == "own" and _geo(c)["ldr"] != _geo(c)["ldc"])),
}
MUTANT_RUNS = [(m, caught_by, c) for m, (caught_by, cases) in MUTANTS.items() for c in cases]


def test_every_mutant_has_cases():
    for m, (_, cases) in MUTANTS.items():
        assert cases, m


@pytest.mark.parametrize("mutant,caught_by,case", MUTANT_RUNS, ids=["%s-%s" % (m, G.case_id(c)) for m, _, c in MUTANT_RUNS])
def test_every_mutant_fails_the_assertion_named_for_it(mutant, caught_by, case):
    failed = run(case, mutant)
    assert caught_by in failed, (mutant, failed)


def test_the_table_holds_every_route_trigger_pair_and_form():
    have = {(c.route, c.trigger) for c in TABLE}
    missing = [p for p in G.REQUIRED if p not in have]
    assert not missing, missing
    for route in G.ROUTES:                                 # what is left out is left out for a reason that is written down
        for t in G.TRIGGERS:
            assert ((route, t) in have) != (t in G.REFUSED[route]), (route, t)
    for route, (kind, _) in G.ROUTES.items():
        if route in ("pair", "pair_qk"):
            continue
        forms = {c.form for c in TABLE if c.route == route}
        want = set(G.FORMS)
        if route == "p11" or kind == "fp4":
            want -= set(G.ROW_BIAS_FORMS)
        if route == "fp4_q4out":
            want -= set(G.RES_FORMS) | {"silu"}
        assert forms == want, (route, want - forms)
    # both fills of every case, K with zero and with one trip of the steady-state loop, every kind of N
    for route in ("p6", "p9", "p10", "p11", "fp8_p6", "fp8_p9", "fp4"):
        mine = [c for c in TABLE if c.route == route]
        assert len({c.K for c in mine}) == 2 and {c.N for c in mine} == {520, 516, 250, 6} and {c.M for c in mine} == {300, 33}, route
    assert {c.K for c in TABLE if c.route == "k64"} == {64}
    assert min(c.K for c in TABLE if c.route == "fp8_p9") >= 256


LEAVES = set(G.C_TRIGGERS + G.R_TRIGGERS + ("gate_off4", "strideGate4", "gsegN4", "perm4", "perm180", "perm37", "n516", "n250", "n6"))


@pytest.mark.parametrize("case", [c for c in TABLE if c.route not in ("pair", "pair_qk", "fp4", "fp4_q4out")],
                         ids=[G.case_id(c) for c in TABLE if c.route not in ("pair", "pair_qk", "fp4", "fp4_q4out")])
def test_each_trigger_alone_decides_the_store_loop(case):
    """The header's rule for the LDS-staged epilogue, applied to the case's geometry: a trigger of LEAVES sends the tile to the
    element-exact loops, every other case of the table stays staged (a per-row bias next to an activation never is)."""
    want = case.trigger not in LEAVES and case.form != "rowbias_gelu"
    assert G.staged(case) == want, (G.case_id(case), G.geometry(case))
    if case.trigger in LEAVES and case.trigger not in G.SHAPE_TRIGGERS and case.form != "rowbias_gelu":
        tight = case._replace(trigger="none")
        assert case.N == 520 and G.staged(tight), "the trigger is the only reason"


def test_the_fills_differ_only_outside_the_live_elements():
    for case in [c for c in TABLE if c.trigger in ("windows", "gaps", "gseg0", "scales") and c.route in ("p10", "fp8_p9", "fp4", "fp4_q4out")]:
        f, h = G.build(case, "friendly"), G.build(case, "hostile")
        for name, of in f.ops.items():
            oh = h.ops[name]
            assert (of.off, of.bs, of.ld) == (oh.off, oh.bs, oh.ld)
            live = torch.zeros(of.full.numel(), dtype=torch.bool)
            of.window(live).fill_(True)
            bf, bh = G._ibits(of.full), G._ibits(oh.full)
            assert torch.equal(bf[live], bh[live]), (name, G.case_id(case))
            assert bool((bf[~live] == 0).all())
            outside = oh.full[~live]
            if outside.dtype == torch.uint8:
                assert bool(((outside == 0x7F) | (outside == 0x77) | (outside == 0xFF)).all())
            else:
                assert bool(torch.isnan(outside.float()).all())
        c = f.fresh_c()
        if not f.q4:
            assert bool((G._ibits(c)[~f.c_mask] == G.CANARY_BITS).all())


def test_the_gelu_reference_does_not_cancel():
    x = torch.tensor([-12.0, -9.5, -6.0, -1.0, 0.0, 1.0, 6.0], dtype=torch.float64)
    y = G.act64(x, G.ACT_GELU)
    assert bool((y[:4] < 0).all()) and y[4] == 0 and abs(y[6].item() - 6.0) < 1e-6
    assert abs(y[3].item() - (-0.15880800939172324)) < 1e-12


def test_the_float32_activation_on_the_eighth_grid_rounds_like_float64():
    """act_apply's float32 form against the float64 one on the 1/8 grid over [-6, 6] (what the cases feed an activation):
    the bf16 roundings agree on every point, so a kernel may differ only by its 1-ulp exp / rcp instructions."""
    x = (torch.arange(-48, 49, dtype=torch.float64) / 8).repeat(20619)[:2000000]
    for act in (G.ACT_GELU, G.ACT_SILU):
        a = act32(x.float(), act).to(G.BF)
        b = G.bf16_rne(G.act64(x, act)).float().to(G.BF)
        assert int((G._ibits(a) != G._ibits(b)).sum()) == 0
