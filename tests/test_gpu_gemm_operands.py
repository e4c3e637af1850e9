"""The GEMM entries (alg_gemm_bf16, _pair, _pair_qk, alg_gemm_fp8, alg_gemm_fp4, _q4out) on guarded, strided and offset operands with
exact data (tests/helpers/gemm_arena.py): every store path of csrc/gemm_kernel.h and csrc/gemm_fp4.hip -- the LDS-staged epilogue
and its four residual loops, the element-exact band with 8-byte quads and with single elements, the permuted V^T stores -- on every
route (ALG_GEMM_PIPE = 6, 9, 10; a PackedB on schedule 11; K = 64; e4m3 under 6 and 9; MXFP4 with a bf16 and with an MXFP4 output;
the pair launch and the pair with the QK norm), each reached by ONE trigger at N = 520 and by the edge shapes N = 516, 250 and 6.
Every case, under a friendly fill of zeros and a hostile fill of NaN outside the live elements:

  1. without an activation the output is BIT FOR BIT the float64 reference of the header's contract: the data makes every float32
     intermediate exact, so no schedule's accumulation order shows;
  2. with one, |got - ref| <= 2^-7 |ref| + 2^-100 (one bf16 step; v_exp_f32 and v_rcp_f32 are 1-ulp instructions), and among the
     elements with |ref| >= 2^-100 at most 1 % differ from bf16(ref): a cap, not a measurement -- the float32 form of act_apply
     on the 1/8 grid inside [-6, 6], where the cases keep the pre-activation values, rounds like the float64 one on every point
     (tests/test_gemm_arena_cpu.py).  The share is printed;
  3. footprint: every C element outside the mask -- the image of [0, N) under the permutation, rows < M, each batch item -- still
     holds the canary; A, B, bias, gate, the scales and a residual of its own are unchanged bit for bit;
  4. fill independence: the hostile and the friendly outputs are bit-equal and finite;
  5. determinism: a second run gives the same bits in the whole arena.

The `second_tile` cases take a batch at which every workgroup of the persistent launch walks at least two tiles (the __syncthreads
between tiles, the LDS ring reused by the next K loop).  tests/test_gemm_arena_cpu.py shows on an emulation that these assertions
catch the ways such addressing goes wrong, and that the table holds every (route, trigger) pair."""
import pytest
import torch

from alg_amd import _lib
from helpers import gemm_arena as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 8
TABLE = G.table(CUS)
HEADS, TEXT_LEN, EPS, Q_SCALE = 4, 17, 1e-6, 0.18033688       # the QK norm of the pair_qk cases


def _launch(call, c_full):
    packed = None
    if call.case.route == "p11":        # packed from the weight's window inside the (hostile-filled) arena
        packed = _lib.PackedB(call.ops["B"].window()[0])
    pos, kw = call.gemm_call(c_full, B=packed)
    (_lib.gemm_fp4 if call.kind == "fp4" else _lib.gemm)(*pos, **kw)


def _report(report):
    for cid, fill, share in report:
        print("activation mismatch share %-60s %-8s %.6f" % (cid, fill, share))


def _drive(case, launch, reference=G.reference):
    """One problem under both fills, the friendly one twice: assertions 1 to 5."""
    f, h = G.build(case, "friendly", DEV), G.build(case, "hostile", DEV)
    y = reference(f)
    outs = []
    for call in (f, h, f):
        c = call.fresh_c()
        launch(call, c)
        outs.append(c)
    torch.cuda.synchronize()
    report = []
    failed = G.failures(f, outs[0], h, outs[1], y, outs[2], report)
    _report(report)
    assert failed == {}, failed


def _fp4_bf16_output(call):
    """alg_gemm_fp4 on the operands of an alg_gemm_fp4_q4out call, into a contiguous bf16 C: the value the header says the fused
    quantiser sees.  Checked against the float64 reference under the activation tolerance before it is used."""
    c, g, ops = call.case, call.g, call.ops
    out = torch.empty(c.batch, c.M, c.N, dtype=BF, device=DEV)
    _lib.gemm_fp4(ops["A"].view, ops["B"].view, out, c.M, c.N, c.K, g["lda"], g["ldb"], c.N, a_scale=ops["a_scale"].view,
                  b_scale=ops["b_scale"].view, strideAScale=g["strideAScale"], strideBScale=g["strideBScale"], bias=ops["bias"].view,
                  batch=c.batch, strideA=g["strideA"], strideB=g["strideB"], strideC=c.M * c.N, act=call.f["act"])
    y = G.reference(call)
    assert bool(((out.double() - y).abs() <= 2.0 ** -7 * y.abs() + G.TINY).all()), G.case_id(c)
    return out.double()


PLAIN = [c for c in TABLE if c.route not in ("pair", "pair_qk")]


@pytest.mark.parametrize("case", PLAIN, ids=[G.case_id(c) for c in PLAIN])
def test_gemm_on_guarded_operands(case, monkeypatch):
    monkeypatch.setenv("ALG_GEMM_PIPE", G.ROUTES[case.route][1])
    q4_act = case.route == "fp4_q4out" and G.form_of(case)["act"] != G.ACT_NONE
    _drive(case, _launch, reference=_fp4_bf16_output if q4_act else G.reference)


PAIRS = [c for c in TABLE if c.route == "pair"]


@pytest.mark.parametrize("case", PAIRS, ids=[G.case_id(c) for c in PAIRS])
def test_gemm_pair_on_guarded_operands(case, monkeypatch):
    """alg_gemm_bf16_pair: a plain problem and the V^T form in one persistent launch (schedule 10)."""
    monkeypatch.setenv("ALG_GEMM_PIPE", G.ROUTES[case.route][1])
    probs = G.pair_cases(case)
    calls = {fill: [G.build(p, fill, DEV) for p in probs] for fill in G.FILLS}
    ys = [G.reference(c) for c in calls["friendly"]]
    outs = []
    for fill in ("friendly", "hostile", "friendly"):
        cs = [c.fresh_c() for c in calls[fill]]
        _lib.gemm_pair(*[c.gemm_call(o) for c, o in zip(calls[fill], cs)])
        outs.append(cs)
    torch.cuda.synchronize()
    for i in range(2):
        failed = G.failures(calls["friendly"][i], outs[0][i], calls["hostile"][i], outs[1][i], ys[i], outs[2][i])
        assert failed == {}, (i, failed)


PAIRS_QK = [c for c in TABLE if c.route == "pair_qk"]


@pytest.mark.parametrize("case", PAIRS_QK, ids=[G.case_id(c) for c in PAIRS_QK])
def test_gemm_pair_qk_on_guarded_operands(case, monkeypatch):
    """alg_gemm_bf16_pair_qk (schedule 9) whose second problem is the V^T form.  V^T is checked like every other call; the Q|K
    tensor is, by the header, bit for bit alg_qk_norm_rope_scaled applied to the plain GEMM's result -- here to the bf16 of the exact
    reference -- and goes through the footprint, fill and determinism assertions as it stands."""
    monkeypatch.setenv("ALG_GEMM_PIPE", G.ROUTES[case.route][1])
    probs = G.pair_cases(case)
    calls = {fill: [G.build(p, fill, DEV) for p in probs] for fill in G.FILLS}
    qk = calls["friendly"][0]
    B, M, N = case.batch, case.M, case.N
    assert N == 2 * HEADS * 64 and qk.g["ldc"] == N and qk.g["strideC"] == M * N
    g = torch.Generator().manual_seed(M + N)
    rn = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(BF).to(DEV)
    wq, bq, wk, bk = (1 + rn(64, sc=0.2)), rn(64, sc=0.2), (1 + rn(64, sc=0.2)), rn(64, sc=0.2)
    ang = (torch.rand(M - TEXT_LEN, 32, generator=g) * 6.28).to(DEV)
    cos, sin = ang.cos().repeat_interleave(2, dim=1).contiguous(), ang.sin().repeat_interleave(2, dim=1).contiguous()
    ys = [G.reference(c) for c in calls["friendly"]]
    want = G.bf16_rne(ys[0]).float().to(BF).contiguous()
    _lib.qk_norm_rope_(want, wq, bq, wk, bk, cos, sin, B, M, HEADS, TEXT_LEN, EPS, q_scale=Q_SCALE)
    outs = []
    for fill in ("friendly", "hostile", "friendly"):
        cs = [c.fresh_c() for c in calls[fill]]
        _lib.gemm_pair_qk(*[c.gemm_call(o) for c, o in zip(calls[fill], cs)], wq, bq, wk, bk, cos, sin, HEADS, TEXT_LEN, EPS, q_scale=Q_SCALE)
        outs.append(cs)
    torch.cuda.synchronize()
    failed = G.failures(calls["friendly"][1], outs[0][1], calls["hostile"][1], outs[1][1], ys[1], outs[2][1])
    assert failed == {}, failed
    qk_h = calls["hostile"][0]
    for call, out in ((qk, outs[0][0]), (qk_h, outs[1][0])):
        got = call.extract(out)
        same = got.view(torch.int16) == want.view(torch.int16)
        assert bool(same.all()), ("qk reference", call.fill, int((~same).sum()), (~same).nonzero()[:4].tolist())
        G.assert_footprint(call, out)
        G.assert_inputs_unchanged(call)
    G.assert_fill_independent(qk_h, outs[1][0], outs[0][0])
    G.assert_deterministic(qk, outs[0][0], outs[2][0])


@pytest.mark.parametrize("route", ["p10", "p11", "fp8_p9", "fp4"])
@pytest.mark.parametrize("form", ["res_gate_bf16", "res_gate_f32_straddle"])
@pytest.mark.parametrize("gseg", [522, 521])
def test_a_gate_seg_stride_off_the_quad_grid_is_refused_before_any_launch(route, form, gseg, monkeypatch):
    """N % 4 == 0: the second gate segment is read with 8- and 16-byte loads at gate + gate_seg_stride + n, so a segment stride that
    is no multiple of 4 is ALG_EINVAL (include/alg_hip.h), and C keeps the canary."""
    monkeypatch.setenv("ALG_GEMM_PIPE", G.ROUTES[route][1])
    K = {"fp8_p9": 256, "fp4": 256}.get(route, 128)
    call = G.build(G.Case(route, form, "gsegN8", 300, 520, K, 2), "friendly", DEV)
    c = call.fresh_c()
    before = c.clone()
    packed = _lib.PackedB(call.ops["B"].window()[0]) if route == "p11" else None
    pos, kw = call.gemm_call(c, B=packed)
    kw["gate_seg_stride"] = gseg
    with pytest.raises(_lib.AlgHipError):
        (_lib.gemm_fp4 if call.kind == "fp4" else _lib.gemm)(*pos, **kw)
    torch.cuda.synchronize()
    assert torch.equal(c.view(torch.int16), before.view(torch.int16))
    G.assert_inputs_unchanged(call)
