"""The offset form of the default d = 64 statement (scripts/gen_attn_pipe.py -> alg_amd/csrc/attn_pipe_off_loop.inc, ALG_ATTN_PP=8)
checked as a program on the CPU: the committed text is what the generator emits, and the statement runs in scripts/asm_emu.py for
an eight-wave workgroup under the weakest memory ordering the ISA allows (tests/test_attn_q64_statement_cpu.py's harness and
orderings; tests/helpers/attn_off_emu.py binds the operands the way attention.hip's frame does):

  * with every offset zero it leaves O, l, t and `code` bit-identical to the zero-offset statement on the same inputs;
  * with per-query offsets from {-90, 0, 37.5, 120} every probability is bf16(exp2(x)) with x the fp32 accumulation -m + k.q that
    STARTS at -m, and the attention stays inside the existing statement test's tolerance against a float64 softmax;
  * a row sum that reaches 2^80 in iteration t ends the statement with code 1, PV(t - 1) and QK(t + 1) done and softmax(t) not;
  * alg_attn_path_tap is declared in the header and exported by the library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import attn_emu as H  # noqa: E402
import attn_off_emu as HO  # noqa: E402

MODES = [(True, False), (False, True), (True, True)]     # (lazy fragment reads, lazy DMA)
TOL = 6e-3                                               # tests/test_attn_q64_statement_cpu.py's
OFFSETS = np.array([-90.0, 0.0, 37.5, 120.0], dtype=np.float32)


def relerr(out, ref):
    return float(np.abs(out - ref).max() / np.abs(ref).max())


def test_committed_inc_is_what_the_generator_emits(tmp_path):
    env = dict(os.environ, ATTN_PIPE_OUT=str(tmp_path / "a.inc"), ATTN_PIPE_OFF_OUT=str(tmp_path / "b.inc"))
    for knob in ("ATTN_PIPE_WAIT_PAIRS", "ATTN_PIPE_NO_NOP", "ATTN_PIPE_SUM16"):
        env.pop(knob, None)
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_attn_pipe.py")], check=True, env=env, capture_output=True)
    csrc = os.path.join(ROOT, "alg_amd", "csrc")
    assert (tmp_path / "b.inc").read_bytes() == open(os.path.join(csrc, "attn_pipe_off_loop.inc"), "rb").read()
    assert (tmp_path / "a.inc").read_bytes() == open(os.path.join(csrc, "attn_pipe_loop.inc"), "rb").read()


def test_offset_text_differs_from_the_zero_offset_text_only_where_it_should():
    """same instruction stream: 16 copies of -m in the warm-up, the 12 first k-steps of QK(t) / QK(t + 1) take v[10:25] as srcC
    (warm-up 2 + 2, four loop phases x 2), the V^T fragments come through the K addresses + 32 KiB"""
    import gen_attn_pipe as GP
    GP.configure(8)
    zero = GP.emit()
    GP.configure(8, offset=True)
    off = GP.emit()
    GP.configure(8)
    movs = [ln for ln in off if ln.startswith("v_mov_b32")]
    assert movs == ["v_mov_b32 v%d, %%[negm]" % (10 + i) for i in range(16)]
    rest = [ln for ln in off if not ln.startswith("v_mov_b32")]
    assert len(rest) == len(zero)
    n_c = 0
    for a, b in zip(zero, rest):
        if a == b:
            continue
        if a.startswith("v_mfma"):
            assert a.endswith(", 0") and b == a[:-1] + "v[10:25]", (a, b)
            n_c += 1
        else:
            m = re.match(r"^(ds_read_b128 a\[\d+:\d+\], )%\[lv(\d)\] offset:(\d+)$", a)
            assert m and b == "%s%%[lk%s] offset:%d" % (m.group(1), m.group(2), int(m.group(3)) + 32768), (a, b)
            assert int(m.group(3)) + 32768 < 65536
    assert n_c == 12 and not any(ln.endswith(", 0") for ln in off if ln.startswith("v_mfma"))
    used = set()
    for ln in off:
        for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", ln):
            used.update(range(int(m.group(1)), int(m.group(2)) + 1) if m.group(1) else [int(m.group(3))])
    assert min(used) == 10 and max(used) == 127              # v[0:9] stay the frame's: nine "v" operands


@pytest.mark.parametrize("T,seed", [(15, 11), (20, 12)])
def test_zero_offsets_are_bit_identical_to_the_zero_offset_statement(T, seed):
    pb = H.Problem(64, T, seed=seed, prescaled=True)
    zeros = np.zeros(pb.Sq, dtype=np.float32)
    for lazy_reads, lazy_dma in MODES:
        a = HO.run_pipe8_off_statement(pb, zeros, lazy_reads, lazy_dma, zero_form=True)
        b = HO.run_pipe8_off_statement(pb, zeros, lazy_reads, lazy_dma)
        assert a["t_exits"] == b["t_exits"] == [1 + 4 * ((T - 3 - 1) // 4)] * 8 and a["codes"] == b["codes"] == [0] * 8
        assert np.array_equal(a["O"].view(np.uint32), b["O"].view(np.uint32))
        assert np.array_equal(a["l"].view(np.uint32), b["l"].view(np.uint32))
    # ... and the shared harness drives the zero-offset statement as attn_emu's own does
    out, t_exit, codes, _, _ = H.run_pipe8_statement(pb, True, True)
    assert t_exit == a["t_exit"] and relerr(HO.finish(pb, a), out) == 0.0


def offset_problem(T, seed, planted_rows=None, planted_key=None):
    """per-query offsets m from OFFSETS, every score of a row inside [m - 30, m + 10]: axis 0 carries m - 10 (keys: 1.0), the other
    axes the usual N(0, 1.44^2) log2 units.  planted: + 100 on one key for some rows (axis 1)."""
    pb = H.Problem(64, T, seed=seed, prescaled=True)
    rng = np.random.default_rng(seed + 100)
    m = OFFSETS[rng.integers(0, 4, pb.Sq)]
    pb.k[:, 0], pb.k[:, 1], pb.q[:, 1] = 1.0, 0.0, 0.0
    pb.q[:, 0] = m - 10.0                                   # -100, -10, 27.5, 110: exact in bf16
    if planted_rows is not None:
        pb.q[planted_rows, 1] = 1.0
        pb.k[planted_key, 1] = 100.0
    pb.pack()
    return pb, m


def chain_scores(pb, m, t):
    """S(t) - m as the matrix pipe forms it: fp32(-m + k-step 0), then one fp32 rounding per further 16-wide k-step"""
    x = (np.float32(0.0) - m)[:, None].astype(np.float32) * np.ones((1, H.KVB), dtype=np.float32)
    kt = pb.k[t * H.KVB:(t + 1) * H.KVB].astype(np.float64)
    for ks in range(4):
        d = pb.q[:, 16 * ks:16 * ks + 16].astype(np.float64) @ kt[:, 16 * ks:16 * ks + 16].T
        x = (x.astype(np.float64) + d).astype(np.float32)
    return x


def expected_probs(x):
    return H.bf16_round(np.exp2(x.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("T,seed", [(15, 21), (20, 22)])
def test_offsets_enter_the_fp32_chain_first_and_the_attention_holds(T, seed):
    pb, m = offset_problem(T, seed)
    assert all((m == o).any() for o in OFFSETS)
    s = pb.q.astype(np.float64) @ pb.k.astype(np.float64).T
    assert (s >= m[:, None] - 30.0).all() and (s <= m[:, None] + 10.0).all()
    ref = pb.reference()
    l_ref = np.exp2(s - m[:, None].astype(np.float64)).sum(axis=1)
    t_last = 1 + 4 * ((T - 3 - 1) // 4)
    for lazy_reads, lazy_dma in MODES:
        r = HO.run_pipe8_off_statement(pb, m, lazy_reads, lazy_dma)
        assert r["t_exits"] == [t_last] * 8 and r["codes"] == [0] * 8
        # the registers the statement leaves: scores of tiles t_last - 1 and t_last (QK runs one tile ahead), probabilities of
        # tiles t_last - 2 and t_last - 1 -- each must be what the chain that starts at -m gives, to the bit
        xs = {t: chain_scores(pb, m, t) for t in (t_last - 2, t_last - 1, t_last)}
        for w in range(8):
            rows = slice(32 * w, 32 * w + 32)
            got_s = [HO.score_tile(r, w, n) for n in ("SA", "SB")]
            got_p = [HO.prob_tile(r, w, n) for n in ("PA", "PB")]
            for t in (t_last - 1, t_last):
                assert any(np.array_equal(g.view(np.uint32), xs[t][rows].view(np.uint32)) for g in got_s), (w, t)
            for t in (t_last - 2, t_last - 1):
                assert any(np.array_equal(g.view(np.uint32), expected_probs(xs[t][rows]).view(np.uint32)) for g in got_p), (w, t)
        out = HO.finish(pb, r)
        assert relerr(out, ref) < TOL, (lazy_reads, lazy_dma, relerr(out, ref))
        l_got = r["l"].astype(np.float64).sum(axis=1) + sum(r["fsum"](t) for t in range(t_last, T))
        assert float(np.abs(l_got / l_ref - 1.0).max()) < TOL


def test_re_entry_at_a_later_t_with_offsets():
    """the frame enters again at t = 5 after a refused tile, with the ring in the state the straight loop leaves it in"""
    pb, m = offset_problem(20, 23)
    r = HO.run_pipe8_off_statement(pb, m, True, True, t0=5)
    assert r["t_exits"] == [17] * 8 and r["codes"] == [0] * 8
    assert relerr(HO.finish(pb, r), pb.reference()) < TOL


def test_a_row_sum_past_2_to_the_80_leaves_with_code_1_and_the_tile_not_done():
    T, tb = 20, 6
    hit = np.zeros(256, dtype=bool)
    hit[5::32] = True                                       # one row of every wave (a wave that leaves stops staging its share of the
    #                                                         tiles: the frame's straight loop would go on doing that, nobody does here)
    pb, m = offset_problem(T, 24, planted_rows=hit, planted_key=tb * H.KVB + 3)
    s = pb.q.astype(np.float64) @ pb.k.astype(np.float64).T
    assert (s[hit, tb * H.KVB + 3] - m[hit] > 80.0).all() and (np.delete(s, tb * H.KVB + 3, axis=1) <= m[:, None] + 10.0).all()
    for lazy_reads, lazy_dma in MODES:
        r = HO.run_pipe8_off_statement(pb, m, lazy_reads, lazy_dma)
        assert r["codes"] == [1] * 8 and r["t_exits"] == [tb] * 8
        vf = pb.v.astype(np.float64)
        # softmax(t) is not done: l and O hold tiles 0 .. t - 1 only (PV(t - 1) is done)
        l_want = sum(r["fsum"](t) for t in range(tb))
        O_want = sum(r["probs"](t) @ vf[t * H.KVB:(t + 1) * H.KVB] for t in range(tb))
        l_got = r["l"].astype(np.float64).sum(axis=1)
        assert float(np.abs(l_got / l_want - 1.0).max()) < 1e-5
        assert float(np.abs(r["O"] - O_want).max() / np.abs(O_want).max()) < TOL
        # QK(t + 1) is done, with the offset in its chain (the refused tile's own scores are the frame's to redo)
        want = chain_scores(pb, m, tb + 1)
        for w in range(8):
            rows = slice(32 * w, 32 * w + 32)
            assert any(np.array_equal(HO.score_tile(r, w, n).view(np.uint32), want[rows].view(np.uint32)) for n in ("SA", "SB")), w


def test_path_tap_is_declared_bound_and_exported():
    import alg_amd
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    assert re.search(r"\bvoid\s+alg_attn_path_tap\(uint64_t\*\s*\w+\);", header)
    assert "alg_attn_path_tap" in alg_amd._lib.EXPORTS and callable(alg_amd._lib.attn_path_tap)
    assert os.path.exists(alg_amd._lib.LIB_PATH), "libalg_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", alg_amd._lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT alg_attn_path_tap\b", out)
