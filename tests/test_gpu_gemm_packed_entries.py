"""Packed weights (alg_pack_b_p11 / _lib.PackedB, ALG_GEMM_B_PACKED11) on every GEMM entry point.  A packed B is readable only by
GEMM schedule 11: the pair launches (alg_gemm_bf16_pair / _pair_qk) read B as a row-major [N][ldb] panel and the e4m3 GEMM reads
bytes, so every entry point must route a packed problem to schedule 11 or refuse it -- and refuse it before anything is written.
Two oracles per case: (a) bit-identity with the single `_lib.gemm` call of the same problem in the same environment (a single
packed call is bit-identical to schedule 10's row-major call: tests/test_gpu_gemm_p11.py), (b) a float64 matmul on the rows at and
around tile edges, which catches a pair and a single call that are wrong in the same way.  Also the tall (slab-split) packed call
in the HunyuanVideo single-stream form (N*J rows into a column window of the [J][D + Mff] buffer), and the GPU packer against the
CPU restatement of its layout (tests/helpers/gemm_emu.py:pack_b_p11), strided weight views and N tails included."""
import ast
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from alg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import gemm_emu  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ALG_EINVAL = -1
SENT = 7.0                 # every C starts as this; what a call must not write keeps it
PIPES = ["10", "9", "6"]


def _gen(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *sh, sc=1.0: (torch.randn(*sh, generator=g, device="cuda") * sc).to(BF)


def _edge_rows(M):
    return torch.tensor(sorted({r for r in (0, 1, 15, 16, 255, 256, M - 1) if r < M}), device="cuda")


def swap23(n):
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


def _close(got, ref, what):
    err, bound = (got.double() - ref).abs().max().item(), 2.0 ** -7 * ref.abs().max().item()
    assert err <= bound, (what, err, bound)


class Lin:
    """a projection with a column bias: C[b, :, :N] = A[b] @ W^T + bias, C rows at pitch ldc (> N unless given)"""

    def __init__(self, rn, a, M, N, K, batch, packed, ldc=None):
        self.a, self.M, self.N, self.K, self.batch = a, M, N, K, batch
        self.w, self.bias = rn(N, K, sc=0.05), rn(N)
        self.B = _lib.PackedB(self.w) if packed else self.w
        self.ldc = N + 8 if ldc is None else ldc

    def fresh(self):
        return torch.full((self.batch, self.M, self.ldc), SENT, dtype=BF, device="cuda")

    def call(self, c):
        return ((self.a, self.B, c, self.M, self.N, self.K, self.K, self.K, self.ldc),
                dict(bias=self.bias, batch=self.batch, strideA=self.M * self.K, strideC=self.M * self.ldc))

    def check(self, c, what):
        assert bool((c[:, :, self.N:] == SENT).all()), (what, "written past N")
        rows, b = _edge_rows(self.M), self.batch - 1
        _close(c[b, rows, :self.N], self.a[b, rows].double() @ self.w.double().t() + self.bias.double(), what)


class VT:
    """the transposed V projection: the weight as A, the activations as B (strideB != 0), a per-row bias, kv index bits 2 and 3
    swapped in the store: C[b, d, swap23(s)] = (Wv @ y[b]^T)[d, s] + bv[d], rows padded to a multiple of 64"""

    def __init__(self, rn, y, S, Dv, K, batch):
        self.y, self.S, self.Dv, self.K, self.batch = y, S, Dv, K, batch
        self.w, self.bias = rn(Dv, K, sc=0.05), rn(Dv)
        self.ldc = (S + 63) // 64 * 64

    def fresh(self):
        return torch.full((self.batch, self.Dv, self.ldc), SENT, dtype=BF, device="cuda")

    def call(self, c):
        return ((self.w, self.y, c, self.Dv, self.S, self.K, self.K, self.K, self.ldc),
                dict(bias=self.bias, batch=self.batch, strideB=self.S * self.K, strideC=self.Dv * self.ldc,
                     flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS))

    def check(self, c, what):
        perm = torch.tensor([swap23(n) for n in range(self.S)], device="cuda")
        outside = torch.ones(self.ldc, dtype=torch.bool, device="cuda")
        outside[perm] = False
        assert bool((c[:, :, outside] == SENT).all()), (what, "written outside the permuted columns")
        rows, b = _edge_rows(self.Dv), self.batch - 1
        ref = self.w[rows].double() @ self.y[b].double().t() + self.bias.double()[rows, None]
        _close(c[b][rows][:, perm], ref, what)


def _singles(*probs):
    cs = [p.fresh() for p in probs]
    for p, c in zip(probs, cs):
        a_, kw = p.call(c)
        _lib.gemm(*a_, **kw)
    return cs


# (M, N1, N2, K, batch): the C2 Q|K / V^T shape, then M and N off the 256-tile, N % 8 != 0, K = 128, K / 64 odd
PAIR_SHAPES = {"c2": (17776, 6144, 3072, 3072, 2), "m1000_n768_k192": (1000, 768, 512, 192, 2),
               "m300_n520_k192": (300, 520, 264, 192, 1), "m257_n250_k128": (257, 250, 1001, 128, 2),
               "m513_n1001_k320": (513, 1001, 96, 320, 1)}
PLACES = ["packed_first", "packed_second", "packed_both", "packed_with_vt", "vt_with_packed"]


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("shape", list(PAIR_SHAPES))
def test_gemm_pair_with_a_packed_weight_equals_its_single_calls(monkeypatch, shape, place, pipe):
    """a PackedB in either problem of alg_gemm_bf16_pair, beside a row-major problem, another packed one, or the V^T projection
    that reads the same activations (the Q|K + V^T fold): the pair's output is the single calls' output, bit for bit, and it
    meets float64; nothing outside either [M, N] window is written"""
    monkeypatch.setenv("ALG_GEMM_PIPE", pipe)
    M, N1, N2, K, batch = PAIR_SHAPES[shape]
    rn = _gen(M + N1 + K)
    y = rn(batch, M, K)
    lin = lambda N, packed: Lin(rn, y, M, N, K, batch, packed)
    probs = {"packed_first": lambda: (lin(N1, True), lin(N2, False)),
             "packed_second": lambda: (lin(N1, False), lin(N2, True)),
             "packed_both": lambda: (lin(N1, True), lin(N2, True)),
             "packed_with_vt": lambda: (lin(N1, True), VT(rn, y, M, N2, K, batch)),
             "vt_with_packed": lambda: (VT(rn, y, M, N2, K, batch), lin(N1, True))}[place]()
    want = _singles(*probs)
    got = [p.fresh() for p in probs]
    _lib.gemm_pair(probs[0].call(got[0]), probs[1].call(got[1]))
    for i, (p, g, w) in enumerate(zip(probs, got, want)):
        what = (shape, place, pipe, i)
        p.check(w, what + ("single",))
        assert torch.equal(g, w), what
        p.check(g, what)


QK_GRID = [(300, 8, 3, 17, True, 1.0), (1000, 4, 1, 0, True, 0.18033688), (257, 12, 2, 257, True, 1.0),
           (530, 4, 2, 100, False, 0.18033688), (300, 16, 2, 17, True, 0.18033688), (130, 32, 1, 0, False, 1.0)]


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("S,heads,N,T,rope,qs", QK_GRID)
def test_gemm_pair_qk_with_a_packed_qk_weight(monkeypatch, pipe, S, heads, N, T, rope, qs):
    """heads % 4 == 0 (the fused store loop's shape) with the Q|K weight packed: the result is the packed single call followed by
    qk_norm_rope_, bit for bit; the single call meets float64 before the norm; V^T is the single call's"""
    monkeypatch.setenv("ALG_GEMM_PIPE", pipe)
    D = heads * 64
    rn = _gen(S + heads)
    y = rn(N, S, D)
    qk, vt = Lin(rn, y, S, 2 * D, D, N, True, ldc=2 * D), VT(rn, y, S, D, D, N)
    wq, bq, wk, bk = (1 + rn(64, sc=0.2)), rn(64, sc=0.2), (1 + rn(64, sc=0.2)), rn(64, sc=0.2)
    ang = torch.rand(max(S - T, 1), 32, generator=torch.Generator(device="cuda").manual_seed(S), device="cuda") * 6.28
    cos = ang.cos().repeat_interleave(2, dim=1).contiguous() if rope else None
    sin = ang.sin().repeat_interleave(2, dim=1).contiguous() if rope else None
    qk0, vt0 = _singles(qk, vt)
    qk.check(qk0, "qk before the norm")
    vt.check(vt0, "vt")
    _lib.qk_norm_rope_(qk0, wq, bq, wk, bk, cos, sin, N, S, heads, T, 1e-6, q_scale=qs)
    qk1, vt1 = qk.fresh(), vt.fresh()
    _lib.gemm_pair_qk(qk.call(qk1), vt.call(vt1), wq, bq, wk, bk, cos, sin, heads, T, 1e-6, q_scale=qs)
    assert torch.equal(vt1, vt0)
    if not torch.equal(qk1, qk0):
        d = (qk1.float() - qk0.float()).abs()
        raise AssertionError("pair_qk != packed gemm + qk_norm_rope_: %d elements, max %.4g" % (int((d > 0).sum()), d.max().item()))


def _quant(x):
    rows, K = x.shape
    q = torch.empty(rows, K, dtype=torch.uint8, device="cuda")
    s = torch.empty(rows, dtype=torch.float32, device="cuda")
    _lib.quantize_fp8_rows(x, q, s, rows, K)
    return q, s


def test_fp8_gemm_refuses_a_packed_weight():
    """the e4m3 GEMM reads B as row-major bytes: a PackedB with row scales is refused in Python, and the flag on a raw call is
    refused by alg_gemm_fp8 itself (ALG_EINVAL, C untouched) -- the same operands without the flag do run"""
    rn = _gen(8)
    M, N, K = 300, 512, 256
    a, w = rn(M, K), rn(N, K, sc=0.05)
    qa, sa = _quant(a)
    qw, sw = _quant(w)
    c = torch.full((M, N), SENT, dtype=BF, device="cuda")
    with pytest.raises(_lib.AlgHipError):
        _lib.gemm(qa, _lib.PackedB(w), c, M, N, K, K, K, N, a_scale=sa, b_scale=sw)
    lib = _lib.load_library()
    args, fp8 = _lib.gemm_args(qa, qw, c, M, N, K, K, K, N, flags=_lib.GEMM_B_PACKED11, a_scale=sa, b_scale=sw)
    assert fp8
    rc = lib.alg_gemm_fp8(ctypes.byref(args), _lib._stream())
    torch.cuda.synchronize()
    assert rc == ALG_EINVAL and b"PACKED11" in lib.alg_last_error()
    assert bool((c == SENT).all())
    args.flags = 0
    assert lib.alg_gemm_fp8(ctypes.byref(args), _lib._stream()) == 0
    assert not bool((c == SENT).any())


def test_convolution_addressing_refuses_a_packed_weight():
    """a raw alg_gemm_bf16 call with valid convolution addressing (3 x 3 taps of 64 channels) and the packed flag"""
    Cin, M, N, wp, hpwp = 64, 256, 64, 8, 64
    K = 9 * Cin
    rn = _gen(5)
    x, w = rn(M + 2 * hpwp + 2 * wp + 3 + 256, Cin), rn(N, K, sc=0.05)
    c = torch.full((M, N), SENT, dtype=BF, device="cuda")
    args, _ = _lib.gemm_args(x, w, c, M, N, K, Cin, K, N, flags=_lib.GEMM_B_PACKED11)
    args.conv_cin_log2, args.conv_wp, args.conv_hpwp, args.conv_kw = 6, wp, hpwp, 3
    lib = _lib.load_library()
    rc = lib.alg_gemm_bf16(ctypes.byref(args), _lib._stream())
    torch.cuda.synchronize()
    assert rc == ALG_EINVAL and b"PACKED11" in lib.alg_last_error()
    assert bool((c == SENT).all())


BAD = ["per_row_bias", "strided_b", "k64", "unaligned_b"]


def _bad(kind, rn, y, S, K, batch):
    """an invalid packed call on the activations y [batch][S][K]: N = 512, two whole column tiles, and every B it names is readable
    as a row-major [batch][N][K] weight"""
    N = 512
    c = torch.full((batch, S, N), SENT, dtype=BF, device="cuda")
    kw = dict(batch=batch, strideA=S * K, strideC=S * N)
    if kind == "per_row_bias":             # the V^T epilogue on a packed weight
        return ((y, _lib.PackedB(rn(N, K, sc=0.05)), c, S, N, K, K, K, N), dict(kw, bias=rn(S), flags=_lib.GEMM_BIAS_PER_ROW)), c
    if kind == "strided_b":                # raw flag with a per-batch B (a whole row-major weight per batch item)
        return ((y, rn(batch, N, K, sc=0.05), c, S, N, K, K, K, N), dict(kw, strideB=N * K, flags=_lib.GEMM_B_PACKED11)), c
    if kind == "k64":                      # raw flag with one k-tile (schedule 11 needs two)
        return ((y, rn(N, 64, sc=0.05), c, S, N, 64, K, 64, N), dict(kw, flags=_lib.GEMM_B_PACKED11)), c
    return ((y, rn(N + 1, K, sc=0.05), c, S, N, K, K, K, N), dict(kw, b_off=1, flags=_lib.GEMM_B_PACKED11)), c   # B not 16-byte aligned


@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("kind", BAD)
def test_a_bad_packed_problem_is_refused_before_the_other_problem_is_launched(monkeypatch, kind, pipe):
    """alg_gemm_bf16_pair(good, bad), (bad, good) and alg_gemm_bf16_pair_qk(good qk, bad): the call raises and neither C changes"""
    monkeypatch.setenv("ALG_GEMM_PIPE", pipe)
    S, heads, batch = 300, 4, 2
    D = heads * 64
    rn = _gen(3)
    y = rn(batch, S, D)
    for form in ("pair", "pair_swapped", "pair_qk"):
        good = Lin(rn, y, S, 2 * D, D, batch, False, ldc=2 * D if form == "pair_qk" else None)
        cg = good.fresh()
        bad, cb = _bad(kind, rn, y, S, D, batch)
        with pytest.raises(_lib.AlgHipError):
            if form == "pair":
                _lib.gemm_pair(good.call(cg), bad)
            elif form == "pair_swapped":
                _lib.gemm_pair(bad, good.call(cg))
            else:
                e = [1 + rn(64, sc=0.2), rn(64, sc=0.2), 1 + rn(64, sc=0.2), rn(64, sc=0.2)]
                _lib.gemm_pair_qk(good.call(cg), bad, *e, None, None, heads, 0, 1e-6)
        assert bool((cg == SENT).all()), (kind, pipe, form, "the good problem was launched")
        assert bool((cb == SENT).all()), (kind, pipe, form, "the bad problem was launched")


# the HunyuanVideo single-stream form: N*J rows into the column window [c_off, c_off + N) of a wide buffer; at ldc = 16384 a
# slab is 130,816 rows, so M = 140,000 makes two
TALL = dict(M=140_000, N=512, K=128, ldc=16384, c_off=256)


def _untouched_outside(c, lo, hi, step=16384):
    for r in range(0, c.shape[0], step):
        blk = c[r:r + step]
        assert bool((blk[:, :lo] == SENT).all()) and bool((blk[:, hi:] == SENT).all()), ("written outside the window", r)


def test_tall_packed_call_through_the_slab_split(monkeypatch):
    monkeypatch.setenv("ALG_GEMM_PIPE", "10")
    M, N, K, ldc, c0 = TALL["M"], TALL["N"], TALL["K"], TALL["ldc"], TALL["c_off"]
    slab = ((1 << 31) - 1) // ldc // 256 * 256
    assert slab == 130_816 and M * ldc >= 1 << 31 and slab < M < 2 * slab
    rn = _gen(140)
    a, w, bias = rn(M, K), rn(N, K, sc=0.05), rn(N)
    c = torch.full((M, ldc), SENT, dtype=BF, device="cuda")
    _lib.gemm(a, _lib.PackedB(w), c, M, N, K, K, K, ldc, bias=bias, c_off=c0)
    got = c[:, c0:c0 + N].clone()
    _untouched_outside(c, c0, c0 + N)
    c[:, c0:c0 + N] = SENT
    _lib.gemm(a, w, c, M, N, K, K, K, ldc, bias=bias, c_off=c0)
    same = torch.equal(c[:, c0:c0 + N], got)
    del c
    assert same, "the packed tall call differs from the row-major one"
    rows = torch.tensor([0, slab - 1, slab, M - 1], device="cuda")
    _close(got[rows], a[rows].double() @ w.double().t() + bias.double(), "tall")
    del got, a


def test_bad_tall_packed_call_is_refused_before_any_slab_runs():
    """a per-row bias on a packed weight, on a call that needs two slabs: refused up front, C untouched"""
    M, N, K, ldc, c0 = TALL["M"], TALL["N"], TALL["K"], TALL["ldc"], TALL["c_off"]
    a = torch.zeros(M, K, dtype=BF, device="cuda")
    pk = _lib.PackedB(torch.zeros(N, K, dtype=BF, device="cuda"))
    c = torch.full((M, ldc), SENT, dtype=BF, device="cuda")
    with pytest.raises(_lib.AlgHipError):
        _lib.gemm(a, pk, c, M, N, K, K, K, ldc, bias=torch.zeros(M, dtype=BF, device="cuda"), flags=_lib.GEMM_BIAS_PER_ROW, c_off=c0)
    untouched = bool((c[:, c0:c0 + N] == SENT).all())
    del c, a
    assert untouched


def _tiles(pk):
    return pk.data.cpu().numpy().view(np.uint16).reshape(-1, pk.K // 64, 4, 2, 4, 64, 8)


def _check_packing(pk, w):
    got, wf = _tiles(pk), w.float().cpu().numpy()
    assert got.shape[0] == (w.shape[0] + 255) // 256
    for t in range(got.shape[0]):
        assert np.array_equal(got[t], gemm_emu.pack_b_p11(wf[256 * t:256 * t + 256], pk.K // 64)), ("tile", t)


@pytest.mark.parametrize("K", [128, 192, 640])
@pytest.mark.parametrize("N", [6, 250, 256, 520])
def test_packer_matches_the_cpu_restatement_of_its_layout(N, K):
    w = _gen(N + K)(N, K)
    _check_packing(_lib.PackedB(w), w)


@pytest.mark.parametrize("N,K", [(6, 128), (250, 192), (520, 640)])
def test_packer_reads_a_column_window_of_a_wider_weight(N, K):
    """w = w_wide[:, 64:64 + K] (row pitch > K): packed like its contiguous copy; rows past N in the last tile are zeros even where
    the packed buffer's memory held other bytes before"""
    w_wide = _gen(N * K)(N, K + 192)
    w = w_wide[:, 64:64 + K]
    assert w.stride(0) == K + 192
    nbytes = int(_lib.load_library().alg_pack_b_p11_bytes(N, K))
    junk = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")   # the caching allocator hands this block to PackedB
    del junk
    pk = _lib.PackedB(w)
    assert torch.equal(pk.data, _lib.PackedB(w.contiguous()).data)
    _check_packing(pk, w)
    last = _tiles(pk)[-1].transpose(1, 3, 4, 0, 2, 5)          # [wave][n-block][lane][k-tile][k-step][8]
    n = 64 * np.arange(4)[:, None, None] + 16 * np.arange(4)[None, :, None] + (np.arange(64) & 15)[None, None, :]
    dead = n >= N - 256 * (_tiles(pk).shape[0] - 1)
    assert dead.any() and not last[dead].any() and last[~dead].any()


def test_this_file_and_the_layout_restatement_import_nothing_from_the_oracle():
    """gemm_emu restates the packed layout from numpy and the scripts/ generators alone; neither it nor this file reads oracle/"""
    for path in (os.path.abspath(__file__), os.path.abspath(gemm_emu.__file__)):
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            names = ([a.name for a in node.names] if isinstance(node, ast.Import) else
                     [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
            assert not any(n.split(".")[0] == "oracle" for n in names), (path, names)
    oracle_dir = os.path.join(ROOT, "oracle") + os.sep
    for v in vars(gemm_emu).values():
        if isinstance(v, types.ModuleType):
            assert not os.path.abspath(getattr(v, "__file__", None) or "").startswith(oracle_dir), v.__name__
