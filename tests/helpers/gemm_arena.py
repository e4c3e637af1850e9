"""Test helper: the operands of the GEMM entries (alg_gemm_bf16, _pair, _pair_qk, alg_gemm_fp8, alg_gemm_fp4, _q4out; include/alg_hip.h)
laid out inside flat ARENAS that belong to the test, with guard bands in front of and behind every operand, filled with data on which
the call's result does not depend on the accumulation order, and a float64 statement of the header's contract to compare with.

An operand is handed to the `_lib` wrappers as a flat view that begins at its first element (the wrappers take `data_ptr()`), with the
pitches and batch strides its geometry gives it.  The geometry of a case is the tight one (pitch = width, batch stride = rows * pitch,
every first element 16-byte aligned) changed by exactly one TRIGGER: the ways a call leaves the LDS-staged epilogue of
csrc/gemm_kernel.h for the element-exact one (an 8-byte but not 16-byte aligned C / R / gate, a pitch or batch stride = 4 (mod 8), a
perm_col0 that is no multiple of 16), a gate_seg_stride of 0 / N + 4 / N + 8, row and column windows on A and B, batch strides with
gaps, batch strides on the scales.

Guards: 256 rows of the operand's pitch in front of and behind every 2-D operand, 1024 elements around the vectors (bias, gate,
scales).  What a prefetch a few tiles past a panel could read lands inside the arena's own allocation; nothing here reaches, or relies
on, memory outside an allocation.

Fills: `friendly` puts zeros everywhere outside the live elements.  `hostile` puts NaN there -- bf16 0x7FC0, e4m3 byte 0x7F, float32
NaN, E8M0 byte 0xFF; packed e2m1 has no NaN, its bytes are 0x77 (6.0 | 6.0) -- so A rows >= M and columns >= K inside lda, B rows
>= N, the bias behind N (or M), the gate behind N inside a segment and behind the second segment, the scales behind M / N, R rows
>= M and columns >= N and every gap between batch items are NaN.  Both fills pre-fill the C arena with the canary 0x7FC1 (a
residual that aliases C then sits in C's window).  A `PackedB` is packed by the test from the hostile-filled weight window.

Exact data: A and B hold a few small integers and halves, the bias and the residual multiples of 1/4, a bf16 gate multiples of 1/4,
a float32 gate multiples of 1/16, e4m3 row scales powers of two in [2^-2, 2^2] that differ from row to row, E8M0 block scales that
differ from block to block.  Then the K-term sum (in ANY order), acc * a_scale * b_scale, + bias, gate * x and r + ... are all exact
in float32: schedules 6, 9, 10, 11, the e4m3 loops and the FP4 kernel have to produce the same bits.  `reference` does not assume
that, it asserts it: every such intermediate, computed in float64, has to survive a round trip through float32.

Pure torch, runs on either device."""
import math
import zlib
from collections import namedtuple

import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
FILLS = ("friendly", "hostile")
NAN_BITS = 0x7FC0
CANARY_BITS = 0x7FC1
GUARD = 256            # rows of every guard band: one tile
VEC_GUARD = 1024       # elements around bias / gate / scales
ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2
BIAS_PER_ROW, PERMUTE_COLS, GATE_F32 = 1, 4, 8         # ALG_GEMM_* of include/alg_hip.h
TINY = 2.0 ** -100

Case = namedtuple("Case", "route form trigger M N K batch")

# ---------------------------------------------------------------------------------------------------------------------- forms
# bias: "col" | "row" (BIAS_PER_ROW); res: None | "alias" (R is C) | "own"; gate: None | "bf16" | "f32";
# split: where seg_split falls -- "mid" inside the first tile of rows, "side" on a tile boundary (every tile wholly on one side),
# "all0" = M (every row takes gate[0])
FORMS = {
    "bias": dict(bias="col"),
    "gelu": dict(bias="col", act=ACT_GELU),
    "silu": dict(bias="col", act=ACT_SILU),
    "vt": dict(bias="row", perm=True),
    "rowbias_gelu": dict(bias="row", act=ACT_GELU),
    "res": dict(bias="col", res="own"),
    "res_gate_bf16": dict(bias="col", res="alias", gate="bf16", split="mid"),
    "res_gate_f32_side": dict(bias="col", res="own", gate="f32", split="side"),
    "res_gate_f32_straddle": dict(bias="col", res="alias", gate="f32", split="mid"),
    "res_alias": dict(bias="col", res="alias"),
    "res_noalias": dict(bias="col", res="own", gate="bf16", split="all0"),
}
ROW_BIAS_FORMS = ("vt", "rowbias_gelu")
RES_FORMS = tuple(f for f, d in FORMS.items() if d.get("res"))


def form_of(case):
    d = dict(bias=None, act=ACT_NONE, perm=False, res=None, gate=None, split=None)
    d.update(FORMS[case.form])
    return d


def seg_split_of(case):
    how = form_of(case)["split"]
    if how == "mid":
        return max(case.M // 3, 1)
    if how == "side":
        return 256 if case.M > 256 else 0
    return case.M if how == "all0" else 0


# --------------------------------------------------------------------------------------------------------------------- routes
# route -> (operand kind, ALG_GEMM_PIPE the GPU test sets)
ROUTES = {"p6": ("bf16", "6"), "p9": ("bf16", "9"), "p10": ("bf16", "10"), "p11": ("bf16", "10"), "k64": ("bf16", "10"),
          "fp8_p6": ("fp8", "6"), "fp8_p9": ("fp8", "9"), "fp4": ("fp4", "10"), "fp4_q4out": ("fp4", "10"),
          "pair": ("bf16", "10"), "pair_qk": ("bf16", "9")}
SHAPE_TRIGGERS = ("n516", "n250", "n6")        # N % 4 == 0 only; N % 4 != 0; less than one quad row (M = 33)
C_TRIGGERS = ("c_off4", "ldc4", "strideC4")
R_TRIGGERS = ("r_off4", "ldr4", "strideR4")
GATE_TRIGGERS = ("gate_off4", "strideGate4", "gseg0", "gsegN4", "gsegN8")
PERM_TRIGGERS = ("perm0", "perm16", "perm4", "perm180", "perm37")
TRIGGERS = ("none",) + SHAPE_TRIGGERS + C_TRIGGERS + R_TRIGGERS + GATE_TRIGGERS + PERM_TRIGGERS + \
    ("windows", "gaps", "scales", "second_tile")
_NO_RES = {t: "the entry takes no residual" for t in R_TRIGGERS + GATE_TRIGGERS}
_NO_PERM = {t: "the route's check refuses PERMUTE_COLS" for t in PERM_TRIGGERS}
_NO_SCALES = {"scales": "bf16 operands carry no scales"}
# what a route's check refuses, or what does not exist on it: (route, trigger) pairs the table leaves out, with the reason
REFUSED = {
    "p6": _NO_SCALES, "p9": _NO_SCALES, "p10": _NO_SCALES, "k64": _NO_SCALES,
    "p11": dict(_NO_SCALES, **{t: "schedule 11 refuses a per-row bias and a column permutation" for t in PERM_TRIGGERS}),
    "fp8_p6": {}, "fp8_p9": {},
    "fp4": dict(_NO_PERM, second_tile="alg_gemm_fp4 launches one workgroup per tile: no second tile"),
    "fp4_q4out": dict(_NO_PERM, **_NO_RES, **{t: "the e2m1 C must be 16-byte aligned, ldc / strideC multiples of 32" for t in C_TRIGGERS},
                      **{t: "N % 32 == 0 is required" for t in SHAPE_TRIGGERS},
                      second_tile="alg_gemm_fp4_q4out launches one workgroup per tile: no second tile"),
    "pair": dict(_NO_SCALES, **_NO_RES),
    "pair_qk": dict(_NO_SCALES, **_NO_RES, **{t: "qk->C is the contiguous [batch][S][2][heads][64] tensor and N = 2 * heads * 64"
                                                for t in SHAPE_TRIGGERS + ("gaps",)}),
}
REQUIRED = [(r, t) for r in ROUTES for t in TRIGGERS if t not in REFUSED[r]]


def case_id(c):
    return "%s-%s-%s-%dx%dx%dx%d" % (c.route, c.form, c.trigger, c.batch, c.M, c.N, c.K)


def table(cus=8):
    """Every case of tests/test_gpu_gemm_operands.py.  cus: the device's CU count -- the `second_tile` cases take a batch at which
    every workgroup of the persistent launch walks at least two tiles (batch * tiles >= 2 * cus + 8)."""
    out = []
    for route, (kind, _) in ROUTES.items():
        k_lo, k_hi = {"bf16": (128, 192), "fp8": (256, 384) if route == "fp8_p9" else (128, 256), "fp4": (256, 512)}[kind]
        if route == "k64":
            k_lo = k_hi = 64
        n_full = 544 if route == "fp4_q4out" else 512 if route == "pair_qk" else 520
        # 256 x 256 tiles per batch item: 2 x 3 at M = 300, N = 520; a pair adds the 1 x 3 of its V^T problem (pair_qk: 2 x 2 + 1 x 3)
        tiles = {"pair": 9, "pair_qk": 7}.get(route, 6)
        many = -(-(2 * cus + 8) // tiles)

        def add(form, trigger, M=300, N=n_full, K=k_lo, batch=2):
            if trigger in REFUSED[route]:
                return
            if form in ROW_BIAS_FORMS and (route == "p11" or kind == "fp4"):
                return                              # refused by the route's check: a per-row bias / a permutation
            if form in RES_FORMS and route == "fp4_q4out":
                return                              # refused: the MXFP4 output has no residual
            if route == "fp4_q4out" and form == "silu":
                return                              # refused: ALG_ACT_NONE or ALG_ACT_GELU_TANH
            out.append(Case(route, form, trigger, M, N, K, batch))

        if route in ("pair", "pair_qk"):
            # the two problems of a pair case: `form` names them; build_pair() makes the calls
            for trig in TRIGGERS:
                if trig == "second_tile":
                    add("bias+vt", trig, batch=many)
                elif trig in SHAPE_TRIGGERS:
                    add("bias+vt", trig, M=33 if trig == "n6" else 300, N={"n516": 516, "n250": 250, "n6": 6}[trig])
                else:
                    add("bias+vt", trig, K=k_hi if trig == "none" else k_lo)
            continue
        for form in FORMS:                                           # every form on the staged epilogue, one steady-state trip
            add(form, "none", K=k_hi)
        for trig, (M, N) in zip(SHAPE_TRIGGERS, ((300, 516), (300, 250), (33, 6))):
            for form in ("bias", "gelu", "vt", "res_gate_bf16", "res_gate_f32_straddle", "res_noalias"):
                add(form, trig, M=M, N=N, batch=3 if M == 33 else 2)
        for trig in C_TRIGGERS:
            for form in ("bias", "silu", "res"):
                add(form, trig)
        for trig in R_TRIGGERS:
            for form in ("res", "res_gate_f32_side"):
                add(form, trig)
        add("res_gate_bf16", "gate_off4")
        add("res_noalias", "gate_off4")
        for trig in ("strideGate4", "gseg0", "gsegN4", "gsegN8"):
            for form in ("res_gate_bf16", "res_gate_f32_side", "res_gate_f32_straddle"):
                add(form, trig)
        for trig in PERM_TRIGGERS:
            add("vt", trig)
        for trig in ("windows", "gaps", "scales"):
            for form in ("bias", "gelu", "vt", "res_gate_bf16", "res_gate_f32_side"):
                add(form, trig)
        for form in ("bias", "res_gate_bf16"):
            add(form, "second_tile", batch=many)
    return out


# ------------------------------------------------------------------------------------------------------------------- geometry
def swap23(n):
    """The column permutation of ALG_GEMM_PERMUTE_COLS: index bits 2 and 3 swapped."""
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


def ceil_to(n, m):
    return (n + m - 1) // m * m


def geometry(case):
    """Pitches, offsets into a row (`*_x`), batch strides and the scalar arguments of one case: the tight geometry with the case's
    trigger applied.  Everything counts elements (MXFP4 A / B: e2m1 elements, two per byte; its scales: bytes)."""
    f, t, M, N, K = form_of(case), case.trigger, case.M, case.N, case.K
    kind = ROUTES[case.route][0]
    q4 = case.route == "fp4_q4out"
    g = dict(lda=K, ldb=K, a_x=0, b_x=0, a_row=0, b_row=0, ldc=ceil_to(N, 32) if q4 else N, c_x=0, c_row=0, r_x=0, r_row=0,
             gate_off=0, gseg=None, bias_off=0, perm_col0=0, gap=0, scale_gap=0)
    g["ldr"] = g["ldc"]
    al = {"bf16": 8, "fp8": 16, "fp4": 32}[kind]
    if t == "c_off4":
        g.update(ldc=N + 8, c_x=4)
    elif t == "ldc4":
        g.update(ldc=N + 4)
    elif t == "r_off4":
        g.update(ldr=N + 8, r_x=4)
    elif t == "ldr4":
        g.update(ldr=N + 4)
    elif t == "gate_off4":
        g.update(gate_off=4)
    elif t in ("gseg0", "gsegN4", "gsegN8"):
        g.update(gseg={"gseg0": 0, "gsegN4": N + 4, "gsegN8": N + 8}[t])
    elif t in PERM_TRIGGERS:
        g.update(perm_col0=int(t[4:]))
    elif t == "windows":       # A and B are row and column windows of wider buffers; C, R one too (16-byte aligned: still staged)
        g.update(lda=K + 2 * al, a_x=al, a_row=3, ldb=K + 3 * al, b_x=2 * al, b_row=5, c_row=2, r_row=7, bias_off=8, gate_off=16)
        if not q4:
            g.update(ldc=N + 24 if N % 4 == 0 else N + 3, c_x=8 if N % 4 == 0 else 3, ldr=N + 40 if N % 4 == 0 else N + 5,
                     r_x=16 if N % 4 == 0 else 1)
        else:
            g.update(ldc=g["ldc"] + 64, c_x=32)
    elif t == "gaps":
        g.update(gap=3)        # rows of the operand's pitch (and 8 more elements) between batch items
    elif t == "scales":
        g.update(scale_gap=24)
    if f["perm"]:              # C points at joint column 0 of a row that holds perm_col0 + N columns, 64 at a time, and a tail
        g["ldc"] = max(g["ldc"], ceil_to(g["perm_col0"] + N, 64) + (4 if t == "ldc4" else 8 if t == "c_off4" else 0))
    if f["res"] == "alias":
        g.update(ldr=g["ldc"], r_x=g["c_x"], r_row=g["c_row"])
    gap = lambda rows, ld: rows * ld + (g["gap"] * ld + 8 if g["gap"] else 0)
    shared_a = f["perm"]       # the V^T form: A is the weight (shared by the batch), B the activations (one per batch item)
    g["strideA"] = 0 if shared_a else gap(M + g["a_row"], g["lda"])
    g["strideB"] = gap(N + g["b_row"], g["ldb"]) if shared_a or (t == "gaps" and case.route != "p11") else 0
    if g["gap"]:
        g["strideA"], g["strideB"] = ceil_to(g["strideA"], al), ceil_to(g["strideB"], al)
    g["strideC"] = gap(M + g["c_row"], g["ldc"]) + (12 if t == "strideC4" else 0)
    if q4:
        g["strideC"] = ceil_to(g["strideC"], 32)
    g["strideR"] = g["strideC"] if f["res"] == "alias" else gap(M + g["r_row"], g["ldr"]) + (12 if t == "strideR4" else 0)
    gs = N if g["gseg"] is None else g["gseg"]
    g["strideGate"] = ceil_to(gs + N, 8) + g["gate_off"] + (8 if g["gap"] else 0) + (12 if t == "strideGate4" else 0)
    if t == "gate_off4":
        g["strideGate"] = ceil_to(gs + N, 8) + 8
    if kind == "fp8":
        g["strideAScale"] = 0 if shared_a else M + g["scale_gap"] + (5 if g["scale_gap"] else 0)
        g["strideBScale"] = ceil_to(N, 4) + g["scale_gap"] if g["strideB"] else 0
    if kind == "fp4":
        g["strideAScale"] = 0 if shared_a else ceil_to(M * (K // 32), 8) + g["scale_gap"]
        g["strideBScale"] = ceil_to(N * (K // 32), 8) + g["scale_gap"] if g["strideB"] else 0
        g["strideOutScales"] = ceil_to(M * (N // 32), 8) + g["scale_gap"] if q4 else 0
    g["seg_split"] = seg_split_of(case)
    g["flags"] = (BIAS_PER_ROW if f["bias"] == "row" else 0) | (PERMUTE_COLS if f["perm"] else 0) | (GATE_F32 if f["gate"] == "f32" else 0)
    return g


def staged(case, g=None):
    """Whether the schedules of csrc/gemm_kernel.h take the case through the LDS-staged epilogue, from the header's rule alone:
    N % 8 == 0, C / R / gate 16-byte aligned with pitches and batch strides in multiples of 8, perm_col0 % 16 == 0, and no per-row
    bias next to an activation or a residual."""
    g, f, N = g or geometry(case), form_of(case), case.N
    ok = N % 8 == 0 and g["ldc"] % 8 == 0 and g["strideC"] % 8 == 0 and g["c_x"] % 8 == 0 and g["perm_col0"] % 16 == 0
    if f["res"]:
        ok = ok and g["ldr"] % 8 == 0 and g["strideR"] % 8 == 0 and g["r_x"] % 8 == 0
    if f["gate"]:
        per16 = 8 if f["gate"] == "bf16" else 4
        ok = ok and g["strideGate"] % 8 == 0 and (N if g["gseg"] is None else g["gseg"]) % 8 == 0 and g["gate_off"] % per16 == 0
    if f["bias"] == "row" and (f["act"] != ACT_NONE or f["res"]):
        ok = False
    return ok


# --------------------------------------------------------------------------------------------------------------------- arenas
class Op:
    """An operand inside the flat tensor `full`: element (b, r, c) at off + b * bs + r * ld + c.  `view` is what a wrapper takes."""

    def __init__(self, full, off, bs, ld, B, rows, cols):
        self.full, self.off, self.bs, self.ld, self.B, self.rows, self.cols = full, off, bs, ld, B, rows, cols

    @property
    def view(self):
        return self.full[self.off:]

    def window(self, full=None):
        return torch.as_strided(self.full if full is None else full, (self.B, self.rows, self.cols), (self.bs, self.ld, 1), self.off)


def _bits16(value, n, device):
    return torch.full((n,), value - 65536 if value >= 32768 else value, dtype=torch.int16, device=device).view(BF)


_HOSTILE_BYTE = {"f8": 0x7F, "e2m1": 0x77, "e8m0": 0xFF}


def _alloc(kind, n, fill, device):
    hostile = fill == "hostile"
    if kind == "bf16":
        return _bits16(NAN_BITS if hostile else 0, n, device)
    if kind == "f32":
        return torch.full((n,), float("nan") if hostile else 0.0, dtype=torch.float32, device=device)
    return torch.full((n,), _HOSTILE_BYTE[kind] if hostile else 0, dtype=torch.uint8, device=device)


def _place(kind, fill, device, B, rows, cols, ld, bs, x=0, row0=0, values=None):
    """An arena for a [B][rows][cols] operand whose first element sits `row0` rows and `x` elements behind the front guard."""
    guard = ceil_to(GUARD * ld, 64) if rows > 1 or ld > cols else VEC_GUARD
    off = guard + row0 * ld + x
    n = off + (B - 1) * bs + (rows - 1) * ld + cols + guard
    op = Op(_alloc(kind, n, fill, device), off, bs, ld, B, rows, cols)
    if values is not None:
        op.window().copy_(values.to(device))
    return op


def _canary(n, device, dtype=BF):
    c = _bits16(CANARY_BITS, (n + 1) // 2 if dtype == torch.uint8 else n, device)
    return c.view(torch.uint8)[:n] if dtype == torch.uint8 else c


def _ibits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


# ----------------------------------------------------------------------------------------------------------------------- data
def _grid(gen, shape, lo, hi, step):
    """Random multiples of `step` in [lo, hi], float64."""
    return torch.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape, generator=gen).double() * step


def _sparse(gen, rows_shape, K, nnz, values):
    """[..., K] with exactly nnz non-zeros per row, drawn from `values`, at positions spread over the whole of K."""
    pos = torch.rand(*rows_shape, K, generator=gen).topk(nnz, dim=-1).indices
    val = torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), (*rows_shape, nnz), generator=gen)]
    return torch.zeros(*rows_shape, K, dtype=torch.float64).scatter_(-1, pos, val)


def make_data(case, g):
    """The compact float64 values of every operand of a case (the same under both fills): a dict.  An activation form keeps
    A sparse and the scales small, so that every pre-activation value lies on the 1/8 grid inside [-6, 6]."""
    f, M, N, K, B = form_of(case), case.M, case.N, case.K, case.batch
    kind = ROUTES[case.route][0]
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    small = f["act"] != ACT_NONE
    Ba, Bb = (1 if g["strideA"] == 0 else B), (1 if g["strideB"] == 0 else B)
    d = {}
    halves = [-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]
    if kind == "bf16":
        d["A"] = _sparse(gen, (Ba, M), K, 4, [-1.0, -0.5, 0.5, 1.0]) if small else _grid(gen, (Ba, M, K), -2, 2, 0.5)
        d["B"] = _grid(gen, (Bb, N, K), -1, 1, 0.5) if small else _grid(gen, (Bb, N, K), -2, 2, 0.5)
    elif kind == "fp8":
        # small: |acc| <= 2 (integers), a_scale * b_scale in [1/8, 2]: |acc * scales| <= 4 on the 1/8 grid
        d["A"] = _sparse(gen, (Ba, M), K, 2, [-1.0, 1.0]) if small else _grid(gen, (Ba, M, K), -2, 2, 0.5)
        d["B"] = _grid(gen, (Bb, N, K), -1, 1, 1.0) if small else _grid(gen, (Bb, N, K), -2, 2, 0.5)
        # powers of two in [2^-2, 2^2]; neighbouring rows (and columns, and batch items) never share one
        m, n = torch.arange(M).reshape(1, M), torch.arange(N).reshape(1, N)
        ba, bb = torch.arange(Ba).reshape(Ba, 1), torch.arange(Bb).reshape(Bb, 1)
        ea = (m + ba) % 3 - 1 if small else (7 * m + ba) % 5 - 2
        eb = -((n + bb) % 3) if small else (3 * n + bb) % 5 - 2
        d["a_scale"], d["b_scale"] = torch.ldexp(torch.ones(Ba, M, dtype=torch.float64), ea), torch.ldexp(torch.ones(Bb, N, dtype=torch.float64), eb)
    else:
        # e2m1 codes times one E8M0 scale per block of 32 along K.  small: 4 terms of |a b| <= 1 on the 1/8 grid
        d["A"] = _sparse(gen, (Ba, M), K, 4, [-1.0, 1.0]) if small else torch.tensor(halves)[torch.randint(0, 9, (Ba, M, K), generator=gen)]
        d["B"] = _grid(gen, (Bb, N, K), -1, 1, 0.5) if small else torch.tensor(halves)[torch.randint(0, 9, (Bb, N, K), generator=gen)]
        lo = -1
        hi = 0 if small else 1
        d["a_exp"] = torch.randint(lo, hi + 1, (Ba, M, K // 32), generator=gen)
        d["b_exp"] = torch.randint(lo, hi + 1, (Bb, N, K // 32), generator=gen)
        for e in (d["a_exp"], d["b_exp"]):                            # the blocks of a row do not all share one scale
            e[..., 0] = lo
            e[..., -1] = hi
    n_bias = M if f["bias"] == "row" else N
    d["bias"] = _grid(gen, (n_bias,), -1.5, 1.5, 0.25)
    if f["res"]:
        d["R"] = _grid(gen, (B, M, N), -4, 4, 0.25)
    if f["gate"]:
        step = 0.25 if f["gate"] == "bf16" else 0.0625
        d["gate"] = _grid(gen, (B, 2, N), -2, 2, step)
        if g["gseg"] == 0:
            d["gate"][:, 1] = d["gate"][:, 0]                        # one gate: both segments are the same elements
    return d


def _e2m1_bytes(vals, exps):
    """Packed e2m1 bytes of values that sit on the e2m1 grid (before their block's scale is applied) -- element 2i in the low
    nibble of byte i -- and the E8M0 scale bytes of `exps`."""
    grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
    code = torch.searchsorted(grid, vals.abs().contiguous())
    assert bool((grid[code] == vals.abs()).all())
    code = (code + 8 * (vals < 0).long()).to(torch.uint8)
    c = code.reshape(*code.shape[:-1], code.shape[-1] // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8), (exps + 127).to(torch.uint8)


# ----------------------------------------------------------------------------------------------------------------------- call
class Call:
    """One call's arenas and arguments under one fill.  ops: name -> Op of every INPUT (A, B, bias, R when it does not alias C,
    gate, a_scale, b_scale); c: the C arena's Op (its `full` is a template: use fresh_c()); c_mask: bool over the C arena, True
    exactly where the call may write; out_scales / s_mask: the same for alg_gemm_fp4_q4out's second output."""

    def __init__(self, case, fill, device):
        self.case, self.fill, self.device = case, fill, device
        self.kind = ROUTES[case.route][0]
        self.q4 = case.route == "fp4_q4out"
        self.f, self.g = form_of(case), geometry(case)
        f, g, M, N, K, B = self.f, self.g, case.M, case.N, case.K, case.batch
        d = self.data = make_data(case, g)
        Ba, Bb = d["A"].shape[0], d["B"].shape[0]
        ops = self.ops = {}
        if self.kind == "bf16":
            ops["A"] = _place("bf16", fill, device, Ba, M, K, g["lda"], g["strideA"], g["a_x"], g["a_row"], d["A"].to(BF))
            ops["B"] = _place("bf16", fill, device, Bb, N, K, g["ldb"], g["strideB"], g["b_x"], g["b_row"], d["B"].to(BF))
        elif self.kind == "fp8":
            ops["A"] = _place("f8", fill, device, Ba, M, K, g["lda"], g["strideA"], g["a_x"], g["a_row"], d["A"].float().to(F8).view(torch.uint8))
            ops["B"] = _place("f8", fill, device, Bb, N, K, g["ldb"], g["strideB"], g["b_x"], g["b_row"], d["B"].float().to(F8).view(torch.uint8))
            ops["a_scale"] = _place("f32", fill, device, Ba, 1, M, M, g["strideAScale"], values=d["a_scale"].float().unsqueeze(1))
            ops["b_scale"] = _place("f32", fill, device, Bb, 1, N, N, g["strideBScale"], values=d["b_scale"].float().unsqueeze(1))
        else:      # byte units: two e2m1 elements per byte
            qa, sa = _e2m1_bytes(d["A"], d["a_exp"])
            qb, sb = _e2m1_bytes(d["B"], d["b_exp"])
            h = lambda name: g[name] // 2
            ops["A"] = _place("e2m1", fill, device, Ba, M, K // 2, h("lda"), h("strideA"), h("a_x"), g["a_row"], qa)
            ops["B"] = _place("e2m1", fill, device, Bb, N, K // 2, h("ldb"), h("strideB"), h("b_x"), g["b_row"], qb)
            kb = K // 32
            ops["a_scale"] = _place("e8m0", fill, device, Ba, 1, M * kb, M * kb, g["strideAScale"], values=sa.reshape(Ba, 1, M * kb))
            ops["b_scale"] = _place("e8m0", fill, device, Bb, 1, N * kb, N * kb, g["strideBScale"], values=sb.reshape(Bb, 1, N * kb))
        ops["bias"] = _place("bf16", fill, device, 1, 1, d["bias"].numel(), d["bias"].numel(), 0, g["bias_off"], values=d["bias"].to(BF).reshape(1, 1, -1))
        if f["res"] == "own":
            ops["R"] = _place("bf16", fill, device, B, M, N, g["ldr"], g["strideR"], g["r_x"], g["r_row"], d["R"].to(BF))
        if f["gate"]:
            gs = N if g["gseg"] is None else g["gseg"]
            segs = 1 if gs == 0 else 2
            vals = d["gate"][:, :segs].to(BF if f["gate"] == "bf16" else torch.float32)
            ops["gate"] = _place("bf16" if f["gate"] == "bf16" else "f32", fill, device, B, segs, N, max(gs, 1), g["strideGate"],
                                 g["gate_off"], values=vals)
            ops["gate"].rows, ops["gate"].ld = 2, gs                # read as two segments (a stride of 0: the same elements)
        # ---- C: the canary everywhere; a residual that aliases C in its window
        cols = torch.tensor([swap23(g["perm_col0"] + n) if f["perm"] else n for n in range(N)], dtype=torch.long, device=device)
        self.cols = cols
        width = int(cols.max()) + 1
        if self.q4:
            self.c = _place("e2m1", "friendly", device, B, M, N // 2, g["ldc"] // 2, g["strideC"] // 2, g["c_x"] // 2, g["c_row"])
            nb = N // 32
            self.out_scales = _place("e8m0", "friendly", device, B, 1, M * nb, M * nb, g["strideOutScales"])
            self.s_mask = torch.zeros(self.out_scales.full.numel(), dtype=torch.bool, device=device)
            self.out_scales.window(self.s_mask).fill_(True)
            self.c_mask = torch.zeros(self.c.full.numel(), dtype=torch.bool, device=device)
            self.c.window(self.c_mask).fill_(True)
        else:
            self.c = _place("bf16", "friendly", device, B, M, width, g["ldc"], g["strideC"], g["c_x"], g["c_row"])
            self.c_mask = torch.zeros(self.c.full.numel(), dtype=torch.bool, device=device)
            self.c.window(self.c_mask)[:, :, cols] = True
        assert int(self.c_mask.sum()) == B * M * (N // 2 if self.q4 else N)
        self.snapshot = {k: _ibits(o.full).clone() for k, o in ops.items()}

    # -- outputs
    def fresh_c(self):
        """A new C arena: the canary everywhere, the residual in C's window when it aliases C."""
        if self.q4:      # two outputs: the pair (e2m1 bytes, E8M0 bytes) stands where the other routes have one arena
            return (_canary(self.c.full.numel(), self.device, torch.uint8), _canary(self.out_scales.full.numel(), self.device, torch.uint8))
        c = _canary(self.c.full.numel(), self.device)
        if self.f["res"] == "alias":
            self.c.window(c)[:, :, self.cols] = self.data["R"].to(BF).to(self.device)
        return c

    def c_view(self, c_full):
        return (c_full[0] if self.q4 else c_full)[self.c.off:]

    def extract(self, c_full):
        """[B, M, N] bf16 out of a C arena, the column permutation undone; for the MXFP4 output [B, M, N / 2 + N / 32] bytes: the
        packed e2m1 row, then its E8M0 scales."""
        if self.q4:
            M, N = self.case.M, self.case.N
            return torch.cat([self.c.window(c_full[0]), self.out_scales.window(c_full[1]).reshape(-1, M, N // 32)], dim=-1)
        return self.c.window(c_full)[:, :, self.cols].clone()

    def residual(self):
        """The residual as the call reads it: (full, Op)."""
        if self.f["res"] == "alias":
            return self.fresh_c(), self.c
        return self.ops["R"].full, self.ops["R"]

    # -- the arguments, in alg_amd._lib's convention
    def gemm_call(self, c_full, B=None):
        """(positional, keyword) arguments of _lib.gemm (bf16 / e4m3 operands) or _lib.gemm_fp4.  B: a PackedB to pass instead of
        the row-major view."""
        c, g, f, ops, fp4 = self.case, self.g, self.f, self.ops, self.kind == "fp4"
        pos = (ops["A"].view, ops["B"].view if B is None else B, self.c_view(c_full), c.M, c.N, c.K, g["lda"], g["ldb"], g["ldc"])
        kw = dict(bias=ops["bias"].view, batch=c.batch, strideA=g["strideA"], strideB=g["strideB"], strideC=g["strideC"],
                  act=f["act"], flags=g["flags"])
        if f["perm"]:
            kw["perm_col0"] = g["perm_col0"]
        if f["res"]:
            kw.update(R=self.c_view(c_full) if f["res"] == "alias" else ops["R"].view, ldr=g["ldr"], strideR=g["strideR"])
        if f["gate"]:
            kw.update(gate=ops["gate"].view, strideGate=g["strideGate"], seg_split=g["seg_split"])
            if g["gseg"] is not None:
                kw["gate_seg_stride"] = g["gseg"]
        if self.kind != "bf16":
            kw.update(a_scale=ops["a_scale"].view, b_scale=ops["b_scale"].view, strideAScale=g["strideAScale"], strideBScale=g["strideBScale"])
        if self.q4:
            kw.update(q_out_scales=c_full[1][self.out_scales.off:], strideOutScales=g["strideOutScales"])
        return pos, kw

    def check_contract(self):
        """The alignment rules of gemm_check / gemm_fp4_check (csrc/gemm.hip, csrc/gemm_fp4.hip), on the real pointers."""
        g, f, N = self.g, self.f, self.case.N
        for name in ("A", "B"):
            assert self.ops[name].view.data_ptr() % 16 == 0, (name, case_id(self.case))
        if N % 4 == 0 and not self.q4:
            assert g["ldc"] % 4 == 0 and g["strideC"] % 4 == 0 and self.c.view.data_ptr() % 8 == 0
            if f["res"] == "own":
                assert g["ldr"] % 4 == 0 and g["strideR"] % 4 == 0 and self.ops["R"].view.data_ptr() % 8 == 0
            if f["gate"]:
                assert g["strideGate"] % 4 == 0 and (g["gseg"] or 0) % 4 == 0
                assert self.ops["gate"].view.data_ptr() % (16 if f["gate"] == "f32" else 8) == 0
            if f["bias"] == "col":
                assert self.ops["bias"].view.data_ptr() % 8 == 0
        if self.q4:
            assert g["ldc"] % 32 == 0 and g["strideC"] % 32 == 0 and self.c.view.data_ptr() % 16 == 0


def build(case, fill="friendly", device="cpu"):
    call = Call(case, fill, device)
    call.check_contract()
    return call


def pair_cases(case):
    """The two problems of a `pair` / `pair_qk` case: a plain GEMM with a column bias (for pair_qk the Q|K projection: 4 heads, N =
    2 * heads * 64 = 512, onto a contiguous C), and the V^T form -- a weight of 160 rows as A (33 at the smallest shape), shared by
    the batch, the activations as B, a per-row bias and the column permutation -- over N = 520 tokens (or the shape trigger's N).
    The trigger applies to the V^T problem, and to the first one where that problem has the operand and keeps its layout."""
    t = case.trigger
    first_trigger = t if t == "second_tile" or (case.route == "pair" and t not in PERM_TRIGGERS) else "none"
    first = Case("p10" if case.route == "pair" else "p9", "bias", first_trigger, case.M, case.N, case.K, case.batch)
    second = Case(first.route, "vt", t, min(case.M, 160), 520 if case.route == "pair_qk" else case.N, case.K, case.batch)
    return first, second


# ------------------------------------------------------------------------------------------------------------------ reference
def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64: integer arithmetic on the bit pattern (45 of the 52 mantissa
    bits go; a carry runs into the exponent as it should), the same on every device.  Normal bf16 range only."""
    bits = x.contiguous().view(torch.int64)
    bits = (bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)
    return bits.view(torch.float64)


def act64(x, act):
    if act == ACT_GELU:        # x / (1 + exp(-2u)): 0.5 x (1 + tanh u) cancels to 0 below x = -9 in float64
        u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)
        return x / (1.0 + torch.exp(-2.0 * u))
    if act == ACT_SILU:
        return x / (1.0 + torch.exp(-x))
    return x


def _exact32(t, what, case):
    assert bool((t.float().double() == t).all()), ("not exact in float32: " + what, case_id(case))
    return t


def _granule_log2(t):
    """The largest e <= 0 ... such that every element of t is a multiple of 2^e (t holds short dyadic numbers)."""
    for e in range(0, -40, -1):
        s = t * 2.0 ** -e
        if bool((s == s.round()).all()):
            return e
    raise AssertionError("not a short dyadic tensor")


def reference(call):
    """C = R + gate * act(A @ B^T + bias) in float64, from the header's contract: the operands are read with as_strided at the
    offsets and strides of the call; the rounding points are bf16 after the bias, bf16 after the activation, r + bf16(g * x) for a
    bf16 gate and one final rounding for ALG_GEMM_GATE_F32.  Asserts that every float32 intermediate of the call -- the K-term sum
    in any order, acc * a_scale * b_scale, + bias, gate * x, r + ... -- is exact.

    Returns y [B, M, N] float64: the value in front of the LAST rounding to bf16.  Without an activation y is exact in float32 and
    the call's result must be bf16(y) bit for bit; with one, y = act64(x) and the result is compared under the tolerance."""
    case, f, g, ops = call.case, call.f, call.g, call.ops
    M, N, K, B = case.M, case.N, case.K, case.batch
    if call.kind == "bf16":
        A, Bm = ops["A"].window().double(), ops["B"].window().double()
    elif call.kind == "fp8":
        A, Bm = ops["A"].window().clone().view(F8).float().double(), ops["B"].window().clone().view(F8).float().double()
    else:
        import _mxfp4
        kb = K // 32
        # (on the host: the emulation's ldexp is exact there)
        A = _mxfp4.dequantize(_mxfp4.unpack(ops["A"].window().cpu()), ops["a_scale"].window().reshape(-1, M, kb).cpu()).to(call.device)
        Bm = _mxfp4.dequantize(_mxfp4.unpack(ops["B"].window().cpu()), ops["b_scale"].window().reshape(-1, N, kb).cpu()).to(call.device)
    acc = A @ Bm.transpose(1, 2) + 0.0                                     # [Ba or Bb broadcast, M, N]
    _exact32(acc, "the K-term sum", case)
    # any order: every term is a multiple of q and the sum of the magnitudes stays below 2^24 q
    q = _granule_log2(A) + _granule_log2(Bm)
    mag = (A.abs() @ Bm.abs().transpose(1, 2)).max().item()
    assert mag <= 2.0 ** (24 + q), ("partial sums may round", case_id(case), mag, q)
    acc = acc.expand(B, M, N)
    if call.kind == "fp8":
        sa = ops["a_scale"].window().double().reshape(-1, M, 1)
        sb = ops["b_scale"].window().double().reshape(-1, 1, N)
        acc = _exact32(acc * _exact32(sa * sb, "a_scale * b_scale", case), "acc * a_scale * b_scale", case)
    bias = ops["bias"].window().double().reshape(-1)
    pre = _exact32(acc + (bias.reshape(1, M, 1) if f["bias"] == "row" else bias.reshape(1, 1, N)), "+ bias", case)
    x = bf16_rne(pre)
    if f["act"] != ACT_NONE:
        assert bool((x.abs() <= 6.0).all()) and bool((x * 8 == (x * 8).round()).all()), ("pre-activation off the 1/8 grid in [-6, 6]", case_id(case))
        return act64(x, f["act"])
    if not f["res"]:
        return pre
    r_full, r_op = call.residual()
    r = r_op.window(r_full)[:, :, call.cols].double() if f["res"] == "alias" else r_op.window().double()
    if f["gate"]:
        gv = ops["gate"].window().double()                                 # [B, 2, N] read at gate_seg_stride (0: one gate)
        rows = torch.arange(M, device=x.device).reshape(1, M, 1)
        gsel = torch.where(rows >= g["seg_split"], gv[:, 1:2, :], gv[:, 0:1, :])
        t = _exact32(gsel * x, "gate * x", case)
        if f["gate"] == "bf16":
            t = bf16_rne(t)
    else:
        t = x
    return _exact32(r + t, "r + ...", case)


def quantized(y_bf):
    """tests/_mxfp4.py's quantiser emulation on a bf16 result [B, M, N]: (packed e2m1 bytes [B, M, N / 2], E8M0 bytes [B, M, N / 32])."""
    import _mxfp4
    codes, scales = _mxfp4.quantize(y_bf.double().cpu())        # on the host: frexp / ldexp are exact there
    return _mxfp4.pack(codes).to(y_bf.device), scales.to(y_bf.device)


# ----------------------------------------------------------------------------------------------------------------- assertions
# One set for the emulation (tests/test_gemm_arena_cpu.py) and the kernels (tests/test_gpu_gemm_operands.py).
def assert_reference(call, c_full, y, report=None):
    """1 / 2: without an activation bit for bit bf16(y); with one |got - y| <= 2^-7 |y| + 2^-100, and among the elements with
    |y| >= 2^-100 at most 1 % may differ from bf16(y).  report: a list that receives (case id, fill, share)."""
    got = call.extract(c_full)
    want = bf16_rne(y).float().to(BF)
    if call.q4:      # y: the bf16 epilogue value the quantiser sees; the output is its quantisation, bit for bit
        want = torch.cat(quantized(want), dim=-1)
    if call.f["act"] == ACT_NONE or call.q4:
        same = _ibits(got) == _ibits(want)
        assert bool(same.all()), ("reference", case_id(call.case), call.fill, int((~same).sum()), (~same).nonzero()[:4].tolist())
        return
    err = (got.double() - y).abs()
    bound = 2.0 ** -7 * y.abs() + TINY
    assert bool((err <= bound).all()), ("reference", case_id(call.case), call.fill, int((err > bound).sum()), (err - bound).max().item())
    big = y.abs() >= TINY
    share = float(((_ibits(got) != _ibits(want)) & big).sum()) / max(int(big.sum()), 1)
    if report is not None:
        report.append((case_id(call.case), call.fill, share))
    assert share <= 0.01, ("reference share", case_id(call.case), call.fill, share)


def assert_footprint(call, c_full):
    """3a: every element of the C arena outside the mask still holds the canary."""
    if call.q4:
        for full, mask in zip(c_full, (call.c_mask, call.s_mask)):
            touched = (full != _canary(full.numel(), full.device, torch.uint8)) & ~mask
            assert not bool(touched.any()), ("footprint", case_id(call.case), call.fill, int(touched.sum()))
        return
    touched = (_ibits(c_full) != CANARY_BITS) & ~call.c_mask
    assert not bool(touched.any()), ("footprint", case_id(call.case), call.fill, int(touched.sum()), touched.nonzero()[:4].flatten().tolist(),
                                     call.c.off, call.g["ldc"])


def assert_inputs_unchanged(call):
    """3b: A, B, bias, gate, the scales and a residual of its own are what they were, bit for bit."""
    for name, op in call.ops.items():
        assert torch.equal(_ibits(op.full), call.snapshot[name]), ("inputs", name, case_id(call.case), call.fill)


def assert_fill_independent(call, c_hostile, c_friendly):
    """4: the hostile and the friendly outputs are equal bit for bit, and finite."""
    h, f = call.extract(c_hostile), call.extract(c_friendly)
    if not call.q4:
        assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(f.float()).all()), ("fill: not finite", case_id(call.case))
    same = _ibits(h) == _ibits(f)
    assert bool(same.all()), ("fill", case_id(call.case), int((~same).sum()), (~same).nonzero()[:4].tolist())


def assert_deterministic(call, c_first, c_second):
    """5: a second run gives the same bits, in the whole arena."""
    for a, b in zip(c_first, c_second) if call.q4 else ((c_first, c_second),):
        assert torch.equal(_ibits(a), _ibits(b)), ("determinism", case_id(call.case), call.fill)


def failures(call_f, c_f, call_h, c_h, y, c_f2=None, report=None):
    """The assertions on one call run under both fills: {name: message} of those that fail -- empty for a correct kernel."""
    checks = [("reference", lambda: (assert_reference(call_f, c_f, y, report), assert_reference(call_h, c_h, y, report))),
              ("footprint", lambda: (assert_footprint(call_f, c_f), assert_footprint(call_h, c_h))),
              ("inputs", lambda: (assert_inputs_unchanged(call_f), assert_inputs_unchanged(call_h))),
              ("fill", lambda: assert_fill_independent(call_h, c_h, c_f))]
    if c_f2 is not None:
        checks.append(("determinism", lambda: assert_deterministic(call_f, c_f, c_f2)))
    failed = {}
    for name, check in checks:
        try:
            check()
        except AssertionError as e:
            failed[name] = str(e)
    return failed
