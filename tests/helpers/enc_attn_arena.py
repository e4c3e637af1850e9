"""Test helper: the operands of the encoder attention entry (alg_attn_bias; include/alg_hip.h "T5Attention / CLIPAttention",
csrc/t5.hip) inside flat ARENAS that belong to the test, exact data for them, and the float64 statement of the header's contract.

Layouts, both through the raw C ABI (three pointers, two pitches):

  compact  what the `_lib.attn_bias` wrapper passes: q | k | v side by side in a [B * L][3 inner] buffer, out [B * L][inner].
  loose    q, k and v column windows of one wider buffer: q at column 8, 16 columns between q and k, 24 between k and v, 40 behind
           v (every window starts at a non-zero multiple of 8 elements, qkv_rstride = 3 inner + 88); out a column window at
           column 6 of a buffer of pitch inner + 20.

Both layouts put GUARD rows of the operand's pitch in front of and behind the rows [0, B * L): what a kernel reads or writes a
workgroup past its last row lands inside the arena's own allocation.

Fills: `friendly` puts zeros outside the live elements, `hostile` bf16 NaN (0x7FC0) into the guard rows and the gap columns.
Live but masked K and V rows are live elements and stay finite: the contract multiplies them by p = 0.  Both fills pre-fill the
out arena with the canary 0x7FC1.

Data.  Both families keep q . k exact: family A's dot products have ONE non-zero term, a power of two (256 at scale 1; 1024 where
the call scales by 0.125 or 80^-0.5, so that the scaled hit stays 112 above a miss -- no |q . k| <= 256 can do that at these
scales), family B's are integers of magnitude <= 24.  Such values are exact in float32 in any accumulation order and exact in
bf16; the bias values are multiples of 1/4; so `s` has the same bits in the kernel and in the reference.

  A "selector"  q holds one code on one column of a row, k one code on one column of a key: q . k is HIT where the columns agree,
     else 0.  The bias table holds 0 in four buckets of a head (other buckets per head) and -256 in the rest.  Every score of a
     row is then the row's top level or at least 112 below it (asserted on every row of every case): float32 exp(-112) is 0
     with or without denormals (half the smallest denormal is e^-104), so p is exactly bf16(1 / n) on the n top-level keys that
     survive and 0 elsewhere.  v holds integers in [-8, 8] that vary with b, j, h and d: p times any partial sum of v has at most
     8 + 13 bits, exact in float32 in any order, and the output is bf16(bf16(1 / n) * sum v): BIT FOR BIT the reference.
     A masked key keeps its k code (it would hit every row that reads its column) and carries v = 2^100: any leaked probability
     changes the bits.  A causally excluded key is live for the rows below it, so its v is an ordinary one; a leak changes n and
     the sum.  Rows with (i + b + h) % 5 == 1 put their code on a column no key uses: all scores 0 (without a bias), every
     surviving key at the top, and a phantom key of [L, Lp) -- zero k, zero score -- would join them and change n.
     bf16(1 / n) must not depend on how the device divides: n_is_safe() holds for every row (tests/test_enc_attn_arena_cpu.py).
  B "graded"    q integers in [-2, 2] on three columns (one of them >= 64 at head_dim 80; in [-1, 1] where the scale is 1, which
     keeps the spread of the scores near that of the scaled modes), k integers in [-2, 2] everywhere, a bias of multiples of 1/4
     in [-4, 4] that differs across buckets and across heads, v from N(0, 1).  The softmax is not one-hot (median over the rows
     with a key of max_j p_j <= 0.5), so every key's p, the mask, the bucket and the diagonal show in the output.
     Bound per element against the float64 value ref = sum_j p_j v_j, p_j = bf16(softmax(s)_j), with A = sum_j p_j |v_j|:

         |got - ref| <= (2^-9 + 2^-13) * (A + |ref|)

     The kernel sees the same s.  2^-13: its float32 exp(s - m) (1 ulp), row sum (8 adds and a 6-step reduction), reciprocal and
     product move a quotient e_j / sum by about 10 float32 ulp, far below a bf16 step, and 512 float32 fmas add at most
     512 * 2^-24 A = 2^-15 A to the p v sum.  2^-9: rounding that sum to bf16 costs half a bf16 step of the result, between
     2^-9 |ref| and 2^-8 |ref| by its place in the binade, and 2^-9 (A + |ref|) >= 2^-8 |ref| since A >= |ref|; the kernel's
     p_j ARE the reference's rounded p_j, except where a quotient lies within float32's reach (F32_REACH, 32 ulp) of a bf16
     rounding midpoint: there the kernel's p_j may land on the other side, a whole step of p_j times |v_j|.  One heavy key doing
     so in a row where |ref| is close to A would break the bound under a correct kernel, so this is a CONDITION on the data,
     from the reference alone: room() adds up, per element, every flip float32 allows, 2^-13 A and the half step, and must not
     exceed the bound anywhere.  A case takes the first draw of its random data on which that holds (B_DRAW);
     tests/test_enc_attn_arena_cpu.py asserts it for every element of every case.

Pure torch; arenas are built on the CPU and moved to `device`."""
import collections
import math

import torch

BF = torch.bfloat16
LAYOUTS = ("compact", "loose")
FILLS = ("friendly", "hostile")
NAN_BITS = 0x7FC0
CANARY_BITS = 0x7FC1
GUARD = 32            # rows of every guard band: one workgroup's rows
B, H = 2, 3           # blockIdx.y = b * H + h: a div / mod that shows
NB = 32               # buckets of the bias table
L_LIST = (1, 33, 63, 64, 65, 77, 226, 257, 448, 512)
LIMIT = {64: 512, 80: 448}
BIG_V = 2.0 ** 100
GAP = 112.0           # float32 exp(-112) == 0
BOUND = 2.0 ** -9 + 2.0 ** -13
F32_REACH = 2.0 ** -19   # relative: 32 float32 ulp, above what exp, the row sum, the reciprocal and the product add up to

MODES = {
    "t5":                dict(d=64, bias=True, mask=True, causal=False, scale=1.0),
    "t5_nomask":         dict(d=64, bias=True, mask=False, causal=False, scale=1.0),
    "clip_text":         dict(d=64, bias=False, mask=False, causal=True, scale=0.125),
    "clip_vision":       dict(d=80, bias=False, mask=False, causal=False, scale=80.0 ** -0.5),
    # what the product never issues and the contract allows
    "x_causal_mask":     dict(d=64, bias=False, mask=True, causal=True, scale=0.125),
    "x_causal_bias":     dict(d=64, bias=True, mask=False, causal=True, scale=0.125),
    "x_d80_mask_causal": dict(d=80, bias=False, mask=True, causal=True, scale=80.0 ** -0.5),
}
PRODUCT_MODES = ("t5", "t5_nomask", "clip_text", "clip_vision")
CROSS_MODES = ("x_causal_mask", "x_causal_bias", "x_d80_mask_causal")
MASK_KINDS = ("tails", "holes", "item", "key0")
# the columns of a head that family A's codes use (neighbours 2t, 2t + 1 of a packed pair; both halves at head_dim 80), the
# column no key uses, and the columns of family B's q
A_COLS = {64: (0, 1, 6, 7, 30, 31, 62, 63), 80: (0, 1, 38, 39, 64, 65, 78, 79)}
A_DEAD = {64: 17, 80: 70}
B_COLS = {64: (1, 6, 40), 80: (1, 40, 70)}
# family B: which draw of the random data a case takes (0 where not listed): found by counting up from 0 until room() <= 1 holds
# on every element and the median of max_j p_j is at most 0.5; the CPU test asserts both for the draw that is used
B_DRAW = {"t5-L33-B": 5, "t5-L64-B": 1, "t5-L65-B": 3, "t5-L226-B": 17, "t5-L257-B": 5, "t5-L448-B": 10, "t5-L512-B": 5,
          "t5_nomask-L63-B": 3, "t5_nomask-L77-B": 2, "t5_nomask-L226-B": 12, "t5_nomask-L257-B": 11, "t5_nomask-L448-B": 1,
          "t5_nomask-L512-B": 45, "clip_text-L77-B": 2, "clip_text-L226-B": 1, "x_causal_mask-L65-B": 2, "x_causal_bias-L65-B": 2}

Case = collections.namedtuple("Case", "mode L family")


def case_id(c):
    return "%s-L%d-%s" % (c.mode, c.L, c.family)


def classes_of(L, d):
    """The boundary classes a length meets."""
    out = set()
    if L in (63, 64, 65):
        out.add("chunk_edge")           # the key-chunk count goes from 1 to 2
    if L > 32 and L % 32:
        out.add("workgroup_tail")       # a last workgroup with fewer than 32 rows
    if L % 4:
        out.add("mod4")                 # the waves of the last round do not all own a row
    if L == LIMIT[d]:
        out.add("limit")
    return out


def table():
    """Every product mode at every length its head_dim takes, the cross combinations at L = 65; family B leaves out L = 1, where
    a softmax over one key is one-hot by definition."""
    cases = []
    for mode in PRODUCT_MODES:
        for L in L_LIST:
            if L <= LIMIT[MODES[mode]["d"]]:
                cases.append(Case(mode, L, "A"))
                if L > 1:
                    cases.append(Case(mode, L, "B"))
    for mode in CROSS_MODES:
        cases += [Case(mode, 65, "A"), Case(mode, 65, "B")]
    return cases


def layouts_of(case):
    """`loose` everywhere; `compact` too at the lengths where the wrapper's layout meets an edge."""
    return LAYOUTS if case.L in (1, 65, 226, LIMIT[MODES[case.mode]["d"]]) else ("loose",)


def mask_kind(case):
    m = MODES[case.mode]
    if not m["mask"]:
        return None
    if m["causal"]:
        return "key0"
    return ("tails", "holes", "item")[L_LIST.index(case.L) % 3]


def make_mask(kind, L):
    """int32 [B, L].  tails: another length per item; holes: zeros in the middle of both items, other places per item;
    item: batch item 1 fully masked, item 0 a tail; key0: key 0 of item 0 masked (row 0 has no key under `causal`) with holes,
    item 1 a tail."""
    m = torch.ones(B, L, dtype=torch.int32)
    j = torch.arange(L)
    if kind == "tails":
        m[0, L - L // 3:] = 0
        m[1, L - L // 5 - 1:] = 0
    elif kind == "holes":
        m[0, (j % 5 == 2) & (j > 0) & (j < L - 1)] = 0
        m[1, (j % 7 >= 4) & (j > 1) & (j < L - 2)] = 0
    elif kind == "item":
        m[0, L - L // 4:] = 0
        m[1, :] = 0
    elif kind == "key0":
        m[0, 0] = 0
        m[0, (j % 6 == 3) & (j < L - 1)] = 0
        m[1, L - L // 3:] = 0
    else:
        raise ValueError(kind)
    return m


class Data:
    """The live elements of a case: q / k / v [B, L, H, d] bf16, table [NB, H] bf16 or None, lut int32 [2 L - 1] or None,
    mask int32 [B, L] or None, scale, causal."""

    def __init__(self, case, q, k, v, table, lut, mask):
        m = MODES[case.mode]
        self.case, self.d, self.L, self.scale, self.causal = case, m["d"], case.L, m["scale"], m["causal"]
        self.q, self.k, self.v, self.table, self.lut, self.mask = q, k, v, table, lut, mask


def make_data(case):
    m, L = MODES[case.mode], case.L
    d = m["d"]
    g = torch.Generator().manual_seed(1000 * L + sorted(MODES).index(case.mode) + 100000 * B_DRAW.get(case_id(case), 0))
    kind = mask_kind(case)
    mask = make_mask(kind, L) if kind else None
    lut = torch.randint(0, NB, (2 * L - 1,), generator=g, dtype=torch.int32) if m["bias"] else None
    bi, ji, hi, di = torch.meshgrid(torch.arange(B), torch.arange(L), torch.arange(H), torch.arange(d), indexing="ij")
    bk, hk = torch.arange(NB).reshape(NB, 1), torch.arange(H).reshape(1, H)
    if case.family == "A":
        code = 16.0 if m["scale"] == 1.0 else 32.0
        cols = torch.tensor(A_COLS[d])
        b3, j3, h3 = bi[..., 0], ji[..., 0], hi[..., 0]
        kcol = cols[(j3 * 3 + h3 * 5 + b3 * 2 + j3 // 8) % 8]
        qcol = cols[(j3 * 5 + h3 + b3 * 3 + j3 // 8) % 8]
        qcol = torch.where((j3 + b3 + h3) % 5 == 1, torch.tensor(A_DEAD[d]), qcol)
        q = torch.zeros(B, L, H, d).scatter_(3, qcol.unsqueeze(-1), code)
        k = torch.zeros(B, L, H, d).scatter_(3, kcol.unsqueeze(-1), code)
        v = ((ji * 7 + di * 3 + hi * 5 + bi * 11 + ji // 16) % 17 - 8).float()
        if mask is not None:
            v = torch.where(mask.reshape(B, L, 1, 1) == 0, torch.tensor(BIG_V), v)
        table = torch.where((bk + 3 * hk) % 8 == 0, 0.0, -256.0) if m["bias"] else None
    else:
        q = torch.zeros(B, L, H, d)
        top = 1 if m["scale"] == 1.0 else 2
        for c in B_COLS[d]:
            q[..., c] = torch.randint(-top, top + 1, (B, L, H), generator=g).float()
        k = torch.randint(-2, 3, (B, L, H, d), generator=g).float()
        v = torch.randn(B, L, H, d, generator=g)
        table = (((bk * 7 + hk * 11) % 33) - 16).float() / 4.0 if m["bias"] else None
    return Data(case, q.to(BF), k.to(BF), v.to(BF), None if table is None else table.to(BF), lut, mask)


# ------------------------------------------------------------------------------------------------------------------ reference
def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64, by integer arithmetic on the bit pattern; magnitudes below
    the smallest normal bf16 go to zero (nothing a case computes lies between: family A's non-top probabilities are e^-112 of
    a top one and are zero in float32 already)."""
    bits = x.contiguous().view(torch.int64)
    bits = (bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)
    r = bits.view(torch.float64)
    return torch.where(x.abs() < 2.0 ** -126, torch.zeros_like(r), r)


Ref = collections.namedtuple("Ref", "out exact A n nokey top_gap pmax flip")


def reference(data, flips=True):
    """include/alg_hip.h "T5Attention / CLIPAttention" op for op in float64, on the live elements.  Returns, as [B, L, H, d]
    float64: out = bf16(sum_j p_j v_j), exact = that sum unrounded, A = sum_j p_j |v_j|; per row [B, H, L]: n = the number of
    surviving keys at the row's top score, top_gap = the distance from the top score to the next one below it (inf if none),
    pmax = max_j p_j; nokey = rows without a surviving key (out is 0 there); flip [B, L, H, d] (with `flips`): see room()."""
    L = data.L
    q, k, v = (t.double().permute(0, 2, 1, 3) for t in (data.q, data.k, data.v))          # [B, H, L, d]
    s = bf16_rne(q @ k.transpose(-1, -2))                                                   # s = bf16(q . k)
    if data.scale != 1.0:
        s = (s.float() * torch.tensor(data.scale, dtype=torch.float32)).to(BF).double()     # bf16(float32(s) * float32(scale))
    i, j = torch.arange(L).reshape(L, 1), torch.arange(L).reshape(1, L)
    if data.table is not None:
        bias = data.table.double()[data.lut.long()[j - i + L - 1]]                          # [L, L, H]
        s = bf16_rne(s + bias.permute(2, 0, 1).unsqueeze(0))
    keep = torch.ones(B, H, L, L, dtype=torch.bool)
    if data.mask is not None:
        keep &= (data.mask != 0).reshape(B, 1, 1, L)
    if data.causal:
        keep &= (j <= i).reshape(1, 1, L, L)
    nokey = ~keep.any(dim=-1)
    s = torch.where(keep, s, torch.tensor(-math.inf, dtype=torch.float64))
    top = s.max(dim=-1, keepdim=True).values
    top = torch.where(nokey.unsqueeze(-1), torch.zeros_like(top), top)
    e = torch.where(keep, torch.exp(s - top), torch.zeros_like(s))
    den = e.sum(dim=-1, keepdim=True)
    x = e / torch.where(den > 0, den, torch.ones_like(den))
    p = bf16_rne(x)                                                                         # p = bf16(softmax(s))
    exact = (p @ v).permute(0, 2, 1, 3)
    A = (p @ v.abs()).permute(0, 2, 1, 3)
    at_top = keep & (s == top)
    below = torch.where(keep & ~at_top, top - s, torch.tensor(math.inf, dtype=torch.float64))
    rows = (at_top.sum(dim=-1), nokey, below.min(dim=-1).values, p.max(dim=-1).values)
    if not flips:
        return Ref(bf16_rne(exact), exact, A, *rows, None)
    # the keys whose quotient lies within float32's reach of a bf16 rounding midpoint, and what their landing on the other side
    # would move: one step of p_j times |v_j|
    binade = torch.exp2(torch.floor(torch.log2(p.clamp_min(2.0 ** -200))))
    step = torch.where(p > 0, binade / 128, torch.zeros_like(p))
    down = torch.where(p == binade, step / 4, step / 2)          # below a power of two the steps are half as wide
    near = torch.minimum((x - (p + step / 2)).abs(), (x - (p - down)).abs()) <= F32_REACH * x
    flip = (torch.where(near & (p > 0), step, torch.zeros_like(step)) @ v.abs()).permute(0, 2, 1, 3)
    return Ref(bf16_rne(exact), exact, A, *rows, flip)


def room(ref):
    """Family B's condition on the data, per element: what a correct float32 kernel can be off by -- the p flips float32 allows,
    2^-13 A for its arithmetic, half a bf16 step of the result -- over the bound.  At most 1 everywhere: the bound is then a
    statement about every correct kernel, not about one."""
    drift = ref.flip + 2.0 ** -13 * ref.A
    half = torch.exp2(torch.floor(torch.log2((ref.exact.abs() + drift).clamp_min(2.0 ** -200))) - 8)
    bound = BOUND * (ref.A + ref.exact.abs())
    return torch.where(ref.A > 0, (drift + half) / bound.clamp_min(2.0 ** -200), torch.zeros_like(bound))


def n_is_safe(n):
    """bf16(1 / n) is the same for the float32 quotient and for that quotient moved by up to 2 ulp either way."""
    q = torch.tensor(1.0, dtype=torch.float32) / torch.as_tensor(n, dtype=torch.float32)
    lo = hi = q
    for _ in range(2):
        lo = torch.nextafter(lo, torch.zeros_like(q))
        hi = torch.nextafter(hi, torch.full_like(q, 2.0))
    return (lo.to(BF) == q.to(BF)) & (hi.to(BF) == q.to(BF))


# ------------------------------------------------------------------------------------------------------------------ arenas
def _bits(value, n):
    return torch.full((n,), value, dtype=torch.int16).view(BF)


class Call:
    """One call's arguments.  qkv / out: the flat arenas; q_off / k_off / v_off / out_off: the first element of each operand;
    qkv_rs / out_rs: the pitches; table / lut / mask: flat device tensors or None; o_mask: True where the call may write."""

    def __init__(self, data, layout, fill, device):
        d, L = data.d, data.L
        inner, rows = H * d, B * L
        self.data, self.layout, self.fill, self.device = data, layout, fill, device
        self.d, self.L, self.inner = d, L, inner
        if layout == "compact":
            self.qkv_rs, cols, self.out_rs, out_x = 3 * inner, (0, inner, 2 * inner), inner, 0
        else:
            self.qkv_rs, cols, self.out_rs, out_x = 3 * inner + 88, (8, inner + 24, 2 * inner + 48), inner + 20, 6
        total = GUARD + rows + GUARD
        qkv = _bits(NAN_BITS, total * self.qkv_rs) if fill == "hostile" else torch.zeros(total * self.qkv_rs, dtype=BF)
        self.q_off, self.k_off, self.v_off = (GUARD * self.qkv_rs + c for c in cols)
        for off, t in ((self.q_off, data.q), (self.k_off, data.k), (self.v_off, data.v)):
            torch.as_strided(qkv, (rows, inner), (self.qkv_rs, 1), off).copy_(t.reshape(rows, inner))
        self.out_off = GUARD * self.out_rs + out_x
        self.out_numel = total * self.out_rs
        o_mask = torch.zeros(self.out_numel, dtype=torch.bool)
        torch.as_strided(o_mask, (rows, inner), (self.out_rs, 1), self.out_off).fill_(True)
        mv = lambda t: None if t is None else t.reshape(-1).contiguous().to(device)
        self.qkv, self.o_mask = qkv.to(device), o_mask.to(device)
        self.table, self.lut, self.mask = mv(data.table), mv(data.lut), mv(data.mask)
        self._before = [None if t is None else t.clone() for t in (self.qkv, self.table, self.lut, self.mask)]
        # what the entry demands (csrc/t5.hip): the pitch a multiple of 8 elements, k and v on 16 bytes
        assert self.qkv_rs % 8 == 0 and self.k_off % 8 == 0 and self.v_off % 8 == 0 and self.qkv.data_ptr() % 16 == 0

    def fresh_out(self):
        return _bits(CANARY_BITS, self.out_numel).to(self.device)

    def extract(self, out_full):
        """[B, L, H, d] out of an out arena."""
        return torch.as_strided(out_full, (B * self.L, self.inner), (self.out_rs, 1), self.out_off).reshape(B, self.L, H, self.d).clone()

    def inputs(self):
        return list(zip(("qkv", "table", "lut", "mask"), (self.qkv, self.table, self.lut, self.mask), self._before))


def build(data, layout="compact", fill="friendly", device="cpu"):
    assert layout in LAYOUTS and fill in FILLS
    return Call(data, layout, fill, device)


# ------------------------------------------------------------------------------------------------------------------ assertions
# One set for the emulation (tests/test_enc_attn_arena_cpu.py) and the kernel (tests/test_gpu_enc_attn_operands.py).
def _i16(t):
    return t.view(torch.int16)


def assert_value(call, out_full, ref, report=None):
    """Family A: bit for bit the reference; a row without a key holds zeros of either sign.  Family B: the derived bound; the
    share of elements that differ from bf16(ref) goes to `report` and is not asserted on."""
    got = call.extract(out_full).cpu()
    nokey = ref.nokey.permute(0, 2, 1).unsqueeze(-1).expand_as(got)                       # [B, L, H, d]
    zeros = (_i16(got) & 0x7FFF) == 0
    assert bool(zeros[nokey].all()), ("rows without a key", case_id(call.data.case), call.layout, call.fill, int((~zeros[nokey]).sum()))
    want = ref.out.to(BF)
    same = (_i16(got) == _i16(want)) | (nokey & zeros)
    if call.data.case.family == "A":
        assert bool(same.all()), ("value", case_id(call.data.case), call.layout, call.fill, int((~same).sum()), (~same).nonzero()[:4].tolist())
        return
    assert bool(torch.isfinite(got.float()).all()), ("value: not finite", case_id(call.data.case), call.layout, call.fill)
    err, bound = (got.double() - ref.exact).abs(), BOUND * (ref.A + ref.exact.abs())
    if report is not None:
        report.append((case_id(call.data.case), call.layout, call.fill, 1.0 - same.float().mean().item(), (err / bound.clamp_min(1e-300)).max().item()))
    bad = err > bound
    assert not bool(bad.any()), ("value", case_id(call.data.case), call.layout, call.fill, int(bad.sum()), (err / bound.clamp_min(1e-300)).max().item())


def assert_footprint(call, out_full):
    """Every element of the out arena outside rows < B * L, columns [0, inner) of the window still holds the canary."""
    touched = _i16(out_full)[~call.o_mask] != CANARY_BITS
    assert not bool(touched.any()), ("footprint", case_id(call.data.case), call.layout, call.fill, int(touched.sum()))


def assert_inputs_unchanged(call):
    for name, now, before in call.inputs():
        if now is not None:
            same = _i16(now) == _i16(before) if now.dtype == BF else now == before
            assert bool(same.all()), ("input changed", name, case_id(call.data.case), call.layout, call.fill)


def assert_fill_independent(call, out_hostile, out_friendly):
    h, f = call.extract(out_hostile), call.extract(out_friendly)
    assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(f.float()).all()), ("fill: not finite", case_id(call.data.case), call.layout)
    same = _i16(h) == _i16(f)
    assert bool(same.all()), ("fill", case_id(call.data.case), call.layout, int((~same).sum()))


def assert_deterministic(call, out_first, out_second):
    same = _i16(out_first) == _i16(out_second)
    assert bool(same.all()), ("determinism", case_id(call.data.case), call.layout, int((~same).sum()))


def failures(call_f, out_f, call_h, out_h, ref, out_f2=None, report=None):
    """The assertions on one call run under both fills: {name: message} of those that fail -- empty for a correct kernel."""
    checks = [("value", lambda: (assert_value(call_f, out_f, ref, report), assert_value(call_h, out_h, ref, report))),
              ("footprint", lambda: (assert_footprint(call_f, out_f), assert_footprint(call_h, out_h),
                                     assert_inputs_unchanged(call_f), assert_inputs_unchanged(call_h))),
              ("fill", lambda: assert_fill_independent(call_h, out_h, out_f))]
    if out_f2 is not None:
        checks.append(("determinism", lambda: assert_deterministic(call_f, out_f, out_f2)))
    failed = {}
    for name, check in checks:
        try:
            check()
        except AssertionError as e:
            failed[name] = str(e)
    return failed
