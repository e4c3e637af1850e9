"""Test helper: operands of the dense attention entries (alg_flash_attn_d64[_ex], alg_flash_attn_d128[_ex], alg_flash_attn_d128_dual;
include/alg_hip.h) laid out inside flat bf16 ARENAS that belong to the test, with guard bands in front of and behind every operand.

An operand is handed to the `_lib` wrappers as a flat view that begins at its first element (the wrappers take `data_ptr()`), with
the strides the layout gives it.  Three layouts, all inside the documented contract (q / k / vt rows 16-byte aligned, o 8-byte
aligned, a V^T pitch of at least Skv rounded up to 64):

  compact  what the kernel tests have always passed: d = 64 reads Q and K out of one [B][S][2 D] buffer and pads V^T to a multiple
           of 128, d = 128 passes [B][S][D] tensors and pads V^T to a multiple of 64; o is [B][Sq][D].
  packed   the product's layout: Q and K in one [B][rows][2 D + 64] buffer (Q at column 0, K at column D; with kv_group > 1
           LLaVA's [L][D + KV]), rows = max(Sq, Skv) + 256, so that the K rows Skv.. exist and belong to the fill; a V^T pitch of
           EXACTLY ceil(Skv / 64) * 64; o a column window of a [B][Sq + 256][D + 200] buffer whose first column is = 4 (mod 8):
           8-byte but not 16-byte aligned (HunyuanVideo writes o into its [J][D + Mff] buffer); batch strides with a gap.
  loose    every stride larger than needed, q_rs != k_rs where the entry has both (the d = 64 entries share them), vt_rs =
           ceil(Skv / 64) * 64 + 72, every operand's first element a non-zero multiple of 8 elements (o: of 4) into its
           row, and o_rs = 4 (mod 8): every other o row is not 16-byte aligned.

Guards: 256 rows of the operand's pitch in front of and behind Q / K / o, 256 V^T rows plus 256 columns around V^T.  What a
prefetch a few tiles past its panel could read or write lands inside the arena's own allocation; nothing here reaches, or relies on,
memory outside an allocation.

Fills: `friendly` puts zeros everywhere outside the live elements, the V^T padding columns [Skv, ceil(Skv / 64) * 64) included.
`hostile` puts bf16 NaN (0x7FC0) everywhere outside the live elements of q / k / vt -- K rows >= Skv, Q rows >= Sq, the columns
between and behind the heads' windows, everything past ceil(Skv / 64) * 64 in a V^T row -- and finite random values in [-4, 4] into
the V^T padding columns: exactly what the header allows ("multiplied by p = 0").  Both fills pre-fill the o arena with the canary
bit pattern 0x7FC1.

Pure torch, runs on either device."""
import math

import torch

BF = torch.bfloat16
LAYOUTS = ("compact", "packed", "loose")
FILLS = ("friendly", "hostile")
NAN_BITS = 0x7FC0
CANARY_BITS = 0x7FC1
GUARD = 256          # rows (and V^T columns) of every guard band: four 64-key tiles


def swap23(n):
    """perm of include/alg_hip.h: logical key s sits at column perm(s) of a V^T row (index bits 2 and 3 swapped)."""
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


def perm_index(n, device="cpu"):
    return torch.tensor([swap23(i) for i in range(n)], dtype=torch.long, device=device)


def ceil64(n):
    return (n + 63) // 64 * 64


def _bits(value, n, device):
    """n bf16 elements holding the 16-bit pattern `value`."""
    return torch.full((n,), value, dtype=torch.int16, device=device).view(BF)


class Rows:
    """A [B][S][heads * d] operand (q, k or o) inside `full`: element (b, s, h, dd) at off + b * bs + s * rs + h * d + dd."""

    def __init__(self, full, off, bs, rs, B, S, width):
        self.full, self.off, self.bs, self.rs, self.B, self.S, self.width = full, off, bs, rs, B, S, width

    @property
    def view(self):
        return self.full[self.off:]

    def window(self, full=None):
        return torch.as_strided(self.full if full is None else full, (self.B, self.S, self.width), (self.bs, self.rs, 1), self.off)


class Vt:
    """V^T [B][rows][pitch] inside `full`: element (b, r, column) at off + b * bs + r * rs + column; `pad` = ceil(Skv / 64) * 64
    columns of a row belong to the operand."""

    def __init__(self, full, off, bs, rs, B, rows, Skv):
        self.full, self.off, self.bs, self.rs, self.B, self.rows, self.Skv = full, off, bs, rs, B, rows, Skv
        self.pad = ceil64(Skv)

    @property
    def view(self):
        return self.full[self.off:]

    def window(self):
        return torch.as_strided(self.full, (self.B, self.rows, self.pad), (self.bs, self.rs, 1), self.off)


class Arena:
    """What build() returns.  q / k / vt / o: Rows / Vt records (`.view` is what a wrapper takes, `.full` the whole arena, `.off`
    the first element's index in it); q_c / k_c / v_c: the compact copies [B, S, heads, d]; o_mask: bool over o.full, True where
    the call may write (exactly B * Sq * H * d elements)."""

    def __init__(self, d, B, H, Sq, Skv, kv_group, layout, fill, q, k, vt, o, q_c, k_c, v_c):
        self.d, self.B, self.H, self.Sq, self.Skv, self.kv_group, self.layout, self.fill = d, B, H, Sq, Skv, kv_group, layout, fill
        self.q, self.k, self.vt, self.o = q, k, vt, o
        self.q_c, self.k_c, self.v_c = q_c, k_c, v_c
        self.o_mask = torch.zeros(o.full.numel(), dtype=torch.bool, device=o.full.device)
        o.window(self.o_mask).fill_(True)

    def fresh_o(self):
        """A new o arena holding the canary everywhere (the views of one Arena may be used by several calls)."""
        return _bits(CANARY_BITS, self.o.full.numel(), self.o.full.device)

    def o_view(self, o_full):
        return o_full[self.o.off:]

    def extract(self, o_full):
        """[B, Sq, H, d] out of an o arena."""
        return self.o.window(o_full).reshape(self.B, self.Sq, self.H, self.d).clone()

    def check_contract(self):
        """What attn64_check / attn128_check demand of the operands (csrc/attention.hip, csrc/attention128_host.h); the base
        addresses are checked on the real pointers."""
        for r in (self.q, self.k, self.vt):
            assert r.rs % 8 == 0 and r.bs % 8 == 0 and r.view.data_ptr() % 16 == 0, (self.layout, r.rs, r.bs, r.off)
        assert self.o.rs % 4 == 0 and self.o.bs % 4 == 0 and self.o.view.data_ptr() % 8 == 0, (self.layout, self.o.rs, self.o.bs)
        assert self.vt.rs >= ceil64(self.Skv)
        if self.d == 64:    # one pair of strides serves q and k
            assert (self.q.bs, self.q.rs) == (self.k.bs, self.k.rs)


def _new(n, fill, device):
    return _bits(NAN_BITS, n, device) if fill == "hostile" else torch.zeros(n, dtype=BF, device=device)


def build(d, B, H, Sq, Skv, kv_group=1, layout="compact", fill="friendly", device="cpu", q=None, k=None, v=None, seed=0):
    """Arenas for one call.  q [B, Sq, H, d], k / v [B, Skv, H / kv_group, d] bf16: the compact copies (drawn from N(0, 1) with
    `seed` when not given; the same seed gives the same values under every layout and fill)."""
    assert d in (64, 128) and layout in LAYOUTS and fill in FILLS and H % kv_group == 0
    assert d == 128 or (Sq == Skv and kv_group == 1)
    Hk = H // kv_group
    D, KV = H * d, Hk * d
    g = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randn(*shape, generator=g).to(BF)
    q = draw(B, Sq, H, d) if q is None else q
    k = draw(B, Skv, Hk, d) if k is None else k
    v = draw(B, Skv, Hk, d) if v is None else v
    q, k, v = q.to(device), k.to(device), v.to(device)
    assert q.shape == (B, Sq, H, d) and k.shape == (B, Skv, Hk, d) and v.shape == k.shape
    pad = ceil64(Skv)

    # ---- Q and K
    shared = layout == "packed" or (layout == "compact" and d == 64)       # one buffer: Q at column 0, K at column D
    if shared:
        if layout == "compact":
            pitch, rows, gap = 2 * D, Sq, 0
        else:
            pitch, rows, gap = (D + KV if kv_group > 1 else 2 * D + 64), max(Sq, Skv) + GUARD, 296
        bs = rows * pitch + gap
        off = GUARD * pitch
        qk_full = _new(off + B * bs + GUARD * pitch, fill, device)
        qr = Rows(qk_full, off, bs, pitch, B, Sq, D)
        kr = Rows(qk_full, off + D, bs, pitch, B, Skv, KV)
    else:
        if layout == "compact":
            q_pitch, k_pitch, q_rows, k_rows, gap, q_x, k_x = D, KV, Sq, Skv, 0, 0, 0
        elif d == 64:      # loose, one pair of strides: two buffers of the same geometry
            q_pitch = k_pitch = D + 72
            q_rows = k_rows = Sq + 3
            gap, q_x, k_x = 136, 24, 40
        else:
            q_pitch, k_pitch, q_rows, k_rows, gap, q_x, k_x = D + 72, KV + 136, Sq + 3, Skv + 5, 136, 24, 40
        q_bs, k_bs = q_rows * q_pitch + gap, k_rows * k_pitch + gap
        q_off, k_off = GUARD * q_pitch + q_x, GUARD * k_pitch + k_x
        qr = Rows(_new(q_off + B * q_bs + GUARD * q_pitch, fill, device), q_off, q_bs, q_pitch, B, Sq, D)
        kr = Rows(_new(k_off + B * k_bs + GUARD * k_pitch, fill, device), k_off, k_bs, k_pitch, B, Skv, KV)
    qr.window().copy_(q.reshape(B, Sq, D))
    kr.window().copy_(k.reshape(B, Skv, KV))

    # ---- V^T
    if layout == "compact":
        vt_rs = (Skv + 127) // 128 * 128 if d == 64 else pad
        vt_gap, vt_x = 0, 0
    elif layout == "packed":
        vt_rs, vt_gap, vt_x = pad, 328, 0
    else:
        vt_rs, vt_gap, vt_x = pad + 72, 328, 16
    vt_bs = KV * vt_rs + vt_gap
    vt_off = GUARD * vt_rs + GUARD + vt_x
    vr = Vt(_new(vt_off + B * vt_bs + GUARD * vt_rs + GUARD, fill, device), vt_off, vt_bs, vt_rs, B, KV, Skv)
    pi = perm_index(pad, device)
    w = vr.window()
    w[:, :, pi[:Skv]] = v.reshape(B, Skv, KV).transpose(1, 2)
    if pad > Skv:
        if fill == "hostile":      # finite, non-zero: the header's "multiplied by p = 0"
            w[:, :, pi[Skv:]] = (torch.rand(B, KV, pad - Skv, generator=g) * 8.0 - 4.0).to(BF).to(device)
        else:
            w[:, :, pi[Skv:]] = 0.0

    # ---- o
    if layout == "compact":
        o_rs, o_rows, o_gap, o_x = D, Sq, 0, 0
    elif layout == "packed":
        o_rs, o_rows, o_gap, o_x = D + 200, Sq + GUARD, 292, 100
    else:
        o_rs, o_rows, o_gap, o_x = D + 76, Sq + 3, 132, 12
    o_bs = o_rows * o_rs + o_gap
    o_off = GUARD * o_rs + o_x
    o_r = Rows(_bits(CANARY_BITS, o_off + B * o_bs + GUARD * o_rs, device), o_off, o_bs, o_rs, B, Sq, D)

    ar = Arena(d, B, H, Sq, Skv, kv_group, layout, fill, qr, kr, vr, o_r, q, k, v)
    ar.check_contract()
    return ar


# ------------------------------------------------------------------------------------------------------------------ references
def sdpa64(q, k, v, scale, causal=False, kv_group=1):
    """float64 softmax(q k^T * scale) v on compact [B, S, heads, d] tensors -> [B, Sq, H, d] float64."""
    qq, kk, vv = (t.double().transpose(1, 2) for t in (q, k, v))
    if kv_group > 1:
        kk, vv = kk.repeat_interleave(kv_group, dim=1), vv.repeat_interleave(kv_group, dim=1)
    sc = qq @ kk.transpose(-1, -2) * scale
    if causal:
        Sq, Skv = sc.shape[-2:]
        sc = sc.masked_fill(torch.ones(Sq, Skv, dtype=torch.bool, device=sc.device).triu(1), -math.inf)
    return (torch.softmax(sc, dim=-1) @ vv).transpose(1, 2)


def failures(ar_f, o_f, ar_h, o_h, baseline, ref=None, max_bound=2e-2, mean_bound=None, strict=True):
    """The four assertions on one call run under both fills of one layout (ar_f / o_f: the friendly arenas and their o arena,
    ar_h / o_h the hostile ones): {name: message} of those that fail -- empty for a correct kernel.  ref = None leaves out 4."""
    checks = [("layout", lambda: (assert_layout_independent(ar_f, o_f, baseline), assert_layout_independent(ar_h, o_h, baseline))),
              ("fill", lambda: assert_fill_independent(ar_h, o_h, o_f)),
              ("footprint", lambda: (assert_footprint(ar_f, o_f), assert_footprint(ar_h, o_h)))]
    if ref is not None:
        checks.append(("reference", lambda: (assert_reference(ar_f, o_f, ref, max_bound, mean_bound, strict),
                                             assert_reference(ar_h, o_h, ref, max_bound, mean_bound, strict))))
    failed = {}
    for name, check in checks:
        try:
            check()
        except AssertionError as e:
            failed[name] = str(e)
    return failed


# ------------------------------------------------------------------------------------------------------------------ assertions
# One set for the emulation (tests/test_attn_arena_cpu.py) and the kernels (tests/test_gpu_attn_operands.py).
def assert_layout_independent(ar, o_full, baseline):
    """1: bit for bit the output on the compact copies."""
    got = ar.extract(o_full)
    same = got.view(torch.int16) == baseline.view(torch.int16)
    assert bool(same.all()), ("layout", ar.layout, ar.fill, int((~same).sum()), (got.double() - baseline.double()).abs().max().item())


def assert_fill_independent(ar, o_hostile, o_friendly):
    """2: what sits outside the live elements (and in the V^T padding columns) does not reach the output."""
    h, f = ar.extract(o_hostile), ar.extract(o_friendly)
    assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(f.float()).all()), ("fill: not finite", ar.layout)
    same = h.view(torch.int16) == f.view(torch.int16)
    assert bool(same.all()), ("fill", ar.layout, int((~same).sum()), (h.double() - f.double()).abs().max().item())


def assert_footprint(ar, o_full):
    """3: every element of the o arena outside the mask still holds the canary."""
    touched = o_full.view(torch.int16)[~ar.o_mask] != CANARY_BITS
    assert not bool(touched.any()), ("footprint", ar.layout, ar.fill, int(touched.sum()))


def assert_reference(ar, o_full, ref, max_bound, mean_bound=None, strict=True):
    """4: against float64 SDPA on the compact copies (max < bound for d = 128, <= bound for d = 64: the existing tests' forms)."""
    err = (ar.extract(o_full).double() - ref).abs()
    mx, mean = err.max().item(), err.mean().item()
    assert (mx < max_bound) if strict else (mx <= max_bound), ("reference max", ar.layout, ar.fill, mx)
    if mean_bound is not None:
        assert mean < mean_bound, ("reference mean", ar.layout, ar.fill, mean)
