"""alg_conv_cl_bf16 against its exact-arithmetic statement (tests/helpers/conv_cl_ref.py), BIT for bit, at the extents where
the GEMM kernel's convolution addressing can go wrong: M tile seams and tails, the tile order's last group, partial N tiles,
both epilogues, every Cin / kt, frame strides, the residual forms, the two-voxel form with and without its skipped MFMA
halves, the stride-2 form, the production pitch, and the persistent loop's second tile.

Every case holds all of this together:
  * x sits in its buffer with EXACTLY the readable slack the header promises (2 Wp + 2 rows, 2 Wp + 3 for the two-voxel form),
    and the slack holds NaN: valid rows never read it, so they come out finite and exact;
  * the whole padded grid of x is random (borders and front frames too): the statement is about flat rows, and a zero border
    would hide a wrong tap exactly where a wrong tap matters;
  * the don't-care rows of a residual hold NaN;
  * y is pre-filled with one bit pattern and sits between two guard bands of one tile-row pitch (256 * ldc elements) holding
    another; after the launch both guards are untouched;
  * valid rows equal the statement under torch.equal -- tolerance zero;
  * two launches are bit-identical."""
import zlib
from typing import NamedTuple, Optional

import pytest
import torch

from alg_amd import _lib
from helpers import conv_cl_ref as R

pytestmark = pytest.mark.gpu

Y_FILL, GUARD = 0x4E4E, 0x5A5A          # bf16 bit patterns (as int16): y before the launch, and the guard bands
BM = 256                                # the GEMM tile's rows


class Case(NamedTuple):
    mode: int
    H: int
    W: int
    Cin: int
    Cout: int
    kt: int
    T: int
    res: Optional[str] = None           # "alias": y = res + conv in place; "off8" / "off4": own buffer at res_off = 8 / 4 elements
    y_off: int = 0                      # extra elements in front of y (4: C is 8- but not 16-byte aligned)
    x_off_frames: int = 0               # frames of x in front of the first one the call is given

    @property
    def id(self):
        s = "%s-%dx%d-ci%d-co%d-kt%d-T%d" % (("plain", "pair", "stride2")[self.mode], self.H, self.W, self.Cin, self.Cout,
                                              self.kt, self.T)
        return s + ("-res_%s" % self.res if self.res else "") + ("-yoff%d" % self.y_off if self.y_off else "") + (
            "-xoff%d" % self.x_off_frames if self.x_off_frames else "")


def _dev():
    return torch.device("cuda:0")


class Inputs(NamedTuple):
    x: torch.Tensor
    w: torch.Tensor
    b: torch.Tensor
    r: Optional[torch.Tensor]           # [T][rows][Cout], NaN in the don't-care rows
    rows: int                           # rows per frame of y
    valid: torch.Tensor


def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(c)).encode()))
    Hp, Wp = c.H + 2, c.W + 2
    frames_in = c.x_off_frames + c.T + c.kt - 1
    x = torch.cat([R.draw(g, frames_in * Hp * Wp * c.Cin, R.X_STEP, R.X_MAX),
                   torch.full((R.slack_rows(Wp, c.mode) * c.Cin,), float("nan"), dtype=torch.bfloat16)])
    w = R.draw(g, c.Cout * c.kt * 9 * c.Cin, R.W_STEP, R.W_MAX).reshape(c.Cout, -1)
    b = R.draw(g, c.Cout, R.B_STEP, R.B_MAX)
    if c.mode == R.PAIR:
        w, b = _lib.pack_conv_pair(w, b, c.kt)
    rows = R.stride2_rows(c.H, Wp) if c.mode == R.STRIDE2 else Hp * Wp
    valid = R.valid_mask(Hp, Wp, c.mode)
    r = None
    if c.res:
        r = R.draw(g, c.T * rows * c.Cout, R.B_STEP, R.B_MAX).reshape(c.T, rows, c.Cout)
        r[:, ~valid] = float("nan")
    R.check_exact(w.shape[1], x, w, b, r)
    d = _dev()
    return Inputs(x.to(d), w.to(d), b.to(d), None if r is None else r.to(d), rows, valid.to(d))


def _launch(c, i):
    """one launch into a fresh guarded buffer -> (y region [T][rows][Cout] bf16, front guard, back guard) as views"""
    Hp, Wp = c.H + 2, c.W + 2
    n, guard = c.T * i.rows * c.Cout, BM * c.Cout * (2 if c.mode == R.PAIR else 1)      # 256 * ldc
    front = guard + c.y_off
    buf = torch.empty(front + n + guard, dtype=torch.int16, device=_dev())
    buf[:front], buf[front:front + n], buf[front + n:] = GUARD, Y_FILL, GUARD
    ybf = buf.view(torch.bfloat16)
    res, res_off = None, 0
    if c.res == "alias":
        ybf[front:front + n] = i.r.reshape(-1)
        res, res_off = ybf, front
    elif c.res:
        res_off = int(c.res[3:])
        res = torch.cat([torch.full((res_off,), float("nan"), dtype=torch.bfloat16, device=_dev()), i.r.reshape(-1)])
    _lib.conv_cl(i.x, i.w, i.b, res, ybf, c.T, Hp, Wp, c.Cin, c.Cout, c.kt, pair=c.mode == R.PAIR, stride2=c.mode == R.STRIDE2,
                 x_off=c.x_off_frames * Hp * Wp * c.Cin, y_off=front, res_off=res_off)
    return ybf[front:front + n].reshape(c.T, i.rows, c.Cout), buf[:front], buf[front + n:]


def _want(c, i):
    return R.conv_cl_statement(i.x, i.w, i.b, None if i.r is None else i.r.reshape(-1), c.T, c.H + 2, c.W + 2, c.Cin, c.Cout,
                               c.kt, c.mode, x_off=c.x_off_frames * (c.H + 2) * (c.W + 2) * c.Cin)


def _assert_exact(c, i, got, want):
    g, w = got[:, i.valid], want[:, i.valid]
    assert bool(torch.isfinite(w.float()).all()), "the statement itself is not finite on a valid row"
    if torch.equal(g, w):
        return
    bad = ~(g == w)                                     # (a NaN in a valid row is bad too)
    t, vi, ch = (int(v) for v in bad.nonzero()[0])
    row = int(i.valid.nonzero()[vi])
    yy, xx = divmod(row, c.W + 2)
    gemm_row = row // 2 if c.mode == R.PAIR else row
    pytest.fail("%s: %d of %d valid elements differ; first at (frame %d, y %d, x %d, channel %d), GEMM row %d = %d mod 256: "
                "got %r, want %r" % (c.id, int(bad.sum()), bad.numel(), t, yy, xx, ch, gemm_row, gemm_row % BM,
                                     float(g[t, vi, ch]), float(w[t, vi, ch])))


def _check(c):
    i = _inputs(c)
    want = _want(c, i)
    got, front, back = _launch(c, i)
    assert bool((front == GUARD).all()), "%s: the launch wrote in front of y" % c.id
    assert bool((back == GUARD).all()), "%s: the launch wrote behind y" % c.id
    _assert_exact(c, i, got, want)
    again, front2, back2 = _launch(c, i)
    assert bool((front2 == GUARD).all() and (back2 == GUARD).all())
    assert torch.equal(again.view(torch.int16), got.view(torch.int16)), "%s: two launches differ" % c.id
    return got


P, PR, S2 = R.PLAIN, R.PAIR, R.STRIDE2

TILES = [
    Case(P, 14, 14, 64, 128, 3, 3),                      # Hp*Wp = 256 = BM: one whole tile, no clamped row
    Case(P, 14, 15, 64, 128, 3, 3),                      # 272 rows: a 16-row tail tile, clamp at m0 = 256 (the last 2 Wp + 2
                                                         # rows of a frame are don't-care: this tail must only do no harm)
    Case(P, 32, 64, 64, 256, 3, 2),                      # 34 x 66 = 2244 rows, 9 M tiles: the last group (of 8) has one tile,
                                                         # and its 196-row tail holds 62 valid rows
]
N_TAILS = [Case(P, 14, 15, 128, co, 3, 2) for co in (4, 12, 64, 192, 320)] + [
    Case(P, 14, 15, 128, 4, 3, 2, y_off=4),              # element epilogue twice over: N % 8 != 0, C not 16-byte aligned
    Case(P, 14, 15, 128, 64, 3, 2, y_off=4),             # ... and by the C pointer alone
]
CIN = [Case(P, 14, 15, ci, 128, kt, 2) for ci in (64, 256, 512) for kt in (3, 1)]   # 1, 4, 8 k-tiles per tap; K = 576 at (64, 1)
FRAMES = [Case(P, 14, 15, 128, 128, 3, T) for T in (1, 2, 7)]
RESIDUAL = [
    Case(P, 14, 15, 128, 128, 3, 2, res="alias"), Case(P, 14, 15, 128, 128, 3, 2, res="off8"),
    Case(P, 14, 15, 128, 128, 3, 2, res="off4"),         # R not 16-byte aligned: the element epilogue with a residual
    Case(P, 14, 15, 128, 12, 3, 2, res="alias"),         # ... and by N % 8 != 0, in place
    Case(P, 32, 64, 64, 320, 1, 2, res="alias"),         # in place over several tiles and a partial N tile
    Case(PR, 14, 14, 128, 128, 3, 2, res="alias"), Case(PR, 14, 15, 128, 64, 3, 2, res="off8"),
]
PAIR_256 = [Case(PR, H, W, ci, 128, kt, 2) for (H, W) in ((8, 13), (14, 14), (32, 64)) for ci in (128, 256) for kt in (3, 1)]
PAIR_NARROW = [Case(PR, 14, 15, 128, co, 3, 2) for co in (64, 4, 12)] + [Case(PR, 32, 64, 128, 64, 3, 2)]
STRIDE_2 = [Case(S2, H, W, ci, co, 1, T, x_off_frames=2 if T == 1 else 0)      # (one frame at x_off = two frames: the CogVideoX encoder)
            for (ci, co) in ((128, 128), (256, 256), (64, 128)) for (H, W) in ((8, 12), (30, 62)) for T in (1, 3)]
PITCH = [Case(PR, 2, 720, 128, 128, 3, 2), Case(P, 2, 720, 128, 4, 3, 2), Case(P, 2, 360, 256, 256, 3, 2),
         Case(PR, 2, 360, 256, 128, 3, 2)]

CASES = TILES + N_TAILS + CIN + FRAMES + RESIDUAL + PAIR_256 + PAIR_NARROW + STRIDE_2 + PITCH
assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_conv_cl_is_its_statement_to_the_bit(c):
    _check(c)


def test_persistent_loop_second_tile():
    """T = 8, 64 x 69 = 4416 rows (18 M tiles) x Cout 512 (2 N tiles) = 288 tiles: more than the grid (the CU count rounded
    down to a multiple of 8), so workgroups take a second tile -- LDS is re-staged right behind the first tile's epilogue."""
    grid = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    T = max(8, grid // 36 + 1)                           # (a bigger device: more frames)
    c = Case(P, 62, 67, 64, 512, 1, T)
    m_tiles, n_tiles = -(-(c.H + 2) * (c.W + 2) // BM), -(-c.Cout // 256)
    assert (m_tiles, n_tiles) == (18, 2) and m_tiles * n_tiles * T > grid, (m_tiles, n_tiles, T, grid)
    _check(c)


def test_conv_route_ignores_gemm_pipe(monkeypatch):
    """the convolution runs schedule 6 whatever ALG_GEMM_PIPE says: same bits under 9 and 6 (and both are the statement's)"""
    c = Case(P, 14, 15, 128, 128, 3, 2)
    monkeypatch.setenv("ALG_GEMM_PIPE", "9")
    a = _check(c)
    monkeypatch.setenv("ALG_GEMM_PIPE", "6")
    b = _check(c)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
