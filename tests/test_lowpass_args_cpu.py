"""The low-pass filters' host path on a machine WITHOUT a GPU: every refusal of alg_down_up, alg_gaussian_blur,
alg_lowpass_tables_build and the three size queries with its exact text and its place in the order of checks (lowpass.hip:
lowpass_check), and the route a valid call takes (lowpass_plan) under ALG_LOWPASS_PATH 0..4.

No operand is ever dereferenced: a refused call returns before any HIP call, and without a device a valid call ends at its first
HIP call -- the LDS opt-in of the planned kernel or, for the global-memory passes, the launch -- whose message names the entry
and the route.  The expected refusals were recorded from the library before check, plan and launch were separated; that part of
the file (everything above "routes") passes unchanged against that library (ALG_HIP_LIB).  The route part is what the separation
made observable: before it the message of a failed call said nothing about the kernel it was headed for.

Without a device the library sizes its grids for 256 compute units, the MI355X's own: the register-blocked kernels take calls of
128 planes and more, the persistent-grid kernels calls of more than 512.

With a GPU the file is skipped: a check lost by mistake would launch a kernel on host pointers."""
import ctypes
import math

import numpy as np
import pytest
import torch

import alg_amd

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")

OK, EINVAL, ELAUNCH, ELIMIT = 0, -1, -2, -3
F32, BF16 = 0, 1
_BUF = ctypes.create_string_buffer(2048)
P0 = (ctypes.addressof(_BUF) + 255) & ~255          # a 256-byte aligned host address
IN, OUT, TAB, WS = (P0 + 256 * i for i in range(4))
BIG = 1 << 40                                       # bytes of workspace "behind" WS: never touched

DU, G = "alg_down_up", "alg_gaussian_blur"
DU_BAD = DU + ": bad argument (planes=%d H=%d W=%d h1=%d w1=%d)"
G_BAD = G + ": bad argument (planes=%d H=%d W=%d)"
DTYPE = "%s: unsupported dtype code %d"
ALIAS = "%s: in and out must not alias"
TABLES = DU + ": tables must be 16-byte aligned"
KSIZE = G + ": kernel size must be odd and positive, got %d"
SIGMA = G + ": sigma must be positive, got %s"
REFLECT = G + ": reflect padding needs ksize/2 < min(H, W) (ksize=%d H=%d W=%d)"
WORKSPACE = ("%s: this shape runs through global-memory passes and needs a 16-byte aligned workspace of %d bytes "
             "(%s_workspace_bytes); got %s / %d bytes")
GRID = "%s: %d planes of %dx%d exceed the global-memory path's grid"
BUILD = "alg_lowpass_tables_build"
BUILD_BAD = BUILD + ": bad argument (tables=%s H=%d W=%d h1=%d w1=%d; 16-byte aligned blob)"
BUILD_SHORT = BUILD + ": blob of %d bytes, alg_lowpass_tables_bytes says %d"


def ptr(p):
    """printf's %p"""
    return "0x%x" % p if p else "(nil)"


@pytest.fixture(scope="module")
def lib():
    return alg_amd.load_library()


def down_up(lib, **kw):
    """A valid call: 4 planes of 12 x 16 -> 6 x 8, fp32, the caller's tap tables"""
    a = dict(inp=IN, out=OUT, planes=4, H=12, W=16, h1=6, w1=8, dtype=F32, round=1, tables=TAB, ws=None, wsb=0)
    a.update(kw)
    rc = lib.alg_down_up(a["inp"], a["out"], a["planes"], a["H"], a["W"], a["h1"], a["w1"], a["dtype"], a["round"], a["tables"],
                         a["ws"], a["wsb"], None)
    return rc, lib.alg_last_error().decode()


def gaussian(lib, **kw):
    """A valid call: 4 planes of 12 x 16, 5 taps, fp32"""
    a = dict(inp=IN, out=OUT, planes=4, H=12, W=16, ksize=5, sigma=1.2, dtype=F32, ws=None, wsb=0)
    a.update(kw)
    rc = lib.alg_gaussian_blur(a["inp"], a["out"], a["planes"], a["H"], a["W"], a["ksize"], a["sigma"], a["dtype"], a["ws"],
                               a["wsb"], None)
    return rc, lib.alg_last_error().decode()


PIXEL = dict(planes=3, H=480, W=720, h1=120, w1=180)              # beyond 160 KiB of LDS: the global-memory passes
PIXEL_BYTES = 4 * 3 * (480 * 180 + 120 * 180 + 120 * 720)
PIXEL_G = dict(planes=3, H=480, W=720, ksize=9)
PIXEL_G_BYTES = 4 * (3 * 480 * 720 + 256)

# ---- alg_down_up: (id, arguments, return code, text)
DU_REFUSALS = [
    ("null in", dict(inp=None), EINVAL, DU_BAD % (4, 12, 16, 6, 8)),
    ("null out", dict(out=None), EINVAL, DU_BAD % (4, 12, 16, 6, 8)),
    ("planes < 0", dict(planes=-1), EINVAL, DU_BAD % (-1, 12, 16, 6, 8)),
    ("H = 0", dict(H=0), EINVAL, DU_BAD % (4, 0, 16, 6, 8)),
    ("W < 0", dict(W=-16), EINVAL, DU_BAD % (4, 12, -16, 6, 8)),
    ("h1 = 0", dict(h1=0), EINVAL, DU_BAD % (4, 12, 16, 0, 8)),
    ("w1 < 0", dict(w1=-8), EINVAL, DU_BAD % (4, 12, 16, 6, -8)),
    ("no planes, no plane", dict(planes=0, H=0), EINVAL, DU_BAD % (0, 0, 16, 6, 8)),
    ("dtype 2", dict(dtype=2), EINVAL, DTYPE % (DU, 2)),
    ("dtype -1", dict(dtype=-1), EINVAL, DTYPE % (DU, -1)),
    ("in == out", dict(out=IN), EINVAL, ALIAS % DU),
    ("tables + 8 bytes", dict(tables=TAB + 8), EINVAL, TABLES),
    ("tables + 4 bytes, bf16", dict(tables=TAB + 4, dtype=BF16), EINVAL, TABLES),
    # the global-memory passes: the grid's limit, then the workspace
    ("pixel plane, no workspace", dict(PIXEL), EINVAL, WORKSPACE % (DU, PIXEL_BYTES, DU, ptr(0), 0)),
    ("pixel plane, no workspace but bytes", dict(PIXEL, wsb=BIG), EINVAL, WORKSPACE % (DU, PIXEL_BYTES, DU, ptr(0), BIG)),
    ("pixel plane, workspace + 8 bytes", dict(PIXEL, ws=WS + 8, wsb=BIG), EINVAL, WORKSPACE % (DU, PIXEL_BYTES, DU, ptr(WS + 8), BIG)),
    ("pixel plane, workspace one byte short", dict(PIXEL, ws=WS, wsb=PIXEL_BYTES - 1), EINVAL,
     WORKSPACE % (DU, PIXEL_BYTES, DU, ptr(WS), PIXEL_BYTES - 1)),
    ("65536 pixel planes", dict(PIXEL, planes=65536, ws=WS, wsb=BIG), ELIMIT, GRID % (DU, 65536, 480, 720)),
    ("65536 rows", dict(planes=1, H=65536, W=4, h1=8, w1=2, ws=WS, wsb=BIG), ELIMIT, GRID % (DU, 1, 65536, 4)),
    ("65536 rows after the first resample", dict(planes=1, H=8, W=2, h1=65536, w1=4, ws=WS, wsb=BIG), ELIMIT, GRID % (DU, 1, 8, 2)),
    # order: the earlier refusal wins
    ("null before dtype", dict(inp=None, dtype=7), EINVAL, DU_BAD % (4, 12, 16, 6, 8)),
    ("size before alias", dict(out=IN, w1=0), EINVAL, DU_BAD % (4, 12, 16, 6, 0)),
    ("dtype before alias", dict(out=IN, dtype=7), EINVAL, DTYPE % (DU, 7)),
    ("alias before tables", dict(out=IN, tables=TAB + 8), EINVAL, ALIAS % DU),
    ("alias before workspace", dict(PIXEL, out=IN), EINVAL, ALIAS % DU),
    ("dtype before the grid's limit", dict(PIXEL, planes=65536, dtype=3), EINVAL, DTYPE % (DU, 3)),
    ("the grid's limit before the workspace", dict(PIXEL, planes=65536), ELIMIT, GRID % (DU, 65536, 480, 720)),
    # the tables are not read by the global-memory passes: their alignment is not asked for there
    ("pixel plane, tables + 8 bytes", dict(PIXEL, tables=TAB + 8), EINVAL, WORKSPACE % (DU, PIXEL_BYTES, DU, ptr(0), 0)),
]


@pytest.mark.parametrize("name,kw,rc,text", DU_REFUSALS, ids=[r[0] for r in DU_REFUSALS])
def test_down_up_refusal(lib, name, kw, rc, text):
    assert down_up(lib, **kw) == (rc, text)


# ---- alg_gaussian_blur
G_REFUSALS = [
    ("null in", dict(inp=None), EINVAL, G_BAD % (4, 12, 16)),
    ("null out", dict(out=None), EINVAL, G_BAD % (4, 12, 16)),
    ("planes < 0", dict(planes=-3), EINVAL, G_BAD % (-3, 12, 16)),
    ("H < 0", dict(H=-12), EINVAL, G_BAD % (4, -12, 16)),
    ("W = 0", dict(W=0), EINVAL, G_BAD % (4, 12, 0)),
    ("no planes, no plane", dict(planes=0, W=0), EINVAL, G_BAD % (0, 12, 0)),
    ("ksize = 0", dict(ksize=0), EINVAL, KSIZE % 0),
    ("ksize < 0", dict(ksize=-3), EINVAL, KSIZE % -3),
    ("ksize even", dict(ksize=4), EINVAL, KSIZE % 4),
    ("sigma = 0", dict(sigma=0.0), EINVAL, SIGMA % "0"),
    ("sigma < 0", dict(sigma=-1.5), EINVAL, SIGMA % "-1.5"),
    ("sigma NaN", dict(sigma=math.nan), EINVAL, SIGMA % "nan"),
    ("ksize / 2 = H", dict(ksize=25), EINVAL, REFLECT % (25, 12, 16)),
    ("ksize / 2 = W", dict(H=40, W=12, ksize=25), EINVAL, REFLECT % (25, 40, 12)),
    ("ksize / 2 > H", dict(ksize=255), EINVAL, REFLECT % (255, 12, 16)),
    ("dtype 2", dict(dtype=2), EINVAL, DTYPE % (G, 2)),
    ("in == out", dict(inp=OUT), EINVAL, ALIAS % G),
    ("pixel plane, no workspace", dict(PIXEL_G), EINVAL, WORKSPACE % (G, PIXEL_G_BYTES, G, ptr(0), 0)),
    ("pixel plane, workspace + 4 bytes", dict(PIXEL_G, ws=WS + 4, wsb=BIG), EINVAL, WORKSPACE % (G, PIXEL_G_BYTES, G, ptr(WS + 4), BIG)),
    ("pixel plane, workspace one byte short", dict(PIXEL_G, ws=WS, wsb=PIXEL_G_BYTES - 1), EINVAL,
     WORKSPACE % (G, PIXEL_G_BYTES, G, ptr(WS), PIXEL_G_BYTES - 1)),
    # more than 255 taps: the global-memory passes, whatever the plane (129 x 129 x 2 floats are 130 KiB)
    ("257 taps, no workspace", dict(planes=2, H=129, W=129, ksize=257), EINVAL,
     WORKSPACE % (G, 4 * (2 * 129 * 129 + 512), G, ptr(0), 0)),
    ("65536 pixel planes", dict(PIXEL_G, planes=65536, ws=WS, wsb=BIG), ELIMIT, GRID % (G, 65536, 480, 720)),
    ("65536 rows", dict(planes=1, H=65536, W=4, ksize=3, ws=WS, wsb=BIG), ELIMIT, GRID % (G, 1, 65536, 4)),
    # order
    ("null before ksize", dict(out=None, ksize=4), EINVAL, G_BAD % (4, 12, 16)),
    ("ksize before sigma", dict(ksize=6, sigma=0.0), EINVAL, KSIZE % 6),
    ("sigma before reflect", dict(ksize=25, sigma=-2.0), EINVAL, SIGMA % "-2"),
    ("reflect before dtype", dict(ksize=25, dtype=9), EINVAL, REFLECT % (25, 12, 16)),
    ("dtype before alias", dict(dtype=9, out=IN), EINVAL, DTYPE % (G, 9)),
    ("alias before workspace", dict(PIXEL_G, out=IN), EINVAL, ALIAS % G),
    ("the grid's limit before the workspace", dict(PIXEL_G, planes=65536), ELIMIT, GRID % (G, 65536, 480, 720)),
]


@pytest.mark.parametrize("name,kw,rc,text", G_REFUSALS, ids=[r[0] for r in G_REFUSALS])
def test_gaussian_refusal(lib, name, kw, rc, text):
    assert gaussian(lib, **kw) == (rc, text)


def test_an_empty_batch_is_done_before_any_check(lib):
    """planes == 0 with a plane size: nothing to do, whatever the rest says (pointers may be null)"""
    assert down_up(lib, planes=0)[0] == OK
    assert down_up(lib, planes=0, inp=None, out=None, dtype=7, h1=0, tables=TAB + 8)[0] == OK
    assert gaussian(lib, planes=0)[0] == OK
    assert gaussian(lib, planes=0, inp=None, out=None, ksize=4, sigma=-1.0, dtype=7)[0] == OK


def test_option_4_sends_latent_planes_through_the_same_refusals(lib, monkeypatch):
    monkeypatch.setenv("ALG_LOWPASS_PATH", "4")
    need = 4 * 4 * (12 * 8 + 6 * 8 + 6 * 16)
    assert lib.alg_down_up_workspace_bytes(4, 12, 16, 6, 8) == need
    assert down_up(lib) == (EINVAL, WORKSPACE % (DU, need, DU, ptr(0), 0))
    assert down_up(lib, tables=TAB + 8, ws=WS, wsb=need - 4) == (EINVAL, WORKSPACE % (DU, need, DU, ptr(WS), need - 4))
    assert down_up(lib, planes=65536, ws=WS, wsb=BIG) == (ELIMIT, GRID % (DU, 65536, 12, 16))
    need = 4 * (4 * 12 * 16 + 256)
    assert lib.alg_gaussian_blur_workspace_bytes(4, 12, 16, 5) == need
    assert gaussian(lib, ws=WS + 8, wsb=BIG) == (EINVAL, WORKSPACE % (G, need, G, ptr(WS + 8), BIG))
    assert gaussian(lib, planes=70000, ws=WS, wsb=BIG) == (ELIMIT, GRID % (G, 70000, 12, 16))


def test_option_1_reads_no_tables(lib, monkeypatch):
    """the plane-per-workgroup kernels build their taps in LDS: misaligned tables are not refused, the call goes on to its launch"""
    monkeypatch.setenv("ALG_LOWPASS_PATH", "1")
    assert down_up(lib, tables=TAB + 8)[0] == ELAUNCH
    assert down_up(lib, out=IN, tables=TAB + 8) == (EINVAL, ALIAS % DU)


# ---- alg_lowpass_tables_build and the three size queries
def build(lib, tables=TAB, nbytes=960, H=12, W=16, h1=6, w1=8):
    rc = lib.alg_lowpass_tables_build(tables, nbytes, H, W, h1, w1, None)
    return rc, lib.alg_last_error().decode()


def test_tables_build_refusals(lib):
    # 12 x 16 -> 6 x 8: tables of 8 x (2 + 5), 6 x (2 + 5), 16 x (2 + 3) and 12 x (2 + 3) words, rounded up to four
    assert lib.alg_lowpass_tables_bytes(12, 16, 6, 8) == 960
    assert build(lib, tables=None) == (EINVAL, BUILD_BAD % (ptr(0), 12, 16, 6, 8))
    assert build(lib, tables=TAB + 8) == (EINVAL, BUILD_BAD % (ptr(TAB + 8), 12, 16, 6, 8))
    assert build(lib, H=0) == (EINVAL, BUILD_BAD % (ptr(TAB), 0, 16, 6, 8))
    assert build(lib, W=-1) == (EINVAL, BUILD_BAD % (ptr(TAB), 12, -1, 6, 8))
    assert build(lib, h1=0) == (EINVAL, BUILD_BAD % (ptr(TAB), 12, 16, 0, 8))
    assert build(lib, w1=0) == (EINVAL, BUILD_BAD % (ptr(TAB), 12, 16, 6, 0))
    assert build(lib, nbytes=956) == (EINVAL, BUILD_SHORT % (956, 960))
    assert build(lib, nbytes=-1) == (EINVAL, BUILD_SHORT % (-1, 960))
    assert build(lib, tables=None, nbytes=0) == (EINVAL, BUILD_BAD % (ptr(0), 12, 16, 6, 8))       # the argument before the size
    rc, text = build(lib)
    assert rc == ELAUNCH and text.startswith(BUILD + ": launch failed: "), text


def test_size_queries_of_no_problem(lib):
    for shape in ((0, 16, 6, 8), (12, -16, 6, 8), (12, 16, 0, 8), (12, 16, 6, -1)):
        assert lib.alg_lowpass_tables_bytes(*shape) == 0
        assert lib.alg_down_up_workspace_bytes(3, *shape) == 0
    assert lib.alg_down_up_workspace_bytes(0, 480, 720, 120, 180) == 0
    assert lib.alg_down_up_workspace_bytes(-3, 480, 720, 120, 180) == 0
    for args in ((0, 480, 720, 9), (-1, 480, 720, 9), (3, 0, 720, 9), (3, 480, -720, 9), (3, 480, 720, 0), (3, 480, 720, -9)):
        assert lib.alg_gaussian_blur_workspace_bytes(*args) == 0


# =====================================================================================================================
# routes.  Without a device the first HIP call of a valid call fails, and its message names the entry and the route
# =====================================================================================================================
PLANE, PERSISTENT, BLOCKED, GLOBAL = "plane-per-workgroup kernel", "persistent-grid kernel", "register-blocked kernel", \
    "global-memory passes"
CUS, CAP = 256, 160 * 1024


def failure(entry, route):
    if route == GLOBAL:
        return "%s (%s): launch failed: " % (entry, route)
    return "%s (%s): hipFuncSetAttribute(%d B LDS): " % (entry, route, CAP)


def aa_taps(n_in, n_out):
    """taps of one antialiased output, in fp32 as the library computes it"""
    scale = np.float32(n_in) / np.float32(n_out)
    return int(math.ceil(max(scale, np.float32(1.0)))) * 2 + 1


def up16(n):
    return (n + 15) & ~15


def up4(n):
    return (n + 3) & ~3


def expected_route(kind, planes, H, W, arg, dtype=F32, option=0, tables=True, aligned=True):
    """include/alg_hip.h, the filter section: which kernel a call of `planes` planes of H x W runs; `arg` = (h1, w1) | ksize"""
    esz, n = (4 if dtype == F32 else 2), H * W
    if kind == "down_up":
        h1, w1 = arg
        taps = dict(dw=aa_taps(W, w1), dh=aa_taps(H, h1), uw=aa_taps(w1, W), uh=aa_taps(h1, H))
        lds = up16(4 * (n + H * w1 + h1 * w1) + w1 * (8 + 4 * taps["dw"]) + h1 * (8 + 4 * taps["dh"]) + W * (8 + 4 * taps["uw"]) +
                   H * (8 + 4 * taps["uh"]))
        wide = False
    else:
        k = arg
        lds, wide = up16(4 * (2 * n + k)), k > 255
    if option == 4 or lds > CAP or wide:
        return GLOBAL
    if option == 1 or (kind == "down_up" and not tables):
        return PLANE
    # the register-blocked kernels
    if option != 2 and W % 2 == 0 and n % 4 == 0 and aligned and planes >= (1 if option == 3 else CUS // 2):
        WS = up4(W)
        if kind == "gaussian":
            pad = k // 2
            fits = 3 <= k <= 19 and pad + 1 < H and pad + 1 < W and \
                16 * ((H * (WS + 2 * up4(pad)) + (H + 2 * pad) * WS + k + 3) // 4) <= CAP and 512 * 32 >= n and 512 * 4 >= H * 2 * pad
        else:
            VS, TP = up4(w1), (taps["dh"] + 1) & ~1
            floats = H * WS + 16 + H * VS + h1 * VS + 16 + up4(h1) + up4(h1 * TP) + H * 4
            fits = taps["uw"] == 3 and taps["uh"] == 3 and taps["dw"] <= 11 and taps["dh"] <= 64 and 4 * floats <= CAP and \
                1024 * 32 >= n and w1 <= 1024 and WS // 4 <= 1024
        if fits:
            return BLOCKED
    # the persistent-grid kernels: 16-byte-granular planes, more than two per CU, at most four 16-byte loads per thread
    if (n * esz) % 16 == 0 and aligned and planes > 2 * CUS and n * esz <= 4 * 16 * 1024:
        if kind == "gaussian":
            fits = 4 * (2 * up4(n) + k) <= CAP
        else:
            a_fl = up4(max(n, up4(h1 * W) + (n * esz + 3) // 4))
            words = up4(w1 * (2 + taps["dw"]) + h1 * (2 + taps["dh"]) + W * (2 + taps["uw"]) + H * (2 + taps["uh"]))
            fits = 4 * (a_fl + H * w1 + up4(h1 * w1) + words + 16) <= CAP and taps["dw"] <= 64 and (H * w1) % 4 == 0
        if fits:
            return PERSISTENT
    return PLANE


def run(lib, kind, planes, H, W, arg, dtype=F32, tables=True, aligned=True, **kw):
    """the call with a workspace large enough for any route; misaligned = in and out 8 bytes off"""
    off = 0 if aligned else 8
    if kind == "down_up":
        return down_up(lib, inp=IN + off, out=OUT + off, planes=planes, H=H, W=W, h1=arg[0], w1=arg[1], dtype=dtype,
                       tables=TAB if tables else None, ws=WS, wsb=BIG, **kw)
    return gaussian(lib, inp=IN + off, out=OUT + off, planes=planes, H=H, W=W, ksize=arg, sigma=1.2, dtype=dtype, ws=WS, wsb=BIG, **kw)


def route_of(lib, kind, *a, **kw):
    entry = DU if kind == "down_up" else G
    rc, text = run(lib, kind, *a, **kw)
    assert rc == ELAUNCH, (rc, text)
    for r in (PLANE, PERSISTENT, BLOCKED, GLOBAL):
        if text.startswith(failure(entry, r)):
            return r
    raise AssertionError(text)


# ---- the calls of the GPU test test_every_route_is_bit_identical: 576 planes of 12 x 16 -- more than two planes per CU, plane
# bytes 16-granular in both dtypes, W even, H * W a multiple of four -- gaussian k = 5, down_up to 6 x 8 (5 and 3 taps)
WALK = [BLOCKED, PLANE, PERSISTENT, BLOCKED, GLOBAL]


@pytest.mark.parametrize("option", range(5))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind,arg", [("down_up", (6, 8)), ("gaussian", 5)], ids=["down_up", "gaussian"])
def test_the_routes_the_gpu_walk_takes(lib, monkeypatch, kind, arg, dtype, option):
    monkeypatch.setenv("ALG_LOWPASS_PATH", str(option))
    assert route_of(lib, kind, 576, 12, 16, arg, dtype) == WALK[option]
    assert expected_route(kind, 576, 12, 16, arg, dtype, option) == WALK[option]


# ---- the plane-count thresholds: 128 = half the CUs (register-blocked), 512 = two per CU (persistent grid, thread counts)
@pytest.mark.parametrize("option", range(5))
@pytest.mark.parametrize("planes", [127, 128, 512, 513])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind,arg", [("down_up", (15, 22)), ("gaussian", 9)], ids=["down_up", "gaussian"])
def test_route_by_plane_count_and_option(lib, monkeypatch, kind, arg, dtype, planes, option):
    """a C2 latent plane (60 x 88: every kernel covers it)"""
    monkeypatch.setenv("ALG_LOWPASS_PATH", str(option))
    want = {0: BLOCKED if planes >= 128 else PLANE, 1: PLANE, 2: PERSISTENT if planes > 512 else PLANE, 3: BLOCKED, 4: GLOBAL}[option]
    assert route_of(lib, kind, planes, 60, 88, arg, dtype) == want
    assert expected_route(kind, planes, 60, 88, arg, dtype, option) == want


# ---- each side of every coverage rule, at 600 planes (both thresholds passed): (id, kind, H, W, arg, dtype, keywords, route)
RULES = [
    ("even W", "gaussian", 12, 16, 5, F32, {}, BLOCKED),
    ("odd W, 16-byte planes", "gaussian", 16, 15, 5, F32, {}, PERSISTENT),
    ("odd W, odd plane", "gaussian", 15, 15, 5, F32, {}, PLANE),
    ("H * W = 2 mod 4, bf16: 4-byte granular planes", "gaussian", 15, 18, 5, BF16, {}, PLANE),
    ("H * W = 2 mod 4, fp32: 8-byte granular planes", "gaussian", 15, 18, 5, F32, {}, PLANE),
    ("H * W = 4 mod 8, bf16: plane bytes not a multiple of 16", "gaussian", 6, 18, 5, BF16, {}, BLOCKED),
    ("H * W = 4 mod 8, bf16, not blocked", "gaussian", 6, 18, 5, BF16, dict(option=2), PLANE),
    ("H * W = 4 mod 8, fp32, not blocked", "gaussian", 6, 18, 5, F32, dict(option=2), PERSISTENT),
    ("ksize 1", "gaussian", 12, 16, 1, F32, {}, PERSISTENT),
    ("ksize 3", "gaussian", 12, 16, 3, F32, {}, BLOCKED),
    ("ksize 19", "gaussian", 24, 32, 19, F32, {}, BLOCKED),
    ("ksize 21", "gaussian", 24, 32, 21, F32, {}, PERSISTENT),
    ("ksize 255", "gaussian", 129, 129, 255, F32, {}, PLANE),
    ("ksize 255, 16-byte planes", "gaussian", 128, 132, 255, F32, {}, PLANE),
    ("ksize 257", "gaussian", 129, 129, 257, F32, {}, GLOBAL),
    ("pad + 1 = H - 1", "gaussian", 9, 16, 15, F32, {}, BLOCKED),
    ("pad + 1 = H", "gaussian", 8, 16, 15, F32, {}, PERSISTENT),
    ("pad + 1 = W", "gaussian", 16, 10, 19, F32, {}, PERSISTENT),
    ("11 down taps", "down_up", 18, 22, (4, 5), F32, {}, BLOCKED),
    ("13 down taps along W", "down_up", 18, 22, (4, 4), F32, {}, PERSISTENT),
    ("13 down taps along W, bf16: 8-byte granular planes", "down_up", 18, 22, (4, 4), BF16, {}, PLANE),
    ("13 down taps along H only", "down_up", 18, 22, (3, 5), F32, {}, BLOCKED),
    ("upsampling first: 5 taps on the way back", "down_up", 12, 16, (24, 32), F32, {}, PERSISTENT),
    ("no tables", "down_up", 12, 16, (6, 8), F32, dict(tables=False), PLANE),
    ("no tables, blocked asked for", "down_up", 12, 16, (6, 8), F32, dict(tables=False, option=3), PLANE),
    ("no tables, global", "down_up", 12, 16, (6, 8), F32, dict(tables=False, option=4), GLOBAL),
    ("in / out 8 bytes off", "down_up", 12, 16, (6, 8), F32, dict(aligned=False), PLANE),
    ("in / out 8 bytes off, gaussian", "gaussian", 12, 16, 5, BF16, dict(aligned=False), PLANE),
    ("in / out 8 bytes off, global", "gaussian", 12, 16, 5, BF16, dict(aligned=False, option=4), GLOBAL),
    ("H * w1 = 2 mod 4", "down_up", 6, 16, (3, 7), F32, dict(option=2), PLANE),
    ("H * w1 = 0 mod 4", "down_up", 6, 16, (3, 8), F32, dict(option=2), PERSISTENT),
    ("64 KiB planes: four prefetch registers at 1024 threads", "gaussian", 128, 128, 5, F32, dict(option=2), PERSISTENT),
    ("64 KiB + 16 bytes", "gaussian", 129, 124 + 8, 5, F32, dict(option=2), PLANE),
    # 160 KiB of LDS.  gaussian, plane-per-workgroup kernel: 16 * ceil((8 H W + 4 k) / 16) bytes
    ("gaussian at 160 KiB", "gaussian", 127, 161, 19, F32, dict(option=1), PLANE),            # 163,664 B
    ("gaussian beyond 160 KiB", "gaussian", 128, 160, 5, F32, dict(option=1), GLOBAL),         # 163,872 B
    ("gaussian at 160 KiB, any route", "gaussian", 127, 161, 19, F32, {}, PLANE),
    # down_up, plane-per-workgroup kernel: X, T1, T2 and the four tap tables
    ("down_up at 160 KiB", "down_up", 180, 160, (45, 40), F32, dict(option=1), PLANE),           # 161,744 B
    ("down_up at 160 KiB, any route", "down_up", 180, 160, (45, 40), F32, {}, BLOCKED),          # (156,208 B of its own layout)
    ("down_up at 160 KiB, not blocked", "down_up", 180, 160, (45, 40), F32, dict(option=2), PLANE),   # 112.5 KiB: 8 prefetch loads
    ("down_up beyond 160 KiB", "down_up", 184, 160, (46, 40), F32, {}, GLOBAL),                  # 165,232 B
    ("down_up beyond 160 KiB, blocked asked for", "down_up", 184, 160, (46, 40), F32, dict(option=3), GLOBAL),
]


@pytest.mark.parametrize("name,kind,H,W,arg,dtype,kw,want", RULES, ids=[r[0] for r in RULES])
def test_each_side_of_every_coverage_rule(lib, monkeypatch, name, kind, H, W, arg, dtype, kw, want):
    kw = dict(kw)
    option = kw.pop("option", 0)
    monkeypatch.setenv("ALG_LOWPASS_PATH", str(option))
    assert route_of(lib, kind, 600, H, W, arg, dtype, **kw) == want
    assert expected_route(kind, 600, H, W, arg, dtype, option, **kw) == want


# ---- every case of tests/test_gpu_lowpass.py's test_bandwidth_shaped_kernels_are_bit_identical_to_the_plane_per_workgroup_kernels:
# that test compares the default route with ALG_LOWPASS_PATH=1, so a case that plans the plane-per-workgroup kernel by default
# compares the kernel with itself.  Its list, with the route each case takes by default: (shape, dtype, kind, arg, route)
BANDWIDTH_CASES = [
    ((1, 13, 16, 60, 90), BF16, "down_up", 0.25, BLOCKED),
    ((8, 13, 16, 60, 90), BF16, "down_up", 0.25, BLOCKED),
    ((8, 13, 16, 60, 90), F32, "down_up", 0.25, BLOCKED),
    ((1, 20, 21, 60, 104), F32, "down_up", 0.4, BLOCKED),
    ((3, 20, 21, 90, 160), F32, "down_up", 0.4, BLOCKED),
    ((2, 16, 1, 90, 160), F32, "down_up", 0.625, PLANE),             # 32 planes: its comment says "C4 first frame", one video frame
    ((1, 16, 3, 32, 32), F32, "down_up", 0.25, PLANE),               # 48 planes: "C1"
    ((2, 16, 1, 44, 76), BF16, "down_up", 0.8125, PLANE),            # 32 planes
    ((1, 20, 21, 60, 104), F32, "gaussian_blur", (9, 15.0), BLOCKED),
    ((8, 20, 21, 60, 104), F32, "gaussian_blur", (9, 7.5), BLOCKED),
    ((8, 13, 16, 60, 90), BF16, "gaussian_blur", (13, 3.0), BLOCKED),
    ((2, 20, 21, 90, 160), F32, "gaussian_blur", (19, 15.0), BLOCKED),
    ((8, 16, 13, 60, 88), BF16, "gaussian_blur", (5, 2.0), BLOCKED),
    ((4, 20, 21, 60, 104), F32, "gaussian_blur", (3, 1.0), BLOCKED),
    ((8, 16, 13, 32, 36), F32, "gaussian_blur", (15, 4.0), BLOCKED),
    ((8, 16, 13, 17, 20), BF16, "gaussian_blur", (7, 1.5), BLOCKED),
    ((8, 16, 13, 18, 24), F32, "gaussian_blur", (17, 9.0), BLOCKED),
    ((8, 16, 13, 30, 44), F32, "gaussian_blur", (11, 3.0), BLOCKED),
    ((8, 16, 13, 30, 46), F32, "gaussian_blur", (5, 1.2), BLOCKED),
    ((8, 16, 13, 34, 50), BF16, "gaussian_blur", (9, 2.5), BLOCKED),
    ((8, 16, 13, 60, 104), F32, "down_up", 0.25, BLOCKED),
    ((8, 16, 13, 44, 76), BF16, "down_up", 0.8125, BLOCKED),
    ((8, 16, 13, 90, 160), F32, "down_up", 0.625, BLOCKED),
    ((8, 16, 13, 30, 46), BF16, "down_up", 0.5, BLOCKED),
    ((8, 16, 13, 31, 44), F32, "down_up", 0.3, BLOCKED),
    ((8, 16, 13, 18, 22), F32, "down_up", 0.2, PERSISTENT),          # 22 -> 4: 13 taps along W, one more than blocked takes
    ((8, 16, 13, 60, 90), F32, "down_up", 0.34, BLOCKED),
]
# The cases that plan the plane-per-workgroup kernel by default.  The GPU test's own comments name them as the single-video /
# single-frame conditions ("C4 first frame", "C1", "a schedule-modulated factor on a bucketed size"): 32 or 48 planes, below the
# 128 a register-blocked launch needs.  For them the GPU comparison is the kernel with itself; the routes they would exercise
# are covered by the many-plane cases of the same shapes below them in the list.
PLANS_PLANE = [((2, 16, 1, 90, 160), F32, "down_up", 0.625), ((1, 16, 3, 32, 32), F32, "down_up", 0.25),
               ((2, 16, 1, 44, 76), BF16, "down_up", 0.8125)]


def _gpu_test_cases():
    """the GPU test's parameter list, read from its decorator (importing the module needs no GPU)"""
    import test_gpu_lowpass as t
    fn = t.test_bandwidth_shaped_kernels_are_bit_identical_to_the_plane_per_workgroup_kernels
    mark, = [m for m in fn.pytestmark if m.name == "parametrize"]
    return [(shape, BF16 if dt == torch.bfloat16 else F32, kind, arg) for shape, dt, kind, arg in mark.args[1]]


def test_the_list_below_is_the_gpu_tests_list():
    assert _gpu_test_cases() == [c[:4] for c in BANDWIDTH_CASES]
    assert [c[:4] for c in BANDWIDTH_CASES if c[4] == PLANE] == PLANS_PLANE


@pytest.mark.parametrize("shape,dtype,kind,arg,want", BANDWIDTH_CASES, ids=["%s %s %s %s" % (c[0], "f32" if c[1] == F32 else "bf16", c[2], c[3])
                                                                            for c in BANDWIDTH_CASES])
def test_default_route_of_the_bit_identity_cases(lib, monkeypatch, shape, dtype, kind, arg, want):
    monkeypatch.delenv("ALG_LOWPASS_PATH", raising=False)
    planes, (H, W) = int(np.prod(shape[:-2])), shape[-2:]
    if kind == "down_up":        # lp_utils.apply_low_pass_filter's target size
        kind, arg = "down_up", (max(1, int(round(H * arg))), max(1, int(round(W * arg))))
    else:
        kind, arg = "gaussian", arg[0]
    got = route_of(lib, kind, planes, H, W, arg, dtype)
    assert got == want == expected_route(kind, planes, H, W, arg, dtype)
    assert (got == PLANE) == (planes < 128)
    monkeypatch.setenv("ALG_LOWPASS_PATH", "1")                   # what the GPU test compares with
    assert route_of(lib, kind, planes, H, W, arg, dtype) == PLANE


# ---- the two workspace queries read the same plan: zero exactly when the route is not the global-memory passes
@pytest.mark.parametrize("option", range(5))
def test_workspace_queries_follow_the_plan(lib, monkeypatch, option):
    monkeypatch.setenv("ALG_LOWPASS_PATH", str(option))
    latent = option == 4
    assert lib.alg_down_up_workspace_bytes(576, 12, 16, 6, 8) == (4 * 576 * (12 * 8 + 6 * 8 + 6 * 16) if latent else 0)
    assert lib.alg_down_up_workspace_bytes(208, 60, 90, 15, 22) == (4 * 208 * (60 * 22 + 15 * 22 + 15 * 90) if latent else 0)
    assert lib.alg_gaussian_blur_workspace_bytes(576, 12, 16, 5) == (4 * (576 * 12 * 16 + 256) if latent else 0)
    assert lib.alg_gaussian_blur_workspace_bytes(420, 60, 104, 9) == (4 * (420 * 60 * 104 + 256) if latent else 0)
    # planes beyond the LDS, and more than 255 taps: whatever the option
    assert lib.alg_down_up_workspace_bytes(3, 480, 720, 120, 180) == PIXEL_BYTES
    assert lib.alg_down_up_workspace_bytes(1, 184, 160, 46, 40) == 4 * (184 * 40 + 46 * 40 + 46 * 160)
    assert lib.alg_down_up_workspace_bytes(1, 180, 160, 45, 40) == (4 * (180 * 40 + 45 * 40 + 45 * 160) if latent else 0)
    assert lib.alg_gaussian_blur_workspace_bytes(3, 480, 720, 9) == PIXEL_G_BYTES
    assert lib.alg_gaussian_blur_workspace_bytes(2, 129, 129, 257) == 4 * (2 * 129 * 129 + 512)
    assert lib.alg_gaussian_blur_workspace_bytes(2, 129, 129, 255) == (4 * (2 * 129 * 129 + 256) if latent else 0)
    assert lib.alg_gaussian_blur_workspace_bytes(1, 128, 160, 5) == 4 * (128 * 160 + 256)
    assert lib.alg_gaussian_blur_workspace_bytes(1, 127, 161, 19) == (4 * (127 * 161 + 256) if latent else 0)


def test_a_valid_call_with_the_default_option(lib, monkeypatch):
    monkeypatch.delenv("ALG_LOWPASS_PATH", raising=False)
    rc, text = run(lib, "down_up", 576, 12, 16, (6, 8))
    assert rc == ELAUNCH and text.startswith("alg_down_up (register-blocked kernel): hipFuncSetAttribute(163840 B LDS): "), text
    rc, text = run(lib, "gaussian", 3, 480, 720, 9)
    assert rc == ELAUNCH and text.startswith("alg_gaussian_blur (global-memory passes): launch failed: "), text
