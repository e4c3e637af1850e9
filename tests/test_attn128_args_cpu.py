"""The d = 128 attention's host path on a machine WITHOUT a GPU: every refusal of the eight entries with its exact text and its
place in the order of checks (attention128.hip: attn128_check; the dual and the e4m3 entry word their own), and the route a valid
call takes (attn128_plan) under ALG_ATTN128_Q64 and ALG_ATTN128_PIPE.

No operand is ever dereferenced: a refused call returns before any HIP call, and without a device a valid call ends at its first
HIP call -- the LDS opt-in of the 64-query or the pipelined kernel, whose message names the route, or the launch of the base
kernel.  The expected refusals were recorded from the library before check, plan and launch were separated; that part of the file
passes unchanged against that library (ALG_HIP_LIB).  The route part is what the separation made observable: before it a failed
opt-in sent the call on to the next kernel without a word.

With a GPU the file is skipped: a check lost by mistake would launch a kernel on host pointers."""
import ctypes

import pytest
import torch

import alg_amd

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")

EINVAL, ELAUNCH, ELIMIT = -1, -2, -3
_BUF = ctypes.create_string_buffer(2048)
P0 = (ctypes.addressof(_BUF) + 255) & ~255          # a 256-byte aligned host address
Q, K, VT, O, TAB, LSE, ORD, K2, VT2, QS, KS, VS = (P0 + 64 * i for i in range(12))

DENSE = "alg_flash_attn_d128"
BAD = "%s: bad argument (batch=%d heads=%d Sq=%d Skv=%d)"
ALIGN = "%s: q/k/vt need 16-byte aligned rows (strides %% 8 == 0), o 8-byte aligned"
PITCH = "%s: vt row stride %d must cover Skv rounded up to 64"
GROUP = "alg_flash_attn_d128_ex: heads=%d must be a multiple of kv_group=%d"
CAUSAL = "alg_flash_attn_d128_ex: causal attention needs Sq == Skv (got %d, %d)"
TABLE = "%s: kv_ranges must be a 4-byte aligned device table and max_ranges in 1..%d (got %s, %d)"
THEADS = "%s: table_heads must be 1 (one table for every head) or heads = %d, got %d"
LSE_ALIGN = "%s: lse must be 4-byte aligned (got %s)"
PREFIX_BUF = "%s: lse_prefix must be a 4-byte aligned device buffer [batch][heads][max_segments][Sq] (got %s)"
ORDER = ("%s: order must be a 4-byte aligned device int32[order_len] with order_len a multiple of 8 and at least "
         "batch * heads * q_blocks = %d (got %s, %d)")
LIMIT = "%s: operands beyond 31-bit byte offsets inside one (batch, head), or grid too large"
DUAL_BAD = "alg_flash_attn_d128_dual: bad argument (batch=%d heads=%d Sq=%d Skv=%d Skv2=%d)"
DUAL_PITCH = "alg_flash_attn_d128_dual: vt row strides %d / %d must cover Skv / Skv2 rounded up to 64"
FP8 = "alg_flash_attn_d128_fp8"
FP8_GROUP = FP8 + ": grouped-query (kv_group=%d) and causal (%d) attention are not covered: use alg_flash_attn_d128_ex"
FP8_ALIGN = FP8 + ": q/k/vt need 16-byte aligned rows (strides % 16 == 0), vt_scale 16-byte, o 8-byte aligned"
FP8_PITCH = FP8 + ": vt row stride %d must cover Skv = %d rounded up to 64"


def ptr(p):
    """printf's %p"""
    return "0x%x" % p if p else "(nil)"


@pytest.fixture(scope="module")
def lib():
    return alg_amd.load_library()


def base(**kw):
    """A valid call: 1 x 2 heads x 300 queries over Skv keys, packed [S][2 * 128] rows, V^T pitch Skv rounded up to 64"""
    Skv = kw.get("Skv", 700)
    pad = (Skv + 63) // 64 * 64
    a = dict(q=Q, k=K, vt=VT, o=O, batch=1, heads=2, Sq=300, Skv=Skv, q_bs=300 * 256, q_rs=256, k_bs=Skv * 256, k_rs=256,
             vt_bs=256 * pad, vt_rs=pad, o_bs=300 * 256, o_rs=256, kv_group=1, causal=0, table=TAB, max_ranges=2, table_heads=1,
             lse=None, order=ORD, order_len=16, lse_prefix=LSE)
    a.update(kw)
    return a


def _run(lib, fn, a, *tail):
    rc = getattr(lib, fn)(a["q"], a["k"], a["vt"], a["o"], a["batch"], a["heads"], a["Sq"], a["Skv"], a["q_bs"], a["q_rs"], a["k_bs"],
                          a["k_rs"], a["vt_bs"], a["vt_rs"], a["o_bs"], a["o_rs"], 0.0883883, *tail, None)
    return rc, lib.alg_last_error().decode()


def call(lib, entry, **kw):
    a = base(**kw)
    if entry == "plain":
        return _run(lib, "alg_flash_attn_d128", a)
    if entry == "ex":
        return _run(lib, "alg_flash_attn_d128_ex", a, a["kv_group"], a["causal"])
    if entry == "ranges":
        return _run(lib, "alg_flash_attn_d128_ranges", a, a["table"], a["max_ranges"])
    if entry == "heads":
        return _run(lib, "alg_flash_attn_d128_ranges_heads", a, a["table"], a["max_ranges"], a["table_heads"], a["lse"])
    if entry == "order":
        return _run(lib, "alg_flash_attn_d128_ranges_order", a, a["table"], a["max_ranges"], a["table_heads"], a["lse"], a["order"],
                    a["order_len"])
    if entry == "prefix":
        return _run(lib, "alg_flash_attn_d128_ranges_prefix", a, a["table"], a["max_ranges"], a["table_heads"], a["lse_prefix"])
    raise KeyError(entry)


def call_dual(lib, **kw):
    """the valid call with a second set of 257 keys at pitch 384"""
    a = base(Skv=512)
    a.update(k2=K2, vt2=VT2, Skv2=257, k2_bs=257 * 256, k2_rs=256, vt2_bs=256 * 384, vt2_rs=384)
    a.update(kw)
    rc = lib.alg_flash_attn_d128_dual(a["q"], a["k"], a["vt"], a["Skv"], a["k_bs"], a["k_rs"], a["vt_bs"], a["vt_rs"], a["k2"], a["vt2"],
                                      a["Skv2"], a["k2_bs"], a["k2_rs"], a["vt2_bs"], a["vt2_rs"], a["o"], a["batch"], a["heads"],
                                      a["Sq"], a["q_bs"], a["q_rs"], a["o_bs"], a["o_rs"], 0.0883883, None)
    return rc, lib.alg_last_error().decode()


def call_fp8(lib, **kw):
    a = base(q_scale=QS, k_scale=KS, vt_scale=VS)
    a.update(kw)
    rc = lib.alg_flash_attn_d128_fp8(a["q"], a["q_scale"], a["k"], a["k_scale"], a["vt"], a["vt_scale"], a["o"], a["batch"], a["heads"],
                                     a["Sq"], a["Skv"], a["q_bs"], a["q_rs"], a["k_bs"], a["k_rs"], a["vt_bs"], a["vt_rs"], a["o_bs"],
                                     a["o_rs"], 0.0883883, a["kv_group"], a["causal"], None)
    return rc, lib.alg_last_error().decode()


NAMES = {"plain": DENSE, "ex": DENSE, "ranges": DENSE + "_ranges", "heads": DENSE + "_ranges_heads", "order": DENSE + "_ranges_order",
         "prefix": DENSE + "_ranges_prefix"}

# ---- the refusals every bf16 entry with one key / value set shares: (id, arguments, text, what follows the entry's name in it)
SHARED = [
    ("null q", dict(q=None), BAD, (1, 2, 300, 700)),
    ("null k", dict(k=None), BAD, (1, 2, 300, 700)),
    ("null vt", dict(vt=None), BAD, (1, 2, 300, 700)),
    ("null o", dict(o=None), BAD, (1, 2, 300, 700)),
    ("batch = 0", dict(batch=0), BAD, (0, 2, 300, 700)),
    ("heads < 0", dict(heads=-2), BAD, (1, -2, 300, 700)),
    ("Sq = 0", dict(Sq=0), BAD, (1, 2, 0, 700)),
    ("q row stride % 8", dict(q_rs=260), ALIGN),
    ("q batch stride % 8", dict(q_bs=300 * 256 + 4), ALIGN),
    ("k row stride % 8", dict(k_rs=260), ALIGN),
    ("k batch stride % 8", dict(k_bs=700 * 256 + 4), ALIGN),
    ("vt row stride % 8", dict(vt_rs=708), ALIGN),
    ("vt batch stride % 8", dict(vt_bs=256 * 704 + 2), ALIGN),
    ("o row stride % 4", dict(o_rs=258), ALIGN),
    ("o batch stride % 4", dict(o_bs=300 * 256 + 2), ALIGN),
    ("q + 8 bytes", dict(q=Q + 8), ALIGN),
    ("k + 8 bytes", dict(k=K + 8), ALIGN),
    ("vt + 8 bytes", dict(vt=VT + 8), ALIGN),
    ("o + 4 bytes", dict(o=O + 4), ALIGN),
    ("vt pitch = Skv rounded to 8", dict(vt_rs=696), PITCH, (696,)),
    ("vt pitch one tile short", dict(Skv=705, k_bs=705 * 256, vt_rs=704, vt_bs=256 * 704), PITCH, (704,)),
    # order: the earlier refusal wins
    ("null before alignment", dict(o=None, q_rs=260, vt_rs=8), BAD, (1, 2, 300, 700)),
    ("size before pitch", dict(Sq=-5, vt_rs=8), BAD, (1, 2, -5, 700)),
    ("alignment before pitch", dict(q=Q + 8, vt_rs=8), ALIGN),
]
SHARED_CASES = [(e, r) for e in NAMES for r in SHARED]


@pytest.mark.parametrize("entry,case", SHARED_CASES, ids=["%s: %s" % (e, r[0]) for e, r in SHARED_CASES])
def test_shared_refusal(lib, entry, case):
    kw, text, args = case[1], case[2], case[3] if len(case) > 3 else ()
    assert call(lib, entry, **kw) == (EINVAL, text % ((NAMES[entry],) + args))


# ---- alg_flash_attn_d128_ex: its two refusals come first, under its own name
EX = [
    ("kv_group = 0", dict(kv_group=0), GROUP % (2, 0)),
    ("kv_group < 0", dict(kv_group=-1), GROUP % (2, -1)),
    ("kv_group no divisor", dict(heads=6, kv_group=4), GROUP % (6, 4)),
    ("causal, Sq != Skv", dict(causal=1), CAUSAL % (300, 700)),
    ("kv_group before causal", dict(kv_group=3, causal=1), GROUP % (2, 3)),
    ("kv_group before null", dict(kv_group=0, q=None), GROUP % (2, 0)),
    ("causal before null", dict(causal=1, k=None), CAUSAL % (300, 700)),
    ("causal before size", dict(causal=1, Sq=0), CAUSAL % (0, 700)),
    ("causal before pitch", dict(causal=1, vt_rs=8), CAUSAL % (300, 700)),
    ("grouped, then alignment", dict(kv_group=2, o=O + 4), ALIGN % DENSE),
    ("causal Sq = Skv, then pitch", dict(causal=1, Skv=300, k_bs=300 * 256, vt_rs=296, vt_bs=256 * 296), PITCH % (DENSE, 296)),
]


@pytest.mark.parametrize("name,kw,text", EX, ids=[r[0] for r in EX])
def test_ex_refusal(lib, name, kw, text):
    assert call(lib, "ex", **kw) == (EINVAL, text)


# ---- the ranged entries: table, table_heads, lse and lse_prefix between "bad argument" and the alignment; order last
def _ranged():
    rows = []
    for e, cap in (("ranges", 4), ("heads", 4), ("order", 4), ("prefix", 12)):
        n = NAMES[e]
        rows += [
            (e, "null table", dict(table=None), TABLE % (n, cap, ptr(0), 2)),
            (e, "table + 2 bytes", dict(table=TAB + 2), TABLE % (n, cap, ptr(TAB + 2), 2)),
            (e, "max_ranges = 0", dict(max_ranges=0), TABLE % (n, cap, ptr(TAB), 0)),
            (e, "max_ranges = cap + 1", dict(max_ranges=cap + 1), TABLE % (n, cap, ptr(TAB), cap + 1)),
            (e, "null before table", dict(q=None, table=None), BAD % (n, 1, 2, 300, 700)),
            (e, "table before alignment", dict(max_ranges=0, q_rs=260), TABLE % (n, cap, ptr(TAB), 0)),
        ]
    rows.append(("prefix", "max_ranges = 5 is a profile table", dict(max_ranges=5, vt_rs=8), PITCH % (NAMES["prefix"], 8)))
    for e in ("heads", "order", "prefix"):
        n = NAMES[e]
        rows += [
            (e, "table_heads = 0", dict(table_heads=0), THEADS % (n, 2, 0)),
            (e, "table_heads = 3", dict(table_heads=3), THEADS % (n, 2, 3)),
            (e, "table before table_heads", dict(table=None, table_heads=3), TABLE % (n, 12 if e == "prefix" else 4, ptr(0), 2)),
            (e, "table_heads = heads, then pitch", dict(table_heads=2, vt_rs=696), PITCH % (n, 696)),
        ]
    for e in ("heads", "order"):
        n = NAMES[e]
        rows += [
            (e, "lse + 2 bytes", dict(lse=LSE + 2), LSE_ALIGN % (n, ptr(LSE + 2))),
            (e, "table_heads before lse", dict(table_heads=5, lse=LSE + 2), THEADS % (n, 2, 5)),
            (e, "lse before alignment", dict(lse=LSE + 1, o=O + 4), LSE_ALIGN % (n, ptr(LSE + 1))),
            (e, "lse given, then alignment", dict(lse=LSE, o=O + 4), ALIGN % n),
        ]
    n = NAMES["prefix"]
    rows += [
        ("prefix", "null lse_prefix", dict(lse_prefix=None), PREFIX_BUF % (n, ptr(0))),
        ("prefix", "lse_prefix + 2 bytes", dict(lse_prefix=LSE + 2), PREFIX_BUF % (n, ptr(LSE + 2))),
        ("prefix", "table_heads before lse_prefix", dict(table_heads=3, lse_prefix=None), THEADS % (n, 2, 3)),
        ("prefix", "lse_prefix before alignment", dict(lse_prefix=None, k_rs=260), PREFIX_BUF % (n, ptr(0))),
    ]
    n = NAMES["order"]       # 1 x 2 heads x 2 blocks of 256 queries = 4 units
    rows += [
        ("order", "null order", dict(order=None), ORDER % (n, 4, ptr(0), 16)),
        ("order", "order + 2 bytes", dict(order=ORD + 2), ORDER % (n, 4, ptr(ORD + 2), 16)),
        ("order", "order_len = 0", dict(order_len=0), ORDER % (n, 4, ptr(ORD), 0)),
        ("order", "order_len % 8", dict(order_len=12), ORDER % (n, 4, ptr(ORD), 12)),
        ("order", "order_len < units", dict(Sq=1100, q_bs=1100 * 256, o_bs=1100 * 256, order_len=8), ORDER % (n, 10, ptr(ORD), 8)),
        ("order", "pitch before order", dict(order=None, vt_rs=696), PITCH % (n, 696)),
        ("order", "alignment before order", dict(order_len=12, vt_bs=256 * 704 + 2), ALIGN % n),
    ]
    return rows


RANGED = _ranged()


@pytest.mark.parametrize("entry,name,kw,text", RANGED, ids=["%s: %s" % (r[0], r[1]) for r in RANGED])
def test_ranged_refusal(lib, entry, name, kw, text):
    assert call(lib, entry, **kw) == (EINVAL, text)


# ---- the dual entry: its own texts, which name both sets
DUAL = [
    ("null q", dict(q=None), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("null k", dict(k=None), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("null vt", dict(vt=None), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("null k2", dict(k2=None), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("null vt2", dict(vt2=None), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("null o", dict(o=None), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("batch = 0", dict(batch=0), DUAL_BAD % (0, 2, 300, 512, 257)),
    ("heads = 0", dict(heads=0), DUAL_BAD % (1, 0, 300, 512, 257)),
    ("Sq < 0", dict(Sq=-1), DUAL_BAD % (1, 2, -1, 512, 257)),
    ("Skv = 0", dict(Skv=0), DUAL_BAD % (1, 2, 300, 0, 257)),
    ("Skv2 = 0", dict(Skv2=0), DUAL_BAD % (1, 2, 300, 512, 0)),
    ("q row stride % 8", dict(q_rs=260), ALIGN % (DENSE + "_dual")),
    ("q batch stride % 8", dict(q_bs=300 * 256 + 4), ALIGN % (DENSE + "_dual")),
    ("k row stride % 8", dict(k_rs=260), ALIGN % (DENSE + "_dual")),
    ("k batch stride % 8", dict(k_bs=512 * 256 + 4), ALIGN % (DENSE + "_dual")),
    ("vt row stride % 8", dict(vt_rs=516), ALIGN % (DENSE + "_dual")),
    ("vt batch stride % 8", dict(vt_bs=256 * 512 + 2), ALIGN % (DENSE + "_dual")),
    ("k2 row stride % 8", dict(k2_rs=260), ALIGN % (DENSE + "_dual")),
    ("k2 batch stride % 8", dict(k2_bs=257 * 256 + 4), ALIGN % (DENSE + "_dual")),
    ("vt2 row stride % 8", dict(vt2_rs=388), ALIGN % (DENSE + "_dual")),
    ("vt2 batch stride % 8", dict(vt2_bs=256 * 384 + 2), ALIGN % (DENSE + "_dual")),
    ("o row stride % 4", dict(o_rs=258), ALIGN % (DENSE + "_dual")),
    ("o batch stride % 4", dict(o_bs=300 * 256 + 2), ALIGN % (DENSE + "_dual")),
    ("q + 8 bytes", dict(q=Q + 8), ALIGN % (DENSE + "_dual")),
    ("k + 8 bytes", dict(k=K + 8), ALIGN % (DENSE + "_dual")),
    ("vt + 8 bytes", dict(vt=VT + 8), ALIGN % (DENSE + "_dual")),
    ("k2 + 8 bytes", dict(k2=K2 + 8), ALIGN % (DENSE + "_dual")),
    ("vt2 + 8 bytes", dict(vt2=VT2 + 8), ALIGN % (DENSE + "_dual")),
    ("o + 4 bytes", dict(o=O + 4), ALIGN % (DENSE + "_dual")),
    ("vt pitch one tile short", dict(vt_rs=448), DUAL_PITCH % (448, 384)),
    ("vt2 pitch one tile short", dict(vt2_rs=256), DUAL_PITCH % (512, 256)),
    ("null before alignment", dict(vt2=None, k2_rs=260), DUAL_BAD % (1, 2, 300, 512, 257)),
    ("alignment before pitch", dict(k2=K2 + 8, vt2_rs=256), ALIGN % (DENSE + "_dual")),
]


@pytest.mark.parametrize("name,kw,text", DUAL, ids=[r[0] for r in DUAL])
def test_dual_refusal(lib, name, kw, text):
    assert call_dual(lib, **kw) == (EINVAL, text)


# ---- the e4m3 entry: rows of bytes (strides % 16), three scale vectors, no grouped or causal form
FP8_CASES = [
    ("null q", dict(q=None), BAD % (FP8, 1, 2, 300, 700)),
    ("null k", dict(k=None), BAD % (FP8, 1, 2, 300, 700)),
    ("null vt", dict(vt=None), BAD % (FP8, 1, 2, 300, 700)),
    ("null o", dict(o=None), BAD % (FP8, 1, 2, 300, 700)),
    ("null q_scale", dict(q_scale=None), BAD % (FP8, 1, 2, 300, 700)),
    ("null k_scale", dict(k_scale=None), BAD % (FP8, 1, 2, 300, 700)),
    ("null vt_scale", dict(vt_scale=None), BAD % (FP8, 1, 2, 300, 700)),
    ("batch = 0", dict(batch=0), BAD % (FP8, 0, 2, 300, 700)),
    ("Skv = 0", dict(Skv=0), BAD % (FP8, 1, 2, 300, 0)),
    ("kv_group = 2", dict(kv_group=2), FP8_GROUP % (2, 0)),
    ("causal", dict(causal=1, Skv=300), FP8_GROUP % (1, 1)),
    ("q row stride % 16", dict(q_rs=264), FP8_ALIGN),
    ("q batch stride % 16", dict(q_bs=300 * 256 + 8), FP8_ALIGN),
    ("k row stride % 16", dict(k_rs=264), FP8_ALIGN),
    ("k batch stride % 16", dict(k_bs=700 * 256 + 8), FP8_ALIGN),
    ("vt row stride % 16", dict(vt_rs=712), FP8_ALIGN),
    ("vt batch stride % 16", dict(vt_bs=256 * 704 + 8), FP8_ALIGN),
    ("o row stride % 4", dict(o_rs=258), FP8_ALIGN),
    ("o batch stride % 4", dict(o_bs=300 * 256 + 2), FP8_ALIGN),
    ("q + 8 bytes", dict(q=Q + 8), FP8_ALIGN),
    ("k + 8 bytes", dict(k=K + 8), FP8_ALIGN),
    ("vt + 8 bytes", dict(vt=VT + 8), FP8_ALIGN),
    ("o + 4 bytes", dict(o=O + 4), FP8_ALIGN),
    ("vt_scale + 8 bytes", dict(vt_scale=VS + 8), FP8_ALIGN),
    ("q_scale + 2 bytes", dict(q_scale=QS + 2), FP8_ALIGN),
    ("k_scale + 2 bytes", dict(k_scale=KS + 2), FP8_ALIGN),
    ("vt pitch one tile short", dict(vt_rs=640), FP8_PITCH % (640, 700)),
    ("null before kv_group", dict(k_scale=None, kv_group=2), BAD % (FP8, 1, 2, 300, 700)),
    ("kv_group before alignment", dict(kv_group=2, q_rs=264), FP8_GROUP % (2, 0)),
    ("alignment before pitch", dict(q_rs=264, vt_rs=640), FP8_ALIGN),
]


@pytest.mark.parametrize("name,kw,text", FP8_CASES, ids=[r[0] for r in FP8_CASES])
def test_fp8_refusal(lib, name, kw, text):
    assert call_fp8(lib, **kw) == (EINVAL, text)


# ---- routes.  Without a device the first HIP call of a valid call fails, and which one it is names the kernel
OPT_IN = "%s: hipFuncSetAttribute(%d B LDS): "
Q64 = OPT_IN % ("alg_flash_attn_d128 (64-query kernel)", 131072)
PIPE = OPT_IN % ("alg_flash_attn_d128 (pipelined kernel)", 131072)
BASE = "alg_flash_attn_d128: launch failed: "


def route(Skv, q64, pipe, causal=0, kv_group=1, fits=True):
    """include/alg_hip.h, the ALG_ATTN128_* paragraph"""
    tiles = (Skv + 63) // 64
    if causal or kv_group != 1 or not fits:
        return BASE
    if q64 and tiles >= (64 if q64 == 1 else 8):
        return Q64
    if pipe and tiles >= 12:
        return PIPE
    return BASE


ROUTES = [(Skv, q64, pipe) for Skv in (4097, 4096, 4032, 768, 767, 704, 512, 449, 448)
          for q64, pipe in ((1, 1), (2, 1), (3, 1), (0, 1), (0, 0), (1, 0))]


def _options(monkeypatch, q64, pipe):
    monkeypatch.setenv("ALG_ATTN128_Q64", str(q64))
    monkeypatch.setenv("ALG_ATTN128_PIPE", str(pipe))     # (conftest: the library re-reads its options, now and when this is undone)


@pytest.mark.parametrize("Skv,q64,pipe", ROUTES, ids=["Skv=%d Q64=%d PIPE=%d" % r for r in ROUTES])
def test_route_of_a_dense_call(lib, monkeypatch, Skv, q64, pipe):
    _options(monkeypatch, q64, pipe)
    for entry in ("plain", "ex"):
        rc, text = call(lib, entry, Skv=Skv)
        assert rc == ELAUNCH and text.startswith(route(Skv, q64, pipe)), text


@pytest.mark.parametrize("q64,pipe", [(1, 1), (2, 1), (0, 1)])
def test_causal_grouped_and_wide_calls_run_the_base_kernel(lib, monkeypatch, q64, pipe):
    _options(monkeypatch, q64, pipe)
    wide = dict(Skv=4097, k_rs=262144, k_bs=4097 * 262144)        # (4,097 + 64) rows x 512 KiB: past 31-bit byte offsets
    for kw in (dict(causal=1, Skv=300), dict(kv_group=2, Skv=4097), dict(kv_group=2, Skv=768), wide):
        rc, text = call(lib, "ex", **kw)
        assert rc == ELAUNCH and text.startswith(BASE), (kw, text)
        assert route(kw["Skv"], q64, pipe, kw.get("causal", 0), kw.get("kv_group", 1), "k_rs" not in kw) == BASE


def test_default_options_are_q64_1_and_pipe_1(lib, monkeypatch):
    monkeypatch.delenv("ALG_ATTN128_Q64", raising=False)
    monkeypatch.delenv("ALG_ATTN128_PIPE", raising=False)
    for Skv in (4096, 4032, 768, 704):
        rc, text = call(lib, "plain", Skv=Skv)
        assert rc == ELAUNCH and text.startswith(route(Skv, 1, 1)), text


@pytest.mark.parametrize("entry", ["ranges", "heads", "order", "prefix"])
@pytest.mark.parametrize("q64", [1, 0, 3])
def test_ranged_entries_run_the_64_query_frame(lib, monkeypatch, entry, q64):
    """whatever the option says and however short the panel: a failed opt-in is a launch error under the entry's name, operands
    beyond the frame's 31-bit offsets are the limit error"""
    _options(monkeypatch, q64, 1)
    for Skv in (4097, 448, 64):
        rc, text = call(lib, entry, Skv=Skv)
        assert rc == ELAUNCH and text.startswith(OPT_IN % (NAMES[entry], 131072)), text
    assert call(lib, entry, Skv=4097, k_rs=262144, k_bs=4097 * 262144) == (ELIMIT, LIMIT % NAMES[entry])


def test_dual_entry_runs_the_base_kernel(lib):
    rc, text = call_dual(lib)
    assert rc == ELAUNCH and text.startswith("alg_flash_attn_d128_dual: launch failed: "), text
    rc, text = call_dual(lib, Skv=4097, k_bs=4097 * 256, vt_rs=4160, vt_bs=256 * 4160)      # long enough for the other two
    assert rc == ELAUNCH and text.startswith("alg_flash_attn_d128_dual: launch failed: "), text


def test_fp8_entry_opts_in_to_64_kib(lib):
    rc, text = call_fp8(lib)
    assert rc == ELAUNCH and text.startswith(OPT_IN % (FP8, 65536)), text
