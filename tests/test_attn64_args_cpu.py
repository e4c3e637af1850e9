"""The d = 64 attention's host path on a machine WITHOUT a GPU: the three refusals of the argument check with their exact texts
and their order, and the launch plan (attention.hip: attn64_plan) as alg_flash_attn_d64_workspace_bytes reports it -- which
shapes get a split-KV tail, with how many units and chunks, under ALG_ATTN_SPLIT_TAIL, ALG_ATTN_VARIANT and the pre-scaled flag.

No operand is ever dereferenced: a refused call returns before any HIP call, and the workspace query is pure.  The expected
values were recorded from the library before check, plan and launch were separated; the file passes unchanged against that
library (ALG_HIP_LIB).

With a GPU the file is skipped: a check lost by mistake would launch a kernel on host pointers."""
import ctypes

import pytest
import torch

import alg_amd
from alg_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")

EINVAL = -1
_BUF = ctypes.create_string_buffer(1024)
P = (ctypes.addressof(_BUF) + 255) & ~255          # a 256-byte aligned host address
Q, K, VT, O, WS = (P + 64 * i for i in range(5))

BAD = "alg_flash_attn_d64: bad argument (batch=%d heads=%d S=%d)"
ALIGN = "alg_flash_attn_d64: q/k/vt need 16-byte aligned rows (strides % 8 == 0), o 8-byte aligned"
PITCH = "alg_flash_attn_d64: vt row stride %d must cover S rounded up to 64"
PRESCALED = _lib.ATTN_Q_PRESCALED


@pytest.fixture(scope="module")
def lib():
    return alg_amd.load_library()


def call(lib, **kw):
    """alg_flash_attn_d64_ex on a valid call (2 x 4 heads x 300 tokens, packed [S][heads * 64] rows, V^T pitch 320) with kw on top"""
    a = dict(q=Q, k=K, vt=VT, o=O, batch=2, heads=4, S=300, q_bs=300 * 256, q_rs=256, vt_bs=256 * 320, vt_rs=320, o_bs=300 * 256,
             o_rs=256, flags=0, ws=None, ws_bytes=0)
    a.update(kw)
    rc = lib.alg_flash_attn_d64_ex(a["q"], a["k"], a["vt"], a["o"], a["batch"], a["heads"], a["S"], a["q_bs"], a["q_rs"], a["vt_bs"],
                                   a["vt_rs"], a["o_bs"], a["o_rs"], 0.125, a["flags"], a["ws"], a["ws_bytes"], None)
    return rc, lib.alg_last_error().decode()


REFUSALS = [
    # ---- the three refusals, in the order the check runs them
    ("null q", dict(q=None), BAD % (2, 4, 300)),
    ("null k", dict(k=None), BAD % (2, 4, 300)),
    ("null vt", dict(vt=None), BAD % (2, 4, 300)),
    ("null o", dict(o=None), BAD % (2, 4, 300)),
    ("batch = 0", dict(batch=0), BAD % (0, 4, 300)),
    ("heads < 0", dict(heads=-3), BAD % (2, -3, 300)),
    ("S = 0", dict(S=0), BAD % (2, 4, 0)),
    ("q row stride % 8", dict(q_rs=260), ALIGN),
    ("q batch stride % 8", dict(q_bs=300 * 256 + 4), ALIGN),
    ("vt row stride % 8", dict(vt_rs=324), ALIGN),
    ("vt batch stride % 8", dict(vt_bs=256 * 320 + 2), ALIGN),
    ("o row stride % 4", dict(o_rs=258), ALIGN),
    ("o batch stride % 4", dict(o_bs=300 * 256 + 2), ALIGN),
    ("q + 8 bytes", dict(q=Q + 8), ALIGN),
    ("k + 8 bytes", dict(k=K + 8), ALIGN),
    ("vt + 8 bytes", dict(vt=VT + 8), ALIGN),
    ("o + 4 bytes", dict(o=O + 4), ALIGN),
    ("vt pitch = S", dict(vt_rs=304), PITCH % 304),
    ("vt pitch one tile short", dict(S=321, vt_rs=320), PITCH % 320),
    # ---- order: the earlier refusal wins
    ("null before alignment", dict(o=None, q_rs=260, vt_rs=8), BAD % (2, 4, 300)),
    ("size before pitch", dict(S=-5, vt_rs=8), BAD % (2, 4, -5)),
    ("alignment before pitch", dict(q=Q + 8, vt_rs=8), ALIGN),
    # ---- flags and workspace do not move the check
    ("pre-scaled, null q", dict(q=None, flags=PRESCALED, ws=WS, ws_bytes=1 << 20), BAD % (2, 4, 300)),
    ("pre-scaled, pitch", dict(vt_rs=256, flags=PRESCALED), PITCH % 256),
]


@pytest.mark.parametrize("name,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(lib, name, kw, text):
    assert call(lib, **kw) == (EINVAL, text)


def test_plain_entry_runs_the_same_check(lib):
    rc = lib.alg_flash_attn_d64(Q, K, VT, O + 4, 2, 4, 300, 300 * 256, 256, 256 * 320, 320, 300 * 256, 256, 0.125, None)
    assert (rc, lib.alg_last_error().decode()) == (EINVAL, ALIGN)
    rc = lib.alg_flash_attn_d64(Q, K, VT, O, 2, 4, 300, 300 * 256, 256, 256 * 320, 256, 300 * 256, 256, 0.125, None)
    assert (rc, lib.alg_last_error().decode()) == (EINVAL, PITCH % 256)


def plan_tail(batch, heads, S):
    """attention.hip's plan_tail with ALG_ATTN_SPLIT_TAIL on: (units, split, tiles) or None.  Every XCD runs 64 workgroups at a
    time; when its last round of 256-query units is at most a quarter full, those units are cut along KV into `split` chunks."""
    nbh, q_blocks, n_tiles = batch * heads, (S + 255) // 256, (S + 63) // 64
    if nbh % 8:
        return None
    per_xcd = nbh // 8 * q_blocks
    r = per_xcd % 64
    if per_xcd < 64 or r == 0 or r > 16 or n_tiles < 64:
        return None
    split = 8 if (r * 8) % 64 == 0 else 16
    return r, split, (n_tiles + split - 1) // split


def tail_bytes(plan):
    """[8 XCDs * units][split][256 rows] x (64 O values + running max + row sum) fp32"""
    return 0 if plan is None else 8 * plan[0] * plan[1] * 256 * 66 * 4


SHAPES = [
    # (batch, heads, S), the plan: (units, split, tiles) or None
    ((2, 48, 17776), (8, 8, 35)),      # the north-star launch: 840 units per XCD = 13 rounds + 8
    ((2, 8, 17776), (12, 16, 18)),
    ((1, 40, 4090), (16, 8, 8)),       # the smallest tail: exactly 64 KV tiles, ragged
    ((1, 8, 16600), (1, 16, 17)),
    ((8, 1, 1200), None),              # 5 units per XCD, 19 KV tiles
    ((1, 7, 17776), None),             # heads spread unevenly over the XCDs
    ((1, 40, 4032), None),             # 63 KV tiles
    ((1, 8, 20500), None),             # last round 17 units: more than a quarter full
    ((1, 64, 2048), None),             # 64 units per XCD: no last round
    ((1, 8, 16128), None),             # 63 units per XCD: less than one round
]
# (id, environment, flags, does the tail plan apply)
SETTINGS = [
    ("default", {}, 0, True),
    ("split tail off", {"ALG_ATTN_SPLIT_TAIL": "0"}, 0, False),
    ("exact variant", {"ALG_ATTN_VARIANT": "1"}, 0, False),
    ("prescaled", {}, PRESCALED, True),
]
PLAN_CASES = [(shape, plan, s) for shape, plan in SHAPES[:6] for s in SETTINGS] + \
             [(shape, plan, SETTINGS[0]) for shape, plan in SHAPES[6:]] + \
             [(SHAPES[0][0], SHAPES[0][1], ("exact variant, prescaled", {"ALG_ATTN_VARIANT": "1"}, PRESCALED, True)),
              (SHAPES[0][0], SHAPES[0][1], ("split tail off, prescaled", {"ALG_ATTN_SPLIT_TAIL": "0"}, PRESCALED, False)),
              (SHAPES[2][0], SHAPES[2][1], ("variant 33", {"ALG_ATTN_VARIANT": "33"}, 0, True))]


@pytest.mark.parametrize("shape,plan,setting", PLAN_CASES, ids=["%dx%dx%d %s" % (*c[0], c[2][0]) for c in PLAN_CASES])
def test_workspace_bytes_follow_the_plan(lib, monkeypatch, shape, plan, setting):
    _, env, flags, tail = setting
    for name in ("ALG_ATTN_SPLIT_TAIL", "ALG_ATTN_VARIANT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)     # (conftest: the library re-reads its options, now and when this is undone)
    assert plan_tail(*shape) == plan
    assert lib.alg_flash_attn_d64_workspace_bytes(*shape, flags) == (tail_bytes(plan) if tail else 0)


def test_workspace_bytes_of_an_empty_problem(lib):
    for shape in ((0, 48, 17776), (2, 0, 17776), (2, 48, 0), (-2, 48, 17776)):
        assert lib.alg_flash_attn_d64_workspace_bytes(*shape, 0) == 0
        assert lib.alg_flash_attn_d64_workspace_bytes(*shape, PRESCALED) == 0
