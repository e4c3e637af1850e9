"""The host path of the eleven row-norm entries (rownorm_host.h; norm.hip: alg_layernorm_modulate, _seg, _fp8, _seg_fp8 and
alg_qk_norm_rope_scaled; wan.hip: alg_layernorm_mod_f32, _fp8, alg_rmsnorm_rope, _fp8; hunyuan.hip: alg_headnorm_rope, _fp8) on a
machine WITHOUT a GPU: every refusal with its return code, exact text and place in the order of checks, and the route a valid
LayerNorm call of either family is planned on.

No operand is ever dereferenced: a refused call returns before any HIP call, and without a device a valid call ends at its
launch, whose message names the entry and -- for the LayerNorm entries -- the route.  Part one (REFUSALS, EMPTY) was recorded from
the library before the change and passes unchanged against it (ALG_HIP_LIB); LIMITS is new: those calls used to launch a grid
truncated to 32 bits (alg_layernorm_modulate_fp8 / _seg_fp8 refused it before, with ALG_EINVAL: in REFUSALS).  Part two (routes)
is what the change made observable.  Without a device the library sizes for 256 CUs.

With a GPU the file is skipped: a check lost by mistake would launch a kernel on host pointers."""
import ctypes

import pytest
import torch

import alg_amd

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")

OK, EINVAL, ELAUNCH, ELIMIT = 0, -1, -2, -3
_BUF = ctypes.create_string_buffer(4096)
P0 = (ctypes.addressof(_BUF) + 255) & ~255
X, Y, Q8, QS, W, B, SC, SH, COS, SIN, HS = (P0 + 256 * i for i in range(11))


@pytest.fixture(scope="module")
def lib():
    return alg_amd.load_library()


def _err(lib, rc):
    return rc, lib.alg_last_error().decode()


def ln(lib, fp8=False, **kw):
    """alg_layernorm_mod_f32(_fp8): 2 x 8 rows of 1024, the modulated form"""
    a = dict(x=X, y=Y, q8=Q8, qs=QS, w=None, b=None, sc=SC, sh=SH, mod=1024, batch=2, rows=8, D=1024)
    a.update(kw)
    if fp8:
        return _err(lib, lib.alg_layernorm_mod_f32_fp8(a["x"], a["q8"], a["qs"], a["w"], a["b"], a["sc"], a["sh"], a["mod"], a["batch"],
                                                       a["rows"], a["D"], 1e-6, None))
    return _err(lib, lib.alg_layernorm_mod_f32(a["x"], a["y"], a["w"], a["b"], a["sc"], a["sh"], a["mod"], a["batch"], a["rows"], a["D"],
                                               1e-6, None))


def rms(lib, fp8=False, **kw):
    """alg_rmsnorm_rope(_fp8): 2 x 8 rows of 1024 with tables"""
    a = dict(x=X, w=W, cos=COS, sin=SIN, xrs=1024, batch=2, rows=8, D=1024, q8=Q8, q8rs=1024, scale=QS, hs=None)
    a.update(kw)
    if fp8:
        return _err(lib, lib.alg_rmsnorm_rope_fp8(a["x"], a["w"], a["cos"], a["sin"], a["xrs"], a["batch"], a["rows"], a["D"], 1e-6, a["q8"],
                                                  a["q8rs"], a["scale"], a["hs"], None))
    return _err(lib, lib.alg_rmsnorm_rope(a["x"], a["w"], a["cos"], a["sin"], a["xrs"], a["batch"], a["rows"], a["D"], 1e-6, None))


def head(lib, fp8=False, **kw):
    """alg_headnorm_rope(_fp8): 2 x 8 rows of 4 heads"""
    a = dict(x=X, w=W, cos=COS, sin=SIN, xrs=512, xbs=4096, batch=2, rows=8, heads=4, rope=8, q8=Q8, q8rs=512, q8bs=4096, scale=QS,
             sbs=32, hs=None)
    a.update(kw)
    if fp8:
        return _err(lib, lib.alg_headnorm_rope_fp8(a["x"], a["w"], a["cos"], a["sin"], a["xrs"], a["xbs"], a["batch"], a["rows"], a["heads"],
                                                   a["rope"], 1e-6, a["q8"], a["q8rs"], a["q8bs"], a["scale"], a["sbs"], a["hs"], None))
    return _err(lib, lib.alg_headnorm_rope(a["x"], a["w"], a["cos"], a["sin"], a["xrs"], a["xbs"], a["batch"], a["rows"], a["heads"],
                                           a["rope"], 1e-6, None))


def lnb(lib, fp8=False, seg=False, **kw):
    """alg_layernorm_modulate(_seg)(_fp8): 2 x 8 rows of 1024, all four bf16 parameter rows"""
    a = dict(x=X, y=Y, q8=Q8, qs=QS, w=W, b=B, sc=SC, sh=SH, mod=1024, segs=1024, batch=2, rows=8, D=1024, xbs=8192, ybs=8192, split=4)
    a.update(kw)
    head_, tail = (a["x"], a["q8"], a["qs"]) if fp8 else (a["x"], a["y"]), (a["batch"], a["rows"], a["D"], a["xbs"])
    prm = (a["w"], a["b"], a["sc"], a["sh"], a["mod"]) + ((a["segs"],) if seg else ())
    tail += (() if fp8 else (a["ybs"],)) + (a["split"], 1e-5, None)
    fn = getattr(lib, "alg_layernorm_modulate" + ("_seg" if seg else "") + ("_fp8" if fp8 else ""))
    return _err(lib, fn(*head_, *prm, *tail))


def qk(lib, fp8=False, **kw):
    """alg_qk_norm_rope_scaled: 2 x 8 tokens of 4 heads (the per-vector kernel; 16 heads: one wave per token)"""
    a = dict(qk=X, wq=W, bq=B, wk=SC, bk=SH, cos=COS, sin=SIN, batch=2, S=8, heads=4, text=2)
    a.update(kw)
    return _err(lib, lib.alg_qk_norm_rope_scaled(a["qk"], a["wq"], a["bq"], a["wk"], a["bk"], a["cos"], a["sin"], a["batch"], a["S"],
                                                 a["heads"], a["text"], 1e-6, 0.18, None))


def lnb_seg(lib, fp8=False, **kw):
    return lnb(lib, fp8, True, **kw)


LNB, LNB8, QK = "alg_layernorm_modulate", "alg_layernorm_modulate_fp8", "alg_qk_norm_rope"     # the names the messages carry
LNB_BAD = "%s: bad argument (batch=%d rows=%d D=%d)"
LNB_D = "%s: D=%d must be a multiple of 512 and <= 8192"
LNB_PAIR = "%s: scale and shift must be given together"
LNB_ALIGN = LNB + ": pointers must be 16-byte aligned"
LNB8_ALIGN = LNB8 + ": x and the parameter rows must be 16-byte aligned, q8 8-byte aligned"
QK_BAD = QK + ": bad argument (batch=%d S=%d heads=%d text_len=%d)"
QK_PAIR = QK + ": cos and sin tables must be given together"
QK_ALIGN = QK + ": pointers must be 16-byte aligned"
LN, LN8 = "alg_layernorm_mod_f32", "alg_layernorm_mod_f32_fp8"
RMS, RMS8 = "alg_rmsnorm_rope", "alg_rmsnorm_rope_fp8"
HD, HD8 = "alg_headnorm_rope", "alg_headnorm_rope_fp8"
LN_SHAPE = "%s: bad shape batch=%d rows=%d D=%d"
NULL = "%s: null pointer"
LN_WIDTH = LN8 + ": the fp8 output needs D %% 512 == 0 and D <= 6144 (D=%d)"
RMS_SHAPE = RMS + ": bad shape batch=%d rows=%d D=%d stride=%d"
RMS8_SHAPE = RMS8 + ": bad shape batch=%d rows=%d D=%d strides=%d / %d"
HD_SHAPE = HD + ": bad shape batch=%d rows=%d heads=%d stride=%d"
HD8_SHAPE = HD8 + ": bad shape batch=%d rows=%d heads=%d strides=%d / %d"
PTR8 = "%s: null or misaligned pointer (x 16-byte, q8 8-byte; scale or head_scale is needed)"
NOT_BUILT = "%s: D=%d is not built (D/512 in {1,2,3,4,6,8,10,12})"

# ---- part one: (id, call, fp8, arguments, return code, text), in the order of the checks; "x before y": the earlier refusal wins
REFUSALS = [
    # the bf16-parameter LayerNorm family: the plain entries forward to the _seg ones with seg_stride = D
    ("lnb null x", lnb, False, dict(x=None), EINVAL, LNB_BAD % (LNB, 2, 8, 1024)),
    ("lnb null y", lnb, False, dict(y=None), EINVAL, LNB_BAD % (LNB, 2, 8, 1024)),
    ("lnb batch = 0", lnb, False, dict(batch=0), EINVAL, LNB_BAD % (LNB, 0, 8, 1024)),
    ("lnb rows < 0", lnb, False, dict(rows=-8), EINVAL, LNB_BAD % (LNB, 2, -8, 1024)),
    ("lnb D = 0", lnb, False, dict(D=0), EINVAL, LNB_BAD % (LNB, 2, 8, 0)),
    ("lnb D = 1028: seg_stride % 8 first", lnb, False, dict(D=1028), EINVAL, LNB_BAD % (LNB, 2, 8, 1028)),
    ("lnb D = 1280", lnb, False, dict(D=1280), EINVAL, LNB_D % (LNB, 1280)),
    ("lnb D = 8704", lnb, False, dict(D=8704), EINVAL, LNB_D % (LNB, 8704)),
    ("lnb scale without shift", lnb, False, dict(sh=None), EINVAL, LNB_PAIR % LNB),
    ("lnb shift without scale", lnb, False, dict(sc=None), EINVAL, LNB_PAIR % LNB),
    ("lnb x + 8 bytes", lnb, False, dict(x=X + 8), EINVAL, LNB_ALIGN),
    ("lnb y + 8 bytes", lnb, False, dict(y=Y + 8), EINVAL, LNB_ALIGN),
    ("lnb weight + 2 bytes", lnb, False, dict(w=W + 2), EINVAL, LNB_ALIGN),
    ("lnb bias + 4 bytes", lnb, False, dict(b=B + 4), EINVAL, LNB_ALIGN),
    ("lnb scale + 8 bytes", lnb, False, dict(sc=SC + 8), EINVAL, LNB_ALIGN),
    ("lnb shift + 8 bytes", lnb, False, dict(sh=SH + 8), EINVAL, LNB_ALIGN),
    ("lnb mod_bstride % 8", lnb, False, dict(mod=1028), EINVAL, LNB_ALIGN),
    ("lnb x_bstride % 8", lnb, False, dict(xbs=8196), EINVAL, LNB_ALIGN),
    ("lnb y_bstride % 8", lnb, False, dict(ybs=8196), EINVAL, LNB_ALIGN),
    ("lnb null before D", lnb, False, dict(x=None, D=1280), EINVAL, LNB_BAD % (LNB, 2, 8, 1280)),
    ("lnb D before pair", lnb, False, dict(D=1280, sh=None), EINVAL, LNB_D % (LNB, 1280)),
    ("lnb pair before alignment", lnb, False, dict(sh=None, x=X + 8), EINVAL, LNB_PAIR % LNB),
    ("lnb_seg seg_stride % 8", lnb_seg, False, dict(segs=1028), EINVAL, LNB_BAD % (LNB, 2, 8, 1024)),
    ("lnb_seg null y", lnb_seg, False, dict(y=None), EINVAL, LNB_BAD % (LNB, 2, 8, 1024)),
    ("lnb_seg D = 1280", lnb_seg, False, dict(D=1280), EINVAL, LNB_D % (LNB, 1280)),
    ("lnb_seg scale without shift", lnb_seg, False, dict(sh=None), EINVAL, LNB_PAIR % LNB),
    ("lnb_seg y + 8 bytes", lnb_seg, False, dict(y=Y + 8), EINVAL, LNB_ALIGN),
    ("lnb8 null q8", lnb, True, dict(q8=None), EINVAL, LNB_BAD % (LNB8, 2, 8, 1024)),
    ("lnb8 null q8_scale", lnb, True, dict(qs=None), EINVAL, LNB_BAD % (LNB8, 2, 8, 1024)),
    ("lnb8 rows = 0", lnb, True, dict(rows=0), EINVAL, LNB_BAD % (LNB8, 2, 0, 1024)),
    ("lnb8 D = 8704", lnb, True, dict(D=8704), EINVAL, LNB_D % (LNB8, 8704)),
    ("lnb8 shift without scale", lnb, True, dict(sc=None), EINVAL, LNB_PAIR % LNB8),
    ("lnb8 x + 8 bytes", lnb, True, dict(x=X + 8), EINVAL, LNB8_ALIGN),
    ("lnb8 q8 + 4 bytes", lnb, True, dict(q8=Q8 + 4), EINVAL, LNB8_ALIGN),
    ("lnb8 q8_scale + 2 bytes", lnb, True, dict(qs=QS + 2), EINVAL, LNB8_ALIGN),
    ("lnb8 bias + 8 bytes", lnb, True, dict(b=B + 8), EINVAL, LNB8_ALIGN),
    ("lnb8 mod_bstride % 8", lnb, True, dict(mod=1028), EINVAL, LNB8_ALIGN),
    ("lnb8 x_bstride % 8", lnb, True, dict(xbs=8196), EINVAL, LNB8_ALIGN),
    ("lnb8 2^33 rows", lnb, True, dict(batch=1 << 17, rows=1 << 16), EINVAL,
     "%s: batch * rows = %d is more than one launch covers" % (LNB8, 1 << 33)),
    ("lnb8 alignment before the limit", lnb, True, dict(batch=1 << 17, rows=1 << 16, q8=Q8 + 4), EINVAL, LNB8_ALIGN),
    ("lnb8_seg seg_stride % 8", lnb_seg, True, dict(segs=1028), EINVAL, LNB_BAD % (LNB8, 2, 8, 1024)),
    ("lnb8_seg null q8", lnb_seg, True, dict(q8=None), EINVAL, LNB_BAD % (LNB8, 2, 8, 1024)),
    ("lnb8_seg D = 1280", lnb_seg, True, dict(D=1280), EINVAL, LNB_D % (LNB8, 1280)),
    ("lnb8_seg q8 + 4 bytes", lnb_seg, True, dict(q8=Q8 + 4), EINVAL, LNB8_ALIGN),
    ("lnb8_seg 2^33 rows", lnb_seg, True, dict(batch=1 << 17, rows=1 << 16), EINVAL,
     "%s: batch * rows = %d is more than one launch covers" % (LNB8, 1 << 33)),
    # alg_qk_norm_rope_scaled
    ("qk null qk", qk, False, dict(qk=None), EINVAL, QK_BAD % (2, 8, 4, 2)),
    ("qk null bk", qk, False, dict(bk=None), EINVAL, QK_BAD % (2, 8, 4, 2)),
    ("qk batch = 0", qk, False, dict(batch=0), EINVAL, QK_BAD % (0, 8, 4, 2)),
    ("qk S < 0", qk, False, dict(S=-8), EINVAL, QK_BAD % (2, -8, 4, 2)),
    ("qk heads = 0", qk, False, dict(heads=0), EINVAL, QK_BAD % (2, 8, 0, 2)),
    ("qk text_len < 0", qk, False, dict(text=-1), EINVAL, QK_BAD % (2, 8, 4, -1)),
    ("qk cos without sin", qk, False, dict(sin=None), EINVAL, QK_PAIR),
    ("qk sin without cos", qk, False, dict(cos=None), EINVAL, QK_PAIR),
    ("qk qk + 8 bytes", qk, False, dict(qk=X + 8), EINVAL, QK_ALIGN),
    ("qk wk + 2 bytes", qk, False, dict(wk=SC + 2), EINVAL, QK_ALIGN),
    ("qk cos + 4 bytes", qk, False, dict(cos=COS + 4), EINVAL, QK_ALIGN),
    ("qk null before tables", qk, False, dict(wq=None, sin=None), EINVAL, QK_BAD % (2, 8, 4, 2)),
    ("qk tables before alignment", qk, False, dict(sin=None, qk=X + 8), EINVAL, QK_PAIR),
    # the fp32-parameter LayerNorm family, RMSNorm + rope, per-head RMSNorm + rope
    ("ln batch < 0", ln, False, dict(batch=-1), EINVAL, LN_SHAPE % (LN, -1, 8, 1024)),
    ("ln rows < 0", ln, False, dict(rows=-8), EINVAL, LN_SHAPE % (LN, 2, -8, 1024)),
    ("ln D = 0", ln, False, dict(D=0), EINVAL, LN_SHAPE % (LN, 2, 8, 0)),
    ("ln null x", ln, False, dict(x=None), EINVAL, NULL % LN),
    ("ln null y", ln, False, dict(y=None), EINVAL, NULL % LN),
    ("ln shape before null", ln, False, dict(x=None, D=-4), EINVAL, LN_SHAPE % (LN, 2, 8, -4)),
    ("ln8 D < 0", ln, True, dict(D=-1), EINVAL, LN_SHAPE % (LN8, 2, 8, -1)),
    ("ln8 null x", ln, True, dict(x=None), EINVAL, NULL % LN8),
    ("ln8 null q8", ln, True, dict(q8=None), EINVAL, NULL % LN8),
    ("ln8 null q8_scale", ln, True, dict(qs=None), EINVAL, NULL % LN8),
    ("ln8 D = 1280", ln, True, dict(D=1280), EINVAL, LN_WIDTH % 1280),
    ("ln8 D = 5 x 512", ln, True, dict(D=2560), EINVAL, LN_WIDTH % 2560),
    ("ln8 D = 6656", ln, True, dict(D=6656), EINVAL, LN_WIDTH % 6656),
    ("ln8 null before width", ln, True, dict(D=1280, qs=None), EINVAL, NULL % LN8),
    ("rms batch < 0", rms, False, dict(batch=-2), EINVAL, RMS_SHAPE % (-2, 8, 1024, 1024)),
    ("rms D = 0", rms, False, dict(D=0), EINVAL, RMS_SHAPE % (2, 8, 0, 1024)),
    ("rms D = 1280", rms, False, dict(D=1280), EINVAL, RMS_SHAPE % (2, 8, 1280, 1024)),
    ("rms stride % 8", rms, False, dict(xrs=1028), EINVAL, RMS_SHAPE % (2, 8, 1024, 1028)),
    ("rms cos without sin", rms, False, dict(sin=None), EINVAL, RMS_SHAPE % (2, 8, 1024, 1024)),
    ("rms null x", rms, False, dict(x=None), EINVAL, NULL % RMS),
    ("rms null weight", rms, False, dict(w=None), EINVAL, NULL % RMS),
    ("rms shape before null", rms, False, dict(x=None, rows=-1), EINVAL, RMS_SHAPE % (2, -1, 1024, 1024)),
    ("rms D = 5 x 512", rms, False, dict(D=2560, xrs=2560), ELIMIT, NOT_BUILT % (RMS, 2560)),
    ("rms null before width", rms, False, dict(D=2560, xrs=2560, w=None), EINVAL, NULL % RMS),
    ("rms8 q8 stride % 8", rms, True, dict(q8rs=1028), EINVAL, RMS8_SHAPE % (2, 8, 1024, 1024, 1028)),
    ("rms8 q8 stride < D", rms, True, dict(q8rs=512), EINVAL, RMS8_SHAPE % (2, 8, 1024, 1024, 512)),
    ("rms8 rows < 0", rms, True, dict(rows=-8), EINVAL, RMS8_SHAPE % (2, -8, 1024, 1024, 1024)),
    ("rms8 null q8", rms, True, dict(q8=None), EINVAL, PTR8 % RMS8),
    ("rms8 neither scale", rms, True, dict(scale=None), EINVAL, PTR8 % RMS8),
    ("rms8 x + 8 bytes", rms, True, dict(x=X + 8), EINVAL, PTR8 % RMS8),
    ("rms8 q8 + 4 bytes", rms, True, dict(q8=Q8 + 4), EINVAL, PTR8 % RMS8),
    ("rms8 D = 7 x 512", rms, True, dict(D=3584, xrs=3584, q8rs=3584), ELIMIT, NOT_BUILT % (RMS8, 3584)),
    ("head heads = 0", head, False, dict(heads=0), EINVAL, HD_SHAPE % (2, 8, 0, 512)),
    ("head row stride % 8", head, False, dict(xrs=516), EINVAL, HD_SHAPE % (2, 8, 4, 516)),
    ("head batch stride % 8", head, False, dict(xbs=4100), EINVAL, HD_SHAPE % (2, 8, 4, 512)),
    ("head row stride < heads x 128", head, False, dict(xrs=504), EINVAL, HD_SHAPE % (2, 8, 4, 504)),
    ("head cos without sin", head, False, dict(sin=None), EINVAL, HD_SHAPE % (2, 8, 4, 512)),
    ("head null x", head, False, dict(x=None), EINVAL, NULL % HD),
    ("head null weight", head, False, dict(w=None), EINVAL, NULL % HD),
    ("head shape before null", head, False, dict(w=None, batch=-1), EINVAL, HD_SHAPE % (-1, 8, 4, 512)),
    ("head8 q8 row stride % 8", head, True, dict(q8rs=516), EINVAL, HD8_SHAPE % (2, 8, 4, 512, 516)),
    ("head8 q8 batch stride % 8", head, True, dict(q8bs=4100), EINVAL, HD8_SHAPE % (2, 8, 4, 512, 512)),
    ("head8 q8 row stride < heads x 128", head, True, dict(q8rs=256), EINVAL, HD8_SHAPE % (2, 8, 4, 512, 256)),
    ("head8 null x", head, True, dict(x=None), EINVAL, PTR8 % HD8),
    ("head8 neither scale", head, True, dict(scale=None), EINVAL, PTR8 % HD8),
    ("head8 q8 + 4 bytes", head, True, dict(q8=Q8 + 4), EINVAL, PTR8 % HD8),
    ("head8 shape before pointers", head, True, dict(q8=None, heads=-1), EINVAL, HD8_SHAPE % (2, 8, -1, 512, 512)),
]


@pytest.mark.parametrize("name,call,fp8,kw,rc,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(lib, name, call, fp8, kw, rc, text):
    assert call(lib, fp8, **kw) == (rc, text)


EMPTY = [(ln, dict(x=None, y=None, q8=None, qs=None)), (rms, dict(x=None, w=None, q8=None, scale=None)),
         (head, dict(x=None, w=None, q8=None, scale=None))]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("zero", [dict(batch=0), dict(rows=0)])
@pytest.mark.parametrize("call,nulls", EMPTY, ids=["ln", "rms", "head"])
def test_an_empty_batch_is_done_after_the_shape_check(lib, call, nulls, zero, fp8):
    """batch * rows == 0: ALG_OK, pointers may be null -- but a bad shape is still refused.  (The bf16-parameter LayerNorm
    entries and alg_qk_norm_rope_scaled have no empty batch: they refuse batch, rows or S <= 0, see REFUSALS.)"""
    assert call(lib, fp8, **zero, **nulls)[0] == OK
    assert call(lib, fp8, batch=0, rows=-1)[0] == EINVAL


def test_valid_calls_of_the_other_entries_reach_their_launch(lib):
    for call, fp8 in ((lnb, False), (lnb, True), (lnb_seg, False), (lnb_seg, True)):
        rc, text = call(lib, fp8)
        assert rc == ELAUNCH and text.startswith(LNB8 if fp8 else LNB), text
    for heads in (4, 16):
        rc, text = qk(lib, heads=heads)
        assert rc == ELAUNCH and text.startswith(QK + ": launch failed: "), text


# ---- NEW with the change: block counts beyond 2^31 - 1 used to be truncated to 32 bits and launched.  2^17 - 4 batch items of
# 2^16 + 2 rows are 2^33 - 8 rows: 2^31 - 2 workgroups of four.  One more row per item crosses 2^31 - 1.
COVERS = "%s: %s = %d is more than one launch covers"
B_LIM, R_FIT, R_OVER = (1 << 17) - 4, (1 << 16) + 2, (1 << 16) + 3
assert (B_LIM * R_FIT + 3) // 4 == 0x7fffffff - 1 and (B_LIM * (R_FIT + 1) + 3) // 4 > 0x7fffffff
# the exact edge: 2^31 - 1 batch items of 4 rows are 2^31 - 1 workgroups; of 5 rows, more
EDGE_FIT, EDGE_OVER = dict(batch=0x7fffffff, rows=4), dict(batch=0x7fffffff, rows=5)
LIMITS = [
    ("lnb", lnb, False, LNB, "batch * rows", 1),
    ("lnb_seg", lnb_seg, False, LNB, "batch * rows", 1),
    ("ln", ln, False, LN, "batch * rows", 1),
    ("ln8", ln, True, LN8, "batch * rows", 1),
    ("rms", rms, False, RMS, "batch * rows", 1),
    ("rms8", rms, True, RMS8, "batch * rows", 1),
]


@pytest.mark.parametrize("name,call,fp8,entry,what,per", LIMITS, ids=[r[0] for r in LIMITS])
def test_more_than_one_launch_covers(lib, name, call, fp8, entry, what, per):
    assert call(lib, fp8, **EDGE_FIT)[0] == ELAUNCH                                     # 2^31 - 1 workgroups: one launch
    assert call(lib, fp8, **EDGE_OVER) == (ELIMIT, COVERS % (entry, what, 5 * 0x7fffffff))   # ceil(5 (2^31 - 1) / 4) > 2^31 - 1
    assert call(lib, fp8, batch=B_LIM, rows=R_FIT)[0] == ELAUNCH
    assert call(lib, fp8, batch=B_LIM, rows=R_OVER) == (ELIMIT, COVERS % (entry, what, B_LIM * R_OVER))
    assert call(lib, fp8, x=None, **EDGE_OVER)[0] == EINVAL                             # the null pointer comes first


@pytest.mark.parametrize("fp8", [False, True])
def test_more_head_vectors_than_one_launch_covers(lib, fp8):
    """sixteen head vectors per workgroup: 2^31 - 1 items of 4 rows x 4 heads are exactly 2^31 - 1 workgroups"""
    entry = HD8 if fp8 else HD
    assert head(lib, fp8, batch=0x7fffffff, rows=4, heads=4)[0] == ELAUNCH
    assert head(lib, fp8, batch=0x7fffffff, rows=1, heads=17, xrs=17 * 128, q8rs=17 * 128) == \
        (ELIMIT, COVERS % (entry, "batch * rows * heads", 17 * 0x7fffffff))
    assert head(lib, fp8, batch=0x7fffffff, rows=1, heads=16, xrs=16 * 128, q8rs=16 * 128)[0] == ELAUNCH
    assert head(lib, fp8, batch=0x7fffffff, rows=4, heads=5, xrs=5 * 128, q8rs=5 * 128, w=None)[0] == EINVAL


# =====================================================================================================================
# routes of alg_layernorm_mod_f32(_fp8): "<entry> (<route>, rpw=<n>, grid=<g>): launch failed: ..."
# =====================================================================================================================
ONE, MANY, GENERIC = "one row per wave", "many rows", "generic width"
MOD = dict(w=None, b=None, sc=SC, sh=SH)
AFFINE = dict(w=W, b=B, sc=None, sh=None)


def many(total_per_item, batch):
    """the parent's formula at 256 CUs: 768 resident workgroups of four waves"""
    total = total_per_item * batch
    rpw = max(8, (total + 4 * 768 - 1) // (4 * 768))
    return MANY, rpw, batch * ((total_per_item + 4 * rpw - 1) // (4 * rpw))


def one(total, route=ONE):
    return route, 1, (total + 3) // 4


ROUTES = [
    ("modulation, 4095 rows", dict(MOD, batch=1, rows=4095), one(4095)),
    ("modulation, 4096 rows", dict(MOD, batch=1, rows=4096), (MANY, 8, 128)),
    ("affine, 4095 rows", dict(AFFINE, batch=1, rows=4095), one(4095)),
    ("affine, 4096 rows", dict(AFFINE, batch=1, rows=4096), (MANY, 8, 128)),
    ("all four parameters", dict(w=W, b=B, batch=1, rows=4096), one(4096)),
    ("scale without shift", dict(MOD, sh=None, batch=1, rows=4096), one(4096)),
    ("D = 6144", dict(MOD, batch=1, rows=4096, D=6144, mod=6144), (MANY, 8, 128)),
    ("D = 6656: no register kernel", dict(MOD, batch=1, rows=4096, D=6656, mod=6656), one(4096, GENERIC)),
    ("mod_bstride % 4", dict(MOD, batch=2, rows=2048, mod=1026), one(4096)),
    ("affine ignores mod_bstride", dict(AFFINE, batch=2, rows=2048, mod=1026), (MANY, 8, 128)),
    ("scale 4 bytes off", dict(MOD, sc=SC + 4, batch=1, rows=4096), one(4096)),
    ("bias 4 bytes off", dict(AFFINE, b=B + 4, batch=1, rows=4096), one(4096)),
    # (5 x 512 passes every many-row condition but no register kernel, one-row or many-row, is instantiated for it: the library has
    # always sent it to the generic-width kernel, and this records that)
    ("5 x 512: eligible, not instantiated", dict(MOD, batch=1, rows=4096, D=2560, mod=2560), one(4096, GENERIC)),
    ("D = 1280", dict(MOD, batch=1, rows=4096, D=1280, mod=1280), one(4096, GENERIC)),
    ("2 x 5003 rows", dict(MOD, batch=2, rows=5003), (MANY, 8, 314)),
    ("2 x 17776 rows", dict(MOD, batch=2, rows=17776, D=5120, mod=5120), many(17776, 2)),
]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("name,kw,want", ROUTES, ids=[r[0] for r in ROUTES])
def test_planned_route(lib, name, kw, want, fp8):
    rc, text = ln(lib, fp8, **kw)
    if fp8 and want[0] == GENERIC:          # the generic kernel has no e4m3 output
        assert (rc, text) == (EINVAL, LN_WIDTH % kw["D"])
        return
    prefix = "%s (%s, rpw=%d, grid=%d): launch failed: " % ((LN8 if fp8 else LN,) + want)
    assert rc == ELAUNCH and text.startswith(prefix), text


# ---- the bf16-parameter family: many rows with all four parameter rows, up to D = 3072, from 4,096 rows; rpw for one resident
# round of 2,048 waves (256 CUs), at least 8.  The e4m3 twins always run one row per wave.
LNB_ROUTES = [
    ("4095 rows, all four", dict(batch=1, rows=4095), one(4095)),
    ("4096 rows, all four", dict(batch=1, rows=4096), (MANY, 8, 128)),
    ("2 x 2048 rows", dict(batch=2, rows=2048, xbs=2048 * 1024, ybs=2048 * 1024), (MANY, 8, 128)),
    ("D = 3072", dict(batch=1, rows=4096, D=3072, mod=3072, segs=3072), (MANY, 8, 128)),
    ("D = 3584", dict(batch=1, rows=4096, D=3584, mod=3584, segs=3584), one(4096)),
    ("no weight", dict(batch=1, rows=4096, w=None), one(4096)),
    ("no bias", dict(batch=1, rows=4096, b=None), one(4096)),
    ("no modulation", dict(batch=1, rows=4096, sc=None, sh=None), one(4096)),
    ("the C2 call: 35,552 rows at D = 3072", dict(batch=2, rows=17776, D=3072, mod=3072, segs=3072, xbs=17776 * 3072,
                                                 ybs=17776 * 3072), (MANY, 18, 494)),
    ("D = 8192", dict(batch=1, rows=16, D=8192, mod=8192, segs=8192), one(16)),
]


@pytest.mark.parametrize("seg", [False, True], ids=["plain", "seg"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("name,kw,want", LNB_ROUTES, ids=[r[0] for r in LNB_ROUTES])
def test_planned_route_of_the_bf16_parameter_family(lib, name, kw, want, fp8, seg):
    rc, text = lnb(lib, fp8, seg, **kw)
    if fp8:
        want = one(kw["batch"] * kw["rows"])
    prefix = "%s (%s, rpw=%d, grid=%d): launch failed: " % ((LNB8 if fp8 else LNB,) + want)
    assert rc == ELAUNCH and text.startswith(prefix), text


def test_norm_rope_launch_message(lib):
    for call, fp8, entry in ((rms, False, RMS), (rms, True, RMS8), (head, False, HD), (head, True, HD8)):
        rc, text = call(lib, fp8)
        assert rc == ELAUNCH and text.startswith(entry + ": launch failed: "), text
