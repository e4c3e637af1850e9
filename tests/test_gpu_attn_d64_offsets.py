"""ALG_ATTN_PP=8: the d = 64 pipelined statement for ANY running softmax offset (attn_pipe_off_loop.inc: -m is srcC of the first QK
k-step) and the frame that returns to it after a refused tile, through alg_flash_attn_d64 as the model calls it (pre-scaled q),
with the path counters of alg_attn_path_tap telling which tiles ran where.

Shapes: batch 2 x 3 heads (six (batch, head) panels over the 8-way grid interleave), S = 1,024 (T = 16 KV tiles, statement
iterations up to tend = 13: room for an entry at t = 1, a refusal, a second entry at t = 5 and a second refusal) and S = 1,000 (ragged,
tend = 12).  A wave = 32 consecutive queries; every launch runs batch x heads x ceil(S / 256) x 8 of them.

Accuracy bound: every output element within 2^-7 x max |v| of a float64 softmax of the SAME bf16 operands -- docs/numerics.md's
derivation (bf16 probabilities and their sum: 2 x 2^-9, the bf16 store: 2^-9, exp2 and the fp32 score chain: the remaining third),
the one tests/test_gpu_trained_like.py applies to the model's operands."""
import functools
import math
import os
import sys

import pytest
import torch

from alg_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from attn_off_emu import frame_path, pp4_path  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
B, NH = 2, 3
D = NH * 64


def _swap23(n):
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


def _waves(S):
    return B * NH * ((S + 255) // 256) * 8


@functools.lru_cache(maxsize=None)
def _operands(kind, S):
    """q (log2 units, as alg_qk_norm_rope_scaled leaves it), k, v as bf16 [B, S, NH, 64] and the float64 reference [B, S, NH, 64]"""
    g = torch.Generator().manual_seed({"gauss": 1, "wide": 2, "negative": 3, "bail": 4}[kind] + S)
    c = 0.125 * math.log2(math.e)
    q = torch.randn(B, S, NH, 64, generator=g) * c
    k = torch.randn(B, S, NH, 64, generator=g)
    v = torch.randn(B, S, NH, 64, generator=g)
    if kind == "wide":
        # every query looks along ONE axis of keys drawn from [-1, 1): scores = gain x k[key, axis] + a little noise, bounded by the
        # gain -- a row's first-tile max is then close to its global max (no refusals) while the x 6 on the odd rows carries
        # them from 16 to 96 log2 units: across the +-64 of the snap
        k = torch.rand(B, S, NH, 64, generator=g) * 2 - 1
        axis = torch.randint(0, 64, (B, S, NH), generator=g)
        q = 0.1 * q + 16.0 * torch.nn.functional.one_hot(axis, 64)
        q[:, 1::2] *= 6.0
    elif kind == "negative":
        q[..., 0], k[..., 0] = 1.0, -150.0                   # every score = -150 + N(0, 1.44^2)
    elif kind == "bail":
        # queries of every second row of every second wave carry 8 on axis 0, all others 0; one key of tile 2 = 12.5 e0, one key of tile
        # 10 = 26 e0: scores 100 and 208 for the planted rows (offset 0 -> 100 -> 208: both more than 80 above), 0 for everybody else
        rows = torch.arange(S)
        planted = ((rows // 32) % 2 == 1) & (rows % 2 == 0)
        q[..., 0] = 0.0
        q[:, planted, :, 0] = 8.0
        k[:, 2 * 64 + 5], k[:, 10 * 64 + 41] = 0.0, 0.0
        k[:, 2 * 64 + 5, :, 0], k[:, 10 * 64 + 41, :, 0] = 12.5, 26.0
    q, k, v = q.to(BF), k.to(BF), v.to(BF)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double())          # log2 units
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s * math.log(2.0), dim=-1), v.double())
    return q, k, v, s, ref


@functools.lru_cache(maxsize=None)
def _device_operands(kind, S):
    q, k, v, _, _ = _operands(kind, S)
    S_pad = (S + 127) // 128 * 128
    qkb = torch.cat([q.reshape(B, S, D), k.reshape(B, S, D)], dim=-1).contiguous().to(DEV)
    vt = torch.zeros(B, D, S_pad, dtype=BF)
    vt[:, :, torch.tensor([_swap23(n) for n in range(S)])] = v.reshape(B, S, D).transpose(1, 2)
    return qkb, vt.to(DEV), S_pad


def _run(kind, S, pp, monkeypatch):
    """-> (output [B, S, NH, 64] on the host, counters [entries, tiles inside the statement, tiles in the straight loop])"""
    qkb, vt, S_pad = _device_operands(kind, S)
    monkeypatch.setenv("ALG_ATTN_PP", pp)
    o = torch.full((B, S, D), 3.0, dtype=BF, device=DEV)
    cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
    _lib.attn_path_tap(cnt)
    try:
        _lib.flash_attn_d64(qkb, qkb, vt, o, B, NH, S, S * 2 * D, 2 * D, D * S_pad, S_pad, S * D, D, 0.125, k_off=D, q_prescaled=True)
        torch.cuda.synchronize()
    finally:
        _lib.attn_path_tap(None)
    return o.cpu().reshape(B, S, NH, 64), [int(x) for x in cnt.cpu()]


def _bound(name, got, kind, S):
    _, _, v, _, ref = _operands(kind, S)
    assert bool(torch.isfinite(got).all()), name
    err = (got.double() - ref).abs().max().item()
    bound = 2.0 ** -7 * v.double().abs().max().item()
    print("%s: max |err| %.3e, bound %.3e" % (name, err, bound))
    assert err <= bound, (name, err, bound)


def _first_tile_max(kind, S):
    return _operands(kind, S)[3][..., :64].max(dim=-1).values                  # [B, NH, S]


def _no_row_bails(kind, S):
    """no row sum can reach 2^80: against the offset tile 0 leaves (its max, or 0 when that lies inside +-64), every later score
    stays below 80 - log2(64 keys) - 4 of slack"""
    s = _operands(kind, S)[3]
    m1 = s[..., :64].max(dim=-1).values
    m = torch.where(m1.abs() < 64.0, torch.zeros_like(m1), m1)
    return bool(((s.max(dim=-1).values - m) < 70.0).all())


def _counts(path, n):
    return [n * x for x in path]


def test_gaussian_operands_pp8_is_bit_identical_to_pp4_and_takes_the_same_path(monkeypatch):
    S = 1024
    assert bool((_first_tile_max("gauss", S).abs() < 64.0).all())                # every offset snaps to zero
    o4, c4 = _run("gauss", S, "4", monkeypatch)
    o8, c8 = _run("gauss", S, "8", monkeypatch)
    print("counters pp4", c4, "pp8", c8)
    assert torch.equal(o8, o4)
    assert c8 == c4 == _counts(frame_path(16, False), _waves(S)) == _counts(pp4_path(16, False, True), _waves(S))
    _bound("gauss pp8", o8, "gauss", S)


def test_wide_scores_every_wave_enters_the_statement_under_pp8(monkeypatch):
    """Half the rows of EVERY wave keep a non-zero offset: ALG_ATTN_PP=4 shuts every wave out of the statement (this is the test that
    fails without the offset form), ALG_ATTN_PP=8 runs what 4 runs on Gaussian operands: one entry and four straight tiles per wave."""
    S = 1024
    kept = (_first_tile_max("wide", S).abs() >= 64.0).double().mean().item()
    assert 0.3 <= kept <= 0.7, kept
    assert _no_row_bails("wide", S)
    _, g4 = _run("gauss", S, "4", monkeypatch)
    o8, c8 = _run("wide", S, "8", monkeypatch)
    o4, c4 = _run("wide", S, "4", monkeypatch)
    print("kept %.3f, counters: gauss pp4" % kept, g4, "wide pp8", c8, "wide pp4", c4)
    _bound("wide pp8", o8, "wide", S)
    _bound("wide pp4", o4, "wide", S)
    W = _waves(S)
    assert c8[0] / W == g4[0] / W == 1 and c8[2] / W == g4[2] / W == 4
    assert c4[1] < c8[1] and c4[1] + c4[2] == c8[1] + c8[2] == 16 * W


def test_all_scores_far_below_zero(monkeypatch):
    S = 1024
    s = _operands("negative", S)[3]
    assert bool((s < -100.0).all()) and _no_row_bails("negative", S)
    o8, c8 = _run("negative", S, "8", monkeypatch)
    print("counters pp8", c8)
    _bound("negative pp8", o8, "negative", S)
    assert c8 == _counts(frame_path(16, False), _waves(S))


def test_a_wave_returns_to_the_statement_after_a_refused_tile(monkeypatch):
    """Planted keys in tiles 2 and 10, each more than 80 log2 units above the offset the row holds when it gets there: a wave with
    such rows leaves at t = 2, redoes tile 2 on the exact path, runs tiles 3 and 4 in the straight form, enters again at t = 5
    (every row of it now with a non-zero offset), leaves at t = 10 and finishes in the straight form (the next entry point, 13, has no
    whole group of four left).  Fails without the feature: ALG_ATTN_PP=4 never returns."""
    S, T = 1024, 16
    s = _operands("bail", S)[3]
    rows = torch.arange(S)
    planted = ((rows // 32) % 2 == 1) & (rows % 2 == 0)
    assert planted.double().mean().item() == 0.25
    assert bool((s[..., :64].max(dim=-1).values.abs() < 64.0).all())           # every row snaps on tile 0
    sp = s[:, :, planted]
    assert bool((sp[..., 2 * 64 + 5] > 80.0).all()) and bool((sp[..., 10 * 64 + 41] - sp[..., 2 * 64 + 5] > 80.0).all())
    rest = torch.ones(S, dtype=torch.bool)
    rest[2 * 64 + 5], rest[10 * 64 + 41] = False, False
    assert bool((s[..., rest].max() < 60.0))                                  # nothing else comes near a refusal
    assert bool((s[:, :, ~planted][..., ~rest] == 0.0).all())
    o8, c8 = _run("bail", S, "8", monkeypatch)
    o4, c4 = _run("bail", S, "4", monkeypatch)
    print("counters pp8", c8, "pp4", c4)
    _bound("bail pp8", o8, "bail", S)
    _bound("bail pp4", o4, "bail", S)
    W = _waves(S)
    plain, hit = frame_path(T, False), frame_path(T, False, refused=(2, 10))
    assert plain == (1, 12, 4) and hit == (2, 6, 10)
    # straight tiles of an affected wave = the no-refusal count + the two refused tiles + the tiles waited out (3, 4 and 11, 12)
    assert hit[2] == plain[2] + 2 + 4
    assert c8 == [W // 2 * (plain[i] + hit[i]) for i in range(3)]
    assert c4 == [W // 2 * (plain[i] + pp4_path(T, False, True, refused=(2,))[i]) for i in range(3)]
    assert c8[0] > W and c4[0] == W and c8[1] > c4[1]


def test_ragged_sequence_with_wide_scores(monkeypatch):
    S = 1000
    assert _no_row_bails("wide", S)
    o8, c8 = _run("wide", S, "8", monkeypatch)
    print("counters pp8", c8)
    _bound("wide ragged pp8", o8, "wide", S)
    assert c8 == _counts(frame_path(16, True), _waves(S)) == _counts((1, 8, 8), _waves(S))


def test_cog_medium_trained_like_forward_under_pp8(monkeypatch):
    """The CogVideoX medium trained-like forward (half of block 0's rows keep an offset, a few hundred are refused) under
    ALG_ATTN_PP=8: on the bf16-eager floor with tests/_parity.py's factors, and the statement's share of block 0's attention launch.
    Per wave tiles inside + tiles straight = T, so `share(8) >= share(4 on Gaussian weights) - (refused + realignment tiles)` is
    counted from the straight side: what ALG_ATTN_PP=8 runs in the straight form beyond the 7 tiles of a Gaussian wave (tile 0, the
    ragged tail from 13 on) are its refused tiles and the tiles up to the next entry point.  Each of them follows a refusal, a
    refusal ends an entry (so there are at most as many as entries), and one costs at most four tiles: the refused one and up to
    three to the next t = 1 (mod 4), or, when no further entry fits, what was left of the last group of four."""
    from _parity import check_floor
    from alg_amd import CogVideoXTransformer3DModel, CogVideoXTransformerConfig
    from helpers.trained_like_cases import cog_case
    from oracle import dit_oracle
    kw, ocfg, wbf, (hs, ehs, ts, rope) = cog_case("medium")
    col = {}
    ref = dit_oracle.dit_forward(ocfg, {k: v.float() for k, v in wbf.items()}, hs.float(), ehs.float(), ts, rope, collect=col)
    bf16 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    monkeypatch.setenv("ALG_ATTN_PP", "8")
    model = CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=DEV)
    out = model(hs.to(DEV), ehs.to(DEV), ts, image_rotary_emb=rope, return_dict=False)[0]
    check_floor("cog_forward_medium_trained_like_pp8", out, ref, bf16, channel_dim=2)
    # block 0's launch alone, on the oracle's q / k / v rounded to bf16 (tests/test_gpu_trained_like.py's operands)
    q, k, v = col["q_0"], col["k_0"], col["v_0"]                                   # [N, H, S, 64]
    N, Hh, S, hd = q.shape
    Dm = Hh * hd
    T = (S + 63) // 64
    assert T == 19 and S % 64
    flat = lambda t: t.transpose(1, 2).reshape(N, S, Dm)
    qs = (q * (0.125 * math.log2(math.e))).to(BF)
    qkb = torch.cat([flat(qs), flat(k.to(BF))], dim=-1).contiguous().to(DEV)
    S_pad = (S + 127) // 128 * 128
    vt = torch.zeros(N, Dm, S_pad, dtype=BF)
    vt[:, :, torch.tensor([_swap23(n) for n in range(S)])] = flat(v.to(BF)).transpose(1, 2)
    vt = vt.to(DEV)
    cnts = {}
    for pp in ("4", "8"):
        monkeypatch.setenv("ALG_ATTN_PP", pp)
        o = torch.empty(N, S, Dm, dtype=BF, device=DEV)
        cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        _lib.attn_path_tap(cnt)
        try:
            _lib.flash_attn_d64(qkb, qkb, vt, o, N, Hh, S, S * 2 * Dm, 2 * Dm, Dm * S_pad, S_pad, S * Dm, Dm, 0.125, k_off=Dm,
                                q_prescaled=True)
            torch.cuda.synchronize()
        finally:
            _lib.attn_path_tap(None)
        cnts[pp] = [int(x) for x in cnt.cpu()]
    W = N * Hh * ((S + 255) // 256) * 8
    gauss = pp4_path(T, True, True)                       # what ALG_ATTN_PP=4 runs per wave on Gaussian weights at this shape
    assert gauss == (1, 12, 7)
    e8, in8, st8 = cnts["8"]
    print("block 0 of the medium trained-like forward, %d waves x %d tiles: pp4 %s, pp8 %s; Gaussian pp4 per wave %s"
          % (W, T, cnts["4"], cnts["8"], gauss))
    assert in8 + st8 == T * W and sum(cnts["4"][1:]) == T * W
    assert e8 >= W                                        # every wave enters, whatever its offsets
    lost = st8 - gauss[2] * W                             # refused + realignment tiles
    assert in8 / (T * W) >= gauss[1] / T - lost / (T * W) - 1e-12
    assert 0 <= lost <= 4 * e8                            # ... and they are explained by the refusals the entry count allows
    assert in8 > cnts["4"][1]
