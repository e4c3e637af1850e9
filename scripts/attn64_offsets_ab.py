#!/usr/bin/env python3
"""A/B of the d = 64 attention kernel alone: ALG_ATTN_PP=4 (the default statement: zero offsets only) against ALG_ATTN_PP=8 (the
offset statement) at the C2 shape [2, 48, 17,776, 64], alternated in one process, HIP events around every launch, the path
counters of alg_attn_path_tap from a launch of their own.  Two operand sets: Gaussian q / k / v (every offset snaps to zero: both
arms run the same instructions) and block 0's q / k / v of the trained-like C2-shape forward (tests/helpers/trained_like.py on the
fp32 oracle, run on the device up to the first attention).

    python scripts/attn64_offsets_ab.py OUT.json [rounds]

Writes one JSON object (appended to profiles/attn64_offsets_ab.json by hand together with the step runs)."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from alg_amd import _lib  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
B, NH, S = 2, 48, 17776
D = NH * 64
FLOP = 4.0 * S * S * 64 * B * NH


def swap23(n):
    return (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)


def pack(q, k, v):
    """q (log2 units), k, v [B, NH, S, 64] on the device -> qkb [B, S, 2 D], V^T [B, D, S_pad] in the kernels' layouts"""
    flat = lambda t: t.transpose(1, 2).reshape(B, S, D)
    qkb = torch.cat([flat(q), flat(k)], dim=-1).to(BF).contiguous()
    S_pad = (S + 127) // 128 * 128
    n = torch.arange(S, device=DEV)
    perm = (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)
    vt = torch.zeros(B, D, S_pad, dtype=BF, device=DEV)
    vt[:, :, perm] = flat(v).to(BF).transpose(1, 2)
    return qkb, vt, S_pad


def gaussian():
    g = torch.Generator(device=DEV).manual_seed(0)
    c = 0.125 * math.log2(math.e)
    q, k, v = (torch.randn(B, NH, S, 64, generator=g, device=DEV) for _ in range(3))
    return pack(q * c, k, v)


class _Stop(Exception):
    pass


class _UpToV0(dict):
    def __setitem__(self, key, value):
        dict.__setitem__(self, key, value)
        if key == "v_0":
            raise _Stop()


def trained_like_block0():
    from helpers.trained_like import trained_like
    from helpers.trained_like_cases import C2
    from oracle import dit_oracle
    kw = dict(C2, num_layers=1)
    ocfg = dit_oracle.DiTConfig(**kw)
    w = trained_like(dit_oracle.init_weights(ocfg, seed=21, std=0.02, randomize_affine=True))
    w = {k: v.to(BF).float().to(DEV) for k, v in w.items()}
    g = torch.Generator().manual_seed(8)
    hs = torch.randn(2, 13, 32, 60, 90, generator=g).to(BF)
    hs[:, 1:, 16:] = 0
    ehs = torch.randn(2, 226, 4096, generator=g).to(BF)
    rope = dit_oracle.rope_tables(ocfg, 480, 720, 13)
    col = _UpToV0()
    try:
        with torch.no_grad():
            dit_oracle.dit_forward(ocfg, w, hs.float().to(DEV), ehs.float().to(DEV), torch.tensor([999, 999], device=DEV),
                                   tuple(t.to(DEV) for t in rope), collect=col)
    except _Stop:
        pass
    q, k, v = col["q_0"], col["k_0"], col["v_0"]
    assert q.shape == (B, NH, S, 64)
    qs = (q * (0.125 * math.log2(math.e))).to(BF)
    m1 = torch.einsum("bhqd,bhkd->bhqk", qs[:, :, :, :].float(), k[:, :, :64].to(BF).float()).amax(dim=-1)
    kept = float((m1.abs() >= 64.0).float().mean())
    return pack(qs, k, v), kept


def launch(qkb, vt, S_pad, o):
    _lib.flash_attn_d64(qkb, qkb, vt, o, B, NH, S, S * 2 * D, 2 * D, D * S_pad, S_pad, S * D, D, 0.125, k_off=D, q_prescaled=True)


def set_pp(pp):
    os.environ["ALG_ATTN_PP"] = pp
    _lib.reload_env()


def measure(name, qkb, vt, S_pad, rounds, reps=5):
    out = {"operands": name, "shape": [B, NH, S, 64], "arms": {"4": [], "8": []}, "counters": {}}
    o = {pp: torch.empty(B, S, D, dtype=BF, device=DEV) for pp in ("4", "8")}
    for pp in ("4", "8"):
        set_pp(pp)
        cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        _lib.attn_path_tap(cnt)
        try:
            launch(qkb, vt, S_pad, o[pp])
            torch.cuda.synchronize()
        finally:
            _lib.attn_path_tap(None)
        out["counters"][pp] = dict(zip(("entries", "tiles_in_statement", "tiles_straight"), (int(x) for x in cnt.cpu())))
    diff = (o["4"].float() - o["8"].float()).abs()
    out["pp8_vs_pp4"] = {"bit_identical": bool(torch.equal(o["4"], o["8"])), "max_abs_diff": float(diff.max()),
                         "finite": bool(torch.isfinite(o["8"].float()).all())}
    for r in range(rounds):
        for pp in ("4", "8"):
            set_pp(pp)
            for _ in range(2):
                launch(qkb, vt, S_pad, o[pp])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            ev[0].record()
            for i in range(reps):
                launch(qkb, vt, S_pad, o[pp])
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
            med = ms[reps // 2]
            out["arms"][pp].append({"round": r, "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                                    "tflops_median": round(FLOP / med / 1e9, 1)})
            print(name, "round", r, "ALG_ATTN_PP=" + pp, "%.3f ms  %.1f TFLOP/s" % (med, FLOP / med / 1e9), flush=True)
    return out


def main():
    path = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    res = {"kernel_only": []}
    qkb, vt, S_pad = gaussian()
    res["kernel_only"].append(measure("gaussian", qkb, vt, S_pad, rounds))
    del qkb, vt
    (qkb, vt, S_pad), kept = trained_like_block0()
    r = measure("trained_like_c2_block0", qkb, vt, S_pad, rounds)
    r["rows_with_first_tile_max_beyond_64"] = round(kept, 4)
    res["kernel_only"].append(r)
    os.environ.pop("ALG_ATTN_PP", None)
    _lib.reload_env()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
