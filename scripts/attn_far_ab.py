"""Measurements of the opt-in far-field attention reuse (alg_amd/attn_far.py) on one GPU, written as one JSON file
(profiles/attn_far_ab.json is a run of this).  One job, arms alternated in one process, package power and clock per arm.

    python scripts/attn_far_ab.py --out profiles/attn_far_ab.json [--only kernel,layer,c2,c3,c4,video] [--steps 50] [--layers N]

  kernel   alg_attn_merge_lse at the C2 (17,776 x 48 heads x 64) and C3 (32,760 x 40 heads x 128) per-sample shapes next to
           alg_lincomb's 2-term in-place add on a bf16 tensor of the same size (the same bytes: two reads, one write)
  layer    at the C2 / C3 / C4 launch shapes, with the half-coverage windows of scripts/attn_window_ab.py (C2: window 2): the dense
           entry (first and last: their distance is the job's spread), the near launch (the grid-aligned window) without and with
           lse, the far launches (one per sample, with lse), the merges (one per sample), and near + far + merge as one unit -- its
           distance to the dense entry is the price of a refresh
  c2 c3 c4 iterations 0-1 of the bench workloads through the pipeline's __call__ in one process: off, window only, far reuse
           (N = 2, a range that holds every timestep: iteration 0 refreshes, iteration 1 reuses), off -- every step timed on its own
  video    one 50-step C2 video: off, far reuse N = 2, N = 4, off (window 2, the default range 100 < t < 800)

No bound is set in advance.  Synthetic Gaussian weights: nothing here says anything about quality."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import bench  # noqa: E402
from alg_amd import _lib  # noqa: E402
from alg_amd.attn_window import complement_ranges, frame_window_ranges, grid_aligned  # noqa: E402
from attn_window_ab import SHAPES, timed, window_for  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda:0")
EVERYWHERE = (-1, 1000000)      # a range that holds every timestep
C2 = dict(frames=13, hw=1350, prefix=226, heads=48, samples=2, window=2)


def kernel_part(iters):
    out = {}
    for name, rows, heads, hd in (("c2_17776x48x64", 17776, 48, 64), ("c3_32760x40x128", 32760, 40, 128)):
        D = heads * hd
        g = torch.Generator(device=DEV).manual_seed(0)
        o, far = (torch.randn(rows, D, generator=g, device=DEV, dtype=BF) for _ in range(2))
        lse, lse_far = (torch.randn(heads * rows, generator=g, device=DEV) * 3.0 for _ in range(2))
        lse_out = torch.empty_like(lse)
        arms = [("lincomb_first", lambda: _lib.lincomb([(1.0, o), (1.0, far)], BF, out=o)),
                ("merge", lambda: _lib.attn_merge_lse(o, lse, far, lse_far, 1, heads, hd, rows, rows * D, D, rows * D, D)),
                ("merge_lse_out", lambda: _lib.attn_merge_lse(o, lse, far, lse_far, 1, heads, hd, rows, rows * D, D, rows * D, D,
                                                              lse_out=lse_out)),
                ("lincomb_last", lambda: _lib.lincomb([(1.0, o), (1.0, far)], BF, out=o))]
        rec = {"rows": rows, "heads": heads, "head_dim": hd, "bytes_moved": 3 * rows * D * 2 + 2 * heads * rows * 4, "arms": {}}
        for label, fn in arms:
            o.normal_()       # (the in-place arms would otherwise walk off to inf)
            r = timed(fn, iters)
            r["gb_per_s"] = rec["bytes_moved"] / (r["median_ms"] * 1e-3) / 1e9
            rec["arms"][label] = r
        a, b = rec["arms"]["lincomb_first"]["median_ms"], rec["arms"]["lincomb_last"]["median_ms"]
        rec["lincomb_ms_mean"], rec["lincomb_spread_ms"] = (a + b) / 2, abs(a - b)
        rec["merge_over_lincomb"] = rec["arms"]["merge"]["median_ms"] / rec["lincomb_ms_mean"]
        out[name] = rec
        del o, far, lse, lse_far, lse_out
        torch.cuda.empty_cache()
    return out


def layer_part(iters):
    out = {}
    for name in ("c2", "c3_32760x40", "c4_119056x24"):
        if name == "c2":
            F, hw, T, heads, N, w = (C2[k] for k in ("frames", "hw", "prefix", "heads", "samples", "window"))
            hd, Sq = 64, T + F * hw
            Skv = Sq
            window = frame_window_ranges(F, hw, w, prefix=T)
            pad = (Sq + 127) // 128 * 128
        else:
            F, hw, valid, rows, heads = SHAPES[name]
            hd, N, Sq, Skv = 128, 1, F * hw + rows, F * hw + valid
            w, window = window_for(F, hw, valid, rows, 0.5)
            pad = (Sq + 63) // 64 * 64
        D = heads * hd
        near = grid_aligned(window)
        far = complement_ranges(near)
        for t in (window, near, far):
            t.device_table
        g = torch.Generator(device=DEV).manual_seed(0)
        qk = torch.randn(N, Sq, 2 * D, generator=g, device=DEV, dtype=BF)
        if hd == 64:
            qk[:, :, :D] *= 0.125 * 1.4426950408889634       # Q pre-scaled: the scores are in log2 units
        vt = torch.randn(N, D, pad, generator=g, device=DEV, dtype=BF)
        o = torch.empty(N, Sq, D, dtype=BF, device=DEV)
        e_o = torch.empty(N, Sq, D, dtype=BF, device=DEV)     # the samples' cache entries of one layer
        lse_n, lse_f = (torch.empty(N, heads, Sq, device=DEV) for _ in range(2))
        if hd == 64:
            args = lambda n_, o_, off: ((qk, qk, vt[off:] if n_ == 1 else vt, o_, n_, heads, Sq, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D),
                                        dict(q_off=off * Sq * 2 * D, k_off=off * Sq * 2 * D + D))
            dense = lambda: _lib.flash_attn_d64(*args(N, o, 0)[0], 0.125, k_off=D, q_prescaled=True)
            plain = lambda t: (lambda: _lib.flash_attn_d64_ranges(*args(N, o, 0)[0], t, k_off=D))
            entry = _lib.flash_attn_d64_ranges_heads
        else:
            scale = 1.0 / 128 ** 0.5
            args = lambda n_, o_, off: ((qk, qk, vt, o_, n_, heads, Sq, Skv, Sq * 2 * D, 2 * D, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D, scale),
                                        dict(q_off=off * Sq * 2 * D, k_off=off * Sq * 2 * D + D, vt_off=off * D * pad))
            dense = lambda: _lib.flash_attn_d128(*args(N, o, 0)[0], k_off=D)
            plain = lambda t: (lambda: _lib.flash_attn_d128_ranges(*args(N, o, 0)[0], t, k_off=D))
            entry = _lib.flash_attn_d128_ranges_heads

        def near_lse():
            a, kw = args(N, o, 0)
            entry(*a, near, lse=lse_n, **kw)

        def far_launches():
            for n in range(N):
                a, kw = args(1, e_o[n], n)
                entry(*a, far, lse=lse_f, lse_off=n * heads * Sq, **kw)

        def merges():
            for n in range(N):
                _lib.attn_merge_lse(o, lse_n, e_o, lse_f, 1, heads, hd, Sq, Sq * D, D, Sq * D, D, o_off=n * Sq * D,
                                    lse_off=n * heads * Sq, far_off=n * Sq * D, lse_far_off=n * heads * Sq)

        def refresh():
            near_lse(), far_launches(), merges()

        def reuse():
            near_lse(), merges()

        arms = [("dense_first", dense), ("window", plain(window)), ("near_no_lse", plain(near)), ("near_lse", near_lse),
                ("far_lse", far_launches), ("merge", merges), ("refresh_near_far_merge", refresh), ("reuse_near_merge", reuse),
                ("dense_last", dense)]
        rec = {"samples": N, "queries": Sq, "keys": Skv, "heads": heads, "head_dim": hd, "attn_window": w,
               "coverage_window": window.coverage, "coverage_near": near.coverage, "coverage_far": far.coverage, "arms": {}}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
            dense()
            torch.cuda.synchronize()
        for label, fn in arms:
            rec["arms"][label] = timed(fn, iters)
        a, b = rec["arms"]["dense_first"]["median_ms"], rec["arms"]["dense_last"]["median_ms"]
        d = rec["dense_ms_mean"] = (a + b) / 2
        rec["dense_spread_ms"] = abs(a - b)
        for r in rec["arms"].values():
            r["ms_over_dense"] = r["median_ms"] / d
        ms = lambda k: rec["arms"][k]["median_ms"]
        rec["refresh_minus_dense_ms"] = ms("refresh_near_far_merge") - d
        rec["near_lse_minus_near_no_lse_ms"] = ms("near_lse") - ms("near_no_lse")
        rec["cost_model"] = {"coverage_near": near.coverage,
                             "N=2": {"arithmetic": (1 + near.coverage) / 2, "measured": (ms("refresh_near_far_merge") + ms("reuse_near_merge")) / 2 / d},
                             "N=4": {"arithmetic": (1 + 3 * near.coverage) / 4, "measured": (ms("refresh_near_far_merge") + 3 * ms("reuse_near_merge")) / 4 / d}}
        out[name] = rec
        del qk, vt, o, e_o, lse_n, lse_f
        gc.collect()
        torch.cuda.empty_cache()
    return out


def run_video(wl, steps):
    """`steps` loop iterations of one video through pipe.__call__, every step timed: [{"ms", "passes", "reused"}], total seconds"""
    marks, trace = [], []

    def cb(pipe, i, t, kw):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        if i + 1 >= steps:
            pipe._interrupt = True
        return {}

    smi = bench.SmiSampler(DEV.index or 0)
    smi.__enter__()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        wl.last_out = wl.pipe(callback_on_step_end=cb, step_trace=trace, **wl.kwargs).frames
        torch.cuda.synchronize()
    finally:
        smi.__exit__(None, None, None)
    total = time.perf_counter() - t0
    st = list(wl.model.attn_far_reuse_stats) if wl.model.attn_far_reuse else []
    per = [{"ms": (m - (marks[i - 1] if i else t0)) * 1e3,
            "passes": next((v for v in trace[i][1:] if isinstance(v, int) and not isinstance(v, bool)), None),
            "reused": bool(st[i]["reused"]) if i < len(st) else False} for i, m in enumerate(marks)]
    sm = smi.summary()
    box = {"power_w": round(sm["power_w"]["mean"], 1), "sclk_mhz": round(sm["sclk_mhz"]["mean"], 1)} if sm and sm.get("power_w") and sm.get("sclk_mhz") else None
    return per, total, box


def arm(wl, steps, window, every, rng):
    m = wl.model
    m.attn_window, m.attn_far_reuse = window, every
    m.attn_far_reuse_t_lo, m.attn_far_reuse_t_hi = rng if rng is not None else (100, 800)
    per, total, box = run_video(wl, steps)
    by = {}
    for r in per[1:] if steps > 2 else per:
        by.setdefault("%s-pass %s" % (r["passes"], "reused" if r["reused"] else "computed"), []).append(r["ms"])
    return {"attn_window": window, "attn_far_reuse": every, "range": [m.attn_far_reuse_t_lo, m.attn_far_reuse_t_hi], "steps": len(per),
            "seconds": total, "ms_per_step": total / max(len(per), 1) * 1e3, "box": box,
            "classes": {k: {"median_ms": statistics.median(v), "n": len(v)} for k, v in sorted(by.items())},
            "reused": "".join("T" if r["reused"] else "F" for r in per), "step_ms": [round(r["ms"], 2) for r in per],
            "attn_far_reuse_bytes": m.attn_far_reuse_bytes, "finite": bool(torch.isfinite(wl.last_out.float()).all().item())}


def workload(name, steps, layers, window, arms):
    argv = ["--workload", name, "--gpus", "1"] + (["--layers", str(layers)] if layers else [])
    wl = bench.WORKLOADS[name](bench.parse_args(argv), DEV, 0, 1, None)
    t0 = time.perf_counter()
    wl.build()
    torch.cuda.synchronize()
    if window is None:     # the half-coverage window of scripts/attn_window_ab.py for this workload's shape
        F, hw, valid, rows, _ = SHAPES[{"c3": "c3_32760x40", "c4": "c4_119056x24", "c5": "c5_75600x40"}[name]]
        window = window_for(F, hw, valid, rows, 0.5)[0]
    res = {"layers": wl.layers, "tokens": wl.config(0)["tokens"], "attn_window": window, "build_seconds": round(time.perf_counter() - t0, 1),
           "arms": {}}
    arm(wl, min(steps, 4), 0, 0, None)                         # warm-up: the workspaces of both pass counts
    arm(wl, min(steps, 4), window, 2, EVERYWHERE)              # ... the tables and the cache's entries
    for tag, on, every, rng in arms:
        res["arms"][tag] = arm(wl, steps, window if on else 0, every, rng)
    wl.model.attn_window = wl.model.attn_far_reuse = 0
    off = [res["arms"]["off_first"], res["arms"]["off_last"]]
    mean_off = res["off_ms_per_step_mean"] = sum(a["ms_per_step"] for a in off) / 2
    res["off_spread_pct"] = abs(off[0]["ms_per_step"] - off[1]["ms_per_step"]) / mean_off * 100
    for tag, a in res["arms"].items():
        a["over_off"] = a["ms_per_step"] / mean_off
        if steps == 2:
            a["iteration_over_off"] = [a["step_ms"][i] / ((off[0]["step_ms"][i] + off[1]["step_ms"][i]) / 2) for i in range(2)]
    res["peak_gib"] = round(torch.cuda.max_memory_allocated(DEV) / 2 ** 30, 1)
    del wl
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="kernel,layer,c2,c3,c4,video")
    ap.add_argument("--steps", type=int, default=50, help="loop iterations per arm of the `video` part (50 = a whole video)")
    ap.add_argument("--layers", type=int, default=0, help="debug: the workloads with fewer blocks")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "weights": "synthetic (seeded Gaussian); says nothing about a trained checkpoint"}
    if os.path.exists(a.out):      # parts measured by an earlier call of the same job are kept
        with open(a.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    two = [("off_first", False, 0, None), ("window_only", True, 0, None), ("far_reuse", True, 2, EVERYWHERE), ("off_last", False, 0, None)]
    for part in a.only.split(","):
        if part == "kernel":
            res["kernel"] = kernel_part(a.iters)
        elif part == "layer":
            res["layer"] = layer_part(a.iters)
        elif part == "c2":
            res["c2"] = workload("c2", 2, a.layers, C2["window"], two)
        elif part in ("c3", "c4"):
            res[part] = workload(part, 2, a.layers, None, two)
        elif part == "video":
            res["video"] = workload("c2", a.steps, a.layers, C2["window"],
                                    [("off_first", False, 0, None), ("far_reuse_2", True, 2, (100, 800)), ("far_reuse_4", True, 4, (100, 800)),
                                     ("off_last", False, 0, None)])
        else:
            raise SystemExit("--only: unknown part %r" % part)
        save()
        print(part, "done", flush=True)


if __name__ == "__main__":
    main()
