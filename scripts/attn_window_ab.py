"""Measurements of the opt-in frame-window self-attention on one GPU, written as one JSON file (profiles/attn_window_ab.json is a
run of this).  One job, arms alternated, package power and shader clock sampled per arm (bench.SmiSampler).

    python scripts/attn_window_ab.py --out profiles/attn_window_ab.json [--only kernel|steps|accuracy]
    python scripts/attn_window_ab.py --family d64 --out profiles/attn_window_d64_ab.json [--only kernel|steps|accuracy]
    python scripts/attn_window_ab.py --family heads64 --out profiles/attn_window_heads_d64_ab.json [--only kernel|steps]
    python scripts/attn_window_ab.py --family order --out profiles/attn_window_order_ab.json [--only kernel|steps]
    python scripts/attn_window_ab.py --family widths --out profiles/attn_window_widths_ab.json [--only kernel|steps]
    python scripts/attn_window_ab.py --family band --out profiles/attn_band_ab.json [--only kernel|steps]

  kernel    alg_flash_attn_d128 against alg_flash_attn_d128_ranges at the three launch shapes (C3 32,760 x 40 heads, C5 75,600 x 40,
            C4 119,056 queries x 118,848 keys x 24 heads): the dense entry (first and last arm: their distance is the job's spread),
            the ranged entry with the one-full-range table, and with the frame windows whose coverage is closest to 3/4, 1/2 and
            1/4 -- milliseconds, coverage, and ms / dense ms
  steps     the C3 / C4 / C5 workloads of bench.py (what `bench.py --workload cX --steps 2 --warmup 1 --set attn_window=W` times:
            loop iterations 0-1 through the pipeline's __call__ behind one warm-up step), attn_window = 0 first and last and the
            1/2-coverage window between them, in one process per workload
  accuracy  4-step ALG samplers on the trained-like Wan and HunyuanVideo models of tests/helpers/trained_like_cases.py at 9 latent
            frames: relative L2 of the final latents with attn_window = 1, 2, 4 against the dense run, next
            to the dense run's distance to the fp32 loop oracle (the bf16-to-fp32 floor of that run)

--family d64 is CogVideoX (profiles/attn_window_d64_ab.json): the kernel arms at the C2 launch shape (2 x 48 heads x 17,776,
d = 64) -- alg_flash_attn_d64_ex in its default form (pre-scaled Q, split-KV tail on) against alg_flash_attn_d64_ranges (one launch,
no tail) with the full-range table and the windows 1 / 2 / 4 --, the C2 steps with attn_window = 2 between two dense runs, and the
accuracy arms on the trained-like CogVideoX model at the medium grid (8 heads x 64, 4 blocks, 9 latent frames of 384 tokens).

--family heads is the per-head window chosen by recall (profiles/attn_window_heads_ab.json), head_dim 128 only: at the same three
launch shapes alg_flash_attn_d128_ranges_heads with the full-range table and with the half-coverage window, each without and with
the lse output, and a per-head table in which every second head is dense -- set against 0.5 * (all dense + all windowed) of the same
job; the first two arms are repeated last (their distance is the job's spread).  Its steps arms time iterations 0-1 of the C3 / C5 /
C4 workloads with attn_window_recall = 0.9 on the half-coverage window (iteration 0 is the calibration forward; on these Gaussian
weights no head reaches 0.9, so iteration 1 is dense) between two runs with attn_window = 0.  No bound is set for any of them.

--family heads64 is the same for head_dim 64 (CogVideoX, profiles/attn_window_heads_d64_ab.json): at the C2 launch shape
alg_flash_attn_d64_ranges_heads with the full-range table and with the window-2 table, each without and with the lse output, a per-head
table in which every second head is dense against 0.5 * (all dense + all windowed) of the same job, and for orientation the shared-table
entry on the window and the dense entry in its default form (split-KV tail on); the steps arms time iterations 0-1 of the C2 workload with
attn_window = 2, attn_window_recall = 0.9 between two runs with the window off (iteration 0 is the calibration forward), and record the
recall minimum, mean and maximum next to the coverage.  No bound is set for any of them.

--family order is the coverage-balanced launch order (profiles/attn_window_order_ab.json; alg_flash_attn_d128_ranges_order at the C3 /
C5 / C4 launch shapes, alg_flash_attn_d64_ranges_order at C2, the half-coverage windows of the records above): all heads dense (first
and last: the job's spread), all heads windowed, every second head dense through the existing entry (twice: their distance is what a
gain has to exceed), through the new entry with the "natural" table (the price of the indirection) and with "lanes" and "units", three
of four heads windowed with natural / "lanes" / "units", and the shared all-windowed table with "lanes" (reported only: the model
predicts no gain).  Each mixed arm is set against 0.5 * (all dense + all windowed) of the same job, and as the fraction of the
available saving it realises.  Its steps arms time iterations 0-1 of the bench workloads with attn_window_balance off / on / "lanes" /
off in one process, attn_window_recall at the workload's recorded mean recall so that about half the heads window.  No bound is set.

--family widths is the per-head window WIDTH from one calibration pass (profiles/attn_window_widths_ab.json;
alg_flash_attn_d128_ranges_prefix, head_dim 128 only).  Kernel arms at the C3 / C5 / C4 launch shapes: the plain full-range launch,
the parent's calibration PAIR (full range with lse + the half-coverage window with lse, timed as one unit, without and with
alg_attn_lse_recall), ONE prefix launch over the 9-segment profile table of the widths (1, 2, half-coverage window) (without and with
alg_attn_prefix_mass), and the dense entry -- first and last, alternated.  The question: does the prefix launch cost less than the pair
by more than the job's spread, and how far above the plain full-range launch is it.  Steps arms: iterations 0-1 of the bench
workloads with attn_window_recall = 0.9 and attn_window_widths off / on / off between two arms with the window off; the calibration
cost per video is an arm's two steps minus the off arms' mean, over a dense step.  No bound is set.

--family band is the position-major band of Wan attn1 (profiles/attn_band_ab.json; alg_attn_rows_position_major,
alg_attn_vt_position_major, position_band_ranges).  Kernel arms at the C3 and C5 launch shapes, band 8: the dense entry first and
last, the all-windowed half-coverage launch, gather + band launch + scatter for ALL heads, the same for every second head with the
others dense through the main launch (band heads absent from its table; once in the kernels' own order and once in the "units"
order of attn_window_balance), and each layout kernel alone as bytes moved per second
(read + written) next to alg_lincomb's 2-term in-place add on a tensor of the same size.  Steps: iterations 0-1 of the C3 workload
with everything off / the recall policy alone / the band on / off.  No bound is set; everything is reported against the spread
between the repeated arms.  On Gaussian weights the band's recall sits near its coverage, so every head stays dense.

Synthetic weights: the accuracy numbers bound nothing on a trained checkpoint, and nothing here measures visual quality."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import bench  # noqa: E402
from alg_amd import _lib  # noqa: E402
from alg_amd.attn_window import (HeadList, balanced_order, frame_profile_segments, frame_window_ranges, full_ranges,  # noqa: E402
                                 head_layout_ranges, head_window_ranges, position_band_ranges, unit_costs)

BF = torch.bfloat16
DEV = torch.device("cuda:0")

# (frames, tokens per frame, prompt keys, prompt rows, heads)
SHAPES = {"c3_32760x40": (21, 1560, 0, 0, 40), "c5_75600x40": (21, 3600, 0, 0, 40), "c4_119056x24": (33, 3600, 48, 256, 24)}


def table_for(F, hw, valid, rows, window):
    S = F * hw
    return frame_window_ranges(F, hw, window, tail=(S, S + valid) if valid else None, rows=S + rows if rows else None)


def window_for(F, hw, valid, rows, coverage):
    """The window whose table's coverage is closest to `coverage`."""
    best = None
    for w in range(1, F):          # (attn_window = 0 is the models' "off")
        t = table_for(F, hw, valid, rows, w)
        if t is not None and (best is None or abs(t.coverage - coverage) < abs(best[1].coverage - coverage)):
            best = (w, t)
    return best


def timed(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    with bench.SmiSampler(0, period=0.05) as smi:
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    s = smi.summary() or {}
    return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "iters": iters,
            "power_w": (s.get("power_w") or {}).get("mean"), "sclk_mhz": (s.get("sclk_mhz") or {}).get("mean")}


def kernel_arms(name, iters):
    F, hw, valid, rows, heads = SHAPES[name]
    S, D = F * hw, heads * 128
    Sq, Skv = S + rows, S + valid
    pad = (Sq + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(Sq, 2 * D, generator=g, device=DEV, dtype=BF)          # the models' layout: Q | K rows, V^T apart
    vt = torch.randn(D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(Sq, D, dtype=BF, device=DEV)
    scale = 1.0 / 128 ** 0.5
    args = (qk, qk, vt, o, 1, heads, Sq, Skv, Sq * 2 * D, 2 * D, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D, scale)
    dense = lambda: _lib.flash_attn_d128(*args, k_off=D)
    ranged = lambda t: (lambda: _lib.flash_attn_d128_ranges(*args, t, k_off=D))
    arms = [("dense_first", dense, 1.0, None), ("full_range", ranged(full_ranges(Sq, Skv)), 1.0, None)]
    for label, cov in (("three_quarters", 0.75), ("half", 0.5), ("quarter", 0.25)):
        w, t = window_for(F, hw, valid, rows, cov)
        t.device_table
        arms.append((label, ranged(t), t.coverage, w))
    arms.append(("dense_last", dense, 1.0, None))
    out = {"queries": Sq, "keys": Skv, "heads": heads, "frames": F, "tokens_per_frame": hw, "arms": {}}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        dense()
        torch.cuda.synchronize()
    for label, fn, cov, w in arms:
        r = timed(fn, iters)
        r.update(coverage=cov, attn_window=w)
        out["arms"][label] = r
    a, b = out["arms"]["dense_first"]["median_ms"], out["arms"]["dense_last"]["median_ms"]
    d = out["dense_ms_mean"] = (a + b) / 2
    out["dense_spread_ms"] = abs(a - b)
    for r in out["arms"].values():
        r["ms_over_dense"] = r["median_ms"] / d
    out["full_range_minus_dense_ms"] = out["arms"]["full_range"]["median_ms"] - d
    out["full_range_within_dense_spread"] = out["full_range_minus_dense_ms"] <= out["dense_spread_ms"]
    del qk, vt, o
    torch.cuda.empty_cache()
    return out


def kernel_arms_heads(name, iters):
    F, hw, valid, rows, heads = SHAPES[name]
    S, D = F * hw, heads * 128
    Sq, Skv = S + rows, S + valid
    pad = (Sq + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(Sq, 2 * D, generator=g, device=DEV, dtype=BF)
    vt = torch.randn(D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(Sq, D, dtype=BF, device=DEV)
    lse = torch.empty(heads, Sq, dtype=torch.float32, device=DEV)
    args = (qk, qk, vt, o, 1, heads, Sq, Skv, Sq * 2 * D, 2 * D, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D, 1.0 / 128 ** 0.5)
    w, half = window_for(F, hw, valid, rows, 0.5)
    full = full_ranges(Sq, Skv)
    mixed = head_window_ranges(half, [h % 2 == 0 for h in range(heads)])
    for t in (half, full, mixed):
        t.device_table
    run = lambda t, l: (lambda: _lib.flash_attn_d128_ranges_heads(*args, t, lse=l, k_off=D))
    arms = [("full_range_first", run(full, None), 1.0), ("window_first", run(half, None), half.coverage),
            ("full_range_lse", run(full, lse), 1.0), ("window_lse", run(half, lse), half.coverage),
            ("half_heads_dense", run(mixed, None), mixed.coverage),
            ("shared_entry_window", lambda: _lib.flash_attn_d128_ranges(*args, half, k_off=D), half.coverage),
            ("full_range_last", run(full, None), 1.0), ("window_last", run(half, None), half.coverage)]
    out = {"queries": Sq, "keys": Skv, "heads": heads, "frames": F, "tokens_per_frame": hw, "attn_window": w, "arms": {}}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        arms[0][1]()
        torch.cuda.synchronize()
    for label, fn, cov in arms:
        r = timed(fn, iters)
        r["coverage"] = cov
        out["arms"][label] = r
    ms = lambda k: out["arms"][k]["median_ms"]
    d = out["full_range_ms_mean"] = (ms("full_range_first") + ms("full_range_last")) / 2
    h = out["window_ms_mean"] = (ms("window_first") + ms("window_last")) / 2
    out["full_range_spread_ms"], out["window_spread_ms"] = abs(ms("full_range_first") - ms("full_range_last")), abs(ms("window_first") - ms("window_last"))
    out["lse_cost_full_range_ms"], out["lse_cost_window_ms"] = ms("full_range_lse") - d, ms("window_lse") - h
    out["half_heads_dense_over_mean_of_both"] = ms("half_heads_dense") / (0.5 * (d + h))
    out["shared_entry_minus_new_entry_window_ms"] = ms("shared_entry_window") - h
    del qk, vt, o, lse
    torch.cuda.empty_cache()
    return out


def step_arms_heads(workload, recall=0.9, window=None):
    if window is not None:
        w_half = window        # (CogVideoX: the window is given; 2 has a coverage of 0.44 at C2)
    else:
        F, hw, valid, rows, _ = SHAPES[{"c3": "c3_32760x40", "c5": "c5_75600x40", "c4": "c4_119056x24"}[workload]]
        w_half = window_for(F, hw, valid, rows, 0.5)[0]
    args = bench.parse_args(["--workload", workload, "--gpus", "1", "--steps", "2", "--warmup", "1"])
    wl = bench.WORKLOADS[workload](args, DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    out = {"attn_window": w_half, "attn_window_recall": recall, "arms": {}}
    for label, w, r in (("off_first", 0, 0.0), ("calibration_then_decided", w_half, recall), ("off_last", 0, 0.0)):
        wl.model.attn_window, wl.model.attn_window_recall = w, r
        bench.run_steps(wl, 1)
        torch.cuda.synchronize()
        with bench.SmiSampler(0) as smi:
            t0 = time.perf_counter()
            bench.run_steps(wl, 2)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
        sm = smi.summary() or {}
        out["arms"][label] = {"attn_window": w, "attn_window_recall": r, "seconds_two_steps": s,
                              "finite": bool(torch.isfinite(wl.last_out.float()).all().item()),
                              "power_w": (sm.get("power_w") or {}).get("mean"), "sclk_mhz": (sm.get("sclk_mhz") or {}).get("mean")}
        if r:
            st = wl.model.attn_window_stats
            flat = [x for rec in st for row in rec["recall"] for x in row]
            out["layers_calibrated"] = len(st)
            out["heads_windowed"] = sum(sum(rec["windowed"]) for rec in st)
            out["recall_min_mean_max"] = [min(flat), sum(flat) / len(flat), max(flat)] if flat else None
    a, b = out["arms"]["off_first"]["seconds_two_steps"], out["arms"]["off_last"]["seconds_two_steps"]
    out["off_seconds_mean"], out["off_spread_seconds"] = (a + b) / 2, abs(a - b)
    out["calibration_step_cost_seconds"] = out["arms"]["calibration_then_decided"]["seconds_two_steps"] - out["off_seconds_mean"]
    out["calibration_step_cost_over_dense_step"] = out["calibration_step_cost_seconds"] / (out["off_seconds_mean"] / 2)
    kvr = [t for t in wl.model._attn_ranges.values() if t is not None]
    out["coverage"] = kvr[0].coverage if kvr else None
    wl.model.attn_window, wl.model.attn_window_recall = 0, 0.0
    del wl
    gc.collect()
    torch.cuda.empty_cache()
    return out


BAND = 8      # positions on each side in the arms of --family band (the issue's C3 example: about 600 of 32,760 keys)


def kernel_arms_band(name, iters):
    F, hw, valid, rows, heads = SHAPES[name]
    assert not valid and not rows                            # Wan shapes: no prompt tokens in the sequence
    S, D = F * hw, heads * 128
    pad = (S + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(S, 2 * D, generator=g, device=DEV, dtype=BF)
    vt = torch.randn(D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(S, D, dtype=BF, device=DEV)
    qp, kp, op = (torch.empty(S, D, dtype=BF, device=DEV) for _ in range(3))
    vtp = torch.empty(D, pad, dtype=BF, device=DEV)
    scale = 1.0 / 128 ** 0.5
    args = (qk, qk, vt, o, 1, heads, S, S, S * 2 * D, 2 * D, S * 2 * D, 2 * D, D * pad, pad, S * D, D, scale)
    w, half = window_for(F, hw, 0, 0, 0.5)
    band = position_band_ranges(F, hw, BAND)
    every, second = HeadList(range(heads), heads), HeadList(range(0, heads, 2), heads)
    main, _ = head_layout_ranges(half, ["band" if h % 2 == 0 else "dense" for h in range(heads)])
    order = balanced_order(unit_costs(main, 1, heads), "units", heads=heads)
    for t in (half, band, every, second, main, order):
        t.device_table

    def gather(hl):
        Dc = hl.n_sel * 128
        _lib.attn_rows_position_major(qk, qp, hl, 128, 1, F, hw, S * 2 * D, 2 * D, S * Dc, Dc)
        _lib.attn_rows_position_major(qk, kp, hl, 128, 1, F, hw, S * 2 * D, 2 * D, S * Dc, Dc, src_off=D)
        _lib.attn_vt_position_major(vt, vtp, hl, 128, 1, F, hw, D * pad, pad, Dc * pad, pad)

    def band_launch(hl):
        Dc = hl.n_sel * 128
        _lib.flash_attn_d128_ranges(qp, kp, vtp, op, 1, hl.n_sel, S, S, S * Dc, Dc, S * Dc, Dc, Dc * pad, pad, S * Dc, Dc, scale, band)

    def scatter(hl):
        Dc = hl.n_sel * 128
        _lib.attn_rows_position_major(op, o, hl, 128, 1, F, hw, S * Dc, Dc, S * D, D, inverse=True)

    def band_all():
        gather(every), band_launch(every), scatter(every)

    def band_half():
        _lib.flash_attn_d128_ranges_heads(*args, main, k_off=D)
        gather(second), band_launch(second), scatter(second)

    def band_half_ordered():
        _lib.flash_attn_d128_ranges_order(*args, main, order, k_off=D)
        gather(second), band_launch(second), scatter(second)

    dense = lambda: _lib.flash_attn_d128(*args, k_off=D)
    x, y = torch.randn(S, D, generator=g, device=DEV, dtype=BF), torch.randn(S, D, generator=g, device=DEV, dtype=BF)
    xv, yv = torch.randn(D, pad, generator=g, device=DEV, dtype=BF), torch.randn(D, pad, generator=g, device=DEV, dtype=BF)
    rows_bytes, vt_bytes = S * D * 2, D * pad * 2
    arms = [("dense_first", dense, None), ("window_half_coverage", lambda: _lib.flash_attn_d128_ranges(*args, half, k_off=D), None),
            ("band_all_heads", band_all, None), ("band_every_second_head", band_half, None),
            ("band_every_second_head_order_units", band_half_ordered, None),
            ("band_launch_alone_all_heads", lambda: band_launch(every), None),
            ("rows_gather_alone", lambda: _lib.attn_rows_position_major(qk, qp, every, 128, 1, F, hw, S * 2 * D, 2 * D, S * D, D), 2 * rows_bytes),
            ("rows_scatter_alone", lambda: scatter(every), 2 * rows_bytes),
            ("lincomb_2term_inplace_rows_size", lambda: _lib.lincomb([(1.0, x), (1.0, y)], BF, out=x), 3 * rows_bytes),
            ("vt_move_alone", lambda: _lib.attn_vt_position_major(vt, vtp, every, 128, 1, F, hw, D * pad, pad, D * pad, pad), 2 * vt_bytes),
            ("lincomb_2term_inplace_vt_size", lambda: _lib.lincomb([(1.0, xv), (1.0, yv)], BF, out=xv), 3 * vt_bytes),
            ("dense_last", dense, None)]
    out = {"queries": S, "keys": S, "heads": heads, "frames": F, "tokens_per_frame": hw, "attn_band": BAND, "attn_window": w,
           "band_coverage": band.coverage, "window_coverage": half.coverage, "arms": {}}
    gather(every)                                           # the band launch alone reads real operands
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        dense()
        torch.cuda.synchronize()
    for label, fn, nbytes in arms:
        r = timed(fn, iters)
        if nbytes is not None:
            r["bytes_moved"] = nbytes
            r["tb_per_s"] = nbytes / (r["median_ms"] * 1e-3) / 1e12
        out["arms"][label] = r
    ms = lambda k: out["arms"][k]["median_ms"]
    d = out["dense_ms_mean"] = (ms("dense_first") + ms("dense_last")) / 2
    out["dense_spread_ms"] = abs(ms("dense_first") - ms("dense_last"))
    for r in out["arms"].values():
        r["ms_over_dense"] = r["median_ms"] / d
    out["layout_moves_ms_all_heads"] = ms("band_all_heads") - ms("band_launch_alone_all_heads")
    del qk, vt, o, qp, kp, op, vtp, x, y, xv, yv
    torch.cuda.empty_cache()
    return out


def step_arms_band(workload="c3", recall=0.9):
    F, hw, valid, rows, _ = SHAPES[{"c3": "c3_32760x40", "c5": "c5_75600x40"}[workload]]
    w_half = window_for(F, hw, valid, rows, 0.5)[0]
    args = bench.parse_args(["--workload", workload, "--gpus", "1", "--steps", "2", "--warmup", "1"])
    wl = bench.WORKLOADS[workload](args, DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    out = {"attn_window": w_half, "attn_window_recall": recall, "attn_band": BAND, "arms": {}}
    for label, w, r, b in (("off_first", 0, 0.0, 0), ("recall_policy_alone", w_half, recall, 0), ("band_on", w_half, recall, BAND),
                           ("off_last", 0, 0.0, 0)):
        wl.model.attn_window, wl.model.attn_window_recall, wl.model.attn_band = w, r, b
        bench.run_steps(wl, 1)
        torch.cuda.synchronize()
        with bench.SmiSampler(0) as smi:
            t0 = time.perf_counter()
            bench.run_steps(wl, 2)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
        sm = smi.summary() or {}
        arm = out["arms"][label] = {"attn_window": w, "attn_window_recall": r, "attn_band": b, "seconds_two_steps": s,
                                    "finite": bool(torch.isfinite(wl.last_out.float()).all().item()),
                                    "power_w": (sm.get("power_w") or {}).get("mean"), "sclk_mhz": (sm.get("sclk_mhz") or {}).get("mean")}
        if b:
            st = wl.model.attn_window_stats
            flat = [x for rec in st for row in rec["recall_band"] for x in row]
            arm["layers_calibrated"] = len(st)
            arm["layouts"] = {l: sum(rec["layout"].count(l) for rec in st) for l in ("window", "band", "dense")}
            arm["recall_band_min_mean_max"] = [min(flat), sum(flat) / len(flat), max(flat)] if flat else None
    a, b = out["arms"]["off_first"]["seconds_two_steps"], out["arms"]["off_last"]["seconds_two_steps"]
    out["off_seconds_mean"], out["off_spread_seconds"] = (a + b) / 2, abs(a - b)
    for label in ("recall_policy_alone", "band_on"):
        out[label + "_minus_off_seconds"] = out["arms"][label]["seconds_two_steps"] - out["off_seconds_mean"]
    out["band_calibration_cost_over_dense_step"] = ((out["arms"]["band_on"]["seconds_two_steps"]
                                                     - out["arms"]["recall_policy_alone"]["seconds_two_steps"]) / (out["off_seconds_mean"] / 2))
    band = position_band_ranges(F, hw, BAND)
    out["band_coverage"] = band.coverage
    wl.model.attn_window, wl.model.attn_window_recall, wl.model.attn_band = 0, 0.0, 0
    del wl
    gc.collect()
    torch.cuda.empty_cache()
    return out


def widths_for(w_half):
    """The candidate widths of --family widths: 1, 2 and the half-coverage window (a 9-segment profile table)."""
    return (1, 2, w_half) if w_half > 2 else (1, 2, 4)


def kernel_arms_widths(name, iters):
    F, hw, valid, rows, heads = SHAPES[name]
    S, D = F * hw, heads * 128
    Sq, Skv = S + rows, S + valid
    pad = (Sq + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(Sq, 2 * D, generator=g, device=DEV, dtype=BF)
    vt = torch.randn(D, pad, generator=g, device=DEV, dtype=BF)
    o, o2 = torch.empty(Sq, D, dtype=BF, device=DEV), torch.empty(Sq, D, dtype=BF, device=DEV)
    lse_full, lse_part = (torch.empty(heads, Sq, dtype=torch.float32, device=DEV) for _ in range(2))
    args = lambda out: (qk, qk, vt, out, 1, heads, Sq, Skv, Sq * 2 * D, 2 * D, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D, 1.0 / 128 ** 0.5)
    w, half = window_for(F, hw, valid, rows, 0.5)
    widths = widths_for(w)
    full = full_ranges(Sq, Skv)
    seg = frame_profile_segments(F, hw, widths, tail=(S, S + valid) if valid else None, rows=S + rows if rows else None)
    n = seg.segments
    prefix = torch.empty(heads, n, Sq, dtype=torch.float32, device=DEV)
    recall, mass = torch.zeros(heads, dtype=torch.float64, device=DEV), torch.zeros(heads * n, dtype=torch.float64, device=DEV)
    for t in (half, full, seg):
        t.device_table

    def pair(reduce):
        _lib.flash_attn_d128_ranges_heads(*args(o), full, lse=lse_full, k_off=D)
        _lib.flash_attn_d128_ranges_heads(*args(o2), half, lse=lse_part, k_off=D)
        if reduce:
            _lib.attn_lse_recall(lse_part, lse_full, recall, heads, Sq, row0=0, rows=S)

    def one_pass(reduce):
        _lib.flash_attn_d128_ranges_prefix(*args(o), seg, prefix, k_off=D)
        if reduce:
            _lib.attn_prefix_mass(prefix, mass, heads, n, Sq, row0=0, rows=S)

    full_range = lambda: _lib.flash_attn_d128_ranges_heads(*args(o), full, k_off=D)
    arms = [("full_range_first", full_range), ("pair_first", lambda: pair(False)), ("prefix_first", lambda: one_pass(False)),
            ("dense_entry", lambda: _lib.flash_attn_d128(*args(o), k_off=D)),
            ("pair_reduced", lambda: pair(True)), ("prefix_reduced", lambda: one_pass(True)),
            ("prefix_last", lambda: one_pass(False)), ("pair_last", lambda: pair(False)), ("full_range_last", full_range)]
    out = {"queries": Sq, "keys": Skv, "heads": heads, "frames": F, "tokens_per_frame": hw, "attn_window": w, "widths": list(widths),
           "segments": n, "window_coverage": half.coverage, "arms": {}}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        full_range()
        torch.cuda.synchronize()
    for label, fn in arms:
        out["arms"][label] = timed(fn, iters)
    ms = lambda k: out["arms"][k]["median_ms"]
    mean, spread = lambda k: (ms(k + "_first") + ms(k + "_last")) / 2, lambda k: abs(ms(k + "_first") - ms(k + "_last"))
    d, pr, px = mean("full_range"), mean("pair"), mean("prefix")
    out["full_range_ms_mean"], out["pair_ms_mean"], out["prefix_ms_mean"] = d, pr, px
    out["spread_ms"] = {"full_range": spread("full_range"), "pair": spread("pair"), "prefix": spread("prefix")}
    out["prefix_over_pair"], out["prefix_over_full_range"], out["pair_over_full_range"] = px / pr, px / d, pr / d
    out["pair_minus_prefix_ms"] = pr - px
    out["prefix_beats_pair_beyond_spread"] = pr - px > max(out["spread_ms"].values())
    out["reduction_cost_ms"] = {"lse_recall": ms("pair_reduced") - pr, "prefix_mass": ms("prefix_reduced") - px}
    del qk, vt, o, o2, lse_full, lse_part, prefix
    torch.cuda.empty_cache()
    return out


def step_arms_widths(workload, recall=0.9):
    F, hw, valid, rows, _ = SHAPES[{"c3": "c3_32760x40", "c5": "c5_75600x40", "c4": "c4_119056x24"}[workload]]
    w_half = window_for(F, hw, valid, rows, 0.5)[0]
    widths = widths_for(w_half)
    args = bench.parse_args(["--workload", workload, "--gpus", "1", "--steps", "2", "--warmup", "1"])
    wl = bench.WORKLOADS[workload](args, DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    out = {"attn_window": w_half, "attn_window_recall": recall, "attn_window_widths": list(widths), "arms": {}}
    for label, w, r, ws in (("off_first", 0, 0.0, None), ("widths_off_first", w_half, recall, None), ("widths_on", w_half, recall, widths),
                            ("widths_off_last", w_half, recall, None), ("off_last", 0, 0.0, None)):
        wl.model.attn_window, wl.model.attn_window_recall, wl.model.attn_window_widths = w, r, ws
        bench.run_steps(wl, 1)
        torch.cuda.synchronize()
        with bench.SmiSampler(0) as smi:
            t0 = time.perf_counter()
            bench.run_steps(wl, 2)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
        sm = smi.summary() or {}
        out["arms"][label] = {"attn_window": w, "attn_window_recall": r, "attn_window_widths": list(ws) if ws else None,
                              "seconds_two_steps": s, "finite": bool(torch.isfinite(wl.last_out.float()).all().item()),
                              "power_w": (sm.get("power_w") or {}).get("mean"), "sclk_mhz": (sm.get("sclk_mhz") or {}).get("mean")}
        if ws:
            st = wl.model.attn_window_stats
            out["layers_calibrated"] = len(st)
            out["heads_by_width"] = {str(x): sum(rec["width"].count(x) for rec in st) for x in (0,) + tuple(widths)}
            per_width = [[x[j] for rec in st for smp in rec["recall_by_width"] for x in smp] for j in range(len(widths))]
            out["recall_by_width_min_mean_max"] = [[min(v), sum(v) / len(v), max(v)] for v in per_width if v]
    sec = lambda k: out["arms"][k]["seconds_two_steps"]
    off = out["off_seconds_mean"] = (sec("off_first") + sec("off_last")) / 2
    two = out["widths_off_seconds_mean"] = (sec("widths_off_first") + sec("widths_off_last")) / 2
    out["off_spread_seconds"], out["widths_off_spread_seconds"] = abs(sec("off_first") - sec("off_last")), abs(sec("widths_off_first") - sec("widths_off_last"))
    out["two_launch_calibration_cost_over_dense_step"] = (two - off) / (off / 2)
    out["one_pass_calibration_cost_over_dense_step"] = (sec("widths_on") - off) / (off / 2)
    wl.model.attn_window, wl.model.attn_window_recall, wl.model.attn_window_widths = 0, 0.0, None
    del wl
    gc.collect()
    torch.cuda.empty_cache()
    return out


# CogVideoX C2: 226 prompt tokens in front of 13 latent frames of 1,350 tokens, 2 samples x 48 heads
C2_F, C2_HW, C2_T, C2_HEADS, C2_N = 13, 1350, 226, 48, 2


def kernel_arms_d64(iters):
    S, D, N = C2_T + C2_F * C2_HW, C2_HEADS * 64, C2_N
    pad = (S + 127) // 128 * 128
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(N, S, 2 * D, generator=g, device=DEV, dtype=BF)          # the model's layout: Q | K rows, V^T apart
    qk[:, :, :D] *= 0.125 * 1.4426950408889634                                # Q pre-scaled: the scores are in log2 units
    vt = torch.randn(N, D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(N, S, D, dtype=BF, device=DEV)
    args = (qk, qk, vt, o, N, C2_HEADS, S, S * 2 * D, 2 * D, D * pad, pad, S * D, D)
    dense = lambda: _lib.flash_attn_d64(*args, 0.125, k_off=D, q_prescaled=True)
    ranged = lambda t: (lambda: _lib.flash_attn_d64_ranges(*args, t, k_off=D))
    arms = [("dense_first", dense, 1.0, None), ("full_range", ranged(full_ranges(S, S)), 1.0, None)]
    for w in (1, 2, 4):
        t = frame_window_ranges(C2_F, C2_HW, w, prefix=C2_T)
        t.device_table
        arms.append(("attn_window_%d" % w, ranged(t), t.coverage, w))
    arms.append(("dense_last", dense, 1.0, None))
    out = {"samples": N, "tokens": S, "heads": C2_HEADS, "frames": C2_F, "tokens_per_frame": C2_HW, "prompt_tokens": C2_T,
           "dense_form": "alg_flash_attn_d64_ex, ALG_ATTN_Q_PRESCALED, split-KV tail on (workspace %d bytes)"
                         % int(_lib.load_library().alg_flash_attn_d64_workspace_bytes(N, C2_HEADS, S, 1)), "arms": {}}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        dense()
        torch.cuda.synchronize()
    for label, fn, cov, w in arms:
        r = timed(fn, iters)
        r.update(coverage=cov, attn_window=w)
        out["arms"][label] = r
    a, b = out["arms"]["dense_first"]["median_ms"], out["arms"]["dense_last"]["median_ms"]
    d = out["dense_ms_mean"] = (a + b) / 2
    out["dense_spread_ms"] = abs(a - b)
    for r in out["arms"].values():
        r["ms_over_dense"] = r["median_ms"] / d
        r["ms_over_dense_minus_coverage"] = r["ms_over_dense"] - r["coverage"]
    out["full_range_minus_dense_ms"] = out["arms"]["full_range"]["median_ms"] - d
    out["full_range_over_dense"] = out["arms"]["full_range"]["median_ms"] / d    # (no split-KV tail: 1.5-5 % expected, attention.hip)
    out["full_range_within_dense_spread"] = out["full_range_minus_dense_ms"] <= out["dense_spread_ms"]
    del qk, vt, o
    torch.cuda.empty_cache()
    return out


def kernel_arms_heads_d64(iters, window=2):
    S, D, N, heads = C2_T + C2_F * C2_HW, C2_HEADS * 64, C2_N, C2_HEADS
    pad = (S + 127) // 128 * 128
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(N, S, 2 * D, generator=g, device=DEV, dtype=BF)          # the model's layout: Q | K rows, V^T apart
    qk[:, :, :D] *= 0.125 * 1.4426950408889634                                # Q pre-scaled: the scores are in log2 units
    vt = torch.randn(N, D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(N, S, D, dtype=BF, device=DEV)
    lse = torch.empty(N, heads, S, dtype=torch.float32, device=DEV)
    args = (qk, qk, vt, o, N, heads, S, S * 2 * D, 2 * D, D * pad, pad, S * D, D)
    win = frame_window_ranges(C2_F, C2_HW, window, prefix=C2_T)
    full = full_ranges(S, S)
    mixed = head_window_ranges(win, [h % 2 == 0 for h in range(heads)])
    for t in (win, full, mixed):
        t.device_table
    run = lambda t, l: (lambda: _lib.flash_attn_d64_ranges_heads(*args, t, lse=l, k_off=D))
    arms = [("full_range_first", run(full, None), 1.0), ("window_first", run(win, None), win.coverage),
            ("full_range_lse", run(full, lse), 1.0), ("window_lse", run(win, lse), win.coverage),
            ("half_heads_dense", run(mixed, None), mixed.coverage),
            ("shared_entry_window", lambda: _lib.flash_attn_d64_ranges(*args, win, k_off=D), win.coverage),
            ("dense_entry_split_tail", lambda: _lib.flash_attn_d64(*args, 0.125, k_off=D, q_prescaled=True), 1.0),
            ("full_range_last", run(full, None), 1.0), ("window_last", run(win, None), win.coverage)]
    out = {"samples": N, "tokens": S, "heads": heads, "frames": C2_F, "tokens_per_frame": C2_HW, "prompt_tokens": C2_T,
           "attn_window": window, "arms": {}}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        arms[0][1]()
        torch.cuda.synchronize()
    for label, fn, cov in arms:
        r = timed(fn, iters)
        r["coverage"] = cov
        out["arms"][label] = r
    ms = lambda k: out["arms"][k]["median_ms"]
    d = out["full_range_ms_mean"] = (ms("full_range_first") + ms("full_range_last")) / 2
    h = out["window_ms_mean"] = (ms("window_first") + ms("window_last")) / 2
    out["full_range_spread_ms"], out["window_spread_ms"] = abs(ms("full_range_first") - ms("full_range_last")), abs(ms("window_first") - ms("window_last"))
    out["lse_cost_full_range_ms"], out["lse_cost_window_ms"] = ms("full_range_lse") - d, ms("window_lse") - h
    out["half_heads_dense_over_mean_of_both"] = ms("half_heads_dense") / (0.5 * (d + h))
    out["shared_entry_minus_new_entry_window_ms"] = ms("shared_entry_window") - h
    out["full_range_over_dense_entry"] = d / ms("dense_entry_split_tail")
    del qk, vt, o, lse
    torch.cuda.empty_cache()
    return out


def _order_arms(run_heads, run_order, win, full, batch, heads, iters):
    """The arms of --family order for one launch shape.  run_heads(table) / run_order(table, order) -> a launch closure."""
    half = head_window_ranges(win, [h % 2 == 0 for h in range(heads)])          # every second head dense
    quarter = head_window_ranges(win, [h % 4 != 0 for h in range(heads)])       # three of four heads windowed
    order = lambda t, policy: balanced_order(unit_costs(t, batch, heads), policy, heads=heads)
    arms = [("all_dense_first", run_heads(full)), ("all_windowed", run_heads(win)),
            ("half_dense_heads_entry_a", run_heads(half)),
            ("half_dense_natural", run_order(half, order(half, "natural"))),
            ("half_dense_lanes", run_order(half, order(half, "lanes"))),
            ("half_dense_units", run_order(half, order(half, "units"))),
            ("half_dense_heads_entry_b", run_heads(half)),
            ("quarter_dense_natural", run_order(quarter, order(quarter, "natural"))),
            ("quarter_dense_lanes", run_order(quarter, order(quarter, "lanes"))),
            ("quarter_dense_units", run_order(quarter, order(quarter, "units"))),
            ("all_windowed_lanes", run_order(win, order(win, "lanes"))),
            ("all_dense_last", run_heads(full))]
    out = {"coverage_window": win.coverage, "arms": {}}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        arms[0][1]()
        torch.cuda.synchronize()
    for label, fn in arms:
        out["arms"][label] = timed(fn, iters)
    ms = lambda k: out["arms"][k]["median_ms"]
    d = out["all_dense_ms_mean"] = (ms("all_dense_first") + ms("all_dense_last")) / 2
    w = ms("all_windowed")
    out["all_dense_spread_ms"] = abs(ms("all_dense_first") - ms("all_dense_last"))
    out["half_dense_natural_spread_ms"] = abs(ms("half_dense_heads_entry_a") - ms("half_dense_heads_entry_b"))
    nat = out["half_dense_heads_entry_ms_mean"] = (ms("half_dense_heads_entry_a") + ms("half_dense_heads_entry_b")) / 2
    out["indirection_cost_ms"] = ms("half_dense_natural") - nat
    for label, dense_frac in [(k, 0.5) for k in out["arms"] if k.startswith("half_dense")] + \
                             [(k, 0.25) for k in out["arms"] if k.startswith("quarter_dense")]:
        ideal = dense_frac * d + (1.0 - dense_frac) * w        # what the mix costs when every head costs what it costs alone
        r = out["arms"][label]
        r["over_mean_of_both"] = r["median_ms"] / ideal
        r["fraction_of_saving"] = (d - r["median_ms"]) / (d - ideal)
    for k in ("lanes", "units"):
        out["half_dense_%s_gain_ms" % k] = nat - ms("half_dense_" + k)
        out["half_dense_%s_is_a_gain" % k] = out["half_dense_%s_gain_ms" % k] > out["half_dense_natural_spread_ms"]
        out["quarter_dense_%s_gain_ms" % k] = ms("quarter_dense_natural") - ms("quarter_dense_" + k)
    out["all_windowed_lanes_minus_heads_entry_ms"] = ms("all_windowed_lanes") - w
    return out


def kernel_arms_order(name, iters):
    F, hw, valid, rows, heads = SHAPES[name]
    S, D = F * hw, heads * 128
    Sq, Skv = S + rows, S + valid
    pad = (Sq + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(Sq, 2 * D, generator=g, device=DEV, dtype=BF)
    vt = torch.randn(D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(Sq, D, dtype=BF, device=DEV)
    args = (qk, qk, vt, o, 1, heads, Sq, Skv, Sq * 2 * D, 2 * D, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D, 1.0 / 128 ** 0.5)
    w, win = window_for(F, hw, valid, rows, 0.5)

    def run_heads(t):
        t.device_table
        return lambda: _lib.flash_attn_d128_ranges_heads(*args, t, k_off=D)

    def run_order(t, order):
        t.device_table, order.device_table
        return lambda: _lib.flash_attn_d128_ranges_order(*args, t, order, k_off=D)

    out = {"queries": Sq, "keys": Skv, "heads": heads, "frames": F, "tokens_per_frame": hw, "attn_window": w}
    out.update(_order_arms(run_heads, run_order, win, full_ranges(Sq, Skv), 1, heads, iters))
    del qk, vt, o
    torch.cuda.empty_cache()
    return out


def kernel_arms_order_d64(iters, window=2):
    S, D, N, heads = C2_T + C2_F * C2_HW, C2_HEADS * 64, C2_N, C2_HEADS
    pad = (S + 127) // 128 * 128
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = torch.randn(N, S, 2 * D, generator=g, device=DEV, dtype=BF)
    qk[:, :, :D] *= 0.125 * 1.4426950408889634                                # Q pre-scaled: the scores are in log2 units
    vt = torch.randn(N, D, pad, generator=g, device=DEV, dtype=BF)
    o = torch.empty(N, S, D, dtype=BF, device=DEV)
    args = (qk, qk, vt, o, N, heads, S, S * 2 * D, 2 * D, D * pad, pad, S * D, D)
    win = frame_window_ranges(C2_F, C2_HW, window, prefix=C2_T)

    def run_heads(t):
        t.device_table
        return lambda: _lib.flash_attn_d64_ranges_heads(*args, t, k_off=D)

    def run_order(t, order):
        t.device_table, order.device_table
        return lambda: _lib.flash_attn_d64_ranges_order(*args, t, order, k_off=D)

    out = {"samples": N, "tokens": S, "heads": heads, "frames": C2_F, "tokens_per_frame": C2_HW, "prompt_tokens": C2_T,
           "attn_window": window}
    out.update(_order_arms(run_heads, run_order, win, full_ranges(S, S), N, heads, iters))
    del qk, vt, o
    torch.cuda.empty_cache()
    return out


# the workloads' recorded mean recalls (profiles/attn_window_heads_ab.json, attn_window_heads_d64_ab.json): about half the heads window
ORDER_RECALL = {"c3": 0.49, "c5": 0.49, "c4": 0.52, "c2": 0.43}


def step_arms_order(workload, window=None):
    if window is not None:
        w_half = window
    else:
        F, hw, valid, rows, _ = SHAPES[{"c3": "c3_32760x40", "c5": "c5_75600x40", "c4": "c4_119056x24"}[workload]]
        w_half = window_for(F, hw, valid, rows, 0.5)[0]
    recall = ORDER_RECALL[workload]
    args = bench.parse_args(["--workload", workload, "--gpus", "1", "--steps", "2", "--warmup", "1"])
    wl = bench.WORKLOADS[workload](args, DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    wl.model.attn_window, wl.model.attn_window_recall = w_half, recall
    out = {"attn_window": w_half, "attn_window_recall": recall, "arms": {}}
    outs = {}
    # (True is "units"; the "lanes" arm rides along so that the two policies are compared at step level too)
    for label, flag in (("balance_off_first", False), ("balance_on", True), ("balance_lanes", "lanes"), ("balance_off_last", False)):
        wl.model.attn_window_balance = flag
        host0 = wl.model.attn_window_order_build_seconds
        bench.run_steps(wl, 1)
        torch.cuda.synchronize()
        with bench.SmiSampler(0) as smi:
            t0 = time.perf_counter()
            bench.run_steps(wl, 2)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
        sm = smi.summary() or {}
        outs[label] = wl.last_out.float().cpu()
        st = wl.model.attn_window_stats
        mixed = [rec for rec in st if 0 < sum(rec["windowed"]) < len(rec["windowed"])]
        out["arms"][label] = {"attn_window_balance": flag, "seconds_two_steps": s,
                              "finite": bool(torch.isfinite(wl.last_out.float()).all().item()),
                              "layers_calibrated": len(st), "layers_mixed": len(mixed),
                              "fraction_of_heads_windowed": (sum(sum(rec["windowed"]) for rec in st) /
                                                             max(1, sum(len(rec["windowed"]) for rec in st))),
                              "orders_cached": len(wl.model._attn_orders),
                              # host time spent building and uploading launch orders in this arm, its warm-up iteration included;
                              # what of it fell inside the two timed iterations is the calibration forward's share
                              "policy": {False: None, True: "units"}.get(flag, flag),
                              "order_build_host_seconds": wl.model.attn_window_order_build_seconds - host0,
                              "power_w": (sm.get("power_w") or {}).get("mean"), "sclk_mhz": (sm.get("sclk_mhz") or {}).get("mean")}
    a, b = out["arms"]["balance_off_first"]["seconds_two_steps"], out["arms"]["balance_off_last"]["seconds_two_steps"]
    out["off_seconds_mean"], out["off_spread_seconds"] = (a + b) / 2, abs(a - b)
    out["on_minus_off_seconds"] = out["arms"]["balance_on"]["seconds_two_steps"] - out["off_seconds_mean"]
    out["lanes_minus_off_seconds"] = out["arms"]["balance_lanes"]["seconds_two_steps"] - out["off_seconds_mean"]
    # (C4 draws fresh latents from its generator on every call: its runs are different videos)
    fixed = "latents" in wl.kwargs
    out["outputs_bit_identical"] = (bool(all(torch.equal(outs["balance_off_first"], o) for o in outs.values())) if fixed else None)
    wl.model.attn_window, wl.model.attn_window_recall, wl.model.attn_window_balance = 0, 0.0, False
    del wl, outs
    gc.collect()
    torch.cuda.empty_cache()
    return out


def accuracy_cog(frames=9, steps=4, layers=4):
    """A 4-step ALG sampler on the trained-like CogVideoX model at the medium grid (tests/helpers/trained_like_cases.py: 8 heads x
    64) with `layers` blocks, `frames` latent frames of 384 tokens behind 10 prompt tokens."""
    from alg_amd import CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel, CogVideoXTransformerConfig
    from helpers.trained_like import trained_like
    from helpers.trained_like_cases import COG_SMALL
    from oracle import ddim_oracle, dit_oracle, loop_oracle
    H, W, C = 32, 48, 8
    kw = dict(COG_SMALL, sample_width=W, sample_height=H, sample_frames=4 * (frames - 1) + 1, num_layers=layers)
    ocfg = dit_oracle.DiTConfig(**kw)
    wbf = {k: v.to(BF) for k, v in trained_like(dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)).items()}
    model = CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=DEV)
    pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(1, frames, C, H, W, generator=g).to(BF)
    first = (torch.randn(1, 1, C, H, W, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)
    alg = dict(num_inference_steps=steps, guidance_scale=6.0, use_low_pass_guidance=True, lp_filter_type="down_up",
               lp_resize_factor=0.25, lp_strength_schedule_type="interval", schedule_interval_start_time=0.0,
               schedule_interval_end_time=0.3)

    def call():
        return pipe(image=None, image_latents=first, latents=lat, prompt_embeds=pe, negative_prompt_embeds=ne, height=H * 8,
                    width=W * 8, num_frames=4 * (frames - 1) + 1, output_type="latent", lp_filter_in_latent=True,
                    **alg).frames.float().cpu()

    dense = call()
    w32 = {k: v.float() for k, v in wbf.items()}
    cond = torch.zeros(1, frames, C, H, W)
    cond[:, :1] = first.float()
    rope = dit_oracle.rope_tables(ocfg, H * 8, W * 8, frames)
    want = loop_oracle.alg_denoise_loop(lambda x, e, ts, r: dit_oracle.dit_forward(ocfg, w32, x, e, ts, r), ddim_oracle.DDIMOracle(),
                                        lat.float(), cond, pe.float(), ne.float(), image_rotary_emb=rope, **alg)
    return {"model": "trained-like CogVideoX, medium grid (8 heads x 64, %d blocks), 10 prompt tokens + %d latent frames x 384 tokens"
                     % (layers, frames), "steps": steps, "bf16_to_fp32_floor_rel_l2": _rel(dense, want.float()),
            "arms": _window_arms(model, call, frames, dense)}


def step_arms(workload, window=None):
    if workload == "c2":
        w_half = window        # (CogVideoX: the window is given; 2 has a coverage of 0.44 at C2)
    else:
        F, hw, valid, rows, _ = SHAPES[{"c3": "c3_32760x40", "c5": "c5_75600x40", "c4": "c4_119056x24"}[workload]]
        w_half = window_for(F, hw, valid, rows, 0.5)[0]
    args = bench.parse_args(["--workload", workload, "--gpus", "1", "--steps", "2", "--warmup", "1"])
    wl = bench.WORKLOADS[workload](args, DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    out = {"attn_window_half": w_half, "arms": {}}
    outs = {}
    for label, w in (("off_first", 0), ("window_half", w_half), ("off_last", 0)):
        wl.model.attn_window = w
        bench.run_steps(wl, 1)
        torch.cuda.synchronize()
        with bench.SmiSampler(0) as smi:
            t0 = time.perf_counter()
            bench.run_steps(wl, 2)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
        sm = smi.summary() or {}
        outs[label] = wl.last_out.float().cpu()
        out["arms"][label] = {"attn_window": w, "seconds": s, "ms_per_step": s / 2 * 1e3, "frames_per_s": wl.frames * 2 / wl.steps_per_video / s,
                              "finite": bool(torch.isfinite(wl.last_out.float()).all().item()),
                              "power_w": (sm.get("power_w") or {}).get("mean"), "sclk_mhz": (sm.get("sclk_mhz") or {}).get("mean")}
    a, b = out["arms"]["off_first"]["ms_per_step"], out["arms"]["off_last"]["ms_per_step"]
    out["off_ms_per_step_mean"], out["off_spread_ms"] = (a + b) / 2, abs(a - b)
    out["window_half_over_off"] = out["arms"]["window_half"]["ms_per_step"] / out["off_ms_per_step_mean"]
    # (C4 draws fresh latents from its generator on every call: its two dense runs are different videos)
    out["off_first_equals_off_last"] = bool(torch.equal(outs["off_first"], outs["off_last"])) if "latents" in wl.kwargs else None
    kvr = [t for t in wl.model._attn_ranges.values() if t is not None]
    out["coverage"] = kvr[0].coverage if kvr else None
    wl.model.attn_window = 0
    del wl, outs
    gc.collect()
    torch.cuda.empty_cache()
    return out


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _window_arms(model, call, frames, dense):
    arms = {}
    for w in (1, 2, 4):
        model.attn_window = w
        model._attn_ranges.clear()
        got = call()
        kvr = [t for t in model._attn_ranges.values() if t is not None]
        arms["attn_window_%d" % w] = {"rel_l2_vs_dense": _rel(got, dense), "coverage": min((t.coverage for t in kvr), default=1.0)}
    model.attn_window = 0
    return arms


def accuracy_wan(frames=9, steps=4):
    """A 4-step ALG sampler on the trained-like medium Wan model (tests/helpers/trained_like_cases.py: 4 heads x 128, 2 blocks) at
    `frames` latent frames of 384 tokens."""
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    from alg_amd.schedulers import UniPCMultistepScheduler
    from alg_amd.transformer_wan import WanTransformer3DModel, WanTransformerConfig
    from helpers.trained_like_cases import wan_case
    from oracle import loop_oracle, wan_oracle
    from oracle.sched_oracle import UniPCOracle
    kw, ocfg, sd, _ = wan_case("medium")
    model = WanTransformer3DModel(WanTransformerConfig(**kw), sd, device=DEV)
    g = torch.Generator().manual_seed(8)
    H, W = 32, 48
    lat, cond = torch.randn(1, 16, frames, H, W, generator=g), torch.randn(1, 20, frames, H, W, generator=g)
    pe, ne = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 512, 64, generator=g).to(BF)
    ie = torch.randn(1, 257, 64, generator=g).to(BF)
    alg = dict(lp_filter_type="down_up", lp_resize_factor=0.4, lp_strength_schedule_type="interval",
               schedule_interval_start_time=0.0, schedule_interval_end_time=0.3)
    pipe = WanImageToVideoPipeline(transformer=model, scheduler=UniPCMultistepScheduler(flow_shift=3.0)).to(DEV)

    def call():
        return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), image_embeds=ie.to(DEV), image_condition=cond.to(DEV),
                    latents=lat.to(DEV), height=H * 8, width=W * 8, num_frames=4 * (frames - 1) + 1, num_inference_steps=steps,
                    guidance_scale=5.0, output_type="latent", use_low_pass_guidance=True, lp_filter_in_latent=True,
                    **alg).frames.float().cpu()

    dense = call()
    sd32 = {k: v.float() for k, v in sd.items()}
    want = loop_oracle.wan_denoise_loop(lambda x, ts, e, ei: wan_oracle.wan_forward(ocfg, sd32, x.float(), ts.float(), e.float(), ei.float()).to(BF),
                                        UniPCOracle(flow_shift=3.0), lat, cond, pe, ne, ie, steps, guidance_scale=5.0,
                                        use_low_pass_guidance=True, **alg)
    return {"model": "trained-like Wan medium (4 heads x 128, 2 blocks), %d latent frames x 384 tokens" % frames, "steps": steps,
            "bf16_to_fp32_floor_rel_l2": _rel(dense, want.float()), "arms": _window_arms(model, call, frames, dense)}


def accuracy_hunyuan(frames=9, steps=4):
    """A 4-step true-CFG ALG sampler on the trained-like small HunyuanVideo model (1 dual + 1 single block, 4 heads x 128) at `frames`
    latent frames of 256 tokens, prompts of 20 tokens (17 / 9 valid)."""
    from alg_amd import FlowMatchEulerDiscreteScheduler, HunyuanVideoImageToVideoPipeline
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
    from helpers.trained_like_cases import hy_case
    from oracle import hy_oracle, loop_oracle
    from oracle.sched_oracle import FlowMatchEulerOracle
    kw, ocfg, sd, _ = hy_case("token_replace")
    sd32 = {k: v.float() for k, v in sd.items()}
    model = HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(**kw), sd, device=DEV)
    g = torch.Generator().manual_seed(8)
    H = W = 32
    lat, img = torch.randn(1, 16, frames, H, W, generator=g), torch.randn(1, 16, 1, H, W, generator=g)
    mk = lambda v: (torch.randn(1, 20, 64, generator=g).to(BF), torch.randn(1, 64, generator=g).to(BF),
                    torch.cat([torch.ones(1, v), torch.zeros(1, 20 - v)], dim=1).to(BF))
    pos, neg = mk(17), mk(9)
    alg = dict(lp_filter_type="down_up", lp_resize_factor=0.625, lp_strength_schedule_type="interval",
               schedule_interval_start_time=0.0, schedule_interval_end_time=0.3)
    pipe = HunyuanVideoImageToVideoPipeline(transformer=model, scheduler=FlowMatchEulerDiscreteScheduler(shift=7.0)).to(DEV)
    d = lambda t_: t_.to(DEV)

    def call():
        return pipe(prompt_embeds=d(pos[0]), pooled_prompt_embeds=d(pos[1]), prompt_attention_mask=d(pos[2]),
                    negative_prompt_embeds=d(neg[0]), negative_pooled_prompt_embeds=d(neg[1]),
                    negative_prompt_attention_mask=d(neg[2]), negative_prompt=None, image_latents=d(img), latents=d(lat),
                    height=H * 8, width=W * 8, num_frames=4 * (frames - 1) + 1, num_inference_steps=steps, true_cfg_scale=6.0,
                    guidance_scale=1.0, output_type="latent", use_low_pass_guidance=True, lp_filter_in_latent=True,
                    **alg).frames[:, :, 1:].float().cpu()

    dense = call()
    want = loop_oracle.hunyuan_denoise_loop(
        lambda x, ts, e, m, p_, g_: hy_oracle.hy_forward(ocfg, sd32, x.float(), ts.float(), e.float(), m.float(), p_.float(), None).to(BF),
        FlowMatchEulerOracle(shift=7.0), lat, img, pos, neg, steps, true_cfg_scale=6.0, guidance_scale=1.0,
        use_low_pass_guidance=True, guidance_embeds=False, **alg)[:, :, 1:]
    return {"model": "trained-like HunyuanVideo small config (4 heads x 128, 1 dual + 1 single block), %d latent frames x 256 tokens"
                     % frames, "steps": steps, "bf16_to_fp32_floor_rel_l2": _rel(dense, want.float()),
            "arms": _window_arms(model, call, frames, dense)}


def accuracy():
    return {"wan": accuracy_wan(), "hunyuan": accuracy_hunyuan()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", choices=["kernel", "steps", "accuracy"], action="append")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--family", choices=["d128", "d64", "heads", "heads64", "order", "widths", "band"], default="d128",
                    help="d128: Wan / HunyuanVideo; d64: CogVideoX (C2); heads: the per-head window chosen by recall (d = 128); "
                         "heads64: the same for d = 64 (CogVideoX, C2); order: the coverage-balanced launch order (both head dims); "
                         "widths: the per-head window width from one calibration pass (d = 128); band: the position-major band "
                         "of Wan attn1 (C3 and C5 kernel arms, C3 steps)")
    ap.add_argument("--workloads", default="c3,c5,c4", help="--family heads / order: the workloads of the steps arms")
    ap.add_argument("--shapes", default=",".join(list(SHAPES) + ["c2_2x48x17776"]), help="--family order: the kernel arms' launch shapes")
    a = ap.parse_args()
    parts = a.only or ["kernel", "accuracy", "steps"]
    res = {}
    if os.path.exists(a.out):
        res = json.load(open(a.out))
    res["device"] = torch.cuda.get_device_name(0)
    res["weights"] = "synthetic; the accuracy arms bound nothing on a trained checkpoint and visual quality is unmeasured"

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    if a.family == "band":
        res["weights"] = ("synthetic Gaussian: the band's recall sits near its coverage, so every head stays dense; hit rates and "
                          "quality on a trained checkpoint are unmeasured")
        if "kernel" in parts:
            res.setdefault("kernel", {})
            for name in ("c3_32760x40", "c5_75600x40"):
                res["kernel"][name] = kernel_arms_band(name, a.iters)
                save()
        if "steps" in parts:
            res["steps"] = {"c3": step_arms_band("c3")}
            save()
        print(json.dumps(res))
        return
    if a.family == "order":
        res["weights"] = ("synthetic Gaussian: which heads window on a trained checkpoint, and so the mix a layer has, is unmeasured; the "
                          "kernel arms fix the mix (every second head dense, three of four windowed)")
        if "kernel" in parts:
            res.setdefault("kernel", {})
            for name in a.shapes.split(","):
                res["kernel"][name] = kernel_arms_order_d64(a.iters) if name.startswith("c2") else kernel_arms_order(name, a.iters)
                save()
        if "steps" in parts:
            res.setdefault("steps", {})
            for wlname in a.workloads.split(","):
                res["steps"][wlname] = step_arms_order(wlname, window=2 if wlname == "c2" else None)
                save()
        print(json.dumps(res))
        return
    if a.family == "widths":
        res["weights"] = ("synthetic Gaussian: recall is about the coverage, so no head reaches a threshold above it and the later "
                          "steps run dense; which widths the heads of a trained checkpoint choose, and the quality, are unmeasured")
        if "kernel" in parts:
            res.setdefault("kernel", {})
            for name in [n for n in a.shapes.split(",") if n in SHAPES]:
                res["kernel"][name] = kernel_arms_widths(name, a.iters)
                save()
        if "steps" in parts:
            res.setdefault("steps", {})
            for wlname in a.workloads.split(","):
                res["steps"][wlname] = step_arms_widths(wlname)
                save()
        print(json.dumps(res))
        return
    if a.family == "heads64":
        res["weights"] = ("synthetic Gaussian: recall is about the coverage, so no head reaches a threshold above it; hit rates and "
                          "quality on a trained checkpoint are unmeasured")
        if "kernel" in parts:
            res["kernel"] = {"c2_2x48x17776": kernel_arms_heads_d64(a.iters)}
            save()
        if "steps" in parts:
            res["steps"] = {"c2": step_arms_heads("c2", window=2)}
            save()
        print(json.dumps(res))
        return
    if a.family == "heads":
        res["weights"] = ("synthetic Gaussian: recall is about the coverage, so no head reaches a threshold above it; hit rates and "
                          "quality on a trained checkpoint are unmeasured")
        if "kernel" in parts:
            res.setdefault("kernel", {})
            for name in SHAPES:
                res["kernel"][name] = kernel_arms_heads(name, a.iters)
                save()
        if "steps" in parts:
            res.setdefault("steps", {})
            for wlname in a.workloads.split(","):
                res["steps"][wlname] = step_arms_heads(wlname)
                save()
        print(json.dumps(res))
        return
    if a.family == "d64":
        if "kernel" in parts:
            res["kernel"] = {"c2_2x48x17776": kernel_arms_d64(a.iters)}
            save()
        if "accuracy" in parts:
            res["accuracy"] = {"cogvideox": accuracy_cog()}
            save()
        if "steps" in parts:
            res["steps"] = {"c2": step_arms("c2", window=2)}
            save()
        print(json.dumps(res))
        return
    if "kernel" in parts:
        res["kernel"] = {}
        for name in SHAPES:
            res["kernel"][name] = kernel_arms(name, a.iters)
            save()
    if "accuracy" in parts:
        res["accuracy"] = accuracy()
        save()
    if "steps" in parts:
        res["steps"] = {}
        for wlname in ("c3", "c5", "c4"):
            res["steps"][wlname] = step_arms(wlname)
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
