"""Measurements of the opt-in attention reuse (alg_amd/attn_reuse.py) on one GPU, written as one JSON file
(profiles/attn_reuse_ab.json is a run of this).  One job, arms alternated in one process, package power and clock per arm.

    python scripts/attn_reuse_ab.py --out profiles/attn_reuse_ab.json [--only c2,c3,c4,c5,deviation] [--steps 50] [--layers N]

  c2           the C2 workload of bench.py (synthetic weights) through the pipeline's __call__, a whole 50-step video per arm: off,
               attn_reuse = 2, attn_reuse = 3, off (range 100 < t < 800, the default).  Every step is timed on its own (a stream
               synchronisation in callback_on_step_end) and classed by (passes, reused): ms per computed and per reused step, the
               share of reused steps, attn_reuse_bytes, and the cost of filling the cache -- a computed step of an armed run
               against the same class of step of the off runs, next to the spread of the two off arms
  c3 c4 c5     the two-iteration window of the bench workloads: off, on with a range that holds every timestep (iteration 0 is the
               first forward of a video and computes, iteration 1 reuses), off
  deviation    a 10-step ALG sampler on the trained-like medium CogVideoX model (tests/helpers/trained_like_cases.py, 4 layers):
               relative L2 distance of the final latents, reuse on against off, next to the distance of the off run to the fp32
               loop oracle (the bf16-to-fp32 floor of that run); with attn_reuse_drift the per-step drift of that run

No bound is set in advance.  Synthetic weights say nothing about how far a trained checkpoint's attention moves between steps;
nothing here measures visual quality."""
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

BF = torch.bfloat16
DEV = torch.device("cuda:0")
EVERYWHERE = (-1, 1000000)      # a range that holds every timestep


def run_video(wl, steps):
    """`steps` loop iterations of one video through pipe.__call__, every step timed: [{"ms", "passes", "reused"}], total seconds"""
    import bench
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
    st = list(getattr(wl.model, "attn_reuse_stats", [])) if getattr(wl.model, "attn_reuse", 0) else []
    per = []
    for i, m in enumerate(marks):
        per.append({"ms": (m - (marks[i - 1] if i else t0)) * 1e3, "passes": next((v for v in trace[i][1:] if isinstance(v, int) and not isinstance(v, bool)), None),
                    "reused": bool(st[i]["reused"]) if i < len(st) else False})
    sm = smi.summary()
    box = {"power_w": round(sm["power_w"]["mean"], 1), "sclk_mhz": round(sm["sclk_mhz"]["mean"], 1)} if sm and sm.get("power_w") and sm.get("sclk_mhz") else None
    return per, total, box


def classes(per, skip_first=True):
    """median ms per (passes, reused) class; the first step of a video carries the pipeline's set-up and is left out"""
    by = {}
    for r in per[1:] if skip_first else per:
        by.setdefault("%s-pass %s" % (r["passes"], "reused" if r["reused"] else "computed"), []).append(r["ms"])
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)} for k, v in sorted(by.items())}


def arm(wl, steps, every, rng):
    wl.model.attn_reuse = every
    if rng is not None:
        wl.model.attn_reuse_t_lo, wl.model.attn_reuse_t_hi = rng
    per, total, box = run_video(wl, steps)
    rec = {"attn_reuse": every, "range": [wl.model.attn_reuse_t_lo, wl.model.attn_reuse_t_hi], "steps": len(per), "seconds": total,
           "ms_per_step": total / max(len(per), 1) * 1e3, "classes": classes(per, skip_first=steps > 2), "box": box,
           "reused": "".join("T" if r["reused"] else "F" for r in per), "reused_share": sum(r["reused"] for r in per) / max(len(per), 1),
           "step_ms": [round(r["ms"], 2) for r in per], "attn_reuse_bytes": wl.model.attn_reuse_bytes,
           "finite": bool(torch.isfinite(wl.last_out.float()).all().item())}
    return rec


def summarise(res, on_names):
    off = [res["arms"]["off_first"], res["arms"]["off_last"]]
    mean_off = sum(a["ms_per_step"] for a in off) / 2
    res["off_ms_per_step_mean"] = mean_off
    res["off_spread_pct"] = abs(off[0]["ms_per_step"] - off[1]["ms_per_step"]) / mean_off * 100
    for name in on_names:
        a = res["arms"][name]
        a["over_off"] = a["ms_per_step"] / mean_off
        fill = {}
        for k, v in a["classes"].items():
            if k.endswith("computed") and all(k in o["classes"] for o in off):
                ref = sum(o["classes"][k]["median_ms"] for o in off) / 2
                fill[k] = {"armed_ms": v["median_ms"], "off_ms": ref, "delta_pct": (v["median_ms"] - ref) / ref * 100,
                           "off_arms_spread_pct": abs(off[0]["classes"][k]["median_ms"] - off[1]["classes"][k]["median_ms"]) / ref * 100}
            if k.endswith("reused"):
                c = k.replace("reused", "computed")
                if all(c in o["classes"] for o in off):
                    ref = sum(o["classes"][c]["median_ms"] for o in off) / 2
                    fill[k] = {"reused_ms": v["median_ms"], "off_computed_ms": ref, "reused_over_computed": v["median_ms"] / ref}
        a["against_off"] = fill


def workload(name, steps, layers, arms):
    import bench
    argv = ["--workload", name, "--gpus", "1"] + (["--layers", str(layers)] if layers else [])
    wl = bench.WORKLOADS[name](bench.parse_args(argv), DEV, 0, 1, None)
    t0 = time.perf_counter()
    wl.build()
    torch.cuda.synchronize()
    res = {"layers": wl.layers, "tokens": wl.config(0)["tokens"], "build_seconds": round(time.perf_counter() - t0, 1), "arms": {}}
    arm(wl, min(steps, 4), 0, None)                           # warm-up: the workspaces of both pass counts
    arm(wl, min(steps, 4), 2, EVERYWHERE)                     # ... and the cache's entries
    for tag, every, rng in arms:
        res["arms"][tag] = arm(wl, steps, every, rng)
    wl.model.attn_reuse = 0
    summarise(res, [t for t, e, _ in arms if e])
    res["peak_gib"] = round(torch.cuda.max_memory_allocated(DEV) / 2 ** 30, 1)
    del wl
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    return res


def deviation(steps=10, layers=4):
    from helpers.trained_like import trained_like
    from helpers.trained_like_cases import COG, COG_SMALL
    from alg_amd import CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel, CogVideoXTransformerConfig
    from oracle import ddim_oracle, dit_oracle, loop_oracle
    kw = dict(COG_SMALL, **COG["medium"][0])
    kw["num_layers"] = layers
    ocfg = dit_oracle.DiTConfig(**kw)
    wbf = {k: v.to(BF) for k, v in trained_like(dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)).items()}
    model = CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=DEV)
    g = torch.Generator().manual_seed(42)
    Fr, C, H, W = 3, 8, 32, 48
    latents = torch.randn(1, Fr, C, H, W, generator=g).to(BF)
    first = (torch.randn(1, 1, C, H, W, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)
    alg = dict(num_inference_steps=steps, guidance_scale=6.0, use_low_pass_guidance=True, lp_filter_type="down_up",
               lp_resize_factor=0.25, lp_strength_schedule_type="linear")

    def run():
        pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
        return pipe(image_latents=first, latents=latents, prompt_embeds=pe, negative_prompt_embeds=ne, height=H * 8, width=W * 8,
                    num_frames=9, output_type="latent", lp_filter_in_latent=True, **alg).frames.float().cpu()

    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    off = run()
    cond = torch.zeros(1, Fr, C, H, W)
    cond[:, :1] = first.float()
    w32 = {k: v.float() for k, v in wbf.items()}
    rope = dit_oracle.rope_tables(ocfg, H * 8, W * 8, Fr)
    ref = loop_oracle.alg_denoise_loop(lambda x, e, ts, r: dit_oracle.dit_forward(ocfg, w32, x, e, ts, r), ddim_oracle.DDIMOracle(),
                                       latents.float(), cond, pe.float(), ne.float(), image_rotary_emb=rope, **alg)
    out = {"model": "trained-like CogVideoX medium (1,162 tokens, 8 heads x 64), %d layers" % layers, "steps": steps,
           "bf16_to_fp32_floor_rel_l2": rel(off, ref.float()), "arms": {}}
    model.attn_reuse_drift = True
    for every in (2, 3):
        model.attn_reuse = every
        got = run()
        st = model.attn_reuse_stats
        out["arms"]["attn_reuse_%d" % every] = {
            "rel_l2_vs_off": rel(got, off), "reused": "".join("T" if r["reused"] else "F" for r in st), "t": [r["t"] for r in st],
            "drift_max_over_keys_and_layers": [round(max(max(k) for k in r["drift"]), 4) if "drift" in r else None for r in st]}
    model.attn_reuse, model.attn_reuse_drift = 0, False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="deviation,c2,c3,c4,c5")
    ap.add_argument("--steps", type=int, default=50, help="loop iterations per C2 arm (50 = a whole video)")
    ap.add_argument("--layers", type=int, default=0, help="debug: the workloads with fewer blocks")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0),
           "weights": "synthetic (seeded Gaussian; the deviation run: trained-like); says nothing about a trained checkpoint's drift"}
    if os.path.exists(a.out):      # parts measured by an earlier call of the same job are kept
        with open(a.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    for part in a.only.split(","):
        if part == "deviation":
            res["deviation"] = deviation()
        elif part == "c2":
            res["c2"] = workload("c2", a.steps, a.layers, [("off_first", 0, None), ("every_2", 2, (100, 800)), ("every_3", 3, (100, 800)),
                                                           ("off_last", 0, None)])
        elif part in ("c3", "c4", "c5"):
            res[part] = workload(part, 2, a.layers, [("off_first", 0, None), ("on", 2, EVERYWHERE), ("off_last", 0, None)])
        else:
            raise SystemExit("--only: unknown part %r" % part)
        save()
        print(part, "done", flush=True)


if __name__ == "__main__":
    main()
