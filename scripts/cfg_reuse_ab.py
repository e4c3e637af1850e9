"""Measurements of the opt-in CFG reuse (alg_amd/cfg_reuse.py) on one GPU, written as one JSON file (profiles/cfg_reuse_ab.json is
a run of this).  One job; every arm in a fresh process, one after the other, arms alternated (off first and last); every step
timed on its own with device events; package power and clock per arm.

    python scripts/cfg_reuse_ab.py --out profiles/cfg_reuse_ab.json [--only deviation,c2,c2_both,c3] [--steps 50] [--layers N]

  c2           the C2 workload of bench.py (synthetic weights) through the pipeline's __call__, a whole 50-step video per arm: off,
               cfg_reuse = 2, cfg_reuse = 3, off (range 100 < t < 800, the default).  A device event behind every step; the steps are
               classed by (scheduled passes, reused): ms per computed and per reused step, a reused step against a computed two-pass
               step of the off arms, an armed computed step (the STORE form of the fused step) against the same step of the off
               arms, next to the spread between the two off arms; the reused steps counted against the rule's own count
  c2_both      the same arms with attn_reuse = 2 in every armed one (both reuses together); reported only
  c3           the two-iteration window of the bench workload (Wan 480p), entered at the schedule's first two-pass iteration as
               bench.py's own two-pass window is: off, on with a range that holds every timestep (the first iteration computes
               and writes the delta, the second reuses it), off.  (C4 runs without CFG and C5 under
               cfg_split: the switch refuses both.)
  deviation    a 10-step ALG sampler on the trained-like medium CogVideoX model (tests/helpers/trained_like_cases.py, 4 layers):
               relative L2 distance of the final latents at N = 2 and N = 3 against the off run, next to the distance of the off
               run to the fp32 loop oracle (the bf16-to-fp32 floor of that run), and the drift per computed step

No bound is set in advance.  Synthetic weights say nothing about how far a trained checkpoint's CFG delta moves between steps;
nothing here measures visual quality."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

EVERYWHERE = (-1, 1000000)      # a range that holds every timestep
MARK = "ARM-RECORD "


def by_the_rule(records, every, lo, hi):
    from alg_amd.cfg_reuse import CfgReuse
    rule, out = CfgReuse(every, lo, hi), []
    for r in records:
        rule.advance()
        hit = rule.decide(r["n_pass"], r["t"], r["forced"])
        if not hit and r["n_pass"] == 2:
            rule.mark_written()
        out.append(hit)
    return out


def run_video(wl, steps, dev, first=0):
    """`steps` loop iterations of one video through pipe.__call__, from iteration `first` on (the pipeline's `_first_step`), a
    device event behind every step: [{"ms", "passes", "reused"}], total seconds, power and clock, the rule's records"""
    import bench
    import torch
    events, trace = [torch.cuda.Event(enable_timing=True)], []

    def cb(pipe, i, t, kw):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        events.append(ev)
        if i + 1 >= first + steps:
            pipe._interrupt = True
        return {}

    if first:
        wl.pipe._first_step = first
    smi = bench.SmiSampler(dev.index or 0)
    smi.__enter__()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    events[0].record()
    try:
        wl.last_out = wl.pipe(callback_on_step_end=cb, step_trace=trace, **wl.kwargs).frames
        torch.cuda.synchronize()
    finally:
        smi.__exit__(None, None, None)
        if first:
            wl.pipe._first_step = 0
    total = time.perf_counter() - t0
    st = list(wl.model.cfg_reuse_stats) if wl.model.cfg_reuse else []
    st = st[-len(trace):]           # (a window that starts behind step 0 records the steps it runs)
    per = []
    for i in range(len(events) - 1):
        ran = next((v for v in trace[i][1:] if isinstance(v, int) and not isinstance(v, bool)), None)
        reused = bool(st[i]["reused"]) if i < len(st) else False
        per.append({"ms": events[i].elapsed_time(events[i + 1]), "passes": 2 if reused else ran, "reused": reused})
    sm = smi.summary()
    box = {"power_w": round(sm["power_w"]["mean"], 1), "sclk_mhz": round(sm["sclk_mhz"]["mean"], 1)} if sm and sm.get("power_w") and sm.get("sclk_mhz") else None
    return per, total, box, st


def classes(per, skip_first=True):
    """median ms per (passes, reused) class; the first step of a video carries the pipeline's set-up and is left out"""
    by = {}
    for r in per[1:] if skip_first else per:
        by.setdefault("%s-pass %s" % (r["passes"], "reused" if r["reused"] else "computed"), []).append(r["ms"])
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)} for k, v in sorted(by.items())}


def one_arm(a):
    """The child: build the workload, warm up, run one arm, print its record."""
    import bench
    import torch
    dev = torch.device("cuda:0")
    name = "c2" if a.part.startswith("c2") else a.part
    argv = ["--workload", name, "--gpus", "1"] + (["--layers", str(a.layers)] if a.layers else [])
    wl = bench.WORKLOADS[name](bench.parse_args(argv), dev, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    lo, hi = (int(v) for v in a.range.split(","))
    # c3: the loop is entered at the schedule's first two-pass iteration, as bench.py's own two-pass window is
    first = bench.schedule_passes(wl).index(2) if name == "c3" else 0

    def switches(cfg, attn):
        wl.model.cfg_reuse, wl.model.cfg_reuse_t_lo, wl.model.cfg_reuse_t_hi = cfg, lo, hi
        wl.model.attn_reuse, wl.model.attn_reuse_t_lo, wl.model.attn_reuse_t_hi = attn, lo, hi

    switches(0, 0)
    run_video(wl, min(a.steps, 4), dev, first)                      # warm-up: the workspaces of the pass counts this window runs
    if a.cfg or a.attn:
        switches(a.cfg, a.attn)
        wl.model.cfg_reuse_t_lo, wl.model.cfg_reuse_t_hi = wl.model.attn_reuse_t_lo, wl.model.attn_reuse_t_hi = EVERYWHERE
        run_video(wl, min(a.steps, 4), dev, first)                  # ... the one-sample workspace, the delta, the attention entries
        switches(a.cfg, a.attn)
    per, total, box, st = run_video(wl, a.steps, dev, first)
    rec = {"cfg_reuse": a.cfg, "attn_reuse": a.attn, "range": [lo, hi], "steps": len(per), "seconds": total,
           "ms_per_step": sum(r["ms"] for r in per) / max(len(per), 1), "wall_ms_per_step": total / max(len(per), 1) * 1e3,
           "classes": classes(per, skip_first=a.steps > 2), "box": box,
           "reused": "".join("T" if r["reused"] else "F" for r in per), "reused_steps": sum(r["reused"] for r in per),
           "reused_steps_by_the_rule": sum(by_the_rule(st, a.cfg, lo, hi)) if a.cfg else 0,
           "step_ms": [round(r["ms"], 2) for r in per], "cfg_reuse_bytes": wl.model.cfg_reuse_bytes,
           "attn_reuse_bytes": wl.model.attn_reuse_bytes, "layers": wl.layers, "tokens": wl.config(0)["tokens"],
           "peak_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1), "device": torch.cuda.get_device_name(0),
           "finite": bool(torch.isfinite(wl.last_out.float()).all().item())}
    print(MARK + json.dumps(rec), flush=True)


def child(extra):
    """One arm in a fresh process (the parent never opens the GPU)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", "-"] + extra, capture_output=True, text=True, cwd=ROOT, timeout=900)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith(MARK)), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("arm %r failed with exit status %d" % (extra, r.returncode))
    return json.loads(line[len(MARK):])


def summarise(res, on_names):
    off = [res["arms"]["off_first"], res["arms"]["off_last"]]
    mean_off = sum(a["ms_per_step"] for a in off) / 2
    res["off_ms_per_step_mean"] = mean_off
    res["off_spread_pct"] = abs(off[0]["ms_per_step"] - off[1]["ms_per_step"]) / mean_off * 100
    for name in on_names:
        a = res["arms"][name]
        a["video_time_over_off"] = a["ms_per_step"] / mean_off
        fill = {}
        for k, v in a["classes"].items():
            c = k.replace("reused", "computed")
            if not all(c in o["classes"] for o in off):
                continue
            ref = sum(o["classes"][c]["median_ms"] for o in off) / 2
            spread = abs(off[0]["classes"][c]["median_ms"] - off[1]["classes"][c]["median_ms"]) / ref * 100
            if k.endswith("computed"):
                fill[k] = {"armed_ms": v["median_ms"], "off_ms": ref, "delta_pct": (v["median_ms"] - ref) / ref * 100, "off_arms_spread_pct": spread}
            else:
                fill[k] = {"reused_ms": v["median_ms"], "off_computed_ms": ref, "reused_over_computed": v["median_ms"] / ref,
                           "off_arms_spread_pct": spread}
        a["against_off"] = fill


def workload(part, steps, layers, arms):
    res = {"arms": {}}
    for tag, cfg, attn, rng in arms:
        res["arms"][tag] = child(["--arm", tag, "--part", part, "--cfg", str(cfg), "--attn", str(attn), "--range=%d,%d" % rng,
                                  "--steps", str(steps), "--layers", str(layers)])
        print(part, tag, "%.1f ms per step" % res["arms"][tag]["ms_per_step"], res["arms"][tag]["reused"], flush=True)
    summarise(res, [t for t, c, m, _ in arms if c or m])
    return res


def deviation(steps=10, layers=4):
    import torch
    from helpers.trained_like import trained_like
    from helpers.trained_like_cases import COG, COG_SMALL
    from alg_amd import CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel, CogVideoXTransformerConfig
    from oracle import ddim_oracle, dit_oracle, loop_oracle
    BF, dev = torch.bfloat16, torch.device("cuda:0")
    kw = dict(COG_SMALL, **COG["medium"][0])
    kw["num_layers"] = layers
    ocfg = dit_oracle.DiTConfig(**kw)
    wbf = {k: v.to(BF) for k, v in trained_like(dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)).items()}
    model = CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=dev)
    g = torch.Generator().manual_seed(42)
    Fr, C, H, W = 3, 8, 32, 48
    latents = torch.randn(1, Fr, C, H, W, generator=g).to(BF)
    first = (torch.randn(1, 1, C, H, W, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)
    alg = dict(num_inference_steps=steps, guidance_scale=6.0, use_low_pass_guidance=True, lp_filter_type="down_up",
               lp_resize_factor=0.25, lp_strength_schedule_type="linear")

    def run():
        pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(dev)
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
           "bf16_to_fp32_floor_rel_l2": rel(off, ref.float()), "arms": {}, "device": torch.cuda.get_device_name(0)}
    model.cfg_reuse_drift = True
    for every, rng in ((2, (100, 800)), (3, (100, 800)), (2, EVERYWHERE), (3, EVERYWHERE)):
        model.cfg_reuse, model.cfg_reuse_t_lo, model.cfg_reuse_t_hi = (every,) + rng
        got = run()
        st = model.cfg_reuse_stats
        out["arms"]["cfg_reuse_%d_range_%d_%d" % ((every,) + rng)] = {
            "rel_l2_vs_off": rel(got, off), "reused": "".join("T" if r["reused"] else "F" for r in st), "t": [r["t"] for r in st],
            "n_pass": [r["n_pass"] for r in st], "drift": [round(r["drift"], 4) if "drift" in r else None for r in st]}
    model.cfg_reuse, model.cfg_reuse_drift = 0, False
    print(MARK + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="deviation,c2,c2_both,c3")
    ap.add_argument("--steps", type=int, default=50, help="loop iterations per C2 arm (50 = a whole video)")
    ap.add_argument("--layers", type=int, default=0, help="debug: the workloads with fewer blocks")
    ap.add_argument("--arm", default=None, help="(internal) run one arm in this process and print its record")
    ap.add_argument("--part", default=None)
    ap.add_argument("--cfg", type=int, default=0)
    ap.add_argument("--attn", type=int, default=0)
    ap.add_argument("--range", default="100,800")
    a = ap.parse_args()
    if a.arm == "deviation":
        return deviation()
    if a.arm is not None:
        return one_arm(a)
    res = {"weights": "synthetic (seeded Gaussian; the deviation run: trained-like); says nothing about a trained checkpoint's drift",
           "timing": "device events behind every step; every arm in a fresh process"}
    if os.path.exists(a.out):      # parts measured by an earlier call of the same job are kept
        with open(a.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    R = (100, 800)
    for part in a.only.split(","):
        if part == "deviation":
            res["deviation"] = child(["--arm", "deviation"])
        elif part == "c2":
            res["c2"] = workload("c2", a.steps, a.layers, [("off_first", 0, 0, R), ("every_2", 2, 0, R), ("every_3", 3, 0, R), ("off_last", 0, 0, R)])
        elif part == "c2_both":
            res["c2_both"] = workload("c2_both", a.steps, a.layers, [("off_first", 0, 0, R), ("attn_2_cfg_2", 2, 2, R), ("attn_2_cfg_3", 3, 2, R),
                                                                     ("off_last", 0, 0, R)])
        elif part == "c3":
            res["c3"] = workload("c3", 2, a.layers, [("off_first", 0, 0, EVERYWHERE), ("on", 2, 0, EVERYWHERE), ("off_last", 0, 0, EVERYWHERE)])
        else:
            raise SystemExit("--only: unknown part %r" % part)
        save()
        print(part, "done", flush=True)


if __name__ == "__main__":
    main()
