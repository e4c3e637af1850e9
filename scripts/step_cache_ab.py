"""Measurements of the opt-in step cache on one GPU, written as one JSON file (profiles/step_cache_ab.json is a run of this).

    python scripts/step_cache_ab.py --out profiles/step_cache_ab.json [--skip-c2] [--steps 50]

  probe        alg_step_cache_probe against alg_lincomb (2-term in-place bf16 add) on the same tensor: achieved bytes / s of both
               at the C2 shape (17,776 x 3,072) and at Wan C5's (75,600 x 5,120); the probe moves 5 S D 2 bytes, the add 3 S D 2
  round_trip   milliseconds from the first probe launch of a forward to the decision on the host (probes of all samples, the copy
               of the sums, the stream synchronisation, `decide`), next to the GPU time of the probes alone
  c2           the C2 workload of bench.py (synthetic weights) through the pipeline's __call__, arms alternated in one process:
               off, step_cache = 1e30 with step_cache_max_consecutive = 1 (every other step skipped, whatever the data), and
               thresholds 0.05 / 0.1 / 0.2 -- seconds, ms per step, frames / s and the hit fraction of each
  deviation    a 10-step ALG sampler on the trained-like medium CogVideoX model (tests/helpers/trained_like_cases.py, 4 layers):
               relative L2 distance of the final latents, cache on against cache off, next to the distance of the cache-off run to
               the fp32 loop oracle (the bf16-to-fp32 floor of that run)

Hit rates on Gaussian weights say nothing about a trained checkpoint; nothing here measures visual quality."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from alg_amd import _lib  # noqa: E402
from alg_amd.step_cache import StepCache  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda:0")


def event_ms(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "iters": iters}


def probe_vs_lincomb(S, D, tok0):
    g = torch.Generator(device=DEV).manual_seed(0)
    keep, x, r, t = (torch.randn(S, D, generator=g, device=DEV).to(BF) for _ in range(4))
    work = torch.empty(_lib.step_cache_workspace_bytes(S, D), dtype=torch.uint8, device=DEV)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    probe = event_ms(lambda: _lib.step_cache_probe(keep, x, r, S, D, tok0, S - tok0, work, sums))
    add = event_ms(lambda: _lib.lincomb([(1.0, x), (1.0, t)], BF, out=x))
    copy = event_ms(lambda: keep.copy_(x))
    nb = S * D * 2
    rate = lambda n, ms: n * nb / (ms["median_ms"] / 1e3) / 1e9
    out = {"S": S, "D": D, "probe": probe, "lincomb_2term_in_place": add, "copy": copy,
           "probe_gbs": rate(5, probe), "lincomb_gbs": rate(3, add), "copy_gbs": rate(2, copy)}
    out["probe_over_lincomb_rate"] = out["probe_gbs"] / out["lincomb_gbs"]
    return out


def round_trip(S, D, N, tok0, iters=20):
    g = torch.Generator(device=DEV).manual_seed(1)
    keep, x = (torch.randn(N, S, D, generator=g, device=DEV).to(BF) for _ in range(2))
    r = [torch.randn(S, D, generator=g, device=DEV).to(BF) for _ in range(N)]
    work = torch.empty(_lib.step_cache_workspace_bytes(S, D), dtype=torch.uint8, device=DEV)
    sums = torch.zeros(N, 2, dtype=torch.float64, device=DEV)
    host = torch.zeros(N, 2, dtype=torch.float64).pin_memory()
    sc = StepCache(threshold=0.1)
    keys = list(range(N))

    def probes():
        for n in range(N):
            _lib.step_cache_probe(keep[n], x[n], r[n], S, D, tok0, S - tok0, work, sums[n])

    wall = []
    for _ in range(iters + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probes()
        host.copy_(sums, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        sc.decide([(a, b) for a, b in host.tolist()], keys, False)
        wall.append((time.perf_counter() - t0) * 1e3)
    wall = sorted(wall[3:])
    gpu = event_ms(probes, iters=iters)
    return {"S": S, "D": D, "samples": N, "launch_to_decision_ms_median": statistics.median(wall), "launch_to_decision_ms_min": wall[0],
            "launch_to_decision_ms_max": wall[-1], "probes_gpu_ms_median": gpu["median_ms"]}


def c2_arms(steps, layers):
    import bench
    args = bench.parse_args(["--workload", "c2", "--gpus", "1"] + (["--layers", str(layers)] if layers else []))
    wl = bench.C2(args, DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    L = wl.layers

    def run(tau, cap, k):
        wl.model.step_cache, wl.model.step_cache_max_consecutive = tau, cap
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bench.run_steps(wl, k)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        st = list(wl.model.step_cache_stats)
        rec = {"step_cache": tau, "step_cache_max_consecutive": cap, "steps": k, "seconds": s, "ms_per_step": s / k * 1e3,
               "frames_per_s": wl.frames * k / wl.steps_per_video / s,
               "finite": bool(torch.isfinite(wl.last_out.float()).all().item())}
        if tau > 0:
            rec["hit_fraction"] = sum(r["hit"] for r in st) / max(len(st), 1)
            rec["hits"] = "".join("H" if r["hit"] else "M" for r in st)
            rec["max_rel_per_step"] = [round(max(r["rel"]), 4) if all(v == v and v != float("inf") for v in r["rel"]) else None for r in st]
        return rec

    run(0.0, 0, 4)          # warm-up: the 3-pass and the 2-pass workspaces
    run(1e30, 1, 4)         # ... and the cache's buffers
    arms = [("off_first", 0.0, 0), ("always_cap1", 1e30, 1), ("tau_0.05", 0.05, 0), ("tau_0.1", 0.1, 0), ("tau_0.2", 0.2, 0),
            ("off_last", 0.0, 0)]
    res = {"layers": L, "steps": steps, "arms": {name: run(tau, cap, steps) for name, tau, cap in arms}}
    off = (res["arms"]["off_first"]["ms_per_step"] + res["arms"]["off_last"]["ms_per_step"]) / 2
    res["off_ms_per_step_mean"] = off
    res["off_spread_pct"] = abs(res["arms"]["off_first"]["ms_per_step"] - res["arms"]["off_last"]["ms_per_step"]) / off * 100
    res["always_cap1_over_off"] = res["arms"]["always_cap1"]["ms_per_step"] / off
    res["predicted_(1+1/L)/2"] = (1 + 1 / L) / 2
    return res


def deviation(taus, steps=10, layers=4):
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
    for tau in taus:
        model.step_cache = tau
        got = run()
        st = model.step_cache_stats
        out["arms"]["tau_%g" % tau] = {"rel_l2_vs_cache_off": rel(got, off), "hits": "".join("H" if r["hit"] else "M" for r in st),
                                      "hit_fraction": sum(r["hit"] for r in st) / len(st)}
    model.step_cache = 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=50, help="loop iterations per C2 arm (50 = a whole video)")
    ap.add_argument("--layers", type=int, default=0, help="debug: C2 with fewer blocks")
    ap.add_argument("--skip-c2", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "weights": "synthetic (seeded Gaussian); hit rates say nothing about a trained checkpoint"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    res["probe"] = {"c2_17776x3072": probe_vs_lincomb(17776, 3072, 226), "wan_c5_75600x5120": probe_vs_lincomb(75600, 5120, 0)}
    save()
    res["round_trip"] = {"c2_2_samples": round_trip(17776, 3072, 2, 226), "c2_3_samples": round_trip(17776, 3072, 3, 226),
                         "wan_c5_2_samples": round_trip(75600, 5120, 2, 0)}
    save()
    torch.cuda.empty_cache()
    res["deviation"] = deviation((0.05, 0.1, 0.2))
    save()
    torch.cuda.empty_cache()
    if not a.skip_c2:
        res["c2"] = c2_arms(a.steps, a.layers)
        rt = res["round_trip"]["c2_2_samples"]["launch_to_decision_ms_median"]
        res["round_trip"]["share_of_an_off_step_pct"] = rt / res["c2"]["off_ms_per_step_mean"] * 100
        save()
    print(json.dumps({k: res[k] for k in res if k != "c2"} | ({"c2": {k: v for k, v in res["c2"].items() if k != "arms"}} if "c2" in res else {})))


if __name__ == "__main__":
    main()
