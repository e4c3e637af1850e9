"""Measurements of the load-time LoRA merge on one GPU, written as one JSON file (profiles/lora_merge.json is a run of this).

    python scripts/lora_merge_bench.py --out profiles/lora_merge.json [--skip-build] [--rounds 3]

  merge    alg_lora_merge over the six block linears of all 42 layers at the C2 shapes (D = 3,072, F4 = 12,288; 252 weights,
           4.76 G parameters, bf16, in place) at R = 64 and with two adapters at R = 64 + 128: total milliseconds by HIP events
           around the whole sweep, achieved FMA rate (2 N K R flop per weight; the chain runs in double) and bytes per second
           (W read + written, A, B and scale read once).  The yardstick in the same job, arms alternated, is
               torch.addmm(W.float(), B * scale, A).to(torch.bfloat16)
           on the same tensors.  It is a yardstick only: it rounds nothing differently on purpose, but its accumulation order
           is the vendor library's and it is never on the product path.  Package power and shader clock per arm.
  build    wall seconds of CogVideoXTransformer3DModel.from_synthetic() at the C2 configuration without and with
           lora=[(file, 1.0)] (a bf16 .safetensors adapter of rank 64 on all 252 block linears, written to a temporary
           directory) -- the sequence run.py --synthetic --lora runs -- arms off / on / off.

No bound is set in advance: exactness and a fixed order are the requirement, and the cost is once per model load."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

import bench  # noqa: E402
from alg_amd import _lib  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda:0")
D, F4, LAYERS = 3072, 12288, 42
LINEARS = (("attn1.to_q", D, D), ("attn1.to_k", D, D), ("attn1.to_v", D, D), ("attn1.to_out.0", D, D),
           ("ff.net.0.proj", F4, D), ("ff.net.2", D, F4))


def sweep_ms(fn, rounds_inside=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with bench.SmiSampler(0, period=0.05) as smi:
        e0.record()
        for _ in range(rounds_inside):
            fn()
        e1.record()
        torch.cuda.synchronize()
    s = smi.summary() or {}
    return e0.elapsed_time(e1) / rounds_inside, (s.get("power_w") or {}).get("mean"), (s.get("sclk_mhz") or {}).get("mean")


def merge_arms(rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    weights = [(torch.randn(N, K, generator=g, device=DEV) * 0.02).to(BF) for _ in range(LAYERS) for _, N, K in LINEARS]
    shapes = sorted({(N, K) for _, N, K in LINEARS})
    out = {"weights": len(weights), "parameters": sum(w.numel() for w in weights), "arms": {}}
    cases = {}
    for label, ranks in (("r64", (64,)), ("r64_plus_r128", (64, 128))):
        R = sum(ranks)
        # one adapter set per shape (a real adapter has one per weight; the kernel reads A and B once per launch either way).
        # The scale is small: the in-place sweeps are repeated and must stay finite
        ab = {(N, K): (torch.randn(R, K, generator=g, device=DEV), torch.randn(N, R, generator=g, device=DEV),
                       torch.cat([torch.full((r,), 1e-4 * (i + 1), device=DEV) for i, r in enumerate(ranks)])) for N, K in shapes}
        cases[label] = (R, ab)

    def kernel(ab):
        for w in weights:
            a, b, s = ab[tuple(w.shape)]
            _lib.lora_merge(w, a, b, s, out=w)

    def yardstick(ab):
        for i, w in enumerate(weights):
            a, b, s = ab[tuple(w.shape)]
            weights[i] = torch.addmm(w.float(), b * s, a).to(BF)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
        kernel(cases["r64"][1])
        torch.cuda.synchronize()
    yardstick(cases["r64"][1])
    torch.cuda.synchronize()
    for label, (R, ab) in cases.items():
        flop = sum(2 * w.shape[0] * w.shape[1] * R for w in weights)
        nbytes = sum(w.numel() * 4 + (w.shape[0] + w.shape[1] + 1) * R * 4 for w in weights)
        rec = {"R": R, "flop": flop, "bytes": nbytes, "kernel": [], "yardstick_addmm": []}
        for _ in range(rounds):                # arms alternated
            for name, fn in (("kernel", kernel), ("yardstick_addmm", yardstick)):
                ms, pw, clk = sweep_ms(lambda: fn(ab))
                rec[name].append({"ms": ms, "power_w": pw, "sclk_mhz": clk})
        for name in ("kernel", "yardstick_addmm"):
            med = statistics.median(r["ms"] for r in rec[name])
            rec[name + "_median_ms"] = med
            rec[name + "_tflops_fma"] = flop / (med / 1e3) / 1e12
            rec[name + "_tb_per_s"] = nbytes / (med / 1e3) / 1e12
        rec["kernel_over_yardstick_time"] = rec["kernel_median_ms"] / rec["yardstick_addmm_median_ms"]
        out["arms"][label] = rec
    assert all(torch.isfinite(w.float()).all().item() for w in weights[:6])
    return out


def build_arms():
    from safetensors.torch import save_file

    from alg_amd import CogVideoXTransformer3DModel, CogVideoXTransformerConfig
    cfg = CogVideoXTransformerConfig()
    assert cfg.inner_dim == D and cfg.num_layers == LAYERS, (cfg.inner_dim, cfg.num_layers)
    g = torch.Generator().manual_seed(1)
    tensors = {}
    for i in range(LAYERS):
        for name, N, K in LINEARS:
            m = "transformer.transformer_blocks.%d.%s" % (i, name)
            tensors[m + ".lora_A.weight"] = (torch.randn(64, K, generator=g) / K ** 0.5).to(BF)
            tensors[m + ".lora_B.weight"] = (torch.randn(N, 64, generator=g) * 0.01).to(BF)
    out = {"adapter": {"rank": 64, "targets": len(tensors) // 2, "dtype": "bfloat16"}, "arms": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "adapter.safetensors")
        save_file(tensors, path)
        out["adapter"]["file_bytes"] = os.path.getsize(path)
        del tensors

        def build(lora):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model = CogVideoXTransformer3DModel.from_synthetic(cfg, device=DEV, lora=lora)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            report = model.lora_report
            del model
            torch.cuda.empty_cache()
            return dt, report

        build(None)                            # not recorded: the first build pays the library load and the allocator's growth
        for label, lora in (("off_first", None), ("lora", [(path, 1.0)]), ("off_last", None)):
            dt, report = build(lora)
            out["arms"].append({"arm": label, "build_seconds": dt, "lora_report": [list(r) for r in report]})
    off = statistics.mean(a["build_seconds"] for a in out["arms"] if a["arm"] != "lora")
    on = next(a["build_seconds"] for a in out["arms"] if a["arm"] == "lora")
    out["build_seconds_off_mean"], out["build_seconds_lora"], out["added_seconds"] = off, on, on - off
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_merge.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-build", action="store_true")
    args = ap.parse_args()
    _lib.load_library()
    result = {"device": torch.cuda.get_device_name(0), "shapes": {"D": D, "F4": F4, "layers": LAYERS}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    result["merge"] = merge_arms(args.rounds)
    save()
    if not args.skip_build:
        result["build"] = build_arms()
        save()
    print(json.dumps({k: result[k] for k in result if k != "device"})[:4000])


if __name__ == "__main__":
    main()
