"""Step time of the CogVideoX-5B-I2V workload (bench.py, C2) with the MXFP4 feed-forward linears off and on, written as one JSON
file (profiles/cog_fp4_step_ab.json and profiles/cog_fp4_fused_ab.json are runs of this).

    python scripts/fp4_step_ab.py --out profiles/cog_fp4_step_ab.json [--parent DIR] [--rounds 2]
    python scripts/fp4_step_ab.py --out profiles/cog_fp4_fused_ab.json --arms A1,A1U,A0 --parent DIR --parent-set fp4=1 --kernels

One GPU, one job, every arm a fresh child process running the same driver line, arms alternated round by round:

    P    the line in DIR (a checkout of the parent commit with its own library built), when --parent is given; without --set
         unless --parent-set names one (fp4=1: the parent's five-launch feed-forward)
    A0   --set fp4=0            A1   --set fp4=1              (bf16 otherwise)
    A1U  --set fp4=1 --set fuse_quant=0      (A1 without the fused producers: norm2 and ff1 write bf16, a quantiser pass each)
    B0   --set fp8=1 --set fp4=0   B1   --set fp8=1 --set fp4=1

The line is `bench.py --gpus 1 --steps 2 --warmup 1 --full` with the legs of --full that do not concern the transformer switched
off (--no-ab --no-calibration --no-other-workloads --no-cpu-baseline).  --full brackets every launch family of the forward with
HIP events and samples package power / shader clock over the timed steps; per arm the file keeps frames / s, ms per step, the
power / clock record and the milliseconds per step of gemm_ff1, gemm_ff2 and the quantiser passes (their time share of the timed
region times the step; one launch per layer and step for the GEMMs, two for the unfused MXFP4 quantiser, none for the fused one).
A child that fails ends the run: nothing more is started behind it.  The file is rewritten after every arm, so a run that is cut
short keeps what it measured.

--kernels adds a kernel-only section (one more child, before the arms) at the C2 shapes -- batch 2 x 17,776 rows, D = 3,072,
F4 = 12,288 -- that times, with device events, every shape warmed first and the two sides alternated round by round:

    norm     alg_layernorm_modulate_mxfp4                      against   alg_layernorm_modulate + alg_quantize_mxfp4_rows
    ff1      alg_gemm_fp4_q4out (bias, GELU-tanh)              against   alg_gemm_fp4 (bias, GELU-tanh) + alg_quantize_mxfp4_rows

(the section lasts well under a second, so its own power / clock record holds a sample or two; the arms carry the real ones).

Synthetic Gaussian weights: nothing here measures quality."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-ab", "--no-calibration", "--no-other-workloads",
        "--no-cpu-baseline"]
ARMS = {"A0": ["--set", "fp4=0"], "A1": ["--set", "fp4=1"], "A1U": ["--set", "fp4=1", "--set", "fuse_quant=0"],
        "B0": ["--set", "fp8=1", "--set", "fp4=0"], "B1": ["--set", "fp8=1", "--set", "fp4=1"]}
NAMES = ("gemm_ff1", "gemm_ff2", "quant", "quant4", "ln_mod", "gemm_out", "gemm_qkv", "gemm_qk", "gemm_vt", "attn")
C2 = dict(batch=2, S=17776, D=3072, F4=12288, T=226)


def run_arm(tag, cwd, extra, limit):
    r = subprocess.run([sys.executable] + LINE + extra, cwd=cwd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("arm %s exited with %d: nothing more is started" % (tag, r.returncode))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    extra_ = out.get("roofline", {}).get("extra", {})
    share = extra_.get("time_share", {})
    ms = out["ms_per_step"]
    return {"frames_per_s": out["value"], "ms_per_step": ms, "finite": out["finite"], "box": extra_.get("box"),
            "ms_per_step_by_name": {k: round(share[k] * ms, 3) for k in NAMES if k in share},
            "layers": out["config"].get("layers")}


def kernel_section(rounds):
    """The child of --kernels: prints one JSON line."""
    import torch

    sys.path.insert(0, ROOT)
    from alg_amd import _lib
    from bench import SmiSampler

    dev = "cuda:0"
    B, S, D, F4, T = C2["batch"], C2["S"], C2["D"], C2["F4"], C2["T"]
    rows = B * S
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g, device=dev) * scale).to(torch.bfloat16)
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
    x, nw, nb = rnd(B, S, D), 1.0 + rnd(D, scale=0.1), rnd(D, scale=0.1)
    mod_cols = 4 * D
    mod = rnd(B, mod_cols, scale=0.3)
    y, h = torch.empty(rows, D, dtype=torch.bfloat16, device=dev), torch.empty(rows, F4, dtype=torch.bfloat16, device=dev)
    q4, q4s, q4h, q4hs = u8(rows, F4 // 2), u8(rows, F4 // 32), u8(rows, F4 // 2), u8(rows, F4 // 32)
    w1, b1 = rnd(F4, D, scale=0.02), rnd(F4, scale=0.1)
    wq, ws = u8(F4, D // 2), u8(F4, D // 32)
    _lib.quantize_mxfp4_rows(w1, wq, ws, F4, D)
    ln = (nw, nb, mod, mod, mod_cols, B, S, D, T, 1e-5)
    lnkw = dict(scale_off=2 * D, shift_off=0)
    ff1 = dict(a_scale=q4s, b_scale=ws, bias=b1, act=_lib.ACT_GELU_TANH, batch=B, strideA=S * D, strideAScale=S * (D // 32),
               strideC=S * F4)

    def norm_unfused():
        _lib.layernorm_modulate(x, y, *ln, **lnkw)
        _lib.quantize_mxfp4_rows(y, q4, q4s, rows, D)

    def norm_fused():
        _lib.layernorm_modulate_mxfp4(x, q4, q4s, *ln, **lnkw)

    def ff1_unfused():
        _lib.gemm_fp4(q4, wq, h, S, F4, D, D, D, F4, **ff1)
        _lib.quantize_mxfp4_rows(h, q4h, q4hs, rows, F4)

    def ff1_fused():
        _lib.gemm_fp4(q4, wq, q4h, S, F4, D, D, D, F4, q_out_scales=q4hs, strideOutScales=S * (F4 // 32), **ff1)

    def gemm_alone():
        _lib.gemm_fp4(q4, wq, h, S, F4, D, D, D, F4, **ff1)

    sides = {"norm_unfused": norm_unfused, "norm_fused": norm_fused, "ff1_unfused": ff1_unfused, "ff1_fused": ff1_fused,
             "ff1_gemm_alone": gemm_alone}
    for fn in sides.values():                                # warm every shape (q4 / q4s hold the norm's output from here on)
        fn()
    torch.cuda.synchronize()
    reps = 5
    ms = {k: [] for k in sides}
    with SmiSampler(0) as smi:
        for _ in range(rounds):
            for name, fn in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / reps)
    med = lambda v: sorted(v)[len(v) // 2]
    doc = {"shapes": C2, "rounds": rounds, "launches_per_sample": reps,
           "ms": {k: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
           "fused_over_unfused": {"norm": round(med(ms["norm_fused"]) / med(ms["norm_unfused"]), 4),
                                  "ff1": round(med(ms["ff1_fused"]) / med(ms["ff1_unfused"]), 4)},
           "box_over_the_whole_section": smi.summary()}
    print(json.dumps(doc), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built")
    ap.add_argument("--parent-set", action="append", default=[], metavar="ATTR=VALUE", help="--set of the P arm (default: none)")
    ap.add_argument("--arms", default="A0,A1,B0,B1", help="comma-separated arms of this tree, from " + ", ".join(ARMS))
    ap.add_argument("--kernels", action="store_true", help="add the kernel-only section (fused producers against the pairs they replace)")
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    a = ap.parse_args()
    if a.kernel_child:
        return kernel_section(a.kernel_rounds)
    if not a.out:
        ap.error("--out is required")
    arms = [t for t in a.arms.split(",") if t]
    for t in arms:
        if t not in ARMS:
            ap.error("unknown arm %s" % t)
    p_extra = [w for s in a.parent_set for w in ("--set", s)]
    plan = ([("P", a.parent, p_extra)] if a.parent else []) + [(t, ROOT, ARMS[t]) for t in arms]
    tags = [t for t, _, _ in plan]
    order, runs = [], {}
    doc = {
        "what": "CogVideoX-5B-I2V (BASELINE config C2) step time per arm (--set of bench.py; fp4 = the MXFP4 feed-forward linears, "
                "fuse_quant=0 = their operands through bf16 and a quantiser pass); P = the parent commit's tree and library; one "
                "MI355X, one job, fresh processes, arms alternated",
        "data": "seeded synthetic Gaussian weights at the CogVideoX-5B-I2V shapes, seeded latents / embeddings (no trained checkpoint)",
        "command": "python " + " ".join(LINE) + " <arm's --set>",
        "arms": dict({t: ARMS[t] for t in arms}, **({"P": (p_extra or "(no --set)")} if a.parent else {})),
    }

    def write():
        done = lambda tag: [runs[k] for k in order if k.rsplit("_", 1)[0] == tag]
        mean = lambda tag, f: sum(f(x) for x in done(tag)) / len(done(tag))
        spread = lambda tag: max(x["ms_per_step"] for x in done(tag)) / min(x["ms_per_step"] for x in done(tag)) - 1.0
        ff = lambda x: sum(x["ms_per_step_by_name"].get(k, 0.0) for k in ("gemm_ff1", "gemm_ff2"))
        have = [t for t in tags if done(t)]
        doc.update({
            "order": order, "runs": runs,
            "summary": {t: {"ms_per_step": mean(t, lambda x: x["ms_per_step"]), "frames_per_s": mean(t, lambda x: x["frames_per_s"]),
                            "run_to_run_rel": spread(t), "runs": len(done(t))} for t in have},
            "ms_per_step_by_name": {t: {k: round(mean(t, lambda x: x["ms_per_step_by_name"].get(k, 0.0)), 3)
                                        for k in ("ln_mod", "gemm_ff1", "gemm_ff2", "quant4", "quant")} for t in have},
            "ff1_plus_ff2_ms_per_step": {t: mean(t, ff) for t in have},
            "quantiser_ms_per_step": {t: {"quant (e4m3)": mean(t, lambda x: x["ms_per_step_by_name"].get("quant", 0.0)),
                                          "quant4 (mxfp4)": mean(t, lambda x: x["ms_per_step_by_name"].get("quant4", 0.0))} for t in have},
        })
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    if a.kernels:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child", "--kernel-rounds", str(a.kernel_rounds)],
                           cwd=ROOT, capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("the kernel-only section exited with %d: nothing more is started" % r.returncode)
        doc["kernels"] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        print("kernels", json.dumps(doc["kernels"]), flush=True)
        write()
    for r in range(1, a.rounds + 1):
        for tag, cwd, extra in plan:
            key = "%s_%d" % (tag, r)
            runs[key] = run_arm(key, cwd, extra, a.limit)
            order.append(key)
            print(key, json.dumps(runs[key]), flush=True)
            write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
