"""Step time of the CogVideoX-5B-I2V workload (bench.py, C2) with the MXFP4 feed-forward linears off and on, written as one JSON
file (profiles/cog_fp4_step_ab.json is a run of this).

    python scripts/fp4_step_ab.py --out profiles/cog_fp4_step_ab.json [--parent DIR] [--rounds 2]

One GPU, one job, every arm a fresh child process running the same driver line, arms alternated round by round:

    P    the line without --set in DIR (a checkout of the parent commit with its own library built), when --parent is given
    A0   --set fp4=0            A1   --set fp4=1              (bf16 otherwise)
    B0   --set fp8=1 --set fp4=0   B1   --set fp8=1 --set fp4=1

The line is `bench.py --gpus 1 --steps 2 --warmup 1 --full` with the legs of --full that do not concern the transformer switched
off (--no-ab --no-calibration --no-other-workloads --no-cpu-baseline).  --full brackets every launch family of the forward with
HIP events and samples package power / shader clock over the timed steps; per arm the file keeps frames / s, ms per step, the
power / clock record and the milliseconds per step of gemm_ff1, gemm_ff2 and the quantiser passes (their time share of the timed
region times the step; one launch per layer and step for the GEMMs, two for the MXFP4 quantiser).  A child that fails ends the run:
nothing more is started behind it.

Synthetic Gaussian weights: nothing here measures quality."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-ab", "--no-calibration", "--no-other-workloads",
        "--no-cpu-baseline"]
ARMS = {"A0": ["--set", "fp4=0"], "A1": ["--set", "fp4=1"], "B0": ["--set", "fp8=1", "--set", "fp4=0"],
        "B1": ["--set", "fp8=1", "--set", "fp4=1"]}
NAMES = ("gemm_ff1", "gemm_ff2", "quant", "quant4", "ln_mod", "gemm_out", "gemm_qkv", "gemm_qk", "gemm_vt", "attn")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    a = ap.parse_args()
    plan = ([("P", a.parent, [])] if a.parent else []) + [(t, ROOT, e) for t, e in ARMS.items()]
    order, runs = [], {}
    for r in range(1, a.rounds + 1):
        for tag, cwd, extra in plan:
            key = "%s_%d" % (tag, r)
            runs[key] = run_arm(key, cwd, extra, a.limit)
            order.append(key)
            print(key, json.dumps(runs[key]), flush=True)
    mean = lambda tag, f: sum(f(runs["%s_%d" % (tag, r)]) for r in range(1, a.rounds + 1)) / a.rounds
    spread = lambda tag: (max(runs["%s_%d" % (tag, r)]["ms_per_step"] for r in range(1, a.rounds + 1)) /
                          min(runs["%s_%d" % (tag, r)]["ms_per_step"] for r in range(1, a.rounds + 1)) - 1.0)
    tags = [t for t, _, _ in plan]
    summary = {t: {"ms_per_step": mean(t, lambda x: x["ms_per_step"]), "frames_per_s": mean(t, lambda x: x["frames_per_s"]),
                   "run_to_run_rel": spread(t)} for t in tags}
    ff = lambda x: sum(x["ms_per_step_by_name"].get(k, 0.0) for k in ("gemm_ff1", "gemm_ff2"))
    doc = {
        "what": "CogVideoX-5B-I2V (BASELINE config C2) step time with the MXFP4 feed-forward linears off / on (--set fp4=0|1), bf16 "
                "otherwise (A) and with --set fp8=1 (B); P = the parent commit's tree and library; one MI355X, one job, fresh "
                "processes, arms alternated",
        "data": "seeded synthetic Gaussian weights at the CogVideoX-5B-I2V shapes, seeded latents / embeddings (no trained checkpoint)",
        "command": "python " + " ".join(LINE) + " <arm's --set>",
        "arms": dict(ARMS, P="(no --set) in the parent commit's tree"), "order": order, "runs": runs, "summary": summary,
        "ff1_plus_ff2_ms_per_step": {t: mean(t, ff) for t in tags},
        "quantiser_ms_per_step": {t: {"quant (e4m3)": mean(t, lambda x: x["ms_per_step_by_name"].get("quant", 0.0)),
                                      "quant4 (mxfp4)": mean(t, lambda x: x["ms_per_step_by_name"].get("quant4", 0.0))} for t in tags},
    }
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
