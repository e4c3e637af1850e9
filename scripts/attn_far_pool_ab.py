"""Measurements of the opt-in pooled far-field attention (alg_amd/attn_pool.py) on one GPU, written as one JSON file
(profiles/attn_far_pool_ab.json is a run of this).  One job, arms alternated in one process, package power and clock per arm.

    python scripts/attn_far_pool_ab.py --out profiles/attn_far_pool_ab.json [--only kernel,layer,c2] [--layers N] [--parent DIR]
                                       [--limit SECONDS]

Every GPU step runs under its own time limit: each part of --only is a child process of its own, ended after --limit seconds
(default 600), and the job STOPS at the first part -- or the first parent-tree child -- that does not end with status 0 (a time
limit, an abort, a fault): what was measured up to there is in the file, nothing more is started on the card.

  kernel   alg_attn_pool_k and alg_attn_pool_vt (G = 2, 4, 8) at the C2 (17,776 x 48 heads x 64) and C3 (32,760 x 40 heads x 128)
           per-sample shapes as bytes per second, next to alg_lincomb's 2-term in-place add on a bf16 tensor of the source's size
           (first and last: their distance is the job's spread)
  layer    at the C2 (window 2), C3 (window 5) and C4 (window 9) launch shapes: the dense entry (first and last), the window alone,
           and per G = 2, 4 the near launch with lse (the window on the 64 G grid), the two poolings, the pooled far launch(es) on the
           pooled operands, the merge with a shift -- each timed on its own, their SUM reported -- and all of them as one unit
           (AttnPoolPass.attention), reported next to the sum; attn_far_reuse's refresh (near + far + merge) and reuse (near +
           merge) from the same job; sum and unit against the cost model c + (1 - c) / G of dense, c the near table's coverage --
           the difference is reported, whatever it is
  c2       iterations 0-1 of the C2 bench workload through the pipeline's __call__ in one process: off, window only, pool G = 4,
           pool G = 2, off -- every step timed on its own.  --parent DIR: the same two iterations, switch off, in a child process
           that imports the package from DIR (a built checkout of the parent commit), first and last

No bound is set in advance.  Synthetic Gaussian weights: nothing here says anything about quality."""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import bench  # noqa: E402
from alg_amd import _lib  # noqa: E402
from alg_amd.attn_pool import AttnPool, AttnPoolPass  # noqa: E402
from alg_amd.attn_window import KV_ALIGN, SelfAttnOperands, complement_ranges, frame_window_ranges, grid_aligned  # noqa: E402
from attn_far_ab import C2, run_video  # noqa: E402
from attn_window_ab import SHAPES, table_for, timed  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda:0")
WINDOWS = {"c2": 2, "c3_32760x40": 5, "c4_119056x24": 9}
GROUPS = (2, 4)


def kernel_part(iters):
    out = {}
    for name, S, heads, hd in (("c2_17776x48x64", 17776, 48, 64), ("c3_32760x40x128", 32760, 40, 128)):
        D = heads * hd
        s_pad = (S + 63) // 64 * 64
        g = torch.Generator(device=DEV).manual_seed(0)
        k = torch.randn(S, D, generator=g, device=DEV, dtype=BF)
        vt = torch.randn(D, s_pad, generator=g, device=DEV, dtype=BF)
        other = torch.randn(S, D, generator=g, device=DEV, dtype=BF)
        lincomb = lambda: _lib.lincomb([(1.0, k), (1.0, other)], BF, out=k)
        rec = {"keys": S, "heads": heads, "head_dim": hd, "lincomb_bytes": 3 * S * D * 2, "arms": {}}

        def run(label, fn, moved):
            k.normal_()
            r = timed(fn, iters)
            r["bytes_moved"] = moved
            r["gb_per_s"] = moved / (r["median_ms"] * 1e-3) / 1e9
            rec["arms"][label] = r

        run("lincomb_first", lincomb, rec["lincomb_bytes"])
        for G in (2, 4, 8):
            P = (S // G + 63) // 64 * 64
            kp = torch.empty(P, D, dtype=BF, device=DEV)
            vp = torch.empty(D, P, dtype=BF, device=DEV)
            run("pool_k_G%d" % G, lambda: _lib.attn_pool_k(k, kp, 1, heads, hd, S, G, S * D, D, P * D, D), (S // G * G + P) * D * 2)
            run("pool_vt_G%d" % G, lambda: _lib.attn_pool_vt(vt, vp, 1, heads, hd, S, G, D * s_pad, s_pad, D * P, P),
                (S // G * G + P) * D * 2)
            del kp, vp
        run("lincomb_last", lincomb, rec["lincomb_bytes"])
        a, b = rec["arms"]["lincomb_first"], rec["arms"]["lincomb_last"]
        rec["lincomb_gb_per_s_mean"] = (a["gb_per_s"] + b["gb_per_s"]) / 2
        rec["lincomb_spread_ms"] = abs(a["median_ms"] - b["median_ms"])
        for label, r in rec["arms"].items():
            r["rate_over_lincomb"] = r["gb_per_s"] / rec["lincomb_gb_per_s_mean"]
        out[name] = rec
        del k, vt, other
        torch.cuda.empty_cache()
    return out


def _direct(name, fn, *a, **kw):
    return fn(*a, **kw)


def layer_part(iters):
    out = {}
    for name in ("c2", "c3_32760x40", "c4_119056x24"):
        w = WINDOWS[name]
        if name == "c2":
            F, hw, T, heads, N = (C2[k] for k in ("frames", "hw", "prefix", "heads", "samples"))
            hd, Sq = 64, T + F * hw
            Skv = Sq
            window = frame_window_ranges(F, hw, w, prefix=T)
            pad = (Sq + 127) // 128 * 128
        else:
            F, hw, valid, rows, heads = SHAPES[name]
            hd, N, Sq, Skv = 128, 1, F * hw + rows, F * hw + valid
            window = table_for(F, hw, valid, rows, w)        # (C3 has no prompt keys: no tail)
            pad = (Sq + 63) // 64 * 64
        D = heads * hd
        near64 = grid_aligned(window)
        far64 = complement_ranges(near64)
        for t in (window, near64, far64):
            t.device_table
        g = torch.Generator(device=DEV).manual_seed(0)
        qk = torch.randn(N, Sq, 2 * D, generator=g, device=DEV, dtype=BF)
        if hd == 64:
            qk[:, :, :D] *= 0.125 * 1.4426950408889634       # Q pre-scaled: the scores are in log2 units
        vt = torch.randn(N, D, pad, generator=g, device=DEV, dtype=BF)
        o = torch.empty(N, Sq, D, dtype=BF, device=DEV)
        e_o = torch.empty(N, Sq, D, dtype=BF, device=DEV)
        lse_n, lse_f = (torch.empty(N, heads, Sq, device=DEV) for _ in range(2))
        scale = 0.125 if hd == 64 else 1.0 / 128 ** 0.5
        ops = SelfAttnOperands(hd, qk, qk, vt, o, N, heads, Sq, Skv, Sq * 2 * D, 2 * D, Sq * 2 * D, 2 * D, D * pad, pad, Sq * D, D, scale,
                               k_off=D, q_prescaled=hd == 64)
        a, offs = ops.args()
        entry = getattr(_lib, "flash_attn_d%d_ranges_heads" % hd)
        plain = getattr(_lib, "flash_attn_d%d_ranges" % hd)
        if hd == 64:
            dense = lambda: _lib.flash_attn_d64(*a, scale, **offs, q_prescaled=True)
        else:
            dense = lambda: _lib.flash_attn_d128(*a, **offs)

        def far_reuse_near():
            entry(*a, near64, lse=lse_n, **offs)

        def far_reuse_far():
            for n in range(N):
                one = dict(o=e_o, batch=1, q_off=ops.q_off + n * ops.q_bs, k_off=ops.k_off + n * ops.k_bs)
                if hd == 64:
                    one["vt"], one["o"] = vt.view(-1)[n * ops.vt_bs:], e_o.view(-1)[n * Sq * D:]
                else:
                    one["vt_off"], one["o_off"] = n * ops.vt_bs, n * Sq * D
                fa, fo = SelfAttnOperands(*ops._replace(**one)).args()
                entry(*fa, far64, lse=lse_f, lse_off=n * heads * Sq, **fo)

        def far_reuse_merge():
            _lib.attn_merge_lse(o, lse_n, e_o, lse_f, N, heads, hd, Sq, Sq * D, D, Sq * D, D)

        arms = [("dense_first", dense), ("window", lambda: plain(*a, window, **offs)),
                ("far_reuse_refresh", lambda: (far_reuse_near(), far_reuse_far(), far_reuse_merge())),
                ("far_reuse_reuse", lambda: (far_reuse_near(), far_reuse_merge()))]
        rec = {"samples": N, "queries": Sq, "keys": Skv, "heads": heads, "head_dim": hd, "attn_window": w,
               "coverage_window": window.coverage, "arms": {}, "groups": {}}
        passes = {}
        for G in GROUPS:
            st = AttnPool()
            near, pooled = st.near_pooled(window, G, hd, DEV)
            P = -(-(Sq // G) // KV_ALIGN) * KV_ALIGN
            p = AttnPoolPass(st, G, [(near, pooled)], N, Sq, P)
            p.attention(_direct, "attn", ops, 0)          # the workspace
            passes[G] = (p, st, near, pooled, P)
            k_rs, vt_rs = (2 * D, pad) if hd == 64 else (D, P)

            def pool(G=G, st=st, P=P, k_rs=k_rs, vt_rs=vt_rs):
                _lib.attn_pool_k(qk, st.k, N, heads, hd, Skv, G, Sq * 2 * D, 2 * D, P * k_rs, k_rs, src_off=D)
                _lib.attn_pool_vt(vt, st.vt, N, heads, hd, Skv, G, D * pad, pad, D * vt_rs, vt_rs)

            def far(G=G, st=st, pooled=pooled, P=P, k_rs=k_rs, vt_rs=vt_rs):     # what AttnPoolPass launches under "attn_far"
                k_bs, vt_bs = P * k_rs, D * vt_rs
                on = dict(k=st.k, vt=st.vt, o=st.o_far, Skv=pooled.Skv, k_bs=k_bs, k_rs=k_rs, vt_bs=vt_bs, vt_rs=vt_rs, o_bs=Sq * D, o_rs=D,
                          k_off=0, vt_off=0, o_off=0)
                if hd == 128:
                    fa, fo = SelfAttnOperands(*ops._replace(**on)).args()
                    return entry(*fa, pooled, lse=st.lse_far, **fo)
                for n in range(N):
                    one = dict(on, batch=1, q_off=n * ops.q_bs, k_off=n * k_bs, vt=st.vt[n * vt_bs:], o=st.o_far[n * Sq * D:], Skv=Sq,
                               k_bs=ops.q_bs)
                    fa, fo = SelfAttnOperands(*ops._replace(**one)).args()
                    entry(*fa, pooled, lse=st.lse_far, lse_off=n * heads * Sq, **fo)

            def merge(G=G, st=st):
                _lib.attn_merge_lse_shift(o, st.lse_near, st.o_far, st.lse_far, N, heads, hd, Sq, Sq * D, D, Sq * D, D, float(G.bit_length() - 1))

            arms += [("near_lse_G%d" % G, lambda near=near, st=st: entry(*a, near, lse=st.lse_near, **offs)), ("pool_G%d" % G, pool),
                     ("far_pooled_G%d" % G, far), ("merge_shift_G%d" % G, merge), ("unit_G%d" % G, lambda p=p: p.attention(_direct, "attn", ops, 0))]
            rec["groups"]["G%d" % G] = {"coverage_near": near.coverage, "coverage_pooled_of_dense": pooled.coverage * pooled.Skv / Skv,
                                        "workspace_bytes": st.bytes}
        arms.append(("dense_last", dense))
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 2.0:      # not recorded: the first recorded arm meets the chip at its power cap, like the others
            dense()
            torch.cuda.synchronize()
        for label, fn in arms:
            rec["arms"][label] = timed(fn, iters)
        ms = lambda k: rec["arms"][k]["median_ms"]
        d = rec["dense_ms_mean"] = (ms("dense_first") + ms("dense_last")) / 2
        rec["dense_spread_ms"] = abs(ms("dense_first") - ms("dense_last"))
        for r in rec["arms"].values():
            r["ms_over_dense"] = r["median_ms"] / d
        for G in GROUPS:
            gr = rec["groups"]["G%d" % G]
            c = gr["coverage_near"]
            gr["sum_of_parts_ms"] = sum(ms(k % G) for k in ("near_lse_G%d", "pool_G%d", "far_pooled_G%d", "merge_shift_G%d"))
            gr["unit_ms"] = ms("unit_G%d" % G)
            gr["sum_over_dense"], gr["unit_over_dense"] = gr["sum_of_parts_ms"] / d, gr["unit_ms"] / d
            gr["cost_model"] = c + (1 - c) / G
            gr["sum_minus_model"], gr["unit_minus_model"] = gr["sum_over_dense"] - gr["cost_model"], gr["unit_over_dense"] - gr["cost_model"]
            gr["unit_over_far_reuse_refresh"] = ms("unit_G%d" % G) / ms("far_reuse_refresh")
            gr["unit_over_far_reuse_N2_mean"] = ms("unit_G%d" % G) / ((ms("far_reuse_refresh") + ms("far_reuse_reuse")) / 2)
        out[name] = rec
        del qk, vt, o, e_o, lse_n, lse_f, passes, ops
        gc.collect()
        torch.cuda.empty_cache()
    return out


def arm(wl, window, group):
    m = wl.model
    m.attn_window, m.attn_far_pool = window, group
    per, total, box = run_video(wl, 2)
    return {"attn_window": window, "attn_far_pool": group, "step_ms": [round(r["ms"], 2) for r in per], "seconds": total, "box": box,
            "attn_far_pool_bytes": m.attn_far_pool_bytes, "finite": bool(torch.isfinite(wl.last_out.float()).all().item())}


PARENT_CHILD = """
import json, sys
sys.path[:0] = [{root!r}, {root!r} + "/scripts"]
import torch, bench
from attn_far_ab import run_video
wl = bench.WORKLOADS["c2"](bench.parse_args(["--workload", "c2", "--gpus", "1"] + {extra!r}), torch.device("cuda:0"), 0, 1, None)
wl.build()
run_video(wl, 2)
per, total, box = run_video(wl, 2)
print("PARENT " + json.dumps({{"step_ms": [round(r["ms"], 2) for r in per], "box": box}}))
"""


class ChildFailed(Exception):
    """A GPU child did not end with status 0 (a time limit, an abort, a fault): nothing more is started on the card."""


def parent_arm(parent, layers, limit):
    """Iterations 0-1 of C2, switch off, from the tree at `parent` in a child process (this process keeps its own GPU state),
    under its own time limit.  ChildFailed, carrying the record, when it does not end with status 0."""
    code = PARENT_CHILD.format(root=os.path.abspath(parent), extra=(["--layers", str(layers)] if layers else []))
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit, cwd=os.path.abspath(parent))
    except subprocess.TimeoutExpired:
        raise ChildFailed({"error": "the parent tree's child ran into its time limit of %d s" % limit, "returncode": None})
    line = next((l for l in r.stdout.splitlines() if l.startswith("PARENT ")), None)
    if r.returncode or line is None:
        raise ChildFailed({"error": (r.stderr or r.stdout)[-2000:], "returncode": r.returncode})
    return json.loads(line[len("PARENT "):])


def c2_part(layers, parent, limit, res):
    """Fills `res` as it goes: a ChildFailed of a parent-tree child leaves what was measured before it."""
    res["arms"] = {}
    if parent:
        try:
            res["arms"]["parent_off_first"] = parent_arm(parent, layers, limit)
        except ChildFailed as e:
            res["arms"]["parent_off_first"] = e.args[0]
            raise
    argv = ["--workload", "c2", "--gpus", "1"] + (["--layers", str(layers)] if layers else [])
    wl = bench.WORKLOADS["c2"](bench.parse_args(argv), DEV, 0, 1, None)
    wl.build()
    torch.cuda.synchronize()
    w = C2["window"]
    res.update({"layers": wl.layers, "tokens": wl.config(0)["tokens"], "attn_window": w})
    for window, group in ((0, 0), (w, 4), (w, 2)):             # warm-up: workspaces, tables
        arm(wl, window, group)
    for tag, window, group in (("off_first", 0, 0), ("window_only", w, 0), ("pool_G4", w, 4), ("pool_G2", w, 2), ("off_last", 0, 0)):
        res["arms"][tag] = arm(wl, window, group)
    wl.model.attn_window = wl.model.attn_far_pool = 0
    off = [res["arms"]["off_first"]["step_ms"], res["arms"]["off_last"]["step_ms"]]
    mean_off = [(off[0][i] + off[1][i]) / 2 for i in range(2)]
    res["off_step_ms_mean"], res["off_spread_pct"] = mean_off, [abs(off[0][i] - off[1][i]) / mean_off[i] * 100 for i in range(2)]
    for a in res["arms"].values():
        if "step_ms" in a:
            a["iteration_over_off"] = [a["step_ms"][i] / mean_off[i] for i in range(2)]
    res["peak_gib"] = round(torch.cuda.max_memory_allocated(DEV) / 2 ** 30, 1)
    del wl
    gc.collect()
    torch.cuda.empty_cache()
    if parent:
        try:
            res["arms"]["parent_off_last"] = parent_arm(parent, layers, limit)
        except ChildFailed as e:
            res["arms"]["parent_off_last"] = e.args[0]
            raise
        for tag in ("parent_off_first", "parent_off_last"):
            a = res["arms"][tag]
            if "step_ms" in a:
                a["iteration_over_off"] = [a["step_ms"][i] / mean_off[i] for i in range(2)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="kernel,layer,c2")
    ap.add_argument("--layers", type=int, default=0, help="debug: the workload with fewer blocks")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its off arm in the same job")
    ap.add_argument("--limit", type=int, default=600, help="seconds every part (and every parent-tree child) may take")
    ap.add_argument("--part", default=None, help="internal: run this one part in this process (what the per-part children do)")
    a = ap.parse_args()
    if a.part is None:     # the driver: one child per part under its own time limit; stop at the first that fails
        for part in a.only.split(","):
            if part not in ("kernel", "layer", "c2"):
                raise SystemExit("--only: unknown part %r" % part)
            cmd = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--part", part, "--layers", str(a.layers), "--iters",
                   str(a.iters), "--limit", str(a.limit)] + (["--parent", a.parent] if a.parent else [])
            try:     # (c2 holds up to two parent-tree children of `limit` seconds each next to its own arms)
                rc = subprocess.run(cmd, timeout=a.limit * (3 if part == "c2" and a.parent else 1)).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit("part %r ran into its time limit of %d s: nothing more is started on the GPU" % (part, a.limit))
            if rc != 0:
                raise SystemExit("part %r ended with status %d: nothing more is started on the GPU" % (part, rc))
            print(part, "done", flush=True)
        return
    res = {"device": torch.cuda.get_device_name(0), "weights": "synthetic (seeded Gaussian); says nothing about a trained checkpoint"}
    if os.path.exists(a.out):      # parts measured by an earlier call of the same job are kept
        with open(a.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    if a.part == "kernel":
        res["kernel"] = kernel_part(a.iters)
    elif a.part == "layer":
        res["layer"] = layer_part(a.iters)
    elif a.part == "c2":
        res["c2"] = {}
        try:
            c2_part(a.layers, a.parent, a.limit, res["c2"])
        except ChildFailed as e:
            save()     # what was measured up to there
            raise SystemExit("c2: the parent tree's child failed (%r): nothing more is started on the GPU" % (e.args[0].get("returncode"),))
    else:
        raise SystemExit("--part: unknown part %r" % a.part)
    save()


if __name__ == "__main__":
    main()
