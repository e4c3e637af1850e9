#!/usr/bin/env python3
"""Route probe of the low-pass filters: the call table of tests/test_lowpass_args_cpu.py on the GPU -- the 576-plane calls of the
GPU route walk and a latent plane at 127 / 128 / 512 / 513 planes, each under ALG_LOWPASS_PATH 0..4 in both dtypes; a call on
each side of every coverage rule of lowpass_plan (lowpass.hip); and every case of the bit-identity test of
tests/test_gpu_lowpass.py under the default option.  Prints one line per call with the SHA-256 of the output (prefilled with a
sentinel).

Two builds of the library that route every call alike print the same lines; under a kernel trace they also dispatch the same
kernels with the same grids (compare with ALG_HIP_LIB=<other build>).
usage: python scripts/probes/lowpass_routes.py                  the calls (needs the GPU)
       python scripts/probes/lowpass_routes.py --listing DIR    the library's dispatches in the kernel trace (csv) under DIR, in order:
                                                                kernel, grid, workgroup, LDS bytes"""
import csv
import glob
import hashlib
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")


def listing(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    col = lambda r, *names: next(r[n] for n in names if n in r)
    for r in rows:
        name = r["Kernel_Name"]
        if "alg::" not in name:      # torch's own fills and copies
            continue
        name = re.sub(r"^void |\([^()]*\)$", "", name).replace("alg::", "")
        print("%s grid=%s,%s,%s wg=%s lds=%s" % (name, col(r, "Grid_Size_X", "Grid_Size"), r.get("Grid_Size_Y", ""), r.get("Grid_Size_Z", ""),
                                                col(r, "Workgroup_Size_X", "Workgroup_Size"), col(r, "LDS_Block_Size", "Group_Segment_Size")))


def calls():
    """(name, option, kind, planes, H, W, arg, dtype code, tables, aligned) from the CPU test's tables"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import test_lowpass_args_cpu as t

    dn = lambda d: "f32" if d == t.F32 else "bf16"
    for kind, arg in (("down_up", (6, 8)), ("gaussian", 5)):
        for dtype in (t.F32, t.BF16):
            for option in range(5):
                yield "walk %s %s path=%d" % (kind, dn(dtype), option), option, kind, 576, 12, 16, arg, dtype, True, True
    for kind, arg in (("down_up", (15, 22)), ("gaussian", 9)):
        for dtype in (t.F32, t.BF16):
            for planes in (127, 128, 512, 513):
                for option in range(5):
                    yield "%s %s planes=%d path=%d" % (kind, dn(dtype), planes, option), option, kind, planes, 60, 88, arg, dtype, True, True
    for name, kind, H, W, arg, dtype, kw, _ in t.RULES:
        yield "rule: " + name, kw.get("option", 0), kind, 600, H, W, arg, dtype, kw.get("tables", True), kw.get("aligned", True)
    for shape, dtype, kind, arg, _ in t.BANDWIDTH_CASES:
        planes, (H, W) = int(np.prod(shape[:-2])), shape[-2:]
        if kind == "down_up":
            arg = (max(1, int(round(H * arg))), max(1, int(round(W * arg))))
        else:
            kind, arg = "gaussian", arg[0]
        yield "case %s %s %s %s" % (shape, dn(dtype), kind, arg), 0, kind, planes, H, W, arg, dtype, True, True


def main():
    import torch

    table = list(calls())
    from alg_amd import _lib

    lib = _lib.load_library()
    DEV = torch.device("cuda:0")
    for name, option, kind, planes, H, W, arg, dtype, tables, aligned in table:
        os.environ["ALG_LOWPASS_PATH"] = str(option)
        _lib.reload_env()
        dt = torch.float32 if dtype == 0 else torch.bfloat16
        n, off = planes * H * W, (0 if aligned else 8 // (4 if dtype == 0 else 2))       # misaligned: in and out 8 bytes off
        g = torch.Generator().manual_seed(H * 1000 + W)      # a CPU generator: the inputs do not depend on the device or its library
        x = torch.zeros(n + off, dtype=dt, device=DEV)
        x[off:] = torch.randn(n, generator=g).to(dt).to(DEV)
        out = torch.full((n + off,), -3.0, dtype=dt, device=DEV)
        xv, ov = x[off:].view(planes, H, W), out[off:]
        if kind == "down_up":
            wsb = int(lib.alg_down_up_workspace_bytes(planes, H, W, *arg))
            ws = _lib.scratch(xv, wsb, "down_up")
            tab = _lib.lowpass_tables(xv, *arg) if tables and wsb == 0 else None
            rc = lib.alg_down_up(_lib._ptr(xv), _lib._ptr(ov), planes, H, W, arg[0], arg[1], dtype, 1, _lib._ptr(tab), _lib._ptr(ws), wsb,
                                 _lib._stream())
        else:
            wsb = int(lib.alg_gaussian_blur_workspace_bytes(planes, H, W, arg))
            ws = _lib.scratch(xv, wsb, "gaussian")
            rc = lib.alg_gaussian_blur(_lib._ptr(xv), _lib._ptr(ov), planes, H, W, arg, 1.2, dtype, _lib._ptr(ws), wsb, _lib._stream())
        _lib._check(rc, name)
        torch.cuda.synchronize()
        bits = out.cpu().view(torch.int32 if dtype == 0 else torch.int16).numpy().tobytes()
        print("%-78s %s" % (name, hashlib.sha256(bits).hexdigest()), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--listing"]:
        listing(sys.argv[2])
    else:
        main()
