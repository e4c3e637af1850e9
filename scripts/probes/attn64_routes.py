#!/usr/bin/env python3
"""Route probe of alg_flash_attn_d64_ex: the call table of tests/test_gpu_dit_kernels.py::test_split_kv_tail_at_small_sizes -- two
ragged shapes whose launch plan has a split-KV tail, (1 x 40 heads x 4,090) and (1 x 8 heads x 16,600); the default softmax
un-pre-scaled and under ALG_ATTN_VARIANT=1, the pre-scaled call under ALG_ATTN_PP 0, 4, 7, 8; each with the tail and with
ALG_ATTN_SPLIT_TAIL=0 -- plus one pre-scaled S = 640 call under ALG_ATTN_PP=7, which attention64_m16.hip declines (ten KV tiles).
Prints one line per call with the SHA-256 of O (prefilled with a sentinel).

Two builds of the library that route every call alike print the same lines; under a kernel trace they also dispatch the same
kernels with the same grids (compare with ALG_HIP_LIB=<other build>).
usage: python scripts/probes/attn64_routes.py                  the calls (needs the GPU)
       python scripts/probes/attn64_routes.py --listing DIR    the library's dispatches in the kernel trace (csv) under DIR, in order:
                                                               kernel, grid, workgroup, LDS bytes"""
import csv
import glob
import hashlib
import math
import os
import re
import sys

SHAPES = [(1, 4090, 40), (1, 16600, 8)]
# template arguments of flash_attn_d64_kernel / flash_attn_d64_pipe_kernel before the softmax forms had names
OLD_NAMES = {"flash_attn_d64_kernel<1, 8, false>": "flash_attn_d64_kernel<EXACT>",
             "flash_attn_d64_kernel<33, 8, false>": "flash_attn_d64_kernel<LAZY>",
             "flash_attn_d64_kernel<33, 8, true>": "flash_attn_d64_kernel<LAZY, SPLIT>",
             "flash_attn_d64_kernel<41, 8, false>": "flash_attn_d64_kernel<PRESCALED>",
             "flash_attn_d64_kernel<41, 8, true>": "flash_attn_d64_kernel<PRESCALED, SPLIT>",
             "flash_attn_d64_pipe_kernel<8, false>": "flash_attn_d64_pipe_kernel<false>",
             "flash_attn_d64_pipe_kernel<8, true>": "flash_attn_d64_pipe_kernel<true>"}
NAMES = {"flash_attn_d64_kernel<(Softmax)0, false>": "flash_attn_d64_kernel<EXACT>",
         "flash_attn_d64_kernel<(Softmax)1, false>": "flash_attn_d64_kernel<LAZY>",
         "flash_attn_d64_kernel<(Softmax)1, true>": "flash_attn_d64_kernel<LAZY, SPLIT>",
         "flash_attn_d64_kernel<(Softmax)2, false>": "flash_attn_d64_kernel<PRESCALED>",
         "flash_attn_d64_kernel<(Softmax)2, true>": "flash_attn_d64_kernel<PRESCALED, SPLIT>"}


def listing(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    col = lambda r, *names: next(r[n] for n in names if n in r)
    for r in rows:
        name = r["Kernel_Name"]
        if "alg::" not in name and "a64m" not in name:      # torch's own fills and copies
            continue
        name = re.sub(r"^void |\([^()]*\)$", "", name).replace("alg::", "")      # (the argument list; "(Softmax)1" stays)
        name = OLD_NAMES.get(name, NAMES.get(name, name))
        print("%s grid=%s wg=%s lds=%s" % (name, col(r, "Grid_Size_X", "Grid_Size"), col(r, "Workgroup_Size_X", "Workgroup_Size"),
                                          col(r, "LDS_Block_Size", "Group_Segment_Size")))


def main():
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from alg_amd import _lib

    BF = torch.bfloat16
    DEV = torch.device("cuda:0")
    swap23 = lambda n: (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)

    def operands(Bn, S, H):
        """test_pipelined_attention_kernel's: a fifth of the rows at a non-zero offset, one late dominant key; Q pre-scaled"""
        g = torch.Generator().manual_seed(S + H)       # CPU generator: the inputs do not depend on the device or its library
        q, k, v = ((torch.randn((Bn, S, H, 64), generator=g)).to(BF) for _ in range(3))
        q[:, : S // 5] *= 9.0
        k[:, (2 * S) // 3] *= 6.0
        D, S_pad = H * 64, (S + 127) // 128 * 128
        qs = (q.float() * (0.125 * 1.4426950408889634)).to(BF)
        qkb = torch.cat([qs.reshape(Bn, S, D), k.reshape(Bn, S, D)], dim=-1).contiguous().to(DEV)
        vt = torch.zeros(Bn, D, S_pad, dtype=BF)
        vt[:, :, torch.tensor([swap23(n) for n in range(S)])] = v.reshape(Bn, S, D).transpose(1, 2)
        return qkb, vt.to(DEV), D, S_pad

    def call(name, Bn, S, H, ops, prescaled, **env):
        for key, value in env.items():
            os.environ["ALG_ATTN_" + key] = value
        _lib.reload_env()
        qkb, vt, D, S_pad = ops
        o = torch.full((Bn, S, D), -3.0, dtype=BF, device=DEV)
        _lib.flash_attn_d64(qkb, qkb, vt, o, Bn, H, S, S * 2 * D, 2 * D, D * S_pad, S_pad, S * D, D,
                            0.125 if prescaled else math.log(2.0), k_off=D, q_prescaled=prescaled)
        torch.cuda.synchronize()
        wsb = _lib.load_library().alg_flash_attn_d64_workspace_bytes(Bn, H, S, _lib.ATTN_Q_PRESCALED if prescaled else 0)
        print("%dx%dx%-6d %-22s workspace=%-9d %s" % (Bn, H, S, name, wsb,
                                                     hashlib.sha256(o.cpu().view(torch.int16).numpy().tobytes()).hexdigest()), flush=True)

    for Bn, S, H in SHAPES:
        ops = operands(Bn, S, H)
        for tail in ("1", "0"):
            t = "tail" if tail == "1" else "single"
            call("variant=33 " + t, Bn, S, H, ops, False, VARIANT="33", PP="4", SPLIT_TAIL=tail)
            call("variant=1 " + t, Bn, S, H, ops, False, VARIANT="1", PP="4", SPLIT_TAIL=tail)
            for pp in ("0", "4", "7", "8"):
                call("prescaled pp=%s %s" % (pp, t), Bn, S, H, ops, True, VARIANT="33", PP=pp, SPLIT_TAIL=tail)
    call("prescaled pp=7 declined", 1, 640, 1, operands(1, 640, 1), True, VARIANT="33", PP="7", SPLIT_TAIL="1")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--listing"]:
        listing(sys.argv[2])
    else:
        main()
