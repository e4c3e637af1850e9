#!/usr/bin/env python3
"""Route probe of the d = 128 attention entries: the call table of tests/test_attn128_args_cpu.py on the GPU -- a dense call of
1 x 2 heads x 300 queries at nine key counts around the thresholds of attn128_plan (attention128.hip) under six settings of
(ALG_ATTN128_Q64, ALG_ATTN128_PIPE), a causal call, a grouped-query call and one whose K rows are too wide for the 31-bit offsets
of the two statement kernels -- plus the dual entry, the four ranged entries over one two-range table and the e4m3 entry.
Prints one line per call with the SHA-256 of O (prefilled with a sentinel), and of lse / lse_prefix where the entry writes one.

Two builds of the library that route every call alike print the same lines; under a kernel trace they also dispatch the same
kernels with the same grids (compare with ALG_HIP_LIB=<other build>).
usage: python scripts/probes/attn128_routes.py                  the calls (needs the GPU)
       python scripts/probes/attn128_routes.py --listing DIR    the library's dispatches in the kernel trace (csv) under DIR, in order:
                                                                kernel, grid, workgroup, LDS bytes"""
import csv
import glob
import hashlib
import os
import re
import sys

B, H, SQ = 1, 2, 300
SKV = (4097, 4096, 4032, 768, 767, 704, 512, 449, 448)
OPTIONS = ((1, 1), (2, 1), (3, 1), (0, 1), (0, 0), (1, 0))      # (ALG_ATTN128_Q64, ALG_ATTN128_PIPE)
WIDE = 262144                                                   # K row stride beyond (Skv + 64) * k_rs * 2 < 2^31 at 4,097 keys


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
        print("%s grid=%s wg=%s lds=%s" % (name, col(r, "Grid_Size_X", "Grid_Size"), col(r, "Workgroup_Size_X", "Workgroup_Size"),
                                          col(r, "LDS_Block_Size", "Group_Segment_Size")))


def main():
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from alg_amd import _lib
    from alg_amd.attn_window import KvRanges, KvRangesHeads, LaunchOrder

    BF = torch.bfloat16
    DEV = torch.device("cuda:0")
    D = H * 128
    scale = 128 ** -0.5
    swap23 = lambda n: (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1)
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).numpy().tobytes()).hexdigest()

    def operands(Sq, Skv, heads_kv=H, seed=0):
        """test_flash_attn_d128_q64_kernel's: half the queries scaled up, one dominant key; a CPU generator, so the inputs do not
        depend on the device or its library"""
        g = torch.Generator().manual_seed(Skv + seed)
        q = torch.randn((B, Sq, D), generator=g).to(BF)
        k, v = (torch.randn((B, Skv, heads_kv * 128), generator=g).to(BF) for _ in range(2))
        q[:, : Sq // 2] *= 6.0
        k[:, Skv // 3] *= 8.0
        pad = (Skv + 63) // 64 * 64
        vt = torch.zeros(B, heads_kv * 128, pad, dtype=BF)
        vt[:, :, torch.tensor([swap23(n) for n in range(pad)])[:Skv]] = v.transpose(1, 2)
        return q.to(DEV), k.to(DEV), vt.to(DEV), pad

    def options(q64, pipe):
        os.environ["ALG_ATTN128_Q64"], os.environ["ALG_ATTN128_PIPE"] = str(q64), str(pipe)
        _lib.reload_env()

    def show(name, o, *more):
        torch.cuda.synchronize()
        print("%-44s %s" % (name, " ".join(sha(t) for t in (o,) + more)), flush=True)

    fresh = lambda Sq: torch.full((B, Sq, D), -3.0, dtype=BF, device=DEV)

    # ---- the dense entry
    for Skv in SKV:
        q, k, vt, pad = operands(SQ, Skv)
        for q64, pipe in OPTIONS:
            options(q64, pipe)
            o = fresh(SQ)
            _lib.flash_attn_d128(q, k, vt, o, B, H, SQ, Skv, SQ * D, D, Skv * D, D, D * pad, pad, SQ * D, D, scale)
            show("dense Skv=%d Q64=%d PIPE=%d" % (Skv, q64, pipe), o)
    for q64, pipe in ((1, 1), (2, 1), (0, 1)):
        options(q64, pipe)
        q, k, vt, pad = operands(SQ, SQ)
        o = fresh(SQ)
        _lib.flash_attn_d128(q, k, vt, o, B, H, SQ, SQ, SQ * D, D, SQ * D, D, D * pad, pad, SQ * D, D, scale, causal=True)
        show("causal Sq=Skv=%d Q64=%d PIPE=%d" % (SQ, q64, pipe), o)
        q, k, vt, pad = operands(SQ, 4097, heads_kv=1)
        o = fresh(SQ)
        _lib.flash_attn_d128(q, k, vt, o, B, H, SQ, 4097, SQ * D, D, 4097 * 128, 128, 128 * pad, pad, SQ * D, D, scale, kv_group=2)
        show("kv_group=2 Skv=4097 Q64=%d PIPE=%d" % (q64, pipe), o)
        q, k, vt, pad = operands(SQ, 4097)
        kw = torch.zeros(4097 * WIDE, dtype=BF, device=DEV)          # the same K at a row stride of 512 KiB
        kw.view(4097, WIDE)[:, :D] = k[0]
        o = fresh(SQ)
        _lib.flash_attn_d128(q, kw, vt, o, B, H, SQ, 4097, SQ * D, D, 4097 * WIDE, WIDE, D * pad, pad, SQ * D, D, scale)
        show("k_rs=%d Skv=4097 Q64=%d PIPE=%d" % (WIDE, q64, pipe), o)
        del kw

    # ---- the dual entry
    options(1, 1)
    q, k, vt, pad = operands(SQ, 512)
    _, k2, vt2, pad2 = operands(SQ, 257, seed=1)
    o = fresh(SQ)
    _lib.flash_attn_d128_dual(q, k, vt, 512, 512 * D, D, D * pad, pad, k2, vt2, 257, 257 * D, D, D * pad2, pad2, o, B, H, SQ, SQ * D, D,
                              SQ * D, D, scale)
    show("dual Skv=512 Skv2=257", o)

    # ---- the ranged entries: one two-range table (per block of 256 queries), statement on and off
    Skv = 1024
    q, k, vt, pad = operands(SQ, Skv)
    table = torch.tensor([[[0, 256], [512, 1000]], [[64, 320], [640, 1024]]], dtype=torch.int32)
    ranges = KvRanges(table, Skv, SQ)
    per_head = KvRangesHeads(torch.stack([table, table.flip(0)]), Skv, SQ)
    order = LaunchOrder(torch.tensor([3, -1, 0, 2, -1, 1, -1, -1], dtype=torch.int32), B, H, 2)
    args = (B, H, SQ, Skv, SQ * D, D, Skv * D, D, D * pad, pad, SQ * D, D, scale)
    for q64 in (1, 3):
        options(q64, 1)
        o = fresh(SQ)
        _lib.flash_attn_d128_ranges(q, k, vt, o, *args, ranges)
        show("ranges Q64=%d" % q64, o)
        o, lse = fresh(SQ), torch.full((B * H * SQ,), -7.0, device=DEV)
        _lib.flash_attn_d128_ranges_heads(q, k, vt, o, *args, per_head, lse=lse)
        show("ranges_heads Q64=%d" % q64, o, lse)
        o, lse = fresh(SQ), torch.full((B * H * SQ,), -7.0, device=DEV)
        _lib.flash_attn_d128_ranges_order(q, k, vt, o, *args, per_head, order, lse=lse)
        show("ranges_order Q64=%d" % q64, o, lse)
        o, pre = fresh(SQ), torch.full((B * H * 2 * SQ,), -7.0, device=DEV)
        _lib.flash_attn_d128_ranges_prefix(q, k, vt, o, *args, per_head, pre)
        show("ranges_prefix Q64=%d" % q64, o, pre)

    # ---- the e4m3 entry: any e4m3 bytes do (padding columns zero), unit-free scales
    options(1, 1)
    Skv, pad = 700, 704
    g = torch.Generator().manual_seed(8)
    q8 = torch.randn((B, SQ, D), generator=g).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    k8 = torch.randn((B, Skv, D), generator=g).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    vt8 = torch.zeros(B, D, pad, dtype=torch.uint8)
    vt8[:, :, :Skv] = torch.randn((B, D, Skv), generator=g).to(torch.float8_e4m3fn).view(torch.uint8)
    qs = (torch.rand((B, SQ, H), generator=g) + 0.5).to(DEV)
    ks = (torch.rand((B, H), generator=g) + 0.5).to(DEV)
    vs = (torch.rand((B, D), generator=g) + 0.5).to(DEV)
    o = fresh(SQ)
    _lib.flash_attn_d128_fp8(q8, qs, k8, ks, vt8.to(DEV), vs, o, B, H, SQ, Skv, SQ * D, D, Skv * D, D, D * pad, pad, SQ * D, D, scale)
    show("fp8 Skv=700", o)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--listing"]:
        listing(sys.argv[2])
    else:
        main()
