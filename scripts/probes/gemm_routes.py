#!/usr/bin/env python3
"""Route probe of the GEMM entries: a fixed list of small seeded calls that covers every route and fallback of alg_gemm_bf16,
alg_gemm_bf16_pair, alg_gemm_bf16_pair_qk, alg_gemm_fp8 and alg_conv_cl_bf16 -- plain, residual + gate, the activations, per-row
bias + column permutation, packed B, e4m3 on either schedule, the convolution modes, pairs that ride in one launch and pairs
that do not, the fused and the fallback QK store, one call cut into M slabs -- under ALG_GEMM_PIPE 10, 9 and 6 where the variable
matters.  Prints one line per call with the SHA-256 of C (prefilled with a sentinel: what a call leaves untouched counts).

Two builds of the library that route every call alike print the same lines; under a kernel trace they also dispatch the same
kernels with the same grids (compare with ALG_HIP_LIB=<other build>).  Shapes: M = 300, N = 520 (edge tiles, two N tiles, a
second M tile), K in {64, 192, 256}, batch <= 2.
usage: python scripts/probes/gemm_routes.py                  the calls (needs the GPU)
       python scripts/probes/gemm_routes.py --listing DIR    the library's dispatches in the kernel trace (csv) under DIR, in order:
                                                             kernel, grid, workgroup, LDS bytes"""
import csv
import glob
import hashlib
import os
import re
import sys

M, N, BATCH = 300, 520, 2
SENT = -3.0


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
        name = re.sub(r"^void |\(.*$", "", name).replace("alg::", "")
        print("%s grid=%s wg=%s lds=%s" % (name, col(r, "Grid_Size_X", "Grid_Size"), col(r, "Workgroup_Size_X", "Workgroup_Size"),
                                          col(r, "LDS_Block_Size", "Group_Segment_Size")))


def main():
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from alg_amd import _lib

    BF = torch.bfloat16
    DEV = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(20)      # CPU generator: the inputs do not depend on the device or its library

    def rn(*sh, sc=1.0, dt=BF):
        return (torch.randn(*sh, generator=gen) * sc).to(dt).to(DEV)

    def out(*sh):
        return torch.full(sh, SENT, dtype=BF, device=DEV)

    def sha(c):
        torch.cuda.synchronize()
        return hashlib.sha256(c.cpu().view(torch.int16).numpy().tobytes()).hexdigest()

    def report(name, pipe, *cs):
        print("%-28s pipe=%-2s %s" % (name, pipe, " ".join(sha(c) for c in cs)), flush=True)

    a = {K: rn(BATCH, M, K) for K in (64, 192, 256)}
    w = {K: rn(N, K, sc=0.05) for K in (64, 192, 256)}
    bias, bias_row = rn(N), rn(M)
    res, gate, gate32 = rn(BATCH, M, N), rn(BATCH, 2, N), rn(BATCH, 2, N, dt=torch.float32)

    def lin(K, B=None, ldc=N, **kw):
        """(args, kwargs) of a batched [M, K] x [N, K]^T call onto a fresh C of row pitch ldc; returns the call and its C"""
        c = out(BATCH, M, ldc)
        kw = dict(dict(bias=bias, batch=BATCH, strideA=M * K, strideC=M * ldc), **kw)
        return ((a[K], w[K] if B is None else B, c, M, N, K, K, K, ldc), kw), c

    resid = dict(R=res, ldr=N, strideR=M * N, gate=gate, strideGate=2 * N, seg_split=100)
    singles = {
        "plain": lambda K: lin(K),
        "residual+gate": lambda K: lin(K, **resid),
        "residual+gate_f32": lambda K: lin(K, **dict(resid, gate=gate32, flags=_lib.GEMM_GATE_F32)),
        "gelu": lambda K: lin(K, act=_lib.ACT_GELU_TANH),
        "silu": lambda K: lin(K, act=_lib.ACT_SILU),
        # the V^T form: a per-row bias and the column permutation inside blocks of 16 (C rows are 528 wide: N rounded up to 16)
        "row_bias+permute": lambda K: lin(K, ldc=528, bias=bias_row, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS),
    }
    for pipe in ("10", "9", "6"):
        os.environ["ALG_GEMM_PIPE"] = pipe
        _lib.reload_env()
        for name, make in singles.items():
            for K in ((64, 192) if name == "plain" else (192,)):     # K = 64: one k-tile, the asm loops decline
                call, c = make(K)
                _lib.gemm(*call[0], **call[1])
                report("%s K=%d" % (name, K), pipe, c)
        # ---- pairs: both pairable; one with a residual; one with a packed B
        pk = _lib.PackedB(w[192])
        for name, second in (("pair", {}), ("pair, residual", resid), ("pair, packed", dict(B=pk))):
            (c1a, c1), (c2a, c2) = lin(192), lin(192, **second)
            _lib.gemm_pair(c1a, c2a)
            report(name, pipe, c1, c2)
        # ---- the QK pair: [batch][M][2][heads][64]; heads = 4 is fused, heads = 3 and a packed B take the fallback
        for heads, packed in ((4, False), (3, False), (4, True)):
            D = heads * 64
            y, wqk, wv = rn(BATCH, M, 192), rn(2 * D, 192, sc=0.05), rn(D, 192, sc=0.05)
            ln = [1 + rn(64, sc=0.2), rn(64, sc=0.2), 1 + rn(64, sc=0.2), rn(64, sc=0.2)]
            cos, sin = rn(M - 20, 64, dt=torch.float32), rn(M - 20, 64, dt=torch.float32)
            cqk, cv = out(BATCH, M, 2 * D), out(BATCH, M, D)
            kw = dict(batch=BATCH, strideA=M * 192)
            first = ((y, wqk, cqk, M, 2 * D, 192, 192, 192, 2 * D), dict(kw, bias=rn(2 * D), strideC=M * 2 * D))
            second = ((y, _lib.PackedB(wv) if packed else wv, cv, M, D, 192, 192, 192, D), dict(kw, bias=rn(D), strideC=M * D))
            _lib.gemm_pair_qk(first, second, *ln, cos, sin, heads, 20, 1e-6, q_scale=0.125)
            report("pair_qk heads=%d%s" % (heads, " packed" if packed else ""), pipe, cqk, cv)
        # ---- e4m3: K = 128 is one k-tile (schedule 6), K = 256 two (schedule 9's e4m3 loop under 9 and 10)
        for K in (128, 256):
            x8, w8 = rn(M, K, sc=2.0), rn(N, K, sc=0.05)
            qx, sx = torch.empty(M, K, dtype=torch.uint8, device=DEV), torch.empty(M, device=DEV)
            qw, sw = torch.empty(N, K, dtype=torch.uint8, device=DEV), torch.empty(N, device=DEV)
            _lib.quantize_fp8_rows(x8, qx, sx, M, K)
            _lib.quantize_fp8_rows(w8, qw, sw, N, K)
            c = out(M, N)
            _lib.gemm(qx, qw, c, M, N, K, K, K, N, bias=bias, a_scale=sx, b_scale=sw)
            report("fp8 K=%d" % K, pipe, c)

    os.environ["ALG_GEMM_PIPE"] = "10"
    _lib.reload_env()
    # ---- routes ALG_GEMM_PIPE has no say in: packed B (schedule 11), the convolutions (schedule 6), the slab split
    for name, kw in (("packed", {}), ("packed residual+gate", resid), ("packed gelu", dict(act=_lib.ACT_GELU_TANH))):
        call, c = lin(192, B=_lib.PackedB(w[192]), **kw)
        _lib.gemm(*call[0], **call[1])
        report(name, "-", c)
    frames, Hp, Wp, Cin, Cout = 2, 10, 12, 64, 64
    # output row r of frame t reads input rows r + dt Hp Wp + dy Wp + dx of frame t: kt = 3 reads two frames past the last
    # output frame, and the last rows of the padded grid 2 Wp + 3 rows further -- one more frame covers that margin
    x = rn(frames + 3, Hp * Wp, Cin)
    for name, kt, kw in (("conv k3x3", 1, {}), ("conv k3x3x3", 3, {}), ("conv two voxels", 1, dict(pair=True)),
                         ("conv stride 2", 1, dict(stride2=True))):
        taps = kt * 3 * (4 if kw.get("pair") else 3)
        vox = 2 if kw.get("pair") else 1
        wc, bc = rn(vox * Cout, taps * Cin, sc=0.05), rn(vox * Cout)
        y = out(frames, Hp * Wp, Cout)
        _lib.conv_cl(x, wc, bc, None, y, frames, Hp, Wp, Cin, Cout, kt, **kw)
        report(name, "-", y)
    # ---- one call cut into two M slabs (built like the tall call of tests/test_gpu_gemm_packed_entries.py): ldc = 16384 makes a
    # slab 130,816 rows; a column window of the wide C
    TM, TN, TK, ldc, c0 = 140_000, 512, 128, 16384, 256
    ta, tw, tb = rn(TM, TK), rn(TN, TK, sc=0.05), rn(TN)
    for name, B in (("tall", tw), ("tall packed", _lib.PackedB(tw))):
        c = out(TM, ldc)
        _lib.gemm(ta, B, c, TM, TN, TK, TK, TK, ldc, bias=tb, c_off=c0)
        clean = bool((c[:, :c0] == SENT).all()) and bool((c[:, c0 + TN:] == SENT).all())
        print("%-28s pipe=%-2s %s outside the window untouched: %s" % (name, "10", sha(c[:, c0:c0 + TN].contiguous()), clean), flush=True)
        del c


if __name__ == "__main__":
    if sys.argv[1:2] == ["--listing"]:
        listing(sys.argv[2])
    else:
        main()
