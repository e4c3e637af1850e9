#!/usr/bin/env python3
"""Result and host-time probe of the row-norm entries (norm.hip, wan.hip, hunyuan.hip; rownorm_host.h): a fixed, seeded list of
calls -- every entry once per route, the e4m3 twins with their bytes and scales -- each printed as one line with the SHA-256 of
what the call wrote, then the one-block Wan and HunyuanVideo forwards of smoke().  Two builds of the library that compute the same
print the same lines (compare with ALG_HIP_LIB=<other build>).
usage: python scripts/probes/rownorm_routes.py            the checksum lines (needs the GPU)
       python scripts/probes/rownorm_routes.py --time     host time per call (enqueue only, 2,000 calls, best and median of 7) and
                                                          device time per call of alg_layernorm_modulate and alg_layernorm_mod_f32
                                                          at a small shape and at the workloads' shapes"""
import hashlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from alg_amd import _lib  # noqa: E402

BF, DEV = torch.bfloat16, torch.device("cuda:0")


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def rnd(g, *shape, dtype=BF, k=1.0):
    return (torch.randn(*shape, generator=g) * k).to(dtype).to(DEV)


def ln_bf16(g, batch, rows, D, w=True, b=True, mod=True, fp8=False, seg=False):
    x = rnd(g, batch, rows, D)
    wt, bs = (rnd(g, D) if w else None), (rnd(g, D, k=0.1) if b else None)
    nseg = 2 if seg else 1
    sc, sh = (rnd(g, batch, nseg * D, k=0.3), rnd(g, batch, nseg * D, k=0.3)) if mod else (None, None)
    split = rows // 3 if seg else rows      # rows from seg_split on read the second segment: none without one
    if fp8:
        q8, qs = torch.full((batch * rows, D), 0x7f, dtype=torch.uint8, device=DEV), torch.full((batch * rows,), -1.0, device=DEV)
        if seg:
            _lib.layernorm_modulate_seg_fp8(x, q8, qs, wt, bs, sc, sh, nseg * D, D, batch, rows, D, split, 1e-5)
        else:
            _lib.layernorm_modulate_fp8(x, q8, qs, wt, bs, sc, sh, nseg * D, batch, rows, D, split, 1e-5)
        return sha(q8, qs)
    y = torch.full_like(x, 7.0)
    if seg:
        _lib.layernorm_modulate_seg(x, y, wt, bs, sc, sh, nseg * D, D, batch, rows, D, split, 1e-5)
    else:
        _lib.layernorm_modulate(x, y, wt, bs, sc, sh, nseg * D, batch, rows, D, split, 1e-5)
    return sha(y)


def ln_f32(g, batch, rows, D, form, fp8=False, off=0, mod_stride=None):
    x = rnd(g, batch, rows, D)
    ms = D if mod_stride is None else mod_stride
    f = lambda n: torch.cat([torch.zeros(off), torch.randn(n, generator=g) * 0.3]).to(DEV)
    wt, bs = (f(D), f(D)) if form in ("affine", "all") else (None, None)
    sc, sh = (f(batch * ms), f(batch * ms)) if form in ("mod", "all") else (None, None)
    lib = _lib.load_library()
    p = lambda t: 0 if t is None else t.data_ptr() + 4 * off
    if fp8:
        q8, qs = torch.full((batch * rows, D), 0x7f, dtype=torch.uint8, device=DEV), torch.full((batch * rows,), -1.0, device=DEV)
        rc = lib.alg_layernorm_mod_f32_fp8(x.data_ptr(), q8.data_ptr(), qs.data_ptr(), p(wt), p(bs), p(sc), p(sh), ms, batch, rows, D, 1e-6,
                                           None)
        out = (q8, qs)
    else:
        y = torch.full_like(x, 7.0)
        rc = lib.alg_layernorm_mod_f32(x.data_ptr(), y.data_ptr(), p(wt), p(bs), p(sc), p(sh), ms, batch, rows, D, 1e-6, None)
        out = (y,)
    assert rc == 0, lib.alg_last_error()
    torch.cuda.synchronize()
    return sha(*out)


def rms(g, batch, rows, D, fp8=False, per_head_scale=False, rope=True):
    x, w = rnd(g, batch, rows, D), rnd(g, D)
    cos, sin = (torch.randn(rows, 64, generator=g).to(DEV), torch.randn(rows, 64, generator=g).to(DEV)) if rope else (None, None)
    if not fp8:
        _lib.rmsnorm_rope_(x, w, cos, sin, D, batch, rows, D, 1e-6)
        return sha(x)
    H = D // 128
    q8 = torch.full((batch * rows, D), 0x7f, dtype=torch.uint8, device=DEV)
    sc = torch.full((batch * rows * H,), -1.0, device=DEV)
    hs = (torch.rand(batch * H, generator=g) * 0.02 + 0.01).to(DEV) if per_head_scale else None
    _lib.rmsnorm_rope_fp8(x, w, cos, sin, D, batch, rows, D, 1e-6, q8, D, scale=None if per_head_scale else sc, head_scale=hs)
    return sha(q8, sc)


def headnorm(g, batch, rows, heads, fp8=False, per_head_scale=False):
    D = heads * 128
    x, w = rnd(g, batch, rows, D), rnd(g, 128)
    cos, sin = torch.randn(rows, 128, generator=g).to(DEV), torch.randn(rows, 128, generator=g).to(DEV)
    if not fp8:
        _lib.headnorm_rope_(x, w, cos, sin, D, rows * D, batch, rows, heads, rows - 3, 1e-6)
        return sha(x)
    q8 = torch.full((batch, rows, D), 0x7f, dtype=torch.uint8, device=DEV)
    sc = torch.full((batch, rows * heads), -1.0, device=DEV)
    hs = (torch.rand(batch * heads, generator=g) * 0.02 + 0.01).to(DEV) if per_head_scale else None
    _lib.headnorm_rope_fp8(x, w, cos, sin, D, rows * D, batch, rows, heads, rows - 3, 1e-6, q8, D, rows * D,
                           scale=None if per_head_scale else sc, scale_bstride=rows * heads, head_scale=hs)
    return sha(q8, sc)


def qk(g, batch, S, heads, text):
    x = rnd(g, batch, S, 2 * heads * 64)
    wq, bq, wk, bk = rnd(g, 64), rnd(g, 64, k=0.1), rnd(g, 64), rnd(g, 64, k=0.1)
    cos, sin = torch.randn(S - text, 64, generator=g).to(DEV), torch.randn(S - text, 64, generator=g).to(DEV)
    _lib.qk_norm_rope_(x, wq, bq, wk, bk, cos, sin, batch, S, heads, text, 1e-6, q_scale=0.18)
    return sha(x)


def quant(g, rows, K):
    x = rnd(g, rows, K, k=2.0)
    q, s = torch.empty(rows, K, dtype=torch.uint8, device=DEV), torch.empty(rows, device=DEV)
    _lib.quantize_fp8_rows(x, q, s, rows, K)
    return sha(q, s)


CALLS = [
    # the bf16-parameter family: one row per wave, many rows (4,096 rows and more, all four parameters, D <= 3072), every twin
    ("layernorm_modulate one-row 2x37x1024", lambda g: ln_bf16(g, 2, 37, 1024)),
    ("layernorm_modulate one-row no-affine 2x37x1536", lambda g: ln_bf16(g, 2, 37, 1536, w=False, b=False)),
    ("layernorm_modulate one-row no-mod 3x50x512", lambda g: ln_bf16(g, 3, 50, 512, mod=False)),
    ("layernorm_modulate one-row 4095x1024", lambda g: ln_bf16(g, 1, 4095, 1024)),
    ("layernorm_modulate many-rows 4096x1024", lambda g: ln_bf16(g, 1, 4096, 1024)),
    ("layernorm_modulate many-rows 2x2101x3072", lambda g: ln_bf16(g, 2, 2101, 3072)),
    ("layernorm_modulate one-row 4100x3584", lambda g: ln_bf16(g, 1, 4100, 3584)),
    ("layernorm_modulate_seg one-row 2x37x1024", lambda g: ln_bf16(g, 2, 37, 1024, seg=True)),
    ("layernorm_modulate_seg many-rows 2x2101x1536", lambda g: ln_bf16(g, 2, 2101, 1536, seg=True)),
    ("layernorm_modulate_fp8 2x37x1024", lambda g: ln_bf16(g, 2, 37, 1024, fp8=True)),
    ("layernorm_modulate_fp8 2x2101x3072", lambda g: ln_bf16(g, 2, 2101, 3072, fp8=True)),
    ("layernorm_modulate_seg_fp8 2x2101x1536", lambda g: ln_bf16(g, 2, 2101, 1536, fp8=True, seg=True)),
    # the fp32-parameter family: one row, many rows (modulation / affine alone), generic width, the fall-backs to one row
    ("layernorm_mod_f32 one-row mod 2x37x1024", lambda g: ln_f32(g, 2, 37, 1024, "mod")),
    ("layernorm_mod_f32 one-row all 2x37x1536", lambda g: ln_f32(g, 2, 37, 1536, "all")),
    ("layernorm_mod_f32 many-rows mod 2x2101x1536", lambda g: ln_f32(g, 2, 2101, 1536, "mod")),
    ("layernorm_mod_f32 many-rows affine 2x2101x1024", lambda g: ln_f32(g, 2, 2101, 1024, "affine")),
    ("layernorm_mod_f32 one-row mod, parameters 4 bytes off 2x2101x1024", lambda g: ln_f32(g, 2, 2101, 1024, "mod", off=1)),
    ("layernorm_mod_f32 one-row mod, stride 1026 2x2101x1024", lambda g: ln_f32(g, 2, 2101, 1024, "mod", mod_stride=1026)),
    ("layernorm_mod_f32 generic 2x257x1280", lambda g: ln_f32(g, 2, 257, 1280, "affine")),
    ("layernorm_mod_f32 generic 5x512 1x4100x2560", lambda g: ln_f32(g, 1, 4100, 2560, "mod")),
    ("layernorm_mod_f32_fp8 one-row mod 2x37x1024", lambda g: ln_f32(g, 2, 37, 1024, "mod", fp8=True)),
    ("layernorm_mod_f32_fp8 many-rows mod 2x2101x1536", lambda g: ln_f32(g, 2, 2101, 1536, "mod", fp8=True)),
    ("layernorm_mod_f32_fp8 many-rows affine 2x2101x1024", lambda g: ln_f32(g, 2, 2101, 1024, "affine", fp8=True)),
    # norm + rope
    ("rmsnorm_rope 2x37x1536", lambda g: rms(g, 2, 37, 1536)),
    ("rmsnorm_rope no tables 2x37x512", lambda g: rms(g, 2, 37, 512, rope=False)),
    ("rmsnorm_rope_fp8 token scales 2x37x1536", lambda g: rms(g, 2, 37, 1536, fp8=True)),
    ("rmsnorm_rope_fp8 head scales 2x37x1024", lambda g: rms(g, 2, 37, 1024, fp8=True, per_head_scale=True)),
    ("headnorm_rope 2x37x3", lambda g: headnorm(g, 2, 37, 3)),
    ("headnorm_rope_fp8 token scales 2x37x3", lambda g: headnorm(g, 2, 37, 3, fp8=True)),
    ("headnorm_rope_fp8 head scales 2x37x5", lambda g: headnorm(g, 2, 37, 5, fp8=True, per_head_scale=True)),
    ("qk_norm_rope per-vector 2x29x4", lambda g: qk(g, 2, 29, 4, 5)),
    ("qk_norm_rope per-token 2x29x16", lambda g: qk(g, 2, 29, 16, 5)),
    # the quantiser itself, loop and register forms
    ("quantize_fp8_rows 40x264", lambda g: quant(g, 40, 264)),
    ("quantize_fp8_rows 40x3072", lambda g: quant(g, 40, 3072)),
]


def forwards():
    """the one-block Wan and HunyuanVideo forwards of smoke()"""
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
    from alg_amd.transformer_wan import WanTransformer3DModel, WanTransformerConfig
    from oracle import hy_oracle, wan_oracle
    g2 = torch.Generator().manual_seed(9)
    wkw = dict(num_attention_heads=4, ffn_dim=1024, num_layers=1, text_dim=64, image_dim=64, added_kv_proj_dim=512)
    wsd = wan_oracle.init_weights(wan_oracle.WanConfig(**wkw), seed=3)
    wx = torch.randn(2, 36, 2, 8, 16, generator=g2).to(BF)
    wt, wi = torch.randn(2, 512, 64, generator=g2).to(BF), torch.randn(2, 257, 64, generator=g2).to(BF)
    ts = torch.tensor([900.0, 900.0])
    wout = WanTransformer3DModel(WanTransformerConfig(**wkw), wsd, device=DEV)(wx.to(DEV), ts.to(DEV), wt.to(DEV), wi.to(DEV),
                                                                              return_dict=False)[0]
    print("%-72s %s" % ("forward Wan, 1 block", sha(wout)))
    hkw = dict(num_attention_heads=4, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
    hsd = hy_oracle.init_weights(hy_oracle.HyConfig(**hkw), seed=4)
    hx, htxt = torch.randn(2, 16, 2, 8, 16, generator=g2).to(BF), torch.randn(2, 16, 64, generator=g2).to(BF)
    hmask = torch.zeros(2, 16)
    hmask[0, :9] = 1
    hmask[1, :16] = 1
    hpool = torch.randn(2, 64, generator=g2).to(BF)
    hout = HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(**hkw), hsd, device=DEV)(
        hx.to(DEV), ts.to(DEV), htxt.to(DEV), hmask.to(DEV).to(BF), hpool.to(DEV), return_dict=False)[0]
    print("%-72s %s" % ("forward HunyuanVideo, 1 double + 1 single block", sha(hout)))


def timing():
    lib = _lib.load_library()
    g = torch.Generator().manual_seed(1)

    def bf16_call(batch, rows, D):
        x, y = rnd(g, batch, rows, D), torch.empty(batch, rows, D, dtype=BF, device=DEV)
        w, b, sc, sh = rnd(g, D), rnd(g, D), rnd(g, batch, D), rnd(g, batch, D)
        a = (x.data_ptr(), y.data_ptr(), w.data_ptr(), b.data_ptr(), sc.data_ptr(), sh.data_ptr(), D, batch, rows, D, rows * D, rows * D, rows,
             1e-5, None)
        return (lambda: lib.alg_layernorm_modulate(*a)), (x, y, w, b, sc, sh)

    def bf16_plain_call(batch, rows, D):          # no weight / bias: ln_mod_kernel at any row count
        x, y = rnd(g, batch, rows, D), torch.empty(batch, rows, D, dtype=BF, device=DEV)
        sc, sh = rnd(g, batch, D), rnd(g, batch, D)
        a = (x.data_ptr(), y.data_ptr(), None, None, sc.data_ptr(), sh.data_ptr(), D, batch, rows, D, rows * D, rows * D, rows, 1e-5, None)
        return (lambda: lib.alg_layernorm_modulate(*a)), (x, y, sc, sh)

    def bf16_fp8_call(batch, rows, D):
        x = rnd(g, batch, rows, D)
        q8, qs = torch.empty(batch * rows, D, dtype=torch.uint8, device=DEV), torch.empty(batch * rows, device=DEV)
        w, b, sc, sh = rnd(g, D), rnd(g, D), rnd(g, batch, D), rnd(g, batch, D)
        a = (x.data_ptr(), q8.data_ptr(), qs.data_ptr(), w.data_ptr(), b.data_ptr(), sc.data_ptr(), sh.data_ptr(), D, batch, rows, D,
             rows * D, rows, 1e-5, None)
        return (lambda: lib.alg_layernorm_modulate_fp8(*a)), (x, q8, qs, w, b, sc, sh)

    def f32_call(batch, rows, D):
        x, y = rnd(g, batch, rows, D), torch.empty(batch, rows, D, dtype=BF, device=DEV)
        sc, sh = torch.randn(batch, D, generator=g).to(DEV), torch.randn(batch, D, generator=g).to(DEV)
        a = (x.data_ptr(), y.data_ptr(), None, None, sc.data_ptr(), sh.data_ptr(), D, batch, rows, D, 1e-6, None)
        return (lambda: lib.alg_layernorm_mod_f32(*a)), (x, y, sc, sh)

    cases = [("alg_layernorm_modulate 2x8x1024 (one row)", bf16_call(2, 8, 1024)),
             ("alg_layernorm_modulate 2x17776x3072 (C2: many rows)", bf16_call(2, 17776, 3072)),
             ("alg_layernorm_modulate no affine 2x17776x3072 (one row)", bf16_plain_call(2, 17776, 3072)),
             ("alg_layernorm_modulate_fp8 2x17776x3072 (C2 --fp8: one row)", bf16_fp8_call(2, 17776, 3072)),
             ("alg_layernorm_mod_f32 2x8x1024 (one row)", f32_call(2, 8, 1024)),
             ("alg_layernorm_mod_f32 1x32760x5120 (Wan 14B: many rows)", f32_call(1, 32760, 5120))]
    for name, (call, keep) in cases:
        small = "x8x" in name
        n = 2000 if small else 50
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        host, dev = [], []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            host.append((t1 - t0) / n * 1e6)
            dev.append(e0.elapsed_time(e1) / n * 1e3)
        print("%-60s host us/call best %.3f median %.3f | stream us/call best %.2f median %.2f" % (
            name, min(host), statistics.median(host), min(dev), statistics.median(dev)), flush=True)


def main():
    if "--time" in sys.argv:
        return timing()
    for i, (name, fn) in enumerate(CALLS):
        g = torch.Generator().manual_seed(100 + i)
        out = fn(g)
        torch.cuda.synchronize()
        print("%-72s %s" % (name, out), flush=True)
    forwards()


if __name__ == "__main__":
    main()
