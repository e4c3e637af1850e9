"""OCP MXFP4 feed-forward linears on the FP4 MFMA (alg_quantize_mxfp4_rows, alg_gemm_fp4, CogVideoXTransformer3DModel(fp4=True)).

The format is fixed in include/alg_hip.h and restated on the host in tests/_mxfp4.py, so the quantiser is held to it bit for bit
and the GEMM's operand lane maps to exact integer data.  The scheme itself (W4A4 on the two feed-forward linears) is this build's
choice -- the reference has no 4-bit path -- so a forward is held to the fp32 oracle on the floor of the reference's execution
mode with exactly those two linears of every block sent through the emulation (tests/_mxfp4.mxfp4_linears), with the unchanged
factors of tests/_parity.py."""
import pytest
import torch

from _mxfp4 import dequantize, mxfp4_linears, pack, quantize, special_blocks, unpack
from _parity import check_floor, rel
from alg_amd import (CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel,
                     CogVideoXTransformerConfig, _lib)
from helpers.trained_like import trained_like
from oracle import dit_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U8 = torch.uint8

SMALL = dict(num_attention_heads=8, attention_head_dim=64, in_channels=16, out_channels=8, num_layers=2,
             time_embed_dim=64, text_embed_dim=128, max_text_seq_length=10, sample_width=12, sample_height=8,
             sample_frames=9, patch_size=2)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _hip_quantize(x, rows, K, x_rstride=None):
    """x on the host (bf16, flat or 2-D) -> (packed bytes [rows, K/2], scales [rows, K/32]) from the HIP quantiser, on the device."""
    q = torch.full((rows, K // 2), 0xA5, dtype=U8, device=DEV)
    s = torch.full((rows, K // 32), 0xFF, dtype=U8, device=DEV)
    _lib.quantize_mxfp4_rows(x.to(DEV), q, s, rows, K, x_rstride=x_rstride)
    return q, s


# ---- 4. the quantiser ------------------------------------------------------------------------------------------------------
def _quantiser_rows(rows, K, seed):
    """Gaussian rows over a wide range of magnitudes, with the special blocks of the CPU test in the leading rows."""
    x = _rand((rows, K), seed) * torch.logspace(-12, 12, rows, base=2.0)[:, None].to(BF)
    sp, _ = special_blocks()
    flat = sp.reshape(-1).to(BF)
    n = min(flat.numel(), x.numel()) // 32 * 32
    x.view(-1)[:n] = flat[:n]
    return x


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_quantiser_bit_exact_against_the_emulation(rows, K):
    x = _quantiser_rows(rows, K, 100 + rows + K)
    codes, scales = quantize(x)
    q, s = _hip_quantize(x, rows, K)
    assert torch.equal(s.cpu(), scales)
    assert torch.equal(q.cpu(), pack(codes))
    assert not bool((s == 0xFF).any())
    if rows * K >= 12 * 32:                                 # all special blocks fit: zero blocks wrote 127, ties went to even
        sp_codes, sp_scales = quantize(special_blocks()[0].to(BF))
        assert torch.equal(unpack(q.cpu()).reshape(-1)[:12 * 32], sp_codes.reshape(-1))
        assert torch.equal(s.cpu().reshape(-1)[:12], sp_scales.reshape(-1))


def test_quantiser_strided_rows():
    rows, K, rs = 5, 256, 264 + 256                         # rows inside a wider buffer, x_rstride % 8 == 0
    buf = _rand((rows, rs), 7, 3.0)
    x = buf[:, :K].contiguous()
    q, s = _hip_quantize(buf, rows, K, x_rstride=rs)
    codes, scales = quantize(x)
    assert torch.equal(s.cpu(), scales) and torch.equal(q.cpu(), pack(codes))


# ---- 5. lane maps, exact ---------------------------------------------------------------------------------------------------
def _exact_operands(M, N, K, seed, identity):
    """e2m1 integers from {0, +-1, +-2, +-3} (codes 0, 2, 4, 5 and their negatives) and scales from {2^-1, 1, 2, 4} per (row,
    block), different for A and B, B asymmetric.  identity: A[m, k] = 1 where k == (m + 3) % K, 0 elsewhere (a shifted identity)."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0, 2, 4, 5, 10, 12, 13], dtype=U8)          # 0, 1, 2, 3, -1, -2, -3
    if identity:
        ca = torch.zeros(M, K, dtype=U8)
        ca[torch.arange(M), (torch.arange(M) + 3) % K] = 2
    else:
        ca = vals[torch.randint(0, 7, (M, K), generator=g)]
    cb = vals[torch.randint(0, 7, (N, K), generator=g)]
    sa = (126 + torch.randint(0, 4, (M, K // 32), generator=g)).to(U8)
    sb = (126 + (torch.arange(N)[:, None] * 3 + torch.arange(K // 32)[None, :] * 5 + 1) % 4).to(U8)
    return ca, sa, cb, sb


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("K", [256, 512])
def test_gemm_fp4_lane_maps_with_exact_integer_data(K, identity):
    """M = 300, N = 260: edge tiles in both directions.  Every product is a multiple of 2^-2 and every partial sum stays below
    2^22 in those units (K * 9 * 16 * 4 < 2^19), so fp32 accumulation is exact in any order and the bf16 store is the only rounding."""
    M, N = 300, 260
    ca, sa, cb, sb = _exact_operands(M, N, K, 40 + K, identity)
    ref64 = dequantize(ca, sa) @ dequantize(cb, sb).t()
    assert float(ref64.abs().max()) * 4 < 2 ** 22 and not torch.equal(ref64[:260, :260], ref64[:260, :260].t())
    c = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    _lib.gemm_fp4(pack(ca).to(DEV), pack(cb).to(DEV), c, M, N, K, K, K, N, a_scale=sa.to(DEV), b_scale=sb.to(DEV))
    assert torch.equal(c.cpu(), ref64.to(BF))


# ---- 6. random operands ----------------------------------------------------------------------------------------------------
def _check_product(c, qa, sa, qw, sw, K):
    """|C - C64| <= 2^-8 |C64| + K 2^-23 sum_k |a_k b_k| per element: the bf16 store, and fp32 accumulation of K exact products."""
    a64, w64 = dequantize(unpack(qa.cpu()), sa.cpu()), dequantize(unpack(qw.cpu()), sw.cpu())
    ref = a64 @ w64.transpose(-1, -2)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (a64.abs() @ w64.abs().transpose(-1, -2))
    err = (c.cpu().double() - ref).abs()
    print("fp4 gemm K=%d: worst element at %.3f of its bound, rel L2 %.2e" % (K, (err / bound.clamp_min(1e-300)).max().item(), rel(c, ref)))
    assert bool((err <= bound).all())


def test_gemm_fp4_random_operands_through_the_hip_quantiser():
    M, N, K = 257, 768, 768
    a, w = _rand((M, K), 51, 2.0), _rand((N, K), 52, 0.05)
    qa, sa = _hip_quantize(a, M, K)
    qw, sw = _hip_quantize(w, N, K)
    c = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    _lib.gemm_fp4(qa, qw, c, M, N, K, K, K, N, a_scale=sa, b_scale=sw)
    _check_product(c, qa, sa, qw, sw, K)


def test_gemm_fp4_batched_with_strides():
    """batch 2: A per item at a padded batch stride, B per item too (strideB / strideBScale), C rows inside a wider buffer."""
    B, M, N, K, ldc = 2, 130, 134, 256, 144   # N % 4 != 0: the element-wise store path
    a, w = _rand((B * (M + 3), K), 53, 1.5), _rand((B * N, K), 54, 0.3)
    qa, sa = _hip_quantize(a, B * (M + 3), K)
    qw, sw = _hip_quantize(w, B * N, K)
    c = torch.full((B, M, ldc), -77.0, dtype=BF, device=DEV)
    _lib.gemm_fp4(qa, qw, c, M, N, K, K, K, ldc, a_scale=sa, b_scale=sw, batch=B, strideA=(M + 3) * K, strideB=N * K,
                  strideC=M * ldc, strideAScale=(M + 3) * (K // 32), strideBScale=N * (K // 32))
    assert bool((c[:, :, N:] == -77.0).all())
    qa_v, sa_v = qa.view(B, M + 3, K // 2)[:, :M], sa.view(B, M + 3, K // 32)[:, :M]
    _check_product(c[:, :, :N], qa_v, sa_v, qw.view(B, N, K // 2), sw.view(B, N, K // 32), K)


# ---- 7. epilogues ----------------------------------------------------------------------------------------------------------
def _gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


def test_gemm_fp4_bias_gelu_tanh():
    """The ff1 form: bias + GELU-tanh, against the same epilogue in fp32 on the float64 product, rounded where nn.Linear and
    the activation round; the bound tests/test_gpu_cog_fp8.py uses for alg_gemm_fp8's epilogue forms (2^-5 absolute)."""
    M, N, K = 600, 520, 256
    a, w, bias = _rand((M, K), 61), _rand((N, K), 62, 0.04), _rand((N,), 63, 0.1)
    qa, sa = _hip_quantize(a, M, K)
    qw, sw = _hip_quantize(w, N, K)
    c = torch.empty(M, N, dtype=BF, device=DEV)
    _lib.gemm_fp4(qa, qw, c, M, N, K, K, K, N, a_scale=sa, b_scale=sw, bias=bias.to(DEV), act=_lib.ACT_GELU_TANH)
    prod = dequantize(unpack(qa.cpu()), sa.cpu()) @ dequantize(unpack(qw.cpu()), sw.cpu()).t()
    lin = (prod.float() + bias.float()).to(BF)
    ref = _gelu_tanh(lin.float()).to(BF)
    err = (c.cpu().float() - ref.float()).abs().max().item()
    print("fp4 gemm, bias + gelu-tanh: max |err| %.3e (outputs up to %.2f)" % (err, ref.float().abs().max().item()))
    assert err <= 2.0 ** -5
    assert (c.cpu().float() - lin.float()).abs().max().item() > 2.0 ** -3       # the activation did run


@pytest.mark.parametrize("T", [7, 256])
def test_gemm_fp4_residual_in_place_bf16_gate_two_segments_batched(T):
    """The ff2 form, as tests/test_gpu_cog_fp8.py states it for alg_gemm_fp8: residual in place, one bf16 gate vector per
    segment (rows < T take gate[0]), batch 2 with per-item A scales; same bound (2^-5 absolute)."""
    B, S, D, K = 2, 600, 512, 256
    a, w, bias = _rand((B * S, K), 31), _rand((D, K), 32, 0.04), _rand((D,), 33, 0.1)
    qa, sa = _hip_quantize(a, B * S, K)
    qw, sw = _hip_quantize(w, D, K)
    prod = dequantize(unpack(qa.cpu()), sa.cpu()) @ dequantize(unpack(qw.cpu()), sw.cpu()).t()
    lin = (prod.float() + bias.float()).to(BF).view(B, S, D)
    r = _rand((B, S, D), 34, 0.5)
    mod_cols = 16 + 2 * D
    gate = _rand((B, mod_cols), 35, 0.5)                    # per item: 16 unused | gate[2][D]
    c = r.clone().to(DEV)
    _lib.gemm_fp4(qa, qw, c, S, D, K, K, K, D, a_scale=sa, b_scale=sw, bias=bias.to(DEV), R=c, ldr=D, gate=gate.to(DEV), gate_off=16,
                  strideGate=mod_cols, seg_split=T, batch=B, strideA=S * K, strideC=S * D, strideR=S * D, strideAScale=S * (K // 32))
    g2 = gate[:, 16:].view(B, 2, D).float()
    seg = (torch.arange(S) >= T).long()
    ref = (r.float() + (g2[:, seg] * lin.float()).to(BF).float()).to(BF)
    err = (c.cpu().float() - ref.float()).abs().max().item()
    print("fp4 gemm, bf16 gate, seg_split=%d: max |err| %.3e (outputs up to %.2f)" % (T, err, ref.float().abs().max().item()))
    assert err <= 2.0 ** -5
    wrong = (r.float() + (g2[:, 1 - seg] * lin.float()).to(BF).float()).to(BF)
    assert (c.cpu().float() - wrong.float()).abs().max().item() > 2.0 ** -3


# ---- 8 - 10. the forward ---------------------------------------------------------------------------------------------------
_CASES = {}


def _case(kind):
    """Weights, inputs and the three oracle runs (fp32, bf16-eager, mxfp4-eager) of a 2-block small CogVideoX: computed once."""
    if kind not in _CASES:
        ocfg = dit_oracle.DiTConfig(**SMALL)
        w32 = dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)
        if kind == "trained_like":
            w32 = trained_like(w32, seed=3)
        wbf = {k: v.to(BF) for k, v in w32.items()}
        g = torch.Generator().manual_seed(1)
        hs = torch.randn(3, 3, 16, 8, 12, generator=g).to(BF)
        ehs = torch.randn(3, 10, 128, generator=g).to(BF)
        ts = torch.tensor([999] * 3)
        rope = dit_oracle.rope_tables(ocfg, 64, 96, 3)
        ref = dit_oracle.dit_forward(ocfg, {k: v.float() for k, v in wbf.items()}, hs.float(), ehs.float(), ts, rope)
        bf16 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
        with mxfp4_linears(wbf) as stats:
            eager4 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
        assert stats["routed"] == 2 * ocfg.num_layers
        _CASES[kind] = dict(wbf=wbf, inputs=(hs, ehs, ts, rope), ref=ref, bf16=bf16, eager4=eager4)
    return _CASES[kind]


def _model(wbf, **kw):
    return CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**SMALL), wbf, device=DEV, **kw)


def _run(model, hs, ehs, ts, rope):
    return model(hs.to(DEV), ehs.to(DEV), ts, image_rotary_emb=rope, return_dict=False)[0]


@pytest.mark.parametrize("kind", ["gaussian", "trained_like"])
def test_fp4_forward_on_the_mxfp4_eager_floor(kind):
    """HIP fp4 forward vs the fp32 oracle within the unchanged factors of tests/_parity.py on the mxfp4-eager floor.  The
    distance to the bf16 model is printed (docs/numerics.md records it), not bounded."""
    c = _case(kind)
    model = _model(c["wbf"], fp4=True)
    assert model.fp4 is True and model.fp8 is False
    out = _run(model, *c["inputs"])
    assert out.shape == c["ref"].shape and out.dtype == BF
    out_bf16 = _run(_model(c["wbf"]), *c["inputs"])
    print("%s: fp4 HIP vs fp32 %.3e (mxfp4-eager floor %.3e, bf16-eager %.3e); fp4 HIP vs bf16 HIP %.3e (mxfp4-eager vs bf16-eager %.3e)"
          % (kind, rel(out, c["ref"]), rel(c["eager4"], c["ref"]), rel(c["bf16"], c["ref"]), rel(out, out_bf16),
             rel(c["eager4"], c["bf16"])))
    check_floor("cog_fp4_forward_" + kind, out, c["ref"], c["eager4"], channel_dim=2)


def test_fp4_switches():
    c = _case("gaussian")
    wbf, inp = c["wbf"], c["inputs"]
    never = _run(_model(wbf), *inp)                         # fp4 never touched: today's forward
    flip = _model(wbf)
    assert flip.fp4 is False
    first = _run(flip, *inp)
    assert torch.equal(first, never)
    flip.fp4 = True
    on = _run(flip, *inp)
    assert torch.equal(on, _run(flip, *inp))                # two fp4 runs are equal
    assert not torch.equal(on, first)
    flip.fp4 = False
    assert torch.equal(_run(flip, *inp), first)             # flipped on and off: the same bits as before
    for L in flip.layers:
        assert all(nm in L and nm + "4" in L for nm in ("wf1", "wf2"))
    built = _model(wbf, fp4=True)
    assert torch.equal(_run(built, *inp), on)               # the lazily quantised model is the one built with fp4=True
    # fp4 with fp8: runs, finite, its own result; built that way or flipped
    both = _model(wbf, fp8=True, fp4=True)
    out_both = _run(both, *inp)
    assert torch.isfinite(out_both.float()).all() and not torch.equal(out_both, on)
    assert all("wf18" not in L and "wf14" in L and "wqk8" in L for L in both.layers)
    flip.fp4 = flip.fp8 = True
    assert torch.equal(_run(flip, *inp), out_both)
    flip.fp4 = flip.fp8 = False
    assert torch.equal(_run(flip, *inp), first)
    # a model built with fp4=True has no bf16 feed-forward to run, and says so
    built.fp4 = False
    with pytest.raises(_lib.AlgHipError, match="fp4=True"):
        _run(built, *inp)
    # composes with the other switches: step cache armed (no hit on a first forward), a frame window, unpacked weights, split Q|K / V
    extra = _model(wbf, fp4=True)
    extra.packed_weights, extra.pair_qkv = False, False
    assert torch.equal(_run(extra, *inp), on)
    extra.pair_qkv, extra.fuse_qk_norm = True, True
    assert torch.equal(_run(extra, *inp), on)
    extra.fuse_qk_norm = False
    extra.attn_window, extra.step_cache = 1, 0.05
    hs, ehs, ts, rope = inp
    win = extra(hs.to(DEV), ehs.to(DEV), ts, image_rotary_emb=rope, return_dict=False, cache_keys=("a", "b", "c"))[0]
    assert torch.isfinite(win.float()).all()


def test_fp4_build_holds_fewer_bytes_and_no_bf16_copy_of_the_two_weights():
    kw = dict(SMALL, num_attention_heads=16, num_layers=4)
    ocfg = dit_oracle.DiTConfig(**kw)
    wbf = {k: v.to(BF) for k, v in dit_oracle.init_weights(ocfg, seed=4, std=0.05).items()}
    cfg = CogVideoXTransformerConfig(**kw)

    def footprint(fp4):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        model = CogVideoXTransformer3DModel(cfg, wbf, device=DEV, fp4=fp4)
        torch.cuda.synchronize()
        return model, torch.cuda.memory_allocated() - before

    m4, b4 = footprint(True)
    for L in m4.layers:
        for nm in ("wf1", "wf2"):
            assert nm not in L and "p" + nm not in L and nm + "8" not in L
            q, s = L[nm + "4"]
            assert q.dtype == U8 and s.dtype == U8 and s.shape == (q.shape[0], q.shape[1] // 16)
        assert "wo" in L and "pwo" in L and "wqk" in L
    del m4
    m16, b16 = footprint(False)
    D = cfg.inner_dim
    ff_params = cfg.num_layers * 8 * D * D
    print("allocated by construction: fp4 %d bytes, bf16 %d bytes (feed-forward weights: %d parameters)" % (b4, b16, ff_params))
    # bf16 build: 2 bytes per feed-forward parameter + its packed copy = 4; fp4 build: 1/2 byte + 1/32 byte of scales: 3 is asked
    assert b4 < b16 and b16 - b4 >= 3.0 * ff_params


def test_fp4_refuses_a_width_that_is_no_multiple_of_256():
    cfg = CogVideoXTransformerConfig(**SMALL)
    cfg.ff_inner_mult = 0.75                                # a feed-forward width of 384
    with pytest.raises(ValueError, match="K % 256"):
        CogVideoXTransformer3DModel(cfg, {}, device=DEV, fp4=True)


def test_alg_sampler_with_the_fp4_transformer_takes_the_bf16_branches():
    """Eight ALG steps (four 3-pass, then four 2-pass) with the fp4 transformer: finite latents, the bf16 pipeline's branch trace."""
    wbf = _case("gaussian")["wbf"]
    g = torch.Generator().manual_seed(7)
    first = (torch.randn(1, 1, 8, 8, 12, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)
    traces, outs = [], []
    for model in (_model(wbf, fp4=True), _model(wbf)):
        pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
        trace = []
        out = pipe(image_latents=first, prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=96, num_frames=9,
                   num_inference_steps=8, output_type="latent", use_low_pass_guidance=True, lp_filter_in_latent=True,
                   lp_filter_type="gaussian_blur", lp_blur_sigma=3.0, lp_blur_kernel_size=3,
                   lp_strength_schedule_type="linear", generator=torch.Generator().manual_seed(0), step_trace=trace).frames
        assert torch.isfinite(out.float()).all()
        traces.append(trace)
        outs.append(out)
    assert [n for _, _, n in traces[0]] == [3, 3, 3, 3, 2, 2, 2, 2]
    assert [(tp, n) for _, tp, n in traces[0]] == [(tp, n) for _, tp, n in traces[1]]
    assert not torch.equal(outs[0], outs[1])
