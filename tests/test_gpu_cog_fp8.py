"""CogVideoXTransformer3DModel(..., fp8=True): e4m3 block linears on the fp8 MFMA.

The scheme is oracle/fp8_oracle.py's (per-token / per-output-channel amax / 448, fp32 accumulation) -- this build's choice, the
reference has no fp8 -- so every accuracy statement here is about the product and its own oracle, on synthetic Gaussian weights
with jittered affines.  The floor of a forward is the reference's execution mode (bf16 weights and activations, eager op order)
with exactly the six quantised linears of every block sent through fp8_oracle.linear (tests/_fp8_floor.py); the bounds are the
unchanged factors of tests/_parity.py against that floor."""
import pytest
import torch

from _fp8_floor import fp8_linears
from _parity import assert_repeatable, check_floor, rel
from alg_amd import (CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel,
                     CogVideoXTransformerConfig, _lib)
from oracle import dit_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn

SMALL = dict(num_attention_heads=8, attention_head_dim=64, in_channels=16, out_channels=8, num_layers=2,
             time_embed_dim=64, text_embed_dim=128, max_text_seq_length=10, sample_width=12, sample_height=8,
             sample_frames=9, patch_size=2)
# tests/test_gpu_dit_forward.py::test_dit_forward_wider_and_ragged_tokens
WIDER = dict(num_attention_heads=16, num_layers=1, max_text_seq_length=7, sample_width=14, sample_height=10)
FP8_NAMES = ("wqk", "wv", "wo", "wf1", "wf2")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
def _norm_then_quantise(x, w, b, mod, mod_bs, batch, rows, D, seg, eps, x_bstride, x_off, scale_off, shift_off):
    y = torch.empty(batch * rows, D, dtype=BF, device=DEV)
    _lib.layernorm_modulate(x, y, w, b, mod, mod, mod_bs, batch, rows, D, seg, eps, x_bstride=x_bstride, x_off=x_off,
                            scale_off=scale_off, shift_off=shift_off)
    q = torch.empty(batch * rows, D, dtype=torch.uint8, device=DEV)
    s = torch.empty(batch * rows, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_rows(y, q, s, batch * rows, D)
    return q, s


def _fused(x, w, b, mod, mod_bs, batch, rows, D, seg, eps, x_bstride, x_off, scale_off, shift_off):
    q = torch.full((batch * rows, D), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full((batch * rows,), -7.0, dtype=torch.float32, device=DEV)
    _lib.layernorm_modulate_fp8(x, q, s, w, b, mod, mod, mod_bs, batch, rows, D, seg, eps, x_bstride=x_bstride, x_off=x_off,
                                scale_off=scale_off, shift_off=shift_off)
    return q, s


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("D", [512, 1024, 3072, 4096])
def test_layernorm_modulate_fp8_is_norm_then_quantiser(D, batch):
    """alg_layernorm_modulate_fp8 == alg_layernorm_modulate into bf16 + alg_quantize_fp8_rows, bytes and scales, bit for bit."""
    rows, eps = 229, 1e-5                                   # not a multiple of the 4 rows of a workgroup
    pad = 64                                                # x_bstride > rows * D, x_off != 0
    x_bstride, x_off = rows * D + pad, 24
    xbuf = _rand((x_off + batch * x_bstride,), 10 + D + batch, 2.0)
    xv = xbuf[x_off:].view(batch, x_bstride)[:, :rows * D].view(batch, rows, D)
    xv[0, 3] = 1.25                                         # a row of all-equal values: variance 0
    xv[batch - 1, rows - 1] *= 40.0                         # and a large one
    w, b = 1.0 + _rand((D,), 1, 0.2), _rand((D,), 2, 0.1)
    mod_bs = 8 + 6 * D                                      # per batch item: 8 unused | shift[2][D] | scale[2][D] | gate[2][D]
    mod = _rand((batch, mod_bs), 3, 0.5)
    shift_off, scale_off = 8, 8 + 2 * D
    for seg in (0, 7, 226, rows):
        for wgt, bia, m in ((w, b, mod), (w, b, None), (None, None, mod)):   # AdaLN-zero | norm_final | no affine
            args = (xbuf, wgt, bia, m, mod_bs if m is not None else 0, batch, rows, D, seg, eps, x_bstride, x_off,
                    scale_off if m is not None else 0, shift_off if m is not None else 0)
            q_ref, s_ref = _norm_then_quantise(*args)
            q_got, s_got = _fused(*args)
            assert torch.equal(s_got, s_ref), (seg, m is None)
            assert torch.equal(q_got, q_ref), (seg, m is None)
            assert (s_got > 0).all()


@pytest.mark.parametrize("D", [512, 1536, 3072])
def test_layernorm_modulate_fp8_many_rows_form(D):
    """>= 4096 rows with all four parameter rows: alg_layernorm_modulate takes its rows-per-wave form there (a wave walks several
    rows, across the text -> video boundary and from one batch item into the next); the fp8 entry point gives that form's bits."""
    batch, rows, seg, eps = 3, 1501, 226, 1e-5
    x = _rand((batch, rows, D), 20 + D, 1.5)
    x[1, 700] = -0.5
    w, b = 1.0 + _rand((D,), 4, 0.2), _rand((D,), 5, 0.1)
    mod = _rand((batch, 6 * D), 6, 0.5)
    args = (x, w, b, mod, 6 * D, batch, rows, D, seg, eps, rows * D, 0, 2 * D, 0)
    q_ref, s_ref = _norm_then_quantise(*args)
    q_got, s_got = _fused(*args)
    assert torch.equal(s_got, s_ref) and torch.equal(q_got, q_ref)
    # the values are the norm's: de-quantised they are within e4m3's half-ulp (2^-4 relative to the row's amax / 448 * 2^k grid)
    y = torch.empty(batch * rows, D, dtype=BF, device=DEV)
    _lib.layernorm_modulate(x, y, w, b, mod, mod, 6 * D, batch, rows, D, seg, eps, scale_off=2 * D, shift_off=0)
    deq = q_got.view(F8).float() * s_got[:, None]
    assert ((deq - y.float()).abs() <= 2.0 ** -4 * y.float().abs() + s_got[:, None] * 2.0 ** -10).all()


def test_layernorm_modulate_fp8_refuses_other_widths_before_any_launch():
    rows = 5
    for D in (768, 8704):
        x = _rand((rows, D), 7)
        q = torch.full((rows, D), 0x5A, dtype=torch.uint8, device=DEV)
        s = torch.full((rows,), -3.0, dtype=torch.float32, device=DEV)
        with pytest.raises(_lib.AlgHipError, match="multiple of 512"):
            _lib.layernorm_modulate_fp8(x, q, s, None, None, None, None, 0, 1, rows, D, 0, 1e-5)
        torch.cuda.synchronize()
        assert (q == 0x5A).all() and (s == -3.0).all()
    x = _rand((rows, 512), 8)
    q = torch.full((rows, 512), 0x5A, dtype=torch.uint8, device=DEV)
    s = torch.full((rows,), -3.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.AlgHipError, match="together"):          # scale without shift
        _lib.layernorm_modulate_fp8(x, q, s, None, None, x, None, 0, 1, rows, 512, 0, 1e-5)
    assert (q == 0x5A).all() and (s == -3.0).all()


# ---- 2. the GEMM form the CogVideoX block uses ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [7, 256])
def test_gemm_fp8_residual_in_place_bf16_gate_two_segments_batched(T):
    """alg_gemm_fp8 as gemm_out / gemm_ff2 call it: residual in place, bf16 gate with one vector per segment (rows < T take
    gate[0], the rest gate[1]; T inside the first 256-row tile and on a tile boundary), batch = 2 with per-item A scales --
    against the fp32 matmul of the de-quantised operands, rounded where the bf16 epilogue rounds."""
    B, S, D, K = 2, 600, 512, 256
    a, w, bias = _rand((B * S, K), 31), _rand((D, K), 32, 0.04), _rand((D,), 33, 0.1)
    qa = torch.empty(B * S, K, dtype=torch.uint8, device=DEV)
    sa = torch.empty(B * S, dtype=torch.float32, device=DEV)
    qw = torch.empty(D, K, dtype=torch.uint8, device=DEV)
    sw = torch.empty(D, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_rows(a, qa, sa, B * S, K)
    _lib.quantize_fp8_rows(w, qw, sw, D, K)
    deq = lambda q, s: q.view(F8).float() * s[:, None]
    lin = (deq(qa, sa) @ deq(qw, sw).t() + bias.float()).to(BF).view(B, S, D)
    r = _rand((B, S, D), 34, 0.5)
    mod_cols = 16 + 2 * D
    gate = _rand((B, mod_cols), 35, 0.5)                    # per item: 16 unused | gate[2][D]
    c = r.clone()
    _lib.gemm(qa, qw, c, S, D, K, K, K, D, bias=bias, R=c, ldr=D, gate=gate, gate_off=16, strideGate=mod_cols, seg_split=T,
              batch=B, strideA=S * K, strideC=S * D, strideR=S * D, a_scale=sa, b_scale=sw, strideAScale=S)
    g2 = gate[:, 16:].view(B, 2, D).float()
    seg = (torch.arange(S, device=DEV) >= T).long()
    gsel = g2[:, seg]                                       # [B, S, D]
    assert not torch.equal(g2[:, 0], g2[:, 1])
    ref = (r.float() + (gsel * lin.float()).to(BF).float()).to(BF)
    err = (c.float() - ref.float()).abs().max().item()
    print("fp8 gemm, bf16 gate, seg_split=%d: max |err| %.3e (outputs up to %.2f)" % (T, err, ref.float().abs().max().item()))
    assert err <= 2.0 ** -5
    # the wrong segment's gate would not pass: the two gates differ by far more than the bound on most elements
    wrong = (r.float() + (g2[:, 1 - seg] * lin.float()).to(BF).float()).to(BF)
    assert (c.float() - wrong.float()).abs().max().item() > 2.0 ** -3


# ---- 3 - 5. the forward ------------------------------------------------------------------------------------------------------
def _pair(overrides=None, seed=3, fp8=True):
    kw = dict(SMALL, **(overrides or {}))
    ocfg = dit_oracle.DiTConfig(**kw)
    w32 = dit_oracle.init_weights(ocfg, seed=seed, std=0.05, randomize_affine=True)
    wbf = {k: v.to(BF) for k, v in w32.items()}
    model = CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=DEV, fp8=fp8)
    return ocfg, wbf, model


def _inputs(ocfg, N, Fr, C, H, W, T, seed, t):
    g = torch.Generator().manual_seed(seed)
    hs = torch.randn(N, Fr, 2 * C, H, W, generator=g).to(BF)
    ehs = torch.randn(N, T, 128, generator=g).to(BF)
    ts = torch.tensor([t] * N)
    rope = dit_oracle.rope_tables(ocfg, H * 8, W * 8, Fr)
    return hs, ehs, ts, rope


def _oracles(ocfg, wbf, hs, ehs, ts, rope):
    """fp32 reference, bf16-eager and e4m3-eager (bf16 activations, the six block linears through fp8_oracle.linear)."""
    ref = dit_oracle.dit_forward(ocfg, {k: v.float() for k, v in wbf.items()}, hs.float(), ehs.float(), ts, rope)
    bf16 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    with fp8_linears(wbf) as stats:
        e4m3 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    assert stats["routed"] == 6 * ocfg.num_layers
    return ref, bf16, e4m3


def _run(model, hs, ehs, ts, rope):
    return model(hs.to(DEV), ehs.to(DEV), ts, image_rotary_emb=rope, return_dict=False)[0]


@pytest.mark.parametrize("case", ["small_2layers", "16heads_ragged"])
def test_fp8_forward_on_the_e4m3_floor_and_anchored_to_bf16(case):
    """3: HIP fp8 forward vs fp32 within the unchanged factors of the e4m3-eager floor.  4: its distance to the bf16 model's
    output, on the same weights, is at most 1.5 x the distance of the two ORACLE runs (e4m3-eager vs bf16-eager)."""
    if case == "small_2layers":
        ocfg, wbf, model = _pair()
        hs, ehs, ts, rope = _inputs(ocfg, 3, 3, 8, 8, 12, 10, 1, 999)
    else:
        ocfg, wbf, model = _pair(WIDER, seed=8)
        hs, ehs, ts, rope = _inputs(ocfg, 2, 3, 8, 10, 14, 7, 2, 459)
    assert model.fp8 is True and model.fuse_quant is True
    ref, bf16, e4m3 = _oracles(ocfg, wbf, hs, ehs, ts, rope)
    out = _run(model, hs, ehs, ts, rope)
    assert out.shape == ref.shape and out.dtype == BF
    e_hip, e_floor = check_floor("cog_fp8_forward_" + case, out, ref, e4m3, channel_dim=2)
    model_bf16 = CogVideoXTransformer3DModel(model.config, wbf, device=DEV)
    out_bf16 = _run(model_bf16, hs, ehs, ts, rope)
    r, anchor = rel(out, out_bf16), rel(e4m3, bf16)
    print("%s: fp8 HIP vs fp32 %.3e (e4m3-eager floor %.3e); fp8 HIP vs bf16 HIP %.3e (e4m3-eager vs bf16-eager %.3e)"
          % (case, e_hip, e_floor, r, anchor))
    assert 0 < r <= 1.5 * anchor, (r, anchor)


def test_fp8_forward_switches():
    """fuse_quant off, a second run, the folded batch assembly: all the same bits; a bf16 model flipped to fp8 and back."""
    ocfg, wbf, model = _pair()
    hs, ehs, ts, rope = _inputs(ocfg, 3, 3, 8, 8, 12, 10, 1, 999)
    out = _run(model, hs, ehs, ts, rope)
    assert torch.equal(out, _run(model, hs, ehs, ts, rope))
    model.fuse_quant = False
    try:
        unfused = _run(model, hs, ehs, ts, rope)
    finally:
        model.fuse_quant = True
    assert torch.equal(out, unfused)
    N, C = 3, 8
    lat, conds = hs[:1, :, :C], [hs[n:n + 1, :, C:] for n in range(N)]
    hs2 = torch.cat([torch.cat([lat] * N), torch.cat(conds)], dim=2)
    out2 = model.forward_assembled(lat.to(DEV), [c.to(DEV) for c in conds], ehs.to(DEV), ts, rope)
    assert torch.equal(out2, _run(model, hs2, ehs, ts, rope))
    # a model built in bf16: fp8 = True quantises lazily and keeps both sets; back to False is the run that never flipped
    flip = CogVideoXTransformer3DModel(model.config, wbf, device=DEV)
    assert flip.fp8 is False
    first = _run(flip, hs, ehs, ts, rope)
    flip.fp8 = True
    as_fp8 = _run(flip, hs, ehs, ts, rope)
    assert torch.equal(as_fp8, out)                        # the lazily quantised model is the one built with fp8=True
    assert not torch.equal(as_fp8, first)
    flip.fp8 = False
    assert torch.equal(_run(flip, hs, ehs, ts, rope), first)
    for L in flip.layers:
        assert all(nm in L and nm + "8" in L for nm in FP8_NAMES)
    # a model built with fp8=True has nothing to run bf16 on, and says so
    model.fp8 = False
    try:
        with pytest.raises(_lib.AlgHipError, match="fp8=True"):
            _run(model, hs, ehs, ts, rope)
    finally:
        model.fp8 = True


def test_fp8_build_keeps_no_bf16_or_packed_copy_of_the_block_weights():
    kw = dict(SMALL, num_attention_heads=16, num_layers=4)             # 1024 wide: the block weights dominate the footprint
    ocfg = dit_oracle.DiTConfig(**kw)
    wbf = {k: v.to(BF) for k, v in dit_oracle.init_weights(ocfg, seed=4, std=0.05).items()}   # on the host, as a checkpoint is
    cfg = CogVideoXTransformerConfig(**kw)

    def footprint(fp8):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        model = CogVideoXTransformer3DModel(cfg, wbf, device=DEV, fp8=fp8)
        torch.cuda.synchronize()
        return model, torch.cuda.memory_allocated() - before

    m8, b8 = footprint(True)
    for L in m8.layers:
        for nm in FP8_NAMES:
            assert nm not in L and "p" + nm not in L
            q, s = L[nm + "8"]
            assert q.dtype == torch.uint8 and s.dtype == torch.float32 and s.shape == (q.shape[0],)
    del m8
    m16, b16 = footprint(False)
    assert all(nm in L for L in m16.layers for nm in FP8_NAMES)
    D = cfg.inner_dim
    block_params = cfg.num_layers * 12 * D * D
    print("allocated by construction: fp8 %d bytes, bf16 %d bytes (block weights: %d parameters)" % (b8, b16, block_params))
    assert b8 < b16
    # bf16 build: 2 bytes per block parameter + the packed copies of wo / wf1 / wf2 (9 of the 12 D^2 per block, 2 bytes each)
    # = 3.5 bytes per block parameter; fp8 build: 1 byte (+ 4 bytes per output channel).  2.5 apart up to the scales and the
    # allocator's rounding: 2 is asked
    assert b16 - b8 >= 2.0 * block_params


def test_fp8_refuses_a_width_the_e4m3_gemm_cannot_take():
    """K % 128 == 0 is alg_gemm_fp8's contract.  Every width the model class accepts today (inner_dim % 512 == 0, an integer
    feed-forward multiple) meets it; the constructor checks it all the same, before it touches a weight, so that a config
    that ever breaks it (here: a feed-forward width of 512 / 8 = 64) is refused there and not at the first launch."""
    cfg = CogVideoXTransformerConfig(**SMALL)
    cfg.ff_inner_mult = 0.125
    with pytest.raises(ValueError, match="K % 128"):
        CogVideoXTransformer3DModel(cfg, {}, device=DEV, fp8=True)


# ---- 6. the real shape ---------------------------------------------------------------------------------------------------
def test_c2_fp8_forward_at_its_real_shape_two_layers_vs_fp32_oracle():
    """The set-up of tests/test_gpu_full_size.py::test_c2_forward_at_its_real_shape_two_layers_vs_fp32_oracle (17,776 = 226 +
    13 * 30 * 45 tokens, 48 heads x 64, 2 layers, N = 2, same seeds) with the model built fp8=True.  fp32 reference on the host;
    the floor is the same oracle with bf16 weights / activations on the device inside fp8_linears (pointers of the device
    copies); then item 4's bound against the bf16 model's output, and repeatability."""
    kw = dict(num_attention_heads=48, attention_head_dim=64, in_channels=32, out_channels=16, num_layers=2,
              time_embed_dim=512, text_embed_dim=4096, max_text_seq_length=226, sample_width=90, sample_height=60,
              sample_frames=49, patch_size=2)
    ocfg = dit_oracle.DiTConfig(**kw)
    wbf = {k: v.to(BF) for k, v in dit_oracle.init_weights(ocfg, seed=21, std=0.02, randomize_affine=True).items()}
    w32 = {k: v.float() for k, v in wbf.items()}
    model = CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=DEV, fp8=True)
    g = torch.Generator().manual_seed(8)
    hs = torch.randn(2, 13, 32, 60, 90, generator=g).to(BF)
    hs[:, 1:, 16:] = 0                                       # the conditioning half: frame 0 real, frames 1..12 zero
    ehs = torch.randn(2, 226, 4096, generator=g).to(BF)
    ts = torch.tensor([999, 999])
    rope = dit_oracle.rope_tables(ocfg, 480, 720, 13)
    assert rope[0].shape == (17550, 64)
    out = assert_repeatable(lambda: _run(model, hs, ehs, ts, rope), times=3, what="fp8 C2 forward")
    assert out.shape == (2, 13, 16, 60, 90)
    del model
    out_bf16 = _run(CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), wbf, device=DEV), hs, ehs, ts, rope)
    wdev = {k: v.to(DEV) for k, v in wbf.items()}
    dev_args = (hs.to(DEV), ehs.to(DEV), ts.to(DEV), tuple(t.to(DEV) for t in rope))
    bf16 = dit_oracle.dit_forward(ocfg, wdev, *dev_args).cpu()
    with fp8_linears(wdev) as stats:
        e4m3 = dit_oracle.dit_forward(ocfg, wdev, *dev_args).cpu()
    assert stats["routed"] == 12
    del wdev, dev_args
    ref = dit_oracle.dit_forward(ocfg, w32, hs.float(), ehs.float(), ts, rope)
    r, anchor = rel(out, out_bf16), rel(e4m3, bf16)
    print("C2 real shape: fp8 HIP vs bf16 HIP %.3e (e4m3-eager vs bf16-eager %.3e); e4m3-eager vs fp32 %.3e, bf16-eager vs fp32 "
          "%.3e, fp8 HIP vs fp32 %.3e" % (r, anchor, rel(e4m3, ref), rel(bf16, ref), rel(out, ref)))
    check_floor("cog_fp8_forward_c2_real_shape_2layers_17776tokens", out, ref, e4m3, channel_dim=2)
    assert 0 < r <= 1.5 * anchor, (r, anchor)


# ---- 7. the sampler --------------------------------------------------------------------------------------------------------
def test_alg_sampler_with_the_fp8_transformer_takes_the_bf16_branches():
    """8 ALG steps (linear-decay schedule: four 3-pass steps, then four 2-pass ones) with the fp8 transformer: finite latents,
    and the branch sequence of the bf16 pipeline (the schedule does not depend on the transformer's arithmetic)."""
    _, wbf, m8 = _pair(seed=6)
    m16 = CogVideoXTransformer3DModel(m8.config, wbf, device=DEV)
    g = torch.Generator().manual_seed(7)
    first = (torch.randn(1, 1, 8, 8, 12, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)
    traces, outs = [], []
    for model in (m8, m16):
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
    assert [s for s, _, _ in traces[0]] == [s for s, _, _ in traces[1]]
    assert not torch.equal(outs[0], outs[1])
