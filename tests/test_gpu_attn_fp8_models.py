"""`transformer.fp8_attention` of the Wan and HunyuanVideo DiTs: the large self-attention on alg_flash_attn_d128_fp8.

The scheme is this build's (the reference has no fp8), so every accuracy statement is about the product and its own oracle.  The
floor of a forward is the reference's execution mode (bf16 weights and activations, eager op order) with exactly the routed
attention calls sent through the eager restatement of the scheme (tests/_attn_fp8_floor.py); the bounds are the unchanged factors
of tests/_parity.py against that floor, and the distance to the bf16 model is anchored to the distance of the two oracle runs, as
tests/test_gpu_cog_fp8.py does.  Real token counts run both oracle executions by torch's own ops on the device (as
tests/test_gpu_full_size_c345.py does) at 4 heads: the attention sees the full sequence, the linears stay small."""
import pytest
import torch

from _attn_fp8_floor import hy_fp8_attention, wan_fp8_attention
from _parity import check_floor, rel
from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
from alg_amd.schedulers import UniPCMultistepScheduler
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
from alg_amd.transformer_wan import WanTransformer3DModel, WanTransformerConfig
from helpers.trained_like import trained_like
from oracle import hy_oracle, loop_oracle, wan_oracle
from oracle.sched_oracle import UniPCOracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

# (N, F, H, W): 288 tokens; 315 (ragged query blocks and KV tiles); C3's 32,760 and C5's 75,600 tokens
WAN_SHAPES = {"small": (2, 3, 16, 24), "ragged": (3, 5, 14, 18), "c3_tokens": (1, 21, 60, 104), "c5_tokens": (1, 21, 90, 160)}


def _wan_setup(shape, weights, layers=2, heads=4):
    kw = dict(num_attention_heads=heads, ffn_dim=1024, num_layers=layers, text_dim=64, image_dim=64, added_kv_proj_dim=heads * 128)
    cfg, ocfg = WanTransformerConfig(**kw), wan_oracle.WanConfig(**kw)
    sd = wan_oracle.init_weights(ocfg, seed=3)
    if weights == "trained_like":
        sd = trained_like(sd)
    N, F, H, W = WAN_SHAPES[shape]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, 36, F, H, W, generator=g).to(BF)
    txt = torch.randn(N, 512, 64, generator=g).to(BF)
    img = torch.randn(N, 257, 64, generator=g).to(BF)
    return cfg, ocfg, sd, (x, torch.tensor([999.0] * N), txt, img)


def _wan_run(model, inputs):
    x, t, txt, img = inputs
    return model(x.to(DEV), t.to(DEV), txt.to(DEV), img.to(DEV), return_dict=False)[0]


def _wan_oracles(ocfg, sd, inputs, device="cpu"):
    """fp32 reference, bf16-eager, and bf16-eager with the self-attention through the e4m3 restatement."""
    x, t, txt, img = (v.to(device) for v in inputs)
    sd = {k: v.to(device) for k, v in sd.items()}
    with torch.no_grad():
        ref = wan_oracle.wan_forward(ocfg, sd, x.float(), t, txt.float(), img.float()).cpu()
        bf16 = wan_oracle.wan_forward(ocfg, sd, x, t, txt, img, dtype=BF).cpu()
        with wan_fp8_attention(ocfg, sd) as stats:
            e4m3 = wan_oracle.wan_forward(ocfg, sd, x, t, txt, img, dtype=BF).cpu()
    assert stats["routed"] == ocfg.num_layers and stats["other"] == 2 * ocfg.num_layers
    return ref, bf16, e4m3


@pytest.mark.parametrize("weights", ["gauss", "trained_like"])
@pytest.mark.parametrize("shape", ["small", "ragged", "c3_tokens", "c5_tokens"])
def test_wan_fp8_attention_forward_on_the_patched_oracle_floor(shape, weights):
    cfg, ocfg, sd, inputs = _wan_setup(shape, weights)
    ref, bf16, e4m3 = _wan_oracles(ocfg, sd, inputs, device="cpu" if shape in ("small", "ragged") else DEV)
    model = WanTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    assert model.fp8_attention is True and model.fp8 is False
    out = _wan_run(model, inputs)
    assert out.shape == ref.shape and out.dtype == BF
    model.fp8_attention = False
    out_bf16 = _wan_run(model, inputs)
    r, anchor = rel(out, out_bf16), rel(e4m3, bf16)
    print("wan %s %s: fp8-attention HIP vs fp32 %.3e (patched-oracle floor %.3e, bf16-eager %.3e); vs bf16 HIP %.3e (the two oracle "
          "runs %.3e)" % (shape, weights, rel(out, ref), rel(e4m3, ref), rel(bf16, ref), r, anchor))
    check_floor("wan_fp8_attention_%s_%s" % (shape, weights), out, ref, e4m3)
    assert 0 < r <= 1.5 * anchor, (r, anchor)


def test_wan_fp8_attention_flag_off_is_todays_forward_and_flips_back():
    cfg, ocfg, sd, inputs = _wan_setup("ragged", "trained_like")
    never = _wan_run(WanTransformer3DModel(cfg, sd, device=DEV), inputs).clone()
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    assert model.fp8_attention is False
    off = _wan_run(model, inputs).clone()
    assert torch.equal(off, never)
    model.fp8_attention = True
    on = _wan_run(model, inputs).clone()
    assert not torch.equal(on, off) and bool(torch.isfinite(on.float()).all())
    assert torch.equal(on, _wan_run(WanTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True), inputs))
    model.fp8_attention = False
    assert torch.equal(_wan_run(model, inputs), never)
    # independent of fp8: e4m3 linears with the flag on run, and differ from e4m3 linears alone
    both = WanTransformer3DModel(cfg, sd, device=DEV, fp8=True, fp8_attention=True)
    small = _wan_setup("small", "trained_like")[3]          # (fp8 linears: the per-token scale rows want 16-byte aligned batches)
    a = _wan_run(both, small).clone()
    both.fp8_attention = False
    b = _wan_run(both, small)
    assert bool(torch.isfinite(a.float()).all()) and not torch.equal(a, b)
    assert torch.equal(b, _wan_run(WanTransformer3DModel(cfg, sd, device=DEV, fp8=True), small))


def test_wan_two_step_sampler_with_fp8_attention():
    """wan:843-927 with the flag on, 2 steps (a 3-pass and a 2-pass one), against the loop oracle driving the fp32 oracle DiT; the
    floor is the same loop over the bf16-eager oracle with its self-attention through the restatement."""
    cfg, ocfg, sd, _ = _wan_setup("small", "gauss", layers=1)
    model = WanTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    g = torch.Generator().manual_seed(8)
    lat, cond = torch.randn(1, 16, 3, 16, 24, generator=g), torch.randn(1, 20, 3, 16, 24, generator=g)
    pe, ne = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 512, 64, generator=g).to(BF)
    ie = torch.randn(1, 257, 64, generator=g).to(BF)
    alg = dict(lp_filter_type="down_up", lp_resize_factor=0.4, lp_strength_schedule_type="interval",
               schedule_interval_start_time=0.0, schedule_interval_end_time=0.3)
    fp32_dit = lambda x, ts, e, ei: wan_oracle.wan_forward(ocfg, sd, x.float(), ts.float(), e.float(), ei.float()).to(BF)
    bf16_dit = lambda x, ts, e, ei: wan_oracle.wan_forward(ocfg, sd, x.to(BF), ts.float(), e, ei, dtype=BF)
    loop = lambda dit, **kw: loop_oracle.wan_denoise_loop(dit, UniPCOracle(flow_shift=3.0), lat, cond, pe, ne, ie, 2,
                                                          guidance_scale=5.0, use_low_pass_guidance=True, **alg, **kw)
    trace_o, trace_p = [], []
    want = loop(fp32_dit, trace=trace_o)
    with wan_fp8_attention(ocfg, sd) as stats:
        floor = loop(bf16_dit)
    assert stats["routed"] >= 2 and stats["other"] == 2 * stats["routed"]
    pipe = WanImageToVideoPipeline(transformer=model, scheduler=UniPCMultistepScheduler(flow_shift=3.0)).to(DEV)
    out = pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), image_embeds=ie.to(DEV),
               image_condition=cond.to(DEV), latents=lat.to(DEV), height=128, width=192, num_frames=9,
               num_inference_steps=2, guidance_scale=5.0, output_type="latent", use_low_pass_guidance=True,
               lp_filter_in_latent=True, step_trace=trace_p, **alg)
    passes = [n for _, n, _ in trace_p]
    assert passes == [n for _, n, _ in trace_o] and passes[0] == 3 and passes[-1] == 2       # both loop branches run
    check_floor("wan_sampler_2steps_fp8_attention", out.frames, want, floor)


# ---- HunyuanVideo ----------------------------------------------------------------------------------------------------------------
# (N, F, H, W, L, valid): 192 + 20 tokens; 180 + 22 (180 % 16 = 4, ragged); C4's 118,800 + 256 tokens (48 valid)
HY_SHAPES = {"small": (2, 3, 16, 16, 20, (13, 20)), "ragged": (2, 3, 12, 20, 22, (22, 5)), "c4_tokens": (1, 33, 90, 160, 256, (48,))}


def _hy_setup(shape, weights, mode="token_replace"):
    kw = dict(num_attention_heads=4, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64,
              pooled_projection_dim=64)
    kw.update(dict(image_condition_type="token_replace", guidance_embeds=False) if mode == "token_replace" else
              dict(image_condition_type="latent_concat", guidance_embeds=True))
    cfg, ocfg = HunyuanVideoTransformerConfig(**kw), hy_oracle.HyConfig(**kw)
    sd = hy_oracle.init_weights(ocfg, seed=3)
    if weights == "trained_like":
        sd = trained_like(sd)
    N, F, H, W, L, valid = HY_SHAPES[shape]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, 16, F, H, W, generator=g).to(BF)
    txt = torch.randn(N, L, 64, generator=g).to(BF)
    mask = torch.zeros(N, L)
    for b, v in enumerate(valid):
        mask[b, :v] = 1
    pooled = torch.randn(N, 64, generator=g).to(BF)
    guid = torch.tensor([6000.0] * N) if kw["guidance_embeds"] else None
    return cfg, ocfg, sd, (x, torch.tensor([996.0] * N), txt, mask, pooled, guid)


def _hy_run(model, inputs):
    x, t, txt, mask, pooled, guid = inputs
    return model(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                 encoder_attention_mask=mask.to(DEV).to(BF), pooled_projections=pooled.to(DEV),
                 guidance=None if guid is None else guid.to(DEV), return_dict=False)[0]


def _hy_oracles(ocfg, sd, inputs, device="cpu"):
    x, t, txt, mask, pooled, guid = (None if v is None else v.to(device) for v in inputs)
    sd = {k: v.to(device) for k, v in sd.items()}
    g32 = None if guid is None else guid.float()
    with torch.no_grad():
        ref = hy_oracle.hy_forward(ocfg, {k: v.float() for k, v in sd.items()}, x.float(), t, txt.float(), mask, pooled.float(),
                                   g32).cpu()
        bf16 = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, guid, dtype=BF).cpu()
        with hy_fp8_attention(ocfg, sd) as stats:
            e4m3 = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, guid, dtype=BF).cpu()
    assert stats["routed"] == ocfg.num_layers + ocfg.num_single_layers and stats["other"] == ocfg.num_refiner_layers
    return ref, bf16, e4m3


@pytest.mark.parametrize("weights", ["gauss", "trained_like"])
@pytest.mark.parametrize("shape", ["small", "ragged", "c4_tokens"])
def test_hunyuan_fp8_attention_forward_on_the_patched_oracle_floor(shape, weights):
    cfg, ocfg, sd, inputs = _hy_setup(shape, weights, mode="token_replace" if shape != "ragged" else "plain_guidance")
    ref, bf16, e4m3 = _hy_oracles(ocfg, sd, inputs, device="cpu" if shape != "c4_tokens" else DEV)
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    out = _hy_run(model, inputs)
    assert out.shape == ref.shape and out.dtype == BF
    model.fp8_attention = False
    out_bf16 = _hy_run(model, inputs)
    assert torch.equal(out_bf16, _hy_run(HunyuanVideoTransformer3DModel(cfg, sd, device=DEV), inputs))     # off: today's bits
    r, anchor = rel(out, out_bf16), rel(e4m3, bf16)
    print("hunyuan %s %s: fp8-attention HIP vs fp32 %.3e (patched-oracle floor %.3e, bf16-eager %.3e); vs bf16 HIP %.3e (the two "
          "oracle runs %.3e)" % (shape, weights, rel(out, ref), rel(e4m3, ref), rel(bf16, ref), r, anchor))
    check_floor("hunyuan_fp8_attention_%s_%s" % (shape, weights), out, ref, e4m3)
    assert 0 < r <= 1.5 * anchor, (r, anchor)
    model.fp8_attention = True
    assert torch.equal(_hy_run(model, inputs), out)                                                        # and back on: the same bits
