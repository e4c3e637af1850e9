"""LoRA adapters merged at load time, through the three transformers, the pipeline loader and a checkpoint directory.

The reference of every forward is the CPU oracle on the FLOAT64-merged weights (tests/helpers/lora_ref.py, which reads the
adapter keys on its own): fp32 for the mathematical result, bf16 in eager op order for the floor, and the HIP forward -- built
from the state dict alg_lora_merge merged -- has to meet the unchanged factors of tests/_parity.py.  Each adapter is sized so
that the output moves by at least 0.2 relative L2 from the forward without it: a dropped adapter cannot pass."""
import dataclasses
import json
import os

import pytest
import torch
from safetensors.torch import save_file

from alg_amd import CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel, lora
from alg_amd.transformer_cogvideox import CogVideoXTransformerConfig
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
from alg_amd.transformer_wan import WanTransformer3DModel, WanTransformerConfig
from alg_amd.weights import synthetic_state_dict
from helpers import lora_ref
from oracle import dit_oracle, hy_oracle, wan_oracle
from _parity import check_floor, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

SMALL = dict(num_attention_heads=8, attention_head_dim=64, in_channels=16, out_channels=8, num_layers=2,
             time_embed_dim=64, text_embed_dim=128, max_text_seq_length=10, sample_width=12, sample_height=8,
             sample_frames=9, patch_size=2)
B0 = "transformer_blocks.0."
COG_SIX = [B0 + m for m in ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")]
SYNTH = dict(seed=21, std=0.05, randomize_affine=True)


def cog_base():
    cfg = CogVideoXTransformerConfig(**SMALL)
    return cfg, {k: v.cpu() for k, v in synthetic_state_dict(cfg, device=DEV, **SYNTH).items()}


def cog_adapters(sd, rel_std=1.0):
    """rank 4 with alpha 8 on the six linears of block 0 and on attn1.to_q of block 1 (lora_A / lora_B, "transformer." prefix);
    rank 8 at scale 0.5 on ff.net.2 of block 0 as well (lora_down / lora_up, no prefix, no alpha)"""
    first = lora_ref.make_adapter(sd, COG_SIX + ["transformer_blocks.1.attn1.to_q"], 4, seed=1, rel_std=rel_std, alpha=8)
    second = lora_ref.make_adapter(sd, [B0 + "ff.net.2"], 8, seed=2, rel_std=rel_std, prefix="", names=("lora_down", "lora_up"))
    return first, second


def cog_inputs():
    g = torch.Generator().manual_seed(1)
    hs = torch.randn(2, 3, 16, 8, 12, generator=g).to(BF)
    ehs = torch.randn(2, 10, 128, generator=g).to(BF)
    return hs, ehs, torch.tensor([999, 999])


def cog_run(model, hs, ehs, ts, rope):
    return model(hs.to(DEV), ehs.to(DEV), ts, image_rotary_emb=rope, return_dict=False)[0]


def split_ref(merged):
    """the float64-merged dict -> (fp32 weights for the mathematical reference, bf16 weights for the eager floor)"""
    return {k: v.float() for k, v in merged.items()}, {k: v.to(BF) for k, v in merged.items()}


def test_cogvideox_forward_with_two_adapters_against_the_oracle_on_float64_merged_weights():
    cfg, sd = cog_base()
    ocfg = dit_oracle.DiTConfig(**SMALL)
    first, second = cog_adapters(sd)
    specs = [{"path": first, "name": "style"}, (second, 0.5)]
    model = CogVideoXTransformer3DModel.from_synthetic(cfg, device=DEV, lora=specs, **SYNTH)
    assert model.lora_report == (lora.LoraReport("style", 1.0, 7, (4,)), lora.LoraReport("adapter1", 0.5, 1, (8,)))
    w32, wbf = split_ref(lora_ref.merge_ref64(sd, [(first, 1.0), (second, 0.5)]))
    hs, ehs, ts = cog_inputs()
    rope = dit_oracle.rope_tables(ocfg, 64, 96, 3)
    ref = dit_oracle.dit_forward(ocfg, w32, hs.float(), ehs.float(), ts, rope)
    eager = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    out = cog_run(model, hs, ehs, ts, rope)
    check_floor("cog_forward_lora_two_adapters", out, ref, eager, channel_dim=2)
    plain = CogVideoXTransformer3DModel.from_synthetic(cfg, device=DEV, **SYNTH)
    assert plain.lora_report == ()
    moved = rel(out, cog_run(plain, hs, ehs, ts, rope))
    print("cog: the adapters move the output by %.3f relative L2" % moved)
    assert moved >= 0.2, moved
    # the second adapter alone is seen too (ff.net.2 of block 0 carries both)
    one = CogVideoXTransformer3DModel.from_synthetic(cfg, device=DEV, lora=specs[:1], **SYNTH)
    assert rel(cog_run(one, hs, ehs, ts, rope), out) > 1e-2


def test_wan_forward_with_adapters_on_attn1_attn2_and_the_feed_forward():
    kw = dict(num_attention_heads=4, ffn_dim=1024, num_layers=2, text_dim=64, image_dim=64, added_kv_proj_dim=512)
    cfg, ocfg = WanTransformerConfig(**kw), wan_oracle.WanConfig(**kw)
    sd = wan_oracle.init_weights(ocfg, seed=3)
    mods = ["blocks.0.attn1.to_q", "blocks.0.attn1.to_out.0", "blocks.0.attn2.to_k", "blocks.0.attn2.add_v_proj",
            "blocks.0.ffn.net.0.proj", "blocks.1.ffn.net.2"]
    ad = lora_ref.make_adapter(sd, mods, 4, seed=3, rel_std=1.0, alpha=8, dtype=torch.float16)     # an fp16 adapter file's values
    sd_hip = dict(sd)
    sd_hip["blocks.1.ffn.net.2.weight"] = sd["blocks.1.ffn.net.2.weight"].float()                  # a checkpoint may ship fp32
    report = lora.merge_into(sd_hip, [(ad, 1.0)], DEV)
    assert report == (lora.LoraReport("adapter0", 1.0, 6, (4,)),)
    assert all(sd_hip[m + ".weight"].dtype == BF and sd_hip[m + ".weight"].is_cuda for m in mods)
    assert all(sd_hip[k] is sd[k] for k in sd if k[:-len(".weight")] not in mods)                  # untargeted: not touched, not moved
    model = WanTransformer3DModel(cfg, sd_hip, device=DEV)
    merged = lora_ref.merge_ref64(sd, [(ad, 1.0)])
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 36, 3, 16, 24, generator=g).to(BF)
    txt, img = torch.randn(2, 512, 64, generator=g).to(BF), torch.randn(2, 257, 64, generator=g).to(BF)
    t = torch.tensor([999.0, 999.0])
    run = lambda m: m(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                      encoder_hidden_states_image=img.to(DEV), return_dict=False)[0]
    ref = wan_oracle.wan_forward(ocfg, merged, x.float(), t, txt.float(), img.float())
    eager = wan_oracle.wan_forward(ocfg, merged, x, t, txt, img, dtype=BF)
    out = run(model)
    check_floor("wan_forward_lora", out, ref, eager)
    moved = rel(out, run(WanTransformer3DModel(cfg, sd, device=DEV)))
    print("wan: the adapter moves the output by %.3f relative L2" % moved)
    assert moved >= 0.2, moved


def test_hunyuan_forward_with_a_dual_block_and_a_single_block_target():
    kw = dict(num_attention_heads=4, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64,
              pooled_projection_dim=64)
    cfg, ocfg = HunyuanVideoTransformerConfig(**kw), hy_oracle.HyConfig(**kw)
    sd = hy_oracle.init_weights(ocfg, seed=3)
    mods = ["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.add_q_proj", "transformer_blocks.0.ff.net.2",
            "single_transformer_blocks.0.proj_mlp"]
    ad = lora_ref.make_adapter(sd, mods, 4, seed=5, rel_std=1.0, alpha=8, dtype=BF)
    sd_hip = dict(sd)
    report = lora.merge_into(sd_hip, [(ad, 1.0)], DEV)
    assert report == (lora.LoraReport("adapter0", 1.0, 4, (4,)),)
    model = HunyuanVideoTransformer3DModel(cfg, sd_hip, device=DEV)
    merged = lora_ref.merge_ref64(sd, [(ad, 1.0)])
    g = torch.Generator().manual_seed(4)
    x, txt = torch.randn(2, 16, 3, 16, 16, generator=g).to(BF), torch.randn(2, 20, 64, generator=g).to(BF)
    mask = torch.zeros(2, 20)
    mask[0, :13] = 1
    mask[1, :20] = 1
    pooled = torch.randn(2, 64, generator=g).to(BF)
    t = torch.tensor([996.0, 996.0])
    guid = torch.tensor([6000.0, 6000.0]) if cfg.guidance_embeds else None
    run = lambda m: m(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                      encoder_attention_mask=mask.to(DEV).to(BF), pooled_projections=pooled.to(DEV),
                      guidance=None if guid is None else guid.to(DEV), return_dict=False)[0]
    ref = hy_oracle.hy_forward(ocfg, {k: v.float() for k, v in merged.items()}, x.float(), t, txt.float(), mask, pooled.float(), guid)
    eager = hy_oracle.hy_forward(ocfg, merged, x, t, txt, mask, pooled, guid, dtype=BF)
    out = run(model)
    check_floor("hunyuan_forward_lora", out, ref, eager)
    moved = rel(out, run(HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)))
    print("hunyuan: the adapter moves the output by %.3f relative L2" % moved)
    assert moved >= 0.2, moved
    # from_synthetic(lora=) is the same plumbing: merge into its own dict, then the constructor
    from alg_amd.transformer_hunyuan_video import synthetic_state_dict as hy_synth
    ssd = hy_synth(cfg, seed=7, device=DEV)
    rep = lora.merge_into(ssd, [(ad, 1.0)], DEV)
    a = HunyuanVideoTransformer3DModel.from_synthetic(cfg, seed=7, device=DEV, lora=[(ad, 1.0)])
    assert a.lora_report == rep == report
    assert torch.equal(run(a), run(HunyuanVideoTransformer3DModel(cfg, ssd, device=DEV)))


@pytest.mark.parametrize("mode", ["fp8", "fp4", "packed_weights"])
def test_cogvideox_composition_is_plumbing(mode):
    """cls(cfg, merge_into'd dict, ...) and from_synthetic(..., lora=specs, ...) give the same bits in every weight form"""
    cfg, sd = cog_base()
    first, second = cog_adapters(sd)
    specs = [{"path": first, "name": "style"}, (second, 0.5)]
    kw = {mode: True} if mode != "packed_weights" else {}
    dev_sd = synthetic_state_dict(cfg, device=DEV, **SYNTH)
    report = lora.merge_into(dev_sd, specs, DEV)
    by_hand = CogVideoXTransformer3DModel(cfg, dev_sd, device=DEV, **kw)
    loaded = CogVideoXTransformer3DModel.from_synthetic(cfg, device=DEV, lora=specs, **SYNTH, **kw)
    assert loaded.packed_weights and by_hand.packed_weights
    assert [r.name for r in loaded.lora_report] == ["style", "adapter1"] and loaded.lora_report == report
    hs, ehs, ts = cog_inputs()
    rope = dit_oracle.rope_tables(dit_oracle.DiTConfig(**SMALL), 64, 96, 3)
    out = cog_run(loaded, hs, ehs, ts, rope)
    assert torch.equal(out, cog_run(by_hand, hs, ehs, ts, rope)) and torch.isfinite(out.float()).all()
    plain = CogVideoXTransformer3DModel.from_synthetic(cfg, device=DEV, **SYNTH, **kw)
    assert rel(out, cog_run(plain, hs, ehs, ts, rope)) >= 0.2


def test_wan_fp8_composition_and_a_model_without_lora_is_todays():
    kw = dict(num_attention_heads=4, ffn_dim=1024, num_layers=1, text_dim=64, image_dim=64, added_kv_proj_dim=512)
    cfg = WanTransformerConfig(**kw)
    from alg_amd.transformer_wan import synthetic_state_dict as wan_synth
    base = wan_synth(cfg, seed=5, device=DEV)
    ad = lora_ref.make_adapter({k: v.cpu() for k, v in base.items() if v.dim() == 2},
                               ["blocks.0.attn1.to_v", "blocks.0.attn2.to_q", "blocks.0.ffn.net.2"], 4, seed=6, alpha=8)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 36, 3, 16, 24, generator=g).to(BF)
    txt, img = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 257, 64, generator=g).to(BF)
    t = torch.tensor([500.0])
    run = lambda m: m(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                      encoder_hidden_states_image=img.to(DEV), return_dict=False)[0]
    merged = dict(base)
    report = lora.merge_into(merged, [(ad, 1.0)], DEV)
    loaded = WanTransformer3DModel.from_synthetic(cfg, seed=5, device=DEV, fp8=True, lora=[(ad, 1.0)])
    assert loaded.lora_report == report and len(report) == 1
    out = run(loaded)
    assert torch.equal(out, run(WanTransformer3DModel(cfg, merged, device=DEV, fp8=True)))
    # without lora: the keyword at its default, None and an empty list are the constructor on the plain dict, bit for bit
    today = run(WanTransformer3DModel(cfg, base, device=DEV, fp8=True))
    for kwargs in ({}, {"lora": None}, {"lora": []}):
        m = WanTransformer3DModel.from_synthetic(cfg, seed=5, device=DEV, fp8=True, **kwargs)
        assert m.lora_report == () and torch.equal(run(m), today)
    assert not torch.equal(out, today)


def test_end_to_end_checkpoint_directory_adapter_file_and_sampler(tmp_path):
    """A tiny CogVideoX checkpoint directory and an adapter .safetensors file (fp16, global lora_alpha in the metadata): a
    2-step ALG sampler through CogVideoXImageToVideoPipeline.from_pretrained(dir, lora=[(file, 0.8)]) gives the latents of the
    pipeline handed a transformer built from the merge_into dict, and other latents than the run without the adapter."""
    root = str(tmp_path / "ckpt")
    small = dict(SMALL, num_layers=1)
    w = {k: v.to(BF) for k, v in dit_oracle.init_weights(dit_oracle.DiTConfig(**small), seed=4, std=0.05,
                                                          randomize_affine=True).items()}
    d = os.path.join(root, "transformer")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(dataclasses.asdict(CogVideoXTransformerConfig(**small)), _class_name="CogVideoXTransformer3DModel"), f)
    save_file({k: v.contiguous() for k, v in w.items()}, os.path.join(d, "diffusion_pytorch_model.safetensors"))
    ad = lora_ref.make_adapter(w, COG_SIX, 4, seed=9, rel_std=1.0, dtype=torch.float16)
    path = str(tmp_path / "motion.safetensors")
    save_file(ad, path, metadata={"lora_alpha": "8"})

    pipe = CogVideoXImageToVideoPipeline.from_pretrained(root, device=DEV, lora=[(path, 0.8)]).to(DEV)
    assert pipe.transformer.lora_report == (lora.LoraReport("motion", 0.8, 6, (4,)),)
    sd = dict(w)
    lora.merge_into(sd, [(dict(ad, __metadata__={"lora_alpha": "8"}), 0.8)], DEV)      # the dict form of the same file
    by_hand = CogVideoXImageToVideoPipeline(transformer=CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**small), sd, device=DEV),
                                            scheduler=CogVideoXDDIMScheduler()).to(DEV)
    plain = CogVideoXImageToVideoPipeline.from_pretrained(root, device=DEV).to(DEV)
    assert plain.transformer.lora_report == ()
    # ... and a transformer instance passed in is left alone, like fp8=
    kept = CogVideoXImageToVideoPipeline.from_pretrained(root, device=DEV, transformer=plain.transformer, lora=[(path, 0.8)])
    assert kept.transformer is plain.transformer and kept.transformer.lora_report == ()

    g = torch.Generator().manual_seed(42)
    lat = torch.randn(1, 3, 8, 8, 12, generator=g).to(BF)
    first = (torch.randn(1, 1, 8, 8, 12, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)
    args = dict(num_inference_steps=2, guidance_scale=6.0, use_low_pass_guidance=True, lp_filter_type="down_up",
                lp_resize_factor=0.25, lp_strength_schedule_type="interval", schedule_interval_end_time=0.04)
    run = lambda p: p(image_latents=first, latents=lat.clone(), prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=96,
                      num_frames=9, output_type="latent", lp_filter_in_latent=True, **args).frames
    out = run(pipe)
    assert torch.equal(out, run(by_hand))
    assert rel(out, run(plain)) > 1e-2
