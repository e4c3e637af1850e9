"""The shapes, weights and inputs of the trained-like cases, shared by tests/test_trained_like_cpu.py (the oracle alone) and
tests/test_gpu_trained_like.py (HIP against it): both must look at the same tensors."""
import torch

from helpers.trained_like import trained_like
from oracle import dit_oracle, hy_oracle, wan_oracle

BF = torch.bfloat16

# tests/test_gpu_dit_forward.py's SMALL and its 16-heads ragged variant; MEDIUM: the same widths on a 3 x 32 x 48 latent grid
# (3 x 16 x 24 = 1,152 video + 10 text tokens = 19 KV tiles: the pipelined attention statement needs at least 8)
COG_SMALL = dict(num_attention_heads=8, attention_head_dim=64, in_channels=16, out_channels=8, num_layers=2,
                 time_embed_dim=64, text_embed_dim=128, max_text_seq_length=10, sample_width=12, sample_height=8,
                 sample_frames=9, patch_size=2)
COG = {
    #           config overrides                                                   N  Fr  H   W   T  wseed iseed  t
    "small": (dict(), 3, 3, 8, 12, 10, 3, 1, 999),
    "ragged": (dict(num_attention_heads=16, num_layers=1, max_text_seq_length=7, sample_width=14, sample_height=10),
               2, 3, 10, 14, 7, 8, 2, 459),
    "medium": (dict(sample_width=48, sample_height=32), 2, 3, 32, 48, 10, 3, 1, 999),
}
C2 = dict(num_attention_heads=48, attention_head_dim=64, in_channels=32, out_channels=16, num_layers=2, time_embed_dim=512,
          text_embed_dim=4096, max_text_seq_length=226, sample_width=90, sample_height=60, sample_frames=49, patch_size=2)


def cog_case(name, **profile):
    """-> (config kwargs, oracle config, bf16 weights, (hs, ehs, ts, rope)); `profile` goes to trained_like()."""
    over, N, Fr, H, W, T, wseed, iseed, t = COG[name]
    kw = dict(COG_SMALL, **over)
    ocfg = dit_oracle.DiTConfig(**kw)
    w32 = trained_like(dit_oracle.init_weights(ocfg, seed=wseed, std=0.05, randomize_affine=True), **profile)
    wbf = {k: v.to(BF) for k, v in w32.items()}
    g = torch.Generator().manual_seed(iseed)
    C = kw["in_channels"]
    hs = torch.randn(N, Fr, C, H, W, generator=g).to(BF)
    ehs = torch.randn(N, T, kw["text_embed_dim"], generator=g).to(BF)
    return kw, ocfg, wbf, (hs, ehs, torch.tensor([t] * N), dit_oracle.rope_tables(ocfg, H * 8, W * 8, Fr))


WAN = {"small": (2, 3, 16, 24), "medium": (2, 3, 32, 48)}     # 288 / 1,152 tokens (5 / 18 KV tiles)


def wan_case(name, heads=4, **profile):
    """-> (config kwargs, oracle config, state dict, (x, t, txt, img))."""
    N, F, H, W = WAN[name]
    kw = dict(num_attention_heads=heads, ffn_dim=1024, num_layers=2, text_dim=64, image_dim=64, added_kv_proj_dim=heads * 128)
    ocfg = wan_oracle.WanConfig(**kw)
    sd = trained_like(wan_oracle.init_weights(ocfg, seed=3), **profile)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, 36, F, H, W, generator=g).to(BF)
    txt = torch.randn(N, 512, 64, generator=g).to(BF)
    img = torch.randn(N, 257, 64, generator=g).to(BF)
    return kw, ocfg, sd, (x, torch.tensor([999.0] * N), txt, img)


def hy_case(mode, **profile):
    """tests/test_gpu_hunyuan_forward.py's small(): -> (config kwargs, oracle config, state dict, (x, t, txt, mask, pooled, guidance))."""
    kw = dict(num_attention_heads=4, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64,
              pooled_projection_dim=64)
    kw.update(dict(image_condition_type="token_replace", guidance_embeds=False) if mode == "token_replace" else
              dict(image_condition_type="latent_concat", guidance_embeds=True))
    ocfg = hy_oracle.HyConfig(**kw)
    sd = trained_like(hy_oracle.init_weights(ocfg, seed=3), **profile)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 3, 16, 16, generator=g).to(BF)
    txt = torch.randn(2, 20, 64, generator=g).to(BF)
    mask = torch.zeros(2, 20)
    mask[0, :13] = 1
    mask[1] = 1
    pooled = torch.randn(2, 64, generator=g).to(BF)
    guid = torch.tensor([6000.0, 6000.0]) if kw["guidance_embeds"] else None
    return kw, ocfg, sd, (x, torch.tensor([996.0, 996.0]), txt, mask, pooled, guid)
