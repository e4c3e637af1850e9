"""`transformer.attn_window` of the Wan and HunyuanVideo DiTs: the large self-attention on alg_flash_attn_d128_ranges with the
frame-window tables of alg_amd/attn_window.py.

The kernel is exact against a masked softmax, so the windowed forward is held to the dense forward's own standard: the yardstick
is the distance between the dense forward and the dense forward whose self-attention launches are replaced by fp32 SDPA in torch,
and the windowed forward may be FACTOR (tests/_parity.py) x that away from the windowed forward whose ranged launches are
replaced by fp32 MASKED SDPA (the mask from ranges_to_mask).  The policy's effect on the result is not judged here."""
import json
import os

import pytest
import torch

from _parity import FACTOR, rel
from alg_amd import _lib
from alg_amd.attn_window import KvRanges, ranges_to_mask
from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
from alg_amd.schedulers import UniPCMultistepScheduler
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
from alg_amd.transformer_wan import WanTransformer3DModel, WanTransformerConfig
from helpers.trained_like import trained_like
from oracle import hy_oracle, wan_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
HEADS = 4      # 4 heads x 128: the models' norm kernels take dim % 512 == 0, so 2 heads (dim 256) is not a model they can run


def _perm(n):
    return torch.tensor([(i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1) for i in range(n)], device=DEV)


def _sdpa_into_o(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale, mask=None,
                 q_off=0, k_off=0, vt_off=0, o_off=0):
    """What alg_flash_attn_d128 / _ranges compute, by torch in fp32 on the same buffers (strides and offsets in elements)."""
    view = lambda t, rows, bs, rs, off: torch.as_strided(t.view(-1), (batch, heads, rows, 128), (bs, 128, rs, 1), off)
    qh, kh = view(q, Sq, q_bs, q_rs, q_off).float(), view(k, Skv, k_bs, k_rs, k_off).float()
    pad = (Skv + 63) // 64 * 64
    vth = torch.as_strided(vt.view(-1), (batch, heads, 128, pad), (vt_bs, 128 * vt_rs, vt_rs, 1), vt_off)
    vh = vth[..., _perm(pad)[:Skv]].float().transpose(-1, -2)              # logical key s sits at column perm(s)
    s = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(~mask.to(s.device), float("-inf"))
    view(o, Sq, o_bs, o_rs, o_off).copy_((torch.softmax(s, dim=-1) @ vh).to(BF))
    return o


def _patch_dense(monkeypatch, Sq_self):
    """_lib.flash_attn_d128 -> fp32 SDPA for the self-attention launches (Sq == Sq_self); any other launch stays."""
    real = _lib.flash_attn_d128

    def fake(q, k, vt, o, batch, heads, Sq, *a, **kw):
        if Sq != Sq_self or kw.get("kv_group", 1) != 1 or kw.get("causal", False):
            return real(q, k, vt, o, batch, heads, Sq, *a, **kw)
        return _sdpa_into_o(q, k, vt, o, batch, heads, Sq, *a, **kw)

    monkeypatch.setattr(_lib, "flash_attn_d128", fake)


def _patch_ranges(monkeypatch):
    """_lib.flash_attn_d128_ranges -> fp32 masked SDPA; returns the list the calls are logged in."""
    calls = []

    def fake(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale, kv_ranges, **kw):
        assert isinstance(kv_ranges, KvRanges) and (kv_ranges.Sq, kv_ranges.Skv) == (Sq, Skv)
        calls.append(kv_ranges)
        return _sdpa_into_o(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale,
                            mask=ranges_to_mask(kv_ranges), **kw)

    monkeypatch.setattr(_lib, "flash_attn_d128_ranges", fake)
    return calls


def _count_ranges(monkeypatch):
    """Counts the ranged launches and lets them through."""
    real, calls = _lib.flash_attn_d128_ranges, []

    def counted(*a, **kw):
        calls.append(a[17])
        return real(*a, **kw)

    monkeypatch.setattr(_lib, "flash_attn_d128_ranges", counted)
    return calls


def _report(case, e_win, e_dense):
    print("%s: windowed HIP vs masked fp32 SDPA %.3e; dense HIP vs fp32 SDPA %.3e (ratio %.2f, bound %.1f)"
          % (case, e_win, e_dense, e_win / max(e_dense, 1e-30), FACTOR))
    dest = os.environ.get("ALG_PARITY_REPORT", "")
    if dest.endswith(".jsonl"):          # a file name: the pair is appended there (any other value: printed only)
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "a") as f:
            f.write(json.dumps({"case": case, "err_windowed_hip_vs_masked_sdpa": e_win, "err_dense_hip_vs_sdpa": e_dense,
                                "ratio": e_win / max(e_dense, 1e-30), "factor": FACTOR, "passed": e_win <= FACTOR * e_dense}) + "\n")


# ---- Wan: F = 6 latent frames of hw = 160 tokens (960 tokens: 3.75 query blocks), window 1, N = 2 -----------------------------------
WAN_F, WAN_HW = 6, 160


def _wan_setup(layers=2):
    kw = dict(num_attention_heads=HEADS, ffn_dim=512, num_layers=layers, text_dim=64, image_dim=64, added_kv_proj_dim=HEADS * 128)
    cfg, ocfg = WanTransformerConfig(**kw), wan_oracle.WanConfig(**kw)
    sd = trained_like(wan_oracle.init_weights(ocfg, seed=3))
    g = torch.Generator().manual_seed(4)
    N = 2
    x = torch.randn(N, 36, WAN_F, 20, 32, generator=g).to(BF)          # patch (1, 2, 2): 10 x 16 = 160 tokens per frame
    txt = torch.randn(N, 512, 64, generator=g).to(BF)
    img = torch.randn(N, 257, 64, generator=g).to(BF)
    return cfg, sd, (x, torch.tensor([999.0] * N), txt, img)


def _wan_run(model, inputs):
    x, t, txt, img = inputs
    return model(x.to(DEV), t.to(DEV), txt.to(DEV), img.to(DEV), return_dict=False)[0].clone()


def test_wan_window_forward_is_exact_to_the_dense_standard(monkeypatch):
    cfg, sd, inputs = _wan_setup()
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    S = WAN_F * WAN_HW
    dense_hip = _wan_run(model, inputs)
    model.attn_window = 1
    win_hip = _wan_run(model, inputs)
    assert bool(torch.isfinite(win_hip.float()).all()) and not torch.equal(win_hip, dense_hip)
    with monkeypatch.context() as m:
        calls = _patch_ranges(m)
        win_ref = _wan_run(model, inputs)
    assert len(calls) == cfg.num_layers and len(set(map(id, calls))) == 1          # one launch per block, one cached table
    assert calls[0].coverage < 1.0 and (calls[0].Sq, calls[0].Skv) == (S, S)
    model.attn_window = 0
    with monkeypatch.context() as m:
        _patch_dense(m, S)
        dense_ref = _wan_run(model, inputs)
    e_win, e_dense = rel(win_hip, win_ref), rel(dense_hip, dense_ref)
    _report("wan_attn_window_F6_hw160_w1", e_win, e_dense)
    assert e_dense > 0
    assert e_win <= FACTOR * e_dense, (e_win, e_dense)


def test_wan_window_off_and_covering_window_are_todays_forward(monkeypatch):
    cfg, sd, inputs = _wan_setup()
    want = _wan_run(WanTransformer3DModel(cfg, sd, device=DEV), inputs)           # a model whose attribute nobody ever set
    calls = _count_ranges(monkeypatch)
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    assert model.attn_window == 0 and model.attn_sink_frames == 1
    assert torch.equal(_wan_run(model, inputs), want) and not calls and not model._attn_ranges   # off: nothing built or launched
    for w in (WAN_F - 1, WAN_F + 3):
        model.attn_window = w
        assert torch.equal(_wan_run(model, inputs), want) and not calls             # the window covers the video: the dense launch
    model.attn_window = 1
    on = _wan_run(model, inputs)
    assert len(calls) == cfg.num_layers and not torch.equal(on, want)
    model.attn_window = 0
    assert torch.equal(_wan_run(model, inputs), want) and len(calls) == cfg.num_layers          # flipped back


def test_wan_window_with_fp8_attention_raises():
    cfg, sd, inputs = _wan_setup()
    model = WanTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    model.attn_window = 1
    with pytest.raises(ValueError, match="fp8_attention"):
        _wan_run(model, inputs)


def test_wan_sampler_runs_its_first_steps_dense(monkeypatch):
    cfg, sd, _ = _wan_setup(layers=1)
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    model.attn_window = 1
    calls = _count_ranges(monkeypatch)
    g = torch.Generator().manual_seed(8)
    lat, cond = torch.randn(1, 16, WAN_F, 20, 32, generator=g), torch.randn(1, 20, WAN_F, 20, 32, generator=g)
    pe, ne = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 512, 64, generator=g).to(BF)
    ie = torch.randn(1, 257, 64, generator=g).to(BF)
    seen, during = [], []

    def at_step_end(pipe, i, t, kw):
        seen.append(len(calls))
        during.append(pipe.transformer.attn_window)

    pipe = WanImageToVideoPipeline(transformer=model, scheduler=UniPCMultistepScheduler(flow_shift=3.0)).to(DEV)
    out = pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), image_embeds=ie.to(DEV), image_condition=cond.to(DEV),
               latents=lat.to(DEV), height=160, width=256, num_frames=4 * (WAN_F - 1) + 1, num_inference_steps=4,
               guidance_scale=5.0, output_type="latent", callback_on_step_end=at_step_end, attn_window_dense_steps=2)
    assert bool(torch.isfinite(out.frames.float()).all())
    assert seen == [0, 0, cfg.num_layers, 2 * cfg.num_layers]                       # ranged launches in the last two steps only
    assert during == [1, 1, 1, 1] and model.attn_window == 1                        # set and restored around each forward


# ---- HunyuanVideo: F = 5 latent frames of hw = 104 tokens, prompt length 32 with valid = [20, 32], window 1 ---------------------------
HY_F, HY_HW, HY_L, HY_VALID = 5, 104, 32, (20, 32)


def _hy_setup():
    kw = dict(num_attention_heads=HEADS, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64,
              pooled_projection_dim=64, image_condition_type="token_replace", guidance_embeds=False)
    cfg, ocfg = HunyuanVideoTransformerConfig(**kw), hy_oracle.HyConfig(**kw)
    sd = trained_like(hy_oracle.init_weights(ocfg, seed=3))
    N = len(HY_VALID)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, 16, HY_F, 16, 26, generator=g).to(BF)                       # patch 2: 8 x 13 = 104 tokens per frame
    txt = torch.randn(N, HY_L, 64, generator=g).to(BF)
    mask = torch.zeros(N, HY_L)
    for b, v in enumerate(HY_VALID):
        mask[b, :v] = 1
    pooled = torch.randn(N, 64, generator=g).to(BF)
    return cfg, sd, (x, torch.tensor([996.0] * N), txt, mask, pooled)


def _hy_run(model, inputs):
    x, t, txt, mask, pooled = inputs
    return model(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                 encoder_attention_mask=mask.to(DEV).to(BF), pooled_projections=pooled.to(DEV), return_dict=False)[0].clone()


def test_hunyuan_window_forward_is_exact_to_the_dense_standard(monkeypatch):
    cfg, sd, inputs = _hy_setup()
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    S, J = HY_F * HY_HW, HY_F * HY_HW + HY_L
    blocks = cfg.num_layers + cfg.num_single_layers
    dense_hip = _hy_run(model, inputs)
    model.attn_window = 1
    win_hip = _hy_run(model, inputs)
    assert bool(torch.isfinite(win_hip.float()).all()) and not torch.equal(win_hip, dense_hip)
    with monkeypatch.context() as m:
        calls = _patch_ranges(m)
        win_ref = _hy_run(model, inputs)
    assert len(calls) == blocks * len(HY_VALID) and len(set(map(id, calls))) == len(HY_VALID)   # per sample, one table each
    assert sorted({c.Skv for c in calls}) == [S + v for v in sorted(HY_VALID)] and all(c.Sq == J and c.coverage < 1 for c in calls)
    model.attn_window = 0
    with monkeypatch.context() as m:
        _patch_dense(m, J)                                                           # (the token refiner's launches stay)
        dense_ref = _hy_run(model, inputs)
    e_win, e_dense = rel(win_hip, win_ref), rel(dense_hip, dense_ref)
    _report("hunyuan_attn_window_F5_hw104_w1", e_win, e_dense)
    assert e_dense > 0
    assert e_win <= FACTOR * e_dense, (e_win, e_dense)


def test_hunyuan_window_off_and_covering_window_are_todays_forward(monkeypatch):
    cfg, sd, inputs = _hy_setup()
    want = _hy_run(HunyuanVideoTransformer3DModel(cfg, sd, device=DEV), inputs)
    calls = _count_ranges(monkeypatch)
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    assert model.attn_window == 0 and model.attn_sink_frames == 1
    assert torch.equal(_hy_run(model, inputs), want) and not calls and not model._attn_ranges
    for w in (HY_F - 1, HY_F + 3):
        model.attn_window = w
        assert torch.equal(_hy_run(model, inputs), want) and not calls
    model.attn_window = 1
    on = _hy_run(model, inputs)
    assert len(calls) == (cfg.num_layers + cfg.num_single_layers) * len(HY_VALID) and not torch.equal(on, want)
    model.attn_window = 0
    assert torch.equal(_hy_run(model, inputs), want)


def test_hunyuan_window_with_fp8_attention_raises():
    cfg, sd, inputs = _hy_setup()
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    model.attn_window = 1
    with pytest.raises(ValueError, match="fp8_attention"):
        _hy_run(model, inputs)
