"""`transformer.attn_window` of the CogVideoX DiT: the joint self-attention on alg_flash_attn_d64_ranges with the frame-window
tables of alg_amd/attn_window.py (prompt tokens in front: `prefix`).

As in test_gpu_attn_window_models.py the kernel is exact against a masked softmax, so the windowed forward is held to the dense
forward's own standard: the yardstick is the distance between the dense forward and the dense forward whose attention launches
are replaced by fp32 SDPA in torch, and the windowed forward may be FACTOR (tests/_parity.py) x that away from the windowed forward
whose ranged launches are replaced by fp32 MASKED SDPA (the mask from ranges_to_mask).  The fp8 block path is held to the same
standard with both pairs taken in fp8 mode.  The policy's effect on the result is not judged here.

The model: trained-like weights, 8 heads x 64, 2 layers, N = 2, six latent frames of 160 tokens behind 10 prompt tokens (970 rows:
3.8 query blocks; the prompt is no multiple of 64, so every frame begins off the tile grid), window 1."""
import functools
import json
import os

import pytest
import torch

from _parity import FACTOR, rel
from alg_amd import _lib
from alg_amd.attn_window import KvRanges, ranges_to_mask
from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
from alg_amd.schedulers import CogVideoXDDIMScheduler
from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel, CogVideoXTransformerConfig
from helpers.trained_like import trained_like
from helpers.trained_like_cases import COG_SMALL
from oracle import dit_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
LN2 = 0.6931471805599453
FRAMES, LAT_H, LAT_W, TEXT, N = 6, 20, 32, 10, 2          # patch 2: 10 x 16 = 160 tokens per latent frame
HW = (LAT_H // 2) * (LAT_W // 2)
S = TEXT + FRAMES * HW
KW = dict(COG_SMALL, sample_width=LAT_W, sample_height=LAT_H, sample_frames=4 * (FRAMES - 1) + 1)


def _perm(n):
    return torch.tensor([(i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1) for i in range(n)], device=DEV)


def _sdpa_into_o(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, unit, mask=None, q_off=0, k_off=0):
    """What alg_flash_attn_d64_ex / _ranges compute, by torch in fp32 on the same buffers (strides and offsets in elements);
    softmax(unit * q k^T): unit = ln 2 for pre-scaled Q (scores in log2 units), the softmax scale otherwise."""
    view = lambda t, bs, rs, off: torch.as_strided(t.view(-1), (batch, heads, S_, 64), (bs, 64, rs, 1), off)
    qh, kh = view(q, q_bs, q_rs, q_off).float(), view(k, q_bs, q_rs, k_off).float()
    pad = (S_ + 63) // 64 * 64
    vth = torch.as_strided(vt.view(-1), (batch, heads, 64, pad), (vt_bs, 64 * vt_rs, vt_rs, 1), 0)
    vh = vth[..., _perm(pad)[:S_]].float().transpose(-1, -2)              # logical key s sits at column perm(s)
    s = qh @ kh.transpose(-1, -2) * unit
    if mask is not None:
        s = s.masked_fill(~mask.to(s.device), float("-inf"))
    view(o, o_bs, o_rs, 0).copy_((torch.softmax(s, dim=-1) @ vh).to(BF))
    return o


def _patch_dense(monkeypatch):
    """_lib.flash_attn_d64 -> fp32 SDPA."""
    def fake(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, scale, q_off=0, k_off=0, q_prescaled=False):
        return _sdpa_into_o(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, LN2 if q_prescaled else scale,
                            q_off=q_off, k_off=k_off)

    monkeypatch.setattr(_lib, "flash_attn_d64", fake)


def _patch_ranges(monkeypatch):
    """_lib.flash_attn_d64_ranges -> fp32 masked SDPA; returns the list the calls are logged in."""
    calls = []

    def fake(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, kv_ranges, q_off=0, k_off=0):
        assert isinstance(kv_ranges, KvRanges) and (kv_ranges.Sq, kv_ranges.Skv) == (S_, S_)
        calls.append(kv_ranges)
        return _sdpa_into_o(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, LN2,
                            mask=ranges_to_mask(kv_ranges), q_off=q_off, k_off=k_off)

    monkeypatch.setattr(_lib, "flash_attn_d64_ranges", fake)
    return calls


def _count_ranges(monkeypatch):
    """Counts the ranged launches and lets them through."""
    real, calls = _lib.flash_attn_d64_ranges, []

    def counted(*a, **kw):
        calls.append(a[13])
        return real(*a, **kw)

    monkeypatch.setattr(_lib, "flash_attn_d64_ranges", counted)
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


@functools.lru_cache(maxsize=None)
def _setup(layers=2):
    """(config, bf16 weights on the host, inputs on the device): shared and left unchanged."""
    kw = dict(KW, num_layers=layers)
    ocfg = dit_oracle.DiTConfig(**kw)
    w32 = trained_like(dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True))
    wbf = {k: v.to(BF) for k, v in w32.items()}
    g = torch.Generator().manual_seed(4)
    hs = torch.randn(N, FRAMES, kw["in_channels"], LAT_H, LAT_W, generator=g).to(BF).to(DEV)
    ehs = torch.randn(N, TEXT, kw["text_embed_dim"], generator=g).to(BF).to(DEV)
    rope = tuple(r.to(DEV) for r in dit_oracle.rope_tables(ocfg, LAT_H * 8, LAT_W * 8, FRAMES))
    return CogVideoXTransformerConfig(**kw), wbf, (hs, ehs, torch.tensor([999.0] * N, device=DEV), rope)


def _model(layers=2, fp8=False):
    cfg, wbf, inputs = _setup(layers)
    return CogVideoXTransformer3DModel(cfg, wbf, device=DEV, fp8=fp8), cfg, inputs


def _run(model, inputs):
    hs, ehs, ts, rope = inputs
    return model(hs, ehs, ts, image_rotary_emb=rope, return_dict=False)[0].clone()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_cog_window_forward_is_exact_to_the_dense_standard(fp8, monkeypatch):
    model, cfg, inputs = _model(fp8=fp8)
    dense_hip = _run(model, inputs)
    model.attn_window = 1
    win_hip = _run(model, inputs)
    assert bool(torch.isfinite(win_hip.float()).all()) and not torch.equal(win_hip, dense_hip)
    with monkeypatch.context() as m:
        calls = _patch_ranges(m)
        win_ref = _run(model, inputs)
    assert len(calls) == cfg.num_layers and len(set(map(id, calls))) == 1          # one launch per block, one cached table
    assert calls[0].coverage < 1.0 and (calls[0].Sq, calls[0].Skv) == (S, S) and calls[0].is_full is False
    assert list(model._attn_ranges) == [(FRAMES, HW, TEXT, 1, 1)]
    model.attn_window = 0
    with monkeypatch.context() as m:
        _patch_dense(m)
        dense_ref = _run(model, inputs)
    e_win, e_dense = rel(win_hip, win_ref), rel(dense_hip, dense_ref)
    _report("cog_attn_window_F6_hw160_T10_w1" + ("_fp8" if fp8 else ""), e_win, e_dense)
    assert e_dense > 0
    assert e_win <= FACTOR * e_dense, (e_win, e_dense)


def test_cog_window_off_and_covering_window_are_todays_forward(monkeypatch):
    want = _run(*_model()[::2])                                                      # a model whose attribute nobody ever set
    calls = _count_ranges(monkeypatch)
    model, cfg, inputs = _model()
    assert model.attn_window == 0 and model.attn_sink_frames == 1 and model._attn_ranges == {}
    assert torch.equal(_run(model, inputs), want) and not calls and not model._attn_ranges   # off: nothing built or launched
    for w in (FRAMES - 1, FRAMES + 3):
        model.attn_window = w
        assert torch.equal(_run(model, inputs), want) and not calls                 # the window covers the video: the dense launch
    model.attn_window = 1
    on = _run(model, inputs)
    assert len(calls) == cfg.num_layers and len(set(map(id, calls))) == 1 and not torch.equal(on, want)
    model.attn_window = 0
    assert torch.equal(_run(model, inputs), want) and len(calls) == cfg.num_layers  # flipped back
    for switch in ("pair_qkv", "packed_weights"):                                   # composes with the launch-shape switches
        setattr(model, switch, False)
    model.attn_window = 1
    assert torch.equal(_run(model, inputs), on)
    model.pair_qkv, model.fuse_qk_norm = True, True
    assert torch.equal(_run(model, inputs), on)


def test_cog_window_without_prescale_raises():
    model, _, inputs = _model()
    model.attn_window, model.attn_prescale = 1, False
    with pytest.raises(ValueError, match="attn_prescale"):
        _run(model, inputs)
    model.attn_window = 0
    assert bool(torch.isfinite(_run(model, inputs).float()).all())                  # off: the per-score form runs as ever


def test_cog_window_with_step_cache_hits_and_stays_finite():
    model, _, inputs = _model()
    model.attn_window, model.step_cache = 1, 10.0                                   # a threshold every probe passes
    hs, ehs, ts, rope = inputs
    keys = ("cond", "uncond")
    a = model(hs, ehs, ts, image_rotary_emb=rope, return_dict=False, cache_keys=keys)[0].clone()
    b = model(hs, ehs, ts, image_rotary_emb=rope, return_dict=False, cache_keys=keys)[0].clone()
    assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())
    assert [s["hit"] for s in model.step_cache_stats] == [False, True]              # the second forward skipped block 1's launch


def test_cog_sampler_runs_its_first_steps_dense(monkeypatch):
    model, cfg, _ = _model(layers=1)
    model.attn_window = 1
    calls = _count_ranges(monkeypatch)
    g = torch.Generator().manual_seed(8)
    C = cfg.in_channels // 2
    lat = torch.randn(1, FRAMES, C, LAT_H, LAT_W, generator=g).to(BF)
    first = (torch.randn(1, 1, C, LAT_H, LAT_W, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, TEXT, 128, generator=g).to(BF), torch.randn(1, TEXT, 128, generator=g).to(BF)
    seen, during = [], []

    def at_step_end(pipe, i, t, kw):
        seen.append(len(calls))
        during.append(pipe.transformer.attn_window)

    pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
    out = pipe(image=None, image_latents=first, latents=lat, prompt_embeds=pe, negative_prompt_embeds=ne, height=LAT_H * 8,
               width=LAT_W * 8, num_frames=4 * (FRAMES - 1) + 1, num_inference_steps=4, guidance_scale=6.0,
               use_low_pass_guidance=False, output_type="latent", callback_on_step_end=at_step_end, attn_window_dense_steps=2)
    assert bool(torch.isfinite(out.frames.float()).all())
    assert seen == [0, 0, cfg.num_layers, 2 * cfg.num_layers]                       # ranged launches in the last two steps only
    assert during == [1, 1, 1, 1] and model.attn_window == 1                        # set and restored around each forward
