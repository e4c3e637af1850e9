"""`transformer.attn_window_recall` of the Wan and HunyuanVideo DiTs (attn_window.HeadWindowHost): off it is the shared-window
forward; an unreachable threshold keeps every head dense and a tiny one every head windowed, bit for bit; mixed heads are held to
the dense forward's own standard against per-head masked fp32 SDPA (the rule of test_gpu_attn_window_models.py, whose set-ups
these tests use); and the Wan sampler calibrates on its last dense step."""
import pytest
import torch

import test_gpu_attn_window_models as M
from _parity import FACTOR, rel
from alg_amd import _lib, attn_window
from alg_amd.attn_window import KvRanges, KvRangesHeads, ranges_to_mask
from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
from alg_amd.schedulers import UniPCMultistepScheduler
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
from alg_amd.transformer_wan import WanTransformer3DModel

pytestmark = pytest.mark.gpu
DEV, BF, HEADS = M.DEV, M.BF, M.HEADS


@pytest.fixture(autouse=True)
def _q64_for_every_call(monkeypatch):
    """ALG_ATTN128_Q64=2: the dense launches of these small shapes run the kernel the ranged entries run."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")


class Wan:
    name = "wan"

    @staticmethod
    def build():
        cfg, sd, inputs = M._wan_setup()
        return WanTransformer3DModel(cfg, sd, device=DEV), inputs, cfg.num_layers, 2, M.WAN_F * M.WAN_HW

    @staticmethod
    def args(inputs):
        x, t, txt, img = inputs
        return (x.to(DEV), t.to(DEV), txt.to(DEV), img.to(DEV)), dict(return_dict=False)


class Hy:
    name = "hunyuan"

    @staticmethod
    def build():
        cfg, sd, inputs = M._hy_setup()
        return (HunyuanVideoTransformer3DModel(cfg, sd, device=DEV), inputs, cfg.num_layers + cfg.num_single_layers, len(M.HY_VALID),
                M.HY_F * M.HY_HW + M.HY_L)

    @staticmethod
    def args(inputs):
        x, t, txt, mask, pooled = inputs
        return (), dict(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                        encoder_attention_mask=mask.to(DEV).to(BF), pooled_projections=pooled.to(DEV), return_dict=False)


FAMILIES = [Wan, Hy]


def run(fam, model, inputs, calibrate=False):
    """One forward as the samplers make it (attn_window.call_transformer)."""
    a, kw = fam.args(inputs)
    return attn_window.call_transformer(model, False, *a, calibrate=calibrate, **kw)[0].clone()


def count(monkeypatch, name):
    real, calls = getattr(_lib, name), []

    def counted(*a, **kw):
        calls.append((a[17], kw.get("lse") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(_lib, name, counted)
    return calls


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_recall_zero_is_todays_windowed_forward(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    model.attn_window = 1
    want = run(fam, model, inputs)                        # today's call: no calibrate, attribute at its default
    heads_calls = count(monkeypatch, "flash_attn_d128_ranges_heads")
    assert model.attn_window_recall == 0.0
    assert torch.equal(run(fam, model, inputs, calibrate=True), want)       # asked to calibrate, but the switch is off
    assert model.attn_window_stats == [] and model._attn_cal is None and not model.attn_window_calibrated and not heads_calls


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_unreachable_threshold_keeps_every_head_dense(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    dense = run(fam, model, inputs)                       # attn_window = 0
    model.attn_window, model.attn_window_recall = 1, 2.0
    heads_calls = count(monkeypatch, "flash_attn_d128_ranges_heads")
    shared_calls = count(monkeypatch, "flash_attn_d128_ranges")
    assert torch.equal(run(fam, model, inputs), dense) and not heads_calls and model._attn_cal is None   # uncalibrated: dense
    assert torch.equal(run(fam, model, inputs, calibrate=True), dense)      # the calibration forward's own output
    per_layer = 2 * (N if fam is Hy else 1)
    assert len(heads_calls) == per_layer * layers and sum(l for _, l in heads_calls) == len(heads_calls)
    stats = model.attn_window_stats
    assert [s["layer"] for s in stats] == list(range(layers)) and model.attn_window_calibrated
    for s in stats:
        assert s["windowed"] == [False] * HEADS and len(s["recall"]) == N and all(len(r) == HEADS for r in s["recall"])
        assert all(0.0 <= x <= 1.0 for r in s["recall"] for x in r), s
        print(fam.name, "layer", s["layer"], "recall", [[round(x, 4) for x in r] for r in s["recall"]])
    bufs = model._attn_cal
    for _ in range(2):
        assert torch.equal(run(fam, model, inputs, calibrate=True), dense)  # calibrated: the marker changes nothing any more
    assert len(heads_calls) == per_layer * layers and not shared_calls and model._attn_cal is bufs and model.attn_window_stats is stats
    model.reset_attn_window_heads()
    assert model.attn_window_stats == [] and not model.attn_window_calibrated
    model.attn_sink_frames = 0                             # a changed sink drops the decisions
    model._attn_decided = (("stale",), [])
    assert torch.equal(run(fam, model, inputs), dense) and not model.attn_window_calibrated


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_tiny_threshold_keeps_every_head_windowed(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    dense = run(fam, model, inputs)
    model.attn_window = 1
    windowed = run(fam, model, inputs)                    # today's windowed forward
    assert not torch.equal(windowed, dense)
    model.attn_window_recall = 1e-9
    assert torch.equal(run(fam, model, inputs, calibrate=True), dense)
    assert all(s["windowed"] == [True] * HEADS for s in model.attn_window_stats) and len(model.attn_window_stats) == layers
    heads_calls = count(monkeypatch, "flash_attn_d128_ranges_heads")
    shared_calls = count(monkeypatch, "flash_attn_d128_ranges")
    for _ in range(2):
        assert torch.equal(run(fam, model, inputs), windowed)
    assert not heads_calls and len(shared_calls) == 2 * layers * (N if fam is Hy else 1)     # today's shared-table launches


def _patch_heads(monkeypatch):
    """_lib.flash_attn_d128_ranges_heads -> fp32 masked SDPA with the per-head masks of the table; returns the logged tables."""
    calls = []

    def fake(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale, kv_ranges, lse=None, **kw):
        assert isinstance(kv_ranges, KvRangesHeads) and (kv_ranges.Sq, kv_ranges.Skv, kv_ranges.heads) == (Sq, Skv, heads)
        assert lse is None
        calls.append(kv_ranges)
        return M._sdpa_into_o(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale,
                              mask=ranges_to_mask(kv_ranges), **kw)

    monkeypatch.setattr(_lib, "flash_attn_d128_ranges_heads", fake)
    return calls


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_mixed_heads_forward_is_exact_to_the_dense_standard(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    dense_hip = run(fam, model, inputs)
    model.attn_window = 1
    shared_hip = run(fam, model, inputs)
    model.attn_window_recall = 0.5
    with monkeypatch.context() as m:
        m.setattr(attn_window, "decide_heads", lambda recall, thr: [h % 2 == 0 for h in range(len(recall[0]))])
        assert torch.equal(run(fam, model, inputs, calibrate=True), dense_hip)
    assert all(s["windowed"] == [True, False] * (HEADS // 2) for s in model.attn_window_stats)
    mixed_hip = run(fam, model, inputs)
    assert bool(torch.isfinite(mixed_hip.float()).all())
    assert not torch.equal(mixed_hip, dense_hip) and not torch.equal(mixed_hip, shared_hip)
    with monkeypatch.context() as m:
        calls = _patch_heads(m)
        mixed_ref = run(fam, model, inputs)
    assert len(calls) == layers * (N if fam is Hy else 1) and all(c.coverage < 1.0 for c in calls)
    assert len(set(map(id, calls))) == (N if fam is Hy else 1)             # one cached table per base table: the layers share it
    model.attn_window = 0
    with monkeypatch.context() as m:
        M._patch_dense(m, Sq)
        dense_ref = run(fam, model, inputs)
    e_mixed, e_dense = rel(mixed_hip, mixed_ref), rel(dense_hip, dense_ref)
    M._report(fam.name + "_attn_window_mixed_heads_w1", e_mixed, e_dense)
    assert e_dense > 0
    assert e_mixed <= FACTOR * e_dense, (e_mixed, e_dense)


def _sampler(model):
    g = torch.Generator().manual_seed(8)
    lat, cond = torch.randn(1, 16, M.WAN_F, 20, 32, generator=g), torch.randn(1, 20, M.WAN_F, 20, 32, generator=g)
    pe, ne = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 512, 64, generator=g).to(BF)
    ie = torch.randn(1, 257, 64, generator=g).to(BF)
    pipe = WanImageToVideoPipeline(transformer=model, scheduler=UniPCMultistepScheduler(flow_shift=3.0)).to(DEV)
    kw = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), image_embeds=ie.to(DEV), image_condition=cond.to(DEV),
              latents=lat.to(DEV), height=160, width=256, num_frames=4 * (M.WAN_F - 1) + 1, num_inference_steps=4, guidance_scale=5.0,
              output_type="latent", attn_window_dense_steps=2)
    return pipe, kw


def test_wan_sampler_calibrates_on_its_last_dense_step(monkeypatch):
    cfg, sd, _ = M._wan_setup(layers=2)
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    pipe, kw = _sampler(model)
    dense_lat = []
    pipe(callback_on_step_end=lambda p, i, t, k: dense_lat.append(k["latents"].clone()), **kw)       # attn_window = 0

    model.attn_window, model.attn_window_recall = 1, 0.5
    monkeypatch.setattr(attn_window, "decide_heads", lambda recall, thr: [h % 2 == 0 for h in range(len(recall[0]))])
    heads_calls = count(monkeypatch, "flash_attn_d128_ranges_heads")
    resets = []
    real_reset = model.reset_attn_window_heads
    monkeypatch.setattr(model, "reset_attn_window_heads", lambda: (resets.append(1), real_reset())[1])
    lat, seen, calibrated = [], [], []

    def at_step_end(p, i, t, k):
        lat.append(k["latents"].clone())
        seen.append((len(heads_calls), sum(l for _, l in heads_calls)))
        calibrated.append(p.transformer.attn_window_calibrated)

    pipe(callback_on_step_end=at_step_end, **kw)
    L = cfg.num_layers
    # step 0: dense launches; step 1: the calibration (two launches with lse per layer); steps 2, 3: one per-head launch per layer
    assert seen == [(0, 0), (2 * L, 2 * L), (3 * L, 2 * L), (4 * L, 2 * L)] and calibrated == [False, True, True, True]
    assert torch.equal(lat[0], dense_lat[0]) and torch.equal(lat[1], dense_lat[1])          # steps 0-1 are dense in output
    assert not torch.equal(lat[3], dense_lat[3]) and bool(torch.isfinite(lat[3].float()).all())
    stats = model.attn_window_stats
    assert len(stats) == L and resets == [1] and model.attn_window == 1

    # the next video starts from no decision ...
    pipe(callback_on_step_end=at_step_end, **kw)
    assert resets == [1, 1] and model.attn_window_stats is not stats and calibrated[4:] == [False, True, True, True]
    assert torch.equal(lat[7], lat[3])

    # ... an active step cache is forced to compute the calibration forward (threshold 1e9: every unforced forward hits) ...
    model.step_cache = 1e9
    del seen[:]
    pipe(callback_on_step_end=at_step_end, **kw)
    assert len(model.attn_window_stats) == L and seen[1][1] - seen[0][1] == 2 * L          # every layer measured on step 1
    rec = model.step_cache_stats
    assert [r["forced"] for r in rec] == [False, True, False, True] and not rec[1]["hit"]
    assert rec[2]["hit"] and seen[2][0] - seen[1][0] == 1                                    # while step 2 did skip the tail
    model.step_cache = 0.0

    # ... cfg_split is refused, and so is a capture of the calibration forward
    with pytest.raises(_lib.AlgHipError, match="cfg_split"):
        pipe(cfg_split=object(), **kw)
    model.reset_attn_window_heads()
    inputs = tuple(t.to(DEV) for t in M._wan_setup(layers=2)[2])                            # on the device before any capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = run(Wan, model, inputs)                                                       # warm-up on the capture stream (dense)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.AlgHipError, match="captured"):
        with torch.cuda.graph(graph, stream=side):
            run(Wan, model, inputs, calibrate=True)
    torch.cuda.synchronize()
    assert not model.attn_window_calibrated and model.attn_window_stats == [] and not model._attn_calibrate
    assert torch.equal(run(Wan, model, inputs), want)                                        # the model is fine afterwards
