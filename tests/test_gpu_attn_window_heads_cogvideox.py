"""`transformer.attn_window_recall` of the CogVideoX DiT (attn_window.HeadWindowHost on alg_flash_attn_d64_ranges_heads): off it is the
shared-window forward; a threshold no head reaches keeps every head dense and a tiny one every head windowed, bit for bit; mixed
heads are held to the dense forward's own standard against per-head masked fp32 SDPA (the rule and the model of
test_gpu_attn_window_cogvideox.py: 8 heads x 64, 2 layers, N = 2, 10 prompt tokens + 6 frames x 160 = 970 rows, window 1; 16 panels
x 4 query blocks, so the dense entry plans no split tail and is the single launch the calibration forward reproduces); and the
sampler calibrates on its last dense step."""
import pytest
import torch

import test_gpu_attn_window_cogvideox as C
from _parity import FACTOR, rel
from alg_amd import _lib, attn_window
from alg_amd.attn_window import HeadWindowHost, KvRanges, KvRangesHeads, ranges_to_mask
from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
from alg_amd.schedulers import CogVideoXDDIMScheduler

pytestmark = pytest.mark.gpu
DEV, BF, HEADS, N, S, TEXT = C.DEV, C.BF, 8, C.N, C.S, C.TEXT


def run(model, inputs, calibrate=False):
    """One forward as the sampler's pieces make it (attn_window.call_transformer)."""
    hs, ehs, ts, rope = inputs
    return attn_window.call_transformer(model, False, hs, ehs, ts, image_rotary_emb=rope, return_dict=False, calibrate=calibrate)[0].clone()


def count(monkeypatch, name):
    """Logs (table, lse given) of every call of _lib.<name> and lets it through."""
    real, calls = getattr(_lib, name), []

    def counted(*a, **kw):
        calls.append((a[13], kw.get("lse") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(_lib, name, counted)
    return calls


def count_dense(monkeypatch):
    real, calls = _lib.flash_attn_d64, []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(_lib, "flash_attn_d64", counted)
    return calls


def measured(model, inputs):
    """[layers][heads]: the recall of every head (its minimum over the samples) under a throw-away threshold; the model is left
    uncalibrated."""
    saved = model.attn_window_recall
    model.attn_window_recall = 0.5
    run(model, inputs, calibrate=True)
    rec = [[min(r[h] for r in s["recall"]) for h in range(HEADS)] for s in model.attn_window_stats]
    model.reset_attn_window_heads()
    model.attn_window_recall = saved
    return rec


def test_the_model_is_a_head_window_host_and_recall_zero_is_todays_windowed_forward(monkeypatch):
    model, cfg, inputs = C._model()
    assert isinstance(model, HeadWindowHost) and model.attn_window_recall == 0.0
    model.attn_window = 1
    want = run(model, inputs)                             # today's call: no calibrate, attribute at its default
    heads_calls = count(monkeypatch, "flash_attn_d64_ranges_heads")
    shared_calls = count(monkeypatch, "flash_attn_d64_ranges")
    assert torch.equal(run(model, inputs, calibrate=True), want)            # asked to calibrate, but the switch is off
    assert len(shared_calls) == cfg.num_layers and not heads_calls
    assert model.attn_window_stats == [] and model._attn_cal is None and not model.attn_window_calibrated


def test_a_threshold_no_head_reaches_keeps_every_head_dense(monkeypatch):
    model, cfg, inputs = C._model()
    layers = cfg.num_layers
    dense = run(model, inputs)                            # attn_window = 0
    model.attn_window = 1
    top = max(x for row in measured(model, inputs) for x in row)
    print("largest recall measured: %.6f" % top)
    assert top < 1.0
    model.attn_window_recall = 0.5 * (top + 1.0)
    heads_calls = count(monkeypatch, "flash_attn_d64_ranges_heads")
    shared_calls = count(monkeypatch, "flash_attn_d64_ranges")
    dense_calls = count_dense(monkeypatch)
    assert torch.equal(run(model, inputs), dense) and not heads_calls       # uncalibrated: dense
    assert len(dense_calls) == layers
    assert torch.equal(run(model, inputs, calibrate=True), dense)           # the calibration forward's own output
    assert len(heads_calls) == 2 * layers and all(l for _, l in heads_calls) and len(dense_calls) == layers
    stats = model.attn_window_stats
    assert [s["layer"] for s in stats] == list(range(layers)) and model.attn_window_calibrated
    for s in stats:
        assert s["windowed"] == [False] * HEADS and len(s["recall"]) == N and all(len(r) == HEADS for r in s["recall"])
        assert all(0.0 < x <= 1.0 for r in s["recall"] for x in r), s
        print("layer", s["layer"], "recall", [[round(x, 4) for x in r] for r in s["recall"]])
    bufs = model._attn_cal
    for _ in range(2):
        assert torch.equal(run(model, inputs, calibrate=True), dense)       # calibrated: the marker changes nothing any more
    assert len(heads_calls) == 2 * layers and not shared_calls and len(dense_calls) == 3 * layers     # flash_attn_d64 only
    assert model._attn_cal is bufs and model.attn_window_stats is stats
    model.reset_attn_window_heads()
    assert model.attn_window_stats == [] and not model.attn_window_calibrated
    model.attn_sink_frames = 0                             # a changed sink drops the decisions
    model._attn_decided = (("stale",), [])
    assert torch.equal(run(model, inputs), dense) and not model.attn_window_calibrated


def test_a_tiny_threshold_keeps_every_head_windowed(monkeypatch):
    model, cfg, inputs = C._model()
    layers = cfg.num_layers
    dense = run(model, inputs)
    model.attn_window = 1
    windowed = run(model, inputs)                         # today's (recall 0) windowed forward
    assert not torch.equal(windowed, dense)
    model.attn_window_recall = 1e-6
    assert torch.equal(run(model, inputs, calibrate=True), dense)
    assert all(s["windowed"] == [True] * HEADS for s in model.attn_window_stats) and len(model.attn_window_stats) == layers
    heads_calls = count(monkeypatch, "flash_attn_d64_ranges_heads")
    shared_calls = count(monkeypatch, "flash_attn_d64_ranges")
    dense_calls = count_dense(monkeypatch)
    for _ in range(2):
        assert torch.equal(run(model, inputs), windowed)
    assert not heads_calls and not dense_calls and len(shared_calls) == 2 * layers          # today's shared-table launches only


def _patch_heads(monkeypatch):
    """_lib.flash_attn_d64_ranges_heads -> fp32 masked SDPA with the per-head masks of the table; returns the logged tables."""
    calls = []

    def fake(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, kv_ranges, lse=None, q_off=0, k_off=0, lse_off=0):
        assert isinstance(kv_ranges, KvRangesHeads) and (kv_ranges.Sq, kv_ranges.Skv, kv_ranges.heads) == (S_, S_, heads)
        assert lse is None
        calls.append(kv_ranges)
        return C._sdpa_into_o(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, C.LN2,
                              mask=ranges_to_mask(kv_ranges), q_off=q_off, k_off=k_off)

    monkeypatch.setattr(_lib, "flash_attn_d64_ranges_heads", fake)
    return calls


def _patch_shared(monkeypatch):
    """_lib.flash_attn_d64_ranges -> fp32 masked SDPA (a layer whose heads all reach the threshold launches the shared table)."""
    def fake(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, kv_ranges, q_off=0, k_off=0):
        assert isinstance(kv_ranges, KvRanges)
        return C._sdpa_into_o(q, k, vt, o, batch, heads, S_, q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs, C.LN2,
                              mask=ranges_to_mask(kv_ranges), q_off=q_off, k_off=k_off)

    monkeypatch.setattr(_lib, "flash_attn_d64_ranges", fake)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_mixed_heads_forward_is_exact_to_the_dense_standard(fp8, monkeypatch):
    """The threshold is the median of the measured recalls: some heads reach it, some do not.  Every attention launch of the mixed
    forward -- the per-head entry and, in a layer whose heads all fall on one side, the shared-table or the dense entry -- is
    replaced by fp32 (masked) SDPA in the reference, as the dense forward's are in its twin."""
    model, cfg, inputs = C._model(fp8=fp8)
    layers = cfg.num_layers
    dense_hip = run(model, inputs)
    model.attn_window = 1
    shared_hip = run(model, inputs)
    rec = sorted(x for row in measured(model, inputs) for x in row)
    thr = 0.5 * (rec[len(rec) // 2 - 1] + rec[len(rec) // 2])
    print("recalls %s, threshold %.6f" % ([round(x, 4) for x in rec], thr))
    assert rec[0] < thr < rec[-1]
    model.attn_window_recall = thr
    assert torch.equal(run(model, inputs, calibrate=True), dense_hip)       # the calibration forward (fp8: through _block_fp8)
    flags = [w for s in model.attn_window_stats for w in s["windowed"]]
    assert any(flags) and not all(flags)                                    # both kinds of head exist
    mixed_hip = run(model, inputs)
    assert bool(torch.isfinite(mixed_hip.float()).all())
    assert not torch.equal(mixed_hip, dense_hip) and not torch.equal(mixed_hip, shared_hip)
    with monkeypatch.context() as m:
        calls = _patch_heads(m)
        _patch_shared(m)
        C._patch_dense(m)
        mixed_ref = run(model, inputs)
    n_mixed = sum(any(s["windowed"]) and not all(s["windowed"]) for s in model.attn_window_stats)
    assert len(calls) == n_mixed and all(c.coverage < 1.0 for c in calls)
    model.attn_window = 0
    with monkeypatch.context() as m:
        C._patch_dense(m)
        dense_ref = run(model, inputs)
    e_mixed, e_dense = rel(mixed_hip, mixed_ref), rel(dense_hip, dense_ref)
    C._report("cog_attn_window_mixed_heads_F6_hw160_T10_w1" + ("_fp8" if fp8 else ""), e_mixed, e_dense)
    assert e_dense > 0
    assert e_mixed <= FACTOR * e_dense, (e_mixed, e_dense)


def _sampler(model, cfg):
    g = torch.Generator().manual_seed(8)
    Cc = cfg.in_channels // 2
    lat = torch.randn(1, C.FRAMES, Cc, C.LAT_H, C.LAT_W, generator=g).to(BF)
    first = (torch.randn(1, 1, Cc, C.LAT_H, C.LAT_W, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, TEXT, 128, generator=g).to(BF), torch.randn(1, TEXT, 128, generator=g).to(BF)
    pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
    # the low-pass schedule holds on steps 0 and 1 (three passes) and is over on steps 2 and 3 (two passes)
    kw = dict(image=None, image_latents=first, latents=lat, prompt_embeds=pe, negative_prompt_embeds=ne, height=C.LAT_H * 8,
              width=C.LAT_W * 8, num_frames=4 * (C.FRAMES - 1) + 1, num_inference_steps=4, guidance_scale=6.0,
              use_low_pass_guidance=True, lp_filter_type="down_up", lp_resize_factor=0.25, lp_strength_schedule_type="interval",
              schedule_interval_start_time=0.0, schedule_interval_end_time=0.4, lp_filter_in_latent=True, output_type="latent",
              attn_window_dense_steps=2)
    return pipe, kw


def test_cog_sampler_calibrates_on_its_last_dense_step(monkeypatch):
    model, cfg, inputs = C._model()
    L = cfg.num_layers
    pipe, kw = _sampler(model, cfg)
    dense_lat = []
    pipe(callback_on_step_end=lambda p, i, t, k: dense_lat.append(k["latents"].clone()), **kw)       # attn_window = 0

    model.attn_window, model.attn_window_recall = 1, 0.5
    monkeypatch.setattr(attn_window, "decide_heads", lambda recall, thr: [h % 2 == 0 for h in range(len(recall[0]))])
    heads_calls = count(monkeypatch, "flash_attn_d64_ranges_heads")
    resets = []
    real_reset = model.reset_attn_window_heads
    monkeypatch.setattr(model, "reset_attn_window_heads", lambda: (resets.append(1), real_reset())[1])
    lat, seen, calibrated, trace = [], [], [], []

    def at_step_end(p, i, t, k):
        lat.append(k["latents"].clone())
        seen.append((len(heads_calls), sum(l for _, l in heads_calls)))
        calibrated.append(p.transformer.attn_window_calibrated)

    pipe(callback_on_step_end=at_step_end, step_trace=trace, **kw)
    assert [n for _, _, n in trace] == [3, 3, 2, 2]                        # the pass count drops behind the calibration step
    # step 0: dense launches; step 1: the calibration (two launches with lse per layer, three samples); steps 2, 3: one per-head
    # launch per layer with the tables decided on three samples, now on two
    assert seen == [(0, 0), (2 * L, 2 * L), (3 * L, 2 * L), (4 * L, 2 * L)] and calibrated == [False, True, True, True]
    assert torch.equal(lat[0], dense_lat[0]) and torch.equal(lat[1], dense_lat[1])          # steps 0-1 are dense in output
    assert not torch.equal(lat[3], dense_lat[3]) and bool(torch.isfinite(lat[3].float()).all())
    stats = model.attn_window_stats
    assert len(stats) == L and all(len(s["recall"]) == 3 for s in stats) and resets == [1] and model.attn_window == 1

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
    model.step_cache = 0.0

    # ... cfg_split is refused, and so is a capture of the calibration forward
    with pytest.raises(_lib.AlgHipError, match="cfg_split"):
        pipe(cfg_split=object(), **kw)
    model.reset_attn_window_heads()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = run(model, inputs)                                                            # warm-up on the capture stream (dense)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.AlgHipError, match="captured"):
        with torch.cuda.graph(graph, stream=side):
            run(model, inputs, calibrate=True)
    torch.cuda.synchronize()
    assert not model.attn_window_calibrated and model.attn_window_stats == [] and not model._attn_calibrate
    assert torch.equal(run(model, inputs), want)                                             # the model is fine afterwards
