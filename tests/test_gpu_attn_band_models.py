"""`transformer.attn_band` of the Wan DiT (attn_window.HeadWindowHost; the set-up of test_gpu_attn_window_models.py: 2 layers, 4
heads, F = 6, HW = 160, N = 2): off it is the recall policy's forward, launch for launch; an unreachable threshold keeps every
head dense; a tiny one gives every head the cheaper candidate; a forced mix of band, window and dense heads is held to the dense
forward's own standard against per-head masked fp32 SDPA, keeps its bits under every launch order and replays from a graph; the
refusals; and the sampler calibrates on its last dense step."""
import pytest
import torch

import test_gpu_attn_window_heads_models as HM
import test_gpu_attn_window_models as M
from _parity import FACTOR, rel
from alg_amd import _lib, attn_window
from alg_amd.attn_window import (KvRanges, KvRangesHeads, frame_window_ranges, mean_unit_cost, position_band_ranges,
                                 position_major_index, ranges_to_mask)
from alg_amd.transformer_wan import WanTransformer3DModel

pytestmark = pytest.mark.gpu
DEV, BF, HEADS = M.DEV, M.BF, M.HEADS
Wan, run = HM.Wan, HM.run
F, HW = M.WAN_F, M.WAN_HW
S = F * HW
BAND = 2
HEADS_FAMILY = ("flash_attn_d128_ranges_heads", "flash_attn_d128_ranges_order", "flash_attn_d128_ranges", "flash_attn_d128")
LAYOUT = ("attn_rows_position_major", "attn_vt_position_major")
MIX = ["band", "window", "dense", "band"]


@pytest.fixture(autouse=True)
def _q64_for_every_call(monkeypatch):
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")


def launches(monkeypatch):
    """Logs (name, Sq) of every attention and layout launch and lets it through; self-attention launches have Sq == S heads == any."""
    log = []
    for name in HEADS_FAMILY + LAYOUT:
        real = getattr(_lib, name)

        def logged(*a, _real=real, _name=name, **kw):
            if _name in LAYOUT or a[6] == S:                              # (cross-attention has Sq == S too: told apart by Skv)
                if _name in LAYOUT or a[7] == S:
                    log.append((_name, kw.get("lse") is not None))
            return _real(*a, **kw)

        monkeypatch.setattr(_lib, name, logged)
    return log


def names(log):
    return [n for n, _ in log]


def test_band_zero_is_the_recall_policys_forward(monkeypatch):
    """attn_band = 0: forwards, stats records and launches are what the recall policy alone gives (a model whose attribute nobody
    set), and nothing is allocated for the band."""
    outs, stats, logs = [], [], []
    for touch in (False, True):
        model, inputs, layers, N, Sq = Wan.build()
        model.attn_window, model.attn_window_recall = 1, 0.5
        if touch:
            model.attn_band = 0
        with monkeypatch.context() as m:
            m.setattr(attn_window, "decide_heads", lambda recall, thr: [h % 2 == 0 for h in range(len(recall[0]))])
            log = launches(m)
            outs.append([run(Wan, model, inputs), run(Wan, model, inputs, calibrate=True), run(Wan, model, inputs)])
        stats.append(model.attn_window_stats)
        logs.append(log)
        assert model._band_ws is None and not model._attn_band_plans and not hasattr(model._attn_cal, "lse_band")
        assert not any(n in LAYOUT for n in names(log))
        assert all(set(s) == {"layer", "recall", "windowed"} for s in model.attn_window_stats)
        assert model._attn_decided[0] == ((F, HW, 1, 1), 0.5)             # today's key
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and stats[0] == stats[1] and logs[0] == logs[1]
    L = 2
    assert names(logs[0]) == ["flash_attn_d128"] * L + ["flash_attn_d128_ranges_heads"] * 2 * L + ["flash_attn_d128_ranges_heads"] * L


def test_unreachable_threshold_keeps_every_head_dense(monkeypatch):
    model, inputs, layers, N, Sq = Wan.build()
    dense = run(Wan, model, inputs)
    model.attn_window, model.attn_window_recall, model.attn_band = 1, 2.0, BAND
    log = launches(monkeypatch)
    assert torch.equal(run(Wan, model, inputs), dense) and model._attn_cal is None and model._band_ws is None   # uncalibrated: dense
    del log[:]
    assert torch.equal(run(Wan, model, inputs, calibrate=True), dense)     # the calibration forward's output is the dense one
    per_layer = ["flash_attn_d128_ranges_heads", "flash_attn_d128_ranges_heads", "attn_rows_position_major", "attn_rows_position_major",
                 "attn_vt_position_major", "flash_attn_d128_ranges_heads"]
    assert names(log) == per_layer * layers and sum(l for n, l in log) == 3 * layers       # three _heads launches with lse per layer
    stats = model.attn_window_stats
    assert len(stats) == layers and model.attn_window_calibrated
    cov = position_band_ranges(F, HW, BAND).coverage
    for s in stats:
        assert s["layout"] == ["dense"] * HEADS and s["windowed"] == [False] * HEADS
        assert len(s["recall_band"]) == N and all(len(r) == HEADS for r in s["recall_band"])
        assert all(0.0 <= x <= 1.0 for r in s["recall_band"] + s["recall"] for x in r), s
        print("layer", s["layer"], "recall_band", [[round(x, 4) for x in r] for r in s["recall_band"]], "band coverage %.4f" % cov)
    assert tuple(model._attn_cal.recall_band.shape) == (layers, N, HEADS)
    assert model._band_ws is not None                                      # allocated on the calibration forward, kept
    scratch = model._band_ws
    del log[:]
    for _ in range(2):
        assert torch.equal(run(Wan, model, inputs), dense)
    assert names(log) == ["flash_attn_d128"] * 2 * layers and model._band_ws is scratch    # only the dense entry afterwards
    model.attn_band = BAND + 1                                             # the key carries the band: the decisions are dropped
    assert torch.equal(run(Wan, model, inputs), dense) and not model.attn_window_calibrated


def test_tiny_threshold_gives_every_head_the_cheaper_candidate(monkeypatch):
    model, inputs, layers, N, Sq = Wan.build()
    dense = run(Wan, model, inputs)
    model.attn_window, model.attn_window_recall, model.attn_band = 1, 1e-9, BAND
    assert torch.equal(run(Wan, model, inputs, calibrate=True), dense)
    cost_w, cost_b = mean_unit_cost(frame_window_ranges(F, HW, 1)), mean_unit_cost(position_band_ranges(F, HW, BAND))
    assert cost_b < cost_w                                                 # 7.25 against 14.25 key tiles per unit: the band
    assert all(s["layout"] == ["band"] * HEADS and s["windowed"] == [False] * HEADS for s in model.attn_window_stats)
    log = launches(monkeypatch)
    out = run(Wan, model, inputs)
    per_layer = ["attn_rows_position_major", "attn_rows_position_major", "attn_vt_position_major", "flash_attn_d128_ranges",
                 "attn_rows_position_major"]
    assert names(log) == per_layer * layers                                # no main launch where every head chose the band
    assert bool(torch.isfinite(out.float()).all()) and not torch.equal(out, dense)
    assert torch.equal(run(Wan, model, inputs), out)


def _patch_reference(monkeypatch):
    """Self-attention by per-head masked fp32 SDPA: the main launch's per-head table as it is (absent heads: zeros, which the
    band heads' rows then replace), the band launch under M[s_q][s_k] = band_mask[pi(s_q)][pi(s_k)] computed on the FRAME-MAJOR
    operands the gathers were handed, written where the scatter would write.  The layout kernels do not run."""
    state = {}
    pi = position_major_index(F, HW)

    def heads_fake(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale, kv_ranges, lse=None, **kw):
        assert isinstance(kv_ranges, KvRangesHeads) and lse is None
        mask = ranges_to_mask(kv_ranges)
        M._sdpa_into_o(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale,
                       mask=mask | ~mask.any(dim=-1, keepdim=True), **kw)      # (an absent head: any finite rows, overwritten below)
        state["main"] = kv_ranges
        return o

    def gather_fake(src, dst, hl, hd, batch, frames, hw, src_bs, src_rs, dst_bs, dst_rs, inverse=False, src_off=0, dst_off=0):
        if not inverse:
            state.setdefault("qk", []).append((src, src_off, src_bs, src_rs))
            state["hl"] = hl
            return dst
        q, k = state.pop("qk")
        vt = state.pop("vt")
        table = state.pop("table")
        mask = ranges_to_mask(table)[pi][:, pi]
        D = dst_rs
        full = torch.empty(batch, frames * hw, D, dtype=BF, device=dst.device)
        M._sdpa_into_o(q[0], k[0], vt[0], full, batch, D // 128, S, S, q[2], q[3], k[2], k[3], vt[2], vt[3], S * D, D, state["scale"],
                       mask=mask, q_off=q[1], k_off=k[1])
        o = torch.as_strided(dst.view(-1), (batch, S, D // 128, 128), (dst_bs, dst_rs, 128, 1), dst_off)
        for h in hl.indices:
            o[:, :, h] = full.view(batch, S, D // 128, 128)[:, :, h]
        return dst

    def vt_fake(src, dst, hl, hd, batch, frames, hw, src_bs, src_rs, dst_bs, dst_rs, **kw):
        state["vt"] = (src, 0, src_bs, src_rs)
        return dst

    def band_fake(q, k, vt, o, batch, heads, Sq, Skv, q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs, scale, kv_ranges, **kw):
        assert isinstance(kv_ranges, KvRanges) and heads == state["hl"].n_sel
        state["table"], state["scale"] = kv_ranges, scale
        state.setdefault("band_launches", []).append(heads)
        return o

    monkeypatch.setattr(_lib, "flash_attn_d128_ranges_heads", heads_fake)
    monkeypatch.setattr(_lib, "attn_rows_position_major", gather_fake)
    monkeypatch.setattr(_lib, "attn_vt_position_major", vt_fake)
    monkeypatch.setattr(_lib, "flash_attn_d128_ranges", band_fake)
    return state


def _forced_mix(monkeypatch, balance=False):
    model, inputs, layers, N, Sq = Wan.build()
    inputs = tuple(t.to(DEV) for t in inputs)
    dense_hip = run(Wan, model, inputs)
    model.attn_window, model.attn_window_recall, model.attn_band, model.attn_window_balance = 1, 0.5, BAND, balance
    with monkeypatch.context() as m:
        m.setattr(attn_window, "decide_layouts", lambda rw, rb, cw, cb, thr: list(MIX))
        assert torch.equal(run(Wan, model, inputs, calibrate=True), dense_hip)
    assert all(s["layout"] == MIX and s["windowed"] == [False, True, False, False] for s in model.attn_window_stats)
    return model, inputs, layers, dense_hip


def test_forced_mix_is_exact_to_the_dense_standard(monkeypatch):
    model, inputs, layers, dense_hip = _forced_mix(monkeypatch)
    log = launches(monkeypatch)
    mixed_hip = run(Wan, model, inputs)
    per_layer = ["flash_attn_d128_ranges_heads", "attn_rows_position_major", "attn_rows_position_major", "attn_vt_position_major",
                 "flash_attn_d128_ranges", "attn_rows_position_major"]
    assert names(log) == per_layer * layers
    assert bool(torch.isfinite(mixed_hip.float()).all()) and not torch.equal(mixed_hip, dense_hip)
    with monkeypatch.context() as m:
        state = _patch_reference(m)
        mixed_ref = run(Wan, model, inputs)
    assert state["band_launches"] == [2] * layers and [r.absent for r in state["main"].per_head] == [True, False, False, True]
    model.attn_window = 0
    with monkeypatch.context() as m:
        M._patch_dense(m, S)
        dense_ref = run(Wan, model, inputs)
    e_mixed, e_dense = rel(mixed_hip, mixed_ref), rel(dense_hip, dense_ref)
    M._report("wan_attn_band_forced_mix_w1_b2", e_mixed, e_dense)
    assert e_dense > 0
    assert e_mixed <= FACTOR * e_dense, (e_mixed, e_dense)


def test_forced_mix_keeps_its_bits_under_every_launch_order_and_replays_from_a_graph(monkeypatch):
    model, inputs, layers, dense_hip = _forced_mix(monkeypatch)
    want = run(Wan, model, inputs)
    for policy in ("units", "lanes"):
        model.attn_window_balance = policy
        with monkeypatch.context() as m:
            log = launches(m)
            assert torch.equal(run(Wan, model, inputs), want), policy
        assert names(log).count("flash_attn_d128_ranges_order") == layers and "flash_attn_d128_ranges_heads" not in names(log)
    model.attn_window_balance = False
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(Wan, model, inputs)                                            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    a, kw = Wan.args(inputs)
    with torch.cuda.graph(graph, stream=side):
        got = model(*a, **kw)[0]
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_refusals_and_a_graph_capture_of_the_calibration_forward():
    cfg, sd, inputs = M._wan_setup()
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    model.attn_window, model.attn_window_recall, model.attn_band = 2, 0.5, BAND
    model.attn_window_widths = (1, 2)
    with pytest.raises(ValueError, match="attn_window_widths"):
        run(Wan, model, inputs, calibrate=True)
    model.attn_window_widths = None
    model.attn_window_recall = 0.0
    with pytest.raises(ValueError, match="attn_band"):
        run(Wan, model, inputs)
    model.attn_window_recall, model.attn_band = 0.5, -1
    with pytest.raises(ValueError, match="attn_band"):
        run(Wan, model, inputs)
    f8 = WanTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    f8.attn_window, f8.attn_window_recall, f8.attn_band = 1, 0.5, BAND
    with pytest.raises(ValueError, match="fp8_attention"):
        run(Wan, f8, inputs, calibrate=True)
    model.attn_band = BAND
    pipe, kw = HM._sampler(model)
    with pytest.raises(_lib.AlgHipError, match="cfg_split"):
        pipe(cfg_split=object(), **kw)
    model.reset_attn_window_heads()
    inputs = tuple(t.to(DEV) for t in inputs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = run(Wan, model, inputs)                                     # warm-up on the capture stream (dense)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.AlgHipError, match="captured"):
        with torch.cuda.graph(graph, stream=side):
            run(Wan, model, inputs, calibrate=True)
    torch.cuda.synchronize()
    assert not model.attn_window_calibrated and model.attn_window_stats == [] and model._band_ws is None
    assert torch.equal(run(Wan, model, inputs), want)


def test_wan_sampler_calibrates_the_band_on_its_last_dense_step(monkeypatch):
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    cfg, sd, _ = M._wan_setup(layers=2)
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    pipe, kw = HM._sampler(model)                                          # 4 steps, attn_window_dense_steps = 2
    assert isinstance(pipe, WanImageToVideoPipeline)
    model.attn_window, model.attn_window_recall, model.attn_band = 1, 0.5, BAND
    monkeypatch.setattr(attn_window, "decide_layouts", lambda rw, rb, cw, cb, thr: list(MIX))
    log = launches(monkeypatch)
    resets = []
    real_reset = model.reset_attn_window_heads
    monkeypatch.setattr(model, "reset_attn_window_heads", lambda: (resets.append(1), real_reset())[1])
    seen, calibrated = [], []

    def at_step_end(p, i, t, k):
        seen.append((sum(l for n, l in log), names(log).count("flash_attn_d128_ranges")))
        calibrated.append(p.transformer.attn_window_calibrated)

    out = pipe(callback_on_step_end=at_step_end, **kw)
    L = cfg.num_layers
    assert attn_window.calibration_step(kw["attn_window_dense_steps"]) == 1
    # step 0: dense; step 1: the calibration (three launches with lse per layer); steps 2, 3: one band launch per layer each
    assert seen == [(0, 0), (3 * L, 0), (3 * L, L), (3 * L, 2 * L)] and calibrated == [False, True, True, True]
    assert bool(torch.isfinite(out.frames.float()).all())
    stats = model.attn_window_stats
    assert len(stats) == L and resets == [1] and all(s["layout"] == MIX for s in stats)
    pipe(callback_on_step_end=at_step_end, **kw)                           # the next video starts from no decision
    assert resets == [1, 1] and model.attn_window_stats is not stats and calibrated[4:] == [False, True, True, True]
