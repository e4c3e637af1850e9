"""`transformer.attn_window_widths` of the Wan and HunyuanVideo DiTs (attn_window.HeadWindowHost): the width of every head from ONE
calibration launch per layer.  The trained-like models of test_gpu_attn_window_heads_models.py at 9 latent frames (Wan: 128 tokens
per frame, hw % 64 == 0; HunyuanVideo: 104 and a prompt tail), the 4-step samplers of test_gpu_attn_window_balance_models.py."""
import math

import pytest
import torch

import test_gpu_attn_window_balance_models as BM
import test_gpu_attn_window_heads_models as HM
import test_gpu_attn_window_models as M
from alg_amd import _lib, attn_window
from alg_amd.attn_window import KvRangesHeads, KvSegments, frame_window_ranges, full_ranges, head_width_ranges

pytestmark = pytest.mark.gpu
DEV, BF, HEADS = M.DEV, M.BF, M.HEADS
FRAMES, WIDTHS = 9, (1, 2, 4)
WAN_HW = 128          # 8 x 16 patches: a frame is two key tiles, the profile's cuts are the window's


@pytest.fixture(autouse=True)
def _nine_frames_and_q64(monkeypatch):
    """9 latent frames for every set-up of the imported modules; ALG_ATTN128_Q64=2 as in those modules."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")
    monkeypatch.setattr(M, "WAN_F", FRAMES)
    monkeypatch.setattr(M, "HY_F", FRAMES)


class Wan(HM.Wan):
    hw = WAN_HW

    @staticmethod
    def build():
        cfg, sd, (x, t, txt, img) = M._wan_setup()
        g = torch.Generator().manual_seed(5)
        x = torch.randn(x.shape[0], 36, FRAMES, 16, 32, generator=g).to(BF)
        return HM.WanTransformer3DModel(cfg, sd, device=DEV), (x, t, txt, img), cfg.num_layers, 2, FRAMES * WAN_HW

    @staticmethod
    def window(w, Sq, Skv, sink=1):
        return frame_window_ranges(FRAMES, WAN_HW, w, sink_frames=sink)


class Hy(HM.Hy):
    hw = M.HY_HW

    @staticmethod
    def window(w, Sq, Skv, sink=1):
        S = FRAMES * M.HY_HW
        return frame_window_ranges(FRAMES, M.HY_HW, w, sink_frames=sink, tail=(S, Skv), rows=Sq)


FAMILIES = [Wan, Hy]
run = HM.run


def spy(monkeypatch, name, after=None):
    real, calls = getattr(_lib, name), []

    def spied(*a, **kw):
        calls.append((a, kw))
        out = real(*a, **kw)
        if after is not None:
            after(a, kw)
        return out

    monkeypatch.setattr(_lib, name, spied)
    return calls


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_widths_unset_is_the_recall_policy_bit_for_bit(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    assert model.attn_window_widths is None
    model.attn_window, model.attn_window_recall = 4, 0.5
    prefix_calls = spy(monkeypatch, "flash_attn_d128_ranges_prefix")
    cal, later, stats = run(fam, model, inputs, calibrate=True), run(fam, model, inputs), model.attn_window_stats
    assert all(sorted(s) == ["layer", "recall", "windowed"] for s in stats)
    model.attn_window_widths = WIDTHS                       # touched ...
    model.attn_window_widths = None                         # ... and off again
    model.reset_attn_window_heads()
    assert torch.equal(run(fam, model, inputs, calibrate=True), cal) and torch.equal(run(fam, model, inputs), later)
    assert model.attn_window_stats == stats and not prefix_calls and hasattr(model._attn_cal, "lse_part")


def _two_launch(fam, log):
    """Behind every prefix launch of a calibration forward: the parent's calibration pair and the dense entry on the SAME
    operands -- the two-launch recall [batch * heads], the largest |lse_full|, and the attention outputs' distance."""
    def after(a, kw):
        q, k, vt, o, batch, heads, Sq, Skv = a[:8]
        strides, scale, seg, prefix = a[8:16], a[16], a[17], a[18]
        assert isinstance(seg, KvSegments) and seg.segments == 2 * len(WIDTHS) + 3
        D = heads * 128
        off = {n: kw.get(n, 0) for n in ("q_off", "k_off", "vt_off")}
        A = (batch, heads, Sq, Skv) + tuple(strides[:6]) + (Sq * D, D, scale)
        scratch = torch.empty(batch, Sq, D, dtype=BF, device=DEV)
        full, part = (torch.empty(batch, heads, Sq, device=DEV) for _ in range(2))
        _lib.flash_attn_d128_ranges_heads(q, k, vt, scratch, *A, full_ranges(Sq, Skv), lse=full, **off)
        got = o.as_strided((batch, Sq, D), (strides[6], strides[7], 1), o.storage_offset() + kw.get("o_off", 0))
        err = (got.float() - scratch.float()).abs()
        _lib.flash_attn_d128_ranges_heads(q, k, vt, scratch, *A, fam.window(WIDTHS[-1], Sq, Skv), lse=part, **off)
        rec = torch.empty(batch * heads, dtype=torch.float64, device=DEV)
        _lib.attn_lse_recall(part, full, rec, batch * heads, Sq, row0=0, rows=FRAMES * fam.hw)
        log.append((rec.view(batch, heads).cpu(), full.abs().max().item(), err.max().item(), err.mean().item()))
    return after


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_one_pass_calibration_measures_every_width(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    dense = run(fam, model, inputs)
    model.attn_window, model.attn_window_recall, model.attn_window_widths = WIDTHS[-1], 0.5, WIDTHS
    with pytest.raises(_lib.AlgHipError, match="captured"):             # a capture of the calibration forward still raises
        with monkeypatch.context() as m:
            m.setattr(_lib, "_capturing", lambda: True)
            run(fam, model, inputs, calibrate=True)
    log = []
    with monkeypatch.context() as m:
        prefix_calls = spy(m, "flash_attn_d128_ranges_prefix", after=_two_launch(fam, log))
        mass_calls = spy(m, "attn_prefix_mass")
        recall_calls = spy(m, "attn_lse_recall")
        out = run(fam, model, inputs, calibrate=True)
    per_layer = N if fam is Hy else 1
    # ONE prefix launch and one reduction per layer (per sample in HunyuanVideo); no scratch output, no lse_part
    assert len(prefix_calls) == len(mass_calls) == layers * per_layer and len(recall_calls) == len(prefix_calls)    # (the spy's own)
    cal = model._attn_cal
    assert not hasattr(cal, "o") and not hasattr(cal, "lse_part") and not hasattr(cal, "lse_full")
    assert bool(torch.isfinite(out.float()).all())
    print(fam.name, "calibration forward vs dense forward: max |diff| %.3e" % (out.float() - dense.float()).abs().max().item())
    stats = model.attn_window_stats
    assert [s["layer"] for s in stats] == list(range(layers)) and model.attn_window_calibrated
    for li, s in enumerate(stats):
        by = s["recall_by_width"]
        assert len(by) == N and all(len(smp) == HEADS and all(len(h) == len(WIDTHS) for h in smp) for smp in by)
        print(fam.name, "layer", li, "recall by width", [[[round(x, 4) for x in h] for h in smp] for smp in by], "width", s["width"])
        for n in range(N):
            for h in range(HEADS):
                r = by[n][h]
                assert all(0.0 <= x <= 1.0 for x in r) and all(a <= b for a, b in zip(r, r[1:])), (li, n, h, r)   # sums of more masses >= 0
                assert s["recall"][n][h] == r[-1]
        for h in range(HEADS):
            ok = [w for j, w in enumerate(WIDTHS) if min(by[n][h][j] for n in range(N)) >= 0.5]
            assert s["width"][h] == (ok[0] if ok else 0)
        assert s["windowed"] == [w > 0 for w in s["width"]]
        # the parent's two-launch recall of the SAME forward.  fp32 LSE slack: each route takes 2^(difference of two fp32
        # log-sum-exps), each rounded and with a 1-ulp log: 3 spacings at the largest |lse| per route, times ln 2 on a recall <= 1
        for n in range(N):
            two, lse_max, e_max, e_mean = log[li * per_layer + n] if fam is Hy else log[li]
            two = two[0] if fam is Hy else two[n]
            slack = 2 * 3 * 2.0 ** (math.floor(math.log2(lse_max)) - 23) * math.log(2.0)
            for h in range(HEADS):
                one = s["recall"][n][h]
                assert one <= min(two[h].item(), 1.0) + slack, (li, n, h, one, two[h].item(), slack)
                if fam.hw % 64 == 0:
                    assert abs(one - min(two[h].item(), 1.0)) <= slack, (li, n, h, one, two[h].item(), slack)
    # the calibration launch IS the dense attention: within the multi-range bound of test_gpu_attn_ranges.py of the dense entry
    for two, lse_max, e_max, e_mean in log:
        assert e_max < 3e-2 and e_mean < 2e-3, (e_max, e_mean)
    print(fam.name, "prefix launch vs dense entry, attention output: max %.3e mean %.3e"
          % (max(x[2] for x in log), max(x[3] for x in log)))


def _mixing_threshold(stats):
    """A threshold between two measured recalls (the widest gap first) at which the heads of some layer choose different widths."""
    r = sorted(set(min(smp[h][j] for smp in s["recall_by_width"]) for s in stats for h in range(HEADS) for j in range(len(WIDTHS))))
    for gap, thr in sorted(((b - a, 0.5 * (a + b)) for a, b in zip(r, r[1:])), reverse=True):
        if any(len(set(attn_window.decide_widths(s["recall_by_width"], WIDTHS, thr))) > 1 for s in stats):
            return thr
    return None


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_later_forwards_launch_every_layers_own_table(fam, monkeypatch):
    model, inputs, layers, N, Sq = fam.build()
    model.attn_window, model.attn_window_recall, model.attn_window_widths = WIDTHS[-1], 0.5, "1,2,4"      # the string form
    run(fam, model, inputs, calibrate=True)
    thr = _mixing_threshold(model.attn_window_stats)
    assert thr is not None
    model.attn_window_recall = thr                           # another threshold: the decisions are dropped
    assert run(fam, model, inputs) is not None and not model.attn_window_calibrated
    run(fam, model, inputs, calibrate=True)
    widths = [s["width"] for s in model.attn_window_stats]
    print(fam.name, "threshold %.4f" % thr, "widths", widths)
    assert len(set(w for ws in widths for w in ws)) >= 2     # the precondition: the heads did not all choose alike
    dense_calls = spy(monkeypatch, "flash_attn_d128")
    shared_calls, heads_calls = spy(monkeypatch, "flash_attn_d128_ranges"), spy(monkeypatch, "flash_attn_d128_ranges_heads")
    prefix_calls = spy(monkeypatch, "flash_attn_d128_ranges_prefix")
    first = run(fam, model, inputs)
    per_layer = N if fam is Hy else 1
    samples = list(M.HY_VALID) if fam is Hy else [None]
    want_shared, want_heads, want_dense = [], [], 0
    for ws in widths:
        for v in samples:
            Skv = Sq if fam is Wan else FRAMES * M.HY_HW + v
            t = head_width_ranges({w: fam.window(w, Sq, Skv) for w in WIDTHS}, ws)
            if isinstance(t, KvRangesHeads):
                want_heads.append(t.table)
            elif t is not None:
                want_shared.append(t.table)
            else:
                want_dense += 1
    assert not prefix_calls
    assert [a[17].table.tolist() for a, kw in heads_calls] == [t.tolist() for t in want_heads]
    assert [a[17].table.tolist() for a, kw in shared_calls] == [t.tolist() for t in want_shared]
    assert all(kw.get("lse") is None for a, kw in heads_calls)
    self_dense = [a for a, kw in dense_calls if a[6] == a[7] == Sq] if fam is Wan else [a for a, kw in dense_calls if a[6] == Sq]
    assert len(self_dense) == want_dense
    assert torch.equal(run(fam, model, inputs), first) and bool(torch.isfinite(first.float()).all())


@pytest.mark.parametrize("family", [BM._wan, BM._hunyuan], ids=lambda f: f.__name__[1:])
def test_balanced_launch_order_keeps_the_samplers_bits_with_widths(family, monkeypatch):
    model, pipe, kw, entry, table_arg = family()
    final = lambda: pipe(**kw).frames.clone()
    model.attn_window, model.attn_window_recall, model.attn_window_widths = WIDTHS[-1], 0.5, WIDTHS
    final()
    thr = _mixing_threshold(model.attn_window_stats)
    assert thr is not None
    model.attn_window_recall = thr
    order_calls, lse_calls = spy(monkeypatch, "flash_attn_d128_ranges_order"), spy(monkeypatch, "attn_lse_recall")
    want = final()
    mixed = [s["layer"] for s in model.attn_window_stats if len(set(s["width"])) > 1]
    print(family.__name__, "threshold %.4f" % thr, "widths", [s["width"] for s in model.attn_window_stats])
    assert mixed and not order_calls and bool(torch.isfinite(want.float()).all())
    model.attn_window_balance = True
    assert torch.equal(final(), want)
    assert order_calls and not lse_calls and all(isinstance(a[17], KvRangesHeads) for a, _ in order_calls)
    if family is BM._wan:
        with pytest.raises(_lib.AlgHipError, match="cfg_split"):
            pipe(cfg_split=object(), **kw)


def test_a_forward_behind_the_calibration_is_captured_and_replays():
    model, inputs, layers, N, Sq = Wan.build()
    inputs = tuple(t.to(DEV) for t in inputs)               # on the device before any capture
    model.attn_window, model.attn_window_recall, model.attn_window_widths = WIDTHS[-1], 0.5, WIDTHS
    run(Wan, model, inputs, calibrate=True)
    model.attn_window_recall = _mixing_threshold(model.attn_window_stats)
    model.reset_attn_window_heads()
    run(Wan, model, inputs, calibrate=True)
    assert model.attn_window_calibrated and any(len(set(s["width"])) > 1 for s in model.attn_window_stats)
    want = run(Wan, model, inputs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(Wan, model, inputs)                             # warm-up on the capture stream
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


def test_the_switch_is_validated_before_any_launch():
    model, inputs, layers, N, Sq = Wan.build()
    model.attn_window, model.attn_window_recall = 4, 0.5
    for bad, msg in (((1, 2), "must equal attn_window"), ((2, 1, 4), "strictly ascending"), ((0, 4), "strictly ascending"),
                     ((1, 2, 3, 4, 5), "at most 4 widths"), ("1,x", "comma-separated"), (4, "sequence of ints")):
        model.attn_window_widths = bad
        with pytest.raises(ValueError, match=msg):
            run(Wan, model, inputs, calibrate=True)
    model.attn_window_widths, model.attn_window_recall = WIDTHS, 0.0
    with pytest.raises(ValueError, match="needs attn_window_recall > 0"):
        run(Wan, model, inputs)
    assert not model.attn_window_calibrated and model._attn_cal is None
    cfg, sd, _ = M._wan_setup()
    model = HM.WanTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    model.attn_window, model.attn_window_recall, model.attn_window_widths = 4, 0.5, WIDTHS
    with pytest.raises(ValueError, match="fp8_attention"):
        run(Wan, model, inputs, calibrate=True)
