"""The host side of the per-head window width from one calibration pass (alg_amd/attn_window.py: KvSegments,
frame_profile_segments, width_segments, decide_widths, head_width_ranges, HeadWindowHost.attn_window_widths), the prototypes of the
two entries under it, and the refusals of the switch.  No GPU."""
import argparse
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import alg_amd._lib
from alg_amd.attn_window import (HeadWindowHost, KvRangesHeads, KvSegments, decide_widths, frame_profile_segments,
                                 frame_window_ranges, full_ranges, head_width_ranges, ranges_to_mask, width_segments)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 4)
SHAPES = [(9, 100), (13, 135), (9, 384), (5, 70), (21, 96)]      # (frames, tokens per frame)


def seg_table(rows):
    return torch.tensor(rows, dtype=torch.int32)


def test_kv_segments_takes_partitions_with_empty_entries_anywhere():
    t = seg_table([[[0, 0], [0, 128], [5, 5], [128, 300], [0, 0]], [[0, 300], [0, 0], [0, 0], [0, 0], [0, 0]]])
    s = KvSegments(t, 300, 512)
    assert (s.q_blocks, s.segments, s.max_ranges, s.Skv, s.Sq, s.coverage) == (2, 5, 5, 300, 512, 1.0)
    assert torch.equal(s.table, t) and s.table is not t
    assert KvSegments(torch.zeros(1, 12, 2, dtype=torch.int32).index_put_((torch.tensor([0]), torch.tensor([11]), torch.tensor([1])),
                                                                            torch.tensor([64], dtype=torch.int32)), 64, 1).segments == 12


@pytest.mark.parametrize("rows,msg", [
    ([[[0, 128], [192, 300]]], r"block 0: the keys \[128, 192\) in front of entry 1 are in no segment"),      # a gap
    ([[[0, 128], [128, 256]]], r"block 0: the keys \[256, 300\) are in no segment"),                           # short of Skv
    ([[[0, 192], [128, 300]]], "block 0: entry 1 .* overlaps"),
    ([[[0, 128], [128, 300], [64, 128]]], "block 0: entry 2 .* not sorted"),
    ([[[128, 300], [0, 128]]], r"block 0: the keys \[0, 128\) in front of entry 0"),                           # descending
    ([[[0, 100], [100, 300]]], "block 0: begin 100 of entry 1 is not a multiple of 64"),
    ([[[0, 301]]], "block 0: end 301 of entry 0 is beyond Skv = 300"),
    ([[[0, 300]], [[0, 300]]], "2 blocks"),
    ([[[0, 0]]], r"block 0: the keys \[0, 300\) are in no segment"),
])
def test_kv_segments_names_the_block_and_the_rule(rows, msg):
    with pytest.raises(ValueError, match=msg):
        KvSegments(seg_table(rows), 300, 256)


def test_kv_segments_refuses_other_shapes_and_types():
    with pytest.raises(ValueError, match=r"segments must be 1\.\.12, got 13"):
        KvSegments(torch.zeros(1, 13, 2, dtype=torch.int32), 64, 1)
    with pytest.raises(ValueError, match="CPU int32 table"):
        KvSegments(torch.zeros(1, 3, 2, dtype=torch.int64), 64, 1)
    with pytest.raises(ValueError, match="CPU int32 table"):
        KvSegments(torch.zeros(3, 2, dtype=torch.int32), 64, 1)


def counted_mask(seg, idx):
    m = torch.zeros(seg.Sq, seg.Skv, dtype=torch.bool)
    for qb in range(seg.q_blocks):
        for i in idx:
            b, e = seg.table[qb, i].tolist()
            if e > b:
                m[qb * 256:(qb + 1) * 256, b:e] = True
    return m


@pytest.mark.parametrize("sink", [0, 1])
@pytest.mark.parametrize("tail", [None, 77])
@pytest.mark.parametrize("F,hw", SHAPES)
def test_profile_segments_partition_the_keys_and_count_a_subset_of_the_window(F, hw, tail, sink):
    S = F * hw
    kw = dict(sink_frames=sink, tail=None if tail is None else (S, S + tail), rows=None if tail is None else S + 200)
    seg = frame_profile_segments(F, hw, WIDTHS, **kw)            # KvSegments has checked that every block is a partition
    assert isinstance(seg, KvSegments) and seg.segments == 2 * len(WIDTHS) + 3 and seg.Skv == S + (tail or 0)
    assert bool(counted_mask(seg, range(seg.segments)).all())
    a = seg.table.numpy()
    assert ((a[..., 0] % 64 == 0) | (a[..., 1] <= a[..., 0])).all()
    for j, idx in enumerate(width_segments(len(WIDTHS))):
        win = frame_window_ranges(F, hw, WIDTHS[j], **kw)
        want = ranges_to_mask(win) if win is not None else torch.ones(seg.Sq, seg.Skv, dtype=torch.bool)
        got = counted_mask(seg, idx)
        assert not bool((got & ~want).any()), (F, hw, WIDTHS[j])                  # a subset: the measured recall is a lower bound
        short = int((want & ~got).sum(dim=1).max())
        assert short <= 126, short
        if hw % 64 == 0 and tail is None:
            assert short == 0                                                      # the cuts are the window's
    if tail is not None:                                                           # prompt-query blocks: everything in the core
        k = len(WIDTHS)
        last = seg.table[-1]
        assert last[k + 1].tolist() == [0, seg.Skv] and int(last.sum()) == seg.Skv


def test_profile_segments_mean_the_same_in_every_block():
    k = len(WIDTHS)
    assert width_segments(k) == [[0, 4, 8], [0, 3, 4, 5, 8], [0, 2, 3, 4, 5, 6, 8]]
    assert width_segments(1) == [[0, 2, 4]]
    seg = frame_profile_segments(9, 128, WIDTHS)                 # 128 tokens per frame: block j holds the frames 2 j and 2 j + 1
    b = seg.table[2].tolist()                                    # frames 4 and 5
    hw = 128
    assert b == [[0, hw], [0, 0], [hw, 2 * hw], [2 * hw, 3 * hw], [3 * hw, 7 * hw], [7 * hw, 8 * hw], [8 * hw, 9 * hw], [0, 0], [0, 0]]
    with pytest.raises(ValueError, match="strictly ascending"):
        frame_profile_segments(9, 128, (2, 2))
    with pytest.raises(ValueError, match="at most 4 widths"):
        frame_profile_segments(9, 128, (1, 2, 3, 4, 5))
    assert frame_profile_segments(9, 128, "1,2").segments == 7


def test_decide_widths_takes_the_narrowest_width_that_holds_on_every_sample():
    rec = [[[0.95, 0.97, 0.99], [0.5, 0.92, 0.99], [0.1, 0.2, 0.95], [0.1, 0.2, 0.3]],
           [[0.91, 0.97, 0.99], [0.95, 0.89, 0.99], [0.1, 0.95, 0.95], [0.9, 0.9, 0.9]]]
    assert decide_widths(rec, WIDTHS, 0.9) == [1, 4, 4, 0]       # the minimum over the samples decides, per width
    assert decide_widths(rec, WIDTHS, 0.0) == [1, 1, 1, 1] and decide_widths(rec, WIDTHS, 1.5) == [0, 0, 0, 0]
    assert decide_widths(rec, WIDTHS, 0.99) == [4, 4, 0, 0]      # equality reaches the threshold
    # monotone: a higher threshold never narrows a head (0 = dense counts as the widest)
    wide = lambda w: math.inf if w == 0 else w
    prev = [1] * 4
    for thr in np.linspace(0.0, 1.0, 41):
        cur = decide_widths(rec, WIDTHS, float(thr))
        assert all(wide(c) >= wide(p) for c, p in zip(cur, prev)), thr
        prev = cur
    nan = float("nan")
    assert decide_widths([[[nan, 0.95, 0.99], [0.95, nan, 0.99], [0.95, 0.96, 0.99]]], WIDTHS, 0.9) == [0, 0, 1]
    for bad in ([], [[]], [[[0.9, 0.9]]], [[[0.9] * 3], [[0.9] * 3, [0.9] * 3]]):
        with pytest.raises(ValueError, match="decide_widths takes"):
            decide_widths(bad, WIDTHS, 0.9)


def test_head_width_ranges_has_three_result_types():
    F, hw = 9, 100
    S = F * hw
    bases = {w: frame_window_ranges(F, hw, w) for w in WIDTHS}
    assert head_width_ranges(bases, [2, 2, 2]) is bases[2]                         # every head alike: the shared table
    assert head_width_ranges(bases, [0, 0]) is None                                # every head dense: the dense launch
    t = head_width_ranges(bases, [1, 0, 4, 2])
    assert isinstance(t, KvRangesHeads) and t.heads == 4 and (t.Sq, t.Skv) == (S, S)
    n = max(b.max_ranges for b in bases.values())
    assert t.max_ranges == n
    masks = ranges_to_mask(t)
    for h, w in enumerate([1, 0, 4, 2]):
        want = ranges_to_mask(bases[w]) if w else torch.ones(S, S, dtype=torch.bool)
        assert torch.equal(masks[h], want), h
        if w:
            assert torch.equal(t.table[h, :, :bases[w].max_ranges], bases[w].table)          # the base's rows, zero-padded
            assert not bool(t.table[h, :, bases[w].max_ranges:].any())
        else:
            assert torch.equal(t.table[h, :, 0], full_ranges(S, S).table[:, 0]) and not bool(t.table[h, :, 1:].any())
    # a width whose window is the dense attention (None) counts as the full range
    assert head_width_ranges({1: bases[1], 8: None}, [8, 8]) is None
    assert torch.equal(ranges_to_mask(head_width_ranges({1: bases[1], 8: None}, [1, 8]))[1], torch.ones(S, S, dtype=torch.bool))
    with pytest.raises(ValueError, match="no table for the chosen width 3"):
        head_width_ranges(bases, [1, 3])
    with pytest.raises(ValueError, match="no head"):
        head_width_ranges(bases, [])


def test_prefixes_to_masses_to_recalls_is_the_direct_mass():
    """A numpy emulation of the chain: float64 scores -> prefix log-sum-exps per segment (what the kernel writes, here in float64)
    -> masses (the definition of alg_attn_prefix_mass) -> recalls (width_segments), against the softmax mass summed directly over
    the counted keys."""
    F, hw, H = 5, 70, 2
    S = F * hw
    rng = np.random.default_rng(3)
    seg = frame_profile_segments(F, hw, WIDTHS)
    n = seg.segments
    s = rng.normal(size=(H, S, S)) * 3.0
    p = np.exp2(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    prefix = np.full((H, n, S), -np.inf)
    for qb in range(seg.q_blocks):
        rows = slice(qb * 256, min((qb + 1) * 256, S))
        acc = np.zeros((H, rows.stop - rows.start))
        for i in range(n):
            b, e = seg.table[qb, i].tolist()
            if e > b:
                acc = acc + np.exp2(s[:, rows, b:e]).sum(axis=-1)
            with np.errstate(divide="ignore"):
                prefix[:, i, rows] = np.log2(acc)
    with np.errstate(invalid="ignore"):
        cum = np.where(np.isneginf(prefix), 0.0, np.exp2(prefix - prefix[:, -1:]))
    mass = np.diff(cum, axis=1, prepend=0.0).mean(axis=-1)                         # [H, n]
    assert np.allclose(mass.sum(axis=1), 1.0, atol=1e-12)
    for j, idx in enumerate(width_segments(len(WIDTHS))):
        got = mass[:, idx].sum(axis=1)
        want = (p * counted_mask(seg, idx).numpy()[None]).sum(axis=-1).mean(axis=-1)
        assert np.allclose(got, want, atol=1e-12), (j, got, want)


def _prototype(name, text):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_exports_and_wrapper_agree_on_the_two_new_entries():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "attention128_q64.hip")).read()
    for name, n_args, wrapper in (("alg_flash_attn_d128_ranges_prefix", 22, "flash_attn_d128_ranges_prefix"),
                                  ("alg_attn_prefix_mass", 8, "attn_prefix_mass")):
        assert name in alg_amd._lib.EXPORTS and callable(getattr(alg_amd._lib, wrapper))
        declared, defined = _prototype(name, header), _prototype(name, src[src.index('extern "C" int ' + name + "("):])
        assert len(declared) == n_args
        strip = lambda a: a.rsplit(" ", 1)[0]                   # the type of an argument
        assert [strip(a) for a in declared] == [strip(a) for a in defined], name
    heads = _prototype("alg_flash_attn_d128_ranges_heads", header)
    prefix = _prototype("alg_flash_attn_d128_ranges_prefix", header)
    assert [a.rsplit(" ", 1)[0] for a in prefix] == [a.rsplit(" ", 1)[0] for a in heads]      # lse -> lse_prefix, nothing else
    assert prefix[-2] == "float* lse_prefix" and prefix[-4] == "int max_segments"


def test_the_wrapper_takes_only_validated_tables_of_the_calls_shape():
    L = alg_amd._lib
    args = (None, None, None, None, 1, 2, 300, 512, 0, 0, 0, 0, 0, 0, 0, 0, 1.0)
    seg = KvSegments(seg_table([[[0, 512]], [[0, 512]]]), 512, 300)
    with pytest.raises(L.AlgHipError, match="KvSegments"):
        L.flash_attn_d128_ranges_prefix(*args, seg.table, None)
    with pytest.raises(L.AlgHipError, match="Sq=256"):
        L.flash_attn_d128_ranges_prefix(*args, KvSegments(seg_table([[[0, 512]]]), 512, 256), None)
    with pytest.raises(L.AlgHipError, match="3 heads"):
        L.flash_attn_d128_ranges_prefix(*args, KvRangesHeads(torch.stack([full_ranges(300, 512).table] * 3), 512, 300), None)


class Host(HeadWindowHost):
    device = "cpu"

    def __init__(self):
        self.attn_window = 4
        self._head_window_init()


def test_the_attribute_is_validated():
    host = Host()
    mode = lambda: host._head_window_mode(("k",), 2, 1, 4, 256, (1, 256, 512))
    assert host.attn_window_widths is None
    host.attn_window_recall = 0.9
    assert mode() == "dense" and host._head_window_widths() is None
    for good in ((1, 2, 4), [4], "1,2,4", "4", (1, 2, 3, 4)):
        host.attn_window_widths = good
        assert mode() == "dense" and host._head_window_widths()[-1] == 4
    for bad, msg in (((1, 2), "must equal attn_window = 4"), ((4, 2), "strictly ascending"), ((2, 2, 4), "strictly ascending"),
                     ((0, 4), "strictly ascending"), ((1.0, 4), "strictly ascending"), ((True, 4), "strictly ascending"),
                     ((), "strictly ascending"), ((1, 2, 3, 4, 5), "at most 4 widths"), ("1;4", "comma-separated"), (4, "sequence of ints")):
        host.attn_window_widths = bad
        with pytest.raises(ValueError, match=msg):
            mode()
    host.attn_window_widths, host.attn_window_recall = (1, 2, 4), 0.0
    with pytest.raises(ValueError, match="needs attn_window_recall > 0"):
        mode()
    # the decision key holds the widths: other widths drop the decisions
    host.attn_window_recall = 0.9
    host._attn_decided = ((("k",), 0.9, (1, 2, 4)), [(1, 0, 4, 2)] * 2)
    assert mode() == "tables"
    host.attn_window_widths = (2, 4)
    assert mode() == "dense" and not host.attn_window_calibrated
    host._attn_decided = ((("k",), 0.9), [(True, False)] * 2)   # ... and so does switching them on behind a two-launch calibration
    assert mode() == "dense" and not host.attn_window_calibrated


def test_the_models_and_pipelines_carry_the_switch():
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    for pipe in (WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline):
        assert inspect.signature(pipe.from_pretrained).parameters["attn_window_widths"].default is None
        assert list(inspect.signature(pipe.__call__).parameters)[-1] == "attn_window_dense_steps"     # __call__ is unchanged
        with pytest.raises(ValueError, match="must equal attn_window"):
            pipe.from_pretrained("/nonexistent", transformer=object(), attn_window=4, attn_window_recall=0.9, attn_window_widths=(1, 2))
        with pytest.raises(ValueError, match="needs attn_window_recall > 0"):
            pipe.from_pretrained("/nonexistent", transformer=object(), attn_window=4, attn_window_widths=(1, 2, 4))
        with pytest.raises(ValueError, match="strictly ascending"):
            pipe.from_pretrained("/nonexistent", transformer=object(), attn_window=4, attn_window_recall=0.9, attn_window_widths=(2, 1, 4))


def test_cogvideox_refuses_the_switch():
    from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    assert isinstance(CogVideoXTransformer3DModel.attn_window_widths, property)
    model = object.__new__(CogVideoXTransformer3DModel)
    model._head_window_init()                                    # None passes
    assert model.attn_window_widths is None
    for value in ((1, 2, 4), "1,2,4", ()):
        with pytest.raises(ValueError, match="not built for head_dim 64"):
            model.attn_window_widths = value
    assert model.attn_window_widths is None
    with pytest.raises(ValueError, match="not built for head_dim 64"):
        CogVideoXImageToVideoPipeline.from_pretrained("/nonexistent", transformer=object(), attn_window=4, attn_window_recall=0.9,
                                                      attn_window_widths=(1, 2, 4))


WAN = {"model": {"path": "Wan-AI/Wan2.1-I2V-14B-480P-Diffusers", "dtype": "bfloat16"}, "generation": {"height": 480}}
HY = {"model": {"path": "hunyuanvideo-community/HunyuanVideo-I2V", "dtype": "bfloat16"}, "generation": {}}
COG = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}


def _ns(**kw):
    base = dict(fp8=False, fp8_attention=False, attn_window=0, attn_window_recall=0.0, attn_window_balance=None,
                attn_window_widths=None, step_cache=0.0, synthetic=True, model_cache_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_run_py_parses_the_flag():
    import run
    assert run.make_parser().parse_args([]).attn_window_widths is None
    ns = run.make_parser().parse_args(["--attn_window", "4", "--attn_window_recall", "0.9", "--attn_window_widths", "1,2,4"])
    assert ns.attn_window_widths == "1,2,4"


@pytest.mark.parametrize("config,kw", [
    (COG, dict(attn_window_widths="1,2,4")),                                             # head_dim 64
    (WAN, dict(attn_window=4, attn_window_widths="1,2,4")),                              # without --attn_window_recall
    (HY, dict(attn_window=4, attn_window_recall=0.9, attn_window_widths="1,2")),         # the last width is not --attn_window
    (WAN, dict(attn_window=4, attn_window_recall=0.9, attn_window_widths="2,1,4")),
    (HY, dict(attn_window=4, attn_window_recall=0.9, attn_window_widths="1,x")),
    (WAN, dict(attn_window=5, attn_window_recall=0.9, attn_window_widths="1,2,3,4,5")),
])
def test_run_py_refusals_name_the_flag(config, kw):
    import run
    with pytest.raises(SystemExit, match="--attn_window_widths"):
        run.build_pipeline(config, _ns(**kw), "cuda")
