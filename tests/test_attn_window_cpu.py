"""The host policy of the frame-window self-attention (alg_amd/attn_window.py) on the CPU: frame_window_ranges against a
brute-force mask, KvRanges' validation rule by rule, and the new export's declaration."""
import os
import re

import pytest
import torch

import alg_amd
from alg_amd.attn_window import KvRanges, frame_window_ranges, ranges_to_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [((6, 160), 1, 1, None), ((5, 104), 0, 1, None), ((21, 1560), 4, 1, None), ((33, 3600), 8, 1, (118800, 118800 + 77))]


@pytest.mark.parametrize("shape,window,sink,tail", CASES)
def test_frame_window_ranges_against_brute_force(shape, window, sink, tail):
    F, hw = shape
    S = F * hw
    r = frame_window_ranges(F, hw, window, sink_frames=sink, tail=tail)
    assert isinstance(r, KvRanges)
    Skv = tail[1] if tail else S
    assert (r.Sq, r.Skv, r.q_blocks) == (S, Skv, (S + 255) // 256)
    assert r.max_ranges <= 4 and tuple(r.table.shape) == (r.q_blocks, r.max_ranges, 2)
    tab = r.table.tolist()
    for j, rows in enumerate(tab):
        used = [(b, e) for b, e in rows if (b, e) != (0, 0)]
        assert used and rows[:len(used)] == [list(u) for u in used], j          # used entries first, at least one
        for i, (b, e) in enumerate(used):
            assert b % 64 == 0 and b < e <= Skv, (j, b, e)
            assert i == 0 or used[i - 1][1] < b, (j, used)                         # sorted, disjoint (touching ones are merged)
    # every query's own +-W frames, the sink and the tail lie inside its block's ranges: what a query must see, per frame
    # (a frame-level brute force keeps the 118,800-row case cheap: the mask is expanded per block, never as [Sq, Skv])
    visits = 0
    for j, rows in enumerate(tab):
        row = torch.zeros(Skv, dtype=torch.bool)
        for b, e in rows:
            row[b:e] = True
        q0, q1 = j * 256, min((j + 1) * 256, S)
        need = torch.zeros(Skv, dtype=torch.bool)
        for f in range(q0 // hw, (q1 - 1) // hw + 1):
            need[max(f - window, 0) * hw:min(f + window + 1, F) * hw] = True
        need[:sink * hw] = True
        if tail:
            need[tail[0]:tail[1]] = True
        assert bool(row[need].all()), j
        visits += int(row.sum()) * (q1 - q0)
    assert abs(r.coverage - visits / (S * Skv)) < 1e-12
    if S * Skv <= 1 << 24:                                                           # the full mask where it is small
        m = ranges_to_mask(r)
        assert tuple(m.shape) == (S, Skv)
        assert abs(r.coverage - m.float().mean().item()) < 1e-6
        q = torch.arange(S)
        k = torch.arange(Skv)
        fq, fk = q // hw, k // hw
        brute = ((fk[None] - fq[:, None]).abs() <= window) | (fk[None] < sink)
        assert bool(m[brute].all())
    assert r.coverage < 1.0


def test_hunyuan_prompt_rows_see_everything():
    F, hw, valid, L = 5, 104, 20, 32
    S = F * hw
    r = frame_window_ranges(F, hw, 1, tail=(S, S + valid), rows=S + L)
    assert (r.Sq, r.Skv) == (S + L, S + valid)
    m = ranges_to_mask(r)
    assert bool(m[S:].all())                                   # prompt queries: every key
    assert bool(m[(S // 256) * 256:].all())                    # and the block that straddles the boundary
    assert bool(m[:, S:].all()) and bool(m[:, :hw - hw % 64].all())     # everybody: the prompt keys and the sink
    assert not bool(m.all())


def test_window_covering_the_video_is_dense():
    assert frame_window_ranges(6, 160, 5) is None
    assert frame_window_ranges(6, 160, 9) is None
    assert frame_window_ranges(5, 104, 4, tail=(520, 540), rows=552) is None
    assert frame_window_ranges(12, 160, 4) is not None


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("rows,rule", [
    ([[[128, 192], [0, 64]], [[0, 512], [0, 0]]], "sorted"),                       # unsorted
    ([[[0, 130], [128, 192]], [[0, 512], [0, 0]]], "overlaps"),                    # overlapping
    ([[[0, 64], [100, 192]], [[0, 512], [0, 0]]], "multiple of 64"),               # unaligned begin
    ([[[0, 64], [128, 513]], [[0, 512], [0, 0]]], "beyond Skv"),                   # end > Skv
    ([[[0, 64], [128, 192]], [[0, 0], [0, 0]]], "block 1: no key"),                # an empty block
    ([[[0, 0], [128, 192]], [[0, 512], [0, 0]]], "behind an unused one"),          # used entries after an unused one
    ([[[64, 64], [0, 0]], [[0, 512], [0, 0]]], "begin < end"),                     # an empty entry that is not (0, 0)
])
def test_kv_ranges_raises_on_each_broken_rule(rows, rule):
    with pytest.raises(ValueError, match=rule):
        KvRanges(_table(rows), 512, 300)


def test_kv_ranges_accepts_a_valid_table_and_counts_coverage():
    r = KvRanges(_table([[[0, 64], [128, 192]], [[0, 512], [0, 0]]]), 512, 300)
    assert (r.q_blocks, r.max_ranges, r.Sq, r.Skv) == (2, 2, 300, 512)
    assert abs(r.coverage - (128 * 256 + 512 * 44) / (300 * 512)) < 1e-12
    assert abs(r.coverage - ranges_to_mask(r).float().mean().item()) < 1e-6
    with pytest.raises(ValueError):
        KvRanges(_table([[[0, 64]]]), 512, 300)                # one block for 300 queries
    with pytest.raises(ValueError):
        KvRanges(torch.zeros(2, 5, 2, dtype=torch.int32), 512, 300)
    with pytest.raises(ValueError):
        KvRanges(torch.zeros(2, 2, 2, dtype=torch.int64), 512, 300)


def test_the_wrapper_takes_only_validated_tables():
    with pytest.raises(alg_amd._lib.AlgHipError, match="KvRanges"):
        alg_amd._lib.flash_attn_d128_ranges(None, None, None, None, 1, 1, 300, 512, 0, 0, 0, 0, 0, 0, 0, 0, 1.0,
                                            _table([[[0, 512]], [[0, 512]]]))


def test_ranges_entry_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    assert "alg_flash_attn_d128_ranges" in declared
    assert "alg_flash_attn_d128_ranges" in alg_amd._lib.EXPORTS
    assert callable(alg_amd._lib.flash_attn_d128_ranges)
    assert re.search(r"alg_flash_attn_d128_ranges\([^;]*const int32_t\* kv_ranges,\s*int max_ranges, void\* stream\);", header)


def test_run_py_has_the_flag_and_a_cogvideox_config_refuses_it():
    import argparse
    import inspect

    import run
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    assert run.make_parser().parse_args([]).attn_window == 0
    assert run.make_parser().parse_args(["--attn_window", "4"]).attn_window == 4
    config = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}
    ns = argparse.Namespace(fp8=False, fp8_attention=False, attn_window=4, synthetic=True, model_cache_dir=None)
    with pytest.raises(SystemExit, match="head_dim 128"):
        run.build_pipeline(config, ns, "cuda")
    config = {"model": {"path": "Wan-AI/Wan2.1-I2V-14B-480P-Diffusers", "dtype": "bfloat16"}, "generation": {"height": 480}}
    ns = argparse.Namespace(fp8=False, fp8_attention=True, attn_window=4, synthetic=True, model_cache_dir=None)
    with pytest.raises(SystemExit, match="fp8_attention"):
        run.build_pipeline(config, ns, "cuda")
    for pipe in (WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline):
        assert list(inspect.signature(pipe.__call__).parameters)[-1] == "attn_window_dense_steps"     # behind the existing extras
        assert inspect.signature(pipe.__call__).parameters["attn_window_dense_steps"].default == 0
        assert inspect.signature(pipe.from_pretrained).parameters["attn_window"].default == 0
