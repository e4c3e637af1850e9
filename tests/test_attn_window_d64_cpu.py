"""The CogVideoX side of the frame window without a GPU: frame_window_ranges(prefix=) -- the prompt tokens in front of the
frames --, the C ABI of alg_flash_attn_d64_ranges, its binding's type check and the pipeline's keywords."""
import inspect
import os
import re

import pytest
import torch

from alg_amd import _lib
from alg_amd.attn_window import KV_ALIGN, Q_BLOCK, KvRanges, frame_window_ranges, ranges_to_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _todays_table(F, hw, W, sink):
    """The prefix-less policy written out independently: sink + window per block, begins rounded down, merged."""
    S = F * hw
    rows = []
    for j in range((S + Q_BLOCK - 1) // Q_BLOCK):
        fa, fb = j * Q_BLOCK // hw, (min((j + 1) * Q_BLOCK, S) - 1) // hw
        want = ([(0, min(sink, F) * hw)] if sink else []) + [(max(fa - W, 0) * hw, min(fb + W + 1, F) * hw)]
        want = sorted((b // KV_ALIGN * KV_ALIGN, e) for b, e in want)
        out = [list(want[0])]
        for b, e in want[1:]:
            if b <= out[-1][1]:
                out[-1][1] = max(out[-1][1], e)
            else:
                out.append([b, e])
        rows.append(out)
    n = max(len(r) for r in rows)
    t = torch.zeros(len(rows), n, 2, dtype=torch.int32)
    for j, r in enumerate(rows):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return t


@pytest.mark.parametrize("F,hw,W,sink", [(13, 1350, 2, 1), (6, 160, 1, 1), (21, 1560, 4, 2), (9, 100, 0, 0), (5, 104, 1, 1)])
def test_prefix_zero_is_todays_table(F, hw, W, sink):
    a = frame_window_ranges(F, hw, W, sink_frames=sink)
    b = frame_window_ranges(F, hw, W, sink_frames=sink, prefix=0)
    assert torch.equal(a.table, b.table) and (a.Sq, a.Skv, a.max_ranges, a.coverage) == (b.Sq, b.Skv, b.max_ranges, b.coverage)
    assert torch.equal(a.table, _todays_table(F, hw, W, sink))


@pytest.mark.parametrize("prefix", [226, 256])
@pytest.mark.parametrize("F,hw,W,sink", [(13, 1350, 1, 1), (6, 160, 1, 1), (9, 100, 2, 2), (7, 300, 0, 1), (8, 333, 1, 0)])
def test_prefixed_tables(prefix, F, hw, W, sink):
    r = frame_window_ranges(F, hw, W, sink_frames=sink, prefix=prefix)
    S = prefix + F * hw
    assert isinstance(r, KvRanges) and (r.Sq, r.Skv) == (S, S) and r.max_ranges <= 4 and 0 < r.coverage < 1
    mask = ranges_to_mask(r)
    frame_of = (torch.arange(S) - prefix).div(hw, rounding_mode="floor")          # < 0: a prompt row
    for q in list(range(prefix, S, 97)) + [prefix, S - 1]:                          # latent queries: text + sink + window are seen
        f = int(frame_of[q])
        want = (frame_of < 0) | ((frame_of >= 0) & (frame_of < sink)) | ((frame_of - f).abs() <= W)
        assert bool(mask[q][want].all()), q
    for j in range(r.q_blocks):
        used = [(int(b), int(e)) for b, e in r.table[j].tolist() if e > b]
        if j * Q_BLOCK < prefix:                                                    # prompt rows, and the block that straddles
            assert used == [(0, S)], j
        assert used and all(b % KV_ALIGN == 0 and 0 <= b < e <= S for b, e in used), j
        assert all(used[i][1] < used[i + 1][0] for i in range(len(used) - 1)), j   # sorted, disjoint, merged where touching
        assert r.table[j, len(used):].abs().sum() == 0                              # unused entries trail as (0, 0)
    assert bool(mask[: min(prefix, S)].all())                                       # prompt queries see everything


def test_prefix_with_tail_raises_and_a_covering_window_is_dense():
    with pytest.raises(ValueError, match="prefix"):
        frame_window_ranges(4, 100, 1, tail=(400, 420), prefix=10)
    with pytest.raises(ValueError):
        frame_window_ranges(4, 100, 1, prefix=-3)
    assert frame_window_ranges(13, 1350, 12, prefix=226) is None
    assert frame_window_ranges(13, 1350, 40, prefix=226) is None
    assert frame_window_ranges(6, 160, 5, sink_frames=0, prefix=70) is None


def test_the_c2_table_has_two_ranges():
    """226 prompt tokens + 13 latent frames of 1,350: the prompt and the sink frame merge into [0, 1576)."""
    for W in (1, 2, 4):
        r = frame_window_ranges(13, 1350, W, prefix=226)
        assert (r.Sq, r.Skv, r.q_blocks, r.max_ranges) == (17776, 17776, 70, 2)
        assert r.table[0].tolist() == [[0, 17776], [0, 0]]                          # the block with the prompt rows
        assert r.table[-1, 0].tolist() == [0, 1576] and int(r.table[-1, 1, 1]) == 17776 and int(r.table[-1, 1, 0]) % 64 == 0
    cov = [frame_window_ranges(13, 1350, W, prefix=226).coverage for W in (1, 2, 4)]
    assert cov == sorted(cov) and 0.25 < cov[0] < cov[2] < 0.75


def test_header_declares_the_ranged_entry_and_the_binding_checks_its_table():
    text = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    m = re.search(r"int\s+alg_flash_attn_d64_ranges\s*\(([^;]*)\)\s*;", text)
    assert m, "alg_flash_attn_d64_ranges is not declared in include/alg_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const void* q", "const void* k", "const void* vt", "void* o", "int batch", "int heads", "int S",
                    "int64_t q_bstride", "int64_t q_rstride", "int64_t vt_bstride", "int64_t vt_rstride", "int64_t o_bstride",
                    "int64_t o_rstride", "const int32_t* kv_ranges", "int max_ranges", "void* stream"]
    assert "alg_flash_attn_d64_ranges" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "attention.hip")).read()
    assert re.search(r'extern "C" int alg_flash_attn_d64_ranges\(', src)
    params = list(inspect.signature(_lib.flash_attn_d64_ranges).parameters)
    assert params == ["q", "k", "vt", "o", "batch", "heads", "S", "q_bstride", "q_rstride", "vt_bstride", "vt_rstride", "o_bstride",
                      "o_rstride", "kv_ranges", "q_off", "k_off"]
    t = torch.zeros(4, 64, dtype=torch.bfloat16)
    table = torch.zeros(1, 1, 2, dtype=torch.int32)
    with pytest.raises(_lib.AlgHipError, match="KvRanges"):                         # before the library or a device is touched
        _lib.flash_attn_d64_ranges(t, t, t, t, 1, 1, 4, 256, 64, 4096, 64, 256, 64, table)
    with pytest.raises(_lib.AlgHipError, match="built for"):
        _lib.flash_attn_d64_ranges(t, t, t, t, 1, 1, 4, 256, 64, 4096, 64, 256, 64, frame_window_ranges(6, 160, 1, prefix=70))


def test_cog_pipeline_keywords_and_transformer_attributes():
    from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline as Pipe
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel as Model
    call = inspect.signature(Pipe.__call__).parameters
    assert list(call)[-1] == "attn_window_dense_steps" and call["attn_window_dense_steps"].default == 0   # behind the existing extras
    assert list(call).index("attn_window_dense_steps") > list(call).index("schedule_exp_decay_rate")     # ... and the reference's
    fp = inspect.signature(Pipe.from_pretrained).parameters
    assert fp["attn_window"].default == 0 and list(fp).index("attn_window") > list(fp).index("cache_dir")
    assert callable(getattr(Model, "_window_ranges")) and list(inspect.signature(Model._window_ranges).parameters) == [
        "self", "frames", "hw", "T"]
    import run
    helptext = run.make_parser().format_help()
    assert "transformer.attn_window" in " ".join(helptext.split())
