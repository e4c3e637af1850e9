"""Position-major band attention, the host side (alg_amd/attn_window.py): the permutation, the band table and its promise, absent
heads in a per-head table, the three-way decision, the C ABI of the two layout entries against the binding and their refusals,
the switch on the Wan transformer / pipeline, and run.py's flag with its refusals.  No GPU."""
import argparse
import ctypes
import inspect
import os
import re

import pytest
import torch

import alg_amd
from alg_amd.attn_window import (HeadList, HeadWindowHost, KvRanges, KvRangesHeads, decide_layouts, frame_window_ranges,
                                 full_ranges, head_layout_ranges, mean_unit_cost, position_band_ranges, position_major_index,
                                 ranges_to_mask, unit_costs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CASES = [(6, 160, 2), (5, 77, 0), (21, 1560, 8), (1, 300, 3), (7, 1, 0)]


@pytest.mark.parametrize("F,HW", [(6, 160), (5, 77), (1, 96), (9, 1), (21, 1560)])
def test_the_permutation_is_a_bijection_and_its_inverse_is_the_transposed_one(F, HW):
    pi, inv = position_major_index(F, HW), position_major_index(HW, F)
    S = F * HW
    assert pi.dtype == torch.int64 and tuple(pi.shape) == (S,) and pi.device.type == "cpu"
    assert torch.equal(pi.sort().values, torch.arange(S))
    assert torch.equal(pi[inv], torch.arange(S)) and torch.equal(inv[pi], torch.arange(S))
    for f, p in ((0, 0), (F - 1, HW - 1), (F // 2, HW // 3)):
        assert pi[f * HW + p] == p * F + f
    with pytest.raises(ValueError):
        position_major_index(0, 4)


@pytest.mark.parametrize("F,HW,band", CASES)
def test_band_table_is_valid_and_holds_every_querys_promised_keys(F, HW, band):
    S = F * HW
    r = position_band_ranges(F, HW, band)
    rows = [[(max(0, qb * 256 // F - band) * F) & ~63, min(HW, (min((qb + 1) * 256, S) - 1) // F + band + 1) * F]
            for qb in range((S + 255) // 256)]
    if all(row == [0, S] for row in rows):                    # (7, 1, 0): one position, so the formula gives the dense attention
        assert r is None and (F, HW, band) == (7, 1, 0)
        return
    assert isinstance(r, KvRanges) and (r.Sq, r.Skv, r.max_ranges) == (S, S, 1) and r.q_blocks == (S + 255) // 256
    KvRanges(r.table, S, S)                                   # validates again from the raw table
    for qb in range(r.q_blocks):                              # the formula of the issue, block by block
        p0, p1 = qb * 256 // F, (min((qb + 1) * 256, S) - 1) // F
        assert r.table[qb, 0].tolist() == [(max(0, p0 - band) * F) & ~63, min(HW, p1 + band + 1) * F]
    # every query (p, f) sees all frames of the positions within `band` of p: rows of the mask, compared run by run
    if S <= 4096:
        mask = ranges_to_mask(r)
        p = torch.arange(S) // F
        want = (p[:, None] - p[None, :]).abs() <= band        # [query row][key row], both position-major
        assert bool((mask | ~want).all()) and bool(mask.any(dim=1).all())
    else:
        for row in (0, 255, 256, S // 2, S - 1):
            b, e = r.table[row // 256, 0].tolist()
            p = row // F
            assert b <= max(0, p - band) * F and min(HW, p + band + 1) * F <= e
    assert 0.0 < r.coverage < 1.0


def test_band_that_covers_every_position_is_the_dense_attention():
    assert position_band_ranges(6, 160, 160) is None and position_band_ranges(6, 160, 1000) is None
    assert position_band_ranges(7, 1, 0) is None              # one position: its own band is everything
    assert position_band_ranges(6, 160, 159) is None          # every block reaches both ends
    with pytest.raises(ValueError):
        position_band_ranges(6, 160, -1)
    c3 = position_band_ranges(21, 1560, 8)                    # the C3 shape of the issue: about 600 of 32,760 keys
    assert 500 <= c3.coverage * 32760 <= 700


def test_absent_heads_are_opt_in_and_cost_nothing():
    good = full_ranges(300, 512).table                         # [2, 1, 2]
    empty = torch.zeros_like(good)
    with pytest.raises(ValueError, match=r"block 0: no key"):
        KvRanges(empty, 512, 300)                              # the default is what it was
    with pytest.raises(ValueError, match=r"head 0: block 0: no key"):
        KvRangesHeads(torch.stack([empty, good]), 512, 300)
    assert not KvRanges(good, 512, 300).absent and not KvRanges(good, 512, 300, absent_ok=True).absent
    a = KvRanges(empty, 512, 300, absent_ok=True)
    assert a.absent and a.coverage == 0.0 and not a.is_full
    half = good.clone()
    half[1] = 0                                                # one block empty, the other not: an error with the argument too
    with pytest.raises(ValueError, match=r"block 1: no key"):
        KvRanges(half, 512, 300, absent_ok=True)
    t = KvRangesHeads(torch.stack([empty, good, empty, good]), 512, 300, absent_ok=True)
    assert [r.absent for r in t.per_head] == [True, False, True, False] and t.coverage == 0.5
    costs = unit_costs(t, 2, 4)
    assert len(costs) == 8 and costs[0] == [0, 0] and costs[2] == [0, 0] and costs[1] == [10, 10] and costs[4:] == costs[:4]
    assert not bool(ranges_to_mask(t)[0].any()) and bool(ranges_to_mask(t)[1].all())


def test_head_layout_ranges_leaves_band_heads_out_of_the_main_table():
    base = frame_window_ranges(6, 160, 1)
    t, band = head_layout_ranges(base, ["band", "window", "dense", "band"])
    assert band == (0, 3) and isinstance(t, KvRangesHeads) and [r.absent for r in t.per_head] == [True, False, False, True]
    assert torch.equal(t.table[1], base.table) and t.per_head[2].is_full
    assert head_layout_ranges(base, ["band"] * 3) == (None, (0, 1, 2))
    t, band = head_layout_ranges(base, ["window", "dense"])
    assert band == () and isinstance(t, KvRangesHeads) and not any(r.absent for r in t.per_head)   # head_window_ranges' table
    assert head_layout_ranges(base, ["window", "window"]) == (base, ()) and head_layout_ranges(base, ["dense"]) == (None, ())
    with pytest.raises(ValueError):
        head_layout_ranges(base, ["window", "strip"])
    hl = HeadList(band or (3, 0), 4)
    assert hl.n_sel == 2 and hl.table.dtype == torch.int32 and hl.table.tolist() == [3, 0]
    for bad in ([], [0, 0], [4], [-1]):
        with pytest.raises(ValueError):
            HeadList(bad, 4)


def test_decide_layouts_picks_the_cheaper_qualifying_candidate():
    thr = 0.9
    #          both, band cheaper | window only | band only | neither | NaN in window | NaN in band
    rw = [[0.95, 0.95, 0.50, 0.5, NAN, 0.95]]
    rb = [[0.95, 0.10, 0.95, 0.5, 0.95, NAN]]
    assert decide_layouts(rw, rb, 10.0, 4.0, thr) == ["band", "window", "band", "dense", "band", "window"]
    assert decide_layouts(rw, rb, 4.0, 10.0, thr) == ["window", "window", "band", "dense", "band", "window"]
    assert decide_layouts(rw, rb, 7.0, 7.0, thr)[0] == "window"                       # a tie goes to the window
    assert decide_layouts([[NAN]], [[NAN]], 1.0, 1.0, 0.0) == ["dense"]              # NaN never qualifies
    # a candidate qualifies only if EVERY sample reaches the threshold
    assert decide_layouts([[0.95, 0.95], [0.95, 0.89]], [[0.95, 0.95], [0.89, 0.95]], 10.0, 4.0, thr) == ["window", "band"]
    assert decide_layouts([[0.3]], [[0.4]], 1.0, 2.0, 2.0) == ["dense"] and decide_layouts([[0.3]], [[0.4]], 3.0, 2.0, 1e-9) == ["band"]
    for bad in (([], []), ([[0.5, 0.5]], [[0.5]]), ([[0.5]], [[0.5], [0.5]])):
        with pytest.raises(ValueError):
            decide_layouts(bad[0], bad[1], 1.0, 1.0, 0.5)
    with pytest.raises(ValueError):
        decide_layouts([[0.5]], [[0.5]], NAN, 1.0, 0.5)
    base, band = frame_window_ranges(6, 160, 1), position_band_ranges(6, 160, 2)
    assert mean_unit_cost(band) < mean_unit_cost(base)                                 # what the model test relies on
    assert mean_unit_cost(base) == sum(unit_costs(base, 1, 1)[0]) / base.q_blocks


def _prototype(name, text):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


ENTRIES = (("alg_attn_rows_position_major", 14, "attn_rows_position_major"), ("alg_attn_vt_position_major", 13, "attn_vt_position_major"))


def test_header_exports_and_wrappers_agree_on_the_two_layout_entries():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "attn_layout.hip")).read()
    lib_src = open(os.path.join(ROOT, "alg_amd", "_lib.py")).read()
    assert "attn_layout.hip" in open(os.path.join(ROOT, "alg_amd", "csrc", "Makefile")).read()
    for name, n_args, wrapper in ENTRIES:
        assert name in alg_amd._lib.EXPORTS and callable(getattr(alg_amd._lib, wrapper))
        declared, defined = _prototype(name, header), _prototype(name, src[src.index('extern "C" int ' + name + "("):])
        assert len(declared) == n_args
        strip = lambda a: a.rsplit(" ", 1)[0]
        assert [strip(a) for a in declared] == [strip(a) for a in defined], name
        m = re.search(r"lib\.%s\.argtypes = (.*?)\n    lib\." % name, lib_src, re.S)
        ns = {k: getattr(alg_amd._lib, k) for k in ("c_void_p", "c_int", "c_int64", "c_float")}
        assert len(eval(m.group(1), ns)) == n_args, name
    assert _prototype("alg_attn_rows_position_major", header)[6:] == ["const int32_t* head_list", "int n_sel", "int head_dim", "int batch",
                                                                      "int frames", "int hw", "int inverse", "void* stream"]
    assert "atomic" not in src.split("namespace alg {", 1)[1].lower()


def test_the_layout_entries_refuse_bad_arguments_before_any_launch():
    """Every refusal comes from the argument checks: the pointers below are never dereferenced (no GPU here)."""
    lib = alg_amd._lib.load_library()
    for name, _, _ in ENTRIES:
        assert hasattr(lib, name)
    P = ctypes.c_void_p
    good = dict(src=0x10000, sbs=960 * 512, srs=512, dst=0x20000, dbs=960 * 256, drs=256, hl=0x30000, n_sel=2, hd=128, batch=2, F=6, hw=160)

    def rows(inverse=0, **kw):
        a = dict(good, **kw)
        return lib.alg_attn_rows_position_major(P(a["src"]), a["sbs"], a["srs"], P(a["dst"]), a["dbs"], a["drs"], P(a["hl"]), a["n_sel"],
                                                a["hd"], a["batch"], a["F"], a["hw"], inverse, P(0))

    def vt(**kw):
        a = dict(good, sbs=512 * 960, srs=960, dbs=256 * 960, drs=960)
        a.update(kw)
        return lib.alg_attn_vt_position_major(P(a["src"]), a["sbs"], a["srs"], P(a["dst"]), a["dbs"], a["drs"], P(a["hl"]), a["n_sel"],
                                              a["hd"], a["batch"], a["F"], a["hw"], P(0))

    bad_common = [dict(src=0), dict(dst=0), dict(hl=0), dict(src=0x10008), dict(dst=0x20002), dict(hl=0x30002), dict(hd=96), dict(hd=0),
                  dict(n_sel=0), dict(batch=0), dict(F=0), dict(hw=0), dict(F=-3), dict(srs=12), dict(dbs=7)]
    for kw in bad_common + [dict(srs=128), dict(drs=128), dict(dbs=100)]:
        assert rows(**kw) == -1, kw
        assert b"alg_attn_rows_position_major" in lib.alg_last_error(), kw
    assert rows(inverse=2) == -1 and b"alg_attn_rows_position_major" in lib.alg_last_error()
    for kw in bad_common + [dict(srs=952), dict(drs=896), dict(hw=161), dict(dbs=255 * 960)]:     # 966 keys need a row stride of 1024
        assert vt(**kw) == -1, kw
        assert b"alg_attn_vt_position_major" in lib.alg_last_error(), kw
    L = alg_amd._lib
    with pytest.raises(L.AlgHipError, match="HeadList"):
        L.attn_rows_position_major(None, None, [0, 1], 128, 1, 6, 160, 0, 0, 0, 0)
    with pytest.raises(L.AlgHipError, match="HeadList"):
        L.attn_vt_position_major(None, None, torch.tensor([0]), 128, 1, 6, 160, 0, 0, 0, 0)
    with pytest.raises(L.AlgHipError, match="head_dim"):
        L.attn_rows_position_major(None, None, HeadList([0], 4), 96, 1, 6, 160, 0, 0, 0, 0)
    with pytest.raises(L.AlgHipError, match="4 heads"):
        L.attn_rows_position_major(None, None, HeadList([0], 4), 128, 1, 6, 160, 0, 256, 0, 128)   # the wide row holds 2 heads


class _Host(HeadWindowHost):
    def __init__(self, **kw):
        self._head_window_init()
        self.attn_window = 0
        self.__dict__.update(kw)


def test_the_switch_validates():
    assert _Host()._head_window_band() == 0                                            # no attribute: off
    assert _Host(attn_band=0)._head_window_band() == 0
    assert _Host(attn_band=3, attn_window=1, attn_window_recall=0.9)._head_window_band() == 3
    for kw in (dict(attn_band=3), dict(attn_band=3, attn_window=1), dict(attn_band=3, attn_window_recall=0.9), dict(attn_band=-1),
               dict(attn_band=1.5), dict(attn_band=True), dict(attn_band="2")):
        with pytest.raises(ValueError, match="attn_band"):
            _Host(**kw)._head_window_band()
    with pytest.raises(ValueError, match="attn_window_widths"):
        _Host(attn_band=3, attn_window=2, attn_window_recall=0.9, attn_window_widths=(1, 2))._head_window_band()
    # the decision key carries the band: changing it drops the decisions
    h = _Host(attn_band=3, attn_window=1, attn_window_recall=0.9)
    h._attn_decided = ((("k",), 0.9, ("band", 3)), [("band", "dense")])
    assert h._head_window_mode(("k",), 1, 1, 2, 256, (1, 256, 256), band=3) == "tables"
    assert h._head_window_mode(("k",), 1, 1, 2, 256, (1, 256, 256), band=4) == "dense" and not h.attn_window_calibrated
    h._attn_decided = ((("k",), 0.9), [(True, False)])                                 # band off: today's key
    assert h._head_window_mode(("k",), 1, 1, 2, 256, (1, 256, 256)) == "tables"


def test_only_the_wan_family_carries_the_switch():
    from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel
    params = list(inspect.signature(WanImageToVideoPipeline.from_pretrained).parameters)
    assert params[-2:] == ["attn_band", "_"] and params[-3] == "attn_window_widths"    # appended behind the existing keywords
    assert inspect.signature(WanImageToVideoPipeline.from_pretrained).parameters["attn_band"].default == 0
    assert list(inspect.signature(WanImageToVideoPipeline.__call__).parameters)[-1] == "attn_window_dense_steps"
    assert "self.attn_band = 0" in inspect.getsource(WanTransformer3DModel.__init__)
    for cls in (HunyuanVideoTransformer3DModel, CogVideoXTransformer3DModel):
        assert not hasattr(cls, "attn_band") and "attn_band" not in inspect.getsource(inspect.getmodule(cls))
    for pipe in (HunyuanVideoImageToVideoPipeline, CogVideoXImageToVideoPipeline):
        assert "attn_band" not in inspect.signature(pipe.from_pretrained).parameters
    # the keyword is checked before anything is loaded
    for kw in (dict(attn_band=2), dict(attn_band=2, attn_window=1), dict(attn_band=-2, attn_window=1, attn_window_recall=0.9),
               dict(attn_band=2, attn_window=2, attn_window_recall=0.9, attn_window_widths=(1, 2)),
               dict(attn_band=2, attn_window=1, attn_window_recall=0.9, fp8_attention=True)):
        with pytest.raises(ValueError, match="attn_band"):
            WanImageToVideoPipeline.from_pretrained("/nonexistent", **kw)


WAN = {"model": {"path": "Wan-AI/Wan2.1-I2V-14B-480P-Diffusers", "dtype": "bfloat16"}, "generation": {"height": 480}}
HY = {"model": {"path": "hunyuanvideo-community/HunyuanVideo-I2V", "dtype": "bfloat16"}, "generation": {}}
COG = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}


def _ns(**kw):
    base = dict(fp8=False, fp8_attention=False, attn_window=0, attn_window_recall=0.0, step_cache=0.0, synthetic=True,
                model_cache_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_run_py_parses_the_flag():
    import run
    assert run.make_parser().parse_args([]).attn_band == 0
    ns = run.make_parser().parse_args(["--attn_window", "4", "--attn_window_recall", "0.9", "--attn_band", "8"])
    assert ns.attn_band == 8 and ns.attn_window == 4


@pytest.mark.parametrize("config,kw", [
    (HY, dict(attn_window=4, attn_window_recall=0.9, attn_band=8)),
    (COG, dict(attn_band=8)),
    (WAN, dict(attn_band=8)),                                          # without --attn_window_recall
    (WAN, dict(attn_window=4, attn_band=8)),
    (WAN, dict(attn_window=4, attn_window_recall=0.9, attn_band=-1)),
    (WAN, dict(attn_window=4, attn_window_recall=0.9, attn_window_widths="1,4", attn_band=8)),
])
def test_run_py_refusals_name_the_flag(config, kw):
    import run
    with pytest.raises(SystemExit, match="--attn_band"):
        run.build_pipeline(config, _ns(**kw), "cuda")
