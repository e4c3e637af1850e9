"""The host side of the coverage-balanced launch order (alg_amd/attn_window.py: LaunchOrder, unit_costs, balanced_order), without a
GPU: what LaunchOrder refuses, that every policy's output is a valid order with the layout it promises, the costs against the
tables they are taken from, the policies against two list-scheduling MODELS of the dispatch, and that header, library and wrapper
agree on the two entries (alg_flash_attn_d128_ranges_order, alg_flash_attn_d64_ranges_order)."""
import heapq
import inspect
import os
import re
import subprocess

import pytest
import torch

import alg_amd
from alg_amd.attn_window import (KV_ALIGN, LANES, ORDER_POLICIES, SEGMENT_COST, KvRanges, KvRangesHeads, LaunchOrder,
                                 balanced_order, frame_window_ranges, full_ranges, head_window_ranges, unit_costs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 2, 3), (2, 3, 3), (1, 9, 2), (3, 40, 5)]


def _order(entries):
    return torch.tensor(entries, dtype=torch.int32)


def test_launch_order_names_the_rule_and_the_first_offending_entry():
    good = [0, 1, 2, 3, 4, 5, -1, -1]
    assert LaunchOrder(_order(good), 1, 2, 3).order.tolist() == good
    with pytest.raises(ValueError, match=r"missing unit 5 \(bh 1, q block 2\)"):
        LaunchOrder(_order([0, 1, 2, 3, 4, -1, -1, -1]), 1, 2, 3)
    with pytest.raises(ValueError, match=r"entry 6: duplicate unit 2 \(first at entry 2"):
        LaunchOrder(_order([0, 1, 2, 3, 4, 5, 2, -1]), 1, 2, 3)
    with pytest.raises(ValueError, match=r"entry 7 is 6: out of range"):
        LaunchOrder(_order([0, 1, 2, 3, 4, 5, -1, 6]), 1, 2, 3)
    with pytest.raises(ValueError, match=r"entry 1 is -2: out of range"):
        LaunchOrder(_order([0, -2, 2, 3, 4, 5, 1, -1]), 1, 2, 3)
    with pytest.raises(ValueError, match=r"length 7 is not a multiple of 8"):
        LaunchOrder(_order(good[:7]), 1, 2, 3)
    with pytest.raises(ValueError, match=r"CPU int32 vector, got torch.int64"):
        LaunchOrder(torch.tensor(good), 1, 2, 3)
    with pytest.raises(ValueError, match=r"CPU int32 vector"):
        LaunchOrder(_order(good).reshape(2, 4), 1, 2, 3)
    kept = _order(good)
    lo = LaunchOrder(kept, 1, 2, 3)
    kept[0] = 5                                   # the order holds a copy
    assert lo.order[0].item() == 0 and len(lo) == 8 and (lo.batch, lo.heads, lo.q_blocks) == (1, 2, 3)


def _costs(B, H, Q):
    """Distinct-ish costs with ties: head-dependent (a dense head costs more) and block-dependent."""
    return [[(7 if (bh % H) % 2 == 0 else 2) + (qb % 2) for qb in range(Q)] for bh in range(B * H)]


def _lanes_of(order):
    return [order.order[x::LANES].tolist() for x in range(LANES)]


@pytest.mark.parametrize("B,H,Q", SHAPES)
def test_every_policy_gives_a_valid_order_with_its_layout(B, H, Q):
    costs = _costs(B, H, Q)
    nbh = B * H
    cost = lambda u: costs[u // Q][u % Q]
    for policy in ORDER_POLICIES:
        lo = balanced_order(costs, policy, heads=H)
        assert isinstance(lo, LaunchOrder) and (lo.batch, lo.heads, lo.q_blocks) == (B, H, Q)
        LaunchOrder(lo.order, B, H, Q)            # validates again: every unit exactly once, -1 elsewhere, length % 8 == 0
    # "natural": the kernels' formula entry for entry, padding exactly where bh >= nbh
    nat = balanced_order(costs, "natural", heads=H).order.tolist()
    assert len(nat) == (nbh + 7) // 8 * 8 * Q
    for b, u in enumerate(nat):
        xcd, idx = b & 7, b >> 3
        slot = idx // Q
        qb, bh = idx - slot * Q, slot * 8 + xcd
        assert u == (bh * Q + qb if bh < nbh else -1), b
    # "lanes": every head on one lane, each lane non-increasing in cost, padding at the end only
    lanes = _lanes_of(balanced_order(costs, "lanes", heads=H))
    where = {}
    for x, lane in enumerate(lanes):
        used = [u for u in lane if u >= 0]
        assert lane == used + [-1] * (len(lane) - len(used)), x
        assert all(cost(a) >= cost(b) for a, b in zip(used, used[1:])), x
        for u in used:
            assert where.setdefault(u // Q, x) == x, (u, x)
    assert sorted(where) == list(range(nbh))
    loads = [sum(cost(u) for u in lane if u >= 0) for lane in lanes]
    assert max(loads) - min(loads) <= max(sum(r) for r in costs)          # greedy: within one head of each other
    # "units": globally non-increasing when read lane-interleaved (= in entry order), ties by (bh, qb)
    un = balanced_order(costs, "units", heads=H).order.tolist()
    used = [u for u in un if u >= 0]
    assert un == used + [-1] * (len(un) - len(used)) and len(un) == (nbh * Q + 7) // 8 * 8
    assert used == sorted(range(nbh * Q), key=lambda u: (-cost(u), u))
    assert balanced_order(costs).order.tolist() == balanced_order(costs, "lanes").order.tolist()          # the default
    with pytest.raises(ValueError, match="policy must be one of"):
        balanced_order(costs, "pool")
    with pytest.raises(ValueError, match="no multiple of heads"):
        balanced_order(costs, "lanes", heads=nbh + 1)


def test_lanes_ties_go_to_the_lower_head_and_the_lower_lane():
    lanes = _lanes_of(balanced_order([[3, 3]] * 9, "lanes"))
    assert lanes[0] == [0, 1, 16, 17] and lanes[1] == [2, 3, -1, -1] and lanes[7] == [14, 15, -1, -1]


def test_unit_costs_on_a_full_range_table():
    for Sq, Skv in ((300, 512), (1300, 2050), (256, 65)):
        c = unit_costs(full_ranges(Sq, Skv), 2, 3)
        assert len(c) == 6 and all(len(r) == (Sq + 255) // 256 for r in c)
        assert all(x == -(-Skv // KV_ALIGN) + SEGMENT_COST for r in c for x in r)
    assert SEGMENT_COST == 2


def _row_cost(row):
    return sum(-(-(e - b) // KV_ALIGN) + SEGMENT_COST for b, e in row.tolist() if e > b)


def test_unit_costs_on_a_head_window_table_are_the_costs_of_the_rows_it_was_built_from():
    base = frame_window_ranges(13, 1350, 2, prefix=226)
    windowed = [h % 3 != 0 for h in range(6)]
    table = head_window_ranges(base, windowed)
    assert isinstance(table, KvRangesHeads)
    c = unit_costs(table, 2, 6)
    full_cost = -(-base.Skv // KV_ALIGN) + SEGMENT_COST
    for bh in range(12):
        h = bh % 6
        for qb in range(base.q_blocks):
            assert c[bh][qb] == (_row_cost(base.table[qb]) if windowed[h] else full_cost), (bh, qb)
            assert c[bh][qb] == _row_cost(table.table[h, qb])
    assert min(min(r) for r in c) < full_cost                 # the window is a window
    assert unit_costs(base, 1, 4) == [[_row_cost(base.table[qb]) for qb in range(base.q_blocks)]] * 4      # one table for every head
    with pytest.raises(ValueError, match="built for 6 heads"):
        unit_costs(table, 1, 5)
    with pytest.raises(ValueError, match="KvRanges"):
        unit_costs(base.table, 1, 4)


def _makespan(order, cost, lanes, slots):
    """List scheduling: the order's blocks, split round-robin over `lanes` independent in-order queues (block b on queue b % lanes),
    each queue with `slots` slots; a block starts on the slot that frees first.  Workgroups that exit (-1) cost nothing."""
    worst = 0
    for x in range(lanes):
        free = [0] * slots
        for u in order[x::lanes]:
            if u >= 0:
                t = heapq.heappop(free) + cost(u)
                heapq.heappush(free, t)
        worst = max(worst, max(free))
    return worst


MODEL_TABLES = {"C2": (lambda: frame_window_ranges(13, 1350, 2, prefix=226), 2, 48),
                "C3": (lambda: frame_window_ranges(21, 1560, 5), 3, 40)}
PATTERNS = {"every second head dense": lambda h: h % 2 == 1, "three of four heads windowed": lambda h: h % 4 != 0}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("shape", sorted(MODEL_TABLES))
def test_the_policies_beat_the_natural_order_in_two_scheduling_models(shape, pattern):
    """This pins the policies against a MODEL of the dispatch, not against the GPU: model A is eight independent lanes of 64 slots
    (block b on lane b & 7), model B one in-order pool of 512 slots; real dispatch lies between the two.  On these inputs the
    natural order takes 1.33-1.83 (A) and 1.03-1.09 (B) of the ideal (total cost / 512 slots), both policies <= 1.03 in both."""
    make, B, H = MODEL_TABLES[shape]
    base = make()
    table = head_window_ranges(base, [PATTERNS[pattern](h) for h in range(H)])
    costs = unit_costs(table, B, H)
    Q = base.q_blocks
    cost = lambda u: costs[u // Q][u % Q]
    ideal = sum(sum(r) for r in costs) / 512.0
    span = {}
    for policy in ORDER_POLICIES:
        order = balanced_order(costs, policy, heads=H).order.tolist()
        span[policy] = (_makespan(order, cost, 8, 64), _makespan(order, cost, 1, 512))
        print("%s, %s, %-7s: model A %.3f, model B %.3f of ideal" % (shape, pattern, policy, span[policy][0] / ideal,
                                                                     span[policy][1] / ideal))
    for policy in ("lanes", "units"):
        assert span[policy][0] < span["natural"][0], policy
        assert span[policy][1] <= span["natural"][1], policy
        assert max(span[policy]) <= 1.03 * ideal, policy                  # what README and DESIGN quote
    assert 1.33 <= span["natural"][0] / ideal <= 1.83 and 1.02 <= span["natural"][1] / ideal <= 1.09


def _prototype(name, text):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_exports_and_wrapper_agree_on_the_two_new_entries():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    lib_src = open(os.path.join(ROOT, "alg_amd", "_lib.py")).read()
    strip = lambda a: a.rsplit(" ", 1)[0]                   # the type of an argument
    for name, heads_name, n_args, wrapper, src_file in (
            ("alg_flash_attn_d128_ranges_order", "alg_flash_attn_d128_ranges_heads", 24, "flash_attn_d128_ranges_order",
             "attention128_q64.hip"),
            ("alg_flash_attn_d64_ranges_order", "alg_flash_attn_d64_ranges_heads", 20, "flash_attn_d64_ranges_order", "attention.hip")):
        src = open(os.path.join(ROOT, "alg_amd", "csrc", src_file)).read()
        assert name in alg_amd._lib.EXPORTS and callable(getattr(alg_amd._lib, wrapper))
        declared, defined = _prototype(name, header), _prototype(name, src[src.index('extern "C" int ' + name + "("):])
        assert len(declared) == n_args
        assert [strip(a) for a in declared] == [strip(a) for a in defined], name
        # the arguments of the _heads entry, then the order, then the stream
        assert declared[:-3] == _prototype(heads_name, header)[:-1]
        assert declared[-3:] == ["const int32_t* order", "int order_len", "void* stream"]
        m = re.search(r"lib\.%s\.argtypes = (.*?)\n    lib\." % name, lib_src, re.S)
        ns = {k: getattr(alg_amd._lib, k) for k in ("c_void_p", "c_int", "c_int64", "c_float")}
        assert len(eval(m.group(1), ns)) == n_args, name
        sig = inspect.signature(getattr(alg_amd._lib, wrapper)).parameters
        assert "order" in sig and sig["lse"].default is None and sig["k_off"].default == 0
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if os.path.exists(alg_amd._lib.LIB_PATH):                  # the built library exports both names
        out = subprocess.run(["nm", "-D", "--defined-only", alg_amd._lib.LIB_PATH], capture_output=True, text=True).stdout
        for name in ("alg_flash_attn_d128_ranges_order", "alg_flash_attn_d64_ranges_order"):
            assert re.search(r" T %s$" % name, out, re.M), name


def test_the_wrappers_take_only_a_launch_order_of_the_calls_shape():
    L = alg_amd._lib
    kvr = full_ranges(300, 512)
    good = balanced_order(unit_costs(kvr, 1, 2), "lanes", heads=2)
    args = (None, None, None, None, 1, 2, 300, 512, 0, 0, 0, 0, 0, 0, 0, 0, 1.0)
    with pytest.raises(L.AlgHipError, match="LaunchOrder"):
        L.flash_attn_d128_ranges_order(*args, kvr, good.order)
    with pytest.raises(L.AlgHipError, match=r"built for \(batch, heads, q_blocks\) = \(1, 3, 2\)"):
        L.flash_attn_d128_ranges_order(*args, kvr, balanced_order(unit_costs(kvr, 1, 3), "lanes", heads=3))
    with pytest.raises(L.AlgHipError, match=r"the call has \(1, 2, 2\)"):
        L.flash_attn_d128_ranges_order(*args, kvr, balanced_order(unit_costs(full_ranges(600, 512), 1, 2), "lanes", heads=2))
    with pytest.raises(L.AlgHipError, match="KvRanges"):
        L.flash_attn_d128_ranges_order(*args, kvr.table, good)
    kvr64 = full_ranges(300, 300)
    args64 = (None, None, None, None, 1, 2, 300, 0, 0, 0, 0, 0, 0)
    with pytest.raises(L.AlgHipError, match="LaunchOrder"):
        L.flash_attn_d64_ranges_order(*args64, kvr64, good.order)
    with pytest.raises(L.AlgHipError, match="built for"):
        L.flash_attn_d64_ranges_order(*args64, kvr64, balanced_order(unit_costs(kvr64, 2, 2), "lanes", heads=2))
    with pytest.raises(L.AlgHipError, match="KvRanges"):
        L.flash_attn_d64_ranges_order(*args64, kvr64.table, good)


def test_the_models_and_pipelines_carry_the_switch():
    from alg_amd.attn_window import HeadWindowHost, _balance_policy
    from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    for pipe in (WanImageToVideoPipeline, HunyuanVideoImageToVideoPipeline, CogVideoXImageToVideoPipeline):
        assert inspect.signature(pipe.from_pretrained).parameters["attn_window_balance"].default is False
    host = HeadWindowHost()
    host._head_window_init()
    assert host.attn_window_balance is False and host._attn_orders == {}
    assert [_balance_policy(v) for v in (False, None, 0, True, 1, "lanes", "units")] == [None] * 3 + ["units"] * 2 + ["lanes", "units"]
    for bad in ("natural", "pool", 2, 0.5):
        with pytest.raises(ValueError, match="attn_window_balance must be"):
            _balance_policy(bad)
    # the flag without a recall threshold is refused where the forward would otherwise ignore it
    host.attn_window_balance = True
    with pytest.raises(ValueError, match="needs attn_window_recall > 0"):
        host._head_window_mode(("k",), 1, 1, 2, 256, (1, 256, 256))
    host._attn_orders["x"] = 1
    host.reset_attn_window_heads()
    assert host._attn_orders == {}
    run_py = open(os.path.join(ROOT, "run.py")).read()
    assert "--attn_window_balance" in run_py


WAN = {"model": {"path": "Wan-AI/Wan2.1-I2V-14B-480P-Diffusers", "dtype": "bfloat16"}, "generation": {"height": 480}}
HY = {"model": {"path": "hunyuanvideo-community/HunyuanVideo-I2V", "dtype": "bfloat16"}, "generation": {}}
COG = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}


def test_run_py_parses_the_flag():
    import run
    assert run.make_parser().parse_args([]).attn_window_balance is None
    assert run.make_parser().parse_args(["--attn_window_balance"]).attn_window_balance == "units"
    ns = run.make_parser().parse_args(["--attn_window", "4", "--attn_window_recall", "0.9", "--attn_window_balance", "lanes"])
    assert ns.attn_window_balance == "lanes" and ns.attn_window_recall == 0.9
    with pytest.raises(SystemExit):
        run.make_parser().parse_args(["--attn_window_balance", "pool"])


@pytest.mark.parametrize("config,kw", [
    (WAN, dict(attn_window_balance="lanes")),                              # without --attn_window_recall
    (HY, dict(attn_window=4, attn_window_balance="units")),
    (COG, dict(attn_window_balance="lanes")),                              # wired for the head_dim 128 models, like its siblings
])
def test_run_py_refusals_name_the_flag(config, kw):
    import argparse

    import run
    base = dict(fp8=False, fp8_attention=False, attn_window=0, attn_window_recall=0.0, step_cache=0.0, synthetic=True,
                model_cache_dir=None)
    base.update(kw)
    with pytest.raises(SystemExit, match="--attn_window_balance"):
        run.build_pipeline(config, argparse.Namespace(**base), "cuda")


@pytest.mark.parametrize("family", ["wan", "hunyuan", "cogvideox"])
def test_from_pretrained_refuses_the_flag_without_a_recall_threshold(family):
    from alg_amd.pipeline_cogvideox_image2video_lowpass import CogVideoXImageToVideoPipeline
    from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
    from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
    pipe = {"wan": WanImageToVideoPipeline, "hunyuan": HunyuanVideoImageToVideoPipeline, "cogvideox": CogVideoXImageToVideoPipeline}[family]
    with pytest.raises(ValueError, match="needs attn_window_recall > 0"):
        pipe.from_pretrained("/nonexistent", attn_window=2, attn_window_balance=True)
    with pytest.raises(ValueError, match="attn_window_balance must be"):
        pipe.from_pretrained("/nonexistent", attn_window=2, attn_window_recall=0.5, attn_window_balance="pool")


def test_a_capture_never_builds_an_order(monkeypatch):
    """An order that is not cached yet would have to be uploaded: inside a stream capture that is refused, not done."""
    from alg_amd.attn_window import HeadWindowHost
    host = HeadWindowHost()
    host._head_window_init()
    host.attn_window_balance = "lanes"
    table = head_window_ranges(frame_window_ranges(6, 160, 1), [True, False])
    monkeypatch.setattr(alg_amd._lib, "_capturing", lambda: True)
    with pytest.raises(alg_amd._lib.AlgHipError, match="cannot be captured"):
        host._layer_order(table, 2)
    assert host._attn_orders == {} and host.attn_window_order_build_seconds == 0.0
    host.attn_window_balance = False
    assert host._layer_order(table, 2) is None
