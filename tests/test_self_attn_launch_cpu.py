"""The self-attention launch ladder the three DiTs share (attn_window.launch_self_attention, calibrate_self_attention,
SelfAttnOperands, HeadWindowHost._window_table / _profile_table / _self_attn_begin), without a device or the library: the _lib
wrappers are recorders, the tables hand-made for Sq = Skv = 512 and two heads, the calibration buffers CPU tensors.  Every rung is
held to the wrapper, the positional tuple, the keywords and the offsets the models' own ladders spelled before they were merged."""
from types import SimpleNamespace

import pytest
import torch

from alg_amd import _lib
from alg_amd.attn_window import (HeadWindowHost, KvRanges, KvRangesHeads, KvSegments, LaunchOrder, SelfAttnOperands, balanced_order,
                                 calibrate_self_attention, frame_profile_segments, frame_window_ranges, full_ranges,
                                 head_window_ranges, launch_self_attention, unit_costs)

S, HEADS, SCALE = 512, 2, 0.125
WRAPPERS = [f"flash_attn_d{d}{s}" for d in (64, 128) for s in ("", "_ranges", "_ranges_heads", "_ranges_order")] + [
    "flash_attn_d128_ranges_prefix", "attn_lse_recall", "attn_prefix_mass"]

SHARED = frame_window_ranges(4, 128, 0)                    # 4 frames of 128 tokens, window 0, one sink frame: two query blocks
PER_HEAD = head_window_ranges(SHARED, [True, False])
FULL = full_ranges(S, S)
SEGMENTS = frame_profile_segments(4, 128, (1,))            # one width: 2 * 1 + 3 = 5 segments
QK, VT, ATT = torch.zeros(1), torch.zeros(2), torch.zeros(3)     # told apart by identity


def test_the_tables_are_what_the_rungs_are_keyed_on():
    assert type(SHARED) is KvRanges and type(PER_HEAD) is KvRangesHeads and type(SEGMENTS) is KvSegments and SEGMENTS.segments == 5
    assert (SHARED.Sq, SHARED.Skv, PER_HEAD.heads, FULL.is_full) == (S, S, HEADS, True)


@pytest.fixture
def calls(monkeypatch):
    """[(profile key, wrapper name, positionals, keywords)] of every launch made through `timed` below."""
    log = []
    for name in WRAPPERS:
        monkeypatch.setattr(_lib, name, lambda *a, _name=name, **kw: log.append((_name, a, kw)))
    return log


def timed(key, fn, *a, **kw):
    fn(*a, **kw)
    timed.keys.append(key)


@pytest.fixture(autouse=True)
def _keys():
    timed.keys = []


def ops128(batch=2, **offs):
    """Wan's record for dim 256 (batch 2), or with offs one HunyuanVideo sample's (batch 1, output rows 768 wide)."""
    o_bs, o_rs = (S * 768, 768) if offs else (S * 256, 256)
    return SelfAttnOperands(128, QK, QK, VT, ATT, batch, HEADS, S, S, S * 512, 512, S * 512, 512, 256 * S, S, o_bs, o_rs, SCALE,
                            **(offs or dict(k_off=256)))


POS128 = (QK, QK, VT, ATT, 2, 2, 512, 512, 262144, 512, 262144, 512, 131072, 512, 131072, 256, SCALE)
OFFS128 = dict(q_off=0, k_off=256, vt_off=0, o_off=0)
HY_OFFS = dict(q_off=262144, k_off=262400, vt_off=131072, o_off=393216)       # sample 1 of J = 512 joint rows
POS_HY = (QK, QK, VT, ATT, 1, 2, 512, 512, 262144, 512, 262144, 512, 131072, 512, 393216, 768, SCALE)


def ops64():
    """CogVideoX's record for inner_dim 128."""
    return SelfAttnOperands(64, QK, QK, VT, ATT, 2, HEADS, S, S, S * 256, 256, S * 256, 256, 128 * S, S, S * 128, 128, SCALE, k_off=128,
                            q_prescaled=True)


POS64 = (QK, QK, VT, ATT, 2, 2, 512, 131072, 256, 65536, 512, 65536, 128)
OFFS64 = dict(q_off=0, k_off=128)


def test_the_two_expansions():
    assert ops128().args() == (POS128, OFFS128) and len(POS128) == 17
    assert ops128(1, **HY_OFFS).args() == (POS_HY, HY_OFFS)
    assert ops64().args() == (POS64, OFFS64) and len(POS64) == 13


@pytest.mark.parametrize("ops, pos, offs, d", [(ops128(), POS128, OFFS128, 128), (ops128(1, **HY_OFFS), POS_HY, HY_OFFS, 128),
                                               (ops64(), POS64, OFFS64, 64)], ids=["wan", "hunyuan", "cogvideox"])
def test_every_rung_of_the_ladder(calls, ops, pos, offs, d):
    order = balanced_order(unit_costs(PER_HEAD, ops.batch, HEADS), "units", heads=HEADS)
    assert type(order) is LaunchOrder and order.batch == ops.batch
    at = len(pos)                                                               # the table's position: 17 (d = 128), 13 (d = 64)
    launch_self_attention(timed, "k0", ops, PER_HEAD, order)
    launch_self_attention(timed, "k1", ops, PER_HEAD)
    launch_self_attention(timed, "k2", ops, SHARED)
    launch_self_attention(timed, "k3", ops, None)
    dense = (pos, offs) if d == 128 else (pos + (SCALE,), dict(offs, q_prescaled=True))
    assert calls == [("flash_attn_d%d_ranges_order" % d, pos + (PER_HEAD, order), offs),
                     ("flash_attn_d%d_ranges_heads" % d, pos + (PER_HEAD,), offs),
                     ("flash_attn_d%d_ranges" % d, pos + (SHARED,), offs),
                     ("flash_attn_d%d" % d,) + dense]
    assert calls[0][1][at] is PER_HEAD and calls[0][1][at + 1] is order and calls[1][1][at] is PER_HEAD and calls[2][1][at] is SHARED
    assert all("lse" not in kw and "lse_off" not in kw for _, _, kw in calls)    # the tests' stand-ins take neither
    assert timed.keys == ["k0", "k1", "k2", "k3"]


def test_the_wrappers_are_looked_up_at_call_time(calls, monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "flash_attn_d128_ranges_heads", lambda *a, **kw: seen.append((a[17], kw.get("lse"))))
    launch_self_attention(timed, "k", ops128(), PER_HEAD)
    assert seen == [(PER_HEAD, None)] and not calls


def two_launch_buffers():
    return SimpleNamespace(widths=None, lse_full=torch.zeros(4), lse_part=torch.zeros(5), o=torch.zeros(6), recall=torch.zeros(7))


@pytest.mark.parametrize("sample0", [0, 1])
def test_two_launch_calibration_of_one_hunyuan_sample(calls, sample0):
    """layer 3, sample `sample0` of 2: lse 2 heads x 512 rows per sample, scratch rows 2 x 128 wide, recall slot 3 * 2 + sample0."""
    cal = two_launch_buffers()
    calibrate_self_attention(timed, "attn_self", ops128(1, **HY_OFFS), cal, 3, 2, sample0, (0, 384), FULL, SHARED)
    lse_off, o_off, out_off = (0, 0, 12) if sample0 == 0 else (1024, 131072, 14)
    scratch = POS_HY[:3] + (cal.o,) + POS_HY[4:14] + (131072, 256, SCALE)
    assert calls == [("flash_attn_d128_ranges_heads", POS_HY + (FULL,), dict(HY_OFFS, lse=cal.lse_full, lse_off=lse_off)),
                     ("flash_attn_d128_ranges_heads", scratch + (SHARED,), dict(HY_OFFS, o_off=o_off, lse=cal.lse_part, lse_off=lse_off)),
                     ("attn_lse_recall", (cal.lse_part, cal.lse_full, cal.recall, 2, 512),
                      dict(row0=0, rows=384, part_off=lse_off, full_off=lse_off, out_off=out_off))]
    assert calls[0][1][17] is FULL and calls[0][2]["lse"] is cal.lse_full and calls[1][1][3] is cal.o and calls[1][2]["lse"] is cal.lse_part
    assert timed.keys == ["attn_self", "attn_calib", "attn_calib"]


def test_two_launch_calibration_of_a_wan_block(calls):
    """The whole batch of 2 at once: 4 panels, every row, recall slot 3 * 2 * 2 heads."""
    cal = two_launch_buffers()
    calibrate_self_attention(timed, "attn_self", ops128(), cal, 3, 2, 0, (0, S), FULL, SHARED)
    assert calls == [("flash_attn_d128_ranges_heads", POS128 + (FULL,), dict(OFFS128, lse=cal.lse_full, lse_off=0)),
                     ("flash_attn_d128_ranges_heads", POS128[:3] + (cal.o,) + POS128[4:] + (SHARED,),
                      dict(OFFS128, lse=cal.lse_part, lse_off=0)),
                     ("attn_lse_recall", (cal.lse_part, cal.lse_full, cal.recall, 4, 512),
                      dict(row0=0, rows=512, part_off=0, full_off=0, out_off=12))]


def test_two_launch_calibration_of_a_cogvideox_block(calls):
    """d = 64: the recall over the latent-query rows [T, S) behind T = 64 prompt tokens; profile key "attn"."""
    cal = two_launch_buffers()
    calibrate_self_attention(timed, "attn", ops64(), cal, 3, 2, 0, (64, S - 64), FULL, SHARED)
    assert calls == [("flash_attn_d64_ranges_heads", POS64 + (FULL,), dict(OFFS64, lse=cal.lse_full, lse_off=0)),
                     ("flash_attn_d64_ranges_heads", POS64[:3] + (cal.o,) + POS64[4:] + (SHARED,),
                      dict(OFFS64, lse=cal.lse_part, lse_off=0)),
                     ("attn_lse_recall", (cal.lse_part, cal.lse_full, cal.recall, 4, 512),
                      dict(row0=64, rows=448, part_off=0, full_off=0, out_off=12))]
    assert calls[0][1][13] is FULL and timed.keys == ["attn", "attn_calib", "attn_calib"]


@pytest.mark.parametrize("sample0", [0, 1])
def test_one_pass_calibration_of_one_hunyuan_sample(calls, sample0):
    """prefix: 2 heads x 5 segments x 512 rows per sample; mass slot (3 * 2 + sample0) x 2 heads x 5 segments."""
    cal = SimpleNamespace(widths=(1,), segments=5, prefix=torch.zeros(4), mass=torch.zeros(5))
    calibrate_self_attention(timed, "attn_self", ops128(1, **HY_OFFS), cal, 3, 2, sample0, (0, 384), None, SEGMENTS)
    prefix_off, out_off = (0, 60) if sample0 == 0 else (5120, 70)
    assert calls == [("flash_attn_d128_ranges_prefix", POS_HY + (SEGMENTS, cal.prefix), dict(HY_OFFS, prefix_off=prefix_off)),
                     ("attn_prefix_mass", (cal.prefix, cal.mass, 2, 5, 512),
                      dict(row0=0, rows=384, prefix_off=prefix_off, out_off=out_off))]
    assert calls[0][1][17] is SEGMENTS and calls[0][1][18] is cal.prefix and calls[0][1][3] is ATT      # into the REAL output
    assert timed.keys == ["attn_self", "attn_calib"]


def test_one_pass_calibration_of_a_wan_block(calls):
    cal = SimpleNamespace(widths=(1,), segments=5, prefix=torch.zeros(4), mass=torch.zeros(5))
    calibrate_self_attention(timed, "attn_self", ops128(), cal, 3, 2, 0, (0, S), None, SEGMENTS)
    assert calls == [("flash_attn_d128_ranges_prefix", POS128 + (SEGMENTS, cal.prefix), dict(OFFS128, prefix_off=0)),
                     ("attn_prefix_mass", (cal.prefix, cal.mass, 4, 5, 512), dict(row0=0, rows=512, prefix_off=0, out_off=60))]


def test_the_d64_record_refuses_what_its_wrappers_cannot_say():
    good = ops64()
    with pytest.raises(AssertionError):
        SelfAttnOperands(*good._replace(Skv=S + 64))                                             # Sq != Skv
    with pytest.raises(AssertionError):
        SelfAttnOperands(*good._replace(k_rs=128))                                               # K strides are Q's
    with pytest.raises(AssertionError):
        SelfAttnOperands(*good._replace(k_bs=S * 128))
    for off in ("vt_off", "o_off"):
        with pytest.raises(AssertionError):
            SelfAttnOperands(*good._replace(**{off: 64}))
    with pytest.raises(AssertionError):
        SelfAttnOperands(*ops128()._replace(q_prescaled=True))                                  # the d = 128 wrappers have no such flag
    with pytest.raises(AssertionError):
        SelfAttnOperands(*good._replace(head_dim=96))


class _Host(HeadWindowHost):
    device, profile = "cpu", None

    def __init__(self, **kw):
        self.attn_window, self.attn_sink_frames = 1, 1
        self._head_window_init()
        self.__dict__.update(kw)


@pytest.fixture
def uploads(monkeypatch):
    """Every table class's upload, stubbed: the list of tables `on` was asked for."""
    log = []
    for cls in (KvRanges, KvRangesHeads, KvSegments, LaunchOrder):
        monkeypatch.setattr(cls, "on", lambda self, device: log.append(self))
    return log


def test_window_table_validates_builds_uploads_and_caches_once(uploads):
    host = _Host()
    t = host._window_table(4, 128)
    assert type(t) is KvRanges and host._window_table(4, 128) is t and uploads == [t] and list(host._attn_ranges) == [(4, 128, 1, 1)]
    assert torch.equal(t.table, frame_window_ranges(4, 128, 1, sink_frames=1).table)
    cog = host._window_table(4, 128, (64,), prefix=64)                           # CogVideoX: T prompt tokens first
    assert torch.equal(cog.table, frame_window_ranges(4, 128, 1, prefix=64).table) and (4, 128, 64, 1, 1) in host._attn_ranges
    hy = host._window_table(4, 128, (20, 532), tail=(512, 532), rows=532)        # HunyuanVideo: 20 valid prompt keys behind
    assert torch.equal(hy.table, frame_window_ranges(4, 128, 1, tail=(512, 532), rows=532).table)
    assert (4, 128, 20, 532, 1, 1) in host._attn_ranges and uploads == [t, cog, hy]
    narrow = host._window_table(4, 128, window=0)                                # one of attn_window_widths
    assert narrow is not t and narrow.coverage < t.coverage and host._window_table(4, 128, window=0) is narrow
    host.attn_sink_frames = 0                                                    # a changed sink builds a new table
    assert host._window_table(4, 128) is not t and (4, 128, 1, 0) in host._attn_ranges
    host.attn_window = 9                                                         # covers the video: the dense attention, cached as such
    n = len(uploads)
    assert host._window_table(4, 128) is None and (4, 128, 9, 0) in host._attn_ranges and len(uploads) == n
    assert host._window_table(4, 128, (64,), prefix=64) is not cog               # (the window is part of the key)


def test_window_table_refuses_a_negative_window_or_sink(uploads):
    with pytest.raises(ValueError, match=r"attn_window and attn_sink_frames must be >= 0 \(got -1, 1\)"):
        _Host(attn_window=-1)._window_table(4, 128)
    with pytest.raises(ValueError, match=r"attn_window and attn_sink_frames must be >= 0 \(got 1, -2\)"):
        _Host(attn_sink_frames=-2)._window_table(4, 128)
    with pytest.raises(ValueError, match=r"attn_window and attn_sink_frames must be >= 0 \(got 1, -2\)"):
        _Host(attn_sink_frames=-2)._profile_table(4, 128, (1,))
    assert not uploads


def test_profile_table_caches_once(uploads):
    host = _Host()
    p = host._profile_table(4, 128, (1,))
    assert type(p) is KvSegments and host._profile_table(4, 128, (1,)) is p and uploads == [p]
    assert list(host._attn_ranges) == [("profile", 4, 128, (1,), 1)] and torch.equal(p.table, SEGMENTS.table)
    hy = host._profile_table(4, 128, (1,), (20, 532), tail=(512, 532), rows=532)
    assert ("profile", 4, 128, 20, 532, (1,), 1) in host._attn_ranges and (hy.Sq, hy.Skv) == (532, 532)


def test_the_plan_resolves_a_layers_table_and_order(uploads):
    host = _Host()
    off = host._self_attn_begin([None], ("k",), 2, 1, HEADS, S, (1, S, 256), 1)
    assert (off.mode, off.cal, off.layer(0)) == (None, None, (None, None))
    off.finish()                                                                 # nothing to end
    shared = host._window_table(4, 128)
    plan = host._self_attn_begin([shared], ("k",), 2, 1, HEADS, S, (1, S, 256), 1)
    assert plan.mode is None and plan.layer(1) == (shared, None)                 # attn_window_recall 0: the shared window
    host.attn_window_recall = 0.9
    plan = host._self_attn_begin([shared], ("k",), 2, 1, HEADS, S, (1, S, 256), 1)
    assert plan.mode == "dense" and plan.layer(1) == (None, None)                # not calibrated yet
    host._attn_decided = ((("k",), 0.9), [(True, True), (True, False)])
    plan = host._self_attn_begin([shared], ("k",), 2, 1, HEADS, S, (1, S, 256), 1)
    assert plan.mode == "tables" and plan.layer(0) == (shared, None)
    table, order = plan.layer(1)
    assert type(table) is KvRangesHeads and order is None and plan.layer(1)[0] is table
    host.attn_window_balance = "units"
    table2, order = plan.layer(1)
    assert table2 is table and type(order) is LaunchOrder and (order.batch, order.heads) == (1, HEADS) and plan.layer(1)[1] is order
