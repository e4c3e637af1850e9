"""Frame-window self-attention for the video DiTs (opt-in, an extension of this port: the reference attends to all keys).

The primitives are alg_flash_attn_d128_ranges (Wan, HunyuanVideo; attention128_q64.hip) and alg_flash_attn_d64_ranges (CogVideoX;
attention.hip), both in include/alg_hip.h: each block of 256 queries attends to a short list of key ranges, exactly (a masked
softmax with the dense kernel's numerics).  The tokens of a video latent are laid out frame by frame, so "the frames f - W ..
f + W" is ONE contiguous run of keys, and the frame window is a host-side policy on top of the primitives:

    KvRanges             a validated table of key ranges, uploaded once; the only thing _lib.flash_attn_d128_ranges and
                         _lib.flash_attn_d64_ranges take
    frame_window_ranges  the policy: conditioning frames (sink) + the frames within `window` of the block's own + the prompt
    ranges_to_mask       the table as a boolean [Sq, Skv] mask (tests, records)

Per-head windows chosen by recall (head_dim 128: alg_flash_attn_d128_ranges_heads; head_dim 64: alg_flash_attn_d64_ranges_heads;
both reduced by alg_attn_lse_recall).  A frame window is nearly
exact for a head whose softmax mass lies in neighbouring frames and wrong for one that spreads it over the video, so with
`attn_window_recall` > 0 the models measure, on one forward of each video, the RECALL of every (layer, head) -- the fraction of
softmax mass its latent queries keep inside the window -- and only the heads that reach the threshold keep the window:

    KvRangesHeads        one validated KvRanges per head, as ONE device table [heads][q_blocks][max_ranges][2]
    head_window_ranges   the window's rows for the windowed heads, the one full range for the others
    decide_heads         recall [samples][heads] -> windowed [heads]: the minimum over the samples reaches the threshold

A launch order balanced by coverage (alg_flash_attn_d128_ranges_order, alg_flash_attn_d64_ranges_order; `attn_window_balance`).  A
layer with dense and windowed heads holds units (head, query block) of very different cost, and the kernels' own order deals heads
to the eight dispatch lanes by bh % 8, head-major.  The launch can take a static order instead, computed here once per table:

    LaunchOrder          a validated order, uploaded once; the only thing the _order wrappers of _lib take
    unit_costs           key tiles (+ SEGMENT_COST per range) of every unit of a table
    balanced_order       "lanes" (heads whole to the least loaded lane, long units first), "units", "natural"

Every workgroup computes what it computed before, so the output is bit-identical for every order.

The window WIDTH per head from one calibration pass (head_dim 128: alg_flash_attn_d128_ranges_prefix, reduced by
alg_attn_prefix_mass; `attn_window_widths`).  The ranged kernel runs a block's key ranges one after the other, so a launch over ALL
keys, cut into nested rings around the block's own frames, yields the forward's attention output AND the softmax mass inside every
candidate width; a head then takes the narrowest width that reaches the recall, else it stays dense:

    KvSegments              a validated partition of [0, Skv) into up to 12 segments per block (the launch is the dense attention)
    frame_profile_segments  the rings: sink | far left | left rings | core | right rings | far right | tail
    width_segments          which segments count for which width
    decide_widths           recall [samples][heads][widths] -> the width per head (0: dense)
    head_width_ranges       the window's rows at each head's own width

The position-major BAND for heads that look at the same spatial position in every frame (Wan attn1; `attn_band`).  In the
frame-major order s = f hw + p such a head's keys are hw tokens apart; in the position-major order p F + f they are one run per
query block, so a band head runs alg_flash_attn_d128_ranges on position-major copies of its Q, K and V^T
(alg_attn_rows_position_major, alg_attn_vt_position_major: attn_layout.hip) and its output is scattered back:

    position_major_index    the permutation pi(f hw + p) = p F + f
    position_band_ranges    the policy: one range per block, every frame of the positions within `band` of the block's own
    HeadList                validated, device-resident head indices: the only thing the layout wrappers of _lib take
    decide_layouts          per head "window" | "band" | "dense": the cheaper of the candidates that reach the recall
    head_layout_ranges      the main launch's per-head table, band heads ABSENT from it (KvRanges(..., absent_ok=True))

Only the policy is an approximation; its visual quality on a trained checkpoint is unmeasured (README), so it is off by default.
"""
import math
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

MAX_SEGMENTS = 12  # alg_flash_attn_d128_ranges_prefix: segments per block of a KvSegments
Q_BLOCK = 256      # queries per workgroup of attention128_q64.hip and of attention.hip
KV_ALIGN = 64      # their key tile: a range begins on the dense kernel's tile grid
MAX_RANGES = 4
LANES = 8          # workgroups b with the same b % 8 share a dispatch lane (an XCD, as observed: the kernels' bh % 8 rule)
SEGMENT_COST = 2   # cost of a key range beyond its tiles, in key tiles: see unit_costs
ORDER_POLICIES = ("lanes", "units", "natural")


class KvRanges:
    """A table int32 [q_blocks][max_ranges][2] of (begin, end) key indices for Sq queries and Skv keys, validated on the CPU:
    in each block the used entries come first, sorted and disjoint, begin % 64 == 0, begin < end <= Skv, unused trailing entries
    are (0, 0), and every block has at least one key.  ValueError names the block and the rule.

    absent_ok=True (opt-in: a head that another launch computes, see head_layout_ranges) also takes the table whose EVERY entry is
    (0, 0): `absent` is then True and the coverage 0; the kernels write zeros and do no other work for such a head.  A table
    with some blocks empty and others not stays an error.

    empty_ok=True (opt-in: the FAR table of the far-field reuse, see complement_ranges) takes blocks without a key next to blocks
    with keys: the kernels write zeros and an lse of -inf for such a block's rows."""

    def __init__(self, table, Skv, Sq, absent_ok=False, empty_ok=False):
        t = torch.as_tensor(table)
        if t.dtype != torch.int32 or t.dim() != 3 or t.shape[2] != 2 or t.device.type != "cpu":
            raise ValueError("KvRanges takes a CPU int32 table [q_blocks][max_ranges][2], got %s %s" % (t.dtype, tuple(t.shape)))
        Skv, Sq = int(Skv), int(Sq)
        if Sq < 1 or Skv < 1:
            raise ValueError("KvRanges needs Sq >= 1 and Skv >= 1 (got %d, %d)" % (Sq, Skv))
        q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
        if t.shape[0] != q_blocks:
            raise ValueError("the table has %d blocks, Sq=%d needs ceil(Sq / %d) = %d" % (t.shape[0], Sq, Q_BLOCK, q_blocks))
        if not 1 <= t.shape[1] <= MAX_RANGES:
            raise ValueError("max_ranges must be 1..%d, got %d" % (MAX_RANGES, t.shape[1]))
        a = t.numpy().astype(np.int64)
        visited = 0
        self.absent = bool(absent_ok) and not a.any()
        for j in range(0 if self.absent else q_blocks):
            prev_end, unused_seen = None, False
            for i in range(a.shape[1]):
                b, e = int(a[j, i, 0]), int(a[j, i, 1])
                if b == 0 and e == 0:
                    unused_seen = True
                    continue
                if unused_seen:
                    raise ValueError("block %d: used entry %d (%d, %d) behind an unused one (used entries come first)" % (j, i, b, e))
                if b % KV_ALIGN:
                    raise ValueError("block %d: begin %d of entry %d is not a multiple of %d" % (j, b, i, KV_ALIGN))
                if not 0 <= b < e:
                    raise ValueError("block %d: entry %d (%d, %d) needs 0 <= begin < end" % (j, i, b, e))
                if e > Skv:
                    raise ValueError("block %d: end %d of entry %d is beyond Skv = %d" % (j, e, i, Skv))
                if prev_end is not None and b < prev_end:
                    raise ValueError("block %d: entry %d (%d, %d) is not sorted behind / overlaps the entry ending at %d"
                                     % (j, i, b, e, prev_end))
                prev_end = e
                visited += (e - b) * min(Q_BLOCK, Sq - j * Q_BLOCK)
            if prev_end is None and not empty_ok:
                raise ValueError("block %d: no key (every block needs at least one range)" % j)
        self.table = t.clone().contiguous()
        self.Skv, self.Sq = Skv, Sq
        self.q_blocks, self.max_ranges = q_blocks, int(t.shape[1])
        self.coverage = visited / float(Sq * Skv)   # visited (query, key) pairs / all pairs; a block's queries share its ranges
        self._device = {}

    def on(self, device):
        """The table on `device`, uploaded once per device (outside any stream capture: the models build their tables before
        the first launch that uses them)."""
        device = torch.device(device)
        dev = torch.cuda.current_device() if device.index is None else device.index
        t = self._device.get(dev)
        if t is None:
            t = self._device[dev] = self.table.to(torch.device("cuda", dev))
        return t

    @property
    def device_table(self):
        """The table on the current device."""
        return self.on("cuda")

    @property
    def is_full(self):
        a = self.table
        return bool((a[:, 0, 0] == 0).all() and (a[:, 0, 1] == self.Skv).all())


class KvRangesHeads:
    """A table int32 [heads][q_blocks][max_ranges][2]: head h's slice is a KvRanges table for (Sq, Skv) and is validated as one
    (ValueError names the head in front of KvRanges' message).  What _lib.flash_attn_d128_ranges_heads takes for table_heads =
    heads, and _lib.flash_attn_d64_ranges_heads for Sq == Skv.  absent_ok: as in KvRanges, per head."""

    def __init__(self, table, Skv, Sq, absent_ok=False):
        t = torch.as_tensor(table)
        if t.dtype != torch.int32 or t.dim() != 4 or t.shape[0] < 1 or t.device.type != "cpu":
            raise ValueError("KvRangesHeads takes a CPU int32 table [heads][q_blocks][max_ranges][2], got %s %s"
                             % (t.dtype, tuple(t.shape)))
        per_head = []
        for h in range(t.shape[0]):
            try:
                per_head.append(KvRanges(t[h], Skv, Sq, absent_ok=absent_ok))
            except ValueError as e:
                raise ValueError("head %d: %s" % (h, e)) from None
        self.per_head = tuple(per_head)
        self.table = t.clone().contiguous()
        self.heads = int(t.shape[0])
        self.Skv, self.Sq = per_head[0].Skv, per_head[0].Sq
        self.q_blocks, self.max_ranges = per_head[0].q_blocks, per_head[0].max_ranges
        self.coverage = sum(r.coverage for r in per_head) / self.heads
        self._device = {}

    on = KvRanges.on
    device_table = KvRanges.device_table


class KvSegments:
    """A table int32 [q_blocks][segments][2] of (begin, end) key indices whose non-empty entries PARTITION [0, Skv) in every
    block, validated on the CPU: 1 <= segments <= 12; an entry with end <= begin is empty and may stand anywhere; the non-empty
    entries of a block are ascending and disjoint, begin % 64 == 0, begin < end <= Skv, and together they cover [0, Skv) exactly
    once -- so a launch over the table IS the dense attention, and the segment index means what the builder says in every block.
    ValueError names the block and the rule.  The only table _lib.flash_attn_d128_ranges_prefix takes besides KvRanges(Heads)."""

    def __init__(self, table, Skv, Sq):
        t = torch.as_tensor(table)
        if t.dtype != torch.int32 or t.dim() != 3 or t.shape[2] != 2 or t.device.type != "cpu":
            raise ValueError("KvSegments takes a CPU int32 table [q_blocks][segments][2], got %s %s" % (t.dtype, tuple(t.shape)))
        Skv, Sq = int(Skv), int(Sq)
        if Sq < 1 or Skv < 1:
            raise ValueError("KvSegments needs Sq >= 1 and Skv >= 1 (got %d, %d)" % (Sq, Skv))
        q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
        if t.shape[0] != q_blocks:
            raise ValueError("the table has %d blocks, Sq=%d needs ceil(Sq / %d) = %d" % (t.shape[0], Sq, Q_BLOCK, q_blocks))
        if not 1 <= t.shape[1] <= MAX_SEGMENTS:
            raise ValueError("segments must be 1..%d, got %d" % (MAX_SEGMENTS, t.shape[1]))
        a = t.numpy().astype(np.int64)
        for j in range(q_blocks):
            covered = 0        # the non-empty entries so far cover [0, covered)
            for i in range(a.shape[1]):
                b, e = int(a[j, i, 0]), int(a[j, i, 1])
                if e <= b:
                    continue
                if b % KV_ALIGN:
                    raise ValueError("block %d: begin %d of entry %d is not a multiple of %d" % (j, b, i, KV_ALIGN))
                if b < 0:
                    raise ValueError("block %d: entry %d (%d, %d) needs 0 <= begin < end" % (j, i, b, e))
                if e > Skv:
                    raise ValueError("block %d: end %d of entry %d is beyond Skv = %d" % (j, e, i, Skv))
                if b < covered:
                    raise ValueError("block %d: entry %d (%d, %d) is not sorted behind / overlaps the entry ending at %d"
                                     % (j, i, b, e, covered))
                if b > covered:
                    raise ValueError("block %d: the keys [%d, %d) in front of entry %d are in no segment (the entries partition "
                                     "[0, Skv))" % (j, covered, b, i))
                covered = e
            if covered != Skv:
                raise ValueError("block %d: the keys [%d, %d) are in no segment (the entries partition [0, Skv))" % (j, covered, Skv))
        self.table = t.clone().contiguous()
        self.Skv, self.Sq = Skv, Sq
        self.q_blocks, self.segments = q_blocks, int(t.shape[1])
        self.max_ranges = self.segments
        self.coverage = 1.0
        self._device = {}

    on = KvRanges.on
    device_table = KvRanges.device_table


class LaunchOrder:
    """A launch order for the ranged attention entries: a CPU int32 vector whose entry b is the unit bh * q_blocks + qb that
    workgroup b runs, or -1 for a workgroup that exits.  Validated on the CPU: the length is a multiple of 8, every unit in
    [0, batch * heads * q_blocks) occurs exactly once, every other entry is -1.  ValueError names the rule and the first
    offending entry."""

    def __init__(self, order, batch, heads, q_blocks):
        t = torch.as_tensor(order)
        if t.dtype != torch.int32 or t.dim() != 1 or t.device.type != "cpu":
            raise ValueError("LaunchOrder takes a CPU int32 vector, got %s %s" % (t.dtype, tuple(t.shape)))
        batch, heads, q_blocks = int(batch), int(heads), int(q_blocks)
        if batch < 1 or heads < 1 or q_blocks < 1:
            raise ValueError("LaunchOrder needs batch, heads, q_blocks >= 1 (got %d, %d, %d)" % (batch, heads, q_blocks))
        n, units = int(t.numel()), batch * heads * q_blocks
        if n == 0 or n % LANES:
            raise ValueError("the order's length %d is not a multiple of %d" % (n, LANES))
        a = t.numpy().astype(np.int64)
        bad = np.nonzero((a < -1) | (a >= units))[0]
        if bad.size:
            raise ValueError("entry %d is %d: out of range (a unit in [0, %d) or -1)" % (bad[0], a[bad[0]], units))
        at = np.nonzero(a >= 0)[0]                       # the entries that hold a unit, in entry order
        count = np.bincount(a[at], minlength=units)
        if (count > 1).any():
            _, first = np.unique(a[at], return_index=True)            # the first entry of every unit
            again = np.setdiff1d(np.arange(at.size), first)
            i = at[again[0]]
            raise ValueError("entry %d: duplicate unit %d (first at entry %d; every unit occurs exactly once)"
                             % (i, a[i], at[np.nonzero(a[at] == a[i])[0][0]]))
        missing = np.nonzero(count == 0)[0]
        if missing.size:
            raise ValueError("missing unit %d (bh %d, q block %d): every unit in [0, %d) occurs exactly once"
                             % (missing[0], missing[0] // q_blocks, missing[0] % q_blocks, units))
        self.order = t.clone().contiguous()
        self.batch, self.heads, self.q_blocks = batch, heads, q_blocks
        self._device = {}

    def on(self, device):
        """The order on `device`, uploaded once per device (outside any stream capture, like KvRanges.on)."""
        device = torch.device(device)
        dev = torch.cuda.current_device() if device.index is None else device.index
        t = self._device.get(dev)
        if t is None:
            t = self._device[dev] = self.order.to(torch.device("cuda", dev))
        return t

    @property
    def device_table(self):
        """The order on the current device."""
        return self.on("cuda")

    def __len__(self):
        return int(self.order.numel())


def unit_costs(kv_ranges, batch, heads):
    """The cost [batch * heads][q_blocks] (a list of lists of ints) of every unit of a launch with the table `kv_ranges`, a
    KvRanges (one table for every head) or a KvRangesHeads built for `heads`: for the unit's table row the sum over its used
    ranges of ceil((end - begin) / 64) key tiles, plus SEGMENT_COST per used range.

    SEGMENT_COST (2 tiles) stands for what a range costs beyond its steady-state tiles -- priming the ring and the C++ tile 0.
    Nobody has measured it.  Only the ORDER that results from the costs matters (balanced_order sorts and sums them), not their
    scale, and a range is a small part of a unit wherever the window is worth having."""
    if isinstance(kv_ranges, KvRangesHeads):
        if kv_ranges.heads != int(heads):
            raise ValueError("unit_costs: the table was built for %d heads, the launch has %d" % (kv_ranges.heads, heads))
    elif not isinstance(kv_ranges, KvRanges):
        raise ValueError("unit_costs takes a KvRanges or a KvRangesHeads, got %s" % type(kv_ranges).__name__)
    if int(batch) < 1 or int(heads) < 1:
        raise ValueError("unit_costs needs batch >= 1 and heads >= 1 (got %d, %d)" % (batch, heads))
    a = kv_ranges.table.numpy().astype(np.int64)          # [q_blocks][max_ranges][2], or with a leading head dimension
    used = a[..., 1] > a[..., 0]
    tiles = (a[..., 1] - a[..., 0] + KV_ALIGN - 1) // KV_ALIGN
    per_head = ((tiles + SEGMENT_COST) * used).sum(axis=-1)          # [q_blocks] or [heads][q_blocks]
    if per_head.ndim == 1:
        per_head = np.broadcast_to(per_head, (int(heads), per_head.shape[0]))
    return np.tile(per_head, (int(batch), 1)).tolist()               # row bh = b * heads + h


def balanced_order(costs, policy="lanes", heads=None):
    """A LaunchOrder for units of cost costs[bh][qb] (unit_costs), laid out so that entry b belongs to lane b & 7.  `heads` (default:
    all of costs' rows, batch 1) only labels the LaunchOrder: a unit's index depends on batch * heads alone.

        "lanes"    heads bh are assigned whole to the lane with the least load so far, in descending order of head cost (ties:
                   the lower bh, the lower lane); each lane's units are then sorted by descending cost (ties: (bh, qb) ascending)
                   and the lanes padded with -1 at the end to the longest.  A head stays on one lane, as in the kernels' own
                   order (the K / V^T locality that bh % 8 gives).
        "units"    all units sorted by descending cost (ties: (bh, qb)) and dealt round-robin over the lanes: the better
                   schedule in a list-scheduling model, at the price of the head-to-lane affinity.
        "natural"  the kernels' own mapping as a table (bh = (b >> 3) // q_blocks * 8 + (b & 7), qb = (b >> 3) % q_blocks): for
                   tests and for pricing the indirection."""
    costs = [list(row) for row in costs]
    if not costs or not costs[0] or any(len(r) != len(costs[0]) for r in costs):
        raise ValueError("balanced_order takes costs[batch * heads][q_blocks] with at least one unit")
    if policy not in ORDER_POLICIES:
        raise ValueError("balanced_order: policy must be one of %s, got %r" % (", ".join(ORDER_POLICIES), policy))
    nbh, qn = len(costs), len(costs[0])
    C = np.asarray(costs, dtype=np.int64)
    by_cost = lambda units: units[np.lexsort((units, -C.reshape(-1)[units]))]      # descending cost, ties by (bh, qb) ascending
    if policy == "natural":
        b = np.arange((nbh + LANES - 1) // LANES * LANES * qn)
        bh, qb = (b >> 3) // qn * LANES + (b & 7), (b >> 3) % qn
        order = np.where(bh < nbh, bh * qn + qb, -1)
    elif policy == "lanes":
        head_cost = C.sum(axis=1)
        load, heads_of = [0] * LANES, [[] for _ in range(LANES)]
        for bh in np.lexsort((np.arange(nbh), -head_cost)).tolist():
            x = min(range(LANES), key=lambda i: (load[i], i))
            load[x] += int(head_cost[bh])
            heads_of[x].append(bh)
        order = np.full((max(len(h) for h in heads_of) * qn, LANES), -1, dtype=np.int64)
        for x, hs in enumerate(heads_of):
            if hs:
                order[:len(hs) * qn, x] = by_cost((np.asarray(sorted(hs))[:, None] * qn + np.arange(qn)[None, :]).reshape(-1))
        order = order.reshape(-1)
    else:      # dealt round-robin over the lanes: entry i of the sorted list is on lane i % 8
        order = np.full((nbh * qn + LANES - 1) // LANES * LANES, -1, dtype=np.int64)
        order[:nbh * qn] = by_cost(np.arange(nbh * qn))
    order = torch.from_numpy(order.astype(np.int32))
    heads = nbh if heads is None else int(heads)
    if heads < 1 or nbh % heads:
        raise ValueError("balanced_order: %d rows of costs are no multiple of heads = %d" % (nbh, heads))
    return LaunchOrder(order, nbh // heads, heads, qn)


def _balance_policy(value):
    """attn_window_balance -> None (off), "lanes" or "units".  True is "units": the policy that won at most launch shapes when the
    two were measured (profiles/attn_window_order_ab.json; README)."""
    if value is False or value is None or value == 0:
        return None
    if value is True or value == 1:
        return "units"
    if value in ("lanes", "units"):
        return value
    raise ValueError("attn_window_balance must be False, True (= \"units\"), \"lanes\" or \"units\", got %r" % (value,))


def head_window_ranges(base, windowed):
    """The per-head table of a layer: head h gets `base`'s rows where windowed[h], else the one full range [(0, Skv)] (zero-padded
    to base.max_ranges).  `base` itself when every head is windowed (the shared-table launch), None when no head is (the dense
    launch)."""
    if not isinstance(base, KvRanges):
        raise ValueError("head_window_ranges takes a KvRanges, got %s" % type(base).__name__)
    windowed = [bool(w) for w in windowed]
    if not windowed:
        raise ValueError("head_window_ranges: no head")
    if all(windowed):
        return base
    if not any(windowed):
        return None
    full = torch.zeros_like(base.table)
    full[:, 0, 1] = base.Skv
    return KvRangesHeads(torch.stack([base.table if w else full for w in windowed]), base.Skv, base.Sq)


def decide_heads(recall, threshold):
    """recall[sample][head] (Python floats: the softmax mass head h's queries keep inside the window, per sample) -> [bool per
    head]: a head keeps the window iff its recall reaches `threshold` on EVERY sample (min over the samples >= threshold).  NaN is
    not windowed."""
    rows = [list(r) for r in recall]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("decide_heads takes recall[samples][heads] with at least one sample and one head")
    thr = float(threshold)
    out = []
    for h in range(len(rows[0])):
        vals = [float(r[h]) for r in rows]
        out.append(not any(math.isnan(v) for v in vals) and min(vals) >= thr)
    return out


def _widths_tuple(widths, what):
    """`widths` (a sequence of ints, or the string "1,2,4") as a strictly ascending tuple of positive ints; ValueError otherwise."""
    if isinstance(widths, str):
        try:
            widths = tuple(int(x) for x in widths.split(","))
        except ValueError:
            raise ValueError("%s: %r is no comma-separated list of ints" % (what, widths)) from None
    try:
        ws = tuple(widths)
    except TypeError:
        raise ValueError("%s must be a sequence of ints, got %r" % (what, widths)) from None
    if (not ws or any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) for w in ws) or ws[0] < 1
            or any(b <= a for a, b in zip(ws, ws[1:]))):
        raise ValueError("%s must be a strictly ascending tuple of positive ints, got %r" % (what, widths))
    if 2 * len(ws) + 3 > MAX_SEGMENTS:
        raise ValueError("%s: %d widths need %d segments, the kernel takes %d (at most %d widths)"
                         % (what, len(ws), 2 * len(ws) + 3, MAX_SEGMENTS, (MAX_SEGMENTS - 3) // 2))
    return tuple(int(w) for w in ws)


def _ascending(values):
    """values with every entry raised to its predecessor's (a running maximum; NaN entries stay and are skipped over)."""
    out = []
    for v in values:
        out.append(max(v, out[-1]) if out and not math.isnan(v) and not math.isnan(out[-1]) else v)
    return out


def width_segments(k):
    """For a frame_profile_segments table of k widths: per width index j the segment indices whose mass counts for width j --
    sink (0), tail (2k + 2), core (k + 1) and the rings 2 .. j + 1 on both sides (left ring r at k - r + 2, right ring r at k + r)."""
    k = int(k)
    out = []
    for j in range(1, k + 1):
        idx = [0, k + 1, 2 * k + 2]
        for r in range(2, j + 1):
            idx += [k - r + 2, k + r]
        out.append(sorted(idx))
    return out


def frame_profile_segments(frames, tokens_per_frame, widths, sink_frames=1, tail=None, rows=None):
    """The keys of frame_window_ranges' layout (no prefix) cut into 2k + 3 segments per block of 256 queries, k = len(widths), as a
    KvSegments: a partition of [0, Skv), so the launch is the dense attention, and the segment index means the same in every block.
    With f64(x) = x - x % 64, F = frames, hw = tokens_per_frame and a block covering the latent frames fa .. fb the cuts are

        E_s = f64(min(sink, F) hw)
        L_j = max(E_s, f64(max(fa - w_j, 0) hw))
        R_j = T0 if min(fb + w_j + 1, F) == F else max(L_1, f64(min(fb + w_j + 1, F) hw))
        T0  = f64(F hw) with a tail, else Skv

    and the segments, in table order,

        [0, E_s) sink | [E_s, L_k) far left | [L_k, L_(k-1)) .. [L_2, L_1) left rings | [L_1, R_1) core |
        [R_1, R_2) .. [R_(k-1), R_k) right rings | [R_k, T0) far right | [T0, Skv) tail

    (empty ones are stored as (0, 0)).  A block that holds any row >= F hw puts [0, Skv) into the core segment.  The mass counted
    for width w_j is sink + tail + core + the rings 2 .. j on both sides (width_segments).

    CONSERVATIVE ROUNDING.  Every cut lies on the 64-key grid, and the cuts are rounded so that for every block and every width
    the counted key set is a SUBSET of what frame_window_ranges(..., window=w_j) visits (which rounds its begins DOWN and keeps its
    ends), short by at most 126 keys; the two are equal where hw % 64 == 0 and there is no tail.  A recall measured on this table
    is therefore a LOWER BOUND for the recall of the table that will be launched."""
    F, hw, sink = int(frames), int(tokens_per_frame), int(sink_frames)
    ws = _widths_tuple(widths, "frame_profile_segments: widths")
    if F < 1 or hw < 1 or sink < 0:
        raise ValueError("frame_profile_segments: frames=%d tokens_per_frame=%d sink_frames=%d" % (F, hw, sink))
    k = len(ws)
    S = F * hw
    Sq = S if rows is None else int(rows)
    f64 = lambda x: x - x % KV_ALIGN
    if tail is not None:
        tb, te = int(tail[0]), int(tail[1])
        if not S <= tb < te:
            raise ValueError("frame_profile_segments: tail (%d, %d) must lie behind the %d video keys and hold a key" % (tb, te, S))
        Skv, T0 = te, f64(S)
    else:
        Skv = T0 = S
    q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
    t = torch.zeros(q_blocks, 2 * k + 3, 2, dtype=torch.int32)
    for j in range(q_blocks):
        r0, r1 = j * Q_BLOCK, min((j + 1) * Q_BLOCK, Sq) - 1
        if r1 >= S:
            t[j, k + 1, 0], t[j, k + 1, 1] = 0, Skv
            continue
        fa, fb = r0 // hw, r1 // hw
        Es = f64(min(sink, F) * hw)
        L = [max(Es, f64(max(fa - w, 0) * hw)) for w in ws]                              # L[0] = L_1 >= L_2 >= ... >= L_k >= E_s
        R = [T0 if min(fb + w + 1, F) == F else max(L[0], f64(min(fb + w + 1, F) * hw)) for w in ws]      # R_1 <= ... <= R_k <= T0
        cuts = [0, Es] + L[::-1] + R + [T0, Skv]                                         # 2k + 4 cuts, ascending
        for i in range(2 * k + 3):
            if cuts[i + 1] > cuts[i]:
                t[j, i, 0], t[j, i, 1] = cuts[i], cuts[i + 1]
    return KvSegments(t, Skv, Sq)


def decide_widths(recall, widths, threshold):
    """recall[sample][head][width index] (Python floats: the softmax mass head h's queries keep inside width w_j, per sample) ->
    [int per head]: the smallest w_j whose recall reaches `threshold` on EVERY sample, else 0 (dense).  A head with a NaN gets 0."""
    ws = _widths_tuple(widths, "decide_widths: widths")
    rows = [[list(h) for h in r] for r in recall]
    if (not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows)
            or any(len(h) != len(ws) for r in rows for h in r)):
        raise ValueError("decide_widths takes recall[samples][heads][%d widths] with at least one sample and one head" % len(ws))
    thr = float(threshold)
    out = []
    for h in range(len(rows[0])):
        vals = [[float(x) for x in r[h]] for r in rows]
        chosen = 0
        if not any(math.isnan(x) for v in vals for x in v):
            for j, w in enumerate(ws):
                if min(v[j] for v in vals) >= thr:
                    chosen = w
                    break
        out.append(chosen)
    return out


def head_width_ranges(base_by_width, chosen):
    """The per-head table of a layer whose heads chose their own width: head h gets the rows of base_by_width[chosen[h]] (the
    frame_window_ranges table of that width; None where that window is the dense attention), or the one full range [(0, Skv)] for
    chosen[h] == 0, zero-padded to the largest max_ranges among the tables in use.  The shared KvRanges when every head chose the
    same width, None when every head is dense, a KvRangesHeads otherwise."""
    chosen = [int(w) for w in chosen]
    if not chosen:
        raise ValueError("head_width_ranges: no head")
    tables = {}
    for w in set(chosen):
        if w == 0:
            tables[w] = None
            continue
        if w not in base_by_width:
            raise ValueError("head_width_ranges: no table for the chosen width %d (have %s)" % (w, sorted(base_by_width)))
        tables[w] = base_by_width[w]
        if tables[w] is not None and not isinstance(tables[w], KvRanges):
            raise ValueError("head_width_ranges takes KvRanges tables, got %s for width %d" % (type(tables[w]).__name__, w))
    used = [t for t in tables.values() if t is not None]
    if not used:
        return None
    if len(tables) == 1:
        return used[0]
    if any((t.Sq, t.Skv) != (used[0].Sq, used[0].Skv) for t in used):
        raise ValueError("head_width_ranges: the tables were built for different (Sq, Skv)")
    n = max(t.max_ranges for t in used)
    full = torch.zeros(used[0].q_blocks, n, 2, dtype=torch.int32)
    full[:, 0, 1] = used[0].Skv
    padded = {}
    for w, t in tables.items():
        if t is None:
            padded[w] = full
        else:
            padded[w] = torch.zeros_like(full)
            padded[w][:, :t.max_ranges] = t.table
    return KvRangesHeads(torch.stack([padded[w] for w in chosen]), used[0].Skv, used[0].Sq)


LAYOUTS = ("window", "band", "dense")


class HeadList:
    """The heads a layout move or a band launch works on: DISTINCT indices in [0, heads), in any order, validated on the CPU and
    uploaded once per device as int32 -- the only thing _lib.attn_rows_position_major / attn_vt_position_major take, so a list
    that reaches the kernels from Python names heads that exist.  Device-resident: a captured forward replays it."""

    def __init__(self, indices, heads):
        idx = [int(i) for i in indices]
        heads = int(heads)
        if not idx or heads < 1:
            raise ValueError("HeadList needs at least one head index and heads >= 1 (got %d indices, heads = %d)" % (len(idx), heads))
        if len(set(idx)) != len(idx):
            raise ValueError("HeadList: the head indices must be distinct, got %r" % (idx,))
        if min(idx) < 0 or max(idx) >= heads:
            raise ValueError("HeadList: head indices must lie in [0, %d), got %r" % (heads, idx))
        self.indices, self.heads, self.n_sel = tuple(idx), heads, len(idx)
        self.table = torch.tensor(idx, dtype=torch.int32)
        self._device = {}

    on = KvRanges.on
    device_table = KvRanges.device_table


def position_major_index(frames, hw):
    """The permutation pi of the position-major token order as a CPU int64 tensor [frames * hw]: pi[f * hw + p] = p * frames + f.
    x_pm[pi] = x_fm moves a frame-major tensor over, x_fm = x_pm[pi] reads it back; the inverse of pi is
    position_major_index(hw, frames)."""
    F, hw = int(frames), int(hw)
    if F < 1 or hw < 1:
        raise ValueError("position_major_index: frames=%d hw=%d" % (F, hw))
    s = torch.arange(F * hw, dtype=torch.int64)
    return (s % hw) * F + s // hw


def position_band_ranges(frames, hw, band):
    """The band policy as a KvRanges for Sq = Skv = frames * hw tokens in POSITION-MAJOR order (row p * frames + f), or None where it
    is the dense attention.  A query at spatial position p is to see every frame of the positions within `band` of p (the
    distance is taken in the flattened position index, as the frame window takes it in frames).  A block of 256 rows holds the
    positions p0 .. p1 and gets the ONE range

        [ (max(0, p0 - band) * frames) rounded down to 64,  min(hw, p1 + band + 1) * frames )

    a superset for each of its queries.  In the frame-major order the same keys are hw tokens apart, one run per frame."""
    F, hw, band = int(frames), int(hw), int(band)
    if F < 1 or hw < 1 or band < 0:
        raise ValueError("position_band_ranges: frames=%d hw=%d band=%d" % (F, hw, band))
    S = F * hw
    per_block = []
    for r0 in range(0, S, Q_BLOCK):
        p0, p1 = r0 // F, (min(r0 + Q_BLOCK, S) - 1) // F
        per_block.append([((max(0, p0 - band) * F) & ~(KV_ALIGN - 1), min(hw, p1 + band + 1) * F)])
    return _table(per_block, S, S)


def decide_layouts(recall_window, recall_band, cost_window, cost_band, threshold):
    """Per head one of "window" | "band" | "dense" from the two candidates' recalls [sample][head] (Python floats) and their costs
    (the mean unit_costs of the candidate's table: one number each, the tables are shared by the heads).  A candidate QUALIFIES
    when its recall reaches `threshold` on every sample (NaN never does); of the qualifying candidates the cheaper one wins, a
    tie goes to the window; a head with no qualifying candidate stays dense."""
    win = decide_heads(recall_window, threshold)
    ban = decide_heads(recall_band, threshold)
    if len(win) != len(ban) or len(list(recall_window)) != len(list(recall_band)):
        raise ValueError("decide_layouts: the two recalls differ in shape")
    cw, cb = float(cost_window), float(cost_band)
    if math.isnan(cw) or math.isnan(cb) or cw < 0 or cb < 0:
        raise ValueError("decide_layouts: costs must be numbers >= 0, got %r and %r" % (cost_window, cost_band))
    out = []
    for w, b in zip(win, ban):
        if w and b:
            out.append("band" if cb < cw else "window")
        else:
            out.append("window" if w else "band" if b else "dense")
    return out


def mean_unit_cost(kv_ranges):
    """The mean of unit_costs over the blocks of a shared table: what decide_layouts compares."""
    row = unit_costs(kv_ranges, 1, 1)[0]
    return sum(row) / float(len(row))


def head_layout_ranges(base, layouts):
    """The MAIN launch's table of a layer whose heads chose `layouts` ("window" | "band" | "dense" each), and the band heads:
    (table, band_heads).  The band heads run in a launch of their own on position-major operands and are ABSENT from the main
    table (all (0, 0): the kernels write zeros for them, the scatter behind overwrites those); the others are what
    head_window_ranges makes them.  With no band head the table is head_window_ranges' (a shared KvRanges, a KvRangesHeads, or
    None for all dense) and band_heads is (); when every head chose the band the table is None and there is no main launch."""
    if not isinstance(base, KvRanges):
        raise ValueError("head_layout_ranges takes a KvRanges, got %s" % type(base).__name__)
    layouts = list(layouts)
    if not layouts or any(l not in LAYOUTS for l in layouts):
        raise ValueError("head_layout_ranges: layouts must be a non-empty list of %s, got %r" % (" | ".join(LAYOUTS), layouts))
    band_heads = tuple(h for h, l in enumerate(layouts) if l == "band")
    if not band_heads:
        return head_window_ranges(base, [l == "window" for l in layouts]), ()
    if len(band_heads) == len(layouts):
        return None, band_heads
    rows = {"window": base.table, "band": torch.zeros_like(base.table), "dense": torch.zeros_like(base.table)}
    rows["dense"][:, 0, 1] = base.Skv
    return KvRangesHeads(torch.stack([rows[l] for l in layouts]), base.Skv, base.Sq, absent_ok=True), band_heads


def full_ranges(Sq, Skv):
    """The one-range table [0, Skv) for every block: the dense attention through the ranged entry."""
    q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
    t = torch.zeros(q_blocks, 1, 2, dtype=torch.int32)
    t[:, 0, 1] = Skv
    return KvRanges(t, Skv, Sq)


def _block_ranges(kv_ranges):
    """The used (begin, end) entries of every block of a KvRanges, as lists of tuples."""
    a = kv_ranges.table.numpy()
    return [[(int(b), int(e)) for b, e in blk if b or e] for blk in a]


def _ranges_table(per_block, Skv, Sq, **kw):
    """The blocks' range lists as a KvRanges (at least one column; a block may be empty where the keywords allow it)."""
    max_ranges = max(1, max(len(r) for r in per_block))
    if max_ranges > MAX_RANGES:
        raise ValueError("a block needs %d key ranges, the kernels take %d" % (max_ranges, MAX_RANGES))
    t = torch.zeros(len(per_block), max_ranges, 2, dtype=torch.int32)
    for j, r in enumerate(per_block):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return KvRanges(t, Skv, Sq, **kw)


def grid_aligned(kv_ranges, grid=KV_ALIGN):
    """The same table with every END rounded up to a multiple of 64 (clamped to Skv) and touching ranges merged: a superset whose
    gaps begin on the kernels' key grid, so that complement_ranges can visit exactly the keys it leaves out.

    grid (a multiple of 64; attn_pool.py: 64 G) > 64: every BEGIN is rounded down and every end up to a multiple of `grid`, and
    every block also gets the keys behind the last multiple of `grid`, [Skv - Skv % grid, Skv): every gap then begins AND ends on
    that grid, so a group of G = grid / 64 consecutive keys lies on one side of every cut."""
    if not isinstance(kv_ranges, KvRanges) or kv_ranges.absent:
        raise ValueError("grid_aligned takes a KvRanges with keys in every block")
    grid = int(grid)
    if grid < KV_ALIGN or grid % KV_ALIGN:
        raise ValueError("grid_aligned: grid=%d must be a positive multiple of %d" % (grid, KV_ALIGN))
    Skv = kv_ranges.Skv
    per_block = []
    for blk in _block_ranges(kv_ranges):
        if grid != KV_ALIGN and Skv % grid:
            blk = blk + [(Skv - Skv % grid, Skv)]
        out = []
        for b, e in blk:
            b, e = b - b % grid, min(-(-e // grid) * grid, Skv)
            if out and b <= out[-1][1]:
                out[-1][1] = max(out[-1][1], e)
            else:
                out.append([b, e])
        per_block.append([tuple(r) for r in out])
    return _ranges_table(per_block, Skv, kv_ranges.Sq)


def pooled_ranges(far, group, Skv=None):
    """The far table of complement_ranges(grid_aligned(table, grid=64 * group)) with every begin and end divided by `group`: the
    ranges of the POOLED keys (pooled key p stands for the keys [p group, (p + 1) group)), on the kernels' 64-key grid, as a
    KvRanges(empty_ok=True) for the same queries.  Skv: the key count the launch will state (default: the far table's keys
    divided by group; the d = 64 entries have one S for queries and keys and state Sq).  ValueError for a table with a begin or
    an end off the 64 group grid: a pooled key would then stand for keys that the near table visits too."""
    group = int(group)
    if not isinstance(far, KvRanges) or group < 1:
        raise ValueError("pooled_ranges takes a KvRanges and a group >= 1")
    per_block = []
    for j, blk in enumerate(_block_ranges(far)):
        for b, e in blk:
            if b % (KV_ALIGN * group) or e % (KV_ALIGN * group):
                raise ValueError("block %d: the far range (%d, %d) does not lie on the %d-key grid (grid_aligned(table, grid=%d) "
                                 "makes it so)" % (j, b, e, KV_ALIGN * group, KV_ALIGN * group))
        per_block.append([(b // group, e // group) for b, e in blk])
    return _ranges_table(per_block, far.Skv // group if Skv is None else int(Skv), far.Sq, empty_ok=True)


def complement_ranges(kv_ranges):
    """The gaps of each block of a grid-aligned table (grid_aligned's result), as a KvRanges(empty_ok=True): with it the two tables
    visit every key of every block exactly once.  A block whose table already holds every key has no range here.  ValueError
    for a table whose gaps would not begin on the key grid (the kernels round a begin DOWN: a key would be visited twice)."""
    if not isinstance(kv_ranges, KvRanges) or kv_ranges.absent:
        raise ValueError("complement_ranges takes a KvRanges with keys in every block")
    Skv = kv_ranges.Skv
    per_block = []
    for j, blk in enumerate(_block_ranges(kv_ranges)):
        gaps, at = [], 0
        for b, e in blk + [(Skv, Skv)]:
            if b > at:
                if at % KV_ALIGN:
                    raise ValueError("block %d: the range ending at %d is not grid-aligned (grid_aligned makes it so)" % (j, at))
                gaps.append((at, b))
            at = e
        per_block.append(gaps)
    return _ranges_table(per_block, Skv, kv_ranges.Sq, empty_ok=True)


def frame_window_ranges(frames, tokens_per_frame, window, sink_frames=1, tail=None, rows=None, prefix=0):
    """The frame-window policy as a KvRanges, or None when it is the dense attention (every block sees every key).

    The keys are `frames` latent frames of `tokens_per_frame` (hw) tokens, frame by frame, optionally followed by other keys of
    which tail = (begin, end) are to be seen by everybody (HunyuanVideo: the sample's valid prompt keys [S, S + valid)); Skv is
    tail's end, or frames * hw.  The queries are rows 0 .. rows - 1 (default frames * hw) in the same order.  A block of 256
    queries covering the latent frames fa .. fb gets
        the sink    [0, sink_frames * hw),
        the window  [(fa - window) * hw, (fb + window + 1) * hw) clipped to the video,
        the tail,
    begins rounded DOWN to a multiple of 64 (a superset: always safe), touching or overlapping ranges merged.  A block that
    holds any row >= frames * hw (prompt queries, and the block that straddles the boundary) gets the single full range.

    prefix > 0 (CogVideoX: the prompt tokens come FIRST, [text; frame 0; frame 1; ...]): the keys and the queries are `prefix`
    rows followed by the frames, frame f's keys are [prefix + f * hw, prefix + (f + 1) * hw), every block sees the keys
    [0, prefix), and a block that holds any row < prefix gets the single full range.  It excludes `tail`."""
    F, hw, W, sink = int(frames), int(tokens_per_frame), int(window), int(sink_frames)
    if F < 1 or hw < 1 or W < 0 or sink < 0:
        raise ValueError("frame_window_ranges: frames=%d tokens_per_frame=%d window=%d sink_frames=%d" % (F, hw, W, sink))
    if int(prefix):
        if tail is not None:
            raise ValueError("frame_window_ranges: prefix and tail exclude each other (the prompt keys lie in front or behind)")
        return _prefixed_ranges(F, hw, W, sink, int(prefix), rows)
    S = F * hw
    Sq = S if rows is None else int(rows)
    if tail is not None:
        tb, te = int(tail[0]), int(tail[1])
        if not S <= tb < te:
            raise ValueError("frame_window_ranges: tail (%d, %d) must lie behind the %d video keys and hold a key" % (tb, te, S))
        Skv = te
    else:
        Skv = S
    q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
    per_block = []
    for j in range(q_blocks):
        r0, r1 = j * Q_BLOCK, min((j + 1) * Q_BLOCK, Sq) - 1
        if r1 >= S:
            per_block.append([(0, Skv)])
            continue
        fa, fb = r0 // hw, r1 // hw
        want = []
        if sink > 0:
            want.append((0, min(sink, F) * hw))
        want.append((max(fa - W, 0) * hw, min(fb + W + 1, F) * hw))
        if tail is not None:
            want.append((tb, te))
        per_block.append(_merged(want))
    return _table(per_block, Skv, Sq)


def _merged(want):
    """The wanted (begin, end) runs of one block: begins rounded down to the tile grid, sorted, touching or overlapping ones merged."""
    want = sorted((b - b % KV_ALIGN, e) for b, e in want)
    merged = [list(want[0])]
    for b, e in want[1:]:
        if b <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([b, e])
    return [tuple(m) for m in merged]


def _table(per_block, Skv, Sq):
    """The blocks' range lists as a KvRanges; None when every block has the single full range."""
    if all(r == [(0, Skv)] for r in per_block):
        return None
    max_ranges = max(len(r) for r in per_block)
    t = torch.zeros(len(per_block), max_ranges, 2, dtype=torch.int32)
    for j, r in enumerate(per_block):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return KvRanges(t, Skv, Sq)


def _prefixed_ranges(F, hw, W, sink, prefix, rows):
    """frame_window_ranges for the layout [prefix; frame 0; frame 1; ...]."""
    if prefix < 0:
        raise ValueError("frame_window_ranges: prefix=%d" % prefix)
    Skv = prefix + F * hw
    Sq = Skv if rows is None else int(rows)
    if Sq > Skv:
        raise ValueError("frame_window_ranges: rows=%d beyond the %d prefix and video rows" % (Sq, Skv))
    q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
    per_block = []
    for j in range(q_blocks):
        r0, r1 = j * Q_BLOCK, min((j + 1) * Q_BLOCK, Sq) - 1
        if r0 < prefix:
            per_block.append([(0, Skv)])
            continue
        fa, fb = (r0 - prefix) // hw, (r1 - prefix) // hw
        want = [(0, prefix + min(sink, F) * hw), (prefix + max(fa - W, 0) * hw, prefix + min(fb + W + 1, F) * hw)]
        per_block.append(_merged(want))
    return _table(per_block, Skv, Sq)


class SelfAttnOperands(namedtuple("SelfAttnOperands", "head_dim q k vt o batch heads Sq Skv q_bs q_rs k_bs k_rs vt_bs vt_rs o_bs o_rs scale "
                                  "q_off k_off vt_off o_off q_prescaled", defaults=(0, 0, 0, 0, False))):
    """What every _lib.flash_attn_d{64,128}* wrapper takes for one self-attention launch group (a block's whole batch in Wan and
    CogVideoX, one sample in HunyuanVideo): strides and offsets in elements.  The d = 64 wrappers have no Skv, no K strides and no
    vt_off / o_off, and a d = 64 record asserts what that assumes; q_prescaled (d = 64 only) is the dense wrapper's flag -- Q
    carries scale * log2(e), the only form the ranged entries have."""
    __slots__ = ()

    def __new__(cls, *a, **k):
        self = super().__new__(cls, *a, **k)
        assert self.head_dim == 128 and not self.q_prescaled or self.head_dim == 64 and (
            self.Sq == self.Skv and (self.k_bs, self.k_rs) == (self.q_bs, self.q_rs) and self.vt_off == 0 and self.o_off == 0), self
        return self

    def args(self):
        """(positionals, offsets): the 17 positionals of a d = 128 wrapper up to `scale`, or the 13 of a d = 64 wrapper (its dense
        one takes `scale` behind them); the table, the order and lse= follow."""
        if self.head_dim == 64:
            return ((self.q, self.k, self.vt, self.o, self.batch, self.heads, self.Sq, self.q_bs, self.q_rs, self.vt_bs, self.vt_rs,
                     self.o_bs, self.o_rs), dict(q_off=self.q_off, k_off=self.k_off))
        return ((self.q, self.k, self.vt, self.o, self.batch, self.heads, self.Sq, self.Skv, self.q_bs, self.q_rs, self.k_bs, self.k_rs,
                 self.vt_bs, self.vt_rs, self.o_bs, self.o_rs, self.scale),
                dict(q_off=self.q_off, k_off=self.k_off, vt_off=self.vt_off, o_off=self.o_off))


def launch_self_attention(timed, name, ops, table, order=None):
    """One self-attention launch of `ops` under the profile key `name`: with `order` (a LaunchOrder) the _order entry, with a
    KvRangesHeads the per-head entry, with a KvRanges the shared-table entry, with None the dense one.  timed(name, fn, *a, **kw)
    makes the call (a model's _timed, or a pass-through)."""
    a, offs = ops.args()
    entry = "flash_attn_d%d" % ops.head_dim       # (the wrappers are looked up in _lib at call time)
    if order is not None:
        return timed(name, getattr(_lib, entry + "_ranges_order"), *a, table, order, **offs)
    if isinstance(table, KvRangesHeads):
        return timed(name, getattr(_lib, entry + "_ranges_heads"), *a, table, **offs)
    if table is not None:
        return timed(name, getattr(_lib, entry + "_ranges"), *a, table, **offs)
    if ops.head_dim == 64:
        return timed(name, _lib.flash_attn_d64, *a, ops.scale, **offs, q_prescaled=ops.q_prescaled)
    return timed(name, _lib.flash_attn_d128, *a, **offs)


def calibrate_self_attention(timed, name, ops, cal, layer, samples, sample0, rows, full, base):
    """The self-attention of `ops` on the calibration forward (HeadWindowHost): the dense output into ops.o under `name`, the
    measurement under "attn_calib".  `cal`: the buffers of _head_window_mode, laid out [layer][sample][head]; `ops` holds the
    samples sample0 .. sample0 + ops.batch - 1 of `samples`; rows = (row0, n): the latent-query rows the recall is taken over.

    cal.widths set: ONE alg_flash_attn_d128_ranges_prefix launch over `base` (the frame_profile_segments table), then
    alg_attn_prefix_mass.  Otherwise the per-head entry with `full` (the one full range; writes lse_full), the same with `base` (the
    window table) into the scratch cal.o [samples][Sq][heads * head_dim] for lse_part, and alg_attn_lse_recall."""
    a, offs = ops.args()
    heads, Sq, slot = ops.heads, ops.Sq, layer * samples + sample0
    if cal.widths is not None:
        p_off = sample0 * heads * cal.segments * Sq
        timed(name, _lib.flash_attn_d128_ranges_prefix, *a, base, cal.prefix, **offs, prefix_off=p_off)
        return timed("attn_calib", _lib.attn_prefix_mass, cal.prefix, cal.mass, ops.batch * heads, cal.segments, Sq, row0=rows[0],
                     rows=rows[1], prefix_off=p_off, out_off=slot * heads * cal.segments)
    entry, lse_off, row = "flash_attn_d%d_ranges_heads" % ops.head_dim, sample0 * heads * Sq, heads * ops.head_dim
    timed(name, getattr(_lib, entry), *a, full, lse=cal.lse_full, **offs, lse_off=lse_off)
    a, offs = SelfAttnOperands(*ops._replace(o=cal.o, o_bs=Sq * row, o_rs=row, o_off=sample0 * Sq * row)).args()
    timed("attn_calib", getattr(_lib, entry), *a, base, lse=cal.lse_part, **offs, lse_off=lse_off)
    return timed("attn_calib", _lib.attn_lse_recall, cal.lse_part, cal.lse_full, cal.recall, ops.batch * heads, Sq, row0=rows[0],
                 rows=rows[1], part_off=lse_off, full_off=lse_off, out_off=slot * heads)


class SelfAttnPlan:
    """How one forward's self-attention launches (HeadWindowHost._self_attn_begin): per launch group g the shared frame-window
    table shared[g] (None: the dense launch), and with attn_window_recall > 0 the mode -- None (off), "dense" (not calibrated yet),
    "tables" or "calibrating" -- with `cal` (the calibration buffers), bases[g] (what the per-head tables are built from: shared[g],
    or with attn_window_widths the {width: table} dict), and on the calibration forward full[g] (the one-full-range table) and
    measure[g] (what the measuring launch runs over: shared[g], or the profile table)."""

    def __init__(self, host, shared, batch):
        self.host, self.shared, self.batch = host, list(shared), int(batch)
        self.mode = self.cal = self.full = self.measure = None
        self.bases = self.shared
        self.far = None       # the forward's attn_far.AttnFarPass (attn_far_reuse) or attn_pool.AttnPoolPass (attn_far_pool), set by
                              # the model; None: off

    def order(self, table):
        """The balanced LaunchOrder of a per-head table (attn_window_balance), else None."""
        return self.host._layer_order(table, self.batch) if isinstance(table, KvRangesHeads) else None

    def layer(self, layer, g=0):
        """(table, order) group g of layer `layer` launches with, outside the calibration forward."""
        if self.mode is None:
            return self.shared[g], None
        if self.mode != "tables":      # dense until calibrated
            return None, None
        table = self.host._layer_table(self.bases[g], layer)
        return table, self.order(table)

    def finish(self, band_table=None):
        """End of the forward: on the calibration forward the decisions and the per-head tables (_head_window_finish)."""
        if self.cal is not None:
            self.host._head_window_finish(self.cal, self.bases, batch=self.batch, band_table=band_table)
        if self.far is not None:
            self.far.finish()


class HeadWindowHost:
    """What a DiT with `attn_window` needs for per-head windows chosen by recall (mixed into WanTransformer3DModel,
    HunyuanVideoTransformer3DModel and CogVideoXTransformer3DModel).

        attn_window_recall   0.0: off -- the forward is the shared-window one, launch for launch.  > 0 (with attn_window > 0): a head
                             keeps the window only where its measured recall reaches this value
        attn_window_stats    after a calibration forward one record per layer:
                             {"layer", "recall": [[per head] per sample], "windowed": [bool per head]}
        attn_window_balance  False: off -- every launch is exactly what it is without the flag.  True (= "units"), "lanes" or "units":
                             a calibrated layer whose table is per-head (dense AND windowed heads) launches the _order entry with a
                             balanced_order of that policy; the output keeps its bits.  Needs attn_window_recall > 0
                             Set it BEFORE the calibration forward where later forwards are captured: that forward builds the
                             orders of its own batch size; any other (another batch size, a flag or policy changed later) is
                             built on the first eager forward that needs it, and a capture that would have to build one raises
        attn_window_widths   None: off -- calibration, tables and stats are exactly what they are without it.  A strictly ascending
                             tuple of positive ints whose last element equals attn_window (or the string "1,2,4"; needs
                             attn_window_recall > 0; head_dim 128 only): every head takes the NARROWEST of these widths that
                             reaches the recall, else it stays dense, and the calibration is ONE launch per layer (below).  The
                             stats records gain "recall_by_width": [[[per width] per head] per sample] and "width": [int per head]
                             (0: dense); "recall" is the recall at the largest width, "windowed" is width > 0
        attn_band            (WanTransformer3DModel only; the other models do not have the attribute) 0: off -- every buffer, key,
                             table, record and launch is what it is without it.  An int > 0 (positions on each side; needs
                             attn_window > 0 and attn_window_recall > 0, ValueError with attn_window_widths): the calibration
                             forward also measures every head's recall inside the position-major band, decide_layouts gives the
                             head the window, the band or the dense launch, and the stats records gain "recall_band"
                             [[per head] per sample] and "layout" [str per head]; "windowed" keeps its meaning, the frame window
        reset_attn_window_heads()   forgets the decisions and the launch orders (the samplers call it at the start of a video)

    With attn_window > 0 and attn_window_recall > 0 a forward is dense until the model is calibrated; the calibration forward is the
    one call_transformer(..., calibrate=True) marks.  Its self-attention output is the dense one (the ranged entry with the one
    full range, which also writes lse_full); a second launch with the window table writes a scratch output and lse_part, and
    alg_attn_lse_recall reduces the two over the latent-query rows into row `layer` of a device buffer [layers][samples][heads].
    One copy to pinned host memory and one stream synchronisation end the forward; decide_heads then runs per layer on the host.
    Later forwards launch, per layer, the dense entry (no head windowed), today's shared-table entry (every head) or
    alg_flash_attn_d128_ranges_heads (CogVideoX, head_dim 64: alg_flash_attn_d64_ranges_heads) with the layer's device-resident
    table: nothing on the host depends on the GPU any more, so they can be captured.

    With attn_window_widths the calibration forward of a layer is one alg_flash_attn_d128_ranges_prefix launch over the
    frame_profile_segments table (per sample in HunyuanVideo) into the REAL attention output -- the exact softmax over all keys,
    in another fp32 summation grouping than the dense entry's, so that one forward is not bit-identical to the dense one
    (docs/numerics.md) -- followed by one alg_attn_prefix_mass over the latent-query rows.  Neither a scratch output nor lse_part
    is allocated.  The masses of the segments that count for a width (width_segments) are summed on the host into
    recall[sample][head][width], decide_widths picks the width, head_width_ranges builds the layer's table.  The measured recall
    is a lower bound of the launched table's (frame_profile_segments: conservative rounding).  Later forwards are launch for
    launch what they are without the widths, with these tables.

    CogVideoX: the recall is taken over the latent-query rows [T, S) of the joint sequence (T prompt tokens first), and its dense
    entry may plan a split-KV tail, which the ranged entry never does: the calibration forward's attention output is the dense
    entry's SINGLE-LAUNCH form bit for bit (what ALG_ATTN_SPLIT_TAIL=0 gives) and differs from a planned tail by that option's
    documented <= 1 bf16 step, in that one forward of the video.

    THE LAUNCHES live in this module, once for the three models.  A forward asks _self_attn_begin for its SelfAttnPlan (the shared
    tables from _window_table, the mode, the calibration buffers, the width bases, the profile and full tables), a block describes
    its operands as a SelfAttnOperands record (HunyuanVideo: one per sample) and hands it to launch_self_attention with the
    (table, order) plan.layer resolves -- or, on the calibration forward, to calibrate_self_attention -- and plan.finish ends the
    forward.  The models keep what is theirs: the e4m3 attention in front, their refusals, and Wan's band around the shared call."""

    def _head_window_init(self):
        self._attn_ranges = {}           # shape + (window, sink) -> KvRanges | None; ("profile", ...) -> KvSegments (built once each)
        self.attn_window_recall = 0.0
        self.attn_window_stats = []
        self._attn_calibrate = False     # set around one forward by call_transformer(calibrate=True)
        self._attn_decided = None        # (key, [windowed per head] per layer)
        self._attn_head_tables = {}      # (base table id, windowed) -> KvRanges | KvRangesHeads | None
        self._attn_cal = None            # the calibration buffers, allocated on the first calibration forward only
        self._attn_full = {}             # (Sq, Skv) -> the one-full-range table of the calibration forward's dense launch
        self.attn_window_balance = False
        self.attn_window_order_build_seconds = 0.0     # host time spent building and uploading launch orders, since construction
        self._attn_orders = {}           # (per-head table id, batch, policy) -> (table, LaunchOrder), next to _attn_head_tables
        self.attn_window_widths = None   # None: off; else the candidate widths (see the class docstring)
        self._attn_width_bases = {}      # (table ids per width) -> {width: KvRanges | None}: what _head_table takes with widths
        self._attn_band_plans = {}       # (base table id, layouts) -> (base, main table | None, HeadList | None): attn_band

    @property
    def attn_window_calibrated(self):
        return self._attn_decided is not None

    def _timed(self, name, fn, *a, **k):
        """fn(*a, **k), bracketed by a HIP event pair under `name` when the model's `profile` is a dict (bench / tests)."""
        if self.profile is None:
            return fn(*a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*a, **k)
        e1.record()
        self.profile.setdefault(name, []).append((e0, e1))
        return r

    def _window_sink(self, window=None):
        window, sink = int(self.attn_window if window is None else window), int(self.attn_sink_frames)
        if window < 0 or sink < 0:
            raise ValueError("attn_window and attn_sink_frames must be >= 0 (got %d, %d)" % (window, sink))
        return window, sink

    def _window_table(self, frames, hw, extra=(), window=None, **layout):
        """The frame_window_ranges table of a video shape -- device-resident, built once per (frames, hw, *extra, window, sink): before
        any capture that replays it -- or None where the window is the dense attention.  window: attn_window, or one of
        attn_window_widths; extra, layout: what else the model's token layout depends on, and frame_window_ranges' keywords for it
        (CogVideoX prefix=T; HunyuanVideo tail=, rows=)."""
        window, sink = self._window_sink(window)
        key = (frames, hw) + tuple(extra) + (window, sink)
        if key not in self._attn_ranges:
            r = frame_window_ranges(frames, hw, window, sink_frames=sink, **layout)
            if r is not None:
                r.on(self.device)   # uploaded here, once
            self._attn_ranges[key] = r
        return self._attn_ranges[key]

    def _profile_table(self, frames, hw, widths, extra=(), **layout):
        """The frame_profile_segments table of the same shape for attn_window_widths (device-resident, built once)."""
        _, sink = self._window_sink()
        key = ("profile", frames, hw) + tuple(extra) + (widths, sink)
        if key not in self._attn_ranges:
            self._attn_ranges[key] = frame_profile_segments(frames, hw, widths, sink_frames=sink, **layout)
            self._attn_ranges[key].on(self.device)
        return self._attn_ranges[key]

    def _self_attn_begin(self, shared, key, layers, samples, heads, rows, o_shape, batch, table_of=None, profile_of=None, band=0):
        """The SelfAttnPlan of one forward.  shared: the attn_window table of every launch group (one; HunyuanVideo: one per sample,
        launched with batch 1), None where the window is off or dense -- then nothing else happens.  key .. o_shape, band: what
        _head_window_mode takes.  table_of(g, width), profile_of(g, widths): the model's cached tables of group g, asked for only
        with attn_window_widths."""
        plan = SelfAttnPlan(self, shared, batch)
        if plan.shared[0] is None:
            return plan
        mode = self._head_window_mode(key, layers, samples, heads, rows, o_shape, band=band)
        if mode not in (None, "dense", "tables"):
            plan.cal, mode = mode, "calibrating"
        plan.mode = mode
        widths = self._head_window_widths() if mode is not None else None
        if widths is not None:   # per group the tables of every candidate width, one profile table for the calibration
            plan.bases = [self._head_width_bases(widths, lambda w, g=g: table_of(g, w)) for g in range(len(plan.shared))]
        if plan.cal is not None:
            plan.full = [self._head_full(t.Sq, t.Skv) for t in plan.shared]
            plan.measure = plan.shared if widths is None else [profile_of(g, widths) for g in range(len(plan.shared))]
        return plan

    def _head_window_widths(self):
        """attn_window_widths validated: None (off) or the tuple of candidate widths."""
        if self.attn_window_widths is None:
            return None
        ws = _widths_tuple(self.attn_window_widths, "attn_window_widths")
        if ws[-1] != int(self.attn_window):
            raise ValueError("attn_window_widths %r: the last (largest) width must equal attn_window = %d"
                             % (self.attn_window_widths, int(self.attn_window)))
        if not float(self.attn_window_recall) > 0.0:
            raise ValueError("attn_window_widths=%r needs attn_window_recall > 0: the width of a head is the narrowest that "
                             "reaches the recall" % (self.attn_window_widths,))
        return ws

    def _head_window_band(self):
        """attn_band validated: 0 (off, also for a model without the attribute) or the positions on each side."""
        band = getattr(self, "attn_band", 0)
        if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or band < 0:
            raise ValueError("attn_band must be a non-negative int (positions on each side; 0 = off), got %r" % (band,))
        if not band:
            return 0
        if not int(getattr(self, "attn_window", 0)) > 0 or not float(self.attn_window_recall) > 0.0:
            raise ValueError("attn_band=%d needs attn_window > 0 and attn_window_recall > 0: the band is a third candidate of the "
                             "per-head decision by recall" % band)
        if self.attn_window_widths is not None:
            raise ValueError("attn_band=%d does not combine with attn_window_widths=%r: their calibrations differ (two launches "
                             "against one pass)" % (band, self.attn_window_widths))
        return int(band)

    def _head_width_bases(self, widths, make):
        """{width: make(width)} (make: the model's cached frame_window_ranges table of that width, or None), the SAME dict for the
        same tables: _head_table keys its cache by the dict's identity."""
        tables = [make(w) for w in widths]
        k = tuple(id(t) for t in tables)
        if k not in self._attn_width_bases:
            self._attn_width_bases[k] = dict(zip(widths, tables))     # (the tables are held: their ids stay their own)
        return self._attn_width_bases[k]

    def reset_attn_window_heads(self):
        self._attn_decided = None
        self._attn_head_tables = {}
        self._attn_orders = {}
        self._attn_band_plans = {}
        self.attn_window_stats = []

    def _head_window_mode(self, key, layers, samples, heads, rows, o_shape, band=0):
        """How this forward's self-attention launches: None (attn_window_recall is 0: the shared window, nothing else happens),
        "dense" (not calibrated, not asked to), "tables" (calibrated for `key`), or the calibration buffers (this IS the
        calibration forward).  `key`: what the decisions depend on (video shape, window, sink).  band > 0 (attn_band, where the
        band is not the dense attention): the key carries it, and the buffers gain lse_band (the band launch's LSE, position-major
        rows), lse_band_rows (the same in frame-major row order) and recall_band."""
        thr = float(self.attn_window_recall)
        policy = _balance_policy(self.attn_window_balance)
        widths = self._head_window_widths()
        if not thr > 0.0:
            if policy is not None:
                raise ValueError("attn_window_balance=%r needs attn_window_recall > 0: it orders the launches of layers with dense "
                                 "and windowed heads, which only the recall policy produces" % (self.attn_window_balance,))
            return None
        key = (key, thr) if widths is None else (key, thr, widths)
        if band:
            key = key + (("band", int(band)),)
        if self._attn_decided is not None and self._attn_decided[0] != key:
            self.reset_attn_window_heads()       # another video shape, window, sink, threshold or widths: the decisions do not carry over
        if self._attn_decided is not None:
            return "tables"
        if not self._attn_calibrate:
            return "dense"
        c = self._attn_cal
        shape = (layers, samples, heads, rows, tuple(o_shape), widths) + ((("band", int(band)),) if band else ())
        if widths is not None:     # one pass: the prefixes of one layer and the masses of all; no scratch output, no lse_part
            if c is None or c.shape != shape:
                c = self._attn_cal = SimpleNamespace(shape=shape, widths=widths, segments=2 * len(widths) + 3)
                dev = self.device
                c.prefix = torch.empty(samples, heads, c.segments, rows, dtype=torch.float32, device=dev)
                c.mass = torch.zeros(layers, samples, heads, c.segments, dtype=torch.float64, device=dev)
                c.host = torch.zeros(layers, samples, heads, c.segments, dtype=torch.float64).pin_memory()
            c.key = key
            return c
        if c is None or c.shape != shape:
            c = self._attn_cal = SimpleNamespace(shape=shape, widths=None)
            dev = self.device
            c.lse_full = torch.empty(samples, heads, rows, dtype=torch.float32, device=dev)
            c.lse_part = torch.empty(samples, heads, rows, dtype=torch.float32, device=dev)
            c.o = torch.empty(*o_shape, dtype=torch.bfloat16, device=dev)   # the windowed launch's output: not used
            c.recall = torch.zeros(layers, samples, heads, dtype=torch.float64, device=dev)
            c.host = torch.zeros(layers, samples, heads, dtype=torch.float64).pin_memory()
            c.band = bool(band)
            if band:
                c.lse_band = torch.empty(samples, heads, rows, dtype=torch.float32, device=dev)
                c.lse_band_rows = torch.empty(samples, heads, rows, dtype=torch.float32, device=dev)
                c.recall_band = torch.zeros(layers, samples, heads, dtype=torch.float64, device=dev)
                c.host_band = torch.zeros(layers, samples, heads, dtype=torch.float64).pin_memory()
        c.key = key
        return c

    def _head_window_finish(self, c, bases, batch=None, band_table=None):
        """End of the calibration forward: the recalls to the host (one copy, one synchronisation), decide_heads per layer, and
        the per-head tables of `bases` (the window tables this forward used) built and uploaded -- with attn_window_balance, also
        the launch order of every per-head table for launches of `batch` items (default: the forward's samples).  An order for
        another batch size is built by _layer_order on the first eager forward that needs it.

        With attn_window_widths: `bases` are the {width: table} dicts of _head_width_bases, the copy brings the segment masses,
        which are summed per width (width_segments; clipped to 1 like the recall), and decide_widths picks every head's width.

        With attn_band (`band_table`: the position_band_ranges table the band launches used): the copy brings recall_band too,
        decide_layouts picks every head's layout from the two recalls and the two tables' mean unit costs, a layer's decision is
        its tuple of layouts, the records gain "recall_band" and "layout" ("windowed" stays: the frame window), and the
        HeadList and the main launch's table of every distinct decision are built and uploaded (_band_plan)."""
        c.host.copy_(c.mass if c.widths is not None else c.recall, non_blocking=True)
        if band_table is not None:
            c.host_band.copy_(c.recall_band, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        decided, stats = [], []
        if band_table is not None:
            (base,) = bases
            cost_w, cost_b = mean_unit_cost(base), mean_unit_cost(band_table)
            clip = lambda rec: [[min(x, 1.0) for x in row] for row in rec]     # as below: NaN stays NaN
            for li, (rec, rec_b) in enumerate(zip(c.host.tolist(), c.host_band.tolist())):
                rec, rec_b = clip(rec), clip(rec_b)
                layouts = decide_layouts(rec, rec_b, cost_w, cost_b, self.attn_window_recall)
                decided.append(tuple(layouts))
                stats.append({"layer": li, "recall": rec, "windowed": [l == "window" for l in layouts], "recall_band": rec_b,
                              "layout": list(layouts)})
            self._attn_decided = (c.key, decided)
            self.attn_window_stats = stats
            batch = c.shape[1] if batch is None else int(batch)
            for layouts in set(decided):
                t, _ = self._band_plan(base, layouts)
                if isinstance(t, KvRangesHeads):
                    self._layer_order(t, batch)
            return
        if c.widths is not None:
            counted = width_segments(len(c.widths))
            for li, layer in enumerate(c.host.tolist()):
                # (clipped to 1 like the recall; a ring's mass is the difference of two roundings and may come out below 0 by an
                # ulp of its prefix, so a width never reports less than the narrower one; NaN stays NaN)
                by_width = [[_ascending([min(sum(m[i] for i in idx), 1.0) for idx in counted]) for m in sample] for sample in layer]
                chosen = decide_widths(by_width, c.widths, self.attn_window_recall)
                decided.append(tuple(chosen))
                stats.append({"layer": li, "recall": [[h[-1] for h in sample] for sample in by_width],
                              "windowed": [w > 0 for w in chosen], "recall_by_width": by_width, "width": chosen})
        for li, rec in enumerate([] if c.widths is not None else c.host.tolist()):
            # a recall is a fraction of softmax mass: where the window holds all of it, the two fp32 LSEs may differ by an ulp
            # the wrong way round (1 + 2e-7 seen), which is clipped here; NaN stays NaN
            rec = [[min(x, 1.0) for x in row] for row in rec]
            windowed = decide_heads(rec, self.attn_window_recall)
            decided.append(tuple(windowed))
            stats.append({"layer": li, "recall": rec, "windowed": windowed})
        self._attn_decided = (c.key, decided)
        self.attn_window_stats = stats
        batch = c.shape[1] if batch is None else int(batch)
        for base in bases:
            for windowed in set(decided):
                t = self._head_table(base, windowed)
                if isinstance(t, KvRangesHeads):
                    self._layer_order(t, batch)

    def _band_plan(self, base, layouts):
        """head_layout_ranges(base, layouts) with the band heads as a HeadList (None: no band head), built and uploaded once."""
        k = (id(base), tuple(layouts))
        if k not in self._attn_band_plans:
            t, band_heads = head_layout_ranges(base, layouts)
            if t is not None:
                t.on(self.device)
            hl = HeadList(band_heads, len(layouts)) if band_heads else None
            if hl is not None:
                hl.on(self.device)
            self._attn_band_plans[k] = (base, t, hl)     # (base is held: its id stays its own)
        return self._attn_band_plans[k][1:]

    def _layer_band_plan(self, base, layer):
        """(main table, HeadList | None) layer `layer` launches with once calibrated with attn_band."""
        return self._band_plan(base, self._attn_decided[1][layer])

    def _head_full(self, Sq, Skv):
        if (Sq, Skv) not in self._attn_full:
            self._attn_full[(Sq, Skv)] = full_ranges(Sq, Skv)
        return self._attn_full[(Sq, Skv)]

    def _head_table(self, base, windowed):
        """head_window_ranges(base, windowed), built and uploaded once -- or, with attn_window_widths, head_width_ranges(base,
        widths chosen) for the {width: table} dict `base` of _head_width_bases."""
        k = (id(base), windowed)
        if k not in self._attn_head_tables:
            t = head_width_ranges(base, windowed) if isinstance(base, dict) else head_window_ranges(base, windowed)
            if t is not None:
                t.on(self.device)
            self._attn_head_tables[k] = (base, t)     # (base is held: its id stays its own)
        return self._attn_head_tables[k][1]

    def _layer_table(self, base, layer):
        """The table layer `layer` launches with once calibrated."""
        return self._head_table(base, self._attn_decided[1][layer])

    def _layer_order(self, table, batch):
        """The LaunchOrder a launch of `batch` items with the per-head table `table` takes under attn_window_balance, or None when
        the flag is off: built and uploaded once per (table, batch, policy).  _head_window_finish builds the orders of the
        calibration forward's batch size, so the forwards of that size behind it find theirs here and can be captured.  Any other
        order -- another batch size (a sampler step with fewer passes than the calibration step), or a flag switched on or a
        policy changed after the calibration -- is built on the first EAGER forward that asks for it; inside a stream capture a
        missing order is an error, not an upload.  attn_window_order_build_seconds adds up the host time spent here."""
        policy = _balance_policy(self.attn_window_balance)
        if policy is None:
            return None
        k = (id(table), int(batch), policy)
        if k not in self._attn_orders:
            if _lib._capturing():   # refused before anything is uploaded
                raise _lib.AlgHipError("attn_window_balance: no launch order for batch %d and policy %r has been built yet, and "
                                       "building one uploads a table, which cannot be captured into a graph -- set the flag "
                                       "before the calibration forward and run one eager forward of this batch size first"
                                       % (batch, policy))
            t0 = time.perf_counter()
            order = balanced_order(unit_costs(table, batch, table.heads), policy, heads=table.heads)
            order.on(self.device)
            self._attn_orders[k] = (table, order)     # (the table is held: its id stays its own)
            self.attn_window_order_build_seconds += time.perf_counter() - t0
        return self._attn_orders[k][1]


def call_transformer(transformer, dense, *args, forward=None, calibrate=False, **kw):
    """transformer(*args, **kw) -- or forward(*args, **kw), a bound method of it (CogVideoX: forward_assembled) -- with its frame
    window switched off for this one forward when `dense` (the samplers' dense early steps, `attn_window_dense_steps`); the
    attribute is restored whatever the forward does.

    calibrate (the samplers: the step max(attn_window_dense_steps, 1) - 1): with attn_window > 0 and attn_window_recall > 0 this
    forward is the CALIBRATION forward of an uncalibrated transformer -- dense in output, it measures the recall of every (layer,
    head) and decides the per-head tables the later forwards use; an active step cache is forced to compute it (a hit would skip
    the layers that have to be measured).  Otherwise, and for every other forward, nothing changes."""
    fn = transformer if forward is None else forward
    if (calibrate and getattr(transformer, "attn_window", 0) and getattr(transformer, "attn_window_recall", 0.0) > 0.0
            and not transformer.attn_window_calibrated):
        if _lib._capturing():   # refused before anything is launched
            raise _lib.AlgHipError("attn window: the calibration forward (attn_window_recall > 0, heads not decided yet) cannot be "
                                   "captured into a graph -- the windowed heads are decided on the host from recalls the GPU has "
                                   "just written; run it eagerly (later forwards replay device-resident tables and can be captured)")
        transformer._attn_calibrate = True
        if "cache_keys" in kw:
            kw["cache_force"] = True
        try:
            return fn(*args, **kw)
        finally:
            transformer._attn_calibrate = False
    if not dense or not getattr(transformer, "attn_window", 0):
        return fn(*args, **kw)
    saved = transformer.attn_window
    transformer.attn_window = 0
    # (alg_amd/attn_far.py, alg_amd/attn_pool.py: a dense step is not a missing window)
    far = bool(getattr(transformer, "attn_far_reuse", 0) or getattr(transformer, "attn_far_pool", 0))
    if far:
        transformer._attn_dense_step = True
    try:
        return fn(*args, **kw)
    finally:
        transformer.attn_window = saved
        if far:
            transformer._attn_dense_step = False


def calibration_step(dense_steps):
    """The sampler step whose forwards calibrate the per-head windows: the last dense one, or step 0 when there is none."""
    return max(int(dense_steps), 1) - 1


def ranges_to_mask(kv_ranges):
    """bool [Sq, Skv]: True where the query's block visits the key; [H, Sq, Skv] for a per-head table."""
    if isinstance(kv_ranges, KvRangesHeads):
        return torch.stack([ranges_to_mask(r) for r in kv_ranges.per_head])
    m = torch.zeros(kv_ranges.Sq, kv_ranges.Skv, dtype=torch.bool)
    a = kv_ranges.table
    for j in range(kv_ranges.q_blocks):
        for i in range(kv_ranges.max_ranges):
            b, e = int(a[j, i, 0]), int(a[j, i, 1])
            if e > b:
                m[j * Q_BLOCK:(j + 1) * Q_BLOCK, b:e] = True
    return m
