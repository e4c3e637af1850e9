"""Frame-window self-attention for the video DiTs (opt-in, an extension of this port: the reference attends to all keys).

The primitives are alg_flash_attn_d128_ranges (Wan, HunyuanVideo; attention128_q64.hip) and alg_flash_attn_d64_ranges (CogVideoX;
attention.hip), both in include/alg_hip.h: each block of 256 queries attends to a short list of key ranges, exactly (a masked
softmax with the dense kernel's numerics).  The tokens of a video latent are laid out frame by frame, so "the frames f - W ..
f + W" is ONE contiguous run of keys, and the frame window is a host-side policy on top of the primitives:

    KvRanges             a validated table of key ranges, uploaded once; the only thing _lib.flash_attn_d128_ranges and
                         _lib.flash_attn_d64_ranges take
    frame_window_ranges  the policy: conditioning frames (sink) + the frames within `window` of the block's own + the prompt
    ranges_to_mask       the table as a boolean [Sq, Skv] mask (tests, records)

Only the policy is an approximation; its visual quality on a trained checkpoint is unmeasured (README), so it is off by default.
"""
import numpy as np
import torch

Q_BLOCK = 256      # queries per workgroup of attention128_q64.hip and of attention.hip
KV_ALIGN = 64      # their key tile: a range begins on the dense kernel's tile grid
MAX_RANGES = 4


class KvRanges:
    """A table int32 [q_blocks][max_ranges][2] of (begin, end) key indices for Sq queries and Skv keys, validated on the CPU:
    in each block the used entries come first, sorted and disjoint, begin % 64 == 0, begin < end <= Skv, unused trailing entries
    are (0, 0), and every block has at least one key.  ValueError names the block and the rule."""

    def __init__(self, table, Skv, Sq):
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
        for j in range(q_blocks):
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
            if prev_end is None:
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


def full_ranges(Sq, Skv):
    """The one-range table [0, Skv) for every block: the dense attention through the ranged entry."""
    q_blocks = (Sq + Q_BLOCK - 1) // Q_BLOCK
    t = torch.zeros(q_blocks, 1, 2, dtype=torch.int32)
    t[:, 0, 1] = Skv
    return KvRanges(t, Skv, Sq)


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


def call_transformer(transformer, dense, *args, forward=None, **kw):
    """transformer(*args, **kw) -- or forward(*args, **kw), a bound method of it (CogVideoX: forward_assembled) -- with its frame
    window switched off for this one forward when `dense` (the samplers' dense early steps, `attn_window_dense_steps`); the
    attribute is restored whatever the forward does."""
    fn = transformer if forward is None else forward
    if not dense or not getattr(transformer, "attn_window", 0):
        return fn(*args, **kw)
    saved = transformer.attn_window
    transformer.attn_window = 0
    try:
        return fn(*args, **kw)
    finally:
        transformer.attn_window = saved


def ranges_to_mask(kv_ranges):
    """bool [Sq, Skv]: True where the query's block visits the key."""
    m = torch.zeros(kv_ranges.Sq, kv_ranges.Skv, dtype=torch.bool)
    a = kv_ranges.table
    for j in range(kv_ranges.q_blocks):
        for i in range(kv_ranges.max_ranges):
            b, e = int(a[j, i, 0]), int(a[j, i, 1])
            if e > b:
                m[j * Q_BLOCK:(j + 1) * Q_BLOCK, b:e] = True
    return m
