"""Frame-window self-attention for the head_dim 128 video DiTs (opt-in, an extension of this port: the reference attends to all keys).

The primitive is alg_flash_attn_d128_ranges (include/alg_hip.h, attention128_q64.hip): each block of 256 queries attends to a
short list of key ranges, exactly (a masked softmax with the dense kernel's numerics).  The tokens of a video latent are laid out
frame by frame, so "the frames f - W .. f + W" is ONE contiguous run of keys, and the frame window is a host-side policy on top
of the primitive:

    KvRanges             a validated table of key ranges, uploaded once; the only thing _lib.flash_attn_d128_ranges takes
    frame_window_ranges  the policy: conditioning frames (sink) + the frames within `window` of the block's own + the prompt
    ranges_to_mask       the table as a boolean [Sq, Skv] mask (tests, records)

Only the policy is an approximation; its visual quality on a trained checkpoint is unmeasured (README), so it is off by default.
"""
import numpy as np
import torch

Q_BLOCK = 256      # queries per workgroup of attention128_q64.hip
KV_ALIGN = 64      # its key tile: a range begins on the dense kernel's tile grid
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


def frame_window_ranges(frames, tokens_per_frame, window, sink_frames=1, tail=None, rows=None):
    """The frame-window policy as a KvRanges, or None when it is the dense attention (every block sees every key).

    The keys are `frames` latent frames of `tokens_per_frame` (hw) tokens, frame by frame, optionally followed by other keys of
    which tail = (begin, end) are to be seen by everybody (HunyuanVideo: the sample's valid prompt keys [S, S + valid)); Skv is
    tail's end, or frames * hw.  The queries are rows 0 .. rows - 1 (default frames * hw) in the same order.  A block of 256
    queries covering the latent frames fa .. fb gets
        the sink    [0, sink_frames * hw),
        the window  [(fa - window) * hw, (fb + window + 1) * hw) clipped to the video,
        the tail,
    begins rounded DOWN to a multiple of 64 (a superset: always safe), touching or overlapping ranges merged.  A block that
    holds any row >= frames * hw (prompt queries, and the block that straddles the boundary) gets the single full range."""
    F, hw, W, sink = int(frames), int(tokens_per_frame), int(window), int(sink_frames)
    if F < 1 or hw < 1 or W < 0 or sink < 0:
        raise ValueError("frame_window_ranges: frames=%d tokens_per_frame=%d window=%d sink_frames=%d" % (F, hw, W, sink))
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
        want = sorted((b - b % KV_ALIGN, e) for b, e in want)
        merged = [list(want[0])]
        for b, e in want[1:]:
            if b <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([b, e])
        per_block.append([tuple(m) for m in merged])
    if all(r == [(0, Skv)] for r in per_block):
        return None
    max_ranges = max(len(r) for r in per_block)
    t = torch.zeros(q_blocks, max_ranges, 2, dtype=torch.int32)
    for j, r in enumerate(per_block):
        for i, (b, e) in enumerate(r):
            t[j, i, 0], t[j, i, 1] = b, e
    return KvRanges(t, Skv, Sq)


def call_transformer(transformer, dense, **kw):
    """transformer(**kw), with its frame window switched off for this one forward when `dense` (the samplers' dense early
    steps, `attn_window_dense_steps`); the attribute is restored whatever the forward does."""
    if not dense or not getattr(transformer, "attn_window", 0):
        return transformer(**kw)
    saved = transformer.attn_window
    transformer.attn_window = 0
    try:
        return transformer(**kw)
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
