"""Opt-in step cache ("first-block cache") of the CogVideoX and Wan DiTs -- an extension, the reference has none.

Block 0 is 1 / L of a forward, and how much its residual r = x1 - x0 moved since the last forward predicts how much the whole
forward moved.  While it barely moved, blocks 1 .. L-1 are replaced by the residual they produced on the last computed
forward (the "tail", x_final - x1):

    keep <- x                                   copy in front of block 0
    block 0                                     bf16 or e4m3, whatever the model runs
    probe, once per sample (alg_step_cache_probe): r1[key] <- bf16(x - keep), keep <- x,
                                                (a, b) = (sum |r - r_prev|, sum |r_prev|) over the video tokens
    the sums go to the host (the one stream synchronisation of an active forward) and `decide` rules:
      hit    x[n] <- bf16(x[n] + tail[key])                    then the head
      miss   blocks 1 .. L-1, tail[key] <- bf16(x[n] - keep[n]) then the head: bit for bit the cache-off forward

A sample's cache entry is keyed by the ROLE of its pass ("uncond_init" / "uncond" / "cond", with the video's index when a call
carries several), not by its batch row: the ALG loop runs 3 passes per step early and 2 later, and "uncond" / "cond" carry over.
One decision per forward, over all its rows.

`StepCache.decide` and the bookkeeping around it are plain host code (tests/test_step_cache_cpu.py); everything that touches
the GPU is a launch of libalg_hip.so or a copy.
"""
from __future__ import annotations

import math

import torch

from . import _lib

BF = torch.bfloat16


class StepCache:
    """The cache of ONE transformer: the rule, its counters, and (from the first active forward on) the buffers."""

    def __init__(self, threshold=0.0, max_consecutive=0):
        self.threshold = float(threshold)            # hit needs a < threshold * b for every key
        self.max_consecutive = int(max_consecutive)  # hits in a row before a computed forward is due; 0 = no cap
        self.stats = []                              # one record per active forward
        self._valid = set()                          # keys whose r1 and tail come from forwards since the last reset
        self._consecutive = 0
        # device state: nothing is allocated before the first active forward
        self._shape = None                           # (S, D)
        self.r1, self.tail = {}, {}                  # key -> [S, D] bf16
        self.keep = None                             # [N, S, D] bf16: x0 in front of block 0, x1 behind the probe
        self._work = self._sums = self._host = None
        self._pending = None

    # ---- the rule (no GPU) -------------------------------------------------------------------------------------------
    def reset(self):
        """Forget every key (the buffers stay): the next forward is computed."""
        self._valid.clear()
        self._consecutive = 0
        del self.stats[:]
        self._pending = None

    def decide(self, sums_per_key, keys, force=False):
        """One decision for a forward whose samples carry `keys`.  `sums_per_key`: the probe's (a, b) per key -- a mapping, or a
        sequence in the order of `keys`.  Hit iff every key has a valid entry, every (a, b) is finite with b > 0 and
        a < threshold * b (in double), `force` is false and fewer than `max_consecutive` hits came in a row.  Appends the
        record to `stats` ("rel" is a / b, infinity where the key has no valid entry or b is 0) and counts the hit.  A miss
        takes the keys' entries out of use until `mark_valid` (the computed forward has finished) puts them back."""
        keys = list(keys)
        pairs = [sums_per_key[k] for k in keys] if isinstance(sums_per_key, dict) else list(sums_per_key)
        if len(pairs) != len(keys):
            raise ValueError("decide: %d keys, %d pairs of sums" % (len(keys), len(pairs)))
        ok, rel = bool(keys), []
        for key, (a, b) in zip(keys, pairs):
            a, b = float(a), float(b)
            fine = key in self._valid and math.isfinite(a) and math.isfinite(b) and b > 0.0
            rel.append(a / b if fine else (float("nan") if a != a or b != b else float("inf")))
            ok = ok and fine and a < self.threshold * b
        capped = self.max_consecutive > 0 and self._consecutive >= self.max_consecutive
        hit = ok and not force and not capped
        self._consecutive = self._consecutive + 1 if hit else 0
        if not hit:                                  # their tails are about to be rewritten: valid again once `end` has run
            self._valid.difference_update(keys)
        self.stats.append({"keys": keys, "rel": rel, "hit": hit, "forced": bool(force)})
        return hit

    def mark_valid(self, keys):
        """After a computed forward: r1 and tail of these keys are current."""
        self._valid.update(keys)

    # ---- the launches ----------------------------------------------------------------------------------------------------
    def _buffers(self, x, keys):
        N, S, D = x.shape
        if self._shape != (S, D):                    # another sequence: nothing cached applies
            self._shape = (S, D)
            self.r1, self.tail, self.keep = {}, {}, None
            self._valid.clear()
            self._work = torch.empty(_lib.step_cache_workspace_bytes(S, D), dtype=torch.uint8, device=x.device)
        if self.keep is None or self.keep.shape[0] < N:
            self.keep = torch.empty(N, S, D, dtype=BF, device=x.device)
            self._sums = torch.zeros(N, 2, dtype=torch.float64, device=x.device)
            self._host = torch.zeros(N, 2, dtype=torch.float64).pin_memory()
        for k in keys:
            if k not in self.r1:                     # zeros: a first probe reads b == 0, never uninitialised memory
                self.r1[k] = torch.zeros(S, D, dtype=BF, device=x.device)
                self.tail[k] = torch.zeros(S, D, dtype=BF, device=x.device)

    def begin(self, x, keys, force, tok0, tok_rows):
        """In front of block 0: x [N, S, D] bf16 is the residual stream, keys one per sample."""
        keys = list(keys)
        if _lib._capturing():
            raise _lib.AlgHipError("step cache: an active forward (step_cache > 0 with cache_keys) cannot be captured into a "
                                   "graph -- its hit / miss decision is taken on the host from sums the GPU has just written; "
                                   "set step_cache = 0 or pass no cache_keys under capture")
        if len(keys) != x.shape[0] or len(set(keys)) != len(keys):
            raise ValueError("step cache: cache_keys must name each of the %d samples once, got %r" % (x.shape[0], keys))
        if x.dtype != BF or not x.is_contiguous():
            raise _lib.AlgHipError("step cache: the residual stream must be a contiguous bfloat16 tensor")
        self._buffers(x, keys)
        self.keep[:x.shape[0]].copy_(x)
        self._pending = (keys, bool(force), int(tok0), int(tok_rows))

    def after_block0(self, x):
        """Behind block 0: probe every sample, fetch the sums, decide.  On a hit x already holds x1 + tail when this returns."""
        keys, force, tok0, tok_rows = self._pending
        N, S, D = x.shape
        for n, k in enumerate(keys):
            _lib.step_cache_probe(self.keep[n], x[n], self.r1[k], S, D, tok0, tok_rows, self._work, self._sums[n])
        self._host[:N].copy_(self._sums[:N], non_blocking=True)
        torch.cuda.current_stream(x.device).synchronize()
        hit = self.decide([(a, b) for a, b in self._host[:N].tolist()], keys, force)
        if hit:
            for n, k in enumerate(keys):
                _lib.lincomb([(1.0, x[n]), (1.0, self.tail[k])], BF, out=x[n])
            self._pending = None
        return hit

    def end(self, x):
        """Behind the last block of a computed forward: tail[key] <- bf16(x[n] - x1[n])."""
        if self._pending is None:
            return
        keys = self._pending[0]
        for n, k in enumerate(keys):
            _lib.lincomb([(1.0, x[n]), (-1.0, self.keep[n])], BF, out=self.tail[k])
        self.mark_valid(keys)
        self._pending = None


class StepCacheHost:
    """What a transformer with a step cache carries: the switches, the record, the reset.  `step_cache` = 0.0 is off: such a
    forward runs the launches of a model without this class, allocates nothing and records nothing."""

    step_cache = 0.0                  # threshold on sum |r - r_prev| / sum |r_prev| of block 0's residual; 0 = off
    step_cache_max_consecutive = 0    # at most this many skipped forwards in a row; 0 = no cap
    _step_cache_obj = None

    def _step_cache_state(self):
        if self._step_cache_obj is None:
            self._step_cache_obj = StepCache()
        return self._step_cache_obj

    @property
    def step_cache_stats(self):
        """One record per active forward since the last reset: {"keys", "rel": [a / b ...], "hit", "forced"}."""
        return self._step_cache_state().stats

    def reset_step_cache(self):
        """Invalidate every key (a new video); the buffers are kept."""
        self._step_cache_state().reset()

    def _step_cache_begin(self, x, cache_keys, cache_force, tok0, tok_rows):
        """The active cache of this forward, armed in front of block 0 -- or None (off: nothing happens)."""
        if cache_keys is None or not self.step_cache > 0.0:
            return None
        sc = self._step_cache_state()
        sc.threshold, sc.max_consecutive = float(self.step_cache), int(self.step_cache_max_consecutive)
        self._timed("step_cache", sc.begin, x, cache_keys, cache_force, tok0, tok_rows)
        return sc


def pass_keys(n_pass, batch):
    """Cache keys of a CFG batch laid out pass-major ([pass 0 of every video | pass 1 ... ]): the last two passes are "uncond"
    and "cond", the extra first pass of a 3-pass step is "uncond_init", a run without CFG has "cond" alone."""
    roles = ("uncond_init", "uncond", "cond")[3 - n_pass:]
    if not 1 <= n_pass <= 3:
        raise ValueError("pass_keys: 1 to 3 passes, got %d" % n_pass)
    return [role if batch == 1 else (role, b) for role in roles for b in range(batch)]


def active(transformer):
    """True when the pipeline has to drive the cache of this transformer (stand-ins without the attribute: never)."""
    tau = getattr(transformer, "step_cache", 0.0)
    return isinstance(tau, (int, float)) and tau > 0.0
