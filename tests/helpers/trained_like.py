"""A second, harsher synthetic weight regime: what a trained video DiT checkpoint looks like to the kernels.

Every other forward / sampler test runs on Gaussian matrices, norm gains of 1 +- 0.1 and biases of a few hundredths.  In that
regime every attention score stays near +-11.5 log2 units, every row of an activation has elements of one size and every norm
gain is about one.  `trained_like(state_dict)` rewrites a `name -> tensor` state dict of any of the three DiTs (the diffusers
names that `oracle.dit_oracle`, `oracle.wan_oracle` / `alg_amd.transformer_wan` and `oracle.hy_oracle` /
`alg_amd.transformer_hunyuan_video` share) into one with

  * QK-norm gains log-normal around `qk_gain` (scores of tens to hundreds of log2 units), and for LayerNorm QK-norms
    (CogVideoX) biases with a component SHARED between norm_q.bias and norm_k.bias: tokens that are not rotated (text) get a
    large common score offset, rotated ones (video) a position-dependent one; RMSNorm QK-norms (Wan, HunyuanVideo) have no
    bias, there the shared component goes into the to_q / to_k biases of the rotated projections;
  * stream-norm gains log-normal (sigma 0.5, clamped at 4), biases of block linears and norms of O(1);
  * a few MASSIVE channels of the residual stream, the same indices for every token, injected through the embedders' biases;
  * a per-tensor scale in [1/2, 2] on every block matrix and a handful of output channels of to_q / to_k / ff proj at 8 x.

Same keys, shapes and dtypes; every tensor is drawn from a CPU generator seeded by (seed, tensor name) alone, so the result
does not depend on dict order or device.  `level` in [0, 1] interpolates every ingredient between "unchanged" (0: the input's
tensors are returned as they are) and the defaults (1); each ingredient has its own switch so that a failing forward can be
bisected.

The defaults were chosen on the CPU oracle (tests/test_trained_like_cpu.py asserts the conditions; the regime they produce is
recorded in profiles/trained_like_regime.json); each says which condition set it."""
import math
import re
import zlib

import torch

# qk_gain: the median of the first KV tile's maximum has to sit near the kernel's snap threshold of 64 log2 units so that both
# kept and snapped offsets occur in one launch (d = 64: scores scale with gain^2 * 11.5)
QK_GAIN = 3.0
QK_GAIN_SIGMA = 0.5          # spread over the head channels (a few dominant ones): at 0.35 block 0 had 1-2 bail-out rows, here > 100
QK_GAIN_CLAMP = 16.0
# RMSNorm QK-norms (Wan, HunyuanVideo, d = 128) have no bias: the shared component goes into the to_q / to_k biases of the rotated
# (self / joint attention, latent stream) projections instead, and the gain's median is set by the same conditions at d = 128
QK_GAIN_RMS = 3.0
QK_PROJ_BIAS_SHARED = 2.0
HEAD_SPREAD = 2.5            # scores of the weakest / strongest head at 1/6 and 6 x the median head's: both sides of 64, and bail-outs
# shared q / k bias component: lifts text-text scores by |b|^2 / sqrt(d) * log2(e) and, through RoPE, makes a video row's
# scores fall with distance -- what produces rows whose later tiles tower over the first one (bail-out candidates)
QK_BIAS_SHARED = 2.0
QK_BIAS_OWN = 0.3
NORM_GAIN_SIGMA = 0.5        # gains of about 0.4 to 2.7, a tail to the clamp
NORM_GAIN_CLAMP = 4.0
BIAS_STD = 0.5               # O(1); the floors of both execution modes stay under a quarter with it
# x the embedder's own output RMS (the embedded stream then has max / RMS(other channels) of about 100, the top of the 50-100 x
# range); the smallest round value that keeps the ratio >= 30 AFTER block 0's updates at every test shape (1024-wide: 31)
MASSIVE_FACTOR = 135.0
# Wan's text embedder feeds no residual stream but the cross-attention context, whose values reach the stream through an ungated
# to_out: at 100 x they become a token-constant component of RMS 16 that buries the massive channels (ratio 7.5 after block 0)
MASSIVE_FACTOR_CONTEXT = 10.0
MASSIVE_CHANNELS = 3         # trained DiTs show two to four
SPREAD = 2.0                 # per-tensor factor in [1 / SPREAD, SPREAD]
HOT_CHANNELS = 4             # output channels of to_q / to_k / ff proj ...
HOT_FACTOR = 8.0             # ... at this multiple (what per-output-channel e4m3 weight scales exist for)

_QK_GAIN = re.compile(r"\.(norm_q|norm_k|norm_added_q|norm_added_k)\.weight$")
_QK_BIAS = re.compile(r"\.(norm_q|norm_k)\.bias$")
_QK_PROJ_BIAS = re.compile(r"\.(attn1|attn)\.to_(q|k)\.bias$")
_BLOCK = re.compile(r"^(transformer_blocks|single_transformer_blocks|blocks)\.\d+\.|^context_embedder\.token_refiner\.")
_HOT = re.compile(r"\.(to_q|to_k|add_q_proj|add_k_proj)\.weight$|\.ffn?(_context)?\.net\.0\.proj\.weight$")
# (embedder bias, the weight whose fan-in and spread give that embedder's output RMS), per model
_EMBEDDERS = (("patch_embed.proj.bias", "patch_embed.proj.weight"), ("patch_embed.text_proj.bias", "patch_embed.text_proj.weight"),
              ("patch_embedding.bias", "patch_embedding.weight"),
              ("condition_embedder.text_embedder.linear_2.bias", "condition_embedder.text_embedder.linear_2.weight"),
              ("x_embedder.proj.bias", "x_embedder.proj.weight"), ("context_embedder.proj_in.bias", "context_embedder.proj_in.weight"))
_CONTEXT_ONLY = ("condition_embedder.text_embedder.linear_2.bias",)
INGREDIENTS = ("qk_gains", "qk_biases", "norm_gains", "biases", "massive", "spread")


def _gen(seed, name, tag=""):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(("%d|%s|%s" % (seed, name, tag)).encode()))


def _randn(shape, g):
    return torch.randn(tuple(shape), generator=g, dtype=torch.float32)


def is_norm_gain(name, t):
    """A 1-D `.weight` that is not a QK-norm: the stream norms (norm1.norm, norm2.norm, norm_final, norm_out.norm, Wan's
    norm2, the refiner's and the image embedder's norms)."""
    return name.endswith(".weight") and t.dim() == 1 and not _QK_GAIN.search(name)


def is_block_or_norm_bias(name, t, sd):
    """Biases of the block linears and of every stream norm (not the QK-norm biases, not the embedders')."""
    if not name.endswith(".bias") or _QK_BIAS.search(name):
        return False
    w = sd.get(name[:-5] + ".weight")
    return bool(_BLOCK.match(name)) or (w is not None and w.dim() == 1)


def massive_channels(sd, seed, count=MASSIVE_CHANNELS):
    """The channel indices and signs of the massive activations: a function of (seed, stream width) only."""
    for bias, _ in _EMBEDDERS:
        if bias in sd:
            D = sd[bias].numel()
            g = _gen(seed, "massive", str(D))
            idx = torch.randperm(D, generator=g)[:count]
            sign = torch.where(torch.rand(count, generator=g) < 0.5, -1.0, 1.0)
            return idx, sign
    return torch.empty(0, dtype=torch.long), torch.empty(0)


def trained_like(sd, seed=0, level=1.0, qk_gains=True, qk_biases=True, norm_gains=True, biases=True, massive=True, spread=True,
                 qk_gain=QK_GAIN, qk_gain_sigma=QK_GAIN_SIGMA, qk_bias_shared=QK_BIAS_SHARED, qk_bias_own=QK_BIAS_OWN,
                 qk_gain_rms=QK_GAIN_RMS, qk_proj_bias_shared=QK_PROJ_BIAS_SHARED, head_spread=HEAD_SPREAD,
                 head_dim=128,
                 norm_gain_sigma=NORM_GAIN_SIGMA, bias_std=BIAS_STD, massive_factor=MASSIVE_FACTOR,
                 massive_factor_context=MASSIVE_FACTOR_CONTEXT,
                 massive_count=MASSIVE_CHANNELS, spread_range=SPREAD, hot_channels=HOT_CHANNELS, hot_factor=HOT_FACTOR):
    """Return a new dict: `sd` in the trained-like regime (see the module text).  `sd` and its tensors are not modified."""
    out = dict(sd)
    if level == 0:
        return out
    lv = float(level)
    emb = {b: w for b, w in _EMBEDDERS if b in sd and w in sd}
    midx, msign = massive_channels(sd, seed, massive_count)
    rms_qk = not any(_QK_BIAS.search(n) for n in sd)          # RMSNorm QK-norms (Wan, HunyuanVideo): no bias of their own
    if rms_qk and qk_gain_rms is not None:
        qk_gain = qk_gain_rms
    for name, t in sd.items():
        new = None
        if _QK_GAIN.search(name):
            if qk_gains:
                g = _gen(seed, name)
                gain = torch.exp(lv * (math.log(qk_gain) + qk_gain_sigma * _randn(t.shape, g)))
                heads = t.numel() // head_dim
                if heads > 1 and t.numel() % head_dim == 0:
                    # one gain vector over all heads (Wan): a ladder of per-head factors from 1 / head_spread to head_spread,
                    # the same for norm_q and norm_k of a block, so that one launch has heads on either side of the threshold
                    ladder = head_spread ** (lv * (2.0 * torch.arange(heads, dtype=torch.float32) / (heads - 1) - 1.0))
                    perm = torch.randperm(heads, generator=_gen(seed, re.sub(r"norm_(added_)?[qk]\.weight$", "", name), "heads"))
                    gain = (gain.view(heads, head_dim) * ladder[perm][:, None]).reshape(t.shape)
                new = gain.clamp(1.0 / QK_GAIN_CLAMP, QK_GAIN_CLAMP)
        elif _QK_BIAS.search(name):
            if qk_biases:
                shared = _randn(t.shape, _gen(seed, re.sub(r"norm_[qk]\.bias$", "norm_qk.bias", name), "shared"))
                new = lv * (qk_bias_shared * shared + qk_bias_own * _randn(t.shape, _gen(seed, name, "own")))
        elif rms_qk and _QK_PROJ_BIAS.search(name):
            if qk_biases:
                shared = _randn(t.shape, _gen(seed, re.sub(r"to_[qk]\.bias$", "to_qk.bias", name), "shared"))
                new = lv * (qk_proj_bias_shared * shared + bias_std * _randn(t.shape, _gen(seed, name, "own")))
        elif is_norm_gain(name, t):
            if norm_gains:
                gain = torch.exp(lv * norm_gain_sigma * _randn(t.shape, _gen(seed, name)))
                new = gain.clamp(1.0 / NORM_GAIN_CLAMP, NORM_GAIN_CLAMP)
        elif name in emb:
            if massive and midx.numel():
                w = sd[emb[name]].float()
                rms = w.std().item() * math.sqrt(w[0].numel())         # the embedder's output RMS on unit-variance inputs
                new = t.float().cpu().clone()
                ctx = massive_factor_context if name in _CONTEXT_ONLY else massive_factor
                new[midx] = msign * (lv * ctx * rms)
        elif is_block_or_norm_bias(name, t, sd):
            if biases:
                new = (1.0 - lv) * t.float().cpu() + lv * bias_std * _randn(t.shape, _gen(seed, name))
        elif _BLOCK.match(name) and name.endswith(".weight") and t.dim() >= 2:
            if spread:
                g = _gen(seed, name)
                f = spread_range ** (lv * (2.0 * torch.rand(1, generator=g).item() - 1.0))
                new = t.float() * f
                if _HOT.search(name):
                    hot = torch.randperm(t.shape[0], generator=g)[:hot_channels].to(t.device)
                    new[hot] = new[hot] * hot_factor ** lv
        if new is not None:
            out[name] = new.to(device=t.device, dtype=t.dtype)
    return out


def attention_regime(q, k, snaps, tile=64, snap_below=64.0, limit_log2=80.0):
    """Which softmax paths of the flash-attention kernels one sample's operands reach.  q, k [heads, S, d] as the kernel gets
    them (QK-normed, rotated); scores in log2 units (q.k / sqrt(d) * log2 e), keys in tiles of `tile` as the kernels walk them.

    The kernels keep a LAZY running offset m: the first tile sets it to that tile's row maximum -- snapped to zero by the d = 64
    kernel when the maximum lies in (-snap_below, snap_below) (`snaps=True`, attention.hip softmax_tile_zero) -- and a later
    tile only raises it (the exact path: a bail-out of the pipelined statement) when its row sum of 2^(score - m) reaches
    2^limit_log2 (ALG_LAZY_SUM_LIMIT).  Returns the fraction of (head, query) rows with |first-tile max| >= / < snap_below, the
    number of rows with at least one bail-out after the first tile, and the extreme first-tile maxima and scores."""
    H, S, d = q.shape
    s = (q.double() @ k.double().transpose(-1, -2)) * (math.log2(math.e) / math.sqrt(d))         # [H, S, S]
    m0 = s[..., :tile].max(dim=-1).values
    kept = m0.abs() >= snap_below
    m = torch.where(kept, m0, torch.zeros_like(m0)) if snaps else m0.clone()
    bailed = torch.zeros_like(kept)
    events = 0
    for t0 in range(tile, S, tile):
        st = s[..., t0:t0 + tile]
        over = torch.logsumexp(st * math.log(2.0), dim=-1) / math.log(2.0) - m >= limit_log2
        events += int(over.sum())
        bailed |= over
        m = torch.where(over, torch.maximum(m, st.max(dim=-1).values), m)
    rows = float(kept.numel())
    return {"rows": int(rows), "kept_fraction": float(kept.sum()) / rows, "snapped_fraction": float((~kept).sum()) / rows,
            "bail_out_rows": int(bailed.sum()), "bail_out_events": events, "first_tile_max_min": float(m0.min()),
            "first_tile_max_max": float(m0.max()), "score_min": float(s.min()), "score_max": float(s.max()),
            "kv_tiles": (S + tile - 1) // tile}


def massive_ratio(x, seed=0, count=MASSIVE_CHANNELS):
    """Residual stream x [B, S, D]: per token, the largest channel magnitude over the RMS of the OTHER channels (the `count`
    largest left out: over all D channels the ratio cannot exceed sqrt(D / count), 13 at the 512-wide test models, whatever
    the weights), and over the RMS of all channels.  Returns the two minima over tokens."""
    a = x.double().abs()
    top = a.topk(count, dim=-1).values
    rest = ((a.pow(2).sum(-1) - top.pow(2).sum(-1)) / (x.shape[-1] - count)).sqrt()
    return float((top[..., 0] / rest).min()), float((top[..., 0] / a.pow(2).mean(-1).sqrt()).min())
