"""The pooled far-field operator (alg_amd/attn_pool.py) in pure torch, float64, with the tables and operands its tests share.

    pool_ref(x, G, dim)                  bf16(fp32 mean over groups of G along dim, ascending order): what attn_pool.hip computes
    operator_ref(q, k, v, near, pooled, G, unit)
                                         the operator by its formula: ONE softmax over [near keys; pooled keys + log2 G]
    partials_ref(...)                    the same by the route the kernels take: near partial, pooled partial, merge by LSE
    windowed_ref(q, k, v, mask, unit)    masked attention (dense: mask of ones), float64
    tables(layout, hw, G)                (window, near, far, pooled) of the test layouts: 9 frames, window 1
    trained_like_qkv(heads)              q, k, v of block 0 of the small trained-like CogVideoX oracle at 9 x 384 + 10 tokens

q [B, H, Sq, d], k / v [B, H, Skv, d]; near [Sq, Skv] and pooled [Sq, P] boolean masks (attn_window.ranges_to_mask); unit: what
turns q . k into log2-domain scores (1 for the pre-scaled d = 64 form, scale * log2(e) otherwise)."""
import math

import torch

from alg_amd.attn_pool import near_far_pooled
from alg_amd.attn_window import frame_window_ranges, ranges_to_mask

BF = torch.bfloat16
FRAMES, WINDOW, PREFIX, TAIL, TAIL_ROWS = 9, 1, 10, 13, 20
LOG2E = 1.4426950408889634


def pool_ref(x, G, dim):
    """[.., n, ..] -> [.., n // G, ..] bf16: the fp32 sum of every group in ascending order, times 1 / G, one rounding."""
    x = x.movedim(dim, 0)
    P = x.shape[0] // G
    g = x[:P * G].float().reshape(P, G, *x.shape[1:])
    acc = g[:, 0].clone()
    for i in range(1, G):
        acc = acc + g[:, i]
    return (acc * (1.0 / G)).to(BF).movedim(0, dim)


def _scores(q, k, unit):
    return q.double() @ k.double().transpose(-1, -2) * unit


def operator_ref(q, k, v, near, pooled, G, unit):
    """The formula, literally: weights 2^s_j on the near keys and G 2^(q . k_g) on the pooled ones, one normalisation."""
    kp, vp = pool_ref(k, G, 2), pool_ref(v, G, 2)
    P = kp.shape[2]
    s = torch.cat([_scores(q, k, unit).masked_fill(~near, -math.inf),
                   (_scores(q, kp, unit) + math.log2(G)).masked_fill(~pooled[:, :P], -math.inf)], dim=-1)
    w = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    return (w @ torch.cat([v.double(), vp.double()], dim=2)) / w.sum(dim=-1, keepdim=True)


def _partial(q, k, v, mask, unit):
    """(o, lse) of the keys of `mask`; a row without a key: zeros and -inf."""
    s = _scores(q, k, unit).masked_fill(~mask, -math.inf)
    m = s.max(dim=-1, keepdim=True).values
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    w = torch.exp2(s - m0)
    l = w.sum(dim=-1, keepdim=True)
    o = torch.where(l > 0, (w @ v.double()) / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(l))
    return o, (m0 + torch.log2(l)).squeeze(-1)


def partials_ref(q, k, v, near, pooled, G, unit):
    """The operator as near partial + pooled partial, merged by their LSEs with the far one shifted by log2 G (float64)."""
    kp, vp = pool_ref(k, G, 2), pool_ref(v, G, 2)
    o_n, a = _partial(q, k, v, near, unit)
    o_f, f = _partial(q, kp, vp, pooled[:, :kp.shape[2]], unit)
    f = f + math.log2(G)
    m = torch.maximum(a, f)
    wa, wf = torch.exp2(a - m).unsqueeze(-1), torch.exp2(f - m).unsqueeze(-1)
    return (wa * o_n + wf * o_f) / (wa + wf)


def windowed_ref(q, k, v, mask, unit):
    return _partial(q, k, v, mask, unit)[0]


def heads_first(x, H):
    """[B, S, H * d] -> [B, H, S, d]"""
    B, S, D = x.shape
    return x.view(B, S, H, D // H).transpose(1, 2)


def rows_first(x):
    """[B, H, S, d] -> [B, S, H * d]"""
    B, H, S, d = x.shape
    return x.transpose(1, 2).reshape(B, S, H * d)


def window_table(layout, hw):
    """The frame-window table of a test layout: "prefix" (CogVideoX: 10 prompt tokens first), "tail" (HunyuanVideo: 13 prompt keys
    behind the video, 20 prompt rows), "plain" (Wan)."""
    S = FRAMES * hw
    if layout == "prefix":
        return frame_window_ranges(FRAMES, hw, WINDOW, prefix=PREFIX)
    if layout == "tail":
        return frame_window_ranges(FRAMES, hw, WINDOW, tail=(S, S + TAIL), rows=S + TAIL_ROWS)
    return frame_window_ranges(FRAMES, hw, WINDOW)


def tables(layout, hw, G, pooled_skv=None):
    w = window_table(layout, hw)
    return (w,) + near_far_pooled(w, G, pooled_skv)


def masks(layout, hw, G):
    """(window, near, pooled) masks: [Sq, Skv], [Sq, Skv], [Sq, Skv // G]"""
    w, near, _, pooled = tables(layout, hw, G)
    return ranges_to_mask(w), ranges_to_mask(near), ranges_to_mask(pooled)


_QKV = {}


def trained_like_qkv(heads=(0, 3)):
    """(q, k, v) bf16 [1, len(heads), S, 64], S = 10 + 9 x 384: the attention operands of block 0 of the small trained-like CogVideoX
    oracle (fp32, CPU) on a 9-frame 32 x 48 latent, q carrying scale * log2(e) as the d = 64 ranged entries want it.  Computed
    once and shared: leave it unchanged."""
    if heads not in _QKV:
        from helpers.trained_like_cases import COG_SMALL
        from helpers.trained_like import trained_like
        from oracle import dit_oracle
        kw = dict(COG_SMALL, sample_width=48, sample_height=32, sample_frames=4 * FRAMES - 3)
        ocfg = dit_oracle.DiTConfig(**kw)
        w32 = trained_like(dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True))
        w32 = {k: v.to(BF).float() for k, v in w32.items()}
        g = torch.Generator().manual_seed(1)
        hs = torch.randn(1, FRAMES, kw["in_channels"], 32, 48, generator=g).to(BF).float()
        ehs = torch.randn(1, PREFIX, kw["text_embed_dim"], generator=g).to(BF).float()
        got = {}
        dit_oracle.dit_forward(ocfg, w32, hs, ehs, torch.tensor([999]), dit_oracle.rope_tables(ocfg, 32 * 8, 48 * 8, FRAMES), collect=got)
        idx = list(heads)
        q = (got["q_0"][:, idx] * (LOG2E / math.sqrt(64.0))).to(BF)
        _QKV[heads] = (q, got["k_0"][:, idx].to(BF), got["v_0"][:, idx].to(BF))
    return _QKV[heads]


def rel_l2(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


def window_vs_pool_errors(G, heads=(0, 3)):
    """(window-only error, pooled error) of the LATENT rows against the dense attention, relative L2, float64, on
    trained_like_qkv: the inequality the GPU test asserts on the kernels' output is first established here."""
    q, k, v = trained_like_qkv(heads)
    wm, near, pooled = masks("prefix", 384, G)
    dense = windowed_ref(q, k, v, torch.ones_like(wm), 1.0)[:, :, 256:]
    win = windowed_ref(q, k, v, wm, 1.0)[:, :, 256:]
    pool = operator_ref(q, k, v, near, pooled, G, 1.0)[:, :, 256:]
    return rel_l2(win, dense), rel_l2(pool, dense)
