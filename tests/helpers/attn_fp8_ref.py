"""Eager restatement of the e4m3 self-attention scheme of alg_flash_attn_d128_fp8 (alg_amd/csrc/attention128_fp8.hip), in plain
torch with torch.float8_e4m3fn, on whatever device its operands live.  It is the floor the kernel and the models built on it are
held to (tests/_parity.py), and the statement of the scheme a reader can run:

  operands   Q: one fp32 scale per (batch, token, head), amax / 448 of the 128-wide head vector (alg_quantize_fp8_rows on rows of 128)
             K: one fp32 scale per (batch, head)  (alg_quantize_fp8_khead: amax / 448 over the head's S x 128 values, or a given bound)
             V: one fp32 scale per (batch, head, channel) row of V^T (alg_quantize_fp8_vt), columns in the kernel's key order
             value = e4m3(clamp(x * (1 / scale), -448, 448))           -- clamp FIRST: torch turns 500 into NaN
  scores     s = sum_d q8 k8 in fp32 (products of e4m3 values are exact), c = scale * log2(e) * q_scale * k_scale per query
  softmax    per 64-key tile and 32-query block: p = exp2(s c - m c + 3) against the block rows' CURRENT offsets m (P scale 2^3);
             a lane owns one query and the keys with (key >> 2) & 1 == h2: if ANY lane sum of the block is not <= 448 (inf / NaN on
             the first tile) the exact path runs for the whole block -- m = max(m, tile max), O and l rescaled by exp2((m_old - m) c),
             p recomputed (every p <= 8).  l += fp32 sum of the UNROUNDED p;  O += e4m3(p) v8 in fp32
  output     bf16(O * v_scale / l)
"""
import math

import torch

F8 = torch.float8_e4m3fn
E4M3_MAX = 448.0
P_SHIFT = 3.0
KVB = 64
QBLOCK = 32


def e4m3(x):
    """Round fp32 to OCP e4m3 and back; saturating (the kernels clamp in front of v_cvt_pk_fp8_f32)."""
    return x.float().clamp(-E4M3_MAX, E4M3_MAX).to(F8).float()


def _scale_of(amax):
    one = torch.ones_like(amax)
    return torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=amax.device), one)


def quantize_rows(x):
    """x [..., 128] (bf16 or fp32 holding bf16 values) -> (e4m3 values as fp32, scale [...])."""
    x = x.float()
    sc = _scale_of(x.abs().amax(dim=-1))
    return e4m3(x * (1.0 / sc)[..., None]), sc


def quantize_khead(k, scale=None):
    """k [B, S, H, 128] -> (e4m3 values as fp32, scale [B, H]); scale given: a bound known beforehand."""
    k = k.float()
    sc = _scale_of(k.abs().amax(dim=(1, 3))) if scale is None else scale.float()
    return e4m3(k * (1.0 / sc)[:, None, :, None]), sc


def quantize_vt(v):
    """v [B, S, H, 128] -> (e4m3 values as fp32 [B, S, H, 128], scale [B, H, 128]): one scale per V^T row."""
    v = v.float()
    sc = _scale_of(v.abs().amax(dim=1))
    return e4m3(v * (1.0 / sc)[:, None]), sc


def vt_position(s):
    """Column of V^T at which the kernel expects key s: 64-key tiles, inside a tile key 32 sub + 8 g + 4 h2 + j sits at
    32 h2 + 16 sub + 4 g + j (the order the S^T accumulator hands a lane its probabilities in)."""
    t, r = s // 64, s % 64
    sub, g, h2, j = r // 32, (r // 8) % 4, (r // 4) % 2, r % 4
    return 64 * t + 32 * h2 + 16 * sub + 4 * g + j


def pack_vt(v8, pad_to=None):
    """e4m3 values [B, S, H, 128] -> V^T [B, H * 128, pad] in the kernel's key order, padding columns zero."""
    B, S, H, D = v8.shape
    pad = pad_to or (S + 63) // 64 * 64
    out = torch.zeros(B, H * D, pad, dtype=v8.dtype, device=v8.device)
    pos = torch.tensor([vt_position(s) for s in range(S)], device=v8.device)
    out[:, :, pos] = v8.permute(0, 2, 3, 1).reshape(B, H * D, S)
    return out


def attention_f64(q, k, v, scale):
    """softmax(scale q k^T) v in float64; q [B, Sq, H, D], k / v [B, Skv, H, D] -> [B, Sq, H, D]."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


def attention_fp8(q8, q_scale, k8, k_scale, v8, v_scale, scale, stats=None):
    """The scheme above.  q8 [B, Sq, H, 128], k8 / v8 [B, Skv, H, 128]: e4m3 values held as fp32; q_scale [B, Sq, H], k_scale
    [B, H], v_scale [B, H, 128].  Returns bf16 [B, Sq, H, 128].  stats (dict): counts "tiles" and "exact" (block, tile) steps and
    records "p_max", the largest value handed to the e4m3 conversion."""
    B, Sq, H, D = q8.shape
    Skv = k8.shape[1]
    dev = q8.device
    f32 = torch.float32
    c = (torch.tensor(scale * 1.4426950408889634, dtype=f32, device=dev) * q_scale.float() * k_scale.float()[:, None, :])
    c = c.permute(0, 2, 1).contiguous()                                   # [B, H, Sq]
    qh = q8.float().permute(0, 2, 1, 3).contiguous()                      # [B, H, Sq, D]
    kh = k8.float().permute(0, 2, 1, 3).contiguous()
    vh = v8.float().permute(0, 2, 1, 3).contiguous()
    m = torch.full((B, H, Sq), -math.inf, dtype=f32, device=dev)          # running offset, in raw score units
    l = torch.zeros(B, H, Sq, dtype=f32, device=dev)
    O = torch.zeros(B, H, Sq, D, dtype=f32, device=dev)
    nblk = (Sq + QBLOCK - 1) // QBLOCK
    blk = torch.arange(Sq, device=dev) // QBLOCK
    for t0 in range(0, Skv, KVB):
        t1 = min(t0 + KVB, Skv)
        s = qh @ kh[:, :, t0:t1].transpose(-1, -2)                        # [B, H, Sq, n]
        h2 = ((torch.arange(t0, t1, device=dev) >> 2) & 1).bool()
        x = s * c[..., None]

        def probs(off):
            return torch.exp2(x + off[..., None])

        p = probs(P_SHIFT - m * c)
        lane = torch.stack([(p * (~h2)).sum(-1), (p * h2).sum(-1)], dim=-1)          # [B, H, Sq, 2]: a lane's 32 values
        bad = ~(lane <= E4M3_MAX)                                                   # also NaN
        bad = bad.any(-1)                                                           # [B, H, Sq]
        trig = torch.zeros(B, H, nblk, dtype=torch.int32, device=dev).index_add_(2, blk, bad.int()) > 0
        trig_q = trig[:, :, blk]                                                    # back to queries
        if trig_q.any():
            m_new = torch.maximum(m, s.amax(-1))
            m_new = torch.where(trig_q, m_new, m)
            alpha = torch.where(trig_q, torch.exp2((m - m_new) * c), torch.ones_like(m))
            m = m_new
            l = l * alpha
            O = O * alpha[..., None]
            p = torch.where(trig_q[..., None], probs(P_SHIFT - m * c), p)
        if stats is not None:
            stats["tiles"] = stats.get("tiles", 0) + B * H * nblk
            stats["exact"] = stats.get("exact", 0) + int(trig.sum().item())
            stats["p_max"] = max(stats.get("p_max", 0.0), float(p.max().item()))
        assert bool((p <= E4M3_MAX).all()), "a probability above the e4m3 range reached the conversion"
        l = l + p.sum(-1)
        O = O + p.clamp(max=E4M3_MAX).to(F8).float() @ vh[:, :, t0:t1]
    out = O * v_scale.float()[:, :, None, :] / l[..., None]
    return out.permute(0, 2, 1, 3).to(torch.bfloat16)


def sdpa_fp8(q, k, v, scale=None, k_scale=None, kv_len=None):
    """bf16 (or fp32) q [B, H, Sq, D], k / v [B, H, Skv, D] -> the scheme's output in the same layout and dtype: the drop-in the
    model-level floors patch over an oracle's self-attention.  k_scale [B, H]: given K scales (the models' bound) instead of the
    measured amax / 448.  kv_len [B]: sample b attends to its first kv_len[b] keys; the operands are quantised over the whole
    length first, as the models do (V^T scales over every column)."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    qt, kt, vt = (t.to(torch.bfloat16).transpose(1, 2) for t in (q, k, v))
    q8, qs = quantize_rows(qt)
    k8, ks = quantize_khead(kt, k_scale)
    v8, vs = quantize_vt(vt)
    if kv_len is None:
        out = attention_fp8(q8, qs, k8, ks, v8, vs, scale)
    else:
        out = torch.cat([attention_fp8(q8[b:b + 1], qs[b:b + 1], k8[b:b + 1, :int(n)], ks[b:b + 1], v8[b:b + 1, :int(n)],
                                       vs[b:b + 1], scale) for b, n in enumerate(kv_len.tolist())])
    return out.transpose(1, 2).to(q.dtype)
