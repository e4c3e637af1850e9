"""alg_attn_merge_lse in pure torch, float64 (include/alg_hip.h): the merge of two partial attentions over disjoint key sets.

    merge_ref(o, lse, o_far, lse_far, heads, head_dim) -> (merged [batch, Sq, heads * head_dim] float64, lse_out [batch, heads, Sq] float64)

o, o_far: [batch, Sq, heads * head_dim] of any float dtype; lse, lse_far: [batch, heads, Sq], log2 domain.  A side whose lse is -inf
carries no mass: the other side's values come through unchanged; both -inf: o, and lse_out = -inf."""
import torch


def merge_ref(o, lse, o_far, lse_far, heads, head_dim):
    B, Sq, D = o.shape
    assert D == heads * head_dim and lse.shape == lse_far.shape == (B, heads, Sq)
    x = o.double().view(B, Sq, heads, head_dim)
    y = o_far.double().view(B, Sq, heads, head_dim)
    a, f = lse.double().transpose(1, 2), lse_far.double().transpose(1, 2)            # [B, Sq, heads]
    m = torch.maximum(a, f)
    dead = torch.isinf(m) & (m < 0)
    m0 = torch.where(dead, torch.zeros_like(m), m)
    wa, wf = torch.exp2(a - m0), torch.exp2(f - m0)                                  # (-inf - 0 -> 0)
    den = torch.where(dead, torch.ones_like(m), wa + wf)
    merged = (wa.unsqueeze(-1) * x + wf.unsqueeze(-1) * y) / den.unsqueeze(-1)
    merged = torch.where(dead.unsqueeze(-1), x, merged)
    lse_out = torch.where(dead, m, m0 + torch.log2(den))
    return merged.reshape(B, Sq, D), lse_out.transpose(1, 2).contiguous()
