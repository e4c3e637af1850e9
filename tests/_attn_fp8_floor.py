"""The e4m3-attention floor of the Wan and HunyuanVideo DiTs (helper of the fp8_attention tests; not a conftest).

`oracle/wan_oracle.py` and `oracle/hy_oracle.py` have no fp8-attention switch, but both send every attention through their
module-level `_sdpa`.  The context managers here replace it, for their duration, by a function that routes exactly the calls
`transformer.fp8_attention` moves onto alg_flash_attn_d128_fp8 -- Wan: the self-attention of every block (recognised by Sq == Skv;
the cross-attentions have 512 / 257 keys); HunyuanVideo: the joint attention of the dual- and single-stream blocks (every call
behind the token refiner's) -- through the eager restatement of the scheme (tests/helpers/attn_fp8_ref.py: sdpa_fp8) with the K
scales the models use (transformer_wan.k_scale_bound of the block's bf16 norm weights), and leaves every other call alone.  The
oracle run inside the context with bf16 weights and activations is "the reference's execution mode with e4m3 self-attention":
the floor the models are held to (tests/_parity.py).  Nothing under oracle/ changes."""
import contextlib

import torch

from alg_amd.transformer_wan import k_scale_bound
from helpers import attn_fp8_ref
from oracle import hy_oracle, wan_oracle

BF = torch.bfloat16


@contextlib.contextmanager
def wan_fp8_attention(cfg, sd):
    original = wan_oracle._sdpa
    stats = {"routed": 0, "other": 0}
    D, heads = cfg.dim, cfg.num_attention_heads

    def sdpa(q, k, v, heads_, *a, **kw):
        if q.shape[1] != k.shape[1]:
            stats["other"] += 1
            return original(q, k, v, heads_, *a, **kw)
        l = stats["routed"] % cfg.num_layers
        stats["routed"] += 1
        B = q.shape[0]
        ks = k_scale_bound(sd["blocks.%d.attn1.norm_k.weight" % l].to(BF), D, heads, rope=True).to(q.device)
        qh, kh, vh = (t.view(B, -1, heads, D // heads).transpose(1, 2) for t in (q, k, v))
        o = attn_fp8_ref.sdpa_fp8(qh, kh, vh, k_scale=ks[None].expand(B, -1))
        return o.transpose(1, 2).reshape(B, -1, D).to(q.dtype)

    wan_oracle._sdpa = sdpa
    try:
        yield stats
    finally:
        wan_oracle._sdpa = original


@contextlib.contextmanager
def hy_fp8_attention(cfg, sd):
    original = hy_oracle._sdpa
    stats = {"routed": 0, "other": 0}
    heads = cfg.num_attention_heads
    per_forward = cfg.num_refiner_layers + cfg.num_layers + cfg.num_single_layers
    bound = lambda name, rope: k_scale_bound(sd[name].to(BF), 128, heads, rope=rope)

    def sdpa(q, k, v, kv_len, *a, **kw):
        i = (stats["routed"] + stats["other"]) % per_forward
        if i < cfg.num_refiner_layers:
            stats["other"] += 1
            return original(q, k, v, kv_len, *a, **kw)
        stats["routed"] += 1
        j = i - cfg.num_refiner_layers
        if j < cfg.num_layers:
            b = "transformer_blocks.%d.attn." % j
            ks = torch.maximum(bound(b + "norm_k.weight", True), bound(b + "norm_added_k.weight", False))
        else:
            ks = bound("single_transformer_blocks.%d.attn.norm_k.weight" % (j - cfg.num_layers), True)
        return attn_fp8_ref.sdpa_fp8(q, k, v, k_scale=ks.to(q.device)[None].expand(q.shape[0], -1), kv_len=kv_len)

    hy_oracle._sdpa = sdpa
    try:
        yield stats
    finally:
        hy_oracle._sdpa = original
