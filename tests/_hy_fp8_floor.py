"""The e4m3-eager floor of the HunyuanVideo DiT (helper of the fp8 tests; not a conftest): tests/_fp8_floor.py's method for
`oracle/hy_oracle.py`.

`hy_forward` has no fp8 switch, but it calls every linear as `F.linear(x, sd[name].to(dtype), ...)` with `F` being
`torch.nn.functional`.  `hy_fp8_linears(sd, dtype)` is a context manager that, for its duration, sends exactly the linears that
`HunyuanVideoTransformer3DModel(..., fp8=True)` quantises -- recognised by the `data_ptr()` of their weight in the state dict it
was given -- to `oracle.fp8_oracle.linear(x, weight, bias, out_dtype=x.dtype)` (per-token / per-output-channel e4m3, fp32
accumulation, one rounding to the activation dtype) and leaves every other `F.linear` call alone:

    transformer_blocks.N         attn.to_q, attn.to_k, attn.to_v, attn.to_out.0, ff.net.0.proj, ff.net.2   (latent stream; 6 calls)
    single_transformer_blocks.N  attn.to_q, attn.to_k, attn.to_v, proj_mlp, proj_out                     (joint rows; 5 calls)

The oracle applies the single blocks' linears to the joint [latents; text] rows and `proj_out` to `torch.cat([a, mlp], dim=2)`,
so the routed `proj_out` quantises the concatenated 5 D-wide row with ONE scale per token -- the product's scheme.  The prompt
stream of the dual blocks (add_q/k/v_proj, to_add_out, ff_context), the token refiner (whose linears carry the same short names
under `context_embedder.`), the embedders, every AdaLN linear and the output head are not routed.

`sd[name].to(dtype)` returns the tensor itself only when it already has that dtype: the state dict must be in the run's dtype for
the pointers to survive, which the helper asserts."""
import contextlib
import re

import torch.nn.functional as F

from oracle import fp8_oracle

DUAL_LINEARS = ("attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0", "ff.net.0.proj", "ff.net.2")
SINGLE_LINEARS = ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp", "proj_out")
_alt = lambda names: "|".join(re.escape(n) for n in names)
_NAME = re.compile(r"^(transformer_blocks\.\d+\.(%s)|single_transformer_blocks\.\d+\.(%s))\.weight$"
                   % (_alt(DUAL_LINEARS), _alt(SINGLE_LINEARS)))


def fp8_weight_names(sd):
    return [k for k in sd if _NAME.match(k)]


def routed_per_forward(cfg):
    """oracle `lin` calls one forward re-routes: q, k and v are separate calls there"""
    return len(DUAL_LINEARS) * cfg.num_layers + len(SINGLE_LINEARS) * cfg.num_single_layers


@contextlib.contextmanager
def hy_fp8_linears(sd, dtype):
    """Route the quantised linears of every block in `sd` (the state dict hy_forward will be called with, in `dtype`, on whatever
    device it lives) through fp8_oracle.linear.  Yields a dict whose "routed" entry counts the re-routed calls and "other" the
    untouched ones.  torch.nn.functional.linear is restored on exit, also when the body raises."""
    names = fp8_weight_names(sd)
    wrong = [k for k in names if sd[k].dtype != dtype]
    assert not wrong, "the state dict must already be in %s (hy_forward's sd[n].to(dtype) would copy %s)" % (dtype, wrong[:3])
    ptrs = {sd[k].data_ptr() for k in names}
    assert len(ptrs) == len(names)
    original = F.linear
    stats = {"routed": 0, "other": 0, "weights": len(ptrs)}

    def linear(x, weight, bias=None):
        if weight.data_ptr() not in ptrs:
            stats["other"] += 1
            return original(x, weight, bias)
        stats["routed"] += 1
        F.linear = original            # fp8_oracle.linear uses F.linear itself
        try:
            return fp8_oracle.linear(x, weight, bias, out_dtype=x.dtype)
        finally:
            F.linear = linear

    F.linear = linear
    try:
        yield stats
    finally:
        F.linear = original
