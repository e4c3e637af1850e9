"""The e4m3-eager floor of the CogVideoX DiT (helper of the fp8 tests; not a conftest).

`oracle/dit_oracle.py` has no fp8 switch, but it calls every linear as `F.linear(x, w[name], ...)` with `F` being
`torch.nn.functional`.  `fp8_linears(weights)` is a context manager that, for its duration, sends exactly the six
block linears that `CogVideoXTransformer3DModel(..., fp8=True)` quantises -- attn1.to_q / to_k / to_v / to_out.0,
ff.net.0.proj, ff.net.2 of every block, recognised by the `data_ptr()` of their weight in the dict it was given -- to
`oracle.fp8_oracle.linear(x, weight, bias, out_dtype=x.dtype)` (per-token / per-output-channel e4m3, fp32 accumulation,
one rounding to the activation dtype) and leaves every other `F.linear` call alone.  The oracle run inside the context
with bf16 weights and activations is "the reference's execution mode with e4m3 block linears": the floor the fp8 model
is held to, as the plain bf16-eager run is the floor of the bf16 model (tests/_parity.py)."""
import contextlib
import re

import torch
import torch.nn.functional as F

from oracle import fp8_oracle

FP8_LINEARS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")
_NAME = re.compile(r"^transformer_blocks\.\d+\.(%s)\.weight$" % "|".join(re.escape(n) for n in FP8_LINEARS))


def fp8_weight_names(weights):
    return [k for k in weights if _NAME.match(k)]


@contextlib.contextmanager
def fp8_linears(weights):
    """Route the six block linears of every block in `weights` (a dit_oracle weight dict: the tensors the oracle will be
    called with, on whatever device they live) through fp8_oracle.linear.  Yields a dict whose "routed" entry counts the
    re-routed calls and "other" the untouched ones.  torch.nn.functional.linear is restored on exit, also when the body
    raises."""
    ptrs = {weights[k].data_ptr() for k in fp8_weight_names(weights)}
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
