"""Host emulation of the OCP MXFP4 scheme of alg_quantize_mxfp4_rows / alg_gemm_fp4 (helper of the fp4 tests; not a conftest).

Format (include/alg_hip.h): blocks of 32 consecutive elements along the last dimension; scale byte (E8M0)
e = clamp(floor(log2(amax)) - 2, -127, 127) + 127, 127 for an all-zero block; elements x * 2^-(e - 127) rounded to nearest, ties
to even, onto the e2m1 grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6, the input's sign bit kept; two elements per byte,
element 2i in the low nibble of byte i.  Everything here is float64 / integer arithmetic on whatever device the input lives on.

`mxfp4_linears(weights)` is the fp4 sibling of tests/_fp8_floor.py: for its duration exactly the two linears that
`CogVideoXTransformer3DModel(..., fp4=True)` runs in MXFP4 -- ff.net.0.proj and ff.net.2 of every block -- go through `linear`
below (W4A4: both operands quantised and de-quantised, fp32 accumulation, one rounding to the activation dtype)."""
import contextlib
import re

import torch
import torch.nn.functional as F

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32
FP4_LINEARS = ("ff.net.0.proj", "ff.net.2")
_NAME = re.compile(r"^transformer_blocks\.\d+\.(%s)\.weight$" % "|".join(re.escape(n) for n in FP4_LINEARS))

TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def special_blocks():
    """[rows, 32] float32 blocks with a known scale each: every tie point (both signs), saturation, zero, a power-of-two amax,
    negative values that round to zero.  Returns (blocks, expected scale exponents e - 127)."""
    rows, exps = [], []
    for k in (0, -3, 5):                                            # block scale 2^k: amax in [4, 8) * 2^k
        s = 2.0 ** k
        ties = [t * s for t in TIES] + [-t * s for t in TIES]
        rows.append(ties + [6.0 * s] + [0.0] * (32 - len(ties) - 1))               # amax 6 s: scale 2^k
        exps.append(k)
        near = [(t + d) * s for t in TIES for d in (-2.0 ** -5, 2.0 ** -5)]         # just off every tie (bf16-exact)
        rows.append(near + [4.0 * s] + [0.0] * (32 - len(near) - 1))
        exps.append(k)
        sat = [6.25 * s, 7.0 * s, 7.75 * s, -6.5 * s, -7.9375 * s]                 # (6, 8) s: saturate to +-6
        rows.append(sat + [5.5 * s, -5.5 * s] + [0.125 * s, -0.125 * s, -0.25 * s, -0.1875 * s] + [0.0] * 21)
        exps.append(k)
    rows.append([0.0] * 32)                                         # the zero block: scale byte 127
    exps.append(0)
    rows.append([-0.0] * 16 + [0.0] * 16)
    exps.append(0)
    rows.append([1.0] + [0.0] * 31)                                 # amax exactly 2^0: floor(log2) - 2 = -2
    exps.append(-2)
    x = torch.tensor(rows, dtype=torch.float32)
    assert torch.equal(x, x.bfloat16().float())                     # every value is a bf16 number
    return x, exps


def quantize(x):
    """x [..., K] (K % 32 == 0) -> (codes [..., K] uint8: bit 3 sign, bits 0-2 index into GRID; scales [..., K / 32] uint8)."""
    K = x.shape[-1]
    assert K % BLOCK == 0
    b = x.double().reshape(*x.shape[:-1], K // BLOCK, BLOCK)
    amax = b.abs().amax(-1)
    _, ex = torch.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, (ex.long() - 1 - 2).clamp(-127, 127) + 127, torch.full_like(ex, 127, dtype=torch.long))
    a = torch.ldexp(b.abs(), (127 - e).unsqueeze(-1).to(torch.int32))
    # round half to even on each binade's step: 0.5 below 2, 1 below 4, 2 above; then saturate
    r = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2)).clamp(max=6.0)
    grid = torch.tensor(GRID, dtype=torch.float64, device=x.device)
    code = torch.searchsorted(grid, r.contiguous())
    assert bool((grid[code] == r).all())
    code = code + 8 * torch.signbit(b).long()
    return code.reshape(x.shape).to(torch.uint8), e.to(torch.uint8)


def dequantize(codes, scales):
    """float64 values of (codes, scales) as `quantize` returns them."""
    grid = torch.tensor(GRID, dtype=torch.float64, device=codes.device)
    c = codes.long()
    v = grid[c & 7] * (1 - 2 * ((c >> 3) & 1)).double()
    K = codes.shape[-1]
    v = v.reshape(*codes.shape[:-1], K // BLOCK, BLOCK)
    v = torch.ldexp(v, (scales.long() - 127).unsqueeze(-1).to(torch.int32))
    return v.reshape(codes.shape)


def pack(codes):
    """[..., K] codes -> [..., K / 2] bytes, element 2i in the low nibble of byte i."""
    c = codes.reshape(*codes.shape[:-1], codes.shape[-1] // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8)


def unpack(q):
    return torch.stack([q & 15, q >> 4], dim=-1).reshape(*q.shape[:-1], q.shape[-1] * 2)


def fake_quant(x):
    return dequantize(*quantize(x))


def linear(x, weight, bias=None, out_dtype=None):
    """W4A4: y = dq(q(x)) @ dq(q(weight))^T + bias with fp32 accumulation, one rounding to out_dtype (default x.dtype).  The
    de-quantised values are exact in fp32 (one mantissa bit times a power of two)."""
    out_dtype = out_dtype or x.dtype
    y = fake_quant(x).float() @ fake_quant(weight).float().t()
    if bias is not None:
        y = y + bias.float()
    return y.to(out_dtype)


def fp4_weight_names(weights):
    return [k for k in weights if _NAME.match(k)]


@contextlib.contextmanager
def mxfp4_linears(weights):
    """Route ff.net.0.proj and ff.net.2 of every block in `weights` (a dit_oracle weight dict, recognised by data_ptr()) through
    `linear` above; every other F.linear call is left alone.  Yields {"routed", "other", "weights"} counters; F.linear is restored
    on exit, also when the body raises."""
    ptrs = {weights[k].data_ptr() for k in fp4_weight_names(weights)}
    original = F.linear
    stats = {"routed": 0, "other": 0, "weights": len(ptrs)}

    def routed(x, weight, bias=None):
        if weight.data_ptr() not in ptrs:
            stats["other"] += 1
            return original(x, weight, bias)
        stats["routed"] += 1
        return linear(x, weight, bias, out_dtype=x.dtype)

    F.linear = routed
    try:
        yield stats
    finally:
        F.linear = original
