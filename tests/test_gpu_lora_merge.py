"""alg_lora_merge on the GPU: out = bf16(W + (scale * B) @ A) with fp32 adapters, accumulated in double, r ascending.

Small, awkward shapes: (N, K) in {(1, 8), (70, 136), (257, 520)} -- one row, a ragged row tile and column tile, several
workgroups along both axes -- and R in {1, 5, 33, 130}, which crosses the 32 rank columns the kernel stages per round.  Leading
dimensions are larger than K and the padding is NaN: it must come back bit-identical and must not reach the result.

  exact data    operands on a grid where every fp32 product, sum and the final add is exact: torch.equal with float64
  in place      out aliases a bf16 W
  identity      scale = 0 and B = 0 give bf16(W)
  position      a row slice or a column slice merged alone has the bits of the full merge (the order of an output element's
                chain does not depend on the tile, the grid or the place in the matrix)
  random data   against float64: every element within one bf16 step, at most 1e-3 of the elements different at all
  two adapters  different ranks and scales in one launch against the float64 reference of their sum"""
import pytest
import torch

from alg_amd import _lib

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [(1, 8), (70, 136), (257, 520)]
RANKS = [1, 5, 33, 130]


def padded(t, pad, dev):
    """t [N, K] inside a NaN-filled [N, K + pad] device buffer: (view, buffer)"""
    N, K = t.shape
    buf = torch.full((N, K + pad), float("nan"), dtype=t.dtype, device=dev)
    buf[:, :K] = t.to(dev)
    return buf[:, :K], buf


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def padding_untouched(buf, K):
    return bool(torch.isnan(buf[:, K:].float()).all().item())


def exact_operands(N, K, R, seed):
    """(Exact in fp32 already, so in the kernel's double all the more.)  W: multiples of 2^-6 with |W| < 2; A: multiples of 2^-2 up to 1; B: multiples of 2^-1 up to 2; scale: a power of two in
    [1/4, 2].  t = scale * B is a multiple of 2^-3 up to 4, every product t * A a multiple of 2^-5 up to 4, a sum of up to 130
    of them a multiple of 2^-5 below 2^10 (15 bits), and W + acc a multiple of 2^-6 below 2^10 + 2 (17 bits): every fp32
    operation is exact (24 bits), so the only rounding is the last one, to bf16."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-127, 128, (N, K), generator=g).float() / 64
    a = torch.randint(-4, 5, (R, K), generator=g).float() / 4
    b = torch.randint(-4, 5, (N, R), generator=g).float() / 2
    s = 2.0 ** torch.randint(-2, 2, (R,), generator=g).float()
    return w, a, b, s


def ref64(w, a, b, s):
    return (w.double() + (s.double() * b.double()) @ a.double()).to(BF)


@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_exact_data_bf16_and_fp32_base_with_nan_padding(device, N, K, R):
    w, a, b, s = exact_operands(N, K, R, seed=N + R)
    want = ref64(w, a, b, s)
    ad, bd, sd = a.to(device), b.to(device), s.to(device)
    # (w is on the bf16 grid: 8 bits are enough for multiples of 2^-6 below 2)
    assert torch.equal(w.to(BF).float(), w)
    for wdt, pad_w in ((BF, 8), (torch.float32, 4)):
        wv, wbuf = padded(w.to(wdt), pad_w, device)
        ov, obuf = padded(torch.zeros(N, K, dtype=BF), 24, device)
        before = wbuf.clone()
        got = _lib.lora_merge(wv, ad, bd, sd, out=ov)
        assert got is ov and torch.equal(ov.cpu(), want), (wdt, (ov.cpu().float() - want.float()).abs().max())
        assert padding_untouched(obuf, K) and padding_untouched(wbuf, K)
        bits = torch.int16 if wdt == BF else torch.int32
        assert torch.equal(wbuf[:, :K].view(bits), before[:, :K].view(bits))                 # the base is only read
        assert torch.equal(_lib.lora_merge(wv, ad, bd, sd).cpu(), want)                      # out = None allocates


@pytest.mark.parametrize("N,K,R", [(1, 8, 5), (70, 136, 33), (257, 520, 130)])
def test_in_place_equals_out_of_place(device, N, K, R):
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF)
    a, b = torch.randn(R, K, generator=g).to(device), torch.randn(N, R, generator=g).to(device)
    s = torch.full((R,), 0.01, device=device)
    wv, wbuf = padded(w, 16, device)
    out = _lib.lora_merge(wv, a, b, s)
    assert same_bits(wv, w.to(device))
    assert _lib.lora_merge(wv, a, b, s, out=wv) is wv
    assert same_bits(wv, out) and padding_untouched(wbuf, K)
    assert not torch.equal(out.cpu(), w)
    # refused, not guessed: an fp32 base in place
    w32 = w.float().to(device)
    with pytest.raises(_lib.AlgHipError, match="bfloat16"):
        _lib.lora_merge(w32, a, b, s, out=w32)


@pytest.mark.parametrize("N,K,R", [(70, 136, 5), (257, 520, 130)])
def test_scale_zero_and_b_zero_give_bf16_of_w(device, N, K, R):
    g = torch.Generator().manual_seed(8)
    w32 = torch.randn(N, K, generator=g) * 0.02
    a, b = torch.randn(R, K, generator=g).to(device), torch.randn(N, R, generator=g).to(device)
    one, zero = torch.ones(R, device=device), torch.zeros(R, device=device)
    for w in (w32.to(BF), w32):
        want = w.to(BF).to(device)
        assert same_bits(_lib.lora_merge(w.to(device), a, b, zero), want)
        assert same_bits(_lib.lora_merge(w.to(device), a, torch.zeros_like(b), one), want)


@pytest.mark.parametrize("R", [33, 130])
def test_position_independence_of_rows_and_columns(device, R):
    N, K = 257, 520
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF).to(device)
    a, b = torch.randn(R, K, generator=g).to(device), torch.randn(N, R, generator=g).to(device)
    s = (torch.rand(R, generator=g) * 0.02).to(device)
    full = _lib.lora_merge(w, a, b, s)
    for r0, r1 in ((0, 1), (63, 130), (129, 257), (200, 203)):      # inside a row tile, across tiles, the ragged tail
        part = _lib.lora_merge(w[r0:r1], a, b[r0:r1].contiguous(), s)
        assert same_bits(part, full[r0:r1]), (r0, r1)
    for c0, c1 in ((0, 8), (120, 136), (128, 520), (504, 520)):     # a view into W (pointer offset, ld = 520) and a slice of A
        part = _lib.lora_merge(w[:, c0:c1], a[:, c0:c1].contiguous(), b, s)
        assert same_bits(part, full[:, c0:c1]), (c0, c1)


def one_bf16_step(x):
    """the spacing of bf16 at |x| (float64 in, float64 out): 2^(floor(log2 |x|) - 7), the smallest normal's for tiny values"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def figures(got, ref64_val, what):
    """(share of elements that differ from bf16(ref64) at all, worst distance in bf16 steps of the larger magnitude), printed"""
    want = ref64_val.to(BF)
    diff = (got.cpu().double() - want.double()).abs()
    step = one_bf16_step(torch.maximum(got.cpu().double().abs(), want.double().abs()))
    share, worst = (diff > 0).double().mean().item(), (diff / step).max().item()
    at = ref64_val.reshape(-1)[(diff / step).argmax()].item()
    print("%s: %d of %d elements differ from bf16(ref64) (share %.2e), worst %.3f bf16 steps (where ref64 = %.3e)"
          % (what, int((diff > 0).sum()), diff.numel(), share, worst, at))
    return share, worst


_RANDOM = {}


def random_cases(device, R):
    """W ~ N(0, 0.02^2) in bf16, A and B ~ N(0, 1), the scale set so that the delta's standard deviation is 0.3, 1 and 3 times
    W's (the delta of one element is a sum of R products of unit normals: std sqrt(R) before the scale).  Merged once per R:
    [(label, share, worst)]."""
    if R not in _RANDOM:
        N, K = 257, 520
        g = torch.Generator().manual_seed(10 + R)
        w = (torch.randn(N, K, generator=g) * 0.02).to(BF)
        a, b = torch.randn(R, K, generator=g), torch.randn(N, R, generator=g)
        out = []
        for ratio in (0.3, 1.0, 3.0):
            s = torch.full((R,), ratio * 0.02 / R ** 0.5)
            got = _lib.lora_merge(w.to(device), a.to(device), b.to(device), s.to(device))
            ref = w.double() + (s.double() * b.double()) @ a.double()
            label = "R=%d delta/W=%.1f" % (R, ratio)
            out.append((label,) + figures(got, ref, label))
        _RANDOM[R] = out
    return _RANDOM[R]


def two_adapter_case(device):
    """ranks 5 and 33 (38 columns: the second adapter straddles the staging round), scales 0.7 and -0.25 times alpha / r"""
    if "two" not in _RANDOM:
        N, K = 257, 520
        g = torch.Generator().manual_seed(11)
        w = (torch.randn(N, K, generator=g) * 0.02).to(BF)
        a1, b1 = torch.randn(5, K, generator=g), torch.randn(N, 5, generator=g)
        a2, b2 = torch.randn(33, K, generator=g), torch.randn(N, 33, generator=g)
        s1, s2 = 0.7 * 0.02 / 5 ** 0.5, -0.25 * 0.02 / 33 ** 0.5
        a, b = torch.cat([a1, a2]), torch.cat([b1, b2], dim=1).contiguous()
        s = torch.cat([torch.full((5,), s1), torch.full((33,), s2)])
        got = _lib.lora_merge(w.to(device), a.to(device), b.to(device), s.to(device))
        ref = w.double() + float(s[0]) * (b1.double() @ a1.double()) + float(s[-1]) * (b2.double() @ a2.double())
        alone = _lib.lora_merge(w.to(device), a1.to(device), b1.to(device), s[:5].to(device))
        _RANDOM["two"] = figures(got, ref, "two adapters") + (not torch.equal(got, alone),)
    return _RANDOM["two"]


@pytest.mark.parametrize("R", [16, 64, 128])
def test_random_data_share_of_elements_that_differ_from_float64(device, R):
    """At most 1e-3 of the elements differ from bf16(ref64) at all.  The cap is a condition, not a tolerance: an fp32 chain in
    this order gives 4e-5 to 2e-4 (CPU emulation), the kernel's double chain differs only where the float64 reference's own
    summation order decides a tie."""
    for label, share, _ in random_cases(device, R):
        assert share <= 1e-3, (label, share)


@pytest.mark.parametrize("R", [16, 64, 128])
def test_random_data_every_element_within_one_bf16_step_of_float64(device, R):
    """Every element is within one bf16 step (of the larger magnitude) of bf16(ref64) -- also where W and the delta cancel almost
    completely (R=16 delta/W=0.3 has an element with ref64 = 3.4e-8 from operands near 3.5e-3).  An fp32 chain misses this: its
    absolute error is an fp32 ulp of the operands per step, 2 to 8 bf16 steps of such a result (a CPU emulation of the fp32
    chain on this file's data: 2 steps at R=16, 2 and 3 at R=128, 8 for the two adapters below).  The kernel accumulates in
    double and rounds the double sum once."""
    for label, _, worst in random_cases(device, R):
        assert worst <= 1.0, (label, worst)


def test_two_adapters_in_one_launch_share_of_elements_that_differ(device):
    share, _, differs_from_first_alone = two_adapter_case(device)
    assert share <= 1e-3, share
    assert differs_from_first_alone


def test_two_adapters_in_one_launch_within_one_bf16_step_of_float64(device):
    """(one element has ref64 = 2.4e-8 from operands near 1e-2: 8 steps off with an fp32 chain)"""
    _, worst, _ = two_adapter_case(device)
    assert worst <= 1.0, worst
