"""alg_attn_drift (alg_amd/csrc/attn_reuse.hip): out[0] = sum |a - b|, out[1] = sum |b| over strided bf16 [rows][cols] operands.

Exact data (integer-valued bf16, |v| <= 64): every difference, every 8-term fp32 partial (<= 8 * 128) and every double sum above
it is exact, so both sums must EQUAL the float64 sums.  Gaussian data: a thread adds the 8 non-negative terms of a vector in fp32
-- 7 additions, each within 2^-24 relative, and the fp32 difference of two bf16 values one more -- so a partial is within
8 * 2^-24 ~ 4.8e-7 of its exact value, and so is a sum of such partials (no cancellation); everything above is double.  The
bound asserted is 1e-6 relative against float64."""
import pytest
import torch

from alg_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SHAPES = [(1, 8, 8, 8),             # one vector
          (3, 64, 64, 64),          # less than a wave
          (257, 192, 192, 448),     # strided like HunyuanVideo's joint row [attention | mlp], an odd row count
          (4096, 512, 512, 512)]    # more vectors than one pass of the capped grid
ids = ["%dx%d-%d-%d" % s for s in SHAPES]
POISON = float("inf")               # between cols and a row stride: a kernel that read it would return inf


def operands(shape, kind, seed):
    rows, cols, a_rs, b_rs = shape
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        a = torch.randint(-64, 65, (rows, cols), generator=g).to(BF)
        b = torch.randint(-64, 65, (rows, cols), generator=g).to(BF)
    else:
        a, b = torch.randn(rows, cols, generator=g).to(BF), (torch.randn(rows, cols, generator=g) * 3.0).to(BF)
    hold_a, hold_b = torch.full((rows, a_rs), POISON, dtype=BF), torch.full((rows, b_rs), POISON, dtype=BF)
    hold_a[:, :cols], hold_b[:, :cols] = a, b
    want = ((a.double() - b.double()).abs().sum().item(), b.double().abs().sum().item())
    return hold_a.to(DEV)[:, :cols], hold_b.to(DEV)[:, :cols], want


def drift(a, b):
    rows, cols = a.shape
    work = torch.empty(_lib.attn_drift_workspace_bytes(rows, cols), dtype=torch.uint8, device=DEV)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    _lib.attn_drift(a, b, work, out[1:3])
    host = out.cpu()
    assert host[0] == -7.0 and host[3] == -7.0           # the two sums and nothing else
    return host[1:3]


def test_the_largest_shape_needs_more_than_one_pass_of_the_capped_grid():
    rows, cols = SHAPES[-1][:2]
    assert rows * cols // 8 > _lib.ATTN_DRIFT_MAX_BLOCKS * _lib.ATTN_DRIFT_THREADS
    assert _lib.attn_drift_workspace_bytes(rows, cols) == _lib.ATTN_DRIFT_MAX_BLOCKS * 16
    for r, c in (s[:2] for s in SHAPES[:-1]):            # ... and the others fit into one
        assert _lib.attn_drift_workspace_bytes(r, c) == -(-r * c // 8 // _lib.ATTN_DRIFT_THREADS) * 16


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_data_gives_the_float64_sums(shape):
    a, b, want = operands(shape, "exact", 1)
    got = drift(a, b)
    assert (got[0].item(), got[1].item()) == want


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gaussian_data_within_the_fp32_partials_bound_and_deterministic(shape):
    a, b, want = operands(shape, "gauss", 2)
    got = drift(a, b)
    rel = [abs(got[i].item() - want[i]) / want[i] for i in range(2)]
    print(shape, "relative errors", rel)
    assert max(rel) <= 1e-6
    again = drift(a, b)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))          # two runs, bitwise


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_a_nan_in_a_reaches_the_first_sum_only(shape):
    a, b, want = operands(shape, "exact", 3)
    a[shape[0] // 2, shape[1] - 3] = float("nan")
    got = drift(a, b)
    assert torch.isnan(got[0]) and got[1].item() == want[1]


def test_no_rows_gives_zeros_and_the_wrapper_refuses_what_the_kernel_cannot_take():
    hold = torch.ones(2, 4, 64, dtype=BF, device=DEV)
    assert drift(hold[0, :0], hold[1, :0]).tolist() == [0.0, 0.0]
    work, out = torch.empty(64, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    x = torch.zeros(4, 64, dtype=BF, device=DEV)
    with pytest.raises(_lib.AlgHipError):
        _lib.attn_drift(x, x.float(), work, out)
    with pytest.raises(_lib.AlgHipError):
        _lib.attn_drift(x, x[:, :32], work, out)
    with pytest.raises(_lib.AlgHipError):
        _lib.attn_drift(x[:, 1:57], x[:, :56], work, out)                       # a misaligned view: the C check refuses it
    with pytest.raises(_lib.AlgHipError):
        _lib.attn_drift(x, x, work[:8], out)
