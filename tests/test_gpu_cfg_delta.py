"""The three entries of the CFG reuse (alg_amd/csrc/cfg_step.hip): alg_cfg_ddim_step_delta, alg_cfg_combine_delta and
alg_cfg_delta_drift.  Every comparison of the first two is torch.equal:

  STORE   the latents / the combined output are the bits of the plain entry with n_pass = 2, and the delta is the torch
          subtraction on the device (fp32 for the DDIM entry, the prediction dtype for the combine entry)
  REUSE   the bits of the plain entry on [u', text], with u' formed by torch on the device: float(text) - delta in fp32 for the
          DDIM entry (which is then handed the fp32 pair), text - delta rounded to the dtype for the combine entry

Sizes: 1, 8, 105 (1x1x3x5x7: the scalar path), 1,123,200 (C2: 13x16x60x90), 2,048 x 256 + 3 (the second trip of the scalar
path's grid-stride loop: its grid is capped at 2,048 blocks of 256 lanes), 2,048 x 256 x 8 + 8 (the second trip of the vector
path, 8 elements per lane), and a view offset by one element (a misaligned base: the scalar path at a multiple-of-8 size).

The drift is compared with torch's float64 sums on the device within the bound of tests/test_gpu_attn_drift.py -- the same
summation scheme, the same argument: a group's 8 non-negative terms are added in fp32, 7 additions each within 2^-24 relative and
the fp32 difference one more, so a partial is within 8 * 2^-24 ~ 4.8e-7 of its exact value and so is their sum (no cancellation);
everything above is double.  Asserted: 1e-6 relative."""
import ctypes

import pytest
import torch

from alg_amd import _lib
from alg_amd.schedulers import CogVideoXDDIMScheduler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
STORE, REUSE = _lib.CFG_DELTA_STORE, _lib.CFG_DELTA_REUSE
C2 = 13 * 16 * 60 * 90
SIZES = [1, 8, 105, C2, 2048 * 256 + 3, 2048 * 256 * 8 + 8]
PAIRS = [(BF, BF), (F32, BF), (F32, F32)]
G = 6.0


def operands(numel, pred_dtype, lat_dtype, seed, offset=0):
    """[uncond | text] of one step, [uncond | text] of an earlier step (where a reused delta comes from) and the latents, on the
    device; offset = 1: the predictions are views one element into their buffers (a misaligned base)."""
    g = torch.Generator().manual_seed(seed)

    def pred():
        hold = torch.zeros(2 * numel + offset, dtype=pred_dtype)
        hold[offset:] = torch.randn(2 * numel, generator=g).to(pred_dtype)
        return hold.to(DEV)[offset:]

    return pred(), pred(), torch.randn(numel, generator=g).to(lat_dtype).to(DEV)


def schedule():
    sched = CogVideoXDDIMScheduler()
    sched.set_timesteps(50)
    return sched, (sched.timesteps[0], sched.timesteps[17], sched.timesteps[-1])


def check_ddim(numel, pred_dtype, lat_dtype, offset=0):
    now, earlier, lat = operands(numel, pred_dtype, lat_dtype, 31 + numel % 97, offset)
    assert (now.data_ptr() % 16 != 0) == bool(offset)
    sched, timesteps = schedule()
    u, tx = now[:numel], now[numel:]
    for t in timesteps:
        # ---- STORE
        want = lat.clone()
        sched.fused_cfg_step_(now, want, 2, G, t)
        got, delta = lat.clone(), torch.full((numel,), -7.0, dtype=F32, device=DEV)
        sched.fused_cfg_step_delta_(now, got, delta, STORE, G, t)
        assert torch.equal(got, want) and not torch.equal(got, lat)
        assert torch.equal(delta, tx.float() - u.float())
        # ---- REUSE: the delta of the earlier step, this step's conditional prediction alone
        old = earlier[numel:].float() - earlier[:numel].float()
        u2 = tx.float() - old
        want = lat.clone()
        sched.fused_cfg_step_(torch.cat([u2, tx.float()]), want, 2, G, t)
        got, kept = lat.clone(), old.clone()
        sched.fused_cfg_step_delta_(tx, got, kept, REUSE, G, t)
        assert torch.equal(got, want) and torch.equal(kept, old)                # REUSE reads the delta and leaves it


def check_combine(numel, dtype, offset=0):
    now, earlier, _ = operands(numel, dtype, dtype, 57 + numel % 89, offset)
    u, tx = now[:numel], now[numel:]
    # ---- STORE
    want = _lib.cfg_combine(now, 2, G)
    delta = torch.full((numel,), -7.0, dtype=dtype, device=DEV)
    got = _lib.cfg_combine_delta(now, delta, STORE, G)
    assert got.dtype == dtype and torch.equal(got, want) and torch.equal(delta, tx - u)
    # ---- REUSE
    old = earlier[numel:] - earlier[:numel]
    u2 = tx - old                                                               # rounded to the dtype by torch
    want = _lib.cfg_combine(torch.cat([u2, tx]), 2, G)
    kept = old.clone()
    got = _lib.cfg_combine_delta(tx, kept, REUSE, G)
    assert torch.equal(got, want) and torch.equal(kept, old)


@pytest.mark.parametrize("pred_dtype,lat_dtype", PAIRS, ids=["bf16-bf16", "f32-bf16", "f32-f32"])
@pytest.mark.parametrize("numel", SIZES)
def test_ddim_step_delta_store_and_reuse(numel, pred_dtype, lat_dtype):
    check_ddim(numel, pred_dtype, lat_dtype)


@pytest.mark.parametrize("pred_dtype,lat_dtype", PAIRS, ids=["bf16-bf16", "f32-bf16", "f32-f32"])
def test_ddim_step_delta_on_a_misaligned_view_runs_the_scalar_path(pred_dtype, lat_dtype):
    check_ddim(2048, pred_dtype, lat_dtype, offset=1)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("numel", SIZES)
def test_combine_delta_store_and_reuse(numel, dtype):
    check_combine(numel, dtype)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_combine_delta_on_a_misaligned_view(dtype):
    check_combine(2048, dtype, offset=1)


def test_batched_shapes_through_the_wrappers():
    """[2 * B, ...] predictions, the delta [B, ...]: the two videos of a call share one launch."""
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(4, 3, 5, 7, generator=g).to(BF).to(DEV)
    delta = torch.empty(2, 3, 5, 7, dtype=BF, device=DEV)
    out = _lib.cfg_combine_delta(pred, delta, STORE, G)
    assert out.shape == (2, 3, 5, 7) and torch.equal(out, _lib.cfg_combine(pred, 2, G)) and torch.equal(delta, pred[2:] - pred[:2])
    u2 = pred[2:] - delta
    assert torch.equal(_lib.cfg_combine_delta(pred[2:].contiguous(), delta, REUSE, G), _lib.cfg_combine(torch.cat([u2, pred[2:]]), 2, G))
    for bad in (lambda: _lib.cfg_combine_delta(pred, delta.float(), STORE, G), lambda: _lib.cfg_combine_delta(pred, delta[:1], STORE, G),
                lambda: _lib.cfg_combine_delta(pred, delta, 2, G), lambda: _lib.cfg_combine_delta(pred[:3], delta, STORE, G),
                lambda: _lib.cfg_ddim_step_delta_(pred, delta.float(), delta, STORE, G, 1.0, 0.1, 1.0, 0.1),
                lambda: _lib.cfg_ddim_step_delta_(pred[2:], delta.float(), delta.float(), STORE, G, 1.0, 0.1, 1.0, 0.1)):
        with pytest.raises(_lib.AlgHipError):
            bad()


# ---- the drift ---------------------------------------------------------------------------------------------------------------
def drift(a, b):
    work = torch.empty(_lib.cfg_delta_drift_workspace_bytes(a.numel()), dtype=torch.uint8, device=DEV)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    _lib.cfg_delta_drift(a, b, work, out[1:3])
    host = out.cpu()
    assert host[0] == -7.0 and host[3] == -7.0           # the two sums and nothing else
    return host[1:3]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("numel", [1, 105, C2])
def test_drift_against_float64_sums_and_deterministic(numel, dtype):
    g = torch.Generator().manual_seed(numel % 1000)
    a, b = torch.randn(numel, generator=g).to(dtype).to(DEV), (torch.randn(numel, generator=g) * 3.0).to(dtype).to(DEV)
    want = ((a.double() - b.double()).abs().sum().item(), b.double().abs().sum().item())
    got = drift(a, b)
    rel = [abs(got[i].item() - want[i]) / want[i] for i in range(2)]
    print(numel, dtype, "relative errors", rel)
    assert max(rel) <= 1e-6
    assert torch.equal(got.view(torch.int64), drift(a, b).view(torch.int64))    # two launches, bitwise
    # exact data (integers up to 64: every fp32 partial and every double sum is exact): the sums EQUAL the float64 sums
    a = torch.randint(-64, 65, (numel,), generator=g).to(dtype).to(DEV)
    b = torch.randint(-64, 65, (numel,), generator=g).to(dtype).to(DEV)
    got = drift(a, b)
    assert (got[0].item(), got[1].item()) == ((a.double() - b.double()).abs().sum().item(), b.double().abs().sum().item())


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_return_einval_and_leave_the_outputs_alone():
    lib = _lib.load_library()
    n = 64
    pred = torch.ones(2 * n + 8, dtype=F32, device=DEV)
    lat, delta, out = (torch.full((n + 8,), -7.0, dtype=F32, device=DEV) for _ in range(3))
    work = torch.full((64,), 0x5A, dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    P = lambda t, byte=0: ctypes.c_void_p(t.data_ptr() + byte)
    s = _lib._stream()
    ddim = lambda pred_=P(pred), pd=0, delta_=P(delta), lat_=P(lat), ld=0, mode=0, numel=n: lib.alg_cfg_ddim_step_delta(
        pred_, pd, delta_, lat_, ld, mode, numel, G, 0.9, 0.4, 1.0, 0.1, s)
    comb = lambda pred_=P(pred), delta_=P(delta), out_=P(out), dt=0, mode=0, numel=n: lib.alg_cfg_combine_delta(
        pred_, delta_, out_, dt, mode, numel, G, s)
    drf = lambda a=P(pred), b=P(lat), dt=0, numel=n, work_=P(work), out_=P(sums): lib.alg_cfg_delta_drift(a, b, dt, numel, work_, out_, s)
    calls = [(ddim, kw) for kw in (dict(mode=2), dict(mode=-1), dict(pd=2), dict(ld=3), dict(numel=-1), dict(pred_=None),
                                   dict(delta_=None), dict(lat_=None), dict(pred_=P(pred, 2)), dict(delta_=P(delta, 1)),
                                   dict(lat_=P(lat, 3)))]
    calls += [(comb, kw) for kw in (dict(mode=2), dict(dt=2), dict(numel=-1), dict(pred_=None), dict(delta_=None), dict(out_=None),
                                    dict(pred_=P(pred, 2)), dict(dt=1, delta_=P(delta, 1)), dict(out_=P(out, 2)))]
    calls += [(drf, kw) for kw in (dict(dt=2), dict(numel=-1), dict(a=None), dict(b=None), dict(work_=None), dict(out_=None),
                                   dict(a=P(pred, 4)), dict(b=P(lat, 8)), dict(work_=P(work, 4)), dict(out_=P(sums, 4)))]
    for call, kw in calls:
        assert call(**kw) == -1, kw                                             # ALG_EINVAL
        assert b"alg_cfg_" in lib.alg_last_error()
    torch.cuda.synchronize()
    for t in (lat, delta, out, sums):
        assert (t == -7.0).all()
    assert (work == 0x5A).all() and (pred == 1.0).all()
    for call in (ddim, comb, drf):
        assert call(numel=0) == 0                                               # nothing to do: ALG_OK, nothing launched
    torch.cuda.synchronize()
    for t in (lat, delta, out, sums):
        assert (t == -7.0).all()
