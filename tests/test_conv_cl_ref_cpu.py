"""The convolution GEMM's reference, pinned WITHOUT a GPU: tests/helpers/conv_cl_ref.py's statement of alg_conv_cl_bf16
(include/alg_hip.h's addressing, evaluated on flat buffers) equals the torch convolutions it stands for, to the bit, in all
three modes; `_lib.pack_conv_pair` turns the plain statement into the two-voxel one; the exactness precondition refuses
what breaks it; and the entry refuses every bad shape before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import alg_amd
from alg_amd import _lib
from helpers import conv_cl_ref as R


def _case(seed, Cin, Cout, kt, T, H, W, res=False):
    g = torch.Generator().manual_seed(seed)
    x = R.draw(g, Cin * T * H * W, R.X_STEP, R.X_MAX).float().reshape(1, Cin, T, H, W)
    w = R.draw(g, Cout * Cin * kt * 9, R.W_STEP, R.W_MAX).float().reshape(Cout, Cin, kt, 3, 3)
    b = R.draw(g, Cout, R.B_STEP, R.B_MAX)
    r = R.draw(g, Cout * T * H * W, R.B_STEP, R.B_MAX).float().reshape(1, Cout, T, H, W) if res else None
    return x, w, b, r


def _torch_conv3d(x, w, b, r, kt):
    """CogVideoXCausalConv3d in fp64 (first frame repeated kt - 1 times, zero spatial padding), bf16 roundings as the kernel's"""
    xin = torch.cat([x[:, :, :1]] * (kt - 1) + [x], dim=2).double()
    y = F.conv3d(xin, w.double(), b.double(), padding=(0, 1, 1)).float().bfloat16()
    if r is not None:
        y = (y.float() + r).bfloat16()
    return y[0].float()                                               # [Cout][T][H][W]


PLAIN_SHAPES = [(64, 8, 3, 3, 4, 5, False), (64, 12, 1, 2, 3, 6, True), (128, 4, 3, 1, 2, 3, True)]


@pytest.mark.parametrize("Cin,Cout,kt,T,H,W,res", PLAIN_SHAPES)
def test_plain_statement_is_conv3d(Cin, Cout, kt, T, H, W, res):
    x, w, b, r = _case(Cin + Cout + kt + T, Cin, Cout, kt, T, H, W, res)
    wl = R.weight_layout(w)
    R.check_exact(kt * 9 * Cin, x, wl, b, r)
    # the slack and the residual's don't-care rows hold NaN: no valid row may see them
    xp = R.padded(x, kt - 1, slack=R.slack_rows(W + 2), slack_fill=float("nan"))
    rv = R.virtual(r, fill=float("nan")) if res else None
    got = R.conv_cl_statement(xp, wl, b, rv, T, H + 2, W + 2, Cin, Cout, kt)
    assert got.shape == (T, (H + 2) * (W + 2), Cout)
    assert torch.equal(R.from_virtual(got, T, H, W, Cout), _torch_conv3d(x, w, b, r, kt))
    m = R.valid_mask(H + 2, W + 2)
    assert int(m.sum()) == H * W and bool(torch.isfinite(got[:, m].float()).all())


@pytest.mark.parametrize("Cin,Cout,kt,T,H,W,res", [(64, 8, 3, 3, 4, 5, True), (64, 12, 1, 2, 3, 6, False), (128, 4, 3, 1, 2, 3, False)])
def test_pair_statement_is_the_plain_statement_and_conv3d(Cin, Cout, kt, T, H, W, res):
    x, w, b, r = _case(Cin + Cout + kt + T, Cin, Cout, kt, T, H, W, res)
    wl = R.weight_layout(w)
    wp, bp = _lib.pack_conv_pair(wl, b, kt)
    assert wp.shape == (2 * Cout, kt * 12 * Cin) and bp.shape == (2 * Cout,)
    R.check_exact(kt * 12 * Cin, x, wp, bp, r)
    xp = R.padded(x, kt - 1, slack=R.slack_rows(W + 2, R.PAIR), slack_fill=float("nan"))
    rv = R.virtual(r, fill=float("nan")) if res else None
    pair = R.conv_cl_statement(xp, wp, bp, rv, T, H + 2, W + 2, Cin, Cout, kt, R.PAIR)
    plain = R.conv_cl_statement(xp, wl, b, rv, T, H + 2, W + 2, Cin, Cout, kt)
    m = R.valid_mask(H + 2, W + 2)
    assert pair.shape == plain.shape and torch.equal(pair[:, m], plain[:, m])
    assert torch.equal(R.from_virtual(pair, T, H, W, Cout), _torch_conv3d(x, w, b, r, kt))


@pytest.mark.parametrize("Cin,Cout,T,H,W,x_off_frames", [(64, 8, 2, 4, 6, 0), (128, 4, 1, 2, 4, 2), (64, 12, 3, 6, 2, 0)])
def test_stride2_statement_is_pad_conv2d(Cin, Cout, T, H, W, x_off_frames):
    x, w, b, _ = _case(Cin + Cout + T, Cin, Cout, 1, T + x_off_frames, H, W)
    wl = R.weight_layout(w)
    R.check_exact(9 * Cin, x, wl, b)
    Hp, Wp = H + 2, W + 2
    xp = R.padded(x, 0, slack=R.slack_rows(Wp), slack_fill=float("nan"))
    got = R.conv_cl_statement(xp, wl, b, None, T, Hp, Wp, Cin, Cout, 1, R.STRIDE2, x_off=x_off_frames * Hp * Wp * Cin)
    assert got.shape == (T, R.stride2_rows(H, Wp), Cout)
    xs = x[0, :, x_off_frames:].permute(1, 0, 2, 3).double()                       # [T][Cin][H][W]
    want = F.conv2d(F.pad(xs, (0, 1, 0, 1)), w[:, :, 0].double(), b.double(), stride=2).float().bfloat16()
    m = R.valid_mask(Hp, Wp, R.STRIDE2)
    assert int(m.sum()) == (H // 2) * (W // 2)
    got = got[:, m].reshape(T, H // 2, W // 2, Cout).permute(0, 3, 1, 2)
    assert torch.equal(got, want)


def test_most_outputs_need_the_rounding():
    """The check would be weak if the exact sums were bf16 values already.  A sum s (a multiple of 2^-5) in [2^e, 2^(e + 1)) is
    a bf16 value only if it is a multiple of 2^(e - 7): one in 2^(e - 2) for e > 2.  At K = 1728 the sums have a standard
    deviation of sqrt(K * E[x^2] * E[w^2]) = sqrt(1728 * 3.125 * 1.5) = 90, which puts about 0.8 of them off the bf16 grid
    (0.07 below 8, all exact; 1/2 of 0.07, 1/4 of 0.14, 1/8 of 0.24, 1/16 of 0.32 ... above); border rows sum fewer taps."""
    x, w, b, _ = _case(1, 64, 16, 3, 2, 4, 5)
    Hp, Wp = 6, 7
    xp = R.padded(x, 2).double().reshape(-1, 64)
    wl = R.weight_layout(w).double()
    taps = torch.tensor([dt * Hp * Wp + dy * Wp + dx for dt in range(3) for dy in range(3) for dx in range(3)])
    rows = torch.arange(Hp * Wp)[R.valid_mask(Hp, Wp)]
    acc = xp[rows[:, None] + taps[None, :]].reshape(len(rows), -1) @ wl.t() + b.double()
    inexact = (acc.float().bfloat16().double() != acc).float().mean().item()
    assert inexact > 0.7, inexact


def test_exactness_precondition_refuses():
    g = torch.Generator().manual_seed(0)
    x, w = R.draw(g, 64, R.X_STEP, R.X_MAX), R.draw(g, 64, R.W_STEP, R.W_MAX)
    x[0], w[0] = R.X_MAX, -R.W_MAX
    b = torch.tensor([R.B_MAX]).bfloat16()
    assert R.check_exact(512 * 27, x, w, b, b) == (512 * 27 * 6.0 + 40.0) * 32       # the largest K any VAE convolution has
    assert R.check_exact(2 ** 16, x, w) < 2.0 ** 24
    with pytest.raises(R.NotExact, match="2\\^24"):
        R.check_exact(2 ** 17, x, w)                                             # 2^17 * 6 * 2^5 >= 2^24
    with pytest.raises(R.NotExact, match="2\\^24"):
        R.check_exact(2 ** 16, x * 2, w)
    with pytest.raises(R.NotExact, match="2\\^24"):
        R.check_exact(64, x, w, b, torch.tensor([2.0 ** 19]))                    # the residual counts
    with pytest.raises(R.NotExact, match="multiple"):
        R.check_exact(64, x + 2.0 ** -4, w)                                      # off the 2^-3 grid
    with pytest.raises(R.NotExact, match="multiple"):
        R.check_exact(64, x, w, torch.tensor([0.3]))
    xs = torch.cat([x, torch.full((8,), float("nan"), dtype=torch.bfloat16)])    # NaN slack is no input
    assert R.check_exact(64, xs, w) == R.check_exact(64, x, w)


REFUSED = [
    # (what, frames, Hp, Wp, Cin, Cout, kt, mode)
    ("kt = 2", 2, 8, 8, 64, 64, 2, R.PLAIN),
    ("Cin = 32", 2, 8, 8, 32, 64, 3, R.PLAIN),
    ("Cin = 96", 2, 8, 8, 96, 64, 3, R.PLAIN),
    ("Cout = 6", 2, 8, 8, 64, 6, 3, R.PLAIN),
    ("Hp = 2", 2, 2, 8, 64, 64, 3, R.PLAIN),
    ("frames = 0", 0, 8, 8, 64, 64, 3, R.PLAIN),
    ("mode = 3", 2, 8, 8, 64, 64, 3, 3),
    ("pair, odd Hp*Wp", 2, 7, 9, 64, 64, 3, R.PAIR),
    ("pair, Cout = 256", 2, 8, 8, 64, 256, 3, R.PAIR),
    ("stride 2, kt = 3", 2, 8, 8, 64, 64, 3, R.STRIDE2),
    ("stride 2, odd Hp", 2, 7, 8, 64, 64, 1, R.STRIDE2),
    ("stride 2, odd Wp", 2, 8, 7, 64, 64, 1, R.STRIDE2),
]


# (with a GPU the test is skipped, as tests/test_gemm_args_cpu.py is: a check lost by mistake would launch on host pointers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")
@pytest.mark.parametrize("what,frames,Hp,Wp,Cin,Cout,kt,mode", REFUSED, ids=[r[0] for r in REFUSED])
def test_entry_refuses_before_any_launch(what, frames, Hp, Wp, Cin, Cout, kt, mode):
    """Validation runs before any launch (and before any HIP call), so it is testable on host pointers -- which are never
    dereferenced: every case returns ALG_EINVAL with the entry's name and the offending shape in alg_last_error()."""
    lib = alg_amd.load_library()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 255) & ~255
    rc = lib.alg_conv_cl_bf16(p, p + 1024, None, None, p + 2048, frames, Hp, Wp, Cin, Cout, kt, mode, None)
    text = lib.alg_last_error().decode()
    assert rc == -1, (what, rc, text)
    assert text.startswith("alg_conv_cl_bf16: bad shape") and "frames=%d Hp=%d Wp=%d Cin=%d Cout=%d kt=%d " % (
        frames, Hp, Wp, Cin, Cout, kt) in text, text
