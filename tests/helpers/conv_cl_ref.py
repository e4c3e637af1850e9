"""Exact-arithmetic reference of alg_conv_cl_bf16 (include/alg_hip.h): the layouts, the header's own statement of the
operation on flat buffers, and inputs for which that statement defines every output bit.

Exactness.  x is drawn as multiples of 2^-3, w as multiples of 2^-2, bias and residual as multiples of 2^-3 (all
bf16-exact), so every product and every partial sum is a multiple of 2^-5.  `check_exact` asserts
    (K * max|x| * max|w| + max|bias| + max|res|) * 2^5 < 2^24:
every partial sum, in ANY summation order, is then an integer below 2^24 times 2^-5, i.e. exact in fp32 -- whatever MFMA
shape or k order a kernel uses.  The result is therefore defined to the bit:
    y = bf16(conv + bias)                      without a residual
    y = bf16(res + bf16(conv + bias))          with one (the convolution returns a bf16 tensor; the add rounds again)
with round-to-nearest-even, which is what `tensor.to(torch.bfloat16)` does to an exactly representable fp32 value."""
import torch
import torch.nn.functional as F

PLAIN, PAIR, STRIDE2 = 0, 1, 2
X_STEP, X_MAX = 2.0 ** -3, 3.0
W_STEP, W_MAX = 2.0 ** -2, 2.0
B_STEP, B_MAX = 2.0 ** -3, 20.0     # 160 steps: 8 significant bits, bf16-exact


class NotExact(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def slack_rows(Wp, mode=PLAIN):
    """rows the header lets the kernel read past the end of x"""
    return 2 * Wp + (3 if mode == PAIR else 2)


def padded(x, time_pad, slack=None, slack_fill=0.0):
    """NCTHW fp32 (B = 1) -> padded channels-last bf16 flat buffer [T + time_pad][H + 2][W + 2][C] + `slack` rows (default
    2 * Wp + 4) of `slack_fill`: zero borders, the first frame repeated `time_pad` times in front (causal padding)."""
    _, C, T, H, W = x.shape
    if time_pad:
        x = torch.cat([x[:, :, :1]] * time_pad + [x], dim=2)
    x = F.pad(x, (1, 1, 1, 1))
    flat = x[0].permute(1, 2, 3, 0).contiguous().bfloat16().reshape(-1)
    n = (2 * (W + 2) + 4 if slack is None else slack) * C
    return torch.cat([flat, torch.full((n,), slack_fill, dtype=torch.bfloat16)])


def virtual(x, fill=7.0):
    """NCTHW (B = 1) -> virtual layout [T][H + 2][W + 2][C] with `fill` in the don't-care rows."""
    x = F.pad(x, (0, 2, 0, 2), value=fill)
    return x[0].permute(1, 2, 3, 0).contiguous().bfloat16().reshape(-1)


def from_virtual(buf, T, H, W, C):
    """virtual layout -> [C][T][H][W] fp32 on the CPU"""
    return buf.reshape(T, H + 2, W + 2, C)[:, :H, :W].permute(3, 0, 1, 2).float().cpu()


def weight_layout(w):
    """[Cout][Cin][kt][3][3] (or [Cout][Cin][3][3]) -> [Cout][kt*9*Cin] bf16: tap-major (dt, dy, dx), channels innermost"""
    co, ci = w.shape[:2]
    return w.reshape(co, ci, -1).permute(0, 2, 1).reshape(co, -1).contiguous().bfloat16()


def stride2_rows(H, Wp):
    """rows per frame of the stride-2 form's output: (Y, X) at row Y * Wp + X, the INPUT's pitch"""
    return H // 2 * Wp


def valid_mask(Hp, Wp, mode=PLAIN):
    """bool [rows per frame of y]: y < H and x < W (stride 2: Y < H / 2 -- every row -- and X < W / 2)"""
    if mode == STRIDE2:
        return (torch.arange(Wp) < (Wp - 2) // 2).repeat((Hp - 2) // 2)
    yy, xx = torch.meshgrid(torch.arange(Hp), torch.arange(Wp), indexing="ij")
    return ((yy < Hp - 2) & (xx < Wp - 2)).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# exact inputs
# ---------------------------------------------------------------------------------------------------------------------
def draw(gen, n, step, bound):
    """n values, uniform over the multiples of `step` in [-bound, bound], as bf16 (exact)"""
    k = int(round(bound / step))
    v = (torch.randint(-k, k + 1, (n,), generator=gen).double() * step).bfloat16()
    assert float(v.double().abs().max()) <= bound
    return v


def check_exact(K, x, w, bias=None, res=None):
    """The precondition under which the statement defines every output bit (module docstring).  NaN-filled slack and
    don't-care rows are not inputs of any valid row and are left out of the maxima."""
    def amax(t):
        if t is None or t.numel() == 0:
            return 0.0
        t = t.double()
        return float(torch.where(torch.isnan(t), torch.zeros_like(t), t.abs()).max())

    for t, step in ((x, X_STEP), (w, W_STEP), (bias, B_STEP), (res, B_STEP)):
        if t is not None:
            q = t.double() / step
            if not bool(((q == q.round()) | torch.isnan(q)).all()):
                raise NotExact("an operand is not a multiple of its step %g" % step)
    bound = (K * amax(x) * amax(w) + amax(bias) + amax(res)) * 2.0 ** 5
    if not bound < 2.0 ** 24:
        raise NotExact("partial sums may leave fp32's exact range: (K * max|x| * max|w| + max|bias| + max|res|) * 2^5 = %g "
                       ">= 2^24 (K = %d)" % (bound, K))
    return bound


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def conv_cl_statement(x, w, bias, res, frames, Hp, Wp, Cin, Cout, kt, mode=PLAIN, x_off=0, res_off=0):
    """include/alg_hip.h's statement of alg_conv_cl_bf16 on flat buffers (offsets in elements), in fp64 (exact for inputs
    that pass `check_exact`).  x: the flat padded input including its slack; w: [Cout][kt*9][Cin], or for PAIR the packed
    [2*Cout][kt*12][Cin] that pack_conv_pair returns (bias then [2*Cout]); res: flat, y's layout, or None.
      PLAIN   row r of frame t:  sum over (dt, dy, dx, c) of x[(t + dt)*Hp*Wp + r + dy*Wp + dx][c] * w[o][(dt, dy, dx)][c]
      PAIR    GEMM row m of frame t is voxels 2m and 2m + 1: columns [v*Cout, (v + 1)*Cout) of
              sum over (dt, dy, dx < 4, c) of x[(t + dt)*Hp*Wp + 2m + dy*Wp + dx][c] * w[v*Cout + o][(dt, dy, dx)][c]
      STRIDE2 row m = Y*Wp + X of frame t (kt = 1): x row t*Hp*Wp + (Wp + 1) + 2m + dy*Wp + dx
    Returns bf16 [frames][rows per frame][Cout] (PAIR: the two voxels of a GEMM row unfolded, i.e. [frames][Hp*Wp][Cout])
    on x's device.  Rows that are not valid (valid_mask) are don't-care; a valid row must not read x's slack (asserted)."""
    dev = x.device
    hpwp = Hp * Wp
    kw, vox = (4, 2) if mode == PAIR else (3, 1)
    step = 2 if mode != PLAIN else 1                      # x rows between consecutive GEMM rows
    base = Wp + 1 if mode == STRIDE2 else 0
    M = stride2_rows(Hp - 2, Wp) if mode == STRIDE2 else hpwp // vox
    assert mode != STRIDE2 or kt == 1
    assert mode != PAIR or hpwp % 2 == 0
    N, K = vox * Cout, kt * 3 * kw * Cin
    xr = x[x_off:]
    xr = xr[: xr.numel() // Cin * Cin].reshape(-1, Cin).double()
    wd = w.reshape(N, K).double().to(dev)
    taps = torch.tensor([dt * hpwp + dy * Wp + dx for dt in range(kt) for dy in range(3) for dx in range(kw)], device=dev)
    rows = base + step * torch.arange(M, device=dev)
    idx = rows[:, None] + taps[None, :]                   # [M][taps]: x row of (GEMM row, tap) in frame 0
    valid = valid_mask(Hp, Wp, mode).to(dev)
    vrow = valid.reshape(M, vox).any(1) if mode == PAIR else valid
    assert int(idx[vrow].max()) < kt * hpwp, "a valid row reads past its frames"
    last = xr.shape[0] - 1
    assert (frames - 1) * hpwp + int(idx[vrow].max()) <= last, "x is shorter than its frames"
    out = torch.empty(frames, M, N, dtype=torch.bfloat16, device=dev)
    for t in range(frames):
        a = xr[(idx + t * hpwp).clamp(max=last)].reshape(M, K)     # (the clamp can only touch don't-care rows)
        acc = a @ wd.t()
        if bias is not None:
            acc = acc + bias.double().to(dev)[None, :]
        out[t] = acc.float().bfloat16()
    out = out.reshape(frames, M * vox, Cout)
    if res is not None:
        r = res[res_off: res_off + out.numel()].reshape(out.shape)
        out = (out.float() + r.float().to(dev)).bfloat16()
    return out
