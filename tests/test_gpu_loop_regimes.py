"""The memory-bound row and elementwise kernels at the trip counts real sizes reach: a grid-stride loop that wraps, a row
walked in several passes, a reduction split across workgroups.  The other kernel tests run each of these loops exactly once.

Every case is sized from CAPS below (cap + a ragged remainder, so the last pass is partial in blocks and in threads), writes
into a slice of a sentinel-filled buffer with GUARD elements on each side (guards untouched, no sentinel left inside), takes
its inputs from a seeded device generator and compares on the device.

Part A (grid-stride wrap) is exact: torch eager on the device op for op, or torch indexing, under torch.equal; the three
activations keep the tolerance of their present tests against fp64.  Part B (passes over a row, splits of a reduction)
compares with fp64 under the bounds written beside each check.

That the cases bite was tried on an MI355X with two scratch builds of the library, loaded through ALG_HIP_LIB:

  * every grid cap of cfg_step.hip, embed.hip, wan.hip, t5.hip and hunyuan.hip doubled (2048 -> 4096, 4096 -> 8192,
    8192 -> 16384, 64 -> 128): no case of part A wraps any more (each size is below twice its cap) and all 31 report
    `passed`, guards and sentinel checks included -- the cases do not depend on the wrap to pass, only to reach it.
    wan_vae.hip and vae.hip have no grid cap to double: their loops stride by the workgroup (2,048 columns, 512 channels,
    256 items) and the split count comes from gn_splits, so part B enters its regimes through the shape alone;
  * every loop's stride doubled instead, so that each second trip is skipped (`stride * 2` in cfg_step.hip, embed.hip,
    wan.hip, t5.hip, hunyuan.hip; `j += 4096`, `c += 1024` in wan_vae.hip; `i += 512` in upsample_kernel, the third split's
    voxels dropped in gn_partial_kernel).  44 of the 50 cases report `failed`: the wrap cases on torch.equal or the sentinel
    left in the skipped stretch (cfg_ddim_step: 0.19 % / 0.05 % of the elements differ), gelu_erf 1.95 > 2^-7, quick_gelu
    5.3 > 2^-6 * 14.5, silu on the sentinel, softmax_hilo, rms_norm_rows, vae_upsample and both groupnorm tests on their
    bounds.  The 6 that pass are the ones that run one trip by design: the two misaligned-base cases, the misaligned lincomb
    term (n = 8,192), softmax_hilo at cols = ld = 2,048 and rms_norm_rows at Cp = 512.  The present kernel tests of the same
    kernels (tests/test_gpu_loops.py, test_gpu_step.py, test_gpu_t5.py, test_gpu_wan_kernels.py, test_gpu_dit_kernels.py,
    test_gpu_clip.py, test_gpu_wan_vae.py, test_gpu_vae.py) pass on that build, 70 of 74; the 4 that fail are cfg_combine at
    2,096,640 elements, the one present case that wraps."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from alg_amd import _lib
from alg_amd.autoencoder_kl_cogvideox import _Level
from alg_amd.pipeline_hunyuan_video_image2video_lowpass import assemble_first_frame
from alg_amd.pipeline_wan_image2video_lowpass import assemble_channel_concat
from alg_amd.schedulers import CogVideoXDDIMScheduler
from oracle import ddim_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32

# name -> (elements one pass covers, where the figure comes from).  A case below names the entry it is sized from.
CAPS = {
    "cfg_ddim_step.vec": (2048 * 256 * 8, "cfg_step.hip alg_cfg_ddim_step: `want > 2048 ? 2048 : want` blocks x 256 x 8 elements"),
    "cfg_ddim_step.scalar": (2048 * 256, "cfg_step.hip alg_cfg_ddim_step: `want > 2048 ? 2048 : want` blocks x 256"),
    "lincomb.scalar": (4096 * 256, "cfg_step.hip alg_lincomb: `want > 4096 ? 4096 : want` blocks x 256"),
    "lincomb.bf16x8": (8192 * 256 * 8, "cfg_step.hip alg_lincomb: `wantv > 8192 ? 8192 : wantv` blocks x 256 x 8 elements"),
    "unipc_update": (4096 * 256, "cfg_step.hip alg_unipc_update: `want > 4096 ? 4096 : want` blocks x 256"),
    # a row gets min(64, ceil(R / 1024)) blocks: below the cap of 64 a thread already takes about four elements, so the
    # row loop wraps from R > 256; R = 16,512 is 17 blocks = 4,352 threads, four trips, the last one short
    "concat_cast.row": (64 * 256, "cfg_step.hip alg_concat_cast: `gx > 64 ? 64 : gx` blocks x 256, gx = (R + 1023) / 1024"),
    "patchify": (4096 * 256, "embed.hip alg_patchify_t: `want > 4096 ? 4096 : want` blocks x 256 threads of p elements"),
    "unpatchify": (4096 * 256, "embed.hip alg_unpatchify_t: `want > 4096 ? 4096 : want` blocks x 256"),
    "wan.grid_for": (8192 * 256, "wan.hip grid_for: `want > 8192 ? 8192 : want` blocks x 256 (patchify3d, unpatchify3d, "
                                 "wan_modulation, gelu_erf)"),
    "t5.grid_for": (8192 * 256, "t5.hip grid_for: `want > 8192 ? 8192 : want` blocks x 256 (embed_rows in 16-byte chunks, "
                                "quick_gelu, mul_bf16)"),
    "silu": (4096 * 256, "hunyuan.hip alg_silu: `want > 4096 ? 4096 : want` blocks x 256"),
    "softmax_hilo.pass": (256 * 8, "wan_vae.hip softmax_hilo_kernel: `j += 2048`, one workgroup of 256 x 8 columns per row"),
    "rms_norm_rows.trip": (64 * 8, "wan_vae.hip rms_norm_rows_kernel: `c += 512`, one wave of 64 x 8 channels per row"),
    "vae_upsample.trip": (256, "vae.hip upsample_kernel: `i += 256` over (2W + 2) * C / 8 items of a row"),
    "gn_splits.voxels": (256, "vae.hip gn_splits: `(hw + 255) / 256` splits of a frame, at most 64 and 2048 / frames"),
}
GUARD = 4096
SENTINEL = -(2.0 ** 120)          # exact in bf16 and fp32, far outside anything a case computes


def cap(name):
    return CAPS[name][0]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, dtype=F32, scale=1.0):
    x = torch.randn(shape, generator=g, device=DEV)
    return (x * scale if scale != 1.0 else x).to(dtype)


class Guarded:
    """`out`: n elements inside a sentinel-filled buffer, GUARD elements behind it and `lead` (>= GUARD) in front.  lead a
    multiple of 8 keeps the 16-byte alignment of the allocation; GUARD + 1 makes a misaligned base."""

    def __init__(self, n, dtype, lead=GUARD):
        assert lead >= GUARD
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.out = self.buf[lead:lead + n]
        assert (self.out.data_ptr() % 16 == 0) == (lead % 8 == 0)

    def check(self, written=True):
        b = self.buf
        assert bool((b[:self.lead] == SENTINEL).all()) and bool((b[self.lead + self.n:] == SENTINEL).all()), "a guard was written"
        if written:
            assert not bool((self.out == SENTINEL).any()), "a sentinel is left inside the output"


def _ragged(n_cap, rem, vec8=False):
    assert rem % 256 != 0 and 0 < rem < n_cap
    if vec8:
        assert rem % 8 == 0 and rem % 2048 != 0
    return n_cap + rem


# ---------------------------------------------------------------------------------------------------------------------
# A. grid-stride wrap
# ---------------------------------------------------------------------------------------------------------------------

def _ddim_reference(pred, lat, n_pass, gs, orc, t):
    """cog:1091-1123 with torch ops on the device, as tests/test_gpu_step.py states it."""
    noise = pred.float()
    if n_pass == 3:
        u0, u, tx = noise.chunk(3)
        noise = u0 + gs * (tx - u)
    elif n_pass == 2:
        u, tx = noise.chunk(2)
        noise = u + gs * (tx - u)
    return orc.step(noise, t, lat).to(lat.dtype)


def _ddim_pair():
    sched, orc = CogVideoXDDIMScheduler(), ddim_oracle.DDIMOracle()
    sched.set_timesteps(50)
    orc.set_timesteps(50)
    return sched, orc, sched.timesteps[17]


@pytest.mark.parametrize("pred_dtype", [BF, F32])
@pytest.mark.parametrize("path", ["vec", "scalar"])
def test_cfg_ddim_step_wraps(pred_dtype, path):
    # CAPS["cfg_ddim_step.vec"] / ["cfg_ddim_step.scalar"]: one pass + 1,003 groups of 8 / + 261 (odd: the scalar kernel)
    numel = _ragged(cap("cfg_ddim_step.vec"), 8 * 1003, vec8=True) if path == "vec" else _ragged(cap("cfg_ddim_step.scalar"), 261)
    g = _gen(31)
    pred = _randn((3, numel), g, pred_dtype)
    lat = _randn((1, numel), g, BF)
    sched, orc, t = _ddim_pair()
    want = _ddim_reference(pred, lat, 3, 6.0, orc, t)
    o = Guarded(numel, BF)
    o.out.copy_(lat[0])
    sched.fused_cfg_step_(pred, o.out, 3, 6.0, t)
    assert torch.equal(o.out, want[0]), (o.out != want[0]).float().mean().item()
    o.check()


@pytest.mark.parametrize("pred_dtype", [BF, F32])
def test_cfg_ddim_step_misaligned_base_takes_the_scalar_path(pred_dtype):
    # numel % 8 == 0 and an aligned pred, latents at buf[1:1 + n]: the launcher's `(uintptr_t)latents % 16` test alone sends
    # the call to the scalar kernel; the bits are those of the aligned (vector) call
    n = 8192
    g = _gen(32)
    pred, lat = _randn((3, n), g, pred_dtype), _randn((n,), g, BF)
    sched, orc, t = _ddim_pair()
    al, mis = Guarded(n, BF), Guarded(n, BF, lead=GUARD + 1)
    for o in (al, mis):
        o.out.copy_(lat)
        sched.fused_cfg_step_(pred, o.out, 3, 6.0, t)
        o.check()
    assert torch.equal(mis.out, al.out)
    assert torch.equal(al.out, _ddim_reference(pred, lat[None], 3, 6.0, orc, t)[0])


@pytest.mark.parametrize("od", [BF, F32])
def test_lincomb_scalar_kernel_wraps(od):
    n = _ragged(cap("lincomb.scalar"), 1001)                    # CAPS["lincomb.scalar"]
    g = _gen(33)
    x, v, w, u = _randn((n,), g), _randn((n,), g, BF), _randn((n,), g), _randn((n,), g, BF)
    want = (0.75 * x + (0.3 * v) + (-1.5) * w + 2.0 * u).to(od)  # each product in its tensor's dtype, fp32 running sum
    o = Guarded(n, od)
    _lib.lincomb([(0.75, x), (0.3, v), (-1.5, w), (2.0, u)], od, out=o.out)
    assert torch.equal(o.out, want)
    o.check()


def _bf16_sum4(a, b, c, d):
    """The all-bf16 kernels: each product rounded to bf16, an fp32 running sum, one rounding at the store."""
    return ((1.0 * a).float() + (0.5 * b) + (-1.25 * c) + (3.0 * d)).to(BF)


def test_lincomb_bf16x8_kernel_wraps_in_place():
    n = _ragged(cap("lincomb.bf16x8"), 8 * 777, vec8=True)      # CAPS["lincomb.bf16x8"]; 33.6 MB a term
    g = _gen(34)
    o = Guarded(n, BF)
    o.out.copy_(_randn((n,), g, BF))
    b, c, d = (_randn((n,), g, BF) for _ in range(3))
    want = _bf16_sum4(o.out, b, c, d)
    got = _lib.lincomb([(1.0, o.out), (0.5, b), (-1.25, c), (3.0, d)], BF, out=o.out)   # in place on term 0
    assert got is o.out and torch.equal(o.out, want)
    o.check()


def test_lincomb_one_misaligned_term_falls_back():
    n = 8192
    g = _gen(35)
    a, b, c, d = (_randn((n,), g, BF) for _ in range(4))
    shifted = torch.zeros(n + 8, dtype=BF, device=DEV)[1:1 + n]
    shifted.copy_(c)
    assert shifted.data_ptr() % 16 == 2
    al, mis = Guarded(n, BF), Guarded(n, BF)
    _lib.lincomb([(1.0, a), (0.5, b), (-1.25, c), (3.0, d)], BF, out=al.out)
    _lib.lincomb([(1.0, a), (0.5, b), (-1.25, shifted), (3.0, d)], BF, out=mis.out)
    al.check(), mis.check()
    assert torch.equal(mis.out, al.out) and torch.equal(al.out, _bf16_sum4(a, b, c, d))


def _unipc_into(out, x, m0, m1, m_new, r, c, k, rk=1.0, rho0=0.0, rho_new=0.0):
    """_lib.unipc_update with the output where the test wants it (the wrapper allocates its own)."""
    _lib._check(_lib.load_library().alg_unipc_update(_lib._p(x), _lib._p(m0), _lib._p(m1), _lib._p(m_new), _lib._p(out), x.numel(),
                                                      r, c, k, rk, rho0, rho_new, _lib._stream()), "alg_unipc_update")


@pytest.mark.parametrize("case", ["p1", "c2"])
def test_unipc_update_wraps(case):
    n = _ragged(cap("unipc_update"), 999)                       # CAPS["unipc_update"]
    g = _gen(36)
    x, m0, m1, mt = (_randn((n,), g) for _ in range(4))
    r, c, k, rk, rho0, rho1 = 0.97, -0.031, -0.029, -1.7, 0.52, 0.49
    rkt = torch.tensor(rk, dtype=F32)                            # the published scheduler divides by a CPU 0-dim fp32 tensor
    o = Guarded(n, F32)
    if case == "p1":
        _unipc_into(o.out, x, m0, None, None, r, c, k)
        got, want = _lib.unipc_update(x, m0, None, None, r, c, k), (r * x - c * m0) - k * 0
    else:
        _unipc_into(o.out, x, m0, m1, mt, r, c, k, rk, rho0, rho1)
        got = _lib.unipc_update(x, m0, m1, mt, r, c, k, rk, rho0, rho1)
        want = (r * x - c * m0) - k * (rho0 * ((m1 - m0) / rkt) + rho1 * (mt - m0))
    assert torch.equal(o.out, want) and torch.equal(got, want)
    o.check()


def _concat_cast_into(out, src0, src1, O, A0, A1, R, s0_ostride, s1_ostride, a1_off):
    """_lib.concat_cast with the output where the test wants it (the wrapper allocates its own)."""
    n = len(src0)
    a0 = (ctypes.c_void_p * n)(*[t.data_ptr() for t in src0])
    a1 = (ctypes.c_void_p * n)(*[t.data_ptr() for t in src1])
    _lib._check(_lib.load_library().alg_concat_cast(a0, _lib._dt(src0[0]), a1, _lib._dt(src1[0]), n, O, A0, A1, R, s0_ostride,
                                                     s1_ostride, a1_off, _lib._p(out), _lib._dt(out), _lib._stream()),
                "alg_concat_cast")


@pytest.mark.parametrize("mode", ["f32_to_bf16", "mixed_to_f32"])
def test_concat_cast_row_wraps(mode):
    # CAPS["concat_cast.row"]: R = 129 * 128 = 16,512 elements a row; three samples (B = 1, three passes)
    H, W = 129, 128
    g = _gen(37)
    lat_dt, od = (F32, BF) if mode == "f32_to_bf16" else (BF, F32)
    # wan:877-889 channel concat (O = 1, A = channels, R = F * H * W)
    lat = _randn((1, 4, 1, H, W), g, lat_dt)
    c0, c1 = _randn((1, 5, 1, H, W), g), _randn((1, 5, 1, H, W), g)
    want = torch.cat([torch.cat([lat] * 3), torch.cat([c0, c1, c1], dim=0)], dim=1).to(od)
    got = assemble_channel_concat(lat, [c0, c1, c1], od)
    assert got.shape == (3, 9, 1, H, W) and torch.equal(got, want)
    o = Guarded(want.numel(), od)
    R = H * W
    _concat_cast_into(o.out, [lat[0]] * 3, [c0[0], c1[0], c1[0]], 1, 4, 5, R, 4 * R, 5 * R, 0)
    assert torch.equal(o.out, want.reshape(-1))
    o.check()
    # hy:1146-1160 first-frame replace (O = channels, A = frames, R = H * W)
    lat = _randn((1, 3, 3, H, W), g, lat_dt)
    img, lp = _randn((1, 3, 1, H, W), g), _randn((1, 3, 1, H, W), g)
    want = torch.cat([torch.cat([img, lp, lp], dim=0), torch.cat([lat] * 3)[:, :, 1:]], dim=2).to(od)
    got = assemble_first_frame(lat, [img, lp, lp], od)
    assert got.shape == (3, 3, 3, H, W) and torch.equal(got, want)
    o = Guarded(want.numel(), od)
    _concat_cast_into(o.out, [img[0], lp[0], lp[0]], [lat[0]] * 3, 3, 1, 2, R, R, 3 * R, 1)
    assert torch.equal(o.out, want.reshape(-1))
    o.check()


@pytest.mark.parametrize("Fr,pt", [(5, 1), (6, 2)])
def test_patchify_unpatchify_wrap(Fr, pt):
    # CAPS["patchify"], CAPS["unpatchify"]: 3 * 5 * 32 * 60 * 45 = 3 * 5 * 16 * 60 * 90 = 1,296,000 threads (p_t = 2: 1,555,200)
    n, C, H, W, p = 3, 16, 60, 90, 2
    assert n * Fr * 2 * C * H * (W // p) > cap("patchify") and n * Fr * C * H * W > cap("unpatchify")
    g = _gen(38 + pt)
    shared = pt == 1                                            # one latent for every sample (batch stride 0), or one each
    lat = _randn((1 if shared else n, Fr, C, H, W), g, BF)
    conds = [_randn((1, Fr, C, H, W), g, BF) for _ in range(n)]
    gh, gw, K = H // p, W // p, 2 * C * pt * p * p
    rows = (Fr // pt) * gh * gw
    o = Guarded(n * rows * K, BF)
    _lib.patchify(lat, 0 if shared else Fr * C * H * W, conds, o.out, n, Fr, C, H, W, p, pt)
    for i in range(n):
        x = torch.cat([lat[0 if shared else i], conds[i][0]], dim=1)            # [F, 2C, H, W] (cog:1068-1070)
        ref = x.reshape(Fr // pt, pt, 2 * C, gh, p, gw, p).permute(0, 3, 5, 2, 1, 4, 6).reshape(rows, K)   # k = (c, t, py, px)
        assert torch.equal(o.out.view(n, rows, K)[i], ref), i
    o.check()
    K = C * pt * p * p
    tok = _randn((n, rows, K), g, BF)
    o = Guarded(n * Fr * C * H * W, BF)
    _lib.unpatchify(tok, o.out, n, Fr, C, H, W, p, pt)
    ref = tok.reshape(n, Fr // pt, gh, gw, C, pt, p, p).permute(0, 1, 5, 4, 2, 6, 3, 7).reshape(n, Fr, C, H, W)
    assert torch.equal(o.out.view(n, Fr, C, H, W), ref)
    o.check()


# The shapes of the Wan 480p call (first of each list below) exceed the cap by a whole number of blocks: 192, 104 * 60 and 5,120
# bring a factor of 256 with them.  The second shape of each list leaves a last block that is partly idle as well.
@pytest.mark.parametrize("N,Fr,H,W", [(2, 4, 60, 104), (1, 7, 60, 106)])
def test_patchify3d_wraps_with_zero_k_padding(N, Fr, H, W):
    C, Kpad = 36, 192                                           # CAPS["wan.grid_for"]: 2 * 4 * 30 * 52 * 192 = 2,396,160
    S = Fr * (H // 2) * (W // 2)
    assert cap("wan.grid_for") < N * S * Kpad < 2 * cap("wan.grid_for") and (N == 2 or N * S * Kpad % 256)
    x = _randn((N, C, Fr, H, W), _gen(40), BF)
    o = Guarded(N * S * Kpad, BF)
    _lib.patchify3d(x, o.out, N, C, Fr, H, W, 2, 2, Kpad)
    out = o.out.view(N, S, Kpad)
    ref = x.view(N, C, Fr, H // 2, 2, W // 2, 2).permute(0, 2, 3, 5, 1, 4, 6).reshape(N, S, C * 4)
    assert torch.equal(out[:, :, :C * 4], ref) and not bool(out[:, :, C * 4:].any())
    o.check()


@pytest.mark.parametrize("channel_major", [False, True])
@pytest.mark.parametrize("H,W", [(60, 104), (62, 102)])
def test_unpatchify3d_wraps(H, W, channel_major):
    N, C, Fr, ldin = 2, 16, 11, 80                              # CAPS["wan.grid_for"]: 2 * 16 * 11 * 60 * 104 = 2,196,480
    gh, gw = H // 2, W // 2
    assert cap("wan.grid_for") < N * C * Fr * H * W < 2 * cap("wan.grid_for") and ldin > C * 4
    assert H == 60 or N * C * Fr * H * W % 256
    tok = _randn((N, Fr * gh * gw, ldin), _gen(41), BF)
    o = Guarded(N * C * Fr * H * W, BF)
    _lib.unpatchify3d(tok, ldin, o.out, N, C, Fr, H, W, 2, 2, channel_major)
    t = tok[:, :, :C * 4]
    if channel_major:                                            # column = c * 4 + py * 2 + px
        ref = t.reshape(N, Fr, gh, gw, C, 2, 2).permute(0, 4, 1, 2, 5, 3, 6)
    else:                                                        # column = (py * 2 + px) * C + c
        ref = t.reshape(N, Fr, gh, gw, 2, 2, C).permute(0, 6, 1, 2, 4, 3, 5)
    assert torch.equal(o.out.view(N, C, Fr, H, W), ref.reshape(N, C, Fr, H, W))
    o.check()


@pytest.mark.parametrize("vec_per_j", [True, False])
@pytest.mark.parametrize("D", [5120, 5004])
def test_wan_modulation_wraps(D, vec_per_j):
    L, N, J = 40, 2, 6                                          # CAPS["wan.grid_for"]: 40 * 2 * 6 * 5120 = 2,457,600
    assert cap("wan.grid_for") < L * N * J * D < 2 * cap("wan.grid_for") and (D == 5120 or L * N * J * D % 256)
    g = _gen(42)
    table = _randn((L, J, D), g)
    vec = _randn((N, J * D if vec_per_j else D), g, BF)
    o = Guarded(L * N * J * D, F32)
    _lib.wan_modulation(table, vec, o.out, L, N, J, D, vec_per_j)
    want = table[:, None] + vec.float().view(1, N, J if vec_per_j else 1, D)
    assert torch.equal(o.out.view(L, N, J, D), want)
    o.check()


def _activation_input(n, g, scale, clamp=None):
    """The input inside its guarded buffer (the activations run in place)."""
    o = Guarded(n, BF)
    x = _randn((n,), g, F32, scale)
    o.out.copy_(x if clamp is None else x.clamp(-clamp, clamp))
    return o, o.out.clone().double()


def test_gelu_erf_wraps():
    # CAPS["wan.grid_for"].  |x| <= 2 keeps |gelu(x)| < 2, where the bf16 half-ulp is at most 2^-8: the 2^-7 of the present test
    # (tests/test_gpu_wan_kernels.py) then leaves 2^-8 for the arithmetic instead of sitting exactly on a rounding tie in [2, 4)
    n = _ragged(cap("wan.grid_for"), 333)
    o, x = _activation_input(n, _gen(43), 1.0, clamp=2.0)
    _lib.gelu_erf_(o.out)
    ref = 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    assert (o.out.double() - ref).abs().max().item() <= 2.0 ** -7
    o.check(written=False)


def test_quick_gelu_wraps():
    n = _ragged(cap("t5.grid_for"), 77)                         # CAPS["t5.grid_for"]; 3 * randn as tests/test_gpu_clip.py
    o, x = _activation_input(n, _gen(44), 3.0)
    _lib.quick_gelu_(o.out)
    ref = x * torch.sigmoid(1.702 * x)
    assert (o.out.double() - ref).abs().max().item() <= 2.0 ** -6 * ref.abs().max().item()
    # That bound is relative to the largest output (about 15 here): f(f(x)) - f(x) never exceeds 0.12, so an element
    # computed twice would hide under it.  Per element, from the kernel's three bf16 roundings (each <= 2^-8 relative):
    # the product and the sigmoid give 2 * 2^-8 |ref|; the rounded argument a = 1.702 x moves the sigmoid by
    # <= 2^-8 |a| (1 - sigmoid(a)) relative, which is <= 0.28 * 2^-8 for a > 0 and, for a < 0, an absolute
    # 2^-8 |x| (2 + |a|) e^-|a| <= 0.7 * 2^-8 in the output.  2.5 |ref| + 0.75 covers both with room for the fp32 arithmetic.
    assert bool(((o.out.double() - ref).abs() <= 2.0 ** -8 * (2.5 * ref.abs() + 0.75)).all())
    o.check(written=False)


def test_mul_bf16_wraps():
    n = _ragged(cap("t5.grid_for"), 333)                        # CAPS["t5.grid_for"]
    g = _gen(45)
    a, b = _randn((n,), g, BF), _randn((n,), g, BF)
    o = Guarded(n, BF)
    _lib.mul_bf16(a, b, o.out)
    assert torch.equal(o.out, a * b)
    o.check()


def test_silu_wraps():
    n = _ragged(cap("silu"), 19)                                # CAPS["silu"]; |x| <= 2 for the reason given at gelu_erf
    g = _gen(46)
    x = _randn((n,), g).clamp(-2.0, 2.0).to(BF)
    o = Guarded(n, BF)
    _lib.silu(x, o.out)
    ref = F.silu(x.double())
    assert (o.out.double() - ref).abs().max().item() <= 2.0 ** -7
    o.check()


def test_embed_rows_wraps_and_clamps():
    n, vocab, D = 4100, 50, 4096                                # CAPS["t5.grid_for"]: 4,100 * 512 chunks of 16 bytes = 2,099,200
    assert n * (D // 8) > cap("t5.grid_for")
    g = _gen(47)
    table = _randn((vocab, D), g, BF)
    ids = torch.randint(-3, vocab + 3, (n,), generator=g, device=DEV)
    ids[-1], ids[0], ids[n // 2] = vocab + 7, -1, vocab          # the last row, computed in the second pass, clamps too
    assert bool((ids < 0).any()) and bool((ids >= vocab).any())
    o = Guarded(n * D, BF)
    _lib.embed_rows(ids, table, o.out)
    assert torch.equal(o.out.view(n, D), table[ids.clamp(0, vocab - 1)])
    o.check()


# ---------------------------------------------------------------------------------------------------------------------
# B. more than one pass over a row, more than one split
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols,ld", [(2048, 2048), (2048, 2048 + 64), (2049, 2112), (2059, 2112), (6240, 6272)])
def test_softmax_hilo_passes(cols, ld):
    # CAPS["softmax_hilo.pass"]: exactly one pass, one column / eleven columns into the second, and the Wan 480p row (4 passes)
    rows, scale = 9, 0.37
    assert ld >= cols and ld % 64 == 0 and (cols + 63) // 64 * 64 in (ld, ld - 64)
    g = _gen(50 + cols % 7)
    s = _randn((rows, cols), g, F32, 6.0)
    s[0, min(2050, cols - 2)] = s[0].max() + 3.0                # row 0: the maximum sits in a later pass (where there is one)
    s[1, cols - 1] = s[1].max() + 3.0                           # row 1: the maximum is the last valid column
    hi = s.to(BF)
    lo = (s - hi.float()).to(BF)
    neg_hi = torch.full((rows, ld), 7.0, dtype=BF, device=DEV)   # junk in the padding columns: lo - neg_hi = 3e4 - 7 would
    lo_p = torch.full((rows, ld), 3e4, dtype=BF, device=DEV)     # win every maximum if it were read
    neg_hi[:, :cols], lo_p[:, :cols] = -hi, lo
    o = Guarded(rows * ld, BF)
    _lib.softmax_hilo(neg_hi, lo_p, o.out, rows, cols, ld, scale)
    p = o.out.view(rows, ld).double()
    ref = torch.softmax((hi.double() + lo.double()) * scale, dim=1)
    # 2^-8: the half-ulp of the bf16 result; 2^-12: room for the fp32 exponent and sum
    excess = ((p[:, :cols] - ref).abs() - (2.0 ** -8 + 2.0 ** -12) * ref).max().item()
    worst = ((p[:, :cols] - ref).abs() / ref).max().item()
    print("softmax_hilo cols=%d ld=%d: worst relative error %.5f" % (cols, ld, worst))
    assert excess <= 0.0, worst
    assert (p[:, :cols].sum(1) - 1.0).abs().max().item() <= 2.0 ** -8
    assert not bool(o.out.view(rows, ld)[:, cols:].any())
    o.check()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C,Cp", [(384, 512), (515, 520), (1000, 1024)])
def test_rms_norm_rows_trips(C, Cp, silu):
    # CAPS["rms_norm_rows.trip"]: Cp = 512 is one full trip, 520 leaves the second trip to lane 0 alone, 1,024 is two full trips
    rows, zero_row = 37, 5
    g = _gen(60 + C % 11)
    x = _randn((rows, Cp), g, BF)
    x[:, C:] = (50.0 * torch.randn(rows, Cp - C, generator=g, device=DEV)).to(BF)   # junk the statistics must not see
    x[zero_row, :C] = 0
    gamma = torch.zeros(Cp, dtype=BF, device=DEV)
    gamma[:C] = (1 + 0.1 * torch.randn(C, generator=g, device=DEV)).to(BF)
    o = Guarded(rows * Cp, BF)
    _lib.rms_norm_rows(x, gamma, o.out, rows, C, Cp, silu)
    y = o.out.view(rows, Cp)
    ref = F.normalize(x.double()[:, :C], dim=1) * C ** 0.5 * gamma.double()[:C]
    ref = F.silu(ref) if silu else ref
    assert (y[:, :C].double() - ref).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item()
    assert not bool(y[:, C:].any())
    assert not bool(y[zero_row].any())                           # F.normalize's eps: an all-zero row gives zeros, not NaN
    o.check()


def _virtual(x, fill=float("nan")):
    """NCTHW (B = 1) on the device -> virtual layout [T][H + 2][W + 2][C] bf16, `fill` in the don't-care rows."""
    return F.pad(x, (0, 2, 0, 2), value=fill)[0].permute(1, 2, 3, 0).contiguous().to(BF).reshape(-1)


@pytest.mark.parametrize("compress,single", [(True, True), (True, False), (False, True)])
def test_vae_upsample_trips(compress, single):
    C, T, H, W = 128, 5, 4, 20                                  # CAPS["vae_upsample.trip"]: 42 * 16 = 672 items a row, 3 trips
    assert 2 * cap("vae_upsample.trip") < (2 * W + 2) * (C // 8) < 3 * cap("vae_upsample.trip")
    x = _randn((1, C, T, H, W), _gen(70), BF).float()
    if compress:
        want = F.interpolate(x, scale_factor=2.0) if not single else torch.cat(
            [F.interpolate(x[:, :, 0], scale_factor=2.0)[:, :, None], F.interpolate(x[:, :, 1:], scale_factor=2.0)], 2)
    else:
        want = x.repeat_interleave(2, 3).repeat_interleave(2, 4)
    T2 = want.shape[2]
    o = Guarded(T2 * (2 * H + 2) * (2 * W + 2) * C, BF)
    _lib.vae_upsample(_virtual(x), o.out, T2, H, W, C, compress, single)
    got = o.out.view(T2, 2 * H + 2, 2 * W + 2, C)
    assert torch.equal(got[:, 1:-1, 1:-1].permute(3, 0, 1, 2).float(), want[0])
    assert not bool(got[:, 0].any() or got[:, -1].any() or got[:, :, 0].any() or got[:, :, -1].any())
    o.check()


def _gn_setup(C, x):
    """5 latent frames at 17 x 31 with the segment layout of the batched decode (_Level, rate 1, scale 1), the launch of
    alg_vae_groupnorm_stats into guarded buffers, and the fp64 statistics of each segment."""
    L, h, w = 5, 17, 31                                         # CAPS["gn_splits.voxels"]: 527 voxels = 3 splits of 176, 176, 175
    lv = _Level(L, h, w, 1, 1)
    T, H, W = lv.T, lv.H, lv.W
    assert (T, H, W) == (5, 17, 31) and 2 * cap("gn_splits.voxels") < H * W <= 3 * cap("gn_splits.voxels")
    geom = _lib.vae_geom(frames=T, H=H, W=W, C=C, first_len=lv.first_len, seg_len=lv.seg_len, lat_first_single=int(lv.single),
                         lat_rate=1, lat_scale=1, lat_h=h, lat_w=w)
    segs = [list(range(lv.first_len))] + [list(range(f, min(f + lv.seg_len, T))) for f in range(lv.first_len, T, lv.seg_len)]
    assert segs == [[0, 1, 2], [3, 4]]
    ws_bytes = _lib.vae_groupnorm_workspace(geom)
    assert ws_bytes == T * 3 * 32 * 2 * 4                        # three splits a frame
    ws, stats = Guarded(ws_bytes // 4, F32), Guarded(len(segs) * 64, F32)
    xv = _virtual(x)
    _lib.vae_groupnorm_stats(xv, geom, 1e-6, ws.out, stats.out)
    want = []
    for fr in segs:
        sg = x[0][:, fr].double().reshape(32, -1)               # a group = C / 32 consecutive channels, every voxel of the segment
        want.append(torch.stack([sg.mean(1), (sg.var(1, unbiased=False) + 1e-6).rsqrt()], 1))
    ws.check(), stats.check()
    return geom, segs, xv, stats, torch.stack(want)


def _stats_close(stats, want):
    got = stats.out.view(-1, 32, 2).double()
    print("groupnorm statistics: worst relative error %.3e" % ((got - want).abs() / want.abs().clamp_min(0.1)).max().item())
    return torch.allclose(got, want, rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("C", [128, 512, 1024, 2048])
def test_vae_groupnorm_three_splits(C):
    # C = 1024 / 2048: `lanes = 256 / chunks` of gn_partial_kernel is 2 / 1
    g = _gen(80 + C // 128)
    T, H, W = 5, 17, 31
    x = _randn((1, C, T, H, W), g, BF, 2.0).float() + 0.5
    x = x.to(BF).float()
    gamma = (1 + 0.2 * torch.randn(C, generator=g, device=DEV)).to(BF)
    beta = (0.2 * torch.randn(C, generator=g, device=DEV)).to(BF)
    zy, zb = _randn((1, C, T, H, W), g, BF).float(), _randn((1, C, T, H, W), g, BF).float()
    geom, segs, xv, stats, stats_want = _gn_setup(C, x)
    assert _stats_close(stats, stats_want)
    # the reference's group norm from the fp64 statistics, then its per-op bf16 roundings
    mean = torch.cat([stats_want[i, :, 0].repeat_interleave(C // 32)[:, None].expand(C, len(fr)) for i, fr in enumerate(segs)], 1)
    rstd = torch.cat([stats_want[i, :, 1].repeat_interleave(C // 32)[:, None].expand(C, len(fr)) for i, fr in enumerate(segs)], 1)
    n = ((x[0].double() - mean[:, :, None, None]) * rstd[:, :, None, None] * gamma.double()[:, None, None, None]
         + beta.double()[:, None, None, None]).to(BF).float()
    tol = lambda want: 2.0 ** -6 * max(1.0, want.abs().max().item())

    def inner(o):
        got = o.out.view(T + 2, H + 2, W + 2, C)
        assert not bool(got[:, 0].any() or got[:, -1].any() or got[:, :, 0].any() or got[:, :, -1].any())
        assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[2])
        return got[2:, 1:-1, 1:-1].permute(3, 0, 1, 2).float()

    # CogVideoXSpatialNorm3D + SiLU (lat_rate = lat_scale = 1: zq is at the activation's resolution)
    zyb = F.pad(torch.cat([zy, zb], 1), (1, 1, 1, 1))
    zyb = torch.cat([zyb[:, :, :1]] * 2 + [zyb], 2)[0].permute(1, 2, 3, 0).contiguous().to(BF)
    o = Guarded((T + 2) * (H + 2) * (W + 2) * C, BF)
    _lib.vae_spatial_norm(xv, stats.out, gamma, beta, zyb, o.out, geom, silu=True)
    a = ((n * zy[0]).to(BF).float() + zb[0]).to(BF).float()
    want = F.silu(a).to(BF).float()
    err = (inner(o) - want).abs()
    assert err.max().item() <= tol(want) and err.mean().item() < 1e-3
    o.check()
    # plain GroupNorm + SiLU (the encoder's norms)
    o = Guarded((T + 2) * (H + 2) * (W + 2) * C, BF)
    _lib.vae_group_norm(xv, stats.out, gamma, beta, o.out, geom, silu=True)
    want = F.silu(n).to(BF).float()
    err = (inner(o) - want).abs()
    assert err.max().item() <= tol(want) and err.mean().item() < 1e-3
    o.check()
    stats.check()


def test_vae_groupnorm_stats_with_a_large_mean():
    # |mean| / std = 16: the one-pass sum x, sum x^2 in fp32 partials loses log2(16^2) = 8 bits of the variance to cancellation;
    # the partials are short (176 voxels x 4 channels) and their reduction is in double, which keeps the statistics inside rtol
    C = 128
    x = (8.0 + 0.5 * torch.randn(1, C, 5, 17, 31, generator=_gen(90), device=DEV)).to(BF).float()
    _, _, _, stats, stats_want = _gn_setup(C, x)
    assert _stats_close(stats, stats_want)
