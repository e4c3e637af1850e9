"""The e4m3 self-attention scheme on the CPU: its eager restatement (tests/helpers/attn_fp8_ref.py) against float64, the V^T
column order against the MFMA lane layouts, and the C ABI names.

Bound of the restatement.  The only rounding the scheme adds to float64 attention on the de-quantised operands is P -> e4m3 at
the scale 2^3 (l is the fp32 sum of the unrounded values).  A converted value y has |e4m3(y) - y| <= max(2^-4 y, 2^-10): three
mantissa bits, subnormal spacing 2^-9.  So per output element
    |O~ - O| <= sum_k max(2^-4 y_k, 2^-10) |v_kd| / l  <=  (2^-4 + n 2^-10 / l) max_k |v_kd|,
and l >= 8: the key holding the row maximum contributes 2^3 * 2^((s_max - m) c) >= 2^3 because the offset m never exceeds the
largest score seen.  With the bf16 rounding of the output (2^-9 relative) and fp32 sums in between (2^-16 is generous):
    |out - ref| <= (2^-4 + n 2^-13) max_k |v_kd| + 2^-8 |ref|."""
import math
import os
import re

import pytest
import torch

import alg_amd
from helpers import attn_fp8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alg_flash_attn_d128_fp8", "alg_quantize_fp8_khead", "alg_quantize_fp8_vt", "alg_rmsnorm_rope_fp8", "alg_headnorm_rope_fp8")
SCALE = 1.0 / math.sqrt(128)


def _operands(N, Sq, Skv, H, seed, kind, far_first_tile=False):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(N, s, H, 128, generator=g) for s in (Sq, Skv, Skv))
    if kind == "trained_like":            # QK gains near 3 and a bias component shared by all tokens of a head
        gq, gk = (3.0 + 0.3 * torch.randn(H, 128, generator=g) for _ in range(2))
        bq, bk = (0.5 * torch.randn(H, 128, generator=g) for _ in range(2))
        q, k = q * gq + bq, k * gk + bk
        v = v * (1.0 + 0.5 * torch.randn(H, 128, generator=g)) + 0.3 * torch.randn(H, 128, generator=g)
    if far_first_tile:
        k[:, :64] *= 0.02
        k[:, 64:] *= 2.5
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


@pytest.mark.parametrize("kind", ["gauss", "trained_like"])
@pytest.mark.parametrize("N,Sq,Skv,H,far", [(1, 70, 200, 2, False), (2, 33, 37, 1, False), (1, 64, 704, 2, False),
                                            (1, 70, 200, 2, True), (1, 64, 704, 2, True)])
def test_restatement_against_float64(N, Sq, Skv, H, far, kind):
    """far: the first 64-key tile lies far below the later maximum, so the offset set on tile 0 has to grow afterwards."""
    q, k, v = _operands(N, Sq, Skv, H, Sq + Skv, kind, far)
    q8, qs = R.quantize_rows(q)
    k8, ks = R.quantize_khead(k)
    v8, vs = R.quantize_vt(v)
    assert float(q8.abs().max()) == 448.0 and float(k8.abs().max()) == 448.0 and float(v8.abs().max()) == 448.0
    vd = v8 * vs[:, None]
    ref = R.attention_f64(q8 * qs[..., None], k8 * ks[:, None, :, None], vd, SCALE)
    stats = {}
    out = R.attention_fp8(q8, qs, k8, ks, v8, vs, SCALE, stats)
    assert out.dtype == torch.bfloat16 and torch.isfinite(out.float()).all()
    vmax = vd.abs().amax(dim=1)[:, None].double()                      # [N, 1, H, 128]
    bound = (2.0 ** -4 + Skv * 2.0 ** -13) * vmax + 2.0 ** -8 * ref.abs()
    err = (out.double() - ref).abs()
    rel = ((out.double() - ref).norm() / ref.norm()).item()
    print("%s far=%s N%d Sq%d Skv%d: rel L2 %.3e, worst element %.3e of its bound; %d of %d steps exact, largest converted %.1f"
          % (kind, far, N, Sq, Skv, rel, (err / bound).max().item(), stats["exact"], stats["tiles"], stats["p_max"]))
    assert bool((err <= bound).all())
    # the 448 bound: nothing above the e4m3 range reaches the conversion (the restatement also asserts it tile by tile), every
    # block takes the exact path on its first tile, and a first tile far below the later maximum forces more of them
    blocks = N * H * ((Sq + 31) // 32)
    assert stats["p_max"] <= 448.0
    assert stats["exact"] >= blocks
    if far:
        assert stats["exact"] > blocks


def test_e4m3_helper_clamps_before_it_converts():
    x = torch.tensor([500.0, -1e9, 448.0, 464.0, 0.0, 2.0 ** -9, 2.0 ** -11])
    assert torch.isnan(x.to(R.F8).float()[0])                          # why the clamp is there
    assert R.e4m3(x).tolist() == [448.0, -448.0, 448.0, 448.0, 0.0, 2.0 ** -9, 0.0]


def test_vt_column_order_is_the_mfma_lane_layout():
    """Plain statement of the two layouts of v_mfma_scale_f32_32x32x64_f8f6f4 the kernel leans on (CDNA4 ISA, matrix layouts):
      * 32 x 32 fp32 accumulator: lane (col = lane % 32, h2 = lane / 32) register e holds row 8 (e / 4) + 4 h2 + e % 4;
      * 8-bit A (32 x 64) and B (64 x 32) operands: lane (row resp. col = lane % 32, h2 = lane / 32) byte j holds k = 32 h2 + j.
    S^T = K Q^T puts keys on accumulator rows, so lane (query, h2) holds the probabilities of 16 keys per 32-key sub-tile; packed
    in register order, byte 16 sub + e, they are the lane's B operand of O^T += V^T P^T -- i.e. contraction index k = 32 h2 + 16 sub
    + e of that MFMA is the key of accumulator row (e, h2) of sub-tile sub.  V^T's A operand must hold that key at column k."""
    for tile in range(3):
        seen = set()
        for lane in range(64):
            h2 = lane // 32
            for sub in range(2):
                for e in range(16):
                    key = 64 * tile + 32 * sub + 8 * (e // 4) + 4 * h2 + e % 4        # accumulator row -> key
                    byte = 16 * sub + e                                                # where the lane packs its probability
                    k_index = 32 * h2 + byte                                           # B operand: lane half h2, byte -> k
                    assert R.vt_position(key) == 64 * tile + k_index
                    seen.add(key)
        assert seen == set(range(64 * tile, 64 * tile + 64))
    # and pack_vt is that permutation with zero padding
    v8 = torch.arange(1, 71, dtype=torch.float32).view(1, 70, 1, 1).expand(1, 70, 1, 128).contiguous()
    vt = R.pack_vt(v8)
    assert vt.shape == (1, 128, 128)
    for s in range(70):
        assert vt[0, 5, R.vt_position(s)].item() == s + 1
    assert int((vt[0, 5] == 0).sum()) == 128 - 70


def test_header_and_exports_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in alg_amd._lib.EXPORTS, name
    assert declared == set(alg_amd._lib.EXPORTS)
    lib = alg_amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.alg_version() == 110
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "attention128_fp8.hip")).read()
    assert "v_mfma_scale_f32_32x32x64_f8f6f4" in src and "__builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4" in src


def test_run_py_flag_is_off_by_default_and_a_cogvideox_config_refuses_it():
    import argparse

    import run
    args = run.make_parser().parse_args([])
    assert args.fp8_attention is False
    assert run.make_parser().parse_args(["--fp8_attention"]).fp8_attention is True
    config = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}, "generation": {}}
    ns = argparse.Namespace(fp8=False, fp8_attention=True, synthetic=True, model_cache_dir=None)
    with pytest.raises(SystemExit, match="head_dim 128"):
        run.build_pipeline(config, ns, "cuda")


def test_k_scale_bound_covers_what_rmsnorm_and_rope_can_produce():
    """The K scale the models hand to the norm pass is a bound: 448 * scale >= any |k| the norm + RoPE can emit, also for an input
    with one dominant channel (where |x| rsqrt(mean x^2) reaches sqrt(n)) under the worst rotation (45 degrees)."""
    from alg_amd.transformer_wan import k_scale_bound
    g = torch.Generator().manual_seed(0)
    for n, heads in ((5120, 40), (128, 3)):
        w = (1.0 + 0.5 * torch.randn(n, generator=g)).bfloat16()
        sc = k_scale_bound(w, n, heads, rope=True)
        assert sc.shape == (heads,) and sc.dtype == torch.float32
        x = torch.zeros(4, n)
        x[0] = torch.randn(n, generator=g)
        x[1, 7] = 1000.0                                                   # one dominant channel
        x[2, 6], x[2, 7] = 3000.0, 3000.0                                  # a dominant pair: both at sqrt(n / 2), rotated onto one axis
        x[3] = 1e-4 * torch.randn(n, generator=g)
        x = x.bfloat16().float()
        y = ((x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)).bfloat16().float() * w.float()).bfloat16().float()
        a, b = y[:, 0::2], y[:, 1::2]
        worst = torch.sqrt(a * a + b * b)                                  # the largest component any rotation of the pair can reach
        per_head = worst.reshape(4, -1, 64).amax(dim=(0, 2)) if n > 128 else worst.amax().expand(heads)
        assert bool((per_head <= 448.0 * sc).all()), (per_head / (448.0 * sc)).max()
        assert float(per_head[0]) > 5.0 * float(per_head[1:].max() if heads > 1 and n > 128 else 1.0)    # the dominant rows do dominate
