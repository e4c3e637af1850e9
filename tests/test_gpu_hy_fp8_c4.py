"""BASELINE config 4 at its own size with e4m3 block linears: the set-up of
tests/test_gpu_full_size_c345.py::test_c4_forward_at_its_real_shape_vs_fp32_oracle (HunyuanVideo width 3072 = 24 heads x 128,
33 x 45 x 80 = 118,800 latent + 256 prompt tokens of which 48 are valid, 1 dual-stream + 1 single-stream block, token-replace
conditioning, the same seeds) with the model built fp8=True.  Here the widths are the real ones: K = 3072, 12288 and the single
block's 15,360-wide [attention | mlp] row go through the register forms of the batched quantiser."""
import pytest
import torch

from _hy_fp8_floor import hy_fp8_linears, routed_per_forward
from _parity import check_floor, rel
from alg_amd import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
from alg_amd.transformer_hunyuan_video import synthetic_state_dict
from oracle import hy_oracle

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"


@pytest.mark.timeout(1800)       # three oracle forwards over 119,056 tokens on the device; the bf16 test beside it runs two
def test_c4_fp8_forward_at_its_real_shape_vs_fp32_oracle():
    """HIP fp8 vs `oracle/hy_oracle.hy_forward` in fp32 on the e4m3-eager floor (the bf16 oracle inside hy_fp8_linears), all oracle
    runs on the device by torch's own ops; and rel(HIP fp8, HIP bf16) <= 1.5 x rel(e4m3-eager, bf16-eager), 1.5 being
    tests/_parity.py's global factor."""
    kw = dict(num_layers=1, num_single_layers=1)
    cfg, ocfg = HunyuanVideoTransformerConfig(**kw), hy_oracle.HyConfig(**kw)
    F, H, W, L = 33, 90, 160, 256
    sd = synthetic_state_dict(cfg, seed=24, device=DEV)
    assert set(sd) == set(hy_oracle.param_shapes(ocfg))
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(1, 16, F, H, W, generator=g, device=DEV).to(BF)
    txt = torch.randn(1, L, cfg.text_embed_dim, generator=g, device=DEV).to(BF)
    mask = torch.zeros(1, L, device=DEV)
    mask[:, :48] = 1
    pooled = torch.randn(1, cfg.pooled_projection_dim, generator=g, device=DEV).to(BF)
    t = torch.full((1,), 996.0, device=DEV)
    run = lambda m: m(hidden_states=x, timestep=t, encoder_hidden_states=txt, encoder_attention_mask=mask.to(BF),
                      pooled_projections=pooled, guidance=None, return_dict=False)[0]
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=True)
    out = run(model)
    assert out.shape == (1, 16, F, H, W) and torch.equal(run(model), out)
    del model
    out_bf16 = run(HunyuanVideoTransformer3DModel(cfg, sd, device=DEV))
    with torch.no_grad():
        bf16 = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, dtype=BF).cpu()
        with hy_fp8_linears(sd, BF) as stats:
            e4m3 = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, dtype=BF).cpu()
        assert stats["routed"] == routed_per_forward(ocfg) == 11
        ref = hy_oracle.hy_forward(ocfg, {k: v.float() for k, v in sd.items()}, x.float(), t, txt.float(), mask, pooled.float()).cpu()
    r, anchor = rel(out, out_bf16), rel(e4m3, bf16)
    print("C4 real shape: fp8 HIP vs bf16 HIP %.3e (e4m3-eager vs bf16-eager %.3e); e4m3-eager vs fp32 %.3e, bf16-eager vs fp32 %.3e, "
          "fp8 HIP vs fp32 %.3e" % (r, anchor, rel(e4m3, ref), rel(bf16, ref), rel(out, ref)))
    check_floor("hy_fp8_forward_c4_real_shape_1dual_1single_119056tokens", out, ref, e4m3)
    assert 0 < r <= 1.5 * anchor, (r, anchor)
