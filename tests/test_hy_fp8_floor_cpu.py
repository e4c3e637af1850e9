"""The e4m3-eager floor helper of the HunyuanVideo DiT (tests/_hy_fp8_floor.py) on the CPU: it routes exactly the linears that
HunyuanVideoTransformer3DModel(..., fp8=True) quantises -- six per dual-stream block (latent stream), five per single-stream block
(joint rows) -- through oracle/fp8_oracle.linear, nothing else, and always puts torch.nn.functional.linear back."""
import pytest
import torch
import torch.nn.functional as F

from _hy_fp8_floor import DUAL_LINEARS, SINGLE_LINEARS, fp8_weight_names, hy_fp8_linears, routed_per_forward
from _parity import rel
from oracle import fp8_oracle, hy_oracle

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
MODES = {"token_replace": dict(image_condition_type="token_replace", guidance_embeds=False),
         "plain_guidance": dict(image_condition_type="latent_concat", guidance_embeds=True)}


def _case(mode, num_layers=1, num_single_layers=1):
    """tests/test_gpu_hunyuan_forward.py's small() (heads 4, D = 512) and its inputs: batch 2, prompt lengths 13 and 20"""
    kw = dict(num_attention_heads=4, num_layers=num_layers, num_single_layers=num_single_layers, num_refiner_layers=1,
              text_embed_dim=64, pooled_projection_dim=64, **MODES[mode])
    ocfg = hy_oracle.HyConfig(**kw)
    sd = hy_oracle.init_weights(ocfg, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 3, 16, 16, generator=g).to(BF)
    txt = torch.randn(2, 20, 64, generator=g).to(BF)
    mask = torch.zeros(2, 20)
    mask[0, :13] = 1
    mask[1] = 1
    pooled = torch.randn(2, 64, generator=g).to(BF)
    guid = torch.tensor([6000.0, 6000.0]) if ocfg.guidance_embeds else None
    return ocfg, sd, (x, torch.tensor([996.0, 996.0]), txt, mask, pooled, guid)


def _forward(ocfg, sd, inputs, dtype=BF):
    x, t, txt, mask, pooled, guid = inputs
    return hy_oracle.hy_forward(ocfg, sd, x.to(dtype), t, txt.to(dtype), mask, pooled.to(dtype), guid, dtype=dtype)


def test_helper_names_the_latent_and_joint_linears_and_no_prompt_or_refiner_linear():
    ocfg, sd, _ = _case("token_replace", num_layers=2, num_single_layers=3)
    names = fp8_weight_names(sd)
    want = ["transformer_blocks.%d.%s.weight" % (i, n) for i in range(2) for n in DUAL_LINEARS]
    want += ["single_transformer_blocks.%d.%s.weight" % (i, n) for i in range(3) for n in SINGLE_LINEARS]
    assert sorted(names) == sorted(want) and len(names) == routed_per_forward(ocfg) == 6 * 2 + 5 * 3
    for k in names:
        assert "context_embedder" not in k and "add_" not in k and "ff_context" not in k and "norm" not in k
    assert "proj_out.weight" not in names and "context_embedder.token_refiner.refiner_blocks.0.attn.to_q.weight" not in names


@pytest.mark.parametrize("mode", sorted(MODES))
def test_helper_routes_six_per_dual_and_five_per_single_block_and_nothing_else(mode):
    ocfg, sd, inputs = _case(mode, num_layers=2, num_single_layers=2)
    original = F.linear
    with hy_fp8_linears(sd, BF) as stats:
        assert F.linear is not original
        e4m3 = _forward(ocfg, sd, inputs)
    assert F.linear is original
    assert stats["weights"] == stats["routed"] == 6 * ocfg.num_layers + 5 * ocfg.num_single_layers == 22
    # every prompt-stream, refiner, AdaLN and embedder call went to torch untouched: count all calls with nothing to route
    with hy_fp8_linears({}, BF) as none:
        bf16 = _forward(ocfg, sd, inputs)
    assert none["routed"] == 0 and none["other"] == stats["routed"] + stats["other"]
    # per forward: patch embed 1, condition embedders 4 (+ 2 guidance), token-replace timestep-0 embedding 2, refiner 5 + 7 per
    # block, dual blocks 2 (+ 1 token replace) AdaLN + 6 prompt-stream, single blocks 1 (+ 1) AdaLN, output head 2
    tr = ocfg.image_condition_type == "token_replace"
    other = (1 + 4 + (2 if ocfg.guidance_embeds else 0) + (2 if tr else 0) + 5 + 7 * ocfg.num_refiner_layers
             + ocfg.num_layers * (2 + tr + 6) + ocfg.num_single_layers * (1 + tr) + 2)
    assert stats["other"] == other, (stats, other)
    # ... and an empty routing is the plain bf16-eager forward
    assert torch.equal(bf16, _forward(ocfg, sd, inputs))
    ref = _forward(ocfg, {k: v.float() for k, v in sd.items()}, inputs, dtype=torch.float32)
    assert e4m3.dtype == BF and not torch.equal(e4m3, bf16)
    e_fp8, e_bf16, d = rel(e4m3, ref), rel(bf16, ref), rel(e4m3, bf16)
    print("%s: e4m3-eager vs fp32 %.3e, bf16-eager vs fp32 %.3e, e4m3-eager vs bf16-eager %.3e" % (mode, e_fp8, e_bf16, d))
    assert e_bf16 < e_fp8 < 0.5 and d > 0


def test_helper_needs_the_state_dict_in_the_run_dtype():
    ocfg, sd, inputs = _case("token_replace")
    with pytest.raises(AssertionError, match="already be in"):
        with hy_fp8_linears(sd, torch.float32):
            pass
    assert F.linear is torch.nn.functional.linear
    # a float32 copy run in float32 is routed as well (the pointers are those of the copy)
    sd32 = {k: v.float() for k, v in sd.items()}
    with hy_fp8_linears(sd32, torch.float32) as stats:
        _forward(ocfg, sd32, inputs, dtype=torch.float32)
    assert stats["routed"] == 11


def test_helper_restores_linear_when_the_body_raises():
    ocfg, sd, _ = _case("token_replace")
    original = F.linear
    with pytest.raises(RuntimeError, match="boom"):
        with hy_fp8_linears(sd, BF):
            assert F.linear is not original
            raise RuntimeError("boom")
    assert F.linear is original
    # an error inside a routed call (shape mismatch in fp8_oracle.linear) leaves the wrapper installed until the context ends
    w = sd["single_transformer_blocks.0.proj_out.weight"]
    with pytest.raises(RuntimeError):
        with hy_fp8_linears(sd, BF):
            F.linear(torch.zeros(2, w.shape[1] + 1, dtype=BF), w)
    assert F.linear is original


@pytest.mark.parametrize("mode", sorted(MODES))
def test_single_block_proj_out_is_quantised_on_the_concatenated_row_with_one_scale_per_token(mode, monkeypatch):
    """The routed proj_out call of a single block sees [attention | gelu(mlp)] (D + M wide) on the joint rows, and its result is
    the hand-written scheme on that row: ONE amax / 448 per token over all D + M values, one per output channel of the weight,
    fp32 accumulation, one rounding to bf16.  Two scales per token (one per half) give other values."""
    ocfg, sd, inputs = _case(mode)
    D, M = ocfg.dim, int(ocfg.dim * ocfg.mlp_ratio)
    w, b = sd["single_transformer_blocks.0.proj_out.weight"], sd["single_transformer_blocks.0.proj_out.bias"]
    seen = []
    inner = fp8_oracle.linear

    def recording(x, weight, bias, out_dtype=None, **kw):
        y = inner(x, weight, bias, out_dtype=out_dtype, **kw)
        if weight.data_ptr() == w.data_ptr():
            seen.append((x.clone(), y.clone()))
        return y

    monkeypatch.setattr(fp8_oracle, "linear", recording)
    with hy_fp8_linears(sd, BF) as stats:
        _forward(ocfg, sd, inputs)
    assert stats["routed"] == 11 and len(seen) == 1
    x, y = seen[0]
    S, L = 3 * 8 * 8, 20
    assert x.shape == (2, S + L, D + M) and x.dtype == BF and y.shape == (2, S + L, D) and y.dtype == BF

    def quantise(t):                                  # rows of t -> (e4m3 values as float32, one float32 scale per row)
        amax = t.float().abs().amax(dim=-1, keepdim=True)
        scale = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0), torch.ones_like(amax))
        return (t.float() * (1.0 / scale)).clamp(-448.0, 448.0).to(F8).float(), scale

    (qx, sx), (qw, sw) = quantise(x.reshape(-1, D + M)), quantise(w)
    want = F.linear(qx * sx, qw * sw, b.float()).to(BF).reshape(2, S + L, D)
    assert torch.equal(y, want)
    assert sx.shape == (2 * (S + L), 1)
    # the attention half and the MLP half have different ranges: a scale per half is another quantisation
    (qa, sa), (qm, sm) = quantise(x.reshape(-1, D + M)[:, :D]), quantise(x.reshape(-1, D + M)[:, D:])
    assert not torch.equal(sa, sm)
    halves = F.linear(torch.cat([qa * sa, qm * sm], dim=1), qw * sw, b.float()).to(BF).reshape(2, S + L, D)
    assert not torch.equal(halves, want)
