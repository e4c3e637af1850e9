"""The trained-like weight profile (tests/helpers/trained_like.py) reaches the regime it is for, and the anchored floor stays
meaningful in it -- conditions on the ORACLE alone, checked without a GPU on the shapes tests/test_gpu_trained_like.py runs.

A profile too mild to leave the kernels' fast paths makes the GPU tests worth nothing; one so harsh that the reference's own
execution mode (bf16-eager, e4m3-eager) falls apart makes the anchored bound vacuous.  So, on the medium shapes (>= 1,100 tokens):

  * attention, per sample: at least a tenth of the (head, query) rows have a first-KV-tile maximum of magnitude >= 64 log2 units
    (the d = 64 kernel keeps a non-zero offset) AND at least a tenth have it < 64 (offset snapped to zero), so that workgroups
    with waves in both modes exist; at least one row whose running sum of 2^(score - offset) leaves [0, 2^80) after the first
    tile (a bail-out of the pipelined statement).  CogVideoX (d = 64): block 0 and the last block.  Wan (d = 128): block 0; the
    d = 128 kernels never snap, the offset is the first tile's maximum, and all three of them (attention128.hip,
    attention128_pipe.hip, attention128_q64.hip) bail out at ALG_LAZY_SUM_LIMIT = 2^80 (common.h);
  * residual stream after block 0: the largest channel >= 30 x the RMS of the other channels on every token.  (Over ALL channels
    the ratio cannot exceed sqrt(D / massive channels) = 13 at these 512-wide models whatever the weights; it is recorded too.)
  * floor conditioning: rel(bf16-eager, fp32) and rel(e4m3-eager, fp32) under HALF of check_floor's sane = 0.5 cap; the output
    finite with a standard deviation in (0.05, 50).

`ALG_TRAINED_LIKE_REGIME=<path>` writes what was measured as JSON (profiles/trained_like_regime.json comes from there)."""
import json
import os

import pytest
import torch

from _fp8_floor import fp8_linears
from _parity import rel
from helpers import trained_like as TL
from helpers.trained_like_cases import BF, cog_case, hy_case, wan_case
from oracle import dit_oracle, hy_oracle, wan_oracle

SANE = 0.5                      # tests/_parity.check_floor's cap on the floor itself
REGIME = {}


def _live(out):
    assert bool(torch.isfinite(out).all())
    assert 0.05 < out.float().std().item() < 50.0
    return out.float().std().item()


def _cog(name, **profile):
    kw, ocfg, wbf, (hs, ehs, ts, rope) = cog_case(name, **profile)
    col = {}
    ref = dit_oracle.dit_forward(ocfg, {k: v.float() for k, v in wbf.items()}, hs.float(), ehs.float(), ts, rope, collect=col)
    bf16 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    with fp8_linears(wbf) as stats:
        e4m3 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    assert stats["routed"] == 6 * ocfg.num_layers
    last = ocfg.num_layers - 1
    attn = {"block_%d" % b: [TL.attention_regime(col["q_%d" % b][n], col["k_%d" % b][n], snaps=True) for n in range(hs.shape[0])]
            for b in sorted({0, last})}
    ratio, ratio_all = TL.massive_ratio(col["block_0"])
    return {"tokens": col["block_0"].shape[1], "attention": attn, "residual_max_over_rms_of_other_channels": ratio,
            "residual_max_over_rms_of_all_channels": ratio_all, "floor_bf16_eager": rel(bf16, ref), "floor_e4m3_eager": rel(e4m3, ref),
            "e4m3_eager_vs_bf16_eager": rel(e4m3, bf16), "output_std": _live(ref)}


def _wan(name, **profile):
    kw, ocfg, sd, (x, t, txt, img) = wan_case(name, **profile)
    col = {}
    ref = wan_oracle.wan_forward(ocfg, sd, x.float(), t, txt.float(), img.float(), collect=col)
    bf16 = wan_oracle.wan_forward(ocfg, sd, x, t, txt, img, dtype=BF)
    e4m3 = wan_oracle.wan_forward(ocfg, sd, x, t, txt, img, dtype=BF, fp8=True)
    attn = {"block_0": [TL.attention_regime(col["q_0"][n], col["k_0"][n], snaps=False) for n in range(x.shape[0])]}
    ratio, ratio_all = TL.massive_ratio(col["block0"])
    return {"tokens": col["block0"].shape[1], "attention": attn, "residual_max_over_rms_of_other_channels": ratio,
            "residual_max_over_rms_of_all_channels": ratio_all, "floor_bf16_eager": rel(bf16, ref), "floor_e4m3_eager": rel(e4m3, ref),
            "e4m3_eager_vs_bf16_eager": rel(e4m3, bf16), "output_std": _live(ref)}


def _check_floors(name, m):
    print(name, json.dumps(m))
    assert m["floor_bf16_eager"] < SANE / 2 and m["floor_e4m3_eager"] < SANE / 2, m
    assert m["floor_e4m3_eager"] > m["floor_bf16_eager"] > 0
    assert m["residual_max_over_rms_of_other_channels"] >= 30.0, m


def _check_attention(m):
    for block, samples in m["attention"].items():
        for n, r in enumerate(samples):
            assert r["kv_tiles"] >= 8                                            # the pipelined statement is entered at all
            assert r["kept_fraction"] >= 0.1 and r["snapped_fraction"] >= 0.1, (block, n, r)
            assert r["bail_out_rows"] >= 1, (block, n, r)


@pytest.mark.parametrize("model,name", [("cog", "small"), ("cog", "ragged"), ("cog", "medium"), ("wan", "small"), ("wan", "medium")])
def test_profile_reaches_the_regime_and_the_floors_stay_meaningful(model, name):
    m = (_cog if model == "cog" else _wan)(name)
    REGIME["%s_%s" % (model, name)] = m
    _check_floors(model + " " + name, m)
    if name == "medium":
        assert m["tokens"] >= 1100
        _check_attention(m)
    path = os.environ.get("ALG_TRAINED_LIKE_REGIME")
    if path:
        with open(path, "w") as f:
            json.dump({"profile": {k.lower(): getattr(TL, k) for k in dir(TL) if k.isupper() and isinstance(getattr(TL, k), (int, float))},
                       "cases": REGIME}, f, indent=1, sort_keys=True)
            f.write("\n")


def test_the_gaussian_regime_reaches_none_of_it():
    """The profile's reason to exist, and the mutation check of this file: with `level=0` (the weights every other forward test
    uses) no row keeps an offset or bails out and no channel stands out; with only the QK gain and the massive factor scaled
    back to 1 the regime assertions above fail."""
    m = _cog("medium", level=0)
    for samples in m["attention"].values():
        for r in samples:
            assert r["kept_fraction"] == 0 and r["bail_out_rows"] == 0 and r["score_max"] < 20
    assert m["residual_max_over_rms_of_other_channels"] < 8
    mild = _cog("medium", qk_gain=1.0, massive_factor=1.0)
    with pytest.raises(AssertionError):
        _check_attention(mild)
    with pytest.raises(AssertionError):
        _check_floors("mild", mild)
    mild = _wan("medium", qk_gain_rms=1.0, massive_factor=1.0)
    with pytest.raises(AssertionError):
        _check_attention(mild)
    with pytest.raises(AssertionError):
        _check_floors("mild", mild)


@pytest.mark.parametrize("mode", ["token_replace", "plain_guidance"])
def test_hunyuan_floor_stays_meaningful(mode):
    kw, ocfg, sd, (x, t, txt, mask, pooled, guid) = hy_case(mode)
    ref = hy_oracle.hy_forward(ocfg, {k: v.float() for k, v in sd.items()}, x.float(), t, txt.float(), mask, pooled.float(), guid)
    eager = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, guid, dtype=BF)
    _live(ref)
    assert 0 < rel(eager, ref) < SANE / 2


# ---- the helper itself ---------------------------------------------------------------------------------------------------------
def _dicts():
    from alg_amd import transformer_hunyuan_video, transformer_wan
    wcfg = transformer_wan.WanTransformerConfig(num_attention_heads=4, ffn_dim=1024, num_layers=2, text_dim=64, image_dim=64,
                                                added_kv_proj_dim=512)
    hcfg = transformer_hunyuan_video.HunyuanVideoTransformerConfig(num_attention_heads=4, num_layers=1, num_single_layers=1,
                                                                   num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
    wan_sd, hy_sd = wan_oracle.init_weights(wan_case("small")[1], seed=3), hy_oracle.init_weights(hy_case("token_replace")[1], seed=3)
    assert set(wan_sd) == set(transformer_wan.parameter_shapes(wcfg)) and set(hy_sd) == set(transformer_hunyuan_video.parameter_shapes(hcfg))
    return {"cog": dit_oracle.init_weights(dit_oracle.DiTConfig(**cog_case("small")[0]), seed=3, std=0.05, randomize_affine=True),
            "wan": wan_sd, "hy": hy_sd}


@pytest.fixture(scope="module")
def dicts():
    return _dicts()


@pytest.mark.parametrize("model", ["cog", "wan", "hy"])
def test_keys_shapes_dtypes_determinism_and_level_zero(dicts, model):
    sd = dicts[model]
    before = {k: v.clone() for k, v in sd.items()}
    out = TL.trained_like(sd, seed=5)
    assert list(out) == list(sd)
    for k, v in sd.items():
        assert out[k].shape == v.shape and out[k].dtype == v.dtype and bool(torch.isfinite(out[k].float()).all()), k
        assert torch.equal(v, before[k]), k                                     # the input is not modified
    again = TL.trained_like(dict(reversed(list(sd.items()))), seed=5)           # independent of dict order
    assert all(torch.equal(out[k], again[k]) for k in sd)
    other = TL.trained_like(sd, seed=6)
    assert any(not torch.equal(out[k], other[k]) for k in sd)
    zero = TL.trained_like(sd, level=0)
    assert list(zero) == list(sd) and all(zero[k] is sd[k] for k in sd) and zero is not sd
    assert sum(not torch.equal(out[k], sd[k]) for k in sd) > len(sd) // 2       # the profile touches most tensors


CHANGES = {   # ingredient -> a pattern every changed name must contain one of
    "qk_gains": ("norm_q.weight", "norm_k.weight", "norm_added_q.weight", "norm_added_k.weight"),
    "qk_biases": ("norm_q.bias", "norm_k.bias", "to_q.bias", "to_k.bias"),
    "norm_gains": ("norm.weight", "norm_final.weight", "norm1.weight", "norm2.weight"),
    "biases": (".bias",),
    "massive": ("patch_embed.proj.bias", "patch_embed.text_proj.bias", "patch_embedding.bias", "text_embedder.linear_2.bias",
                "x_embedder.proj.bias", "context_embedder.proj_in.bias"),
    "spread": (".weight",),
}


@pytest.mark.parametrize("model", ["cog", "wan", "hy"])
@pytest.mark.parametrize("ingredient", TL.INGREDIENTS)
def test_each_ingredient_alone_changes_only_the_tensors_it_names(dicts, model, ingredient):
    sd = dicts[model]
    off = {i: False for i in TL.INGREDIENTS}
    assert all(torch.equal(v, sd[k]) for k, v in TL.trained_like(sd, **off).items())
    out = TL.trained_like(sd, **dict(off, **{ingredient: True}))
    changed = [k for k in sd if not torch.equal(out[k], sd[k])]
    assert changed, ingredient
    assert all(any(p in k for p in CHANGES[ingredient]) for k in changed), changed
    full = TL.trained_like(sd)
    if ingredient == "biases":
        assert not any(".norm_q." in k or ".norm_k." in k or any(p in k for p in CHANGES["massive"]) for k in changed), changed
    if ingredient == "spread":
        assert all(sd[k].dim() >= 2 and k.split(".")[0] in ("transformer_blocks", "single_transformer_blocks", "blocks", "context_embedder")
                   for k in changed), changed
    if ingredient == "massive":
        idx, sign = TL.massive_channels(sd, 0)
        for k in changed:
            d = (out[k].float() - sd[k].float()).abs()
            assert int((d > 0).sum()) == len(idx) == TL.MASSIVE_CHANNELS
            assert torch.equal(torch.sign(out[k].float()[idx]), sign)
    # ingredients do not interact: what one writes alone is what the full profile holds for those tensors
    assert all(torch.equal(out[k], full[k]) for k in changed)
