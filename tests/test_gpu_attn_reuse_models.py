"""`transformer.attn_reuse` of the three DiTs (alg_amd/attn_reuse.py) on the small trained-like models, bf16 and e4m3 linears.

Every identity here is exact (torch.equal):
  1. a computed (store) forward with the switch on is the switch-off forward, and the switch at 0 allocates nothing;
  2. a reusing forward launches nothing whose only consumer is the self-attention;
  3. store at (X, t), reuse at the same (X, t): the store forward's output;
  4. the splice: reuse at (X', t') equals a switch-off forward at (X', t') whose self-attention launches are replaced -- through
     the seam attn_window.launch_self_attention, by code that knows nothing of the cache -- by the outputs recorded at (X, t);
  5. key routing: entries stored by three samples keyed uncond_init / uncond / cond feed two samples keyed uncond / cond."""
import pytest
import torch

from alg_amd import _lib
from helpers.attn_reuse_cases import ROLES, Family, Seam, keys_at

pytestmark = pytest.mark.gpu
T_A, T_B = 600, 500          # both inside the default range (100, 800)

FAMILIES = {}


def family(name):
    if name not in FAMILIES:
        FAMILIES[name] = Family(name)
    return FAMILIES[name]


CASES = [(f, fp8) for f in ("cog", "wan", "hy") for fp8 in (False, True)]
ids = ["%s-%s" % (f, "e4m3" if fp8 else "bf16") for f, fp8 in CASES]


def store_then_reuse(fam, model, a, b, roles_a, roles_b):
    """store at `a`, one sampler step later reuse at `b` -> (store output, reuse output)"""
    model.reset_attn_reuse()
    out_a = fam.run(model, a, keys_at(roles_a, a["t"]))
    model.attn_reuse_advance()
    out_b = fam.run(model, b, keys_at(roles_b, b["t"]))
    assert [r["reused"] for r in model.attn_reuse_stats] == [False, True]
    return out_a, out_b


@pytest.mark.parametrize("name,fp8", CASES, ids=ids)
def test_computed_is_todays_reuse_is_idempotent_and_the_splice(name, fp8):
    fam = family(name)
    model = fam.build(fp8)
    n = 2
    a, b = fam.inputs(n, 11, T_A), fam.inputs(n, 12, T_B)
    roles = ROLES[1:]

    # ---- switch off: today's forward, with or without keys; nothing allocated
    with Seam(fam, n, "record") as rec:
        plain_a = fam.run(model, a)
    assert rec.calls == fam.layers * (n if name == "hy" else 1) and len(rec.recorded) == fam.layers * n
    assert torch.equal(fam.run(model, a, keys_at(roles, T_A)), plain_a)
    assert model._attn_reuse_obj is None and model.attn_reuse_bytes == 0          # no state, no buffer, no record
    with Seam(fam, n, "replay", rec.recorded):
        spliced_b = fam.run(model, b)                  # E: everything of (X', t') but the attention outputs, which are A's
    plain_b = fam.run(model, b)
    assert not torch.equal(spliced_b, plain_b)

    # ---- 1. and 3.: the store forward is the switch-off forward; reusing at the same inputs gives it again
    model.attn_reuse = 2
    out_a, again = store_then_reuse(fam, model, a, a, roles, roles)
    assert torch.equal(out_a, plain_a)
    assert torch.equal(again, plain_a)
    rows, D = model._attn_reuse_obj._shape[1:]
    assert model.attn_reuse_bytes == fam.layers * n * rows * D * 2

    # ---- 4. the splice
    out_a, out_b = store_then_reuse(fam, model, a, b, roles, roles)
    assert torch.equal(out_a, plain_a)
    assert torch.equal(out_b, spliced_b)

    # ---- outside the range, forced, or too old: computed, and today's
    model.reset_attn_reuse()
    fam.run(model, a, keys_at(roles, T_A))
    for inp, t, force, adv in ((b, 900, False, 1), (b, T_B, True, 1), (b, T_B, False, 2)):
        for _ in range(adv):
            model.attn_reuse_advance()
        assert torch.equal(fam.run(model, inp, keys_at(roles, t), force), plain_b)
        assert model.attn_reuse_stats[-1]["reused"] is False
    model.attn_reuse = 0
    assert torch.equal(fam.run(model, b, keys_at(roles, T_B)), plain_b)


@pytest.mark.parametrize("name,fp8", CASES, ids=ids)
def test_key_routing_three_stored_samples_feed_two(name, fp8):
    fam = family(name)
    model = fam.build(fp8)
    a, b = fam.inputs(3, 21, T_A), fam.inputs(2, 22, T_B)
    with Seam(fam, 3, "record") as rec:
        plain_a = fam.run(model, a)
    with Seam(fam, 2, "replay", rec.recorded, rows=[1, 2]):
        want = fam.run(model, b)                       # the splice fed with A's rows 1 and 2
    with Seam(fam, 2, "replay", rec.recorded, rows=[0, 1]):
        wrong = fam.run(model, b)
    assert not torch.equal(want, wrong)                # the three samples' attention outputs do differ
    model.attn_reuse = 2
    out_a, out_b = store_then_reuse(fam, model, a, b, ROLES, ROLES[1:])
    assert torch.equal(out_a, plain_a)
    assert torch.equal(out_b, want)
    assert sorted(model._attn_reuse_obj.entries) == sorted(ROLES)


SPIED = ("gemm", "gemm_pair", "gemm_pair_qk", "qk_norm_rope_", "rmsnorm_rope_", "rmsnorm_rope_fp8", "headnorm_rope_", "headnorm_rope_fp8",
         "quantize_fp8_vt", "layernorm_modulate", "layernorm_modulate_seg", "layernorm_mod_f32")


def launches(fam, model, inp, keys, monkeypatch):
    """(profile key -> count, _lib wrapper -> count) of one forward"""
    counts = {}

    def counted(name, real):
        def call(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return real(*a, **kw)
        return call

    with monkeypatch.context() as mp:
        for nm in [n for n in dir(_lib) if n.startswith("flash_attn_") and callable(getattr(_lib, n))] + list(SPIED):
            mp.setattr(_lib, nm, counted(nm, getattr(_lib, nm)))
        model.profile = {}
        fam.run(model, inp, keys)
        torch.cuda.synchronize()
        timed = {k: len(v) for k, v in model.profile.items()}
        model.profile = None
    return timed, counts


ATTENTION_ONLY = ("gemm_qkv", "gemm_qk", "gemm_vt", "qk_norm_rope", "headnorm_rope", "attn", "attn_self", "vt_quant", "attn_calib")


@pytest.mark.parametrize("name,fp8", CASES, ids=ids)
def test_a_reusing_forward_launches_nothing_the_attention_alone_consumes(name, fp8, monkeypatch):
    fam = family(name)
    model = fam.build(fp8)
    model.attn_reuse = 2
    inp, L, n = fam.inputs(2, 31, T_A), fam.layers, 2
    roles = ROLES[1:]
    timed_c, lib_c = launches(fam, model, inp, keys_at(roles, T_A), monkeypatch)
    model.attn_reuse_advance()
    timed_r, lib_r = launches(fam, model, inp, keys_at(roles, T_A), monkeypatch)
    assert [r["reused"] for r in model.attn_reuse_stats] == [False, True]
    flash = lambda c: {k: v for k, v in c.items() if k.startswith("flash_attn_")}
    print(name, fp8, "computed", timed_c, lib_c, "reused", timed_r, lib_r)
    for key in ATTENTION_ONLY:
        assert key not in timed_r, key
    assert timed_r["attn_reuse"] == L and timed_c["attn_reuse"] == L        # the loads, and the stores of the computed forward
    for key in ("gemm_ff1", "gemm_ff2") if name != "hy" else ("gemm_ff1",):
        assert timed_r[key] == timed_c[key] >= 1, key
    if name == "cog":
        assert timed_c["attn"] == L and timed_r["gemm_out"] == timed_c["gemm_out"] == L
        assert timed_c["ln_mod"] == 2 * timed_r["ln_mod"] >= 2 * L             # norm1 went, norm2 (the same launches) stayed
        assert flash(lib_r) == {} and sum(flash(lib_c).values()) >= L
        assert "qk_norm_rope_" not in lib_r and lib_c["qk_norm_rope_"] == L and "gemm_pair" not in lib_r
        assert lib_c["gemm"] + lib_c.get("gemm_pair", 0) - lib_r["gemm"] == (2 if fp8 else 1) * L      # Q|K and V^T, or their pair launch
    elif name == "wan":
        assert timed_c["attn_self"] == L and timed_r["gemm_out"] == timed_c["gemm_out"] == L
        assert timed_r["attn_cross"] == timed_c["attn_cross"] == L and timed_r["gemm_cout"] == L
        assert timed_c["ln_mod"] - timed_r["ln_mod"] == L
        assert timed_c["rms_rope"] - timed_r["rms_rope"] == 2 * L and timed_r["rms_rope"] == L       # the cross-attention's Q norm stays
        assert lib_c["rmsnorm_rope_"] - lib_r["rmsnorm_rope_"] == 2 * L
        assert flash(lib_r) == {"flash_attn_d128_dual": L}                   # the cross-attention alone
        assert lib_c["gemm"] + lib_c.get("gemm_pair", 0) - lib_r["gemm"] == (2 if fp8 else 1) * L
    else:
        assert timed_c["attn_self"] == L and timed_r["gemm_out"] == timed_c["gemm_out"] == 1 and timed_r["gemm_out_mlp"] == 1
        assert timed_c["ln_mod"] - timed_r["ln_mod"] == 1                    # the dual block's latent norm1; the single block's norm stays
        refiner = lib_r.get("flash_attn_d128", 0)
        assert flash(lib_r) == {"flash_attn_d128": refiner} and lib_c["flash_attn_d128"] == refiner + L * n   # the token refiner's stay
        assert lib_c["headnorm_rope_"] == 4 + 2 and "headnorm_rope_" not in lib_r
        assert lib_c["gemm"] - lib_r["gemm"] == 4 + 2                        # dual: Q|K and V of both streams; single: Q|K, V^T
        assert lib_c["layernorm_modulate_seg"] - lib_r["layernorm_modulate_seg"] == (1 if fp8 else 2)   # both streams' norm1 (fp8: the latent one is another entry)


def test_a_measuring_forward_under_graph_capture_raises():
    fam = family("wan")
    model = fam.build()
    model.attn_reuse, model.attn_reuse_drift = 2, True
    inp = fam.inputs(2, 41, T_A)
    fam.run(model, inp, keys_at(ROLES[1:], T_A))       # eager: allocates, stores
    model.attn_reuse_advance()
    model.attn_reuse_advance()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.AlgHipError, match="attn_reuse_drift"):
        with torch.cuda.graph(g):
            fam.run(model, inp, keys_at(ROLES[1:], T_A))
    torch.cuda.synchronize()
