"""The three ALG samplers driving `transformer.attn_reuse` (alg_amd/attn_reuse.py): 8 steps on the small trained-like models.

The expected `reused` column is DERIVED from the rule: with N = 2 and a range that holds the timesteps of steps 2 .. 5 only,
step 0 is forced and step 1 is outside the range (both computed; step 1 rewrites the entries: age 0), step 2 finds them one step
old and reuses, step 3 finds them two steps old (> N - 1) and computes, step 4 reuses again -- also across the 3 -> 2 pass
hand-over, "uncond" and "cond" carry over --, step 5 computes (age 2), steps 6 and 7 are outside the range (7 is forced too):
F F T F T F F F.  The tests recompute that column from the records' own (keys, t, forced) with a fresh AttnReuse and assert both."""
import pytest
import torch

from alg_amd.attn_reuse import AttnReuse
from helpers.sampler_cases import SAMPLERS, STEPS, cog_sampler, wan_sampler

pytestmark = pytest.mark.gpu
F, T = False, True
WANT = [F, F, T, F, T, F, F, F]
K3, K2 = ["uncond_init", "uncond", "cond"], ["uncond", "cond"]


def by_the_rule(records, every, lo, hi):
    """The `reused` column the records should carry, recomputed from their own keys, t and forced flag (one forward per step)."""
    rule, out = AttnReuse(every, lo, hi), []
    for r in records:
        rule.advance()
        hit = rule.decide(r["keys"], r["t"], r["forced"])
        if not hit:
            rule.mark_written(r["keys"])
        out.append(hit)
    return out


@pytest.mark.parametrize("name", ["cog", "wan", "hy"])
def test_sampler_pattern_range_off_no_stale_cache_and_drift(name):
    model, run = SAMPLERS[name]()
    plain, passes, ts = run()
    assert len(ts) == STEPS and passes[0] == 3 and passes[-1] == 2          # the ALG loop: 3 passes early, 2 later
    assert model._attn_reuse_obj is None and model.attn_reuse_bytes == 0     # switch off: nothing allocated, nothing recorded
    assert all(a > b for a, b in zip(ts, ts[1:]))
    lo, hi = int((ts[5] + ts[6]) / 2), int((ts[1] + ts[2]) / 2)             # holds the timesteps of steps 2 .. 5 only
    assert ts[6] < lo < ts[5] and ts[2] < hi < ts[1]

    # ---- pattern
    model.attn_reuse, model.attn_reuse_t_lo, model.attn_reuse_t_hi = 2, lo, hi
    out, passes2, _ = run()
    st = [dict(r) for r in model.attn_reuse_stats]
    print(name, "timesteps", ts, "range", (lo, hi), "reused", [r["reused"] for r in st])
    assert passes2 == passes and [r["keys"] for r in st] == [K3 if n == 3 else K2 for n in passes]
    assert [r["t"] for r in st] == ts
    assert [r["forced"] for r in st] == [T] + [F] * (STEPS - 2) + [T]       # the first forward of a video, the last step
    assert [r["reused"] for r in st] == by_the_rule(st, 2, lo, hi) == WANT
    assert torch.isfinite(out.float()).all() and not torch.equal(out, plain)
    keys = 3
    rows, D = model._attn_reuse_obj._shape[1:]
    assert model.attn_reuse_bytes == model._attn_reuse_obj._shape[0] * keys * rows * D * 2

    # ---- no stale cache: the same video again, from an empty cache
    again, _, _ = run()
    assert torch.equal(again, out)
    assert model.attn_reuse_stats[0]["reused"] is False and [r["reused"] for r in model.attn_reuse_stats] == WANT

    # ---- the drift diagnostic: every computed forward behind the first measures; the latents do not move
    model.attn_reuse_drift = True
    measured, _, _ = run()
    assert torch.equal(measured, out)
    st = model.attn_reuse_stats
    assert [r["reused"] for r in st] == WANT and "drift" not in st[0]
    layers = model._attn_reuse_obj._shape[0]
    for r in st[1:]:
        if r["reused"]:
            assert "drift" not in r
            continue
        d = torch.tensor(r["drift"], dtype=torch.float64)
        assert d.shape == (len(r["keys"]), layers) and torch.isfinite(d).all() and (d > 0).all(), r
    print(name, "drift per computed step (max over keys and layers):", ["%.3f" % max(max(k) for k in r["drift"]) for r in st if "drift" in r])
    model.attn_reuse_drift = False

    # ---- a range that holds no timestep: the switch-off sampler, bit for bit
    model.attn_reuse_t_lo, model.attn_reuse_t_hi = 2000, 3000
    off, _, _ = run()
    assert torch.equal(off, plain) and not any(r["reused"] for r in model.attn_reuse_stats)
    # N = 3: two reused steps behind every computed one
    model.attn_reuse, model.attn_reuse_t_lo, model.attn_reuse_t_hi = 3, lo, hi
    run()
    st = model.attn_reuse_stats
    assert [r["reused"] for r in st] == by_the_rule(st, 3, lo, hi) == [F, F, T, T, F, T, F, F]
    model.attn_reuse = 0
    assert torch.equal(run()[0], plain)


def test_wan_window_calibration_step_is_never_reused():
    model, run = wan_sampler(frames=5)                  # (with three latent frames a window of 1 covers the video: nothing to calibrate)
    _, _, ts = run()
    model.attn_reuse, model.attn_reuse_t_lo, model.attn_reuse_t_hi = 2, int((ts[5] + ts[6]) / 2), int((ts[1] + ts[2]) / 2)
    model.attn_window, model.attn_window_recall = 1, 0.5
    out, _, _ = run(attn_window_dense_steps=3)          # the calibration forward is step 2 -- a step the schedule would reuse
    st = model.attn_reuse_stats
    assert st[2]["forced"] is True and st[2]["reused"] is False
    assert [r["reused"] for r in st] == by_the_rule(st, 2, model.attn_reuse_t_lo, model.attn_reuse_t_hi) == [F, F, F, T, F, T, F, F]
    assert model.attn_window_calibrated and len(model.attn_window_stats) == 2
    assert torch.isfinite(out.float()).all()


def test_cfg_split_and_step_cache_are_refused():
    model, run = cog_sampler()
    model.attn_reuse = 2
    with pytest.raises(ValueError, match="cfg_split"):
        run(cfg_split=object())
    model.step_cache = 0.1
    with pytest.raises(ValueError, match="step_cache"):
        run()
