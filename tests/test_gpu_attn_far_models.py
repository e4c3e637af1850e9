"""`transformer.attn_far_reuse` of the three DiTs (alg_amd/attn_far.py) on the small trained-like models, at frame counts where a
window of 1 is narrower than the video (helpers/attn_far_cases.py), and through the three ALG samplers.

  1. the switch at 0 is the window-only forward of a model that never heard of it, bit for bit, and allocates nothing;
  2. a refresh forward (near + far + merge: the exact softmax over all keys from two bf16-rounded partials) against the DENSE forward
     (window 0) of the same inputs: relative L2 no larger than that run's own distance between the dense bf16 forward and the fp32
     oracle -- the floor-anchored rule of tests/_parity.py with the run's own floor, no factor;
  3. the same inputs twice with one advance between: the second forward records `reused`, launches no far pass, and gives the
     first one's bits;
  4. forced refresh, invalidation by another shape, by a dense step, reset at the start of a video;
  5. the samplers, 8 steps, the range opened: the final-latent relative L2 against the dense run for window only, far reuse N = 2
     and N = 4, attn_reuse N = 2 -- reported; on CogVideoX at window 1 far reuse N = 2 must beat window only (the feature's premise)."""
import pytest
import torch

from _parity import rel
from alg_amd import _lib
from alg_amd.attn_window import call_transformer
from helpers.attn_far_cases import FarFamily
from helpers.attn_reuse_cases import ROLES, keys_at
from helpers.sampler_cases import SAMPLERS, STEPS

pytestmark = pytest.mark.gpu
T_A = 600                      # inside the default range (100, 800)
NAMES = ("cog", "wan", "hy")
FAMILIES = {}


def family(name):
    if name not in FAMILIES:
        FAMILIES[name] = FarFamily(name)
    return FAMILIES[name]


def counted(fam, model, inp, keys, monkeypatch, force=False):
    """(output, {wrapper name: calls}) of one forward"""
    counts = {}

    def spy(name, real):
        def call(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return real(*a, **kw)
        return call

    with monkeypatch.context() as mp:
        for nm in [n for n in dir(_lib) if n.startswith("flash_attn_") and callable(getattr(_lib, n))] + ["attn_merge_lse"]:
            mp.setattr(_lib, nm, spy(nm, getattr(_lib, nm)))
        out = fam.run(model, inp, keys, force)
    return out, counts


@pytest.mark.parametrize("name", NAMES)
def test_switch_off_refresh_against_dense_and_reuse_of_the_same_inputs(name, monkeypatch):
    fam = family(name)
    n, L, roles = 2, fam.layers, ROLES[1:]
    hd = 64 if name == "cog" else 128
    entry = "flash_attn_d%d_ranges_heads" % hd
    inp = fam.inputs(n, 11, T_A)
    keys = lambda: keys_at(roles, T_A)

    # ---- 1. the switch at 0: a model that never heard of it
    fresh = fam.build()
    fresh.attn_window = 1
    window_only = fam.run(fresh, inp)
    model = fam.build()
    dense = fam.run(model, inp)
    model.attn_window = 1
    assert model.attn_far_reuse == 0
    assert torch.equal(fam.run(model, inp, keys()), window_only) and not torch.equal(window_only, dense)
    assert model._attn_far_obj is None and model.attn_far_reuse_bytes == 0 and fresh._attn_far_obj is None

    # ---- 2. a refresh forward against the dense forward, held to the run's own bf16 floor
    model.attn_far_reuse = 2
    model.reset_attn_far_reuse()
    refresh, c_refresh = counted(fam, model, inp, keys(), monkeypatch)
    floor = rel(dense, fam.oracle(inp))
    e_refresh, e_window = rel(refresh, dense), rel(window_only, dense)
    print("%s: refresh forward vs dense forward %.3e; window only vs dense %.3e; dense bf16 forward vs fp32 oracle (the floor) %.3e"
          % (name, e_refresh, e_window, floor))
    assert bool(torch.isfinite(refresh.float()).all())
    assert e_refresh <= floor, (e_refresh, floor)
    near_launches = L * (n if name == "hy" else 1)
    assert c_refresh[entry] == near_launches + L * n and c_refresh["attn_merge_lse"] == L * n      # per-sample far launches
    rows, D, heads = model._attn_far_obj._shape[1:]
    assert D == heads * hd and model.attn_far_reuse_bytes == L * n * (rows * D * 2 + heads * rows * 4)

    # ---- 3. one advance, the same inputs: reused, no far pass, the first forward's bits
    model.attn_far_reuse_advance()
    again, c_reuse = counted(fam, model, inp, keys(), monkeypatch)
    assert [r["reused"] for r in model.attn_far_reuse_stats] == [False, True]
    assert model.attn_far_reuse_stats[1] == {"keys": roles, "t": float(T_A), "reused": True, "forced": False}
    assert c_reuse[entry] == near_launches and c_reuse["attn_merge_lse"] == L * n
    assert {k: v for k, v in c_reuse.items() if k not in (entry, "attn_merge_lse")} == \
           {k: v for k, v in c_refresh.items() if k not in (entry, "attn_merge_lse")}           # every other attention launch stays
    assert torch.equal(again, refresh)
    # other inputs one step on: the near field is fresh, so the forward is neither the refresh of the old inputs nor window-only
    model.attn_far_reuse_advance()
    model.attn_far_reuse = 3
    moved_inp = fam.inputs(n, 12, T_A - 50)
    moved = fam.run(model, moved_inp, keys_at(roles, T_A - 50))
    assert model.attn_far_reuse_stats[-1]["reused"] is True
    fresh_moved = fam.run(fresh, moved_inp)
    assert not torch.equal(moved, fresh_moved) and not torch.equal(moved, refresh) and bool(torch.isfinite(moved.float()).all())
    model.attn_far_reuse = 2


@pytest.mark.parametrize("name", NAMES)
def test_forced_refresh_other_shape_dense_step_range_and_reset(name):
    fam = family(name)
    model = fam.build()
    model.attn_window, model.attn_far_reuse = 1, 2
    n, roles = 2, ROLES[1:]
    inp = fam.inputs(n, 21, T_A)
    keys = lambda t=T_A: keys_at(roles, t)
    reused = lambda: [r["reused"] for r in model.attn_far_reuse_stats]

    def step(inp_=inp, t=T_A, force=False):
        model.attn_far_reuse_advance()
        return fam.run(model, inp_, keys(t), force)

    model.reset_attn_far_reuse()
    first = step()
    step()
    assert reused() == [False, True]
    forced = step(force=True)                                # the last step of a schedule: a refresh whatever the age says
    assert reused()[-1] is False and model.attn_far_reuse_stats[-1]["forced"] is True and torch.equal(forced, first)
    step()
    assert reused()[-1] is True
    outside = step(t=900)                                    # outside (t_lo, t_hi): a refresh step, i.e. exact attention
    assert reused()[-1] is False and torch.equal(outside, fam.run(model, inp, keys(900), True))
    step()
    assert reused()[-1] is True
    # another shape drops everything cached
    other = fam.inputs(n, 22, T_A, frames=fam.frames + 2)
    step(other)
    assert reused()[-1] is False
    step(inp)
    assert reused()[-1] is False
    step(inp)
    assert reused()[-1] is True
    # a dense step (the samplers' attn_window_dense_steps) launches the dense entry and leaves the entries invalid
    model.attn_far_reuse = 4
    records = len(model.attn_far_reuse_stats)
    model.attn_far_reuse_advance()
    dense_out = call_transformer(model, True, forward=lambda: fam.run(model, inp, keys()))
    assert len(model.attn_far_reuse_stats) == records and model.attn_window == 1
    plain = fam.build()
    assert torch.equal(dense_out, fam.run(plain, inp))
    step()
    assert reused()[-1] is False
    step()
    assert reused()[-1] is True
    # a window that covers the video: the dense launch, nothing cached
    model.attn_window = fam.frames
    assert torch.equal(step(), dense_out) and len(model.attn_far_reuse_stats) == records + 2
    model.attn_window = 1
    # the start of a video
    model.reset_attn_far_reuse()
    assert model.attn_far_reuse_stats == []
    assert torch.equal(step(), first) and reused() == [False]
    assert model.attn_far_reuse_bytes > 0                    # the buffers are kept


def test_refusals_reach_the_forward_and_the_sampler():
    fam = family("wan")
    model = fam.build()
    inp = fam.inputs(2, 31, T_A)
    model.attn_far_reuse = 2
    with pytest.raises(ValueError, match="attn_far_reuse=2 with attn_window=0"):
        fam.run(model, inp, keys_at(ROLES[1:], T_A))
    model.attn_window, model.attn_reuse = 1, 2
    with pytest.raises(ValueError, match="attn_far_reuse=2 with attn_reuse=2"):
        fam.run(model, inp, keys_at(ROLES[1:], T_A))
    model.attn_reuse = 0
    cog = family("cog").build()
    cog.attn_window, cog.attn_far_reuse, cog.attn_prescale = 1, 2, False
    with pytest.raises(ValueError, match="attn_prescale"):
        family("cog").run(cog, family("cog").inputs(2, 32, T_A), keys_at(ROLES[1:], T_A))
    torch.cuda.synchronize()


ARMS = (("window only", dict(attn_window=1)), ("far reuse N = 2", dict(attn_window=1, attn_far_reuse=2)),
        ("far reuse N = 4", dict(attn_window=1, attn_far_reuse=4)), ("attn_reuse N = 2", dict(attn_reuse=2)))
OPEN = dict(attn_far_reuse_t_lo=-1, attn_far_reuse_t_hi=10 ** 6, attn_reuse_t_lo=-1, attn_reuse_t_hi=10 ** 6)
F, T = False, True


@pytest.mark.parametrize("name", NAMES)
def test_samplers_four_arms_against_the_dense_run(name):
    """Final-latent relative L2 against the dense run, 8 steps, trained-like weights: printed; the figures are in the README."""
    frames = dict(cog=11, wan=5, hy=7)[name]
    model, run = SAMPLERS[name](frames=frames)
    dense, passes, ts = run()
    assert len(ts) == STEPS
    for k, v in OPEN.items():
        setattr(model, k, v)
    err = {}
    for arm, switches in ARMS:
        for k, v in switches.items():
            setattr(model, k, v)
        out, passes2, _ = run()
        assert passes2 == passes and bool(torch.isfinite(out.float()).all())
        err[arm] = rel(out, dense)
        if "attn_far_reuse" in switches:
            N = switches["attn_far_reuse"]
            st = model.attn_far_reuse_stats
            want = [not (i == 0 or i == STEPS - 1 or i % N == 0) for i in range(STEPS)]
            assert [r["reused"] for r in st] == want, (arm, [r["reused"] for r in st])
            assert [r["forced"] for r in st] == [T] + [F] * (STEPS - 2) + [T] and [r["t"] for r in st] == ts
            assert torch.equal(run()[0], out)                 # no stale cache: the same video again, from an empty cache
        for k in switches:
            setattr(model, k, 0)
    print(name, "final latents vs the dense run:", ", ".join("%s %.3e" % kv for kv in err.items()))
    assert torch.equal(run()[0], dense)                       # every switch back at 0: the dense sampler
    if name == "cog":      # the feature's premise, no margin: at window 1 the cached far field beats dropping it
        assert err["far reuse N = 2"] < err["window only"], err
