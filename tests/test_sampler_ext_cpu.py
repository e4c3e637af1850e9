"""alg_amd/sampler_ext.py -- the samplers' one driver of the transformers' opt-in extensions -- against a recording stand-in
transformer: what a video's construction refuses and resets, what every step's forward sees (attn_window, the calibration flag,
cache_keys / cache_force), from_pretrained's window switches, and lora.build.  Every expected value is a literal derived from the
rules ("Sampler extensions"), none is computed by the module under test.  No GPU."""
import os
from types import SimpleNamespace

import pytest

from alg_amd import _lib, lora, sampler_ext
from alg_amd.attn_reuse import StepKeys
from alg_amd.sampler_ext import SamplerExtensions, apply_switches, window_switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K3, K2 = ["uncond_init", "uncond", "cond"], ["uncond", "cond"]
F, T = False, True


class Dit:
    """The switch attributes, the resets, the reuse's advance and record, the calibration state; `events` is the order of
    everything the driver did to it, `calls` what each forward saw at call time."""

    def __init__(self, **switches):
        self.step_cache, self.attn_reuse, self.attn_reuse_t_lo, self.attn_reuse_t_hi = 0.0, 0, 100, 800
        self.attn_window, self.attn_window_recall = 0, 0.0
        self._attn_calibrate = self.attn_window_calibrated = False
        self.attn_reuse_stats, self.events, self.calls = [], [], []
        vars(self).update(switches)

    def reset_step_cache(self):
        self.events.append("reset_step_cache")

    def reset_attn_reuse(self):
        self.events.append("reset_attn_reuse")
        del self.attn_reuse_stats[:]

    def reset_attn_window_heads(self):
        self.events.append("reset_attn_window_heads")
        self.attn_window_calibrated = False

    def attn_reuse_advance(self):
        self.events.append("advance")

    def __call__(self, *args, **kw):
        self.events.append("forward")
        self.calls.append(dict(args=args, kw=kw, attn_window=self.attn_window, calibrate=self._attn_calibrate))
        if self.attn_reuse:                  # like the models: one record per active forward
            self.attn_reuse_stats.append({"keys": list(kw["cache_keys"])})
        if self._attn_calibrate:
            self.attn_window_calibrated = True
        return "prediction"


def run_video(dit, passes, batch=1, dense_steps=0, timesteps=None, **kw):
    ext = SamplerExtensions(dit, len(passes), dense_steps, **kw)
    del dit.events[:]                        # (what the construction did is asserted by the caller before / apart)
    for i, n_pass in enumerate(passes):
        t = 1000 - 100 * i if timesteps is None else timesteps[i]
        assert ext.step(i, t, n_pass, batch)("x", y=i) == "prediction"
        assert dit.calls[-1]["args"] == ("x",) and dit.calls[-1]["kw"]["y"] == i
        assert dit._attn_calibrate is False                                    # restored whatever the step was
    return ext


def column(dit, name):
    return [c[name] if name in c else c["kw"].get(name, "absent") for c in dit.calls]


# ---- window, recall, calibration -----------------------------------------------------------------------------------------------
def test_dense_steps_switch_the_window_off_and_restore_it():
    dit = Dit(attn_window=3)
    SamplerExtensions(dit, 6, 2)
    assert dit.events == []                                                    # no recall: nothing to reset
    run_video(dit, [3, 3, 3, 2, 2, 2], dense_steps=2)
    assert column(dit, "attn_window") == [0, 0, 3, 3, 3, 3] and dit.attn_window == 3
    assert column(dit, "calibrate") == [F] * 6
    assert column(dit, "cache_keys") == ["absent"] * 6 and column(dit, "cache_force") == ["absent"] * 6


def test_recall_resets_once_and_calibrates_on_the_last_dense_step():
    # the calibration forward keeps attn_window (call_transformer: the model itself runs it dense in output and measures), so
    # with a recall the forwards see 0, w (calibrating), w, w, w, w
    dit = Dit(attn_window=3, attn_window_recall=0.9)
    SamplerExtensions(dit, 6, 2)
    assert dit.events == ["reset_attn_window_heads"]
    run_video(dit, [3, 3, 3, 2, 2, 2], dense_steps=2)
    assert dit.events == ["forward"] * 6                                       # the reset came once, at construction
    assert column(dit, "calibrate") == [F, T, F, F, F, F]
    assert column(dit, "attn_window") == [0, 3, 3, 3, 3, 3] and dit.attn_window == 3
    again = Dit(attn_window=3, attn_window_recall=0.9)
    run_video(again, [3, 3, 2, 2], dense_steps=0)
    assert column(again, "calibrate") == [T, F, F, F] and column(again, "attn_window") == [3, 3, 3, 3]
    late = Dit(attn_window=3, attn_window_recall=0.9)
    run_video(late, [3, 3, 2, 2], dense_steps=1)
    assert column(late, "calibrate") == [T, F, F, F] and column(late, "attn_window") == [3, 3, 3, 3]
    off = Dit(attn_window=0, attn_window_recall=0.9)                           # a recall without a window drives nothing
    SamplerExtensions(off, 4, 2)
    run_video(off, [3, 3, 2, 2], dense_steps=2)
    assert off.events == ["forward"] * 4 and column(off, "calibrate") == [F] * 4


# ---- step cache ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,want3,want2", [
    (1, K3, K2),
    (2, [("uncond_init", 0), ("uncond_init", 1), ("uncond", 0), ("uncond", 1), ("cond", 0), ("cond", 1)],
     [("uncond", 0), ("uncond", 1), ("cond", 0), ("cond", 1)])])
def test_step_cache_keys_and_the_forced_last_step(batch, want3, want2):
    dit = Dit(step_cache=0.1)
    SamplerExtensions(dit, 4)
    assert dit.events == ["reset_step_cache"]

    def no_host_timestep(t):
        raise AssertionError("the timestep is taken to the host only while the reuse is on")

    run_video(dit, [3, 3, 2, 2], batch=batch, host_timestep=no_host_timestep)
    assert dit.events == ["forward"] * 4
    assert column(dit, "cache_keys") == [want3, want3, want2, want2]
    assert not any(isinstance(k, StepKeys) for k in column(dit, "cache_keys"))
    assert column(dit, "cache_force") == [F, F, F, T]


def test_step_cache_is_forced_on_the_calibration_step():
    dit = Dit(step_cache=0.1, attn_window=2, attn_window_recall=0.9)
    SamplerExtensions(dit, 4, 2)
    assert dit.events == ["reset_step_cache", "reset_attn_window_heads"]
    run_video(dit, [3, 3, 2, 2], dense_steps=2)
    assert column(dit, "calibrate") == [F, T, F, F]
    assert column(dit, "cache_force") == [F, T, F, T]                         # step 1 through call_transformer, step 3 the last
    assert column(dit, "cache_keys") == [K3, K3, K2, K2]


# ---- attention reuse ---------------------------------------------------------------------------------------------------------
def test_reuse_advances_once_per_step_and_names_the_host_timestep():
    dit = Dit(attn_reuse=2)
    SamplerExtensions(dit, 4)
    assert dit.events == ["reset_attn_reuse"]
    seen = []

    def host_timestep(t):
        seen.append(t)
        return int(t)

    run_video(dit, [3, 3, 2, 2], timesteps=[900.5, 700.5, 500.5, 300.5], host_timestep=host_timestep)
    assert dit.events == ["advance", "forward"] * 4
    assert seen == [900.5, 700.5, 500.5, 300.5]
    keys = column(dit, "cache_keys")
    assert keys == [K3, K3, K2, K2] and all(type(k) is StepKeys for k in keys)
    assert [k.timestep for k in keys] == [900.0, 700.0, 500.0, 300.0]
    assert column(dit, "cache_force") == [T, F, F, T]                         # no record yet; the last step
    default = Dit(attn_reuse=3)
    run_video(default, [2, 2], timesteps=[812.25, 40.75])                      # host_timestep=float
    assert [k.timestep for k in column(default, "cache_keys")] == [812.25, 40.75]
    assert column(default, "cache_force") == [T, T]


# ---- nothing on -------------------------------------------------------------------------------------------------------------------
def test_everything_off_and_bare_stand_ins_are_called_as_ever():
    def no_host_timestep(t):
        raise AssertionError("the timestep is taken to the host only while the reuse is on")

    dit = Dit()
    before = {k: v for k, v in vars(dit).items() if k not in ("events", "calls")}
    SamplerExtensions(dit, 4, 2)
    run_video(dit, [3, 3, 2, 2], dense_steps=2, host_timestep=no_host_timestep)
    assert dit.events == ["forward"] * 4
    assert [sorted(c["kw"]) for c in dit.calls] == [["y"]] * 4               # no cache_keys / cache_force keyword at all
    assert {k: v for k, v in vars(dit).items() if k not in ("events", "calls")} == before

    got = []
    fn = lambda hidden_states, timestep: got.append((hidden_states, timestep)) or "p"       # a signature without the keywords
    ext = SamplerExtensions(fn, 3, 1, host_timestep=no_host_timestep)
    assert [ext.step(i, 5, 2, 1)(hidden_states=i, timestep=5) for i in range(3)] == ["p"] * 3
    assert got == [(0, 5), (1, 5), (2, 5)] and vars(fn) == {}

    ns = SimpleNamespace()
    ext = SamplerExtensions(ns, 2, 1, cfg_split=object(), forward=fn, host_timestep=no_host_timestep)
    assert ext.step(0, 5, 3, 1)(7, 8) == "p" and got[-1] == (7, 8) and vars(ns) == {}


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_what_does_not_compose_is_refused_at_construction():
    with pytest.raises(_lib.AlgHipError, match="step_cache > 0 with cfg_split"):
        SamplerExtensions(Dit(step_cache=0.1), 4, cfg_split=object())
    dit = Dit(attn_window=2, attn_window_recall=0.9)
    with pytest.raises(_lib.AlgHipError, match="attn_window_recall > 0 with cfg_split"):
        SamplerExtensions(dit, 4, cfg_split=object())
    assert dit.events == []                                                    # refused before the reset
    with pytest.raises(ValueError, match="attn_reuse=2 with cfg_split"):
        SamplerExtensions(Dit(attn_reuse=2), 4, cfg_split=object())
    with pytest.raises(ValueError, match="attn_reuse=2 with step_cache=0.1"):
        SamplerExtensions(Dit(attn_reuse=2, step_cache=0.1), 4)
    with pytest.raises(ValueError, match="attn_reuse=1"):
        SamplerExtensions(Dit(attn_reuse=1), 4)
    SamplerExtensions(Dit(attn_window=2), 4, cfg_split=object())               # a plain window composes with the split


# ---- from_pretrained's window switches ---------------------------------------------------------------------------------------------
COG, WAN, HY = dict(widths_built=False, recall_needs_window=True), {}, {}


@pytest.mark.parametrize("flags", [COG, WAN, HY], ids=["cog", "wan", "hy"])
def test_window_switches_refusals(flags):
    cog = flags is COG
    for bad in (dict(attn_window_balance="rows"), dict(attn_window=2, attn_window_recall=0.9, attn_window_balance=2)):
        with pytest.raises(ValueError, match="attn_window_balance must be"):
            window_switches(**{**dict(attn_window=0, attn_window_recall=0.0, attn_window_balance=False, attn_window_widths=None), **bad},
                            **flags)
    with pytest.raises(ValueError, match="attn_window_balance=True needs attn_window_recall > 0"):
        window_switches(2, 0.0, True, None, **flags)
    first = "not built for head_dim 64" if cog else None                       # CogVideoX refuses any widths, before every other rule
    for args, message in [((4, 0.9, False, (4, 2)), "strictly ascending"), ((4, 0.9, False, "2,x"), "comma-separated"),
                          ((4, 0.9, False, (1, 2)), "must equal attn_window = 4"),
                          ((4, 0.0, False, (1, 4)), "needs attn_window_recall > 0: the width"),
                          ((4, 0.9, "rows", (1, 4)), "attn_window_balance must be")]:
        with pytest.raises(ValueError, match=first or message):
            window_switches(*args, **flags)
    for args, message in [((0, 0.0, False, None, 2), "attn_band=2 needs attn_window > 0 and attn_window_recall > 0"),
                          ((1, 0.0, False, None, 2), "attn_band=2 needs"), ((1, 0.9, False, None, -2), "non-negative int"),
                          ((1, 0.9, False, None, 2, True), "attn_band=2 does not compose with fp8_attention")]:
        with pytest.raises(ValueError, match=message):
            window_switches(*args, **flags)
    with pytest.raises(ValueError, match=first or "attn_band=2 does not combine with attn_window_widths"):
        window_switches(2, 0.9, False, (1, 2), 2, **flags)
    if cog:
        with pytest.raises(ValueError, match="attn_window_recall=0.9 needs attn_window > 0"):
            window_switches(0, 0.9, False, None, **flags)
        with pytest.raises(ValueError, match="attn_window_recall=0.9 needs attn_window > 0"):     # in front of the balance rules
            window_switches(0, 0.9, "rows", None, **flags)
    else:                                                                      # the other two families accept it, as ever
        assert window_switches(0, 0.9, False, None, **flags) == {"attn_window_recall": 0.9}


@pytest.mark.parametrize("flags", [COG, WAN, HY], ids=["cog", "wan", "hy"])
def test_window_switches_returns_and_apply_sets_exactly_what_was_given(flags):
    assert window_switches(0, 0.0, False, None, **flags) == {}
    apply_switches(object(), {})                                               # everything off: a stand-in is not touched
    got = window_switches("2", "0.9", "lanes", None, step_cache="0.05", **flags)
    assert got == {"step_cache": 0.05, "attn_window": 2, "attn_window_recall": 0.9, "attn_window_balance": "lanes"}
    assert [type(v) for v in got.values()] == [float, int, float, str]
    assert window_switches(2, 0.0, False, None, **flags) == {"attn_window": 2}
    assert window_switches(0, 0.0, False, None, step_cache=0.1, **flags) == {"step_cache": 0.1}
    assert window_switches(3, 0.9, True, None, 4, **flags) == {"attn_band": 4, "attn_window": 3, "attn_window_recall": 0.9,
                                                              "attn_window_balance": True}
    if flags is not COG:
        assert window_switches(4, 0.9, False, "1,2,4", **flags) == {"attn_window": 4, "attn_window_recall": 0.9,
                                                                    "attn_window_widths": (1, 2, 4)}
    m = SimpleNamespace(untouched=1)
    apply_switches(m, {"attn_window": 2, "attn_window_widths": (1, 2)})
    assert vars(m) == {"untouched": 1, "attn_window": 2, "attn_window_widths": (1, 2)}


# ---- lora.build ------------------------------------------------------------------------------------------------------------------
def test_lora_build_constructs_with_the_keywords_and_attaches_the_report():
    class Stub:
        lora_report = None

        def __init__(self, config, state_dict, device=None, **kw):
            self.seen = (config, state_dict, device, kw)

    sd = {}
    model = lora.build(Stub, "config", sd, None, "cpu", fp8=True, fp4=False)
    assert type(model) is Stub and model.seen == ("config", sd, "cpu", {"fp8": True, "fp4": False}) and model.seen[1] is sd
    assert model.lora_report == () and lora.build(Stub, "c", {}, [], "cpu").lora_report == ()


# ---- one copy --------------------------------------------------------------------------------------------------------------------
def test_the_loops_and_loaders_hold_no_copy_of_the_wiring():
    src = lambda *p: open(os.path.join(ROOT, *p)).read()
    for family in ("cogvideox", "wan", "hunyuan_video"):
        text = src("alg_amd", "pipeline_%s_image2video_lowpass.py" % family)
        for word in ("reset_step_cache", "reset_attn_window_heads", "attn_reuse_advance", "calibration_step", "pass_keys", "step_keys"):
            assert word not in text, (family, word)
        assert "sampler_ext.SamplerExtensions(" in text and "ext.step(" in text
        assert "merge_into(" not in src("alg_amd", "transformer_%s.py" % family)
    assert "merge_into(" not in src("run.py")
    assert sampler_ext.call_transformer.__module__ == "alg_amd.attn_window"   # composed, not replaced
