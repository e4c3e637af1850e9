"""The three ALG samplers through alg_amd/sampler_ext.py, on the small trained-like models, 4 steps.

The videos have 11 / 5 / 7 latent frames (274 / 480 / 468 tokens): the fewest of these samplers at which a window of 1 is narrower
than the video.  With fewer, every query block of 256 rows reaches every frame through its neighbours and the sink frame,
frame_window_ranges returns None, and the calibration step would have nothing to calibrate.

A spy around the model's forward records what every step's forward was handed (cache_keys, cache_force) and the model's
`attn_window` / `_attn_calibrate` at that moment; the columns are asserted against literals.  The pass counts follow from the
schedules of helpers/sampler_cases.py at 4 steps (t = i / 3): CogVideoX "linear" to 0.5 -> strengths 1, 1/3, 0, 0 -> 3 3 2 2 passes;
Wan "interval" [0, 0.3] and HunyuanVideo [0, 0.25] -> 3 2 2 2.

The latents are then compared bit for bit with a run that drives the same model BY HAND: the pipeline is handed a wrapper without
any switch attribute (so the module under test arms nothing and adds nothing), and the wrapper does, per forward, what the loops
did before they shared a driver -- the resets at its construction, attn_reuse_advance, explicit StepKeys, the force rule, and
attn_window.call_transformer with the dense and calibrate flags."""
import pytest
import torch

from alg_amd import attn_window
from alg_amd.attn_reuse import StepKeys
from helpers.sampler_cases import SAMPLERS

pytestmark = pytest.mark.gpu
STEPS = 4
F, T = False, True
K3, K2 = ["uncond_init", "uncond", "cond"], ["uncond", "cond"]
PASSES = {"cog": [3, 3, 2, 2], "wan": [3, 2, 2, 2], "hy": [3, 2, 2, 2]}
KEYS = {"cog": [K3, K3, K2, K2], "wan": [K3, K2, K2, K2], "hy": [K3, K2, K2, K2]}
FORWARD = {"cog": "forward_assembled", "wan": "__call__", "hy": "__call__"}
FRAMES = {"cog": 11, "wan": 5, "hy": 7}
LAYERS = 2


def spy_on(monkeypatch, model, name, log):
    real = getattr(type(model), name)

    def spy(self, *args, **kw):
        keys = kw.get("cache_keys")
        log.append(dict(keys=None if keys is None else list(keys), t=getattr(keys, "timestep", None), kw=sorted(k for k in kw if k.startswith("cache_")),
                        force=kw.get("cache_force"), window=self.attn_window, calibrate=self._attn_calibrate))
        return real(self, *args, **kw)

    monkeypatch.setattr(type(model), name, spy)


class ByHand:
    """What the pipeline is handed for the by-hand run: dtype and config, and a forward that wires the extensions itself."""

    def __init__(self, model, name, host_timestep, timesteps, keys=None, dense_steps=0, recall=False):
        self.model, self.fn, self.i = model, getattr(model, name), 0
        self.host_timestep, self.timesteps, self.keys, self.dense_steps, self.recall = host_timestep, timesteps, keys, dense_steps, recall
        if keys is not None:
            model.reset_attn_reuse()
        if recall:
            model.reset_attn_window_heads()

    dtype = property(lambda self: self.model.dtype)
    config = property(lambda self: self.model.config)

    def forward_assembled(self, *args, **kw):
        i, m = self.i, self.model
        self.i += 1
        cache_kw = {}
        if self.keys is not None:
            m.attn_reuse_advance()
            cache_kw = dict(cache_keys=StepKeys(self.keys[i], self.host_timestep(self.timesteps[i])),
                            cache_force=i == len(self.timesteps) - 1 or not m.attn_reuse_stats)
        return attn_window.call_transformer(m, i < self.dense_steps, *args, forward=self.fn,
                                            calibrate=self.recall and i == max(self.dense_steps, 1) - 1, **cache_kw, **kw)

    __call__ = forward_assembled


@pytest.mark.parametrize("name", ["cog", "wan", "hy"])
def test_reuse_and_window_runs_see_the_columns_and_equal_the_by_hand_run(name, monkeypatch):
    model, run = SAMPLERS[name](frames=FRAMES[name], steps=STEPS)
    host_timestep = int if name == "cog" else float
    log = []
    spy_on(monkeypatch, model, FORWARD[name], log)
    plain, passes, ts = run()
    assert passes == PASSES[name] and len(ts) == STEPS and all(a > b for a, b in zip(ts, ts[1:]))
    assert [(r["kw"], r["window"], r["calibrate"]) for r in log] == [([], 0, F)] * STEPS     # everything off: no cache keyword

    # ---- attention reuse, N = 2, a range that holds the timesteps of steps 1 and 2 only
    lo, hi = int((ts[2] + ts[3]) / 2), int((ts[0] + ts[1]) / 2)
    assert ts[3] < lo < ts[2] and ts[1] < hi < ts[0]
    model.attn_reuse, model.attn_reuse_t_lo, model.attn_reuse_t_hi = 2, lo, hi
    del log[:]
    out, _, _ = run()
    print(name, "timesteps", ts, "range", (lo, hi), "reused", [r["reused"] for r in model.attn_reuse_stats])
    assert [r["keys"] for r in log] == KEYS[name]                              # "uncond" and "cond" carry over the 3 -> 2 hand-over
    assert [r["t"] for r in log] == [float(host_timestep(t)) for t in ts]
    assert [r["force"] for r in log] == [T, F, F, T]                           # no record yet; the last step
    assert [(r["window"], r["calibrate"]) for r in log] == [(0, F)] * STEPS
    # step 0 forced; step 1 finds every key one step old and reuses; step 2 finds them two steps old; step 3 is forced
    assert [r["reused"] for r in model.attn_reuse_stats] == [F, T, F, F]
    assert not torch.equal(out, plain)
    by_hand = ByHand(model, FORWARD[name], host_timestep, ts, keys=KEYS[name])
    want, _, _ = run(transformer=by_hand)
    assert by_hand.i == STEPS and torch.equal(out, want)
    model.attn_reuse = 0

    # ---- per-head windows by recall, two dense steps: step 0 runs with the window off, step 1 is the calibration forward (the
    # model keeps attn_window and runs it dense in output), steps 2 and 3 run windowed
    model.attn_window, model.attn_window_recall = 1, 0.9
    del log[:]
    out, _, _ = run(attn_window_dense_steps=2)
    assert [r["window"] for r in log] == [0, 1, 1, 1] and [r["calibrate"] for r in log] == [F, T, F, F]
    assert [r["kw"] for r in log] == [[]] * STEPS
    assert model.attn_window == 1 and model._attn_calibrate is False           # restored
    assert torch.isfinite(out.float()).all()
    assert model.attn_window_calibrated and len(model.attn_window_stats) == LAYERS        # one calibration, one record per layer
    stats = [dict(r) for r in model.attn_window_stats]
    want, _, _ = run(transformer=ByHand(model, FORWARD[name], host_timestep, ts, dense_steps=2, recall=True))
    assert torch.equal(out, want) and [r["windowed"] for r in model.attn_window_stats] == [r["windowed"] for r in stats]
    assert model.attn_window == 1 and model._attn_calibrate is False
