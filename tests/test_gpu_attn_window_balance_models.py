"""`transformer.attn_window_balance` of the three DiTs (attn_window.HeadWindowHost), through the samplers on the trained-like test
models of test_gpu_attn_window_heads_models.py (Wan, HunyuanVideo) and test_gpu_attn_window_heads_cogvideox.py (CogVideoX): with a
recall threshold that leaves at least one layer with dense AND windowed heads, the final latents with the flag on (True = "units",
"lanes") are the flag-off run's bit for bit, the _order entry is launched for exactly the launches of the mixed layers and never
with the flag off, reset_attn_window_heads() drops the orders, and the flag without a recall threshold is refused."""
import pytest
import torch

import test_gpu_attn_window_heads_cogvideox as HC
import test_gpu_attn_window_heads_models as HM
import test_gpu_attn_window_models as M
from alg_amd import _lib
from alg_amd.attn_window import KvRangesHeads, LaunchOrder, balanced_order, unit_costs
from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
from alg_amd.schedulers import FlowMatchEulerDiscreteScheduler
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
from alg_amd.transformer_wan import WanTransformer3DModel

pytestmark = pytest.mark.gpu
DEV, BF = M.DEV, M.BF


@pytest.fixture(autouse=True)
def _q64_for_every_call(monkeypatch):
    """ALG_ATTN128_Q64=2: the dense launches of these small shapes run the kernel the ranged entries run."""
    monkeypatch.setenv("ALG_ATTN128_Q64", "2")


def _wan():
    cfg, sd, _ = M._wan_setup(layers=2)
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    pipe, kw = HM._sampler(model)
    return model, pipe, kw, "flash_attn_d128", 17


def _hunyuan():
    cfg, sd, _ = M._hy_setup()
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    g = torch.Generator().manual_seed(8)
    lat, img = torch.randn(1, 16, M.HY_F, 16, 26, generator=g), torch.randn(1, 16, 1, 16, 26, generator=g)
    mk = lambda v: (torch.randn(1, M.HY_L, 64, generator=g).to(BF), torch.randn(1, 64, generator=g).to(BF),
                    torch.cat([torch.ones(1, v), torch.zeros(1, M.HY_L - v)], dim=1).to(BF))
    pos, neg = mk(M.HY_VALID[1]), mk(M.HY_VALID[0])
    d = lambda t_: t_.to(DEV)
    pipe = HunyuanVideoImageToVideoPipeline(transformer=model, scheduler=FlowMatchEulerDiscreteScheduler(shift=7.0)).to(DEV)
    # true CFG without the low-pass branch: two passes per step, one launch per sample and layer
    kw = dict(prompt_embeds=d(pos[0]), pooled_prompt_embeds=d(pos[1]), prompt_attention_mask=d(pos[2]),
              negative_prompt_embeds=d(neg[0]), negative_pooled_prompt_embeds=d(neg[1]), negative_prompt_attention_mask=d(neg[2]),
              negative_prompt=None, image_latents=d(img), latents=d(lat), height=128, width=208, num_frames=4 * (M.HY_F - 1) + 1,
              num_inference_steps=4, true_cfg_scale=6.0, guidance_scale=1.0, output_type="latent", use_low_pass_guidance=False,
              attn_window_dense_steps=2)
    return model, pipe, kw, "flash_attn_d128", 17


def _cogvideox():
    model, cfg, _ = HC.C._model()
    pipe, kw = HC._sampler(model, cfg)
    return model, pipe, kw, "flash_attn_d64", 13


def _spy(monkeypatch, name, table_arg):
    """Logs (table, order or None, lse given) of every call of _lib.<name> and lets it through."""
    real, calls = getattr(_lib, name), []

    def spied(*a, **kw):
        calls.append((a[table_arg], a[table_arg + 1] if name.endswith("_order") else None, kw.get("lse") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(_lib, name, spied)
    return calls


def _mixing_threshold(stats):
    """A threshold between two heads' recalls (minimum over the samples) of one layer: that layer gets dense AND windowed heads."""
    for s in stats:
        r = sorted(set(min(row[h] for row in s["recall"]) for h in range(len(s["recall"][0]))))
        gaps = [(b - a, 0.5 * (a + b)) for a, b in zip(r, r[1:])]
        if gaps:
            return max(gaps)[1]
    return None


@pytest.mark.parametrize("family", [_wan, _hunyuan, _cogvideox], ids=lambda f: f.__name__[1:])
def test_balanced_launch_order_keeps_the_samplers_bits(family, monkeypatch):
    model, pipe, kw, entry, table_arg = family()
    final = lambda: pipe(**kw).frames.clone()

    # a first run, to see the recalls this model has on these inputs
    model.attn_window, model.attn_window_recall = 1, 0.5
    final()
    thr = _mixing_threshold(model.attn_window_stats)
    print(family.__name__, "recalls", [[round(min(r[h] for r in s["recall"]), 3) for h in range(len(s["recall"][0]))]
                                        for s in model.attn_window_stats], "threshold", thr)
    assert thr is not None                                   # the precondition: two heads of a layer differ in recall

    model.attn_window_recall = thr
    heads_calls, order_calls = _spy(monkeypatch, entry + "_ranges_heads", table_arg), _spy(monkeypatch, entry + "_ranges_order", table_arg)
    assert model.attn_window_balance is False
    want = final()
    mixed = [li for li, s in enumerate(model.attn_window_stats) if 0 < sum(s["windowed"]) < len(s["windowed"])]
    assert mixed, model.attn_window_stats                    # the precondition: at least one layer is mixed
    assert not order_calls and model._attn_orders == {}      # never with the flag off
    off_mixed = [t for t, _, lse in heads_calls if not lse]
    assert off_mixed and all(isinstance(t, KvRangesHeads) for t in off_mixed)
    calib = len(heads_calls) - len(off_mixed)

    for flag, policy in ((True, "units"), ("lanes", "lanes")):
        del heads_calls[:], order_calls[:]
        model.attn_window_balance = flag
        got = final()
        assert torch.equal(got, want), flag
        # the launches of the mixed layers, all of them and nothing else, went to the _order entry; the calibration is untouched
        assert [t.table.tolist() for t, _, _ in order_calls] == [t.table.tolist() for t in off_mixed], flag
        assert len(heads_calls) == calib and all(lse for _, _, lse in heads_calls), flag
        assert len(order_calls) % len(mixed) == 0
        for t, order, lse in order_calls:
            assert isinstance(order, LaunchOrder) and not lse
            n = order.batch
            assert torch.equal(order.order, balanced_order(unit_costs(t, n, t.heads), policy, heads=t.heads).order)
        assert model._attn_orders and all(k[2] == policy for k in model._attn_orders)
        # the batch sizes launched, and at most one more: the calibration forward's own, built at its end
        built, launched = {k[1] for k in model._attn_orders}, {o.batch for _, o, _ in order_calls}
        assert launched <= built and len(built - launched) <= 1, (built, launched)
        assert model.attn_window_order_build_seconds > 0.0
        model.reset_attn_window_heads()
        assert model._attn_orders == {} and model._attn_head_tables == {}

    # the flag without a recall threshold is refused
    model.attn_window_recall = 0.0
    with pytest.raises(ValueError, match="needs attn_window_recall > 0"):
        final()
    model.attn_window_balance = "pool"
    model.attn_window_recall = thr
    with pytest.raises(ValueError, match="attn_window_balance must be"):
        final()
