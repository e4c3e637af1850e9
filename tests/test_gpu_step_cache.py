"""The opt-in step cache (alg_amd/step_cache.py) on the GPU: alg_step_cache_probe against torch, the hit / miss bit identities
of the two transformers, the keys and the forced last step of the two samplers.

Every identity here is exact.  The only tolerance is on the probe's two sums: non-negative terms (no cancellation), summed
with at most 1,024 fp32 additions per chain and in double above that: 1,024 * 2^-24 ~ 6.1e-5 < 1e-4 relative against torch's
double sums (the kernel's fp32 chains are 8 long)."""
import pytest
import torch

from test_gpu_cog_fp8 import SMALL, _inputs as cog_inputs, _pair as cog_pair
from test_gpu_wan_forward import inputs as wan_inputs, small as wan_small
from alg_amd import (CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel,
                     CogVideoXTransformerConfig, _lib)
from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
from alg_amd.schedulers import UniPCMultistepScheduler
from alg_amd.transformer_wan import WanTransformer3DModel
from oracle import wan_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
KEYS = ["uncond", "cond"]
ALWAYS = 1e30                  # a threshold every finite change is under: the decisions no longer depend on the data


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded(t, fill):
    """A copy of `t` with 64 guard elements on either side: (whole buffer, the view the kernel gets)."""
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf[GUARD:GUARD + t.numel()].view(t.shape)


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _probe_case(rows, D, zero_prev, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(rows, D, generator=g).to(BF)
    x1 = (x0.float() + 0.3 * torch.randn(rows, D, generator=g)).to(BF)
    rp = torch.zeros(rows, D, dtype=BF) if zero_prev else (0.3 * torch.randn(rows, D, generator=g)).to(BF)
    if rows >= 3:
        x0[rows // 2] *= 40.0
        x1[rows // 2] *= 40.0               # one large row
        x1[rows - 2] = x0[rows - 2]         # one row block 0 left alone: r == 0 there
    return x0, x1, rp


def _run_probe(x0, x1, rp, tok0, tok_rows):
    rows, D = x0.shape
    nws = _lib.step_cache_workspace_bytes(rows, D)
    bufs = dict(keep=_guarded(x0, 7.0), x1=_guarded(x1, 7.0), r=_guarded(rp, 7.0),
                work=_guarded(torch.zeros(nws // 8, dtype=torch.float64), -3.0),
                sums=_guarded(torch.full((2,), -1.0, dtype=torch.float64), -3.0))
    _lib.step_cache_probe(bufs["keep"][1], bufs["x1"][1], bufs["r"][1], rows, D, tok0, tok_rows, bufs["work"][1], bufs["sums"][1])
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert _guards_intact(buf, -3.0 if name in ("work", "sums") else 7.0), name
    return bufs["keep"][1].cpu(), bufs["x1"][1].cpu(), bufs["r"][1].cpu(), bufs["sums"][1].cpu()


@pytest.mark.parametrize("zero_prev", [False, True])
@pytest.mark.parametrize("rows,D,tok0,tok_rows", [(229, 512, 10, 219), (1501, 3072, 226, 1275), (77, 5120, 0, 77), (1, 8, 0, 1)])
def test_probe_against_torch(rows, D, tok0, tok_rows, zero_prev):
    x0, x1, rp = _probe_case(rows, D, zero_prev, seed=rows + D)
    keep, x1_after, r, sums = _run_probe(x0, x1, rp, tok0, tok_rows)
    r_ref = (x1.float() - x0.float()).to(BF)
    assert torch.equal(r, r_ref)
    assert torch.equal(keep, x1) and torch.equal(x1_after, x1)            # keep now holds x1; x1 itself is only read
    if rows >= 3:
        assert not r_ref[rows - 2].any() and r_ref[rows // 2].float().abs().max() > 1.0
    tok = slice(tok0, tok0 + tok_rows)
    a_ref = (r_ref[tok].double() - rp[tok].double()).abs().sum().item()
    b_ref = rp[tok].double().abs().sum().item()
    a, b = sums.tolist()
    print("probe %dx%d rows [%d, %d): a %.9e (torch %.9e, rel %.2e)  b %.9e (torch %.9e)"
          % (rows, D, tok0, tok0 + tok_rows, a, a_ref, abs(a - a_ref) / a_ref, b, b_ref))
    assert a_ref > 0 and abs(a - a_ref) <= 1e-4 * a_ref
    if zero_prev:
        assert b == 0.0 and b_ref == 0.0
    else:
        assert b_ref > 0 and abs(b - b_ref) <= 1e-4 * b_ref
    if 0 < tok_rows < rows:   # the rows outside the window are not counted: the full-range sums are larger by far more than the bound
        assert a < (1 - 1e-3) * (r_ref.double() - rp.double()).abs().sum().item()
    again = _run_probe(x0, x1, rp, tok0, tok_rows)                        # deterministic: a second run gives the same bits
    assert torch.equal(again[2], r) and torch.equal(again[0], keep)
    assert torch.equal(again[3].view(torch.int64), sums.view(torch.int64))


def test_probe_with_no_rows_and_with_an_empty_window():
    x0, x1, rp = _probe_case(5, 64, False, seed=1)
    keep, _, r, sums = _run_probe(x0, x1, rp, 2, 0)                       # an empty window: the pass runs, the sums are zero
    assert torch.equal(r, (x1.float() - x0.float()).to(BF)) and torch.equal(keep, x1) and sums.tolist() == [0.0, 0.0]
    # rows == 0 is fine (an empty torch tensor has no pointer to hand over: straight through the C entry point)
    k, y, r0 = (torch.full((8,), 7.0, dtype=BF, device=DEV) for _ in range(3))
    work, s0 = torch.zeros(2, dtype=torch.float64, device=DEV), torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
    rc = _lib.load_library().alg_step_cache_probe(k.data_ptr(), y.data_ptr(), r0.data_ptr(), 0, 8, 0, 0, work.data_ptr(),
                                                  s0.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and s0.tolist() == [0.0, 0.0] and all((t == 7.0).all() for t in (k, y, r0))
    with pytest.raises(_lib.AlgHipError, match="alg_step_cache_probe"):
        _run_probe(x0, x1, rp, 3, 3)


# ---- 2. the two transformers ----------------------------------------------------------------------------------------------------
class Cog:
    name = "cog"

    @staticmethod
    def build(layers, fp8, more_layers=None):
        """`layers`-deep model; with more_layers also a deeper one FROM THE SAME STATE DICT (its block 0 is the same block)."""
        ocfg, wbf, deep = cog_pair(dict(num_layers=more_layers or layers), seed=3, fp8=fp8)
        Cog.ocfg = ocfg
        if more_layers is None:
            return deep
        return CogVideoXTransformer3DModel(CogVideoXTransformerConfig(**dict(SMALL, num_layers=layers)), wbf, device=DEV, fp8=fp8), deep

    @staticmethod
    def inputs(seed, t):
        hs, ehs, ts, rope = cog_inputs(Cog.ocfg, 2, 3, 8, 8, 12, 10, seed, t)
        return hs.to(DEV), ehs.to(DEV), ts.to(DEV).float(), tuple(r.to(DEV) for r in rope)

    @staticmethod
    def run(model, inp, **kw):
        hs, ehs, ts, rope = inp
        return model(hs, ehs, ts, image_rotary_emb=rope, return_dict=False, **kw)[0]

    @staticmethod
    def x(model):
        (ws,) = model._ws.values()
        return ws["x"]


class Wan:
    name = "wan"

    @staticmethod
    def build(layers, fp8, more_layers=None):
        cfg, ocfg = wan_small(layers=more_layers or layers)
        sd = wan_oracle.init_weights(ocfg, seed=3)
        deep = WanTransformer3DModel(cfg, sd, device=DEV, fp8=fp8)
        if more_layers is None:
            return deep
        return WanTransformer3DModel(wan_small(layers=layers)[0], sd, device=DEV, fp8=fp8), deep

    @staticmethod
    def inputs(seed, t):
        x, txt, img = wan_inputs(2, 3, 16, 24, seed)
        return x.to(DEV), torch.tensor([t, t], device=DEV), txt.to(DEV), img.to(DEV)

    @staticmethod
    def run(model, inp, **kw):
        x, t, txt, img = inp
        return model(hidden_states=x, timestep=t, encoder_hidden_states=txt, encoder_hidden_states_image=img, return_dict=False,
                     **kw)[0]

    @staticmethod
    def x(model):
        (ws,) = model._ws.values()
        return ws.x


def _spy_x0(model, seen):
    """Records the residual stream the cache is armed with: the hidden state in front of block 0."""
    sc = model._step_cache_state()
    begin = sc.begin

    def spy(x, *a):
        seen.append(x.clone())
        return begin(x, *a)

    sc.begin = spy
    return sc


def _bf_sub(a, b):
    return (a.float() - b.float()).to(BF)


@pytest.mark.parametrize("fam", [Cog, Wan], ids=lambda f: f.name)
def test_cache_off_with_keys_is_the_plain_forward(fam):
    model = fam.build(3, False)
    inp = fam.inputs(1, 999.0)
    plain = fam.run(model, inp)
    assert model.step_cache == 0.0 and model.step_cache_max_consecutive == 0
    before = torch.cuda.memory_allocated()
    out = fam.run(model, inp, cache_keys=KEYS, cache_force=False)
    assert torch.equal(out, plain)
    assert model.step_cache_stats == [] and model._step_cache_state().keep is None
    assert torch.cuda.memory_allocated() - before <= (out.numel() * 2 + 511) // 512 * 512     # nothing but the output was allocated
    model.step_cache = 0.1                                                # on, but no keys: plain too
    assert torch.equal(fam.run(model, inp), plain) and model.step_cache_stats == []


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("fam", [Cog, Wan], ids=lambda f: f.name)
def test_miss_then_hit_three_layers(fam, fp8):
    m1, m3 = fam.build(1, fp8, more_layers=3)
    inp_a, inp_b = fam.inputs(1, 999.0), fam.inputs(2, 700.0)
    off_a, x_final_a = fam.run(m3, inp_a), None
    x_final_a = fam.x(m3).clone()
    off_b = fam.run(m3, inp_b)
    fam.run(m1, inp_a)
    x1_a = fam.x(m1).clone()                                             # the 1-layer model's residual stream ends behind block 0
    fam.run(m1, inp_b)
    x1_b = fam.x(m1).clone()
    assert not torch.equal(x1_a, x_final_a) and not torch.equal(x1_a, x1_b)

    seen = []
    sc = _spy_x0(m3, seen)
    m3.step_cache = ALWAYS
    out = fam.run(m3, inp_a, cache_keys=KEYS)                            # nothing cached: computed, and the plain forward bit for bit
    assert torch.equal(out, off_a)
    assert [r["hit"] for r in m3.step_cache_stats] == [False] and m3.step_cache_stats[0]["keys"] == KEYS
    x0_a = seen[0]
    tails = {}
    for n, k in enumerate(KEYS):
        assert torch.equal(sc.tail[k], _bf_sub(x_final_a[n], x1_a[n])), k
        assert torch.equal(sc.r1[k], _bf_sub(x1_a[n], x0_a[n])), k
        assert sc.tail[k].any() and sc.r1[k].any()
        tails[k] = sc.tail[k].clone()
    assert torch.equal(sc.keep[:2], x1_a)

    out_b = fam.run(m3, inp_b, cache_keys=KEYS)                          # other latents, another timestep: a hit all the same
    assert [r["hit"] for r in m3.step_cache_stats] == [False, True]
    rel = m3.step_cache_stats[1]["rel"]
    assert len(rel) == 2 and all(0 < v < float("inf") for v in rel)
    x0_b = seen[1]
    for n, k in enumerate(KEYS):
        assert torch.equal(fam.x(m3)[n], (x1_b[n].float() + tails[k].float()).to(BF)), k
        assert torch.equal(sc.tail[k], tails[k]), k                       # refreshed on misses only
        assert torch.equal(sc.r1[k], _bf_sub(x1_b[n], x0_b[n])), k        # refreshed by every probe
    assert torch.isfinite(out_b.float()).all() and not torch.equal(out_b, off_b)

    out_f = fam.run(m3, inp_b, cache_keys=KEYS, cache_force=True)        # forced: computed, the plain forward again
    assert torch.equal(out_f, off_b)
    assert m3.step_cache_stats[2]["hit"] is False and m3.step_cache_stats[2]["forced"] is True
    m3.reset_step_cache()
    assert m3.step_cache_stats == []
    assert torch.equal(fam.run(m3, inp_a, cache_keys=KEYS), off_a) and m3.step_cache_stats[0]["hit"] is False
    with pytest.raises(ValueError, match="cache_keys"):
        fam.run(m3, inp_a, cache_keys=["cond", "cond"])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("fam", [Cog, Wan], ids=lambda f: f.name)
def test_one_layer_hits_are_exact_through_the_head(fam, fp8):
    """One block: the tail is exactly zero, so a hit adds 0 and the head sees the plain forward's hidden state."""
    model = fam.build(1, fp8)
    inps = [fam.inputs(1, 999.0), fam.inputs(2, 700.0), fam.inputs(1, 999.0)]
    plain = [fam.run(model, i) for i in inps]
    model.step_cache = ALWAYS
    for inp, want in zip(inps, plain):
        assert torch.equal(fam.run(model, inp, cache_keys=KEYS), want)
    assert [r["hit"] for r in model.step_cache_stats] == [False, True, True]
    sc = model._step_cache_state()
    assert all(not sc.tail[k].any() for k in KEYS) and all(sc.r1[k].any() for k in KEYS)


def test_an_active_forward_under_graph_capture_raises():
    model = Cog.build(3, False)
    inp = Cog.inputs(1, 999.0)
    model.step_cache = ALWAYS
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = Cog.run(model, inp)                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.AlgHipError, match="captured"):
        with torch.cuda.graph(graph, stream=side):
            Cog.run(model, inp, cache_keys=KEYS)
    torch.cuda.synchronize()
    assert model.step_cache_stats == [] and model._step_cache_state().keep is None
    assert torch.equal(Cog.run(model, inp), want)                         # the model is fine afterwards


# ---- 3. the two samplers --------------------------------------------------------------------------------------------------------
def _rule(records, tau, cap):
    """The decisions the records should carry, recomputed from their own `rel` and `forced` and the cap."""
    out, run = [], 0
    for r in records:
        hit = all(v < tau for v in r["rel"]) and not r["forced"] and not (cap and run >= cap)
        run = run + 1 if hit else 0
        out.append(hit)
    return out


def _cog_sampler():
    _, wbf, model = cog_pair(dict(num_layers=3), seed=6, fp8=False)
    g = torch.Generator().manual_seed(7)
    first = (torch.randn(1, 1, 8, 8, 12, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)

    def run(**kw):
        pipe = CogVideoXImageToVideoPipeline(transformer=model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
        trace = []
        out = pipe(image_latents=first, prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=96, num_frames=9,
                   num_inference_steps=8, output_type="latent", use_low_pass_guidance=True, lp_filter_in_latent=True,
                   lp_filter_type="gaussian_blur", lp_blur_sigma=3.0, lp_blur_kernel_size=3,
                   lp_strength_schedule_type="linear", generator=torch.Generator().manual_seed(0), step_trace=trace, **kw).frames
        assert [n for _, _, n in trace] == [3, 3, 3, 3, 2, 2, 2, 2]
        return out

    return model, run


def test_cog_sampler_keys_forced_last_step_cap_and_rule():
    model, run = _cog_sampler()
    plain = run()
    assert model.step_cache_stats == []
    assert torch.equal(run(), plain)
    M, H = False, True
    K3 = ["uncond_init", "uncond", "cond"]

    model.step_cache = ALWAYS
    out = run()
    st = model.step_cache_stats
    assert [r["hit"] for r in st] == [M, H, H, H, H, H, H, M]
    assert [r["forced"] for r in st] == [False] * 7 + [True]
    assert [r["keys"] for r in st] == [K3] * 4 + [KEYS] * 4
    assert st[4]["hit"] is True                                            # "uncond" and "cond" carried over from the 3-pass steps
    assert torch.isfinite(out.float()).all() and not torch.equal(out, plain)
    assert torch.equal(run(), out)                                         # a second call starts from an empty cache: same video
    assert [r["hit"] for r in model.step_cache_stats] == [M, H, H, H, H, H, H, M]

    model.step_cache_max_consecutive = 2
    out2 = run()
    assert [r["hit"] for r in model.step_cache_stats] == [M, H, H, M, H, H, M, M]
    assert torch.isfinite(out2.float()).all() and not torch.equal(out2, plain) and not torch.equal(out2, out)

    for tau, cap in ((0.1, 0), (0.1, 1), (0.7, 0), (0.7, 1)):   # 0.7: in the middle of this run's changes, so both outcomes occur
        model.step_cache, model.step_cache_max_consecutive = tau, cap
        out3 = run()
        st = model.step_cache_stats
        print("cog sampler tau %.2f cap %d: rel %s hits %s" % (tau, cap, [["%.3f" % v for v in r["rel"]] for r in st],
                                                              [r["hit"] for r in st]))
        assert len(st) == 8 and st[0]["hit"] is False and st[-1]["forced"] is True
        assert [r["hit"] for r in st] == _rule(st, tau, cap)
        assert torch.isfinite(out3.float()).all()

    with pytest.raises(_lib.AlgHipError, match="cfg_split"):
        run(cfg_split=object())
    model.step_cache, model.step_cache_max_consecutive = 0.0, 0
    assert torch.equal(run(), plain)                                       # off again: the plain sampler


def test_wan_sampler_keys_carry_over_the_pass_count_change():
    cfg, ocfg = wan_small(layers=3)
    model = WanTransformer3DModel(cfg, wan_oracle.init_weights(ocfg, seed=7), device=DEV)
    g = torch.Generator().manual_seed(8)
    lat, cond = torch.randn(1, 16, 3, 16, 24, generator=g), torch.randn(1, 20, 3, 16, 24, generator=g)
    pe, ne = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 512, 64, generator=g).to(BF)
    ie = torch.randn(1, 257, 64, generator=g).to(BF)

    def run(**kw):
        pipe = WanImageToVideoPipeline(transformer=model, scheduler=UniPCMultistepScheduler(flow_shift=3.0)).to(DEV)
        trace = []
        out = pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), image_embeds=ie.to(DEV),
                   image_condition=cond.to(DEV), latents=lat.to(DEV), height=128, width=192, num_frames=9,
                   num_inference_steps=6, guidance_scale=5.0, output_type="latent", use_low_pass_guidance=True,
                   lp_filter_in_latent=True, step_trace=trace, lp_filter_type="down_up", lp_resize_factor=0.4,
                   lp_strength_schedule_type="interval", schedule_interval_start_time=0.0, schedule_interval_end_time=0.3,
                   **kw).frames
        assert [n for _, n, _ in trace] == [3, 3, 2, 2, 2, 2]
        return out

    plain = run()
    assert model.step_cache_stats == []
    M, H = False, True
    model.step_cache = ALWAYS
    out = run()
    st = model.step_cache_stats
    assert [r["hit"] for r in st] == [M, H, H, H, H, M] and [r["forced"] for r in st] == [False] * 5 + [True]
    assert [r["keys"] for r in st] == [["uncond_init", "uncond", "cond"]] * 2 + [KEYS] * 4
    assert st[2]["hit"] is True                                            # the first 2-pass step found "uncond" and "cond"
    assert torch.isfinite(out.float()).all() and not torch.equal(out, plain)
    for tau in (0.1, 0.3):                                                 # 0.3: in the middle of this run's changes
        model.step_cache = tau
        run()
        st = model.step_cache_stats
        print("wan sampler tau %.1f: rel %s hits %s" % (tau, [["%.3f" % v for v in r["rel"]] for r in st], [r["hit"] for r in st]))
        assert len(st) == 6 and [r["hit"] for r in st] == _rule(st, tau, 0)
    with pytest.raises(_lib.AlgHipError, match="cfg_split"):
        run(cfg_split=object())
    model.step_cache = 0.0
    assert torch.equal(run(), plain)
