"""The three ALG samplers on the small trained-like DiTs of helpers/attn_reuse_cases.py (2 layers), three latent frames unless
`frames` says otherwise: one builder per family, each returning the model and a `run` that samples one seeded video to latents.
Shared by tests/test_gpu_attn_reuse_samplers.py and tests/test_gpu_sampler_ext.py.

    model, run = cog_sampler(frames, steps)
    latents, passes per step, timesteps = run(transformer=None, **pipeline_call_keywords)

`transformer`: what the pipeline is handed in place of the model (a wrapper around it)."""
import torch

from alg_amd import CogVideoXDDIMScheduler, CogVideoXImageToVideoPipeline
from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
from alg_amd.pipeline_wan_image2video_lowpass import WanImageToVideoPipeline
from alg_amd.schedulers import FlowMatchEulerDiscreteScheduler, UniPCMultistepScheduler
from helpers.attn_reuse_cases import BF, DEV, Family

STEPS = 8


def cog_sampler(frames=3, steps=STEPS):
    fam = Family("cog")
    model = fam.build()
    g = torch.Generator().manual_seed(7)
    first = (torch.randn(1, 1, 8, 8, 12, generator=g) * 0.7).to(BF)
    pe, ne = torch.randn(1, 10, 128, generator=g).to(BF), torch.randn(1, 10, 128, generator=g).to(BF)

    def run(transformer=None, **kw):
        pipe = CogVideoXImageToVideoPipeline(transformer=transformer or model, scheduler=CogVideoXDDIMScheduler()).to(DEV)
        trace = []
        out = pipe(image_latents=first, prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=96, num_frames=4 * (frames - 1) + 1,
                   num_inference_steps=steps, output_type="latent", use_low_pass_guidance=True, lp_filter_in_latent=True,
                   lp_filter_type="gaussian_blur", lp_blur_sigma=3.0, lp_blur_kernel_size=3,
                   lp_strength_schedule_type="linear", generator=torch.Generator().manual_seed(0), step_trace=trace, **kw).frames
        return out, [n for _, _, n in trace], [float(t) for t in pipe.scheduler.timesteps]

    return model, run


def wan_sampler(frames=3, steps=STEPS):
    fam = Family("wan")
    model = fam.build()
    g = torch.Generator().manual_seed(8)
    lat, cond = torch.randn(1, 16, frames, 16, 24, generator=g), torch.randn(1, 20, frames, 16, 24, generator=g)
    pe, ne = torch.randn(1, 512, 64, generator=g).to(BF), torch.randn(1, 512, 64, generator=g).to(BF)
    ie = torch.randn(1, 257, 64, generator=g).to(BF)

    def run(transformer=None, **kw):
        pipe = WanImageToVideoPipeline(transformer=transformer or model, scheduler=UniPCMultistepScheduler(flow_shift=3.0)).to(DEV)
        trace = []
        out = pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), image_embeds=ie.to(DEV),
                   image_condition=cond.to(DEV), latents=lat.to(DEV), height=128, width=192, num_frames=4 * (frames - 1) + 1,
                   num_inference_steps=steps, guidance_scale=5.0, output_type="latent", use_low_pass_guidance=True,
                   lp_filter_in_latent=True, step_trace=trace, lp_filter_type="down_up", lp_resize_factor=0.4,
                   lp_strength_schedule_type="interval", schedule_interval_start_time=0.0, schedule_interval_end_time=0.3,
                   **kw).frames
        return out, [n for _, n, _ in trace], [float(t) for t in pipe.scheduler.timesteps]

    return model, run


def hy_sampler(frames=3, steps=STEPS):
    fam = Family("hy")
    model = fam.build()
    g = torch.Generator().manual_seed(9)
    lat, img = torch.randn(1, 16, frames, 16, 16, generator=g), torch.randn(1, 16, 1, 16, 16, generator=g)
    mk = lambda v: (torch.randn(1, 20, 64, generator=g).to(BF), torch.randn(1, 64, generator=g).to(BF),
                    torch.cat([torch.ones(1, v), torch.zeros(1, 20 - v)], dim=1).to(BF))
    pos, neg = mk(20), mk(13)
    d = lambda t_: t_.to(DEV)

    def run(transformer=None, **kw):
        pipe = HunyuanVideoImageToVideoPipeline(transformer=transformer or model,
                                                scheduler=FlowMatchEulerDiscreteScheduler(shift=7.0)).to(DEV)
        trace = []
        out = pipe(prompt_embeds=d(pos[0]), pooled_prompt_embeds=d(pos[1]), prompt_attention_mask=d(pos[2]),
                   negative_prompt_embeds=d(neg[0]), negative_pooled_prompt_embeds=d(neg[1]), negative_prompt_attention_mask=d(neg[2]),
                   negative_prompt=None, image_latents=d(img), latents=d(lat), height=128, width=128, num_frames=4 * (frames - 1) + 1,
                   num_inference_steps=steps, true_cfg_scale=6.0, guidance_scale=6.0, output_type="latent", use_low_pass_guidance=True,
                   lp_filter_in_latent=True, step_trace=trace, lp_filter_type="down_up", lp_resize_factor=0.625,
                   lp_strength_schedule_type="interval", schedule_interval_start_time=0.0, schedule_interval_end_time=0.25,
                   **kw).frames
        return out, [n for _, n, _ in trace], [float(t) for t in pipe.scheduler.timesteps]

    return model, run


SAMPLERS = {"cog": cog_sampler, "wan": wan_sampler, "hy": hy_sampler}
