"""CogVideoX image-to-video sampler with Adaptive Low-pass Guidance, MI355X-native.

Drop-in for the reference's ``pipeline_cogvideox_image2video_lowpass.CogVideoXImageToVideoPipeline``
(boundary b-2 of SURVEY.md section 8): same class name, same ``__call__`` keyword arguments and defaults
(reference cog:727-774), same ``check_inputs`` errors (cog:463-524), same output object with ``.frames``.

What runs where
    * the denoising loop (cog:1000-1140) is restructured around two fused launches per step plus the DiT:
      ``transformer.forward_assembled`` (CFG batch assembly folded into the patch gather, no torch.cat) and
      ``scheduler.fused_cfg_step_`` (float(); chunk; combine; DDIM step; cast -- one kernel, in place);
    * ``prepare_lp`` (cog:586-703) filters the conditioning latents with the HIP low-pass kernels, once per
      *distinct* schedule strength instead of every step (the reference re-filters all 50 steps), and without
      the two permute+contiguous copies (both filters are per (H, W) plane, so the plane order is irrelevant);
    * schedule scalars stay on the host in float64, bit-exact with the reference (they drive ``== 0`` tests).

Components that are once-per-video and outside the hot path (text encoder, VAE, video post-processing;
SURVEY.md section 8f "next" rows) are injected duck-typed objects, exactly as diffusers registers them; when
they are absent the caller passes ``prompt_embeds`` / ``negative_prompt_embeds`` (reference kwargs) and
``image_latents`` (extension kwarg) and asks for ``output_type="latent"``.  ``cfg_split=`` (extension kwarg, an
``alg_amd.parallel.CFGPairSplit``) evaluates the cond / uncond passes of one video on two GPUs.
"""
from __future__ import annotations

import inspect
import math
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import torch

from . import _lib, attn_far, attn_pool, attn_reuse, cfg_reuse, lp_utils, sampler_ext
from .schedulers import CogVideoXDDIMScheduler, CogVideoXDPMScheduler
from .transformer_cogvideox import CogVideoXTransformer3DModel


@dataclass
class CogVideoXPipelineOutput:
    frames: Any


def get_resize_crop_region_for_grid(src, tgt_width, tgt_height):
    """reference cog:76-91."""
    h, w = src
    if h / w > tgt_height / tgt_width:
        new_h, new_w = tgt_height, int(round(tgt_height / h * w))
    else:
        new_w, new_h = tgt_width, int(round(tgt_width / w * h))
    top = int(round((tgt_height - new_h) / 2.0))
    left = int(round((tgt_width - new_w) / 2.0))
    return (top, left), (top + new_h, left + new_w)


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, sigmas=None, **kwargs):
    """reference cog:95-151."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("Only one of `timesteps` or `sigmas` can be passed. Please choose one to set custom values")
    accepted = set(inspect.signature(scheduler.set_timesteps).parameters.keys())
    if timesteps is not None:
        if "timesteps" not in accepted:
            raise ValueError(
                f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        return scheduler.timesteps, len(scheduler.timesteps)
    if sigmas is not None:
        if "sigmas" not in accepted:
            raise ValueError(
                f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                f" sigmas schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
        return scheduler.timesteps, len(scheduler.timesteps)
    scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
    return scheduler.timesteps, num_inference_steps


def rotary_tables(embed_dim, crops_coords, grid_size, temporal_size, theta=10000.0, max_size=None):
    """diffusers get_3d_rotary_pos_embed (use_real) -> (cos, sin) each [T*H*W, embed_dim] fp32: the 'linspace' grid over
    `crops_coords` (CogVideoX 1.0) or, with `max_size`, the 'slice' grid (CogVideoX 1.5: integer positions of
    arange(max), cut to the grid).  Head-dim split t/h/w = d/4, 3d/8, 3d/8; each axis' cos/sin repeat-interleaved x2."""
    gh, gw = grid_size
    if max_size is None:
        (top, left), (bottom, right) = crops_coords
        axis_h = torch.linspace(top, bottom * (gh - 1) / gh, gh, dtype=torch.float32)
        axis_w = torch.linspace(left, right * (gw - 1) / gw, gw, dtype=torch.float32)
    else:
        if gh > max_size[0] or gw > max_size[1]:
            raise ValueError("the latent grid exceeds the transformer's sample size (slice rotary embedding)")
        axis_h = torch.arange(max_size[0], dtype=torch.float32)[:gh]
        axis_w = torch.arange(max_size[1], dtype=torch.float32)[:gw]
    axis_t = torch.arange(temporal_size, dtype=torch.float32)

    def axis_table(dim, pos):
        inv = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float32)[: dim // 2] / dim))
        ang = torch.outer(pos, inv)
        return ang.cos().repeat_interleave(2, dim=1).float(), ang.sin().repeat_interleave(2, dim=1).float()

    dt, dh, dw = embed_dim // 4, embed_dim // 8 * 3, embed_dim // 8 * 3
    (ct, st), (ch, sh), (cw, sw) = axis_table(dt, axis_t), axis_table(dh, axis_h), axis_table(dw, axis_w)

    def join(a_t, a_h, a_w):
        a_t = a_t[:, None, None, :].expand(-1, gh, gw, -1)
        a_h = a_h[None, :, None, :].expand(temporal_size, -1, gw, -1)
        a_w = a_w[None, None, :, :].expand(temporal_size, gh, -1, -1)
        return torch.cat([a_t, a_h, a_w], dim=-1).reshape(temporal_size * gh * gw, -1).contiguous()

    return join(ct, ch, cw), join(st, sh, sw)


class CogVideoXImageToVideoPipeline:
    _optional_components: List[str] = []
    model_cpu_offload_seq = "text_encoder->transformer->vae"
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]

    def __init__(self, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler=None):
        self.tokenizer, self.text_encoder, self.vae = tokenizer, text_encoder, vae
        self.transformer, self.scheduler = transformer, scheduler
        vcfg = getattr(vae, "config", None)
        self.vae_scale_factor_spatial = 2 ** (len(vcfg.block_out_channels) - 1) if vcfg is not None else 8
        self.vae_scale_factor_temporal = vcfg.temporal_compression_ratio if vcfg is not None else 4
        self.vae_scaling_factor_image = vcfg.scaling_factor if vcfg is not None else 0.7
        self._device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self._guidance_scale = 1.0
        self._num_timesteps = 0
        self._attention_kwargs = None
        self._current_timestep = None
        self._interrupt = False
        self._lp_cache = {}

    # -- construction ---------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, model_path, torch_dtype=torch.bfloat16, cache_dir=None, transformer=None,
                        scheduler=None, vae=None, text_encoder=None, tokenizer=None, device="cuda", fp8=False,
                        fp4=False, step_cache=0.0, attn_window=0, attn_window_recall=0.0, attn_window_balance=False, attn_window_widths=None,
                        lora=None, **_):
        """Local-disk loader of a diffusers-format CogVideoX-I2V directory (`run.py:38-52`; no hub download here):
        `transformer/`, `vae/`, `text_encoder/` (T5), `tokenizer/`, `scheduler/` -- each read if its sub-directory
        exists and no instance was passed in.  Without a text encoder the call needs `prompt_embeds`, without a VAE
        `image_latents` and `output_type="latent"`.  `fp8=True` loads the transformer with e4m3 block linears
        (CogVideoXTransformer3DModel(..., fp8=True)); `fp4=True` with MXFP4 feed-forward
        linears (CogVideoXTransformer3DModel(..., fp4=True)); neither has an effect on a transformer instance passed in.
        `step_cache` (a threshold), `attn_window` (latent frames on each side), `attn_window_recall` (needs attn_window > 0 here)
        and `attn_window_balance` set the transformer's attributes of these names, also on an instance passed in; all are off by
        default, `attn_window_widths` (head_dim 128 only) is refused, and sampler_ext.window_switches raises ValueError for what
        does not compose before anything is loaded.  `lora` (alg_amd/lora.py) and, from the trailing keywords (the order of the
        named ones is pinned), `attn_reuse`, `attn_reuse_t_lo`, `attn_reuse_t_hi` (alg_amd/attn_reuse.py) and `cfg_reuse`, `cfg_reuse_t_lo`,
        `cfg_reuse_t_hi` (alg_amd/cfg_reuse.py) go to the transformer loader: like `fp8` they have no effect on a transformer instance passed in."""
        import os

        reuse_kw = dict(attn_reuse.switches_from(_), **cfg_reuse.switches_from(_))
        # far-field reuse (alg_amd/attn_far.py): its three trailing keywords, refused here where they do not compose
        reuse_kw.update(attn_far.pipeline_switches(_, reuse_kw, attn_window=attn_window, attn_window_recall=attn_window_recall,
                                                    attn_window_balance=attn_window_balance,
                                                    attn_window_widths=attn_window_widths, step_cache=step_cache))
        # pooled far field (alg_amd/attn_pool.py): its trailing keyword, refused here where it does not compose
        reuse_kw.update(attn_pool.pipeline_switches(_, reuse_kw, attn_window=attn_window, attn_window_recall=attn_window_recall,
                                                     attn_window_balance=attn_window_balance,
                                                     attn_window_widths=attn_window_widths))
        switches = sampler_ext.window_switches(attn_window, attn_window_recall, attn_window_balance, attn_window_widths,
                                               step_cache=step_cache, widths_built=False, recall_needs_window=True)

        from .autoencoder_kl_cogvideox import AutoencoderKLCogVideoX
        from .text_encoder_t5 import T5EncoderModel
        from .weights import load_tokenizer

        has = lambda sub: os.path.isdir(os.path.join(model_path, sub))
        if transformer is None:
            transformer = CogVideoXTransformer3DModel.from_pretrained(model_path, torch_dtype=torch_dtype,
                                                                      device=device, fp8=fp8, fp4=fp4, lora=lora,
                                                                      **reuse_kw)
        sampler_ext.apply_switches(transformer, switches)
        if vae is None and has("vae"):
            vae = AutoencoderKLCogVideoX.from_pretrained(model_path, device=device)
        if text_encoder is None and has("text_encoder"):
            text_encoder = T5EncoderModel.from_pretrained(model_path, device=device)
        if tokenizer is None:
            tokenizer = load_tokenizer(model_path, "tokenizer")
        if scheduler is None:
            scheduler = CogVideoXDDIMScheduler()
            if has("scheduler"):
                # scheduler/scheduler_config.json names its class: CogVideoX-5b-I2V ships the DDIM scheduler, CogVideoX1.5-5B-I2V
                # the DPM one (the loop's second `step` signature, cog:1114-1122)
                import json
                with open(os.path.join(model_path, "scheduler", "scheduler_config.json")) as f:
                    name = json.load(f).get("_class_name", "CogVideoXDDIMScheduler")
                known = {"CogVideoXDDIMScheduler": CogVideoXDDIMScheduler, "CogVideoXDPMScheduler": CogVideoXDPMScheduler}
                if name not in known:
                    raise NotImplementedError("scheduler class %r is not built (CogVideoXDDIMScheduler / CogVideoXDPMScheduler)" % name)
                scheduler = known[name].from_pretrained(model_path)
        return cls(tokenizer, text_encoder, vae, transformer, scheduler)

    def to(self, device=None, *args, **kwargs):
        if device is not None and not isinstance(device, torch.dtype):
            self._device = torch.device(device)
        return self

    @property
    def _execution_device(self):
        return self._device

    def maybe_free_model_hooks(self):
        pass

    # -- properties the reference exposes (cog:705-723) -------------------------------------------------
    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def attention_kwargs(self):
        return self._attention_kwargs

    @property
    def current_timestep(self):
        return self._current_timestep

    @property
    def interrupt(self):
        return self._interrupt

    # -- once-per-video host work ------------------------------------------------------------------------
    def check_inputs(self, image, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs,
                     latents=None, prompt_embeds=None, negative_prompt_embeds=None):
        """Same conditions and messages as reference cog:463-524 (``image`` may additionally be None when the
        caller supplies ``image_latents``)."""
        try:
            import PIL.Image as _pil
            pil_type = _pil.Image
        except Exception:  # pragma: no cover
            pil_type = ()
        if image is not None and not isinstance(image, (torch.Tensor, list)) and not isinstance(image, pil_type):
            raise ValueError(
                "`image` has to be of type `torch.Tensor` or `PIL.Image.Image` or `List[PIL.Image.Image]` but is"
                f" {type(image)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]
            raise ValueError(
                f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found {bad}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(
                f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                " only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError(
                "Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(
                f"Cannot forward both `prompt`: {prompt} and `negative_prompt_embeds`:"
                f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(
                f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError(
                    "`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                    f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds`"
                    f" {negative_prompt_embeds.shape}.")

    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance=True, num_videos_per_prompt=1,
                      prompt_embeds=None, negative_prompt_embeds=None, max_sequence_length=226, device=None,
                      dtype=None):
        """reference cog:270-350.  The T5 encoder is a once-per-video "next" component: when it is not injected
        the caller must pass embeddings."""
        device = device or self._execution_device

        def embed(texts):
            if self.text_encoder is None or self.tokenizer is None:
                raise _lib.AlgHipError(
                    "no text encoder is attached to this pipeline: pass `prompt_embeds` / `negative_prompt_embeds` "
                    "(T5 embeddings [B, %d, text_dim]); the encoder is a once-per-video component outside the hot "
                    "path" % max_sequence_length)
            texts = [texts] if isinstance(texts, str) else texts
            tok = self.tokenizer(texts, padding="max_length", max_length=max_sequence_length, truncation=True,
                                 add_special_tokens=True, return_tensors="pt")
            return self.text_encoder(tok.input_ids.to(device))[0]

        if prompt_embeds is None:
            prompt_embeds = embed(prompt)
        batch = prompt_embeds.shape[0]
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            neg = negative_prompt or ""
            neg = batch * [neg] if isinstance(neg, str) else neg
            if prompt is not None and type(prompt) is not type(negative_prompt if negative_prompt is not None else prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got"
                                f" {type(negative_prompt)} != {type(prompt)}.")
            if batch != len(neg):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(neg)}, but `prompt`:"
                                 f" {prompt} has batch size {batch}.")
            negative_prompt_embeds = embed(neg)
        dtype = dtype or self.transformer.dtype
        prompt_embeds = prompt_embeds.to(device=device, dtype=dtype)
        if negative_prompt_embeds is not None:
            negative_prompt_embeds = negative_prompt_embeds.to(device=device, dtype=dtype)
        return prompt_embeds, negative_prompt_embeds

    def preprocess_image(self, image, height, width):
        """Minimal VideoProcessor.preprocess: tensors are taken as [B,3,H,W] in [-1,1]; PIL images are resized
        (Lanczos) and scaled to [-1,1]."""
        if isinstance(image, torch.Tensor):
            return image if image.ndim == 4 else image.unsqueeze(0)
        import numpy as np
        imgs = image if isinstance(image, list) else [image]
        arr = [np.asarray(im.convert("RGB").resize((width, height), resample=1), dtype=np.float32) / 255.0 for im in imgs]
        t = torch.from_numpy(np.stack(arr)).permute(0, 3, 1, 2).contiguous()
        return 2.0 * t - 1.0

    def prepare_latents(self, image, batch_size=1, num_channels_latents=16, num_frames=13, height=60, width=90,
                        dtype=None, device=None, generator=None, latents=None, image_latents=None):
        """reference cog:352-425: initial noise [B, F_lat, C, h, w] and the conditioning latents (frame 0 = VAE
        latent of the image x scaling factor, frames 1.. zero).  ``image_latents`` (extension) bypasses the VAE:
        either the full [B, F_lat, C, h, w] tensor or just frame 0 as [B, 1, C, h, w]."""
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(
                f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        f_lat = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        h, w = height // self.vae_scale_factor_spatial, width // self.vae_scale_factor_spatial
        shape = (batch_size, f_lat, num_channels_latents, h, w)
        p_t = getattr(self.transformer.config, "patch_size_t", None)
        if p_t is not None:  # cog:380-382: CogVideoX 1.5 pads the noise to a multiple of patch_size_t
            shape = shape[:1] + (shape[1] + shape[1] % p_t,) + shape[2:]
        if image_latents is None:
            if self.vae is None:
                raise _lib.AlgHipError(
                    "no VAE is attached to this pipeline: pass `image_latents` (the scaled VAE latent of the "
                    "conditioning image, [B, 1, C, H/8, W/8]); the VAE is a once-per-video component outside the hot path")
            frames = image.unsqueeze(2)  # [B, C, 1, H, W]
            enc = []
            for i in range(frames.shape[0]):
                g = generator[i] if isinstance(generator, list) else generator
                enc.append(self.vae.encode(frames[i:i + 1].contiguous()).latent_dist.sample(g))
            first = torch.cat(enc, dim=0).to(dtype).permute(0, 2, 1, 3, 4)  # [B, 1, C, h, w]
            if not self.vae.config.invert_scale_latents:
                first = self.vae_scaling_factor_image * first
            else:
                first = 1 / self.vae_scaling_factor_image * first
        else:
            first = image_latents.to(device=device, dtype=dtype)
        if first.shape[1] >= f_lat:
            cond = first.contiguous()
        else:
            cond = torch.zeros((batch_size, f_lat, num_channels_latents, h, w), device=device, dtype=dtype)
            cond[:, : first.shape[1]] = first.to(device)
        if p_t is not None and cond.shape[1] % p_t:  # cog:413-416: repeat the leading frame(s) in front
            cond = torch.cat([cond[:, : cond.shape[1] % p_t], cond], dim=1).contiguous()
        if latents is None:
            if isinstance(generator, list):
                parts = [torch.randn((1,) + shape[1:], generator=g, device=g.device, dtype=dtype) for g in generator]
                latents = torch.cat(parts, dim=0).to(device)
            else:
                gdev = generator.device if generator is not None else device
                latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
        else:
            latents = latents.to(device)
        latents = latents * self.scheduler.init_noise_sigma
        return latents, cond

    def decode_latents(self, latents):
        """reference cog:428-433."""
        if self.vae is None:
            raise _lib.AlgHipError("no VAE is attached to this pipeline: use output_type='latent'")
        if hasattr(self.vae, "decode_latents"):
            # the HIP decoder takes the sampler's [B, F, C, h, w] layout and applies 1 / scaling_factor while packing
            return self.vae.decode_latents(latents.contiguous())
        z = latents.permute(0, 2, 1, 3, 4)
        return self.vae.decode(1 / self.vae_scaling_factor_image * z).sample

    def prepare_extra_step_kwargs(self, generator, eta):
        """reference cog:446-461."""
        accepted = set(inspect.signature(self.scheduler.step).parameters.keys())
        kw = {}
        if "eta" in accepted:
            kw["eta"] = eta
        if "generator" in accepted:
            kw["generator"] = generator
        return kw

    def _prepare_rotary_positional_embeddings(self, height, width, num_frames, device):
        """reference cog:542-584: the cropped linspace grid (CogVideoX 1.0) or the slice grid over
        (num_frames + p_t - 1) // p_t temporal positions (CogVideoX 1.5)."""
        cfg = self.transformer.config
        p, p_t = cfg.patch_size, cfg.patch_size_t
        gh = height // (self.vae_scale_factor_spatial * p)
        gw = width // (self.vae_scale_factor_spatial * p)
        if p_t is None:
            crops = get_resize_crop_region_for_grid((gh, gw), cfg.sample_width // p, cfg.sample_height // p)
            cos, sin = rotary_tables(cfg.attention_head_dim, crops, (gh, gw), num_frames)
        else:
            cos, sin = rotary_tables(cfg.attention_head_dim, None, (gh, gw), (num_frames + p_t - 1) // p_t,
                                     max_size=(cfg.sample_height // p, cfg.sample_width // p))
        return cos.to(device), sin.to(device)

    # -- ALG conditioning ---------------------------------------------------------------------------------
    def prepare_lp(self, lp_filter_type, lp_blur_sigma, lp_blur_kernel_size, lp_resize_factor, generator, num_frames,
                   use_low_pass_guidance, lp_filter_in_latent, orig_image_latents, orig_image_tensor):
        """reference cog:586-703.  Latent branch: per-plane filter of ``[B, F, C, H, W]`` (no permutes needed);
        pixel branch: filter the RGB image, re-encode with the VAE (needs an attached VAE), pad with zero frames."""
        if not use_low_pass_guidance:
            return None
        p_t = getattr(self.transformer.config, "patch_size_t", None)

        def pad_t(x):  # cog:673-680 / 693-699: CogVideoX 1.5 repeats leading frames up to a multiple of patch_size_t
            if p_t is not None and x.size(1) % p_t:
                n = min(p_t - x.size(1) % p_t, x.shape[1])
                x = torch.cat([x[:, :n], x], dim=1)
            return x

        if lp_filter_in_latent:
            out = lp_utils.apply_low_pass_filter(orig_image_latents, lp_filter_type, lp_blur_sigma,
                                                 lp_blur_kernel_size, lp_resize_factor)
            return pad_t(out).to(dtype=orig_image_latents.dtype).contiguous()
        if self.vae is None:
            raise _lib.AlgHipError("lp_filter_in_latent=False re-encodes the filtered image every step and needs a VAE")
        img = lp_utils.apply_low_pass_filter(orig_image_tensor, lp_filter_type, lp_blur_sigma, lp_blur_kernel_size,
                                             lp_resize_factor)
        enc = self.vae.encode(img.unsqueeze(2).contiguous()).latent_dist.sample(generator=generator)
        if not self.vae.config.invert_scale_latents:
            enc = self.vae_scaling_factor_image * enc
        else:
            enc = 1 / self.vae_scaling_factor_image * enc
        enc = enc.permute(0, 2, 1, 3, 4)
        f_lat = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        if f_lat > enc.shape[1]:
            pad = torch.zeros((enc.shape[0], f_lat - enc.shape[1]) + tuple(enc.shape[2:]), device=enc.device,
                              dtype=enc.dtype)
            enc = torch.cat([enc, pad], dim=1)
        else:
            enc = enc[:, :f_lat]
        return pad_t(enc).to(dtype=orig_image_latents.dtype).contiguous()

    def _cached_lp(self, key, make):
        hit = self._lp_cache.get(key)
        if hit is None:
            hit = make()
            self._lp_cache[key] = hit
        return hit

    # -- the sampler ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(
        self,
        image=None,
        prompt: Optional[Union[str, List[str]]] = None,
        negative_prompt: Optional[Union[str, List[str]]] = None,
        height: Optional[int] = None,
        width: Optional[int] = None,
        num_frames: int = 49,
        num_inference_steps: int = 50,
        timesteps: Optional[List[int]] = None,
        guidance_scale: float = 6.0,
        use_dynamic_cfg: bool = False,
        num_videos_per_prompt: int = 1,
        eta: float = 0.0,
        generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
        latents: Optional[torch.Tensor] = None,
        prompt_embeds: Optional[torch.Tensor] = None,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        output_type: str = "pil",
        return_dict: bool = True,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        callback_on_step_end: Optional[Callable] = None,
        callback_on_step_end_tensor_inputs: List[str] = ["latents"],
        max_sequence_length: int = 226,
        use_low_pass_guidance: bool = False,
        lp_filter_type: str = "none",
        lp_filter_in_latent: bool = False,
        lp_blur_sigma: float = 15.0,
        lp_blur_kernel_size: float = 0.02734375,
        lp_resize_factor: float = 0.25,
        lp_strength_schedule_type: str = "none",
        schedule_blur_kernel_size: bool = False,
        schedule_interval_start_time: float = 0.0,
        schedule_interval_end_time: float = 0.05,
        schedule_linear_start_weight: float = 1.0,
        schedule_linear_end_weight: float = 0.0,
        schedule_linear_end_time: float = 0.5,
        schedule_exp_decay_rate: float = 10.0,
        image_latents: Optional[torch.Tensor] = None,
        step_trace: Optional[list] = None,
        cfg_split=None,
        attn_window_dense_steps: int = 0,
    ) -> Union[CogVideoXPipelineOutput, Tuple]:
        """Keyword-compatible with the reference ``__call__`` (cog:727-774); ``image_latents`` and ``step_trace``
        are extensions (VAE bypass; per-step (strength, two_pass, n_forward) log for tests), and so is
        ``attn_window_dense_steps``: the first that many steps run the transformer's opt-in frame window dense."""
        tcfg = self.transformer.config
        if hasattr(callback_on_step_end, "tensor_inputs"):
            callback_on_step_end_tensor_inputs = callback_on_step_end.tensor_inputs
        height = height or tcfg.sample_height * self.vae_scale_factor_spatial
        width = width or tcfg.sample_width * self.vae_scale_factor_spatial
        num_frames = num_frames or tcfg.sample_frames
        num_videos_per_prompt = 1  # the reference overwrites it too (cog:903)

        self.check_inputs(image, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, latents,
                          prompt_embeds, negative_prompt_embeds)
        if image is None and image_latents is None:
            raise ValueError("Provide `image` (needs an attached VAE) or `image_latents`.")
        self._guidance_scale = guidance_scale
        self._current_timestep = None
        self._attention_kwargs = attention_kwargs
        self._interrupt = False
        self._lp_cache = {}

        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None:
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        device = self._execution_device
        if device.type != "cuda":
            raise _lib.AlgHipError("the ALG sampler's hot path is HIP-only: move the pipeline to a GPU "
                                   "(`pipe.to('cuda')`); there is no CPU fallback")
        do_cfg = guidance_scale > 1.0

        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, negative_prompt, do_cfg, num_videos_per_prompt, prompt_embeds, negative_prompt_embeds,
            max_sequence_length, device)
        if do_cfg and use_low_pass_guidance:  # cog:948-951
            prompt_embeds_init = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
            prompt_embeds_3 = torch.cat([negative_prompt_embeds, negative_prompt_embeds, prompt_embeds], dim=0)
        elif do_cfg:  # cog:952-955
            prompt_embeds_init = prompt_embeds_3 = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
        else:
            prompt_embeds_init = prompt_embeds_3 = prompt_embeds
        dtype = prompt_embeds.dtype

        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps)
        self._num_timesteps = len(timesteps)

        # cog:961-968: CogVideoX 1.5 pads the latent frames to a multiple of patch_size_t
        latent_frames = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        additional_frames = 0
        if tcfg.patch_size_t is not None and latent_frames % tcfg.patch_size_t != 0:
            additional_frames = tcfg.patch_size_t - latent_frames % tcfg.patch_size_t
            num_frames += additional_frames * self.vae_scale_factor_temporal
        image_tensor = None
        if image is not None and (image_latents is None or not lp_filter_in_latent):
            image_tensor = self.preprocess_image(image, height, width).to(device, dtype=dtype)
        latent_channels = tcfg.in_channels // 2
        latents, image_latents = self.prepare_latents(
            image_tensor, batch_size * num_videos_per_prompt, latent_channels, num_frames, height, width, dtype,
            device, generator, latents, image_latents)
        latents = latents.to(dtype).contiguous().clone()  # updated in place by the fused step
        image_latents = image_latents.contiguous()

        image_rotary_emb = (self._prepare_rotary_positional_embeddings(height, width, latents.size(1), device)
                            if tcfg.use_rotary_positional_embeddings else None)
        ofs_emb = None if tcfg.ofs_embed_dim is None else latents.new_full((1,), fill_value=2.0)  # cog:998

        if not isinstance(self.scheduler, CogVideoXDDIMScheduler) or not hasattr(self.transformer, "forward_assembled"):
            raise TypeError("this sampler drives alg_amd's CogVideoXTransformer3DModel and CogVideoXDDIMScheduler "
                            "(fused HIP step); other components are not wired yet")
        # `eta` (cog:446-461) reaches scheduler.step through extra_step_kwargs in the reference; the published CogVideoXDDIMScheduler /
        # CogVideoXDPMScheduler accept the argument and never read it (their updates are deterministic given the DPM scheduler's
        # own noise draw), so any value samples exactly like eta = 0 -- here too (unpinned: diffusers is absent)
        is_dpm = isinstance(self.scheduler, CogVideoXDPMScheduler)
        old_pred_original_sample = None  # cog:998

        B = latents.shape[0]
        # the transformer's opt-in extensions (alg_amd/sampler_ext.py): refusals and resets here, one callable per step below
        ext = sampler_ext.SamplerExtensions(self.transformer, len(timesteps), attn_window_dense_steps, cfg_split,
                                            forward=self.transformer.forward_assembled, host_timestep=int, do_cfg=do_cfg)
        # every timestep of the schedule on the device ONCE: a step takes a view of it (no host tensor + H2D copy per step)
        ts_dev = torch.as_tensor([int(t_) for t_ in timesteps], dtype=torch.float32).to(device)
        for i, t in enumerate(timesteps):
            if self._interrupt:
                continue
            self._current_timestep = t
            strength = None
            if not use_low_pass_guidance:
                two_pass = True
            if do_cfg and use_low_pass_guidance:
                strength = lp_utils.get_lp_strength(
                    step_index=i, total_steps=num_inference_steps,
                    lp_strength_schedule_type=lp_strength_schedule_type,
                    schedule_interval_start_time=schedule_interval_start_time,
                    schedule_interval_end_time=schedule_interval_end_time,
                    schedule_linear_start_weight=schedule_linear_start_weight,
                    schedule_linear_end_weight=schedule_linear_end_weight,
                    schedule_linear_end_time=schedule_linear_end_time,
                    schedule_exp_decay_rate=schedule_exp_decay_rate)
                two_pass = (strength == 0 or not use_low_pass_guidance)
                if lp_strength_schedule_type == "exponential" and strength < 0.1:
                    two_pass = True
                sigma_i = lp_blur_sigma * strength
                ksize_i = lp_blur_kernel_size * strength if schedule_blur_kernel_size else lp_blur_kernel_size
                factor_i = 1.0 - (1.0 - lp_resize_factor) * strength
                if lp_filter_in_latent:
                    # the filter is a pure function of (type, sigma, k, factor): launch it once per distinct value
                    lp_lat = self._cached_lp(
                        (lp_filter_type, sigma_i, ksize_i, type(ksize_i), factor_i),
                        lambda: self.prepare_lp(lp_filter_type, sigma_i, ksize_i, factor_i, generator, num_frames,
                                                use_low_pass_guidance, True, image_latents, image_tensor))
                else:  # pixel branch consumes the generator every step (cog:645) -> never cached
                    lp_lat = self.prepare_lp(lp_filter_type, sigma_i, ksize_i, factor_i, generator, num_frames,
                                             use_low_pass_guidance, False, image_latents, image_tensor)
                if two_pass:
                    cond_groups, embeds = [lp_lat, lp_lat], prompt_embeds_init          # cog:1068
                else:
                    cond_groups, embeds = [image_latents, lp_lat, lp_lat], prompt_embeds_3  # cog:1070
            elif do_cfg:
                cond_groups, embeds = [image_latents, image_latents], prompt_embeds_init
            else:
                # reference quirk (cog:1011-1012, 1084): with ALG on and guidance_scale <= 1, `two_pass` is unbound
                if use_low_pass_guidance:
                    raise NameError("name 'two_pass' is not defined (use_low_pass_guidance=True needs guidance_scale > 1)")
                cond_groups, embeds = [image_latents], prompt_embeds_init
            n_pass = len(cond_groups)
            # CFG reuse (alg_amd/cfg_reuse.py; off: the plain plan, nothing below differs): a reused step runs the conditional
            # pass alone -- the last group, the last B rows of the embeddings -- and rebuilds the unconditional prediction
            plan = ext.cfg_plan(i, t, n_pass)
            if plan.reuse:
                cond_groups, embeds, n_pass = cond_groups[-1:], embeds[-B:], 1
            conds = [g[b:b + 1] for g in cond_groups for b in range(B)]
            lat_in = latents if B == 1 else torch.cat([latents] * n_pass, dim=0)
            ts = ts_dev[i:i + 1].expand(n_pass * B)
            dit = ext.step(i, t, n_pass, B)
            if cfg_split is not None and n_pass > 1:
                # alg_amd.parallel.CFGPairSplit: this rank evaluates its share of the CFG passes, one all-gather merges
                # the predictions; combine + step below run identically on both ranks of the pair
                rows = [p_ * B + b for p_ in cfg_split.my_passes(n_pass) for b in range(B)]
                lat_l = latents if B == 1 else torch.cat([latents] * (len(rows) // B), dim=0)
                local = dit(lat_l, [conds[r] for r in rows], embeds[rows].contiguous(), ts[:len(rows)], image_rotary_emb, ofs=ofs_emb)
                noise_pred = cfg_split.merge(local, n_pass, B)
            else:
                noise_pred = dit(lat_in, conds, embeds, ts, image_rotary_emb, ofs=ofs_emb)
            gs = guidance_scale
            if do_cfg and not use_low_pass_guidance and use_dynamic_cfg:  # cog:1105-1108
                gs = 1 + guidance_scale * (
                    (1 - math.cos(math.pi * ((num_inference_steps - int(t)) / num_inference_steps) ** 5.0)) / 2)
                self._guidance_scale = gs
            if is_dpm:
                # cog:1091-1123, DPM branch: float(); CFG combine in fp32; the two-output step; cast back
                pred32 = noise_pred.float()
                if plan.mode is not None:
                    pred32 = _lib.cfg_combine_delta(pred32, plan.delta(latents.shape, torch.float32, device), plan.mode, gs)
                elif n_pass > 1:
                    pred32 = _lib.cfg_combine(pred32, n_pass, gs)
                new_lat, old_pred_original_sample = self.scheduler.step(
                    pred32, old_pred_original_sample, t, timesteps[i - 1] if i > 0 else None, latents,
                    generator=generator, return_dict=False)
                latents = _lib.lincomb([(1.0, new_lat)], dtype)
            elif plan.mode is not None:
                self.scheduler.fused_cfg_step_delta_(noise_pred, latents, plan.delta(latents.shape, torch.float32, device),
                                                     plan.mode, gs, t)
            else:
                self.scheduler.fused_cfg_step_(noise_pred, latents, n_pass, gs, t)
            plan.finish()
            if step_trace is not None:
                step_trace.append((strength, bool(two_pass), n_pass * B))
            if callback_on_step_end is not None:
                cb_kwargs = {"latents": latents, "prompt_embeds": prompt_embeds,
                             "negative_prompt_embeds": negative_prompt_embeds}
                cb_kwargs = {k: cb_kwargs[k] for k in callback_on_step_end_tensor_inputs}
                outs = callback_on_step_end(self, i, t, cb_kwargs) or {}
                new_lat = outs.pop("latents", latents)
                if new_lat is not latents:
                    latents = new_lat.to(dtype).contiguous().clone()
                    ext.cfg_invalidate()
                new_pe = outs.pop("prompt_embeds", prompt_embeds)
                new_ne = outs.pop("negative_prompt_embeds", negative_prompt_embeds)
                if new_pe is not prompt_embeds or new_ne is not negative_prompt_embeds:
                    # cog:1126-1134: the callback may replace the embeddings the next forward uses.  The reference hands it
                    # the already concatenated batch; here the two halves are exposed under the same names and the
                    # pre-concatenated CFG batches are rebuilt from what the callback returned.
                    prompt_embeds, negative_prompt_embeds = new_pe.to(device, dtype), (
                        None if new_ne is None else new_ne.to(device, dtype))
                    ext.cfg_invalidate()
                    if do_cfg and use_low_pass_guidance:
                        prompt_embeds_init = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
                        prompt_embeds_3 = torch.cat([negative_prompt_embeds, negative_prompt_embeds, prompt_embeds], dim=0)
                    elif do_cfg:
                        prompt_embeds_init = prompt_embeds_3 = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
                    else:
                        prompt_embeds_init = prompt_embeds_3 = prompt_embeds
        self._current_timestep = None

        if output_type != "latent":
            latents = latents[:, additional_frames:]  # cog:1144: discard the CogVideoX 1.5 padding frames
        if output_type == "latent":
            video = latents
        elif output_type in ("pil", "uint8") and hasattr(self.vae, "decode_latents"):
            # decode + postprocess_video + the writer's uint8 conversion (run:121-125) end in one kernel: [B, F, H, W, 3]
            video = self.vae.decode_latents(latents.contiguous(), to_uint8=True)
            if output_type == "pil":
                from PIL import Image
                video = [[Image.fromarray(f) for f in vid] for vid in video.cpu().numpy()]
        else:
            video = self.decode_latents(latents)
            video = self.postprocess_video(video, output_type)
        self.maybe_free_model_hooks()
        if not return_dict:
            return (video,)
        return CogVideoXPipelineOutput(frames=video)

    def postprocess_video(self, video, output_type="pil"):
        """VideoProcessor.postprocess_video (cog:1148): [B, C, F, H, W] in [-1, 1] -> 'pt' | 'np' | 'pil'; the
        denormalisation runs in the video's dtype, as the tensor ops of the published processor do."""
        v = (video * 0.5 + 0.5).clamp(0, 1)
        if output_type == "pt":
            return v.permute(0, 2, 1, 3, 4)
        arr = v.permute(0, 2, 3, 4, 1).cpu().float().numpy()  # [B, F, H, W, C]
        if output_type == "np":
            return arr
        if output_type == "pil":
            from PIL import Image
            return [[Image.fromarray((f * 255).round().astype("uint8")) for f in vid] for vid in arr]
        raise ValueError(f"{output_type} is not supported. Make sure to choose one of ['np', 'pt', 'pil']")
