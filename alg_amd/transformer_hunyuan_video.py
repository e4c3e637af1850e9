"""HunyuanVideo image-to-video DiT forward, MI355X-native.

Drop-in for the component the reference's HunyuanVideo sampler calls at pipeline_hunyuan_video_image2video_lowpass.py:
1243-1252 (``transformer(hidden_states=, timestep=, encoder_hidden_states=, encoder_attention_mask=, pooled_projections=,
guidance=, attention_kwargs=, return_dict=False)[0]``) and reads ``.dtype`` and ``.config.{image_condition_type,
in_channels, guidance_embeds, patch_size}`` from (hy:1016, 1049-1051, 1116, 781).  The arithmetic follows diffusers'
HunyuanVideoTransformer3DModel (diffusers @ be2fb77, not in the reference tree -- parity unpinned, oracle/hy_oracle.py);
state-dict names are diffusers'.

Layout: one joint residual buffer ``[N, S + L, D]`` with the S latent tokens first and the L (padded) prompt tokens
after them, so the 20 dual-stream blocks address the two streams as row ranges and the 40 single-stream blocks run in
place on the whole buffer.  Padded prompt tokens are masked as attention KEYS in the published model, i.e. every query
attends to the prefix ``S + valid[b]`` of the joint sequence: ``alg_flash_attn_d128`` is launched per sample with that
key length (their own rows are carried along and never read by a latent).  "token_replace" conditioning maps onto the
two-segment modulation / gate support the CogVideoX kernels already have: rows < first-frame tokens take the
timestep-0 vectors (``alg_layernorm_modulate_seg``, ``alg_gemm_bf16`` gate segments).
Kernels: alg_patchify3d, alg_timestep_embedding, alg_gemm_bf16 (all linears, fused SiLU / GELU-tanh / gated-residual
epilogues, V written transposed), alg_masked_mean, alg_silu, alg_lincomb, alg_layernorm_modulate(_seg), alg_headnorm_rope,
alg_flash_attn_d128, alg_unpatchify3d.  No CPU fallback.

fp8 mode only (``fp8=True``; allocated on the first fp8 forward of a shape):
    q8     [N * J, D + M] bytes  OCP e4m3 copy of the current GEMM input (rows of K = D, M or D + M bytes, contiguous)
    q8s    [N, J4] float32       its per-token scales, J4 = J rounded up to a multiple of 4 (the V^T GEMM reads them as its B
                                 scales, 16 bytes at a time, per batch item)
Kernels added by it: alg_layernorm_modulate_seg_fp8, alg_quantize_fp8_rows_batched, alg_gemm_fp8.
"""
from __future__ import annotations

import glob
import json
import math
import os
from dataclasses import asdict, dataclass
from types import SimpleNamespace

import torch

from . import _lib
from .attn_far import AttnFarHost
from .attn_pool import AttnPoolHost
from .attn_reuse import AttnReuseHost
from .cfg_reuse import CfgReuseHost
from .attn_window import HeadWindowHost, SelfAttnOperands, calibrate_self_attention, launch_self_attention
from .transformer_wan import k_scale_bound

BF = torch.bfloat16


@dataclass
class HunyuanVideoTransformerConfig:
    in_channels: int = 16
    out_channels: int = 16
    num_attention_heads: int = 24
    attention_head_dim: int = 128
    num_layers: int = 20
    num_single_layers: int = 40
    num_refiner_layers: int = 2
    mlp_ratio: float = 4.0
    patch_size: int = 2
    patch_size_t: int = 1
    qk_norm: str = "rms_norm"
    guidance_embeds: bool = False
    text_embed_dim: int = 4096
    pooled_projection_dim: int = 768
    rope_theta: float = 256.0
    rope_axes_dim: tuple = (16, 56, 56)
    image_condition_type: str = "token_replace"

    @property
    def dim(self):
        return self.num_attention_heads * self.attention_head_dim

    def to_dict(self):
        return asdict(self)


def parameter_shapes(cfg):
    """diffusers state-dict name -> shape (all bf16 after from_pretrained(torch_dtype=bf16))."""
    D, M = cfg.dim, int(cfg.dim * cfg.mlp_ratio)
    p, pt = cfg.patch_size, cfg.patch_size_t
    s = {}

    def lin(name, n_out, n_in):
        s[name + ".weight"] = (n_out, n_in)
        s[name + ".bias"] = (n_out,)

    s["x_embedder.proj.weight"] = (D, cfg.in_channels, pt, p, p)
    s["x_embedder.proj.bias"] = (D,)
    ce = "context_embedder."
    lin(ce + "time_text_embed.timestep_embedder.linear_1", D, 256)
    lin(ce + "time_text_embed.timestep_embedder.linear_2", D, D)
    lin(ce + "time_text_embed.text_embedder.linear_1", D, cfg.text_embed_dim)
    lin(ce + "time_text_embed.text_embedder.linear_2", D, D)
    lin(ce + "proj_in", D, cfg.text_embed_dim)
    for l in range(cfg.num_refiner_layers):
        b = ce + f"token_refiner.refiner_blocks.{l}."
        for n in ("norm1", "norm2"):
            s[b + n + ".weight"] = (D,)
            s[b + n + ".bias"] = (D,)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            lin(b + "attn." + n, D, D)
        lin(b + "ff.net.0.proj", M, D)
        lin(b + "ff.net.2", D, M)
        lin(b + "norm_out.linear", 2 * D, D)
    te = "time_text_embed."
    lin(te + "timestep_embedder.linear_1", D, 256)
    lin(te + "timestep_embedder.linear_2", D, D)
    lin(te + "text_embedder.linear_1", D, cfg.pooled_projection_dim)
    lin(te + "text_embedder.linear_2", D, D)
    if cfg.guidance_embeds:
        lin(te + "guidance_embedder.linear_1", D, 256)
        lin(te + "guidance_embedder.linear_2", D, D)
    for l in range(cfg.num_layers):
        b = f"transformer_blocks.{l}."
        lin(b + "norm1.linear", 6 * D, D)
        lin(b + "norm1_context.linear", 6 * D, D)
        for n in ("to_q", "to_k", "to_v", "to_out.0", "add_q_proj", "add_k_proj", "add_v_proj", "to_add_out"):
            lin(b + "attn." + n, D, D)
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            s[b + "attn." + n + ".weight"] = (cfg.attention_head_dim,)
        lin(b + "ff.net.0.proj", M, D)
        lin(b + "ff.net.2", D, M)
        lin(b + "ff_context.net.0.proj", M, D)
        lin(b + "ff_context.net.2", D, M)
    for l in range(cfg.num_single_layers):
        b = f"single_transformer_blocks.{l}."
        lin(b + "norm.linear", 3 * D, D)
        for n in ("to_q", "to_k", "to_v"):
            lin(b + "attn." + n, D, D)
        for n in ("norm_q", "norm_k"):
            s[b + "attn." + n + ".weight"] = (cfg.attention_head_dim,)
        lin(b + "proj_mlp", M, D)
        lin(b + "proj_out", D, D + M)
    lin("norm_out.linear", 2 * D, D)
    lin("proj_out", pt * p * p * cfg.out_channels, D)
    return s


def synthetic_state_dict(cfg, seed=1234, device="cuda"):
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for name, shape in parameter_shapes(cfg).items():
        r = lambda: torch.randn(shape, generator=g, device=dev, dtype=torch.float32)
        if name.endswith("weight") and len(shape) == 1:
            t = 1.0 + 0.1 * r()
        elif name.endswith("bias"):
            t = 0.02 * r()
        else:
            t = r() / math.prod(shape[1:]) ** 0.5
        sd[name] = t.to(BF)
    return sd


class HunyuanVideoTransformer3DModel(AttnReuseHost, AttnFarHost, AttnPoolHost, CfgReuseHost, HeadWindowHost):
    dtype = BF
    # what lora.merge_into did to the state dict this model was built from (from_pretrained / from_synthetic(lora=...)): a tuple
    # of lora.LoraReport(name, scale, targets, ranks) per adapter; () without LoRA
    lora_report = ()

    # the block linears that fp8 mode quantises, per output channel (attribute names of a block's weights): dual blocks, latent
    # stream: to_q | to_k, to_v, to_out.0, ff.net.0.proj, ff.net.2; single blocks: to_q | to_k, to_v, proj_mlp, proj_out
    FP8_DUAL = ("wqk", "v", "o", "f1", "f2")
    FP8_SINGLE = ("wqk", "v", "mlp", "out")

    def __init__(self, config: HunyuanVideoTransformerConfig, weights: dict, device="cuda", fp8_attention=False, fp8=False):
        """``fp8=True`` (opt-in): the large block linears run on the fp8 MFMA (alg_gemm_fp8) in oracle/fp8_oracle.py's scheme --
        weights quantised once to OCP e4m3 with one scale per output channel, activations with one scale per token in front of
        each GEMM, fp32 accumulation, one rounding to bf16 in the epilogue.  Quantised: in the dual-stream blocks the LATENT
        stream's attn.to_q | to_k, attn.to_v, attn.to_out.0, ff.net.0.proj, ff.net.2; in the single-stream blocks, on the joint
        [latents; text] rows, attn.to_q | to_k, attn.to_v, proj_mlp and proj_out (whose operand is the 15,360-wide row
        [attention | gelu(mlp)] with ONE scale per token).  Everything else stays bf16 exactly as without the flag: the prompt
        stream of the dual blocks (add_q/k/v_proj, to_add_out, ff_context), the token refiner, the embedders, all AdaLN
        linears, the output head, the norms, the attention and the residual stream.  Built this way the model keeps no bf16 (or
        packed) copy of the quantised weights and cannot run a bf16 forward.  ``model.fp8`` may also be flipped on a model built
        in bf16 (A/B runs): the e4m3 copies are then made on the first fp8 forward and both sets are kept.  Needs dim % 512 == 0
        and dim * mlp_ratio % 128 == 0.  Independent of ``fp8_attention``.

        ``fp8_attention=True`` (opt-in, may be flipped between calls): the joint attention of the dual- and single-stream
        blocks runs on alg_flash_attn_d128_fp8 -- the per-head RMSNorm + RoPE pass writes Q (one scale per token and head) and K
        (one scale per head, transformer_wan.k_scale_bound) as e4m3 itself, V^T is quantised per row behind its GEMMs.  The token
        refiner stays bf16.  Off, the forward is the bf16 one bit for bit."""
        self.fp8_attention = bool(fp8_attention)
        # > 0 (opt-in, an extension: alg_amd/attn_window.py; may be flipped between calls): in the joint attention of the dual-
        # and single-stream blocks a block of latent queries attends to the conditioning frames (attn_sink_frames), to the latent
        # frames within attn_window of its own and to the sample's valid prompt keys; prompt queries see everything.  The launches
        # stay per sample (alg_flash_attn_d128_ranges).  0: today's launches, nothing allocated
        self.attn_window = 0
        self.attn_sink_frames = 1
        # attn_window_recall > 0 (opt-in, with attn_window > 0): only the heads whose measured recall (over the latent queries,
        # minimum over the samples) reaches it keep the window (attn_window.HeadWindowHost).  0.0: the shared window, nothing allocated
        self._head_window_init()
        # N >= 2 (opt-in, an extension: alg_amd/attn_reuse.py): a forward that is handed `cache_keys` with the step's timestep
        # (attn_reuse.step_keys) computes every block's joint attention on every N-th step while attn_reuse_t_lo < t < attn_reuse_t_hi
        # and reads its latent and prompt rows back from a per-key cache on the steps between.  Skipped then -- dual blocks: both
        # streams' norm1, the four Q|K / V projections, the four head norms, the attention; single blocks: Q|K, V^T, the head norms
        # and the attention (the norm and proj_mlp stay: the MLP half needs them).  0: every forward is the plain one, launch for
        # launch, nothing allocated.  attn_reuse_drift: the diagnostic (AttnReuseHost)
        self.attn_reuse = 0
        # N >= 2 (opt-in, an extension: alg_amd/attn_far.py; needs attn_window > 0): the keys inside the frame window are attended
        # to fresh on every step, the keys outside it on every N-th step while attn_far_reuse_t_lo < t < attn_far_reuse_t_hi and
        # from the cached partial (output and LSE) on the steps between, merged by alg_attn_merge_lse.  0: nothing differs
        self.attn_far_reuse = 0
        # G in {2, 4, 8} (opt-in, an extension: alg_amd/attn_pool.py; needs attn_window > 0): the keys outside the frame window are
        # attended to on every step as groups of G consecutive keys pooled into one (mean k, mean v, a score bias of log2 G), merged
        # with the window's partial by alg_attn_merge_lse_shift.  No state across steps.  0: nothing differs
        self.attn_far_pool = 0
        self.fp8 = bool(fp8)
        if config.qk_norm != "rms_norm" or config.attention_head_dim != 128 or config.patch_size_t != 1:
            raise NotImplementedError("the HunyuanVideo DiT path is built for rms_norm, head_dim 128, patch_size_t 1")
        if sum(config.rope_axes_dim) != config.attention_head_dim:
            raise ValueError("rope_axes_dim must add up to the head dimension")
        self.config = config
        if self.fp8:
            self._check_fp8_shapes()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AlgHipError("HunyuanVideoTransformer3DModel runs on the GPU only (HIP kernels); no CPU fallback")
        _lib.load_library()
        missing = [k for k in parameter_shapes(config) if k not in weights]
        if missing:
            raise KeyError("state dict is missing %d tensors, e.g. %s" % (len(missing), missing[:3]))
        dev, D = self.device, config.dim
        bf = lambda n: weights[n].to(device=dev, dtype=BF).contiguous()
        cat = lambda *ns: torch.cat([bf(n) for n in ns], dim=0).contiguous()
        lin = lambda pre: (bf(pre + ".weight"), bf(pre + ".bias"))
        w = SimpleNamespace()
        kin = config.in_channels * config.patch_size ** 2
        self.k_patch = (kin + 63) // 64 * 64
        wp = torch.zeros(D, self.k_patch, dtype=BF, device=dev)
        wp[:, :kin] = bf("x_embedder.proj.weight").reshape(D, kin)
        w.patch_w, w.patch_b = wp, bf("x_embedder.proj.bias")
        ce, te = "context_embedder.", "time_text_embed."
        w.r_t1, w.r_t2 = lin(ce + "time_text_embed.timestep_embedder.linear_1"), lin(ce + "time_text_embed.timestep_embedder.linear_2")
        w.r_x1, w.r_x2 = lin(ce + "time_text_embed.text_embedder.linear_1"), lin(ce + "time_text_embed.text_embedder.linear_2")
        w.r_in = lin(ce + "proj_in")
        self.refiner = []
        for l in range(config.num_refiner_layers):
            b = ce + f"token_refiner.refiner_blocks.{l}."
            R = SimpleNamespace()
            R.n1w, R.n1b, R.n2w, R.n2b = bf(b + "norm1.weight"), bf(b + "norm1.bias"), bf(b + "norm2.weight"), bf(b + "norm2.bias")
            R.wqk = cat(b + "attn.to_q.weight", b + "attn.to_k.weight")
            R.bqk = cat(b + "attn.to_q.bias", b + "attn.to_k.bias")
            R.v, R.o = lin(b + "attn.to_v"), lin(b + "attn.to_out.0")
            R.f1, R.f2, R.ada = lin(b + "ff.net.0.proj"), lin(b + "ff.net.2"), lin(b + "norm_out.linear")
            self.refiner.append(R)
        w.t1, w.t2 = lin(te + "timestep_embedder.linear_1"), lin(te + "timestep_embedder.linear_2")
        w.p1, w.p2 = lin(te + "text_embedder.linear_1"), lin(te + "text_embedder.linear_2")
        if config.guidance_embeds:
            w.g1, w.g2 = lin(te + "guidance_embedder.linear_1"), lin(te + "guidance_embedder.linear_2")
        self.dual = []
        for l in range(config.num_layers):
            b = f"transformer_blocks.{l}."
            L = SimpleNamespace()
            L.ada, L.ada_c = lin(b + "norm1.linear"), lin(b + "norm1_context.linear")
            L.wqk = cat(b + "attn.to_q.weight", b + "attn.to_k.weight")
            L.bqk = cat(b + "attn.to_q.bias", b + "attn.to_k.bias")
            L.wqk_c = cat(b + "attn.add_q_proj.weight", b + "attn.add_k_proj.weight")
            L.bqk_c = cat(b + "attn.add_q_proj.bias", b + "attn.add_k_proj.bias")
            L.v, L.v_c = lin(b + "attn.to_v"), lin(b + "attn.add_v_proj")
            L.o, L.o_c = lin(b + "attn.to_out.0"), lin(b + "attn.to_add_out")
            L.nq, L.nk = bf(b + "attn.norm_q.weight"), bf(b + "attn.norm_k.weight")
            L.nq_c, L.nk_c = bf(b + "attn.norm_added_q.weight"), bf(b + "attn.norm_added_k.weight")
            L.f1, L.f2 = lin(b + "ff.net.0.proj"), lin(b + "ff.net.2")
            L.f1_c, L.f2_c = lin(b + "ff_context.net.0.proj"), lin(b + "ff_context.net.2")
            # one K scale per head covers the latent keys (norm_k + RoPE) and the prompt keys (norm_added_k) of the joint sequence
            L.k8_scale = torch.maximum(k_scale_bound(L.nk, 128, config.num_attention_heads, rope=True),
                                       k_scale_bound(L.nk_c, 128, config.num_attention_heads, rope=False))
            if self.fp8:
                L.packed = {}
                self._quantize_block(L, self.FP8_DUAL, drop_bf16=True)
            else:
                L.packed = {id(t): _lib.PackedB(t) for t in (L.wqk, L.o[0], L.f1[0], L.f2[0])}     # the latent stream's linears (see packed_weights)
            self.dual.append(L)
        self.single = []
        for l in range(config.num_single_layers):
            b = f"single_transformer_blocks.{l}."
            L = SimpleNamespace()
            L.ada = lin(b + "norm.linear")
            L.wqk = cat(b + "attn.to_q.weight", b + "attn.to_k.weight")
            L.bqk = cat(b + "attn.to_q.bias", b + "attn.to_k.bias")
            L.v = lin(b + "attn.to_v")
            L.nq, L.nk = bf(b + "attn.norm_q.weight"), bf(b + "attn.norm_k.weight")
            L.mlp, L.out = lin(b + "proj_mlp"), lin(b + "proj_out")
            L.k8_scale = k_scale_bound(L.nk, 128, config.num_attention_heads, rope=True)
            if self.fp8:
                L.packed = {}
                self._quantize_block(L, self.FP8_SINGLE, drop_bf16=True)
            else:
                L.packed = {id(t): _lib.PackedB(t) for t in (L.wqk, L.mlp[0], L.out[0])}
            self.single.append(L)
        w.ada_out, w.out = lin("norm_out.linear"), lin("proj_out")
        self.w = w
        self._ws = {}
        self._rope_cache = {}
        self.profile = None  # set to a dict to collect (start, stop) HIP event pairs per kernel family of the large launches
        # True (default): the weight-times-token linears of the latent / joint stream (Q|K, out, ff1, ff2; single blocks: Q|K, proj_mlp,
        # proj_out) keep a copy packed in MFMA-fragment order (alg_pack_b_p11) and run GEMM schedule 11 (bit-identical to schedule 10);
        # False, or ALG_GEMM_PIPE set to another schedule than 10: the row-major weights.  The prompt stream's few rows stay as they are.
        self.packed_weights = True

    def _check_fp8_shapes(self):
        D, M = self.config.dim, int(self.config.dim * self.config.mlp_ratio)
        if D % 512:
            raise ValueError("fp8=True: the norm that writes the e4m3 tokens needs D %% 512 == 0, this config has dim = %d" % D)
        if M % 128:
            raise ValueError("fp8=True: the e4m3 GEMM needs K %% 128 == 0, this config has dim = %d and an MLP width of %d"
                             % (D, M))

    @staticmethod
    def _quantize_block(L, names, drop_bf16):
        """e4m3 copies (bytes, per-output-channel float32 scales) of a block's listed linears under "<name>8"; drop_bf16: the
        bf16 weight goes (its bias stays)."""
        for nm in names:
            held = getattr(L, nm)
            wt = held[0] if isinstance(held, tuple) else held
            q = torch.empty(wt.shape, dtype=torch.uint8, device=wt.device)
            sc = torch.empty(wt.shape[0], dtype=torch.float32, device=wt.device)
            _lib.quantize_fp8_rows(wt, q, sc, wt.shape[0], wt.shape[1])
            setattr(L, nm + "8", (q, sc))
            if drop_bf16:
                setattr(L, nm, (None, held[1]) if isinstance(held, tuple) else None)

    @classmethod
    def from_synthetic(cls, config=None, seed=1234, device="cuda", fp8_attention=False, fp8=False, lora=None):
        """`lora` (a path, (path_or_dict, scale), {"path", "scale", "name"} or a list of them: alg_amd/lora.py) is merged into
        the state dict before the model is built from it."""
        from . import lora as _lora
        config = config or HunyuanVideoTransformerConfig()
        sd = synthetic_state_dict(config, seed=seed, device=device)
        return _lora.build(cls, config, sd, lora, device, fp8_attention=fp8_attention, fp8=fp8)

    @classmethod
    def from_pretrained(cls, path, subfolder="transformer", torch_dtype=BF, device="cuda", fp8_attention=False, fp8=False,
                        lora=None, **_):
        """Load a diffusers-format checkpoint directory from local disk.  `lora` (as in from_synthetic) is merged into the state
        dict before the model is built from it; in a multi-rank run every rank merges for itself behind the weight broadcast.  `attn_reuse`, `attn_reuse_t_lo` and `attn_reuse_t_hi` (taken from the trailing keywords; alg_amd/attn_reuse.py) set the
        model's attention-reuse switches: 0 / 100 / 800 by default, attn_reuse = 1 and lo >= hi are ValueErrors.  `cfg_reuse`,
        `cfg_reuse_t_lo` and `cfg_reuse_t_hi` (alg_amd/cfg_reuse.py) set the samplers' CFG-reuse switches the same way."""
        from . import cfg_reuse as _cfg_reuse
        from .attn_reuse import apply_switches, switches_from
        reuse = switches_from(_)
        cfg_switches = _cfg_reuse.switches_from(_)
        from . import attn_far as _attn_far
        far_switches = _attn_far.switches_from(_)     # attn_far_reuse, attn_far_reuse_t_lo, attn_far_reuse_t_hi
        from . import attn_pool as _attn_pool
        pool_switches = _attn_pool.switches_from(_)   # attn_far_pool
        root = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        cfg_path = os.path.join(root, "config.json")
        if not os.path.exists(cfg_path):
            raise FileNotFoundError("%s not found: weights must be on local disk (no network access in this build; use "
                                    "HunyuanVideoTransformer3DModel.from_synthetic)" % cfg_path)
        with open(cfg_path) as f:
            raw = json.load(f)
        fields = HunyuanVideoTransformerConfig.__dataclass_fields__
        cfg = HunyuanVideoTransformerConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in raw.items()
                                               if k in fields})
        from .weights import read_shards
        from . import lora as _lora
        model = _lora.build(cls, cfg, read_shards(root), lora, device, fp8_attention=fp8_attention, fp8=fp8)
        apply_switches(model, reuse)
        _cfg_reuse.apply_switches(model, cfg_switches)
        _attn_far.apply_switches(model, far_switches)
        _attn_pool.apply_switches(model, pool_switches)
        return model

    def to(self, *a, **k):
        return self

    def rope_tables(self, F_, H, W):
        key = (F_, H, W)
        hit = self._rope_cache.get(key)
        if hit is None:
            cfg = self.config
            sizes = (F_ // cfg.patch_size_t, H // cfg.patch_size, W // cfg.patch_size)
            grids = torch.meshgrid(*[torch.arange(0, n, dtype=torch.float32) for n in sizes], indexing="ij")
            cos, sin = [], []
            for dim, grid in zip(cfg.rope_axes_dim, grids):
                freqs = 1.0 / (cfg.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.float32)[: dim // 2] / dim))
                ang = torch.outer(grid.reshape(-1), freqs)
                cos.append(ang.cos().repeat_interleave(2, dim=1))
                sin.append(ang.sin().repeat_interleave(2, dim=1))
            hit = (torch.cat(cos, dim=1).float().to(self.device).contiguous(),
                   torch.cat(sin, dim=1).float().to(self.device).contiguous())
            self._rope_cache[key] = hit
        return hit

    def _workspace(self, N, S, L):
        key = (N, S, L)
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()
            cfg, dev = self.config, self.device
            D, M = cfg.dim, int(cfg.dim * cfg.mlp_ratio)
            J = S + L
            e = lambda *s, dt=BF: torch.empty(*s, dtype=dt, device=dev)
            z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=dev)
            ws = SimpleNamespace(J=J, J_pad=(J + 63) // 64 * 64, L_pad=(L + 63) // 64 * 64)
            ws.patches = e(N, S, self.k_patch)
            ws.x, ws.y = e(N, J, D), e(N, J, D)
            ws.qk = e(N, J, 2 * D)
            ws.vt = z(N, D, ws.J_pad)
            ws.am = e(N, J, D + M)                       # [attention out | mlp hidden] per token (single-block proj_out input)
            ws.tok = e(N, S, self.w.out[0].shape[0])
            ws.tsin = e(2 * N, 256)
            ws.h1, ws.tA, ws.tB = e(2 * N, D), e(2 * N, D), e(2 * N, D)
            ws.emb2, ws.semb2 = e(N, 2, D), e(N, 2, D)    # [token-replace embedding, timestep embedding] per sample
            ws.semb1 = e(N, D)
            ws.mod = e(N, 2, 6 * D)
            ws.modc = e(N, 6 * D)
            ws.mod_out = e(N, 2 * D)
            # token refiner
            ws.pool, ws.rt = e(N, cfg.text_embed_dim), e(N, D)
            ws.e, ws.en = e(N, L, D), e(N, L, D)
            ws.eqk, ws.evt, ws.ea = e(N, L, 2 * D), z(N, D, ws.L_pad), e(N, L, D)
            ws.eh = e(N, L, M)
            ws.rgate = e(N, 2 * D)
            self._ws[key] = ws
        if self.fp8_attention and not hasattr(ws, "a8"):   # e4m3 operands of the joint attention: only once the flag is on
            cfg, dev = self.config, self.device
            D, heads, J = cfg.dim, cfg.num_attention_heads, ws.J
            ws.a8 = torch.empty(N, J, 2 * D, dtype=torch.uint8, device=dev)               # Q | K, the layout of ws.qk
            ws.a8s = torch.empty(N, J, heads, dtype=torch.float32, device=dev)            # Q scales
            ws.k8s = torch.stack([Lw.k8_scale for Lw in self.dual + self.single])[:, None, :].expand(-1, N, -1).contiguous()
            ws.vt8 = torch.zeros(N, D, ws.J_pad, dtype=torch.uint8, device=dev)
            ws.vt8s = torch.empty(N, D, dtype=torch.float32, device=dev)
        if self.fp8 and not hasattr(ws, "q8"):             # e4m3 operands of the block linears: only once the flag is on
            cfg, dev = self.config, self.device
            ws.q8 = torch.empty(N * ws.J, cfg.dim + int(cfg.dim * cfg.mlp_ratio), dtype=torch.uint8, device=dev)
            ws.q8s = torch.empty(N * ((ws.J + 3) // 4 * 4), dtype=torch.float32, device=dev)
        return ws

    def _fp8_weights(self):
        """A model built in bf16 whose `fp8` attribute was set afterwards: the e4m3 weights next to the bf16 ones, made once."""
        blocks = self.dual + self.single
        if blocks and not hasattr(blocks[0], "wqk8"):
            self._check_fp8_shapes()
            for L in self.dual:
                self._quantize_block(L, self.FP8_DUAL, drop_bf16=False)
            for L in self.single:
                self._quantize_block(L, self.FP8_SINGLE, drop_bf16=False)

    def _window_ranges(self, frames, hw, valid, J, window=None):
        """The frame-window table of one sample of this video shape (HeadWindowHost._window_table: cached per (F, hw, valid, J,
        window, sink)), or None where the window is the dense attention.  Keys: frames * hw latent tokens, then `valid` prompt keys.
        window: attn_window, or one of attn_window_widths."""
        if self.fp8_attention:
            raise ValueError("attn_window does not compose with fp8_attention: the e4m3 attention kernel takes no key ranges")
        S = frames * hw
        return self._window_table(frames, hw, (valid, J), window=window, tail=(S, S + valid), rows=J)

    def _joint_attention(self, ws, plan, bi, valid, S, scale):
        """The joint attention of block bi (its index in dual + single order) from ws.qk / ws.vt into the front of ws.am's rows:
        one launch per sample over its S latent and valid[b] prompt keys -- the e4m3 kernel (fp8_attention), or what `plan` says."""
        cfg, T = self.config, self._timed
        D, heads, N, J, AM = cfg.dim, cfg.num_attention_heads, len(valid), ws.J, ws.am.shape[2]
        f8, prof = self.fp8_attention, self.profile
        if f8:   # V^T of the joint sequence (latent and prompt columns) per row, in the fp8 kernel's key order
            T("vt_quant", _lib.quantize_fp8_vt, ws.vt, ws.vt8, ws.vt8s, N, D, J, D * ws.J_pad, ws.J_pad, D * ws.J_pad, ws.J_pad)
        if prof is not None:   # one event pair around the samples' launches
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        direct = lambda name, fn, *a, **k: fn(*a, **k)
        for b in range(N):
            if f8:
                _lib.flash_attn_d128_fp8(ws.a8, ws.a8s, ws.a8, ws.k8s, ws.vt8, ws.vt8s, ws.am, 1, heads, J, S + valid[b],
                                         J * 2 * D, 2 * D, J * 2 * D, 2 * D, D * ws.J_pad, ws.J_pad, J * AM, AM, scale,
                                         q_off=b * J * 2 * D, qs_off=b * J * heads, k_off=b * J * 2 * D + D,
                                         ks_off=(bi * N + b) * heads, vt_off=b * D * ws.J_pad, vts_off=b * D, o_off=b * J * AM)
                continue
            ops = SelfAttnOperands(128, ws.qk, ws.qk, ws.vt, ws.am, 1, heads, J, S + valid[b], J * 2 * D, 2 * D, J * 2 * D, 2 * D,
                                   D * ws.J_pad, ws.J_pad, J * AM, AM, scale, q_off=b * J * 2 * D, k_off=b * J * 2 * D + D,
                                   vt_off=b * D * ws.J_pad, o_off=b * J * AM)
            if plan.far is not None:   # attn_far_reuse / attn_far_pool: near launch, (far launch,) merge of sample b
                plan.far.attention(direct, "attn_self", ops, bi, group=b, sample0=b)
            elif plan.cal is not None:   # the calibration forward: the recall over the latent queries only
                calibrate_self_attention(direct, "attn_self", ops, plan.cal, bi, N, b, (0, S), plan.full[b], plan.measure[b])
            else:
                launch_self_attention(direct, "attn_self", ops, *plan.layer(bi, b))
        if prof is not None:
            e1.record()
            prof.setdefault("attn_self", []).append((e0, e1))

    def __call__(self, hidden_states, timestep, encoder_hidden_states, encoder_attention_mask, pooled_projections,
                 guidance=None, attention_kwargs=None, return_dict=True, cache_keys=None, cache_force=False):
        """cache_keys (one hashable per sample, naming the role of its pass, as an attn_reuse.StepKeys that carries the step's
        timestep) names the samples' attention-cache entries when `attn_reuse` >= 2; cache_force computes this forward (and
        rewrites them) whatever the schedule says (the first and the last step of a schedule, a calibration forward)."""
        cfg, w, G, T = self.config, self.w, _lib.gemm, self._timed
        if hidden_states.device.type != "cuda":
            raise _lib.AlgHipError("HunyuanVideoTransformer3DModel needs device tensors; there is no CPU fallback")
        N, C, F_, H, W = hidden_states.shape
        p = cfg.patch_size
        if C != cfg.in_channels or H % p or W % p:
            raise ValueError(f"hidden_states must be [N, {cfg.in_channels}, F, H, W] with H, W divisible by {p}")
        if cfg.guidance_embeds and guidance is None:
            raise ValueError("this checkpoint has a guidance embedder: pass `guidance`")
        D, M, heads = cfg.dim, int(cfg.dim * cfg.mlp_ratio), cfg.num_attention_heads
        S, first = F_ * (H // p) * (W // p), (H // p) * (W // p)
        if S % 4:
            raise NotImplementedError("the joint [latents; text] layout needs a multiple of 4 latent tokens")
        L = encoder_hidden_states.shape[1]
        fp8 = bool(self.fp8)
        if fp8:
            self._fp8_weights()
        elif (self.dual + self.single) and (self.dual + self.single)[0].wqk is None:
            raise _lib.AlgHipError("this model was built with fp8=True and holds no bf16 copy of its block weights: build it "
                                   "with fp8=False to run (or switch between) both modes")
        ws = self._workspace(N, S, L)
        J, dev = ws.J, self.device
        tr = cfg.image_condition_type == "token_replace"
        cos, sin = self.rope_tables(F_, H, W)
        scale = 1.0 / math.sqrt(cfg.attention_head_dim)
        valid_t = encoder_attention_mask.to(device=dev).float().sum(dim=1).to(torch.int32).contiguous()
        valid = valid_t.tolist()                                   # one small D2H per forward (key lengths are host scalars)
        if min(valid) < 1:
            raise ValueError("every prompt needs at least one unmasked token")
        hs = hidden_states.to(BF).contiguous()
        txt = encoder_hidden_states.to(device=dev, dtype=BF).contiguous()
        pooled = pooled_projections.to(device=dev, dtype=BF).contiguous()
        t = timestep.to(device=dev, dtype=torch.float32).reshape(-1)
        t = (t.expand(N) if t.numel() == 1 else t).contiguous()

        def temb_of(tvals, l1, l2, out, rows):
            """Timesteps(256) -> Linear -> SiLU -> Linear for `rows` scalars -> out [rows, D]."""
            _lib.timestep_embedding(tvals, ws.tsin, rows, 256, True)
            G(ws.tsin, l1[0], ws.h1, rows, D, 256, 256, 256, D, bias=l1[1], act=_lib.ACT_SILU)
            G(ws.h1, l2[0], out, rows, D, D, D, D, D, bias=l2[1])

        # ---- conditioning: temb (and the timestep-0 "token replace" embedding) ----
        temb_of(torch.cat([torch.zeros_like(t), t]).contiguous(), w.t1, w.t2, ws.tA, 2 * N)      # rows [0..N) = t 0, [N..2N) = t
        G(pooled, w.p1[0], ws.h1, N, D, cfg.pooled_projection_dim, cfg.pooled_projection_dim, cfg.pooled_projection_dim, D,
          bias=w.p1[1], act=_lib.ACT_SILU)
        G(ws.h1, w.p2[0], ws.tB, N, D, D, D, D, D, bias=w.p2[1])                                   # pooled projection
        pooled_e = ws.tB[:N]
        emb_t = _lib.lincomb([(1.0, ws.tA[N:2 * N].contiguous()), (1.0, pooled_e.contiguous())], BF)
        if cfg.guidance_embeds:
            g_in = guidance.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            gbuf = torch.empty(N, D, dtype=BF, device=dev)
            _lib.timestep_embedding(g_in, ws.tsin, N, 256, True)
            G(ws.tsin, w.g1[0], ws.h1, N, D, 256, 256, 256, D, bias=w.g1[1], act=_lib.ACT_SILU)
            G(ws.h1, w.g2[0], gbuf, N, D, D, D, D, D, bias=w.g2[1])
            emb_t = _lib.lincomb([(1.0, emb_t), (1.0, gbuf)], BF)
        emb_tr = _lib.lincomb([(1.0, ws.tA[:N].contiguous()), (1.0, pooled_e.contiguous())], BF) if tr else emb_t
        ws.emb2[:, 0].copy_(emb_tr)
        ws.emb2[:, 1].copy_(emb_t)
        _lib.silu(ws.emb2, ws.semb2)
        _lib.silu(emb_t.contiguous(), ws.semb1)

        # ---- patch embed into the latent rows of the joint buffer ----
        _lib.patchify3d(hs, ws.patches, N, C, F_, H, W, p, p, self.k_patch)
        G(ws.patches, w.patch_w, ws.x, S, D, self.k_patch, self.k_patch, self.k_patch, D, bias=w.patch_b, batch=N,
          strideA=S * self.k_patch, strideC=J * D)

        # ---- token refiner on the prompt tokens -> text rows of the joint buffer ----
        Td = cfg.text_embed_dim
        _lib.masked_mean(txt, valid_t, ws.pool, N, L, Td)
        temb_of(t, w.r_t1, w.r_t2, ws.tA, N)
        G(ws.pool, w.r_x1[0], ws.h1, N, D, Td, Td, Td, D, bias=w.r_x1[1], act=_lib.ACT_SILU)
        G(ws.h1, w.r_x2[0], ws.tB, N, D, D, D, D, D, bias=w.r_x2[1])
        r_temb = _lib.lincomb([(1.0, ws.tA[:N].contiguous()), (1.0, ws.tB[:N].contiguous())], BF)
        _lib.silu(r_temb, ws.rt)
        G(txt, w.r_in[0], ws.e, N * L, D, Td, Td, Td, D, bias=w.r_in[1])
        n_ref = len(self.refiner)
        for li, R in enumerate(self.refiner):
            last = li == n_ref - 1
            G(ws.rt, R.ada[0], ws.rgate, N, 2 * D, D, D, D, 2 * D, bias=R.ada[1])           # gate_msa | gate_mlp
            _lib.layernorm_modulate(ws.e, ws.en, R.n1w, R.n1b, None, None, 0, N, L, D, 0, 1e-6)
            G(ws.en, R.wqk, ws.eqk, N * L, 2 * D, D, D, D, 2 * D, bias=R.bqk)
            G(R.v[0], ws.en, ws.evt, D, L, D, D, D, ws.L_pad, bias=R.v[1], batch=N, strideB=L * D, strideC=D * ws.L_pad,
              flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
            for b in range(N):
                _lib.flash_attn_d128(ws.eqk, ws.eqk, ws.evt, ws.ea, 1, heads, L, valid[b], L * 2 * D, 2 * D, L * 2 * D, 2 * D,
                                     D * ws.L_pad, ws.L_pad, L * D, D, scale, q_off=b * L * 2 * D, k_off=b * L * 2 * D + D,
                                     vt_off=b * D * ws.L_pad, o_off=b * L * D)
            G(ws.ea, R.o[0], ws.e, L, D, D, D, D, D, bias=R.o[1], R=ws.e, ldr=D, gate=ws.rgate, strideGate=2 * D,
              gate_seg_stride=0, batch=N, strideA=L * D, strideC=L * D, strideR=L * D)
            _lib.layernorm_modulate(ws.e, ws.en, R.n2w, R.n2b, None, None, 0, N, L, D, 0, 1e-6)
            G(ws.en, R.f1[0], ws.eh, N * L, M, D, D, D, M, bias=R.f1[1], act=_lib.ACT_SILU)
            # the last refiner block writes the refined prompt straight into the text rows of the joint buffer
            G(ws.eh, R.f2[0], ws.x if last else ws.e, L, D, M, M, M, D, bias=R.f2[1], R=ws.e, ldr=D, gate=ws.rgate,
              gate_off=D, strideGate=2 * D, gate_seg_stride=0, batch=N, strideA=L * M, strideC=(J if last else L) * D,
              strideR=L * D, c_off=(S * D if last else 0))
        if n_ref == 0:
            ws.x[:, S:].copy_(ws.e)

        mod_bs, seg = (12 * D, 6 * D) if tr else (6 * D, 0)
        split = first if tr else 0

        f8 = self.fp8_attention
        H8 = _lib.headnorm_rope_fp8
        kvr = [self._window_ranges(F_, first, valid[b], J) for b in range(N)] if self.attn_window else [None] * N   # None: dense
        # this forward's joint-attention launches, one group per sample: the shared window, or per-head tables chosen by recall
        plan = self._self_attn_begin(kvr, (F_, first, int(self.attn_window), int(self.attn_sink_frames)),
                                     len(self.dual) + len(self.single), N, heads, J, (N, J, D), batch=1,
                                     table_of=lambda b, w_: self._window_ranges(F_, first, valid[b], J, window=w_),
                                     profile_of=lambda b, ws_: self._profile_table(F_, first, ws_, (valid[b], J),
                                                                                   tail=(S, S + valid[b]), rows=J))
        # far-field reuse (alg_amd/attn_far.py): None -- off (or a dense step, or a window that covers the video)
        # pooled far field (alg_amd/attn_pool.py): None -- off (or a dense step, or a window that covers the video); it takes the
        # place of the far-field reuse in plan.far and refuses to run next to it
        pool = self._attn_pool_begin(kvr, N, heads, 128, J)
        plan.far = pool if pool is not None else self._attn_far_begin(cache_keys, cache_force, kvr, N,
                                                                      len(self.dual) + len(self.single), heads, 128, J)
        attention = lambda bi: self._joint_attention(ws, plan, bi, valid, S, scale)
        # attention reuse (alg_amd/attn_reuse.py): None -- off, nothing below differs from the plain forward.  An entry holds the J
        # joint rows (latents, then prompt) of every block; att_rows: their place in the front columns of ws.am, per sample
        ar = self._attn_reuse_begin(cache_keys, cache_force, N, len(self.dual) + len(self.single), J, D)
        reuse = ar is not None and ar.reuse
        att_rows = [ws.am[n, :, :D] for n in range(N)] if ar is not None else None

        def ada(lin_, rows_in, out, n_out, two):
            """AdaLN linear on silu(emb): `two` -> both embeddings of every sample ([N][2][n_out]), else temb only."""
            G(rows_in, lin_[0], out, (2 * N if two else N), n_out, D, D, D, n_out, bias=lin_[1])

        AM = D + M
        if fp8:
            # e4m3 operands (self.fp8): every quantised linear reads ws.q8 / ws.q8s, filled in front of it by the norm itself or by
            # the quantiser.  The scales of a batch item start at a multiple of 4 floats (the V^T GEMM reads them as B scales, 16
            # bytes at a time): rows % 4 == 0 (the latent rows always; the joint rows of the published shapes) -> the rows of all
            # items are contiguous and one launch covers them, otherwise one launch per item.
            q8, q8s = ws.q8, ws.q8s
            items_of = lambda rows: ((0, N),) if rows % 4 == 0 else tuple((n, 1) for n in range(N))
            s4 = lambda rows: (rows + 3) // 4 * 4

            def norm8(rows, mod_t, mbs, sg, sc_off, sh_off):
                """LayerNorm + modulation of rows [0, rows) of every item of ws.x -> e4m3 rows [N * rows, D] + scales"""
                for n0, nb in items_of(rows):
                    T("ln_mod", _lib.layernorm_modulate_seg_fp8, ws.x, q8, q8s, None, None, mod_t, mod_t, mbs, sg, nb, rows, D, split,
                      1e-6, x_bstride=J * D, x_off=n0 * J * D, scale_off=n0 * mbs + sc_off, shift_off=n0 * mbs + sh_off,
                      q8_off=n0 * rows * D, q8_scale_off=n0 * s4(rows))

            def quant8(rows, K_, col):
                """columns [col, col + K_) of rows [0, rows) of every item of ws.am -> e4m3 rows [N * rows, K_] + scales"""
                for n0, nb in items_of(rows):
                    T("quant", _lib.quantize_fp8_rows_batched, ws.am, q8, q8s, nb, rows, K_, J * AM, AM, x_off=n0 * J * AM + col,
                      q_off=n0 * rows * K_, scale_off=n0 * s4(rows))

            def lin8(name, w8, C, rows, n_out, K_, ldc, **kw):
                """C[n] = epilogue(q8[n] @ W^T) per batch item: A = the e4m3 tokens, rows of K_ bytes"""
                T(name, G, q8, w8[0], C, rows, n_out, K_, K_, K_, ldc, a_scale=q8s, b_scale=w8[1], batch=N, strideA=rows * K_,
                  strideAScale=s4(rows), **kw)

            def vt8(w8, bias, rows):
                """V^T of rows [0, rows): the weight is the A operand, the (already quantised) tokens are B"""
                T("gemm_vt", G, w8[0], q8, ws.vt, D, rows, D, D, D, ws.J_pad, a_scale=w8[1], b_scale=q8s, strideBScale=s4(rows),
                  bias=bias, batch=N, strideB=rows * D, strideC=D * ws.J_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)

        # ---- dual-stream blocks: latent rows [0, S) and text rows [S, J) of the joint buffer ----
        use_packed = self.packed_weights and os.environ.get("ALG_GEMM_PIPE", "10") == "10"
        PK = lambda Lw_, t: (Lw_.packed.get(id(t)) or t) if use_packed else t     # the packed copy of a block's weight, if it has one
        for bi, Lw in enumerate(self.dual):
            ada(Lw.ada, ws.semb2 if tr else ws.semb1, ws.mod, 6 * D, tr)     # [N][2][6D] (token replace) or [N][6D]
            mv = ws.mod
            ada(Lw.ada_c, ws.semb1, ws.modc, 6 * D, False)
            # shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp at +0, +D, ... of every 6D vector
            if reuse:   # attn_reuse: the cached joint rows stand in for both streams' norm1, projections, head norms and the attention
                T("attn_reuse", ar.load, bi, att_rows)
            else:
                if fp8:
                    norm8(S, mv, mod_bs, seg, D, 0)
                else:
                    T("ln_mod", _lib.layernorm_modulate_seg, ws.x, ws.y, None, None, mv, mv, mod_bs, seg, N, S, D, split, 1e-6,
                      x_bstride=J * D, y_bstride=J * D, scale_off=D, shift_off=0)
                _lib.layernorm_modulate_seg(ws.x, ws.y, None, None, ws.modc, ws.modc, 6 * D, 0, N, L, D, 0, 1e-6,
                                            x_bstride=J * D, y_bstride=J * D, x_off=S * D, y_off=S * D, scale_off=D, shift_off=0)
                if fp8:
                    lin8("gemm_qk", Lw.wqk8, ws.qk, S, 2 * D, D, 2 * D, bias=Lw.bqk, strideC=J * 2 * D)
                else:
                    T("gemm_qk", G, ws.y, PK(Lw, Lw.wqk), ws.qk, S, 2 * D, D, D, D, 2 * D, bias=Lw.bqk, batch=N, strideA=J * D, strideC=J * 2 * D)
                G(ws.y, Lw.wqk_c, ws.qk, L, 2 * D, D, D, D, 2 * D, bias=Lw.bqk_c, batch=N, strideA=J * D, strideC=J * 2 * D,
                  a_off=S * D, c_off=S * 2 * D)
                if fp8:
                    vt8(Lw.v8, Lw.v[1], S)
                else:
                    T("gemm_vt", G, Lw.v[0], ws.y, ws.vt, D, S, D, D, D, ws.J_pad, bias=Lw.v[1], batch=N, strideB=J * D,
                      strideC=D * ws.J_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
                G(Lw.v_c[0], ws.y, ws.vt, D, L, D, D, D, ws.J_pad, bias=Lw.v_c[1], batch=N, strideB=J * D,
                  strideC=D * ws.J_pad, b_off=S * D, perm_col0=S, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
                # latent rows: norm_q / norm_k + rope; prompt rows: norm_added_q / norm_added_k, no rope
                if f8:   # the same four norms, writing e4m3 Q | K (and the Q scales) instead of updating ws.qk
                    qkb, sb, hs = J * 2 * D, J * heads, bi * N * heads
                    T("headnorm_rope", H8, ws.qk, Lw.nq, cos, sin, 2 * D, qkb, N, S, heads, S, 1e-6, ws.a8, 2 * D, qkb, scale=ws.a8s,
                      scale_bstride=sb)
                    T("headnorm_rope", H8, ws.qk, Lw.nk, cos, sin, 2 * D, qkb, N, S, heads, S, 1e-6, ws.a8, 2 * D, qkb, head_scale=ws.k8s,
                      hs_off=hs, x_off=D, q8_off=D)
                    H8(ws.qk, Lw.nq_c, None, None, 2 * D, qkb, N, L, heads, 0, 1e-6, ws.a8, 2 * D, qkb, scale=ws.a8s, scale_bstride=sb,
                       x_off=S * 2 * D, q8_off=S * 2 * D, scale_off=S * heads)
                    H8(ws.qk, Lw.nk_c, None, None, 2 * D, qkb, N, L, heads, 0, 1e-6, ws.a8, 2 * D, qkb, head_scale=ws.k8s, hs_off=hs,
                       x_off=S * 2 * D + D, q8_off=S * 2 * D + D)
                else:
                    T("headnorm_rope", _lib.headnorm_rope_, ws.qk, Lw.nq, cos, sin, 2 * D, J * 2 * D, N, S, heads, S, 1e-6)
                    T("headnorm_rope", _lib.headnorm_rope_, ws.qk, Lw.nk, cos, sin, 2 * D, J * 2 * D, N, S, heads, S, 1e-6, x_off=D)
                    _lib.headnorm_rope_(ws.qk, Lw.nq_c, None, None, 2 * D, J * 2 * D, N, L, heads, 0, 1e-6, x_off=S * 2 * D)
                    _lib.headnorm_rope_(ws.qk, Lw.nk_c, None, None, 2 * D, J * 2 * D, N, L, heads, 0, 1e-6, x_off=S * 2 * D + D)
                attention(bi)
                if ar is not None:
                    T("attn_reuse", ar.store, bi, att_rows)
            if fp8:
                quant8(S, D, 0)
                lin8("gemm_out", Lw.o8, ws.x, S, D, D, D, bias=Lw.o[1], R=ws.x, ldr=D, gate=mv, gate_off=2 * D, strideGate=mod_bs,
                     gate_seg_stride=seg, seg_split=split, strideC=J * D, strideR=J * D)
            else:
                T("gemm_out", G, ws.am, PK(Lw, Lw.o[0]), ws.x, S, D, D, AM, D, D, bias=Lw.o[1], R=ws.x, ldr=D, gate=mv, gate_off=2 * D,
                  strideGate=mod_bs, gate_seg_stride=seg, seg_split=split, batch=N, strideA=J * AM, strideC=J * D, strideR=J * D)
            G(ws.am, Lw.o_c[0], ws.x, L, D, D, AM, D, D, bias=Lw.o_c[1], R=ws.x, ldr=D, gate=ws.modc, gate_off=2 * D,
              strideGate=6 * D, gate_seg_stride=0, batch=N, strideA=J * AM, strideC=J * D, strideR=J * D, a_off=S * AM,
              c_off=S * D, r_off=S * D)
            if fp8:
                norm8(S, mv, mod_bs, seg, 4 * D, 3 * D)
            else:
                T("ln_mod", _lib.layernorm_modulate_seg, ws.x, ws.y, None, None, mv, mv, mod_bs, seg, N, S, D, split, 1e-6,
                  x_bstride=J * D, y_bstride=J * D, scale_off=4 * D, shift_off=3 * D)
            _lib.layernorm_modulate_seg(ws.x, ws.y, None, None, ws.modc, ws.modc, 6 * D, 0, N, L, D, 0, 1e-6,
                                        x_bstride=J * D, y_bstride=J * D, x_off=S * D, y_off=S * D, scale_off=4 * D,
                                        shift_off=3 * D)
            if fp8:
                lin8("gemm_ff1", Lw.f18, ws.am, S, M, D, AM, bias=Lw.f1[1], act=_lib.ACT_GELU_TANH, strideC=J * AM, c_off=D)
            else:
                T("gemm_ff1", G, ws.y, PK(Lw, Lw.f1[0]), ws.am, S, M, D, D, D, AM, bias=Lw.f1[1], act=_lib.ACT_GELU_TANH, batch=N,
                  strideA=J * D, strideC=J * AM, c_off=D)
            G(ws.y, Lw.f1_c[0], ws.am, L, M, D, D, D, AM, bias=Lw.f1_c[1], act=_lib.ACT_GELU_TANH, batch=N, strideA=J * D,
              strideC=J * AM, a_off=S * D, c_off=S * AM + D)
            if fp8:
                quant8(S, M, D)
                lin8("gemm_ff2", Lw.f28, ws.x, S, D, M, D, bias=Lw.f2[1], R=ws.x, ldr=D, gate=mv, gate_off=5 * D, strideGate=mod_bs,
                     gate_seg_stride=seg, seg_split=split, strideC=J * D, strideR=J * D)
            else:
                T("gemm_ff2", G, ws.am, PK(Lw, Lw.f2[0]), ws.x, S, D, M, AM, M, D, bias=Lw.f2[1], R=ws.x, ldr=D, gate=mv, gate_off=5 * D,
                  strideGate=mod_bs, gate_seg_stride=seg, seg_split=split, batch=N, strideA=J * AM, strideC=J * D, strideR=J * D,
                  a_off=D)
            G(ws.am, Lw.f2_c[0], ws.x, L, D, M, AM, M, D, bias=Lw.f2_c[1], R=ws.x, ldr=D, gate=ws.modc, gate_off=5 * D,
              strideGate=6 * D, gate_seg_stride=0, batch=N, strideA=J * AM, strideC=J * D, strideR=J * D, a_off=S * AM + D,
              c_off=S * D, r_off=S * D)

        # ---- single-stream blocks, in place on the joint buffer ----
        smod_bs, sseg = (6 * D, 3 * D) if tr else (3 * D, 0)
        for bi, Lw in enumerate(self.single, start=len(self.dual)):
            if tr:
                G(ws.semb2, Lw.ada[0], ws.mod, 2 * N, 3 * D, D, D, D, 3 * D, bias=Lw.ada[1])       # [N][2][3D]: shift, scale, gate
            else:
                G(ws.semb1, Lw.ada[0], ws.mod, N, 3 * D, D, D, D, 3 * D, bias=Lw.ada[1])
            if fp8:   # one norm over the joint rows feeds proj_mlp, Q|K and V^T
                norm8(J, ws.mod, smod_bs, sseg, D, 0)
                lin8("gemm_ff1", Lw.mlp8, ws.am, J, M, D, AM, bias=Lw.mlp[1], act=_lib.ACT_GELU_TANH, strideC=J * AM, c_off=D)
                if not reuse:
                    lin8("gemm_qk", Lw.wqk8, ws.qk, J, 2 * D, D, 2 * D, bias=Lw.bqk, strideC=J * 2 * D)
                    vt8(Lw.v8, Lw.v[1], J)
            else:
                T("ln_mod", _lib.layernorm_modulate_seg, ws.x, ws.y, None, None, ws.mod, ws.mod, smod_bs, sseg, N, J, D, split, 1e-6,
                  scale_off=D, shift_off=0)
                T("gemm_ff1", G, ws.y, PK(Lw, Lw.mlp[0]), ws.am, N * J, M, D, D, D, AM, bias=Lw.mlp[1], act=_lib.ACT_GELU_TANH, c_off=D)
                if not reuse:
                    T("gemm_qk", G, ws.y, PK(Lw, Lw.wqk), ws.qk, N * J, 2 * D, D, D, D, 2 * D, bias=Lw.bqk)
                    T("gemm_vt", G, Lw.v[0], ws.y, ws.vt, D, J, D, D, D, ws.J_pad, bias=Lw.v[1], batch=N, strideB=J * D,
                      strideC=D * ws.J_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
            if reuse:   # attn_reuse: the cached attention columns go in front of gelu(mlp) in the [attention | gelu(mlp)] buffer
                T("attn_reuse", ar.load, bi, att_rows)
            else:
                if f8:
                    T("headnorm_rope", H8, ws.qk, Lw.nq, cos, sin, 2 * D, J * 2 * D, N, J, heads, S, 1e-6, ws.a8, 2 * D, J * 2 * D,
                      scale=ws.a8s, scale_bstride=J * heads)
                    T("headnorm_rope", H8, ws.qk, Lw.nk, cos, sin, 2 * D, J * 2 * D, N, J, heads, S, 1e-6, ws.a8, 2 * D, J * 2 * D,
                      head_scale=ws.k8s, hs_off=bi * N * heads, x_off=D, q8_off=D)
                else:
                    T("headnorm_rope", _lib.headnorm_rope_, ws.qk, Lw.nq, cos, sin, 2 * D, J * 2 * D, N, J, heads, S, 1e-6)
                    T("headnorm_rope", _lib.headnorm_rope_, ws.qk, Lw.nk, cos, sin, 2 * D, J * 2 * D, N, J, heads, S, 1e-6, x_off=D)
                attention(bi)
                if ar is not None:
                    T("attn_reuse", ar.store, bi, att_rows)
            if fp8:   # the whole [attention | gelu(mlp)] row, ONE scale per token
                quant8(J, AM, 0)
                lin8("gemm_out_mlp", Lw.out8, ws.x, J, D, AM, D, bias=Lw.out[1], R=ws.x, ldr=D, gate=ws.mod, gate_off=2 * D,
                     strideGate=smod_bs, gate_seg_stride=sseg, seg_split=split, strideC=J * D, strideR=J * D)
            else:
                T("gemm_out_mlp", G, ws.am, PK(Lw, Lw.out[0]), ws.x, J, D, AM, AM, AM, D, bias=Lw.out[1], R=ws.x, ldr=D, gate=ws.mod, gate_off=2 * D,
                  strideGate=smod_bs, gate_seg_stride=sseg, seg_split=split, batch=N, strideA=J * AM, strideC=J * D,
                  strideR=J * D)

        plan.finish()
        if ar is not None:
            ar.finish()

        # ---- output head: AdaLayerNormContinuous (scale | shift), projection, unpatchify ----
        G(ws.semb1, w.ada_out[0], ws.mod_out, N, 2 * D, D, D, D, 2 * D, bias=w.ada_out[1])
        _lib.layernorm_modulate_seg(ws.x, ws.y, None, None, ws.mod_out, ws.mod_out, 2 * D, 0, N, S, D, 0, 1e-6,
                                    x_bstride=J * D, y_bstride=J * D, scale_off=0, shift_off=D)
        n_out = w.out[0].shape[0]
        G(ws.y, w.out[0], ws.tok, S, n_out, D, D, D, n_out, bias=w.out[1], batch=N, strideA=J * D, strideC=S * n_out)
        out = torch.empty(N, cfg.out_channels, F_, H, W, dtype=BF, device=dev)
        _lib.unpatchify3d(ws.tok, n_out, out, N, cfg.out_channels, F_, H, W, p, p, channel_major=True)
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
