"""Wan 2.1 image-to-video DiT forward, MI355X-native.

Drop-in for the component the reference's Wan sampler calls at pipeline_wan_image2video_lowpass.py:910-917
(``transformer(hidden_states=, timestep=, encoder_hidden_states=, encoder_hidden_states_image=, attention_kwargs=,
return_dict=False)[0]``) and reads ``.dtype`` (wan:799) and ``.config.patch_size`` (wan:550) from.  The arithmetic follows
diffusers' WanTransformer3DModel (diffusers @ be2fb77, not in the reference tree -- parity unpinned, see
oracle/wan_oracle.py); state-dict names are diffusers', so a local checkpoint loads 1:1.

The forward is nothing but launch order over the C ABI of libalg_hip.so:
    alg_patchify3d -> alg_gemm_bf16 (patch embed) ; alg_timestep_embedding_f32 -> alg_linear_f32 x2 (fp32 time embedder)
    -> alg_gemm_bf16 (time_proj) -> alg_wan_modulation (scale_shift_table + temb for all 40 blocks in one launch)
    text / image embedders: alg_gemm_bf16 (+GELU-tanh), alg_layernorm_mod_f32, alg_gelu_erf
    per block:  alg_layernorm_mod_f32 -> alg_gemm_bf16 (fused QK; V written transposed + permuted) -> alg_rmsnorm_rope x2
                -> alg_flash_attn_d128 -> alg_gemm_bf16 (out proj, fp32-gate residual epilogue)
                (fp8_attention: alg_rmsnorm_rope_fp8 x2 + alg_quantize_fp8_vt -> alg_flash_attn_d128_fp8 in their place)
                alg_layernorm_mod_f32 -> q GEMM + rmsnorm ; text / image K (GEMM + rmsnorm) and V^T (GEMM)
                -> alg_flash_attn_d128 x2 -> alg_lincomb (text + image) -> alg_gemm_bf16 (out proj + residual)
                alg_layernorm_mod_f32 -> alg_gemm_bf16 (GELU-tanh) -> alg_gemm_bf16 (fp32-gate residual)
    alg_layernorm_mod_f32 -> alg_gemm_bf16 (proj_out) -> alg_unpatchify3d
PyTorch owns device memory and the stream only; there is no CPU fallback.
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
from .attn_window import HeadWindowHost, SelfAttnOperands, calibrate_self_attention, launch_self_attention, position_band_ranges
from .attn_far import AttnFarHost
from .attn_pool import AttnPoolHost
from .attn_reuse import AttnReuseHost
from .cfg_reuse import CfgReuseHost
from .step_cache import StepCacheHost

BF = torch.bfloat16


@dataclass
class WanTransformerConfig:
    patch_size: tuple = (1, 2, 2)
    num_attention_heads: int = 40
    attention_head_dim: int = 128
    in_channels: int = 36
    out_channels: int = 16
    text_dim: int = 4096
    freq_dim: int = 256
    ffn_dim: int = 13824
    num_layers: int = 40
    cross_attn_norm: bool = True
    qk_norm: str = "rms_norm_across_heads"
    eps: float = 1e-6
    image_dim: int = 1280
    added_kv_proj_dim: int = 5120
    rope_max_seq_len: int = 1024
    pos_embed_seq_len: int = None

    @property
    def dim(self):
        return self.num_attention_heads * self.attention_head_dim

    def to_dict(self):
        return asdict(self)


def parameter_shapes(cfg):
    """diffusers state-dict name -> (shape, dtype kept after from_pretrained(torch_dtype=bf16))."""
    D, Ff = cfg.dim, cfg.ffn_dim
    pt, ph, pw = cfg.patch_size
    f32 = torch.float32
    s = {"patch_embedding.weight": ((D, cfg.in_channels, pt, ph, pw), BF), "patch_embedding.bias": ((D,), BF)}
    ce = "condition_embedder."
    s[ce + "time_embedder.linear_1.weight"] = ((D, cfg.freq_dim), f32)
    s[ce + "time_embedder.linear_1.bias"] = ((D,), f32)
    s[ce + "time_embedder.linear_2.weight"] = ((D, D), f32)
    s[ce + "time_embedder.linear_2.bias"] = ((D,), f32)
    for n, shp in (("time_proj", (6 * D, D)), ("text_embedder.linear_1", (D, cfg.text_dim)),
                   ("text_embedder.linear_2", (D, D))):
        s[ce + n + ".weight"] = (shp, BF)
        s[ce + n + ".bias"] = ((shp[0],), BF)
    if cfg.image_dim is not None:
        I = cfg.image_dim
        for n, shp in (("image_embedder.ff.net.0.proj", (I, I)), ("image_embedder.ff.net.2", (D, I))):
            s[ce + n + ".weight"] = (shp, BF)
            s[ce + n + ".bias"] = ((shp[0],), BF)
        for n, d in (("image_embedder.norm1", I), ("image_embedder.norm2", D)):
            s[ce + n + ".weight"] = ((d,), BF)
            s[ce + n + ".bias"] = ((d,), BF)
        if cfg.pos_embed_seq_len is not None:   # first-last-frame checkpoints (FLF2V): learned position embedding of the 2 x 257 image tokens
            s[ce + "image_embedder.pos_embed"] = ((1, cfg.pos_embed_seq_len, I), BF)
    for l in range(cfg.num_layers):
        b = f"blocks.{l}."
        s[b + "scale_shift_table"] = ((1, 6, D), f32)
        for a in ("attn1", "attn2"):
            names = ["to_q", "to_k", "to_v", "to_out.0"]
            if a == "attn2" and cfg.added_kv_proj_dim is not None:
                names += ["add_k_proj", "add_v_proj"]
            for n in names:
                s[b + f"{a}.{n}.weight"] = ((D, D), BF)
                s[b + f"{a}.{n}.bias"] = ((D,), BF)
            s[b + f"{a}.norm_q.weight"] = ((D,), BF)
            s[b + f"{a}.norm_k.weight"] = ((D,), BF)
            if a == "attn2" and cfg.added_kv_proj_dim is not None:
                s[b + f"{a}.norm_added_k.weight"] = ((D,), BF)
        if cfg.cross_attn_norm:
            s[b + "norm2.weight"] = ((D,), f32)
            s[b + "norm2.bias"] = ((D,), f32)
        s[b + "ffn.net.0.proj.weight"] = ((Ff, D), BF)
        s[b + "ffn.net.0.proj.bias"] = ((Ff,), BF)
        s[b + "ffn.net.2.weight"] = ((D, Ff), BF)
        s[b + "ffn.net.2.bias"] = ((D,), BF)
    s["scale_shift_table"] = ((1, 2, D), f32)
    n_out = cfg.out_channels * pt * ph * pw
    s["proj_out.weight"] = ((n_out, D), BF)
    s["proj_out.bias"] = ((n_out,), BF)
    return s


def synthetic_state_dict(cfg, seed=1234, device="cuda"):
    """Seeded synthetic weights at the configured shapes (no network here): 1/sqrt(fan_in) matrices, small biases,
    gains around 1, generated on the device tensor by tensor."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for name, (shape, dt) in parameter_shapes(cfg).items():
        r = lambda: torch.randn(shape, generator=g, device=dev, dtype=torch.float32)
        if "scale_shift_table" in name:
            t = r() / shape[-1] ** 0.5
        elif name.endswith("weight") and len(shape) == 1:
            t = 1.0 + 0.1 * r()
        elif name.endswith("bias"):
            t = 0.02 * r()
        elif name.endswith("pos_embed"):
            t = 0.5 * r()
        else:
            t = r() / math.prod(shape[1:]) ** 0.5
        sd[name] = t.to(dt)
    return sd


def k_scale_bound(norm_weight, norm_dim, heads, rope):
    """The K scale of alg_flash_attn_d128_fp8 is one number per (batch, head), and the norm pass that writes K as e4m3 has to
    know it before it has seen a token.  RMSNorm bounds its output whatever the input: |x_i| * rsqrt(mean(x^2) + eps) <=
    sqrt(norm_dim), times |w_i|, times sqrt(2) when RoPE rotates a pair -- so  1.02 * sqrt(norm_dim [* 2]) * max_head |w| / 448
    (2 % for the two bf16 roundings on the way) is a scale under which no key can leave the e4m3 range.  It is 10-100 x the
    scale a measured amax would give; e4m3 is a floating-point format, so that costs range, not precision: keys down to 2^-6 of
    the bound / 448 keep their three mantissa bits (docs/numerics.md).  norm_weight: [heads * 128] (norm across heads) or [128]
    (per-head norm, shared by all heads).  Returns float32 [heads]."""
    w = norm_weight.float().abs().reshape(-1, 128).amax(dim=1)
    if w.numel() == 1:
        w = w.expand(heads)
    return (w * (1.02 * math.sqrt(norm_dim * (2.0 if rope else 1.0)) / 448.0)).contiguous()


class WanTransformer3DModel(StepCacheHost, AttnReuseHost, AttnFarHost, AttnPoolHost, CfgReuseHost, HeadWindowHost):
    dtype = BF
    # what lora.merge_into did to the state dict this model was built from (from_pretrained / from_synthetic(lora=...)): a tuple
    # of lora.LoraReport(name, scale, targets, ranks) per adapter; () without LoRA
    lora_report = ()

    def __init__(self, config: WanTransformerConfig, weights: dict, device="cuda", fp8=False, fp8_attention=False):
        """``fp8=True`` (BASELINE config 5): the seven large linears of every block run on the fp8 MFMA -- weights are
        quantised once to OCP e4m3 with one scale per output channel, activations per token right before each GEMM
        (alg_quantize_fp8_rows); norms, attention, embedders and the residual stream stay bf16 / fp32.

        ``fp8_attention=True`` (opt-in, independent of ``fp8``, may be flipped between calls): the self-attention of every
        block runs on alg_flash_attn_d128_fp8 -- the RMSNorm + RoPE pass writes Q (one scale per token and head) and K (one
        scale per head: ``k_scale_bound``) as e4m3 itself, V^T is quantised per row behind its GEMM.  Cross-attention stays
        bf16.  Off, the forward is the bf16 one bit for bit."""
        self.fp8 = bool(fp8)
        self.fp8_attention = bool(fp8_attention)
        self.pair_qkv = True     # bf16: Q|K and V^T projections of a block as one alg_gemm_bf16_pair launch (bit-identical)
        self.dual_cross = True   # I2V: text + image cross-attention of a block as one alg_flash_attn_d128_dual launch (bit-identical to two launches + add)
        self.fuse_quant = True   # fp8: the modulated LayerNorm writes the e4m3 tokens + row scales itself (bit-identical to the quantiser pass)
        # bf16: the five weight-times-token linears of a block outside the Q|K / V^T pair (out, cross q, cross out, ff1, ff2) keep a copy
        # packed in MFMA-fragment order (alg_pack_b_p11) and run GEMM schedule 11 (bit-identical to schedule 10); False, or
        # ALG_GEMM_PIPE set to another schedule than 10: the row-major weights
        self.packed_weights = True
        # > 0 (opt-in, an extension: alg_amd/step_cache.py): a forward that is handed `cache_keys` probes block 0's residual and,
        # while it moved by less than this fraction since the last forward, replaces blocks 1 .. L-1 by the residual they produced
        # on the last computed forward.  0.0: every forward is the plain one, launch for launch.
        self.step_cache = 0.0
        self.step_cache_max_consecutive = 0   # at most this many skipped forwards in a row (0: no cap)
        # N >= 2 (opt-in, an extension: alg_amd/attn_reuse.py): a forward that is handed `cache_keys` with the step's timestep
        # (attn_reuse.step_keys) computes every block's SELF-attention on every N-th step while attn_reuse_t_lo < t < attn_reuse_t_hi
        # and reads it back from a per-key cache on the steps between, skipping the first ln_mod, Q|K / V^T, both rms_rope and attn1 in
        # whatever form it runs; the cross-attention and the feed-forward run as ever.  0: every forward is the plain one, launch
        # for launch, nothing allocated.  attn_reuse_drift: the diagnostic (AttnReuseHost)
        self.attn_reuse = 0
        # N >= 2 (opt-in, an extension: alg_amd/attn_far.py; needs attn_window > 0): the keys inside the frame window are attended
        # to fresh on every step, the keys outside it on every N-th step while attn_far_reuse_t_lo < t < attn_far_reuse_t_hi and
        # from the cached partial (output and LSE) on the steps between, merged by alg_attn_merge_lse.  0: nothing differs
        self.attn_far_reuse = 0
        # G in {2, 4, 8} (opt-in, an extension: alg_amd/attn_pool.py; needs attn_window > 0): the keys outside the frame window are
        # attended to on every step as groups of G consecutive keys pooled into one (mean k, mean v, a score bias of log2 G), merged
        # with the window's partial by alg_attn_merge_lse_shift.  No state across steps.  0: nothing differs
        self.attn_far_pool = 0
        # > 0 (opt-in, an extension: alg_amd/attn_window.py; may be flipped between calls): the self-attention of every block
        # attends to the conditioning frames (attn_sink_frames) and to the latent frames within attn_window of the query block's
        # own, as ONE alg_flash_attn_d128_ranges launch for the whole batch.  0: today's launches, nothing allocated
        self.attn_window = 0
        self.attn_sink_frames = 1
        # attn_window_recall > 0 (opt-in, with attn_window > 0): only the heads whose measured recall reaches it keep the window
        # (attn_window.HeadWindowHost: attn_window_stats, reset_attn_window_heads).  0.0: the shared window, nothing allocated
        self._head_window_init()
        # attn_band > 0 (opt-in, with attn_window > 0 and attn_window_recall > 0; Wan only): a third candidate per head, the BAND -- the
        # same and the `attn_band` neighbouring spatial positions in every frame -- measured on the calibration forward like the
        # window; a head that chose it runs on position-major copies of its Q, K and V^T (alg_attn_rows_position_major,
        # alg_attn_vt_position_major), where those keys are one run per query block.  0: nothing allocated, launched or recorded
        self.attn_band = 0
        self._band_ws = None      # position-major scratch, allocated on the calibration forward and kept
        if config.qk_norm != "rms_norm_across_heads" or config.attention_head_dim != 128:
            raise NotImplementedError("the Wan DiT path is built for rms_norm_across_heads and head_dim 128")
        if tuple(config.patch_size)[0] != 1:
            raise NotImplementedError("temporal patch size 1 only (every Wan 2.1 checkpoint)")
        if config.pos_embed_seq_len is not None and config.image_dim is None:
            raise ValueError("pos_embed_seq_len (FLF2V) needs an image embedder (image_dim)")
        self.config = config
        self.device = torch.device(device)
        dev = self.device
        if dev.type != "cuda":
            raise _lib.AlgHipError("WanTransformer3DModel runs on the GPU only (HIP kernels); there is no CPU fallback")
        _lib.load_library()
        missing = [k for k in parameter_shapes(config) if k not in weights]
        if missing:
            raise KeyError("state dict is missing %d tensors, e.g. %s" % (len(missing), missing[:3]))
        D = config.dim
        bf = lambda n: weights[n].to(device=dev, dtype=BF).contiguous()
        f32 = lambda n: weights[n].to(device=dev, dtype=torch.float32).contiguous()
        w = SimpleNamespace()
        # patch embed: Conv3d weight [D, C, 1, ph, pw] -> [D, Kpad] rows (c, py, px), zero padded to K % 64 == 0
        kin = config.in_channels * config.patch_size[1] * config.patch_size[2]
        self.k_patch = (kin + 63) // 64 * 64
        wp = torch.zeros(D, self.k_patch, dtype=BF, device=dev)
        wp[:, :kin] = bf("patch_embedding.weight").reshape(D, kin)
        w.patch_w, w.patch_b = wp, bf("patch_embedding.bias")
        ce = "condition_embedder."
        w.t1_w, w.t1_b = f32(ce + "time_embedder.linear_1.weight"), f32(ce + "time_embedder.linear_1.bias")
        w.t2_w, w.t2_b = f32(ce + "time_embedder.linear_2.weight"), f32(ce + "time_embedder.linear_2.bias")
        w.tp_w, w.tp_b = bf(ce + "time_proj.weight"), bf(ce + "time_proj.bias")
        w.x1_w, w.x1_b = bf(ce + "text_embedder.linear_1.weight"), bf(ce + "text_embedder.linear_1.bias")
        w.x2_w, w.x2_b = bf(ce + "text_embedder.linear_2.weight"), bf(ce + "text_embedder.linear_2.bias")
        self.has_image = config.image_dim is not None
        if self.has_image:
            ie = ce + "image_embedder."
            w.in1_w, w.in1_b = f32(ie + "norm1.weight"), f32(ie + "norm1.bias")   # FP32LayerNorm: weight.float()
            w.in2_w, w.in2_b = f32(ie + "norm2.weight"), f32(ie + "norm2.bias")
            w.if1_w, w.if1_b = bf(ie + "ff.net.0.proj.weight"), bf(ie + "ff.net.0.proj.bias")
            w.if2_w, w.if2_b = bf(ie + "ff.net.2.weight"), bf(ie + "ff.net.2.bias")
            # FLF2V (wan:805-812 hands [first, last] CLIP embeddings as 2 x 257 tokens): WanImageEmbedding.pos_embed [1, 514, I]
            w.img_pos = bf(ie + "pos_embed").reshape(-1, config.image_dim) if config.pos_embed_seq_len is not None else None
        w.tables = torch.stack([f32(f"blocks.{l}.scale_shift_table").reshape(6, D)
                                for l in range(config.num_layers)]).contiguous()      # [L, 6, D]
        w.table_out = f32("scale_shift_table").reshape(1, 2, D).contiguous()
        w.out_w, w.out_b = bf("proj_out.weight"), bf("proj_out.bias")
        self.blocks = []
        for l in range(config.num_layers):
            b = f"blocks.{l}."
            L = SimpleNamespace()
            L.wqk = torch.cat([bf(b + "attn1.to_q.weight"), bf(b + "attn1.to_k.weight")], dim=0).contiguous()
            L.bqk = torch.cat([bf(b + "attn1.to_q.bias"), bf(b + "attn1.to_k.bias")]).contiguous()
            L.wv, L.bv = bf(b + "attn1.to_v.weight"), bf(b + "attn1.to_v.bias")
            L.wo, L.bo = bf(b + "attn1.to_out.0.weight"), bf(b + "attn1.to_out.0.bias")
            L.nq, L.nk = bf(b + "attn1.norm_q.weight"), bf(b + "attn1.norm_k.weight")
            L.k8_scale = k_scale_bound(L.nk, D, config.num_attention_heads, rope=True)    # [heads] fp32 (fp8_attention)
            L.n2w = f32(b + "norm2.weight") if config.cross_attn_norm else None
            L.n2b = f32(b + "norm2.bias") if config.cross_attn_norm else None
            L.cq_w, L.cq_b = bf(b + "attn2.to_q.weight"), bf(b + "attn2.to_q.bias")
            L.ck_w, L.ck_b = bf(b + "attn2.to_k.weight"), bf(b + "attn2.to_k.bias")
            L.cv_w, L.cv_b = bf(b + "attn2.to_v.weight"), bf(b + "attn2.to_v.bias")
            L.co_w, L.co_b = bf(b + "attn2.to_out.0.weight"), bf(b + "attn2.to_out.0.bias")
            L.cnq, L.cnk = bf(b + "attn2.norm_q.weight"), bf(b + "attn2.norm_k.weight")
            if config.added_kv_proj_dim is not None:
                L.ak_w, L.ak_b = bf(b + "attn2.add_k_proj.weight"), bf(b + "attn2.add_k_proj.bias")
                L.av_w, L.av_b = bf(b + "attn2.add_v_proj.weight"), bf(b + "attn2.add_v_proj.bias")
                L.cnak = bf(b + "attn2.norm_added_k.weight")
            L.f1_w, L.f1_b = bf(b + "ffn.net.0.proj.weight"), bf(b + "ffn.net.0.proj.bias")
            L.f2_w, L.f2_b = bf(b + "ffn.net.2.weight"), bf(b + "ffn.net.2.bias")
            if self.fp8:
                for name in ("wqk", "wv", "wo", "cq_w", "co_w", "f1_w", "f2_w"):
                    wt = getattr(L, name)
                    q = torch.empty(wt.shape, dtype=torch.uint8, device=dev)
                    sc = torch.empty(wt.shape[0], dtype=torch.float32, device=dev)
                    _lib.quantize_fp8_rows(wt, q, sc, wt.shape[0], wt.shape[1])
                    setattr(L, name, (q, sc))          # the bf16 copy is dropped: half the weight memory
            else:
                L.packed = {name: _lib.PackedB(getattr(L, name)) for name in ("wo", "cq_w", "co_w", "f1_w", "f2_w")}
            self.blocks.append(L)
        self.w = w
        self._ws = {}
        self._rope_cache = {}
        self.profile = None  # dict name -> [ms] when set (bench / tests)

    # ---- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, config=None, seed=1234, device="cuda", fp8=False, fp8_attention=False, lora=None):
        """`lora` (a path, (path_or_dict, scale), {"path", "scale", "name"} or a list of them: alg_amd/lora.py) is merged into
        the state dict before the model is built from it."""
        from . import lora as _lora
        config = config or WanTransformerConfig()
        sd = synthetic_state_dict(config, seed=seed, device=device)
        return _lora.build(cls, config, sd, lora, device, fp8=fp8, fp8_attention=fp8_attention)

    @classmethod
    def from_pretrained(cls, path, subfolder="transformer", torch_dtype=BF, device="cuda", fp8=False, fp8_attention=False,
                        lora=None, **_):
        """Load a diffusers-format checkpoint directory (config.json + *.safetensors) from local disk.  `lora` (as in
        from_synthetic) is merged into the state dict before the model is built from it; in a multi-rank run every rank merges
        for itself behind the weight broadcast.  `attn_reuse`, `attn_reuse_t_lo` and `attn_reuse_t_hi` (taken from the trailing keywords; alg_amd/attn_reuse.py) set the
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
                                    "WanTransformer3DModel.from_synthetic for shape-faithful synthetic weights)" % cfg_path)
        with open(cfg_path) as f:
            raw = json.load(f)
        fields = WanTransformerConfig.__dataclass_fields__
        cfg = WanTransformerConfig(**{k: (tuple(v) if k == "patch_size" else v) for k, v in raw.items() if k in fields})
        from .weights import read_shards
        from . import lora as _lora
        model = _lora.build(cls, cfg, read_shards(root), lora, device, fp8=fp8, fp8_attention=fp8_attention)
        apply_switches(model, reuse)
        _cfg_reuse.apply_switches(model, cfg_switches)
        _attn_far.apply_switches(model, far_switches)
        _attn_pool.apply_switches(model, pool_switches)
        return model

    def to(self, *args, **kwargs):
        return self

    # ---- helpers -----------------------------------------------------------------------------------------------------
    def rope_tables(self, F_, H, W):
        """WanRotaryPosEmbed as (cos, sin) fp32 [S, 64]: axis split (44, 42, 42) of the 128-wide head, float64 angles."""
        key = (F_, H, W)
        hit = self._rope_cache.get(key)
        if hit is None:
            cfg = self.config
            d = cfg.attention_head_dim
            pt, ph, pw = cfg.patch_size
            h_dim = w_dim = 2 * (d // 6)
            t_dim = d - h_dim - w_dim
            tabs = []
            for dim in (t_dim, h_dim, w_dim):
                freqs = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float64)[: dim // 2] / dim))
                tabs.append(torch.outer(torch.arange(cfg.rope_max_seq_len, dtype=torch.float64), freqs))
            ppf, pph, ppw = F_ // pt, H // ph, W // pw
            ang = torch.cat([tabs[0][:ppf].view(ppf, 1, 1, -1).expand(ppf, pph, ppw, -1),
                             tabs[1][:pph].view(1, pph, 1, -1).expand(ppf, pph, ppw, -1),
                             tabs[2][:ppw].view(1, 1, ppw, -1).expand(ppf, pph, ppw, -1)], dim=-1)
            ang = ang.reshape(ppf * pph * ppw, -1)
            hit = (torch.cos(ang).float().to(self.device).contiguous(), torch.sin(ang).float().to(self.device).contiguous())
            self._rope_cache[key] = hit
        return hit

    def _workspace(self, N, S, n_txt, n_img):
        key = (N, S, n_txt, n_img)
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()  # one shape at a time: the buffers are large
            cfg, dev = self.config, self.device
            D, Ff = cfg.dim, cfg.ffn_dim
            e = lambda *s, dt=BF: torch.empty(*s, dtype=dt, device=dev)
            z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=dev)
            ws = SimpleNamespace()
            ws.S_pad = (S + 63) // 64 * 64
            ws.patches = e(N, S, self.k_patch)
            ws.x, ws.y, ws.att, ws.qc = e(N, S, D), e(N, S, D), e(N, S, D), e(N, S, D)
            ws.qk = e(N, S, 2 * D)
            ws.vt = z(N, D, ws.S_pad)              # padding columns stay zero (multiplied by p = 0)
            ws.h = e(N, S, Ff)
            ws.o2 = None                           # second cross-attention output: only the two-launch form (dual_cross off) needs it
            ws.tok = e(N, S, self.w.out_w.shape[0])
            if self.fp8:
                ws.q8 = e(N * S, max(D, Ff), dt=torch.uint8)      # e4m3 copy of the current GEMM input
                ws.q8s = e(N * S, dt=torch.float32)
            ws.temb_f32 = e(N, cfg.freq_dim, dt=torch.float32)
            ws.t1 = e(N, D, dt=torch.float32)
            ws.temb, ws.temb_silu = e(N, D), e(N, D)
            ws.tproj = e(N, 6 * D)
            ws.mod = e(cfg.num_layers, N, 6, D, dt=torch.float32)
            ws.mod_out = e(1, N, 2, D, dt=torch.float32)
            ws.txt_h, ws.txt = e(N, n_txt, D), e(N, n_txt, D)
            ws.kt = e(N, n_txt, D)
            ws.txt_pad = (n_txt + 63) // 64 * 64
            ws.vtt = z(N, D, ws.txt_pad)
            if n_img:
                I = cfg.image_dim
                ws.img_n, ws.img_h = e(N, n_img, I), e(N, n_img, I)
                ws.img_p, ws.img = e(N, n_img, D), e(N, n_img, D)
                ws.ki = e(N, n_img, D)
                ws.img_pad = (n_img + 63) // 64 * 64
                ws.vti = z(N, D, ws.img_pad)
            self._ws[key] = ws
        if self.fp8_attention and not hasattr(ws, "a8"):   # e4m3 operands of the self-attention: only once the flag is on
            cfg, dev = self.config, self.device
            D, heads = cfg.dim, cfg.num_attention_heads
            ws.a8 = torch.empty(N, S, 2 * D, dtype=torch.uint8, device=dev)              # Q | K, the layout of ws.qk
            ws.a8s = torch.empty(N, S, heads, dtype=torch.float32, device=dev)           # Q scales
            ws.k8s = torch.stack([L.k8_scale for L in self.blocks])[:, None, :].expand(-1, N, -1).contiguous()   # [layers, N, heads]
            ws.vt8 = torch.zeros(N, D, ws.S_pad, dtype=torch.uint8, device=dev)
            ws.vt8s = torch.empty(N, D, dtype=torch.float32, device=dev)
        return ws

    def _window_ranges(self, frames, hw, window=None):
        """The frame-window table of this video shape (HeadWindowHost._window_table: cached per (F, hw, window, sink)), or None
        where the window is the dense attention.  window: attn_window, or one of attn_window_widths."""
        if self.fp8_attention:
            raise ValueError("attn_window does not compose with fp8_attention: the e4m3 attention kernel takes no key ranges")
        return self._window_table(frames, hw, window=window)

    def _band_ranges(self, frames, hw, band):
        """The position_band_ranges table of this video shape (device-resident, built once), or None where the band is the dense
        attention."""
        key = ("band", frames, hw, band)
        if key not in self._attn_ranges:
            r = position_band_ranges(frames, hw, band)
            if r is not None:
                r.on(self.device)
            self._attn_ranges[key] = r
        return self._attn_ranges[key]

    def _band_scratch(self, N, S, D, S_pad):
        """Position-major Q, K, O [N, S, D] and V^T [N, D, S_pad] for up to all heads; a launch over fewer heads uses the front of
        each compactly.  Allocated on the calibration forward (never inside a capture) and kept."""
        b = self._band_ws
        if b is None or b.shape != (N, S, D, S_pad):
            if _lib._capturing():
                raise _lib.AlgHipError("attn_band: the position-major scratch for batch %d has not been allocated yet, which a "
                                       "capture cannot do -- run one eager forward of this batch size first" % N)
            e = lambda *s_: torch.empty(*s_, dtype=BF, device=self.device)
            b = self._band_ws = SimpleNamespace(shape=(N, S, D, S_pad), q=e(N, S, D), k=e(N, S, D), o=e(N, S, D), vt=e(N, D, S_pad))
        return b

    def _band_attention(self, T, ws, bs, hl, table, N, F_, S, S_pad, scale, lse=None):
        """The band launch of the heads `hl` (a HeadList): gather Q, K and V^T position-major into the scratch, one ranged launch
        over the compact buffers into bs.o (with `lse`: the _heads entry, which also writes the LSE)."""
        D, n, hw = self.config.dim, hl.n_sel, S // F_
        Dc = n * 128
        T("attn_layout", _lib.attn_rows_position_major, ws.qk, bs.q, hl, 128, N, F_, hw, S * 2 * D, 2 * D, S * Dc, Dc)
        T("attn_layout", _lib.attn_rows_position_major, ws.qk, bs.k, hl, 128, N, F_, hw, S * 2 * D, 2 * D, S * Dc, Dc, src_off=D)
        T("attn_layout", _lib.attn_vt_position_major, ws.vt, bs.vt, hl, 128, N, F_, hw, D * S_pad, S_pad, Dc * S_pad, S_pad)
        A = (bs.q, bs.k, bs.vt, bs.o, N, n, S, S, S * Dc, Dc, S * Dc, Dc, Dc * S_pad, S_pad, S * Dc, Dc, scale, table)
        if lse is not None:
            T("attn_calib", _lib.flash_attn_d128_ranges_heads, *A, lse=lse)
        else:
            T("attn_band", _lib.flash_attn_d128_ranges, *A)

    def _self_attention(self, T, ws, plan, li, band_t, N, F_, S, scale):
        """Block li's self-attention from ws.qk / ws.vt into ws.att: the launch (or calibration) of `plan`, and around it, with
        attn_band (band_t: the band table), the band heads' launch on position-major operands."""
        D, heads, S_pad = self.config.dim, self.config.num_attention_heads, ws.S_pad
        ops = SelfAttnOperands(128, ws.qk, ws.qk, ws.vt, ws.att, N, heads, S, S, S * 2 * D, 2 * D, S * 2 * D, 2 * D, D * S_pad, S_pad,
                               S * D, D, scale, k_off=D)
        if plan.far is not None:   # attn_far_reuse / attn_far_pool: near launch, (far launches,) merge
            return plan.far.attention(T, "attn_self", ops, li)
        cal = plan.cal
        if cal is not None:   # the calibration forward: the dense output, the window's recall
            calibrate_self_attention(T, "attn_self", ops, cal, li, N, 0, (0, S), plan.full[0], plan.measure[0])
            if band_t is not None:   # the third candidate: every head on position-major operands, for its LSE only
                all_heads = self._band_plan(plan.shared[0], ("band",) * heads)[1]
                self._band_attention(T, ws, self._band_scratch(N, S, D, S_pad), all_heads, band_t, N, F_, S, S_pad, scale,
                                     lse=cal.lse_band)
                # (rows p F + f -> f hw + p: a torch transpose of the fp32 LSE, once per layer per video)
                cal.lse_band_rows.view(N, heads, F_, S // F_).copy_(cal.lse_band.view(N, heads, S // F_, F_).transpose(-1, -2))
                T("attn_calib", _lib.attn_lse_recall, cal.lse_band_rows, cal.lse_full, cal.recall_band, N * heads, S,
                  out_off=li * N * heads)
            return
        band_heads = None
        if band_t is not None and plan.mode == "tables":   # the main launch's table without the band heads
            table, band_heads = self._layer_band_plan(plan.bases[0], li)
            order = plan.order(table)
        else:
            table, order = plan.layer(li)
        if band_heads is None or band_heads.n_sel < heads:   # (every head chose the band: no main launch)
            launch_self_attention(T, "attn_self", ops, table, order)
        if band_heads is not None:   # behind the main launch, which wrote zeros to these heads' slices of ws.att
            bs = self._band_scratch(N, S, D, S_pad)
            self._band_attention(T, ws, bs, band_heads, band_t, N, F_, S, S_pad, scale)
            Dc = band_heads.n_sel * 128
            T("attn_layout", _lib.attn_rows_position_major, bs.o, ws.att, band_heads, 128, N, F_, S // F_, S * Dc, Dc, S * D, D,
              inverse=True)

    # ---- forward -----------------------------------------------------------------------------------------------------
    def __call__(self, hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image=None,
                 attention_kwargs=None, return_dict=True, cache_keys=None, cache_force=False):
        """cache_keys (one hashable per sample, naming the role of its pass) arms the step cache when `step_cache` > 0;
        cache_force computes this forward whatever the probe says (the last step of a schedule).  With `attn_reuse` >= 2 the same
        keys, as an attn_reuse.StepKeys that carries the step's timestep, name the samples' attention-cache entries, and
        cache_force computes (and rewrites them) whatever the schedule says."""
        cfg, w, G, T = self.config, self.w, _lib.gemm, self._timed
        if hidden_states.device.type != "cuda":
            raise _lib.AlgHipError("WanTransformer3DModel needs device tensors; there is no CPU fallback")
        N, C, F_, H, W = hidden_states.shape
        pt, ph, pw = cfg.patch_size
        if C != cfg.in_channels or H % ph or W % pw:
            raise ValueError(f"hidden_states must be [N, {cfg.in_channels}, F, H, W] with H, W divisible by the patch size")
        if self.has_image and encoder_hidden_states_image is None:
            raise ValueError("this checkpoint has an image embedder: pass encoder_hidden_states_image")
        D, Ff, heads = cfg.dim, cfg.ffn_dim, cfg.num_attention_heads
        S = F_ * (H // ph) * (W // pw)
        n_txt = encoder_hidden_states.shape[1]
        if encoder_hidden_states_image is not None and cfg.pos_embed_seq_len is not None:
            # FLF2V: the [first, last] image embeddings arrive as separate batch rows ([2 N, 257, I], wan:805-812 + wan:904-908) and
            # are one sample's 2 x 257 tokens: WanImageEmbedding views them as [N, 514, I] before anything else
            b2, s2, i2 = encoder_hidden_states_image.shape
            if (b2 * s2) % cfg.pos_embed_seq_len or b2 * s2 // cfg.pos_embed_seq_len != N:
                raise ValueError("FLF2V: encoder_hidden_states_image %s does not view as [%d, %d, %d]" % (
                    tuple(encoder_hidden_states_image.shape), N, cfg.pos_embed_seq_len, i2))
            encoder_hidden_states_image = encoder_hidden_states_image.reshape(N, cfg.pos_embed_seq_len, i2)
        n_img = encoder_hidden_states_image.shape[1] if encoder_hidden_states_image is not None else 0
        ws = self._workspace(N, S, n_txt, n_img)
        S_pad, scale = ws.S_pad, 1.0 / math.sqrt(cfg.attention_head_dim)
        cos, sin = self.rope_tables(F_, H, W)
        hs = hidden_states.to(BF).contiguous()
        ehs_in = encoder_hidden_states.to(BF).contiguous()

        # ---- embedders ----
        T("patchify", _lib.patchify3d, hs, ws.patches, N, C, F_, H, W, ph, pw, self.k_patch)
        T("gemm_patch", G, ws.patches, w.patch_w, ws.x, N * S, D, self.k_patch, self.k_patch, self.k_patch, D, bias=w.patch_b)
        t = timestep.to(device=self.device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(N)
        t = t.contiguous()
        _lib.timestep_embedding_f32(t, ws.temb_f32, N, cfg.freq_dim)
        _lib.linear_f32(ws.temb_f32, w.t1_w, w.t1_b, ws.t1, None, None, N, D, cfg.freq_dim, act=1)
        _lib.linear_f32(ws.t1, w.t2_w, w.t2_b, None, ws.temb, ws.temb_silu, N, D, D, act=0)
        G(ws.temb_silu, w.tp_w, ws.tproj, N, 6 * D, D, D, D, 6 * D, bias=w.tp_b)
        _lib.wan_modulation(w.tables, ws.tproj, ws.mod, cfg.num_layers, N, 6, D, True)
        _lib.wan_modulation(w.table_out, ws.temb, ws.mod_out, 1, N, 2, D, False)
        G(ehs_in, w.x1_w, ws.txt_h, N * n_txt, D, cfg.text_dim, cfg.text_dim, cfg.text_dim, D, bias=w.x1_b,
          act=_lib.ACT_GELU_TANH)
        G(ws.txt_h, w.x2_w, ws.txt, N * n_txt, D, D, D, D, D, bias=w.x2_b)
        if n_img:
            I = cfg.image_dim
            im = encoder_hidden_states_image.to(BF).contiguous()
            if w.img_pos is not None:   # x + pos_embed in the embedder's dtype (one bf16 rounding), per sample (the table has no batch)
                im = torch.stack([_lib.lincomb([(1.0, im[n]), (1.0, w.img_pos)], BF) for n in range(N)])
            _lib.layernorm_mod_f32(im, ws.img_n, w.in1_w, w.in1_b, None, None, 0, N, n_img, I, 1e-5)
            G(ws.img_n, w.if1_w, ws.img_h, N * n_img, I, I, I, I, I, bias=w.if1_b)
            _lib.gelu_erf_(ws.img_h)
            G(ws.img_h, w.if2_w, ws.img_p, N * n_img, D, I, I, I, D, bias=w.if2_b)
            _lib.layernorm_mod_f32(ws.img_p, ws.img, w.in2_w, w.in2_b, None, None, 0, N, n_img, D, 1e-5)

        mod_bs = 6 * D

        def lin(name, A, Wt, C, M_, N_, K_, lda, ldc, requant=True, **kw):
            """C = epilogue(A @ W^T): bf16, or e4m3 operands when the block weights are quantised (A is re-quantised per
            token unless the previous call already left its e4m3 copy in the workspace)."""
            if not self.fp8:
                return T(name, G, A, (packed.get(id(Wt)) or Wt) if packed else Wt, C, M_, N_, K_, lda, K_, ldc, **kw)
            if requant:
                T("quant", _lib.quantize_fp8_rows, A, ws.q8, ws.q8s, N * S, K_, x_rstride=lda)
            sa = kw.pop("strideA", 0)
            return T(name, G, ws.q8, Wt[0], C, M_, N_, K_, K_, K_, ldc, a_scale=ws.q8s, b_scale=Wt[1],
                     strideA=(S * K_ if sa else 0), strideAScale=(S if sa else 0), **kw)

        # fp8 blocks: the norms write the e4m3 tokens + row scales straight into the GEMM operand workspace (the bytes
        # alg_quantize_fp8_rows would make of the bf16 norm output); ws.y is not touched
        fuse_q = self.fp8 and D % 512 == 0 and self.fuse_quant

        def ln_mod(wgt, bia, sc, sh, bs, **kw):
            if fuse_q:
                return T("ln_mod", _lib.layernorm_mod_f32_fp8, ws.x, ws.q8, ws.q8s, wgt, bia, sc, sh, bs, N, S, D, cfg.eps, **kw)
            return T("ln_mod", _lib.layernorm_mod_f32, ws.x, ws.y, wgt, bia, sc, sh, bs, N, S, D, cfg.eps, **kw)

        use_packed = not self.fp8 and self.packed_weights and os.environ.get("ALG_GEMM_PIPE", "10") == "10"
        packed = None
        # attention reuse (alg_amd/attn_reuse.py): None -- off, nothing below differs from the plain forward; refused next to a step cache
        ar = self._attn_reuse_begin(cache_keys, cache_force, N, len(self.blocks), S, D)
        sc = self._step_cache_begin(ws.x, cache_keys, cache_force, 0, S)   # None: off, nothing below differs from the plain forward
        kvr = self._window_ranges(F_, S // F_) if self.attn_window else None    # None: the dense launch
        # attn_band validated (needs the recall policy, excludes the widths); 0: off -- also on a forward the sampler runs with the
        # window switched off (call_transformer: the dense early steps)
        band = self._head_window_band() if self.attn_window else 0
        band_t = self._band_ranges(F_, S // F_, band) if band and kvr is not None else None    # None: off, or the band is dense
        # this forward's self-attention launches: the shared window, or per-head tables chosen by recall (attn_window.SelfAttnPlan)
        plan = self._self_attn_begin([kvr], (F_, S // F_, int(self.attn_window), int(self.attn_sink_frames)), len(self.blocks), N,
                                     heads, S, (N, S, D), batch=N, band=band if band_t is not None else 0,
                                     table_of=lambda g, w_: self._window_ranges(F_, S // F_, window=w_),
                                     profile_of=lambda g, ws_: self._profile_table(F_, S // F_, ws_))
        # far-field reuse (alg_amd/attn_far.py): None -- off (or a dense step, or a window that covers the video)
        # pooled far field (alg_amd/attn_pool.py): None -- off (or a dense step, or a window that covers the video); it takes the
        # place of the far-field reuse in plan.far and refuses to run next to it
        pool = self._attn_pool_begin([kvr], N, heads, 128, S)
        plan.far = pool if pool is not None else self._attn_far_begin(cache_keys, cache_force, [kvr], N, len(self.blocks), heads, 128, S)
        for li, L in enumerate(self.blocks):
            if li == 1 and sc is not None and T("step_cache", sc.after_block0, ws.x):
                break                 # hit: x = x1 + the cached tail, straight to the head
            if use_packed:   # lin() looks the row-major weight up by identity
                packed = {id(getattr(L, name)): pw for name, pw in L.packed.items()}
            m0 = li * N * 6 * D  # element offset of this block's [N, 6, D] modulation: shift, scale, gate, c_shift, c_scale, c_gate
            # ---- self-attention ----
            if ar is not None and ar.reuse:   # attn_reuse: the cached attention output stands in for everything up to it
                T("attn_reuse", ar.load, li, ws.att)
            else:
                ln_mod(None, None, ws.mod, ws.mod, mod_bs, scale_off=m0 + D, shift_off=m0)
                vt_kw = dict(bias=L.bv, batch=N, strideB=S * D, strideC=D * S_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
                if self.fp8:
                    lin("gemm_qk", ws.y, L.wqk, ws.qk, N * S, 2 * D, D, D, 2 * D, requant=not fuse_q, bias=L.bqk)
                    # V^T: the weight is the A operand, the (already quantised) tokens are B
                    T("gemm_vt", G, L.wv[0], ws.q8, ws.vt, D, S, D, D, D, S_pad, a_scale=L.wv[1], b_scale=ws.q8s, strideBScale=S, **vt_kw)
                elif self.pair_qkv:   # both projections read y: one persistent launch (alg_gemm_bf16_pair), bit-identical
                    T("gemm_qkv", _lib.gemm_pair, ((ws.y, L.wqk, ws.qk, N * S, 2 * D, D, D, D, 2 * D), dict(bias=L.bqk)),
                      ((L.wv, ws.y, ws.vt, D, S, D, D, D, S_pad), vt_kw))
                else:
                    lin("gemm_qk", ws.y, L.wqk, ws.qk, N * S, 2 * D, D, D, 2 * D, bias=L.bqk)
                    T("gemm_vt", G, L.wv, ws.y, ws.vt, D, S, D, D, D, S_pad, **vt_kw)
                if self.fp8_attention:   # e4m3 Q | K straight out of the norm, V^T per row, attention on the fp8 MFMA
                    T("rms_rope", _lib.rmsnorm_rope_fp8, ws.qk, L.nq, cos, sin, 2 * D, N, S, D, cfg.eps, ws.a8, 2 * D, scale=ws.a8s)
                    T("rms_rope", _lib.rmsnorm_rope_fp8, ws.qk, L.nk, cos, sin, 2 * D, N, S, D, cfg.eps, ws.a8, 2 * D,
                      head_scale=ws.k8s, hs_off=li * N * heads, x_off=D, q8_off=D)
                    T("vt_quant", _lib.quantize_fp8_vt, ws.vt, ws.vt8, ws.vt8s, N, D, S, D * S_pad, S_pad, D * S_pad, S_pad)
                    T("attn_self", _lib.flash_attn_d128_fp8, ws.a8, ws.a8s, ws.a8, ws.k8s, ws.vt8, ws.vt8s, ws.att, N, heads, S, S,
                      S * 2 * D, 2 * D, S * 2 * D, 2 * D, D * S_pad, S_pad, S * D, D, scale, k_off=D, ks_off=li * N * heads)
                else:
                    T("rms_rope", _lib.rmsnorm_rope_, ws.qk, L.nq, cos, sin, 2 * D, N, S, D, cfg.eps)
                    T("rms_rope", _lib.rmsnorm_rope_, ws.qk, L.nk, cos, sin, 2 * D, N, S, D, cfg.eps, x_off=D)
                    self._self_attention(T, ws, plan, li, band_t, N, F_, S, scale)
                if ar is not None:
                    T("attn_reuse", ar.store, li, ws.att)
            lin("gemm_out", ws.att, L.wo, ws.x, S, D, D, D, D, bias=L.bo, R=ws.x, ldr=D, gate=ws.mod,
                gate_off=m0 + 2 * D, strideGate=mod_bs, batch=N, strideA=S * D, strideC=S * D, strideR=S * D,
                seg_split=1 << 30, flags=_lib.GEMM_GATE_F32)
            # ---- cross-attention: image tokens and text tokens attend separately, outputs are added ----
            if cfg.cross_attn_norm:
                ln_mod(L.n2w, L.n2b, None, None, 0)
                lin("gemm_cq", ws.y, L.cq_w, ws.qc, N * S, D, D, D, D, requant=not fuse_q, bias=L.cq_b)
            else:
                lin("gemm_cq", ws.x, L.cq_w, ws.qc, N * S, D, D, D, D, bias=L.cq_b)
            T("rms_rope", _lib.rmsnorm_rope_, ws.qc, L.cnq, None, None, D, N, S, D, cfg.eps)
            G(ws.txt, L.ck_w, ws.kt, N * n_txt, D, D, D, D, D, bias=L.ck_b)
            _lib.rmsnorm_rope_(ws.kt, L.cnk, None, None, D, N, n_txt, D, cfg.eps)
            G(L.cv_w, ws.txt, ws.vtt, D, n_txt, D, D, D, ws.txt_pad, bias=L.cv_b, batch=N, strideB=n_txt * D,
              strideC=D * ws.txt_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
            if n_img:
                G(ws.img, L.ak_w, ws.ki, N * n_img, D, D, D, D, D, bias=L.ak_b)
                _lib.rmsnorm_rope_(ws.ki, L.cnak, None, None, D, N, n_img, D, cfg.eps)
                G(L.av_w, ws.img, ws.vti, D, n_img, D, D, D, ws.img_pad, bias=L.av_b, batch=N, strideB=n_img * D,
                  strideC=D * ws.img_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
            if n_img and self.dual_cross:   # sdpa(q, k, v) + sdpa(q, k_img, v_img): one launch, Q read once, no add pass
                T("attn_cross", _lib.flash_attn_d128_dual, ws.qc, ws.kt, ws.vtt, n_txt, n_txt * D, D, D * ws.txt_pad, ws.txt_pad,
                  ws.ki, ws.vti, n_img, n_img * D, D, D * ws.img_pad, ws.img_pad, ws.att, N, heads, S, S * D, D, S * D, D, scale)
            else:
                T("attn_cross", _lib.flash_attn_d128, ws.qc, ws.kt, ws.vtt, ws.att, N, heads, S, n_txt, S * D, D, n_txt * D, D,
                  D * ws.txt_pad, ws.txt_pad, S * D, D, scale)
                if n_img:
                    if ws.o2 is None:
                        ws.o2 = torch.empty_like(ws.att)
                    T("attn_cross", _lib.flash_attn_d128, ws.qc, ws.ki, ws.vti, ws.o2, N, heads, S, n_img, S * D, D, n_img * D,
                      D, D * ws.img_pad, ws.img_pad, S * D, D, scale)
                    T("add", _lib.lincomb, [(1.0, ws.att), (1.0, ws.o2)], BF, out=ws.att)
            lin("gemm_cout", ws.att, L.co_w, ws.x, N * S, D, D, D, D, bias=L.co_b, R=ws.x, ldr=D)
            # ---- feed-forward ----
            ln_mod(None, None, ws.mod, ws.mod, mod_bs, scale_off=m0 + 4 * D, shift_off=m0 + 3 * D)
            lin("gemm_ff1", ws.y, L.f1_w, ws.h, N * S, Ff, D, D, Ff, requant=not fuse_q, bias=L.f1_b,
                act=_lib.ACT_GELU_TANH)
            lin("gemm_ff2", ws.h, L.f2_w, ws.x, S, D, Ff, Ff, D, bias=L.f2_b, R=ws.x, ldr=D, gate=ws.mod,
                gate_off=m0 + 5 * D, strideGate=mod_bs, batch=N, strideA=S * Ff, strideC=S * D, strideR=S * D,
                seg_split=1 << 30, flags=_lib.GEMM_GATE_F32)

        if sc is not None:
            if len(self.blocks) == 1:  # no tail to skip: the probe and the rule run all the same (x + 0 on a hit)
                T("step_cache", sc.after_block0, ws.x)
            T("step_cache", sc.end, ws.x)   # computed forward: tail <- x - x1 (a no-op behind a hit)

        plan.finish(band_table=band_t)
        if ar is not None:
            ar.finish()

        # ---- output head ----
        _lib.layernorm_mod_f32(ws.x, ws.y, None, None, ws.mod_out, ws.mod_out, 2 * D, N, S, D, cfg.eps, scale_off=D,
                               shift_off=0)
        n_out = w.out_w.shape[0]
        G(ws.y, w.out_w, ws.tok, N * S, n_out, D, D, D, n_out, bias=w.out_b)
        out = torch.empty(N, cfg.out_channels, F_, H, W, dtype=BF, device=self.device)
        _lib.unpatchify3d(ws.tok, n_out, out, N, cfg.out_channels, F_, H, W, ph, pw)
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
