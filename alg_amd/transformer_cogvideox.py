"""CogVideoXTransformer3DModel forward on hand-written gfx950 kernels.

Mirrors the component protocol the reference loop requires of its injected transformer:

    transformer(hidden_states=, encoder_hidden_states=, timestep=, ofs=, image_rotary_emb=,
                attention_kwargs=, return_dict=False)[0]        (pipeline_cogvideox_image2video_lowpass.py:1082-1090)
    transformer.config.{sample_height, sample_width, sample_frames, patch_size, patch_size_t, in_channels,
                        use_rotary_positional_embeddings, ofs_embed_dim, attention_head_dim}, transformer.dtype

The arithmetic follows diffusers' CogVideoXTransformer3DModel (diffusers @ be2fb77, not in the reference
tree -- parity unpinned); the weight dict uses the diffusers state-dict names so a real
checkpoint maps 1:1.  Host code here only owns buffers and launch order: every FLOP and every byte of the
forward moves through libalg_hip.so (GEMM + epilogues, flash attention, LayerNorm/AdaLN, QK-norm + RoPE,
patch gather / unpatchify, timestep sinusoid).

HBM layout (all bf16, allocated once per batch size N and reused every step):
    x      [N, S, D]        residual stream, S = text_len + patches, text tokens first
    y      [N, S, D]        LayerNorm+modulate output (GEMM A operand)
    qk     [N, S, 2, H, 64] fused Q|K projection, normalised + rotated in place
    vt     [N, H*64, S_pad] V^T written directly by a transposed GEMM (kv order permuted for the MFMA B operand)
    att    [N, S, D]        attention output (A operand of the out-projection)
    h      [N, S, 4D]       GELU(FF1)
    mod    [N, L*12D + 4D]  every AdaLN shift/scale/gate vector of the forward, one GEMM
fp8 mode only (allocated on the first fp8 forward of a shape):
    q8     [N*S, 4D] bytes  OCP e4m3 copy of the current GEMM input (rows of K = D or 4D bytes, contiguous)
    q8s    [N, S4] float32  its per-token scales, S4 = S rounded up to a multiple of 4 (the V^T GEMM reads them as its B scales,
                            16 bytes at a time, per batch item)
fp4 mode only (allocated on the first fp4 forward of a shape):
    q4     [N*S, 2D] bytes  OCP MXFP4 copy of the current feed-forward GEMM input (rows of K/2 bytes, K = D or 4D, contiguous):
                            with fuse_quant norm2 writes it (rows of D/2 bytes) and ff1 reads it
    q4s    [N*S, D/8] bytes its E8M0 block scales (rows of K/32 bytes)
    q4h    [N*S, 2D] bytes  with fuse_quant: GELU(FF1) as ff1's epilogue writes it, MXFP4 (rows of 2D bytes), ff2's input -- a
                            second buffer, since ff1 cannot write the one it reads (h is then not written at all)
    q4hs   [N*S, D/8] bytes its E8M0 block scales
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, asdict
from typing import Optional

import torch

from . import _lib
from .attn_far import AttnFarHost
from .attn_pool import AttnPoolHost
from .attn_reuse import AttnReuseHost
from .cfg_reuse import CfgReuseHost
from .attn_window import HeadWindowHost, SelfAttnOperands, calibrate_self_attention, launch_self_attention
from .step_cache import StepCacheHost


@dataclass
class CogVideoXTransformerConfig:
    """Defaults = THUDM/CogVideoX-5b-I2V."""

    num_attention_heads: int = 48
    attention_head_dim: int = 64
    in_channels: int = 32
    out_channels: int = 16
    num_layers: int = 42
    time_embed_dim: int = 512
    text_embed_dim: int = 4096
    max_text_seq_length: int = 226
    sample_width: int = 90
    sample_height: int = 60
    sample_frames: int = 49
    patch_size: int = 2
    patch_size_t: Optional[int] = None
    temporal_compression_ratio: int = 4
    ff_inner_mult: int = 4
    norm_eps: float = 1e-5
    qk_norm_eps: float = 1e-6
    flip_sin_to_cos: bool = True
    freq_shift: int = 0
    use_rotary_positional_embeddings: bool = True
    use_learned_positional_embeddings: bool = True
    ofs_embed_dim: Optional[int] = None
    spatial_interpolation_scale: float = 1.875
    temporal_interpolation_scale: float = 1.0

    @property
    def inner_dim(self):
        return self.num_attention_heads * self.attention_head_dim

    def to_dict(self):
        return asdict(self)


def _bf(t, device):
    return t.to(device=device, dtype=torch.bfloat16).contiguous()


class CogVideoXTransformer3DModel(StepCacheHost, AttnReuseHost, AttnFarHost, AttnPoolHost, CfgReuseHost, HeadWindowHost):
    dtype = torch.bfloat16
    # what lora.merge_into did to the state dict this model was built from (from_pretrained / from_synthetic(lora=...)): a tuple
    # of lora.LoraReport(name, scale, targets, ranks) per adapter; () without LoRA
    lora_report = ()

    # the block linears that fp8 mode quantises, per output channel: Q|K, V, attention out, feed-forward in / out
    FP8_WEIGHTS = ("wqk", "wv", "wo", "wf1", "wf2")

    # the two feed-forward linears that fp4 mode runs with MXFP4 weights and activations
    FP4_WEIGHTS = ("wf1", "wf2")

    def __init__(self, config: CogVideoXTransformerConfig, weights: dict, device="cuda", fp8=False, fp4=False):
        """``fp8=True``: the five block linears (attn1.to_q | to_k, to_v, to_out.0, ff.net.0.proj, ff.net.2) run on the fp8
        MFMA (alg_gemm_fp8) -- weights quantised once to OCP e4m3 with one scale per output channel, activations per token
        in front of each GEMM; embedders, the AdaLN GEMM, proj_out, norms, attention and the residual stream stay bf16.
        Built this way the model keeps no bf16 (or packed) copy of those weights.  ``model.fp8`` may also be flipped on a
        model built in bf16 (A/B runs): the e4m3 copies are then made on the first fp8 forward and both sets are kept.

        ``fp4=True`` (an extension, off by default): ff.net.0.proj and ff.net.2 of every block run with OCP MXFP4 weights and
        activations (W4A4, alg_gemm_fp4: e2m1 elements, one E8M0 scale per 32 along K) -- weights quantised once per output
        channel, the norm2 output and the GELU output per token, by the kernels that compute them (``fuse_quant``, as for e4m3;
        off: each is written bf16 first and quantised by a pass of its own); everything else as ``fp8`` decides.
        Built this way the model keeps no bf16, packed or e4m3 copy of those two weights; ``model.fp4`` may be flipped on a
        model built without it exactly like ``fp8``."""
        cfg = self.config = config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AlgHipError("CogVideoXTransformer3DModel runs on the GPU only (HIP kernels, no CPU fallback)")
        if cfg.attention_head_dim != 64:
            raise _lib.AlgHipError("the attention kernel is specialised for head_dim 64")
        if cfg.ofs_embed_dim is not None and cfg.ofs_embed_dim != cfg.time_embed_dim:
            raise _lib.AlgHipError("ofs_embed_dim must equal time_embed_dim (emb = emb + ofs_emb)")
        D = cfg.inner_dim
        if D % 512:
            raise _lib.AlgHipError("inner_dim must be a multiple of 512 (LayerNorm kernel tiling)")
        self.fp8 = bool(fp8)
        if self.fp8:
            self._check_fp8_shapes()
        self.fp4 = bool(fp4)
        if self.fp4:
            self._check_fp4_shapes()
        # fp8: the modulated LayerNorms write the e4m3 tokens + row scales themselves (alg_layernorm_modulate_fp8; bit-identical
        # to the norm into y followed by the quantiser pass, which is what False runs).  fp4: norm2 and ff1's epilogue write the
        # MXFP4 operands of ff1 and ff2 themselves (alg_layernorm_modulate_mxfp4, alg_gemm_fp4_q4out; the same bits again)
        self.fuse_quant = True
        _lib.load_library()
        # True (default): the softmax scale * log2(e) rides in Q's last rounding and the attention takes log2-unit scores
        # (alg_qk_norm_rope_scaled + ALG_ATTN_Q_PRESCALED); False keeps the per-score multiply (A/B and parity tests)
        self.attn_prescale = True
        # True (default): the Q|K projection and the transposed V projection of a block go out as one alg_gemm_bf16_pair
        # launch (bit-identical to the two launches; False keeps them apart: A/B runs, tests)
        self.pair_qkv = True
        # True: the per-head QK LayerNorm + rotary embedding runs inside the Q|K projection's store loop (alg_gemm_bf16_pair_qk;
        # bit-identical to the stand-alone kernel behind the pair launch, one read + one write of qk less).  Off by default:
        # measured on the same box (profiles/r4_fuse_qk_norm_ab.txt) the ~20 VALU operations per element cost more in a
        # one-wave-per-SIMD store loop (+9.5 ms per step) than the stand-alone kernel at full occupancy (8.4 ms per step)
        self.fuse_qk_norm = False
        # True (default): the attention-output and feed-forward weights are also kept packed in MFMA-fragment order
        # (alg_pack_b_p11, once, here) and those three GEMMs run schedule 11 (1 x 4 waves, the weight straight from L2 into registers;
        # bit-identical to schedule 10).  False, or ALG_GEMM_PIPE set to another schedule than 10: the row-major weights (A/B runs).
        # The Q|K projection stays on the pair launch with V^T (whose B operand is the activation): on schedule 11 with V^T as its own
        # launch the step was 0.4 % slower (profiles/r6_bench_steps10_ab_packed_qk.json).
        self.packed_weights = True
        # > 0 (opt-in, an extension: alg_amd/step_cache.py): a forward that is handed `cache_keys` probes block 0's residual and,
        # while sum |r - r_prev| < step_cache * sum |r_prev| over the video tokens of every sample, replaces blocks 1 .. L-1 by the
        # residual they produced on the last computed forward.  0.0: every forward is the plain one, launch for launch.
        self.step_cache = 0.0
        self.step_cache_max_consecutive = 0   # at most this many skipped forwards in a row (0: no cap)
        # N >= 2 (opt-in, an extension: alg_amd/attn_reuse.py): a forward that is handed `cache_keys` with the step's timestep
        # (attn_reuse.step_keys) computes every block's self-attention on every N-th step while attn_reuse_t_lo < t < attn_reuse_t_hi
        # and reads it back from a per-key cache on the steps between, skipping norm1, Q|K, V^T, qk_norm_rope and the attention.
        # 0: every forward is the plain one, launch for launch, nothing allocated.  attn_reuse_drift: the diagnostic (AttnReuseHost)
        self.attn_reuse = 0
        # N >= 2 (opt-in, an extension: alg_amd/attn_far.py; needs attn_window > 0): the keys inside the frame window are attended
        # to fresh on every step, the keys outside it on every N-th step while attn_far_reuse_t_lo < t < attn_far_reuse_t_hi and
        # from the cached partial (output and LSE) on the steps between, merged by alg_attn_merge_lse.  0: nothing differs
        self.attn_far_reuse = 0
        # G in {2, 4, 8} (opt-in, an extension: alg_amd/attn_pool.py; needs attn_window > 0): the keys outside the frame window are
        # attended to on every step as groups of G consecutive keys pooled into one (mean k, mean v, a score bias of log2 G), merged
        # with the window's partial by alg_attn_merge_lse_shift.  No state across steps.  0: nothing differs
        self.attn_far_pool = 0
        # > 0 (opt-in, an extension: alg_amd/attn_window.py; may be flipped between calls): in the joint attention of every block a
        # block of latent queries attends to the prompt keys, to the conditioning frames (attn_sink_frames) and to the latent frames
        # within attn_window of its own; prompt queries see everything.  ONE alg_flash_attn_d64_ranges launch for the whole batch.
        # 0: today's launches, nothing allocated
        self.attn_window = 0
        self.attn_sink_frames = 1
        # attn_window_recall > 0 (opt-in, with attn_window > 0): only the heads whose measured recall reaches it keep the window
        # (attn_window.HeadWindowHost: attn_window_stats, reset_attn_window_heads).  0.0: the shared window, nothing allocated
        self._head_window_init()      # (attn_window_widths stays None: the property below refuses anything else)
        self._sincos = {}
        dev = self.device
        w = weights
        p = cfg.patch_size
        self.p_t = cfg.patch_size_t or 1   # CogVideoX 1.5: Linear patch embed over (c, t, py, px), frames folded in p_t
        self.k_patch = cfg.in_channels * p * p * self.p_t
        if self.k_patch % 64 or cfg.text_embed_dim % 64 or cfg.time_embed_dim % 64:
            raise _lib.AlgHipError("GEMM K dimensions must be multiples of 64")
        self.w_patch = _bf(w["patch_embed.proj.weight"].reshape(D, self.k_patch), dev)
        self.b_patch = _bf(w["patch_embed.proj.bias"], dev)
        self.w_text = _bf(w["patch_embed.text_proj.weight"], dev)
        self.b_text = _bf(w["patch_embed.text_proj.bias"], dev)
        self.pos_emb = _bf(w["patch_embed.pos_embedding"][0], dev) if cfg.use_learned_positional_embeddings else None
        self.w_t1 = _bf(w["time_embedding.linear_1.weight"], dev)
        self.b_t1 = _bf(w["time_embedding.linear_1.bias"], dev)
        self.w_t2 = _bf(w["time_embedding.linear_2.weight"], dev)
        self.b_t2 = _bf(w["time_embedding.linear_2.bias"], dev)
        if cfg.ofs_embed_dim is not None:  # CogVideoX 1.5: emb = time_embedding(t) + ofs_embedding(Timesteps(ofs))
            self.w_o1, self.b_o1 = _bf(w["ofs_embedding.linear_1.weight"], dev), _bf(w["ofs_embedding.linear_1.bias"], dev)
            self.w_o2, self.b_o2 = _bf(w["ofs_embedding.linear_2.weight"], dev), _bf(w["ofs_embedding.linear_2.bias"], dev)

        # AdaLN linears of all layers + norm_out, concatenated into one [TOT, time_embed_dim] weight.  Rows are
        # re-ordered from diffusers' chunk order (shift, scale, gate, enc_shift, enc_scale, enc_gate) to
        # (shift_txt, shift_vid, scale_txt, scale_vid, gate_txt, gate_vid) so each quantity is a [2][D] pair
        # indexed by segment (0 = text rows, 1 = video rows), which is what the kernels consume.
        def reorder6(t):
            c = t.chunk(6, dim=0)
            return torch.cat([c[3], c[0], c[4], c[1], c[5], c[2]], dim=0)

        mw, mb = [], []
        self.layers = []
        for i in range(cfg.num_layers):
            b = "transformer_blocks.%d." % i
            L = {}
            for nm in ("norm1", "norm2"):
                mw.append(reorder6(w[b + nm + ".linear.weight"]))
                mb.append(reorder6(w[b + nm + ".linear.bias"]))
                L[nm + "_w"] = _bf(w[b + nm + ".norm.weight"], dev)
                L[nm + "_b"] = _bf(w[b + nm + ".norm.bias"], dev)
            L["wqk"] = _bf(torch.cat([w[b + "attn1.to_q.weight"], w[b + "attn1.to_k.weight"]], dim=0), dev)
            L["bqk"] = _bf(torch.cat([w[b + "attn1.to_q.bias"], w[b + "attn1.to_k.bias"]], dim=0), dev)
            L["wv"] = _bf(w[b + "attn1.to_v.weight"], dev)
            L["bv"] = _bf(w[b + "attn1.to_v.bias"], dev)
            for nm in ("norm_q", "norm_k"):
                L[nm + "_w"] = _bf(w[b + "attn1." + nm + ".weight"], dev)
                L[nm + "_b"] = _bf(w[b + "attn1." + nm + ".bias"], dev)
            L["wo"] = _bf(w[b + "attn1.to_out.0.weight"], dev)
            L["bo"] = _bf(w[b + "attn1.to_out.0.bias"], dev)
            L["wf1"] = _bf(w[b + "ff.net.0.proj.weight"], dev)
            L["bf1"] = _bf(w[b + "ff.net.0.proj.bias"], dev)
            L["wf2"] = _bf(w[b + "ff.net.2.weight"], dev)
            L["bf2"] = _bf(w[b + "ff.net.2.bias"], dev)
            if self.fp4:
                self._quantize_layer_fp4(L, drop_bf16=True)
            if self.fp8:
                self._quantize_layer(L, drop_bf16=True)
            else:
                for nm in ("wo", "wf1", "wf2"):
                    if nm in L:
                        L["p" + nm] = _lib.PackedB(L[nm])
            self.layers.append(L)
        # norm_out: chunk order (shift, scale) -> (shift, shift, scale, scale) so both segments are valid
        ow, ob = w["norm_out.linear.weight"], w["norm_out.linear.bias"]
        sh_w, sc_w = ow.chunk(2, dim=0)
        sh_b, sc_b = ob.chunk(2, dim=0)
        mw.append(torch.cat([sh_w, sh_w, sc_w, sc_w], dim=0))
        mb.append(torch.cat([sh_b, sh_b, sc_b, sc_b], dim=0))
        self.w_mod = _bf(torch.cat(mw, dim=0), dev)
        self.b_mod = _bf(torch.cat(mb, dim=0), dev)
        self.mod_cols = self.w_mod.shape[0]  # L*12D + 4D
        self.norm_final_w = _bf(w["norm_final.weight"], dev)
        self.norm_final_b = _bf(w["norm_final.bias"], dev)
        self.norm_out_w = _bf(w["norm_out.norm.weight"], dev)
        self.norm_out_b = _bf(w["norm_out.norm.bias"], dev)
        self.w_out = _bf(w["proj_out.weight"], dev)
        self.b_out = _bf(w["proj_out.bias"], dev)
        self._ws = {}
        self._rope_cache = {}
        self.profile = None  # set to a dict to collect (start, stop) HIP event pairs per kernel family

    def _check_fp8_shapes(self):
        cfg = self.config
        D, F4 = cfg.inner_dim, cfg.ff_inner_mult * cfg.inner_dim
        if D % 128 or F4 % 128:
            raise ValueError("fp8=True: the e4m3 GEMM needs K %% 128 == 0, this config has inner_dim = %d and a feed-forward "
                             "width of %d" % (D, F4))

    def _check_fp4_shapes(self):
        cfg = self.config
        D, F4 = cfg.inner_dim, cfg.ff_inner_mult * cfg.inner_dim
        if D % 256 or F4 % 256:
            raise ValueError("fp4=True: the MXFP4 GEMM needs K %% 256 == 0, this config has inner_dim = %d and a feed-forward "
                             "width of %d" % (D, F4))

    @staticmethod
    def _quantize_layer_fp4(L, drop_bf16):
        """MXFP4 copies (packed e2m1 bytes [N, K/2], E8M0 block scales [N, K/32]) of a block's feed-forward weights under "<name>4"."""
        for nm in CogVideoXTransformer3DModel.FP4_WEIGHTS:
            wt = L[nm]
            n, k = wt.shape
            q = torch.empty(n, k // 2, dtype=torch.uint8, device=wt.device)
            sc = torch.empty(n, k // 32, dtype=torch.uint8, device=wt.device)
            _lib.quantize_mxfp4_rows(wt, q, sc, n, k)
            L[nm + "4"] = (q, sc)
            if drop_bf16:
                del L[nm]

    @staticmethod
    def _quantize_layer(L, drop_bf16):
        """e4m3 copies (bytes, per-output-channel float32 scales) of a block's five linears under "<name>8" (a model built with
        fp4=True holds no bf16 feed-forward weights: those two are then left out)."""
        for nm in CogVideoXTransformer3DModel.FP8_WEIGHTS:
            if nm not in L:
                continue
            wt = L[nm]
            q = torch.empty(wt.shape, dtype=torch.uint8, device=wt.device)
            sc = torch.empty(wt.shape[0], dtype=torch.float32, device=wt.device)
            _lib.quantize_fp8_rows(wt, q, sc, wt.shape[0], wt.shape[1])
            L[nm + "8"] = (q, sc)
            if drop_bf16:
                del L[nm]

    def _positional(self, Hh, Ww, Fr, S):
        """The joint [text; video] positional embedding added behind the patch embedding, [S, D] bf16, or None.
        CogVideoXPatchEmbed (the transformer cog:1082 calls): the learned table when the frame count is the configured one,
        otherwise -- and for checkpoints with neither learned nor rotary embeddings (CogVideoX-2B style) -- the 3-D sincos
        embedding computed for the actual grid (`get_3d_sincos_pos_embed`: a quarter of the width for time, three quarters for
        (h, w), positions divided by the interpolation scales), zero rows for the text tokens."""
        cfg = self.config
        learned = cfg.use_learned_positional_embeddings
        if not learned and cfg.use_rotary_positional_embeddings:
            return None
        pre_frames = (Fr - 1) * cfg.temporal_compression_ratio + 1
        if learned and pre_frames == cfg.sample_frames and self.pos_emb is not None and self.pos_emb.shape[0] == S:
            return self.pos_emb
        p = cfg.patch_size
        gh, gw, gt = Hh // p, Ww // p, Fr // self.p_t
        key = (gh, gw, gt)
        hit = self._sincos.get(key)
        if hit is None:
            D = cfg.inner_dim
            ds, dt = 3 * D // 4, D // 4

            def sc1(dim, pos):
                omega = 1.0 / 10000 ** (torch.arange(dim // 2, dtype=torch.float64) / (dim / 2.0))
                out = torch.outer(pos.reshape(-1).double(), omega)
                return torch.cat([out.sin(), out.cos()], dim=1)

            hh = torch.arange(gh, dtype=torch.float32) / cfg.spatial_interpolation_scale
            ww = torch.arange(gw, dtype=torch.float32) / cfg.spatial_interpolation_scale
            tt = torch.arange(gt, dtype=torch.float32) / cfg.temporal_interpolation_scale
            grid = torch.stack(torch.meshgrid(ww, hh, indexing="xy"), dim=0).reshape(2, 1, gh, gw)
            sp = torch.cat([sc1(ds // 2, grid[0]), sc1(ds // 2, grid[1])], dim=1)            # [gh * gw, ds]
            tp = sc1(dt, tt)                                                                   # [gt, dt]
            pe = torch.cat([tp[:, None].expand(-1, gh * gw, -1), sp[None].expand(gt, -1, -1)], dim=-1).reshape(gt * gh * gw, D)
            joint = torch.zeros(cfg.max_text_seq_length + pe.shape[0], D, dtype=torch.float32)
            joint[cfg.max_text_seq_length:] = pe.float()
            hit = joint.to(device=self.device, dtype=torch.bfloat16).contiguous()
            self._sincos[key] = hit
        if hit.shape[0] != S:
            raise ValueError("positional embedding covers %d tokens, the sequence has %d" % (hit.shape[0], S))
        return hit

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, config=None, seed=1234, std=0.02, device="cuda", randomize_affine=False, fp8=False, fp4=False,
                       lora=None):
        """Seeded synthetic weights at the configured shapes, generated on the device tensor by tensor (the
        real checkpoint cannot be downloaded here).  Matrices N(0, std^2), biases 0, norm gains 1.  `lora` (a path,
        (path_or_dict, scale), {"path", "scale", "name"} or a list of them: alg_amd/lora.py) is merged into the state dict
        before the model is built from it."""
        from . import lora as _lora
        from .weights import synthetic_state_dict

        config = config or CogVideoXTransformerConfig()
        sd = synthetic_state_dict(config, seed=seed, std=std, device=device, randomize_affine=randomize_affine)
        return _lora.build(cls, config, sd, lora, device, fp8=fp8, fp4=fp4)

    @classmethod
    def from_pretrained(cls, path, subfolder="transformer", torch_dtype=torch.bfloat16, device="cuda", fp8=False, fp4=False,
                        lora=None, **_):
        """Load a diffusers-format checkpoint directory (config.json + *.safetensors) from local disk.  `lora` (as in
        from_synthetic) is merged into the state dict before the model is built from it; in a multi-rank run every rank reads
        the adapter file and merges for itself behind the weight broadcast (alg_lora_merge gives every rank the same bits).  `attn_reuse`, `attn_reuse_t_lo` and `attn_reuse_t_hi` (taken from the trailing keywords; alg_amd/attn_reuse.py) set the
        model's attention-reuse switches: 0 / 100 / 800 by default, attn_reuse = 1 and lo >= hi are ValueErrors.  `cfg_reuse`,
        `cfg_reuse_t_lo` and `cfg_reuse_t_hi` (alg_amd/cfg_reuse.py) set the samplers' CFG-reuse switches the same way."""
        from . import cfg_reuse as _cfg_reuse
        from .attn_reuse import apply_switches, switches_from
        from . import lora as _lora
        from .weights import load_diffusers_transformer

        reuse = switches_from(_)
        cfg_switches = _cfg_reuse.switches_from(_)
        from . import attn_far as _attn_far
        far_switches = _attn_far.switches_from(_)     # attn_far_reuse, attn_far_reuse_t_lo, attn_far_reuse_t_hi
        from . import attn_pool as _attn_pool
        pool_switches = _attn_pool.switches_from(_)   # attn_far_pool
        config, sd = load_diffusers_transformer(path, subfolder)
        model = _lora.build(cls, config, sd, lora, device, fp8=fp8, fp4=fp4)
        apply_switches(model, reuse)
        _cfg_reuse.apply_switches(model, cfg_switches)
        _attn_far.apply_switches(model, far_switches)
        _attn_pool.apply_switches(model, pool_switches)
        return model

    def to(self, *args, **kwargs):
        return self

    # ------------------------------------------------------------------------------------------------
    def _workspace(self, N, S, P):
        key = (N, S, P)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        cfg, dev = self.config, self.device
        D = cfg.inner_dim
        bf = dict(device=dev, dtype=torch.bfloat16)
        S_pad = (S + 127) // 128 * 128  # V^T pitch.  The attention takes ceil(S / 64) * 64 (tests/test_gpu_attn_operands.py); 128 is kept
        ws = dict(
            S_pad=S_pad,
            x=torch.empty(N, S, D, **bf),
            y=torch.empty(N, S, D, **bf),
            qk=torch.empty(N, S, 2 * D, **bf),
            vt=torch.zeros(N, D, S_pad, **bf),  # pad columns stay zero (stores are guarded)
            att=torch.empty(N, S, D, **bf),
            h=torch.empty(N, S, cfg.ff_inner_mult * D, **bf),
            patches=torch.empty(N, P, self.k_patch, **bf),
            tsin=torch.empty(N, D, **bf),
            t1=torch.empty(N, cfg.time_embed_dim, **bf),
            semb=torch.empty(N, cfg.time_embed_dim, **bf),
            mod=torch.empty(N, self.mod_cols, **bf),
            po=torch.empty(N * P, self.w_out.shape[0], **bf),
        )
        if len(self._ws) >= 4:  # 2-pass and 3-pass shapes both stay resident; anything older is dropped
            self._ws.pop(next(iter(self._ws)))
        self._ws[key] = ws
        return ws

    def _fp8_state(self, ws, N, S):
        """The e4m3 operand workspace of a shape (made on its first fp8 forward) and, for a model built in bf16 whose `fp8`
        attribute was set afterwards, the e4m3 weights next to the bf16 ones."""
        if "q8" not in ws:
            F4 = self.config.ff_inner_mult * self.config.inner_dim
            ws["q8"] = torch.empty(N * S, F4, dtype=torch.uint8, device=self.device)
            ws["q8s"] = torch.empty(N * ((S + 3) // 4 * 4), dtype=torch.float32, device=self.device)
        if self.layers and "wqk8" not in self.layers[0]:
            self._check_fp8_shapes()
            for L in self.layers:
                self._quantize_layer(L, drop_bf16=False)
        return ws["q8"], ws["q8s"]

    def _fp4_state(self, ws, N, S):
        """The MXFP4 operand workspace of a shape (made on its first fp4 forward) and, for a model built without fp4 whose `fp4`
        attribute was set afterwards, the MXFP4 feed-forward weights next to the ones it was built with."""
        if "q4" not in ws:
            F4 = self.config.ff_inner_mult * self.config.inner_dim
            ws["q4"] = torch.empty(N * S, F4 // 2, dtype=torch.uint8, device=self.device)
            ws["q4s"] = torch.empty(N * S, F4 // 32, dtype=torch.uint8, device=self.device)
        if self.fuse_quant and "q4h" not in ws:
            F4 = self.config.ff_inner_mult * self.config.inner_dim
            ws["q4h"] = torch.empty(N * S, F4 // 2, dtype=torch.uint8, device=self.device)
            ws["q4hs"] = torch.empty(N * S, F4 // 32, dtype=torch.uint8, device=self.device)
        if self.layers and "wf14" not in self.layers[0]:
            if "wf1" not in self.layers[0]:
                raise _lib.AlgHipError("this model was built with fp8=True and holds no bf16 copy of its feed-forward weights to "
                                       "quantise to MXFP4: build it with fp4=True (or fp8=False) to run fp4")
            self._check_fp4_shapes()
            for L in self.layers:
                self._quantize_layer_fp4(L, drop_bf16=False)
        return ws["q4"], ws["q4s"]

    def _ff_fp4(self, L, ws, N, S, T, m2):
        """The feed-forward half of a block with MXFP4 operands.  fuse_quant (three launches): norm2 writes q4 / q4s itself, ff1's
        epilogue writes GELU(FF1) as q4h / q4hs, ff2 reads those -- no bf16 y or h goes through memory.  Otherwise (five
        launches, the same bits): norm2 into y (bf16), y and then the GELU output quantised per token into q4 / q4s in front
        of the two alg_gemm_fp4 launches."""
        cfg, TM = self.config, self._timed
        D = cfg.inner_dim
        F4 = cfg.ff_inner_mult * D
        x, y, h, mod, q4, q4s = ws["x"], ws["y"], ws["h"], ws["mod"], ws["q4"], ws["q4s"]
        if self.fuse_quant:
            q4h, q4hs = ws["q4h"], ws["q4hs"]
            TM("ln_mod", _lib.layernorm_modulate_mxfp4, x, q4, q4s, L["norm2_w"], L["norm2_b"], mod, mod, self.mod_cols, N, S, D,
               T, cfg.norm_eps, scale_off=m2 + 2 * D, shift_off=m2)
            TM("gemm_ff1", _lib.gemm_fp4, q4, L["wf14"][0], q4h, S, F4, D, D, D, F4, a_scale=q4s, b_scale=L["wf14"][1],
               bias=L["bf1"], act=_lib.ACT_GELU_TANH, batch=N, strideA=S * D, strideAScale=S * (D // 32), strideC=S * F4,
               q_out_scales=q4hs, strideOutScales=S * (F4 // 32))
            TM("gemm_ff2", _lib.gemm_fp4, q4h, L["wf24"][0], x, S, D, F4, F4, F4, D, a_scale=q4hs, b_scale=L["wf24"][1],
               bias=L["bf2"], R=x, ldr=D, gate=mod, gate_off=m2 + 4 * D, strideGate=self.mod_cols, seg_split=T, batch=N,
               strideA=S * F4, strideAScale=S * (F4 // 32), strideC=S * D, strideR=S * D)
            return
        TM("ln_mod", _lib.layernorm_modulate, x, y, L["norm2_w"], L["norm2_b"], mod, mod, self.mod_cols, N, S, D,
           T, cfg.norm_eps, scale_off=m2 + 2 * D, shift_off=m2)
        TM("quant4", _lib.quantize_mxfp4_rows, y, q4, q4s, N * S, D)
        TM("gemm_ff1", _lib.gemm_fp4, q4, L["wf14"][0], h, S, F4, D, D, D, F4, a_scale=q4s, b_scale=L["wf14"][1], bias=L["bf1"],
           act=_lib.ACT_GELU_TANH, batch=N, strideA=S * D, strideAScale=S * (D // 32), strideC=S * F4)
        TM("quant4", _lib.quantize_mxfp4_rows, h, q4, q4s, N * S, F4)
        TM("gemm_ff2", _lib.gemm_fp4, q4, L["wf24"][0], x, S, D, F4, F4, F4, D, a_scale=q4s, b_scale=L["wf24"][1], bias=L["bf2"],
           R=x, ldr=D, gate=mod, gate_off=m2 + 4 * D, strideGate=self.mod_cols, seg_split=T, batch=N, strideA=S * F4,
           strideAScale=S * (F4 // 32), strideC=S * D, strideR=S * D)

    def _block_fp8(self, L, ws, q8, q8s, N, S, T, m1, m2, cos, sin, scale, q_scale, prescale, plan, li, fp4=False, ar=None):
        """One transformer block with e4m3 operands on its five linears: the launch order of the bf16 block, each GEMM input
        quantised per token into q8 / q8s first (by the LayerNorm itself where a norm produces it)."""
        cfg, G, TM = self.config, _lib.gemm, self._timed
        D, Hn = cfg.inner_dim, cfg.num_attention_heads
        F4 = cfg.ff_inner_mult * D
        x, y, qk, vt, att, h, mod, S_pad = ws["x"], ws["y"], ws["qk"], ws["vt"], ws["att"], ws["h"], ws["mod"], ws["S_pad"]
        # The scales of a batch item start at a multiple of 4 floats (the V^T GEMM reads them as B scales, 16 bytes at a time).
        # S % 4 == 0 (the 5B-I2V shape: 226 + 17,550 tokens): the rows of all items are contiguous and one launch quantises
        # them all; otherwise one launch per item.
        SS = (S + 3) // 4 * 4
        items = ((0, N),) if SS == S else tuple((n, 1) for n in range(N))

        def quant(src, K_):
            for n0, nb in items:
                TM("quant", _lib.quantize_fp8_rows, src, q8, q8s, nb * S, K_, x_off=n0 * S * K_, q_off=n0 * S * K_,
                   scale_off=n0 * SS)

        def ln_mod(nw, nb, m):
            if not self.fuse_quant:
                TM("ln_mod", _lib.layernorm_modulate, x, y, nw, nb, mod, mod, self.mod_cols, N, S, D, T, cfg.norm_eps,
                   scale_off=m + 2 * D, shift_off=m)
                return quant(y, D)
            for n0, n_ in items:
                TM("ln_mod", _lib.layernorm_modulate_fp8, x, q8, q8s, nw, nb, mod, mod, self.mod_cols, n_, S, D, T, cfg.norm_eps,
                   x_off=n0 * S * D, scale_off=n0 * self.mod_cols + m + 2 * D, shift_off=n0 * self.mod_cols + m,
                   q8_off=n0 * S * D, q8_scale_off=n0 * SS)

        def lin(name, wt, C, N_, K_, ldc, **kw):
            """C[n] = epilogue(q8[n] @ W^T) per batch item: A = the e4m3 tokens in the workspace, rows of K_ bytes"""
            TM(name, G, q8, wt[0], C, S, N_, K_, K_, K_, ldc, a_scale=q8s, b_scale=wt[1], batch=N, strideA=S * K_,
               strideAScale=SS, strideC=S * ldc, **kw)

        if ar is not None and ar.reuse:   # attn_reuse: the cached attention output stands in for everything up to it
            TM("attn_reuse", ar.load, li, att)
        else:
            ln_mod(L["norm1_w"], L["norm1_b"], m1)
            lin("gemm_qk", L["wqk8"], qk, 2 * D, D, 2 * D, bias=L["bqk"])
            # V^T: the weight is the A operand, the (already quantised) tokens are B
            TM("gemm_vt", G, L["wv8"][0], q8, vt, D, S, D, D, D, S_pad, a_scale=L["wv8"][1], b_scale=q8s, strideBScale=SS,
               bias=L["bv"], batch=N, strideB=S * D, strideC=D * S_pad, flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS)
            TM("qk_norm_rope", _lib.qk_norm_rope_, qk, L["norm_q_w"], L["norm_q_b"], L["norm_k_w"], L["norm_k_b"], cos, sin, N, S, Hn, T,
               cfg.qk_norm_eps, q_scale=q_scale)
            self._attention(ws, plan, li, N, S, T, scale, prescale)
            if ar is not None:
                TM("attn_reuse", ar.store, li, att)
        quant(att, D)
        lin("gemm_out", L["wo8"], x, D, D, D, bias=L["bo"], R=x, ldr=D, gate=mod, gate_off=m1 + 4 * D,
            strideGate=self.mod_cols, seg_split=T, strideR=S * D)
        if fp4:
            return self._ff_fp4(L, ws, N, S, T, m2)
        ln_mod(L["norm2_w"], L["norm2_b"], m2)
        lin("gemm_ff1", L["wf18"], h, F4, D, F4, bias=L["bf1"], act=_lib.ACT_GELU_TANH)
        quant(h, F4)
        lin("gemm_ff2", L["wf28"], x, D, F4, D, bias=L["bf2"], R=x, ldr=D, gate=mod, gate_off=m2 + 4 * D,
            strideGate=self.mod_cols, seg_split=T, strideR=S * D)

    @property
    def attn_window_widths(self):
        """The per-head window WIDTH of the head_dim 128 models (attn_window.HeadWindowHost): always None here."""
        return None

    @attn_window_widths.setter
    def attn_window_widths(self, value):
        if value is not None:   # refused, not dropped: alg_flash_attn_d64_ranges_heads has no prefix form
            raise ValueError("attn_window_widths=%r: the per-head window width (one-pass calibration) is not built for head_dim 64"
                             % (value,))

    def _window_ranges(self, frames, hw, T):
        """The frame-window table of this sequence shape -- T prompt tokens, then `frames` latent frames of hw tokens
        (HeadWindowHost._window_table: cached per (frames, hw, T, window, sink)).  None: the window covers the video, the launches
        are the dense ones."""
        if not self.attn_prescale:
            raise ValueError("attn_window needs attn_prescale = True: alg_flash_attn_d64_ranges has one softmax form (pre-scaled Q)")
        return self._window_table(frames, hw, (T,), prefix=T)

    def _attention(self, ws, plan, li, N, S, T, scale, prescale):
        """softmax(q k^T * scale) v of the joint sequence from qk / vt into att, as `plan` says for layer li: the dense launch, the
        frame-window table's, a per-head table's -- or, on the calibration forward, the dense output (the per-head entry with the
        one full range: the dense entry's single-launch form, bit for bit) and the window's recall over the latent-query rows
        [T, S)."""
        D, Hn, S_pad = self.config.inner_dim, self.config.num_attention_heads, ws["S_pad"]
        ops = SelfAttnOperands(64, ws["qk"], ws["qk"], ws["vt"], ws["att"], N, Hn, S, S, S * 2 * D, 2 * D, S * 2 * D, 2 * D, D * S_pad,
                               S_pad, S * D, D, scale, k_off=D, q_prescaled=prescale)
        if plan.far is not None:   # attn_far_reuse / attn_far_pool: near launch, (far launches,) merge
            return plan.far.attention(self._timed, "attn", ops, li)
        if plan.cal is not None:
            return calibrate_self_attention(self._timed, "attn", ops, plan.cal, li, N, 0, (T, S - T), plan.full[0], plan.measure[0])
        return launch_self_attention(self._timed, "attn", ops, *plan.layer(li))

    def _rope(self, image_rotary_emb):
        if image_rotary_emb is None:
            return None, None
        cos, sin = image_rotary_emb
        key = (cos.data_ptr(), sin.data_ptr(), tuple(cos.shape))
        hit = self._rope_cache.get(key)
        if hit is None:
            hit = (cos.to(device=self.device, dtype=torch.float32).contiguous(),
                   sin.to(device=self.device, dtype=torch.float32).contiguous())
            self._rope_cache = {key: hit}
        return hit

    # ------------------------------------------------------------------------------------------------
    def forward_assembled(self, latents, conds, encoder_hidden_states, timestep, image_rotary_emb=None, ofs=None,
                          cache_keys=None, cache_force=False):
        """The loop's form of the forward, with the CFG batch assembly (cog:1060-1070) folded into the patch
        gather: sample n sees channels [latents | conds[n]].

        latents [1 or N, F, C, H, W] bf16; conds: list of N tensors [1, F, C, H, W] (or [F, C, H, W]) bf16;
        encoder_hidden_states [N, T, text_dim]; timestep [N].  Returns noise prediction [N, F, C_out, H, W] bf16.

        cache_keys (one hashable per sample, naming the role of its pass) arms the step cache when `step_cache` > 0;
        cache_force computes this forward whatever the probe says (the last step of a schedule).  With `attn_reuse` >= 2 the same
        keys, as an attn_reuse.StepKeys that carries the step's timestep, name the samples' attention-cache entries, and
        cache_force computes (and rewrites them) whatever the schedule says.
        """
        cfg = self.config
        N = len(conds)
        lat = latents.to(device=self.device, dtype=torch.bfloat16).contiguous()
        Bl, Fr, C, Hh, Ww = lat.shape
        if Bl not in (1, N):
            raise ValueError("latents batch must be 1 or len(conds)")
        if 2 * C != cfg.in_channels:
            raise ValueError("latents have %d channels, transformer expects in_channels=%d" % (C, cfg.in_channels))
        conds = [c.to(device=self.device, dtype=torch.bfloat16).contiguous() for c in conds]
        for c in conds:
            if c.numel() != Fr * C * Hh * Ww:
                raise ValueError("conditioning latents must have shape [1, F, C, H, W] matching the latents")
        ehs = encoder_hidden_states.to(device=self.device, dtype=torch.bfloat16).contiguous()
        if ehs.shape[0] != N:
            raise ValueError("encoder_hidden_states batch %d != %d samples" % (ehs.shape[0], N))
        T = ehs.shape[1]
        p, p_t = cfg.patch_size, self.p_t
        if Fr % p_t:
            raise ValueError("latent frames (%d) must be a multiple of patch_size_t=%d (cog:963-968 pads them)" % (Fr, p_t))
        P = (Fr // p_t) * (Hh // p) * (Ww // p)
        S = T + P
        D, Hn = cfg.inner_dim, cfg.num_attention_heads
        if cfg.use_learned_positional_embeddings:
            if cfg.sample_width != Ww or cfg.sample_height != Hh:
                raise ValueError(
                    "It is currently not possible to generate videos at a different resolution that the defaults. "
                    "This should only be the case with 'THUDM/CogVideoX-5b-I2V'.")
        pos_emb = self._positional(Hh, Ww, Fr, S)
        ws = self._workspace(N, S, P)
        x, y, qk, vt, att, h, mod = ws["x"], ws["y"], ws["qk"], ws["vt"], ws["att"], ws["h"], ws["mod"]
        fp8 = bool(self.fp8)
        if fp8:
            q8, q8s = self._fp8_state(ws, N, S)
        elif self.layers and "wqk" not in self.layers[0]:
            raise _lib.AlgHipError("this model was built with fp8=True and holds no bf16 copy of its block weights: build it "
                                   "with fp8=False to run (or switch between) both modes")
        fp4 = bool(self.fp4)
        if fp4:
            self._fp4_state(ws, N, S)
        elif self.layers and "wf1" not in self.layers[0] and not (fp8 and "wf18" in self.layers[0]):
            raise _lib.AlgHipError("this model was built with fp4=True and holds no bf16 (or e4m3) copy of its feed-forward "
                                   "weights: build it with fp4=False to run (or switch between) both modes")
        S_pad = ws["S_pad"]
        cos, sin = self._rope(image_rotary_emb)
        G = _lib.gemm
        TM = self._timed

        # 1. timestep embedding: sinusoid -> linear_1 + SiLU -> linear_2 (+ SiLU: only silu(temb) is consumed)
        ts = timestep.to(device=self.device, dtype=torch.float32).contiguous()
        if ts.numel() != N:
            ts = ts.reshape(-1)[:1].expand(N).contiguous()
        _lib.timestep_embedding(ts, ws["tsin"], N, D, cfg.flip_sin_to_cos)
        E = cfg.time_embed_dim
        G(ws["tsin"], self.w_t1, ws["t1"], N, E, D, D, D, E, bias=self.b_t1, act=_lib.ACT_SILU)
        if cfg.ofs_embed_dim is None:
            G(ws["t1"], self.w_t2, ws["semb"], N, E, E, E, E, E, bias=self.b_t2, act=_lib.ACT_SILU)
        else:
            if ofs is None:
                raise ValueError("this transformer has an ofs embedding: pass `ofs` (cog:998)")
            O = cfg.ofs_embed_dim
            emb, osin, o1, oemb = (torch.empty(N, E, device=self.device, dtype=torch.bfloat16) for _ in range(4))
            G(ws["t1"], self.w_t2, emb, N, E, E, E, E, E, bias=self.b_t2)
            ofs_v = ofs.to(device=self.device, dtype=torch.float32).reshape(-1)
            ofs_v = (ofs_v if ofs_v.numel() == N else ofs_v[:1].expand(N)).contiguous()
            _lib.timestep_embedding(ofs_v, osin, N, O, cfg.flip_sin_to_cos)
            G(osin, self.w_o1, o1, N, O, O, O, O, O, bias=self.b_o1, act=_lib.ACT_SILU)
            G(o1, self.w_o2, oemb, N, O, O, O, O, O, bias=self.b_o2)
            _lib.lincomb([(1.0, emb), (1.0, oemb)], torch.bfloat16, out=emb)
            _lib.silu(emb, ws["semb"])
        # every AdaLN vector of the forward in one GEMM
        G(ws["semb"], self.w_mod, mod, N, self.mod_cols, E, E, E, self.mod_cols, bias=self.b_mod)

        # 2. patch embedding (+ positional embedding as the residual operand), text tokens first
        G(ehs, self.w_text, x, T, D, cfg.text_embed_dim, cfg.text_embed_dim, cfg.text_embed_dim, D,
          bias=self.b_text, R=pos_emb, ldr=D, batch=N, strideA=T * cfg.text_embed_dim, strideC=S * D)
        _lib.patchify(lat, 0 if Bl == 1 else Fr * C * Hh * Ww, conds, ws["patches"], N, Fr, C, Hh, Ww, p, p_t)
        G(ws["patches"], self.w_patch, x, P, D, self.k_patch, self.k_patch, self.k_patch, D, bias=self.b_patch,
          R=pos_emb, ldr=D, r_off=T * D, batch=N, strideA=P * self.k_patch, strideC=S * D, c_off=T * D)

        # 3. transformer blocks
        scale = 1.0 / math.sqrt(cfg.attention_head_dim)
        prescale = self.attn_prescale
        q_scale = scale * 1.4426950408889634 if prescale else 1.0
        F4 = cfg.ff_inner_mult * D
        packed = self.packed_weights and os.environ.get("ALG_GEMM_PIPE", "10") == "10"
        wo_k, wf1_k, wf2_k = ("pwo", "pwf1", "pwf2") if packed else ("wo", "wf1", "wf2")
        kvr = self._window_ranges(Fr // p_t, (Hh // p) * (Ww // p), T) if self.attn_window else None   # None: the dense launch
        # attention reuse (alg_amd/attn_reuse.py): None -- off, nothing below differs from the plain forward; refused next to a step cache
        ar = self._attn_reuse_begin(cache_keys, cache_force, N, len(self.layers), S, D)
        sc = self._step_cache_begin(x, cache_keys, cache_force, T, P)   # None: off, nothing below differs from the plain forward
        # this forward's attention launches: the shared window, or per-head tables chosen by recall (attn_window.SelfAttnPlan)
        plan = self._self_attn_begin([kvr], (Fr // p_t, (Hh // p) * (Ww // p), T, int(self.attn_window), int(self.attn_sink_frames)),
                                     len(self.layers), N, Hn, S, (N, S, D), batch=N)
        # far-field reuse (alg_amd/attn_far.py): None -- off (or a dense step, or a window that covers the video)
        # pooled far field (alg_amd/attn_pool.py): None -- off (or a dense step, or a window that covers the video); it takes the
        # place of the far-field reuse in plan.far and refuses to run next to it
        pool = self._attn_pool_begin([kvr], N, Hn, 64, S)
        plan.far = pool if pool is not None else self._attn_far_begin(cache_keys, cache_force, [kvr], N, len(self.layers), Hn, 64, S)
        for li, L in enumerate(self.layers):
            if li == 1 and sc is not None and TM("step_cache", sc.after_block0, x):
                break                 # hit: x = x1 + the cached tail, straight to the head
            m1 = li * 12 * D          # norm1: shift @+0, scale @+2D, gate @+4D (each [2][D])
            m2 = m1 + 6 * D           # norm2
            if fp8:
                self._block_fp8(L, ws, q8, q8s, N, S, T, m1, m2, cos, sin, scale, q_scale, prescale, plan, li, fp4, ar)
                continue
            if ar is not None and ar.reuse:   # attn_reuse: the cached attention output stands in for everything up to it
                TM("attn_reuse", ar.load, li, att)
            else:
                TM("ln_mod", _lib.layernorm_modulate, x, y, L["norm1_w"], L["norm1_b"], mod, mod, self.mod_cols, N, S, D,
                   T, cfg.norm_eps, scale_off=m1 + 2 * D, shift_off=m1)
                qk_call = ((y, L["wqk"], qk, S, 2 * D, D, D, D, 2 * D), dict(bias=L["bqk"], batch=N, strideA=S * D, strideC=S * 2 * D))
                vt_call = ((L["wv"], y, vt, D, S, D, D, D, S_pad), dict(bias=L["bv"], batch=N, strideB=S * D, strideC=D * S_pad,
                                                                       flags=_lib.GEMM_BIAS_PER_ROW | _lib.GEMM_PERMUTE_COLS))
                # the softmax scale * log2(e) rides in Q's last rounding (attn_prescale = False: scaled per score in the attention)
                if self.pair_qkv and self.fuse_qk_norm:   # ... and QK LayerNorm + rope in the Q|K store loop: qk is written once
                    TM("gemm_qkv", _lib.gemm_pair_qk, qk_call, vt_call, L["norm_q_w"], L["norm_q_b"], L["norm_k_w"], L["norm_k_b"], cos, sin,
                                   Hn, T, cfg.qk_norm_eps, q_scale=q_scale)
                else:
                    if self.pair_qkv:   # both projections read y: ONE persistent launch, the two partial last rounds become one
                        TM("gemm_qkv", _lib.gemm_pair, qk_call, vt_call)
                    else:
                        TM("gemm_qk", G, *qk_call[0], **qk_call[1])
                        TM("gemm_vt", G, *vt_call[0], **vt_call[1])
                    TM("qk_norm_rope", _lib.qk_norm_rope_, qk, L["norm_q_w"], L["norm_q_b"], L["norm_k_w"], L["norm_k_b"], cos, sin, N, S, Hn, T,
                                       cfg.qk_norm_eps, q_scale=q_scale)
                self._attention(ws, plan, li, N, S, T, scale, prescale)
                if ar is not None:
                    TM("attn_reuse", ar.store, li, att)
            TM("gemm_out", G, att, L[wo_k], x, S, D, D, D, D, D, bias=L["bo"], R=x, ldr=D, gate=mod, gate_off=m1 + 4 * D,
              strideGate=self.mod_cols, seg_split=T, batch=N, strideA=S * D, strideC=S * D, strideR=S * D)
            if fp4:
                self._ff_fp4(L, ws, N, S, T, m2)
                continue
            TM("ln_mod", _lib.layernorm_modulate, x, y, L["norm2_w"], L["norm2_b"], mod, mod, self.mod_cols, N, S, D,
               T, cfg.norm_eps, scale_off=m2 + 2 * D, shift_off=m2)
            TM("gemm_ff1", G, y, L[wf1_k], h, S, F4, D, D, D, F4, bias=L["bf1"], act=_lib.ACT_GELU_TANH, batch=N, strideA=S * D,
              strideC=S * F4)
            TM("gemm_ff2", G, h, L[wf2_k], x, S, D, F4, F4, F4, D, bias=L["bf2"], R=x, ldr=D, gate=mod, gate_off=m2 + 4 * D,
              strideGate=self.mod_cols, seg_split=T, batch=N, strideA=S * F4, strideC=S * D, strideR=S * D)

        if sc is not None:
            if len(self.layers) == 1:  # no tail to skip: the probe and the rule run all the same (x + 0 on a hit)
                TM("step_cache", sc.after_block0, x)
            TM("step_cache", sc.end, x)   # computed forward: tail <- x - x1 (a no-op behind a hit)

        plan.finish()
        if ar is not None:
            ar.finish()

        # 4. norm_final over the joint sequence, AdaLayerNorm on the video tokens, proj_out, unpatchify
        _lib.layernorm_modulate(x, y, self.norm_final_w, self.norm_final_b, None, None, 0, N, S, D, T, cfg.norm_eps)
        mo = cfg.num_layers * 12 * D   # norm_out: shift pair @+0, scale pair @+2D
        _lib.layernorm_modulate(y, att, self.norm_out_w, self.norm_out_b, mod, mod, self.mod_cols, N, P, D, 0,
                                cfg.norm_eps, x_bstride=S * D, y_bstride=P * D, x_off=T * D, scale_off=mo + 2 * D,
                                shift_off=mo)
        n_out = self.w_out.shape[0]
        G(att, self.w_out, ws["po"], N * P, n_out, D, D, D, n_out, bias=self.b_out)
        out = torch.empty(N, Fr, cfg.out_channels, Hh, Ww, device=self.device, dtype=torch.bfloat16)
        _lib.unpatchify(ws["po"], out, N, Fr, cfg.out_channels, Hh, Ww, p, p_t)
        return out

    def __call__(self, hidden_states, encoder_hidden_states, timestep, timestep_cond=None, ofs=None,
                 image_rotary_emb=None, attention_kwargs=None, return_dict=True, cache_keys=None, cache_force=False):
        """diffusers-style entry: hidden_states [N, F, 2C, H, W] (latents and condition already concatenated on
        the channel axis, cog:1068-1070)."""
        if timestep_cond is not None:
            raise NotImplementedError("timestep_cond is not used by the CogVideoX I2V checkpoints")
        C = hidden_states.shape[2] // 2
        lat = hidden_states[:, :, :C].contiguous()
        conds = [hidden_states[n:n + 1, :, C:].contiguous() for n in range(hidden_states.shape[0])]
        out = self.forward_assembled(lat, conds, encoder_hidden_states, timestep, image_rotary_emb, ofs=ofs,
                                     cache_keys=cache_keys, cache_force=cache_force)
        if not return_dict:
            return (out,)
        return TransformerOutput(sample=out)


@dataclass
class TransformerOutput:
    sample: torch.Tensor
