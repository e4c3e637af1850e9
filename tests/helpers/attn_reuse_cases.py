"""The three small trained-like DiTs (tests/helpers/trained_like_cases.py: cog_case, wan_case, hy_case) as the attention-reuse
tests drive them: one `Family` per model with its weights, seeded inputs of any batch size at the case's shapes, and a forward
that takes cache keys.  Shared by tests/test_gpu_attn_reuse_models.py and the samplers of tests/helpers/sampler_cases.py."""
import torch

from alg_amd import transformer_cogvideox, transformer_hunyuan_video, transformer_wan
from alg_amd.attn_reuse import StepKeys
from helpers.trained_like_cases import cog_case, hy_case, wan_case

DEV = "cuda:0"
BF = torch.bfloat16
ROLES = ["uncond_init", "uncond", "cond"]


class Family:
    """name, module (where the seam launch_self_attention is looked up), layers, build(fp8) -> model, inputs(n, seed, t),
    run(model, inputs, keys=None, force=False) -> the forward's output (a clone)"""

    def __init__(self, name):
        self.name = name
        getattr(self, "_" + name)()

    # ---- CogVideoX: small, 2 layers, 10 prompt + 144 video tokens
    def _cog(self):
        kw, ocfg, wbf, (_, _, _, rope) = cog_case("small")
        self.module, self.layers = transformer_cogvideox, kw["num_layers"]
        cfg = transformer_cogvideox.CogVideoXTransformerConfig(**kw)
        self.build = lambda fp8=False: transformer_cogvideox.CogVideoXTransformer3DModel(cfg, wbf, device=DEV, fp8=fp8)

        def inputs(n, seed, t):
            g = torch.Generator().manual_seed(seed)
            hs = torch.randn(n, 3, kw["in_channels"], 8, 12, generator=g).to(BF)
            ehs = torch.randn(n, 10, kw["text_embed_dim"], generator=g).to(BF)
            return dict(hs=hs.to(DEV), ehs=ehs.to(DEV), ts=torch.tensor([t] * n), t=t)

        def run(model, inp, keys=None, force=False):
            kw_ = {} if keys is None else dict(cache_keys=keys, cache_force=force)
            return model(inp["hs"], inp["ehs"], inp["ts"], image_rotary_emb=rope, return_dict=False, **kw_)[0].clone()

        self.inputs, self.run = inputs, run

    # ---- Wan: small, 2 layers, 288 tokens, text + image cross-attention
    def _wan(self):
        kw, ocfg, sd, _ = wan_case("small")
        self.module, self.layers = transformer_wan, kw["num_layers"]
        cfg = transformer_wan.WanTransformerConfig(**kw)
        self.build = lambda fp8=False: transformer_wan.WanTransformer3DModel(cfg, sd, device=DEV, fp8=fp8)

        def inputs(n, seed, t):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(n, 36, 3, 16, 24, generator=g).to(BF)
            txt, img = torch.randn(n, 512, 64, generator=g).to(BF), torch.randn(n, 257, 64, generator=g).to(BF)
            return dict(x=x.to(DEV), ts=torch.tensor([float(t)] * n).to(DEV), txt=txt.to(DEV), img=img.to(DEV), t=t)

        def run(model, inp, keys=None, force=False):
            kw_ = {} if keys is None else dict(cache_keys=keys, cache_force=force)
            return model(inp["x"], inp["ts"], inp["txt"], inp["img"], return_dict=False, **kw_)[0].clone()

        self.inputs, self.run = inputs, run

    # ---- HunyuanVideo: token_replace, 1 dual + 1 single block, 192 latent + 20 prompt rows, ragged prompt lengths
    def _hy(self):
        kw, ocfg, sd, _ = hy_case("token_replace")
        self.module, self.layers = transformer_hunyuan_video, kw["num_layers"] + kw["num_single_layers"]
        cfg = transformer_hunyuan_video.HunyuanVideoTransformerConfig(**kw)
        self.build = lambda fp8=False: transformer_hunyuan_video.HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=fp8)

        def inputs(n, seed, t):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(n, 16, 3, 16, 16, generator=g).to(BF)
            txt, pooled = torch.randn(n, 20, 64, generator=g).to(BF), torch.randn(n, 64, generator=g).to(BF)
            mask = torch.zeros(n, 20)
            for b in range(n):
                mask[b, :(13, 20, 7)[b % 3]] = 1
            return dict(x=x.to(DEV), ts=torch.tensor([float(t)] * n).to(DEV), txt=txt.to(DEV), mask=mask.to(DEV).to(BF),
                        pooled=pooled.to(DEV), t=t)

        def run(model, inp, keys=None, force=False):
            kw_ = {} if keys is None else dict(cache_keys=keys, cache_force=force)
            return model(hidden_states=inp["x"], timestep=inp["ts"], encoder_hidden_states=inp["txt"],
                         encoder_attention_mask=inp["mask"], pooled_projections=inp["pooled"], return_dict=False, **kw_)[0].clone()

        self.inputs, self.run = inputs, run


def keys_at(roles, t):
    return StepKeys(list(roles), t)


class Seam:
    """attn_window.launch_self_attention as the family's transformer module sees it, replaced for the length of a `with`.
    mode "record": every launch runs, and the rows it wrote are kept per (layer, sample).  mode "replay": nothing is launched; the
    rows recorded for (layer, rows[sample]) are written where the launch would have written them."""

    def __init__(self, fam, samples, mode, recorded=None, rows=None):
        self.fam, self.samples, self.mode = fam, samples, mode
        self.recorded = {} if recorded is None else recorded
        self.rows = list(range(samples)) if rows is None else list(rows)
        self.calls = 0

    def _views(self, ops):
        W = ops.heads * ops.head_dim
        return torch.as_strided(ops.o, (ops.batch, ops.Sq, W), (ops.o_bs, ops.o_rs, 1), ops.o.storage_offset() + ops.o_off)

    def __call__(self, timed, name, ops, table, order=None):
        groups = self.samples // ops.batch                      # launches per layer: 1 (the whole batch), or one per sample
        layer, s0 = self.calls // groups, (self.calls % groups) * ops.batch
        self.calls += 1
        out = self._views(ops)
        if self.mode == "record":
            self.real(timed, name, ops, table, order)
            for b in range(ops.batch):
                self.recorded[(layer, s0 + b)] = out[b].clone()
        else:
            for b in range(ops.batch):
                out[b].copy_(self.recorded[(layer, self.rows[s0 + b])])

    def __enter__(self):
        self.real = self.fam.module.launch_self_attention
        self.fam.module.launch_self_attention = self
        return self

    def __exit__(self, *exc):
        self.fam.module.launch_self_attention = self.real
