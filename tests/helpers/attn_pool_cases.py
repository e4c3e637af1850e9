"""The three small trained-like DiTs of helpers/attn_far_cases.py (11 / 5 / 7 latent frames) on LARGER frames, shared by
tests/test_gpu_attn_pool_models.py.  At the far-reuse test's frame sizes (24 / 96 / 64 tokens a frame) a near table widened to the
64 G key grid holds every key and nothing is left to pool; here a frame has 96 / 384 / 256 tokens, so that at window 1 and G = 2
or 4 some query blocks have far keys -- and CogVideoX's block with the prompt rows and HunyuanVideo's prompt rows have none.

    fam = PoolFamily("cog"); model = fam.build(); inp = fam.inputs(n, seed, t); out = fam.run(model, inp)
    fam.window_table()            the frame-window table the model builds for these inputs (window 1), on the CPU
    cog_oracle_errors(inp, G)     the fp32 CPU oracle of CogVideoX with its attention replaced by the window-only and by the pooled
                                  operator: (window-only, pooled) relative L2 against the dense oracle"""
import math

import torch

from alg_amd.attn_window import frame_window_ranges, ranges_to_mask
from helpers import attn_pool_ref as R
from helpers.attn_far_cases import FarFamily
from helpers.attn_reuse_cases import BF, DEV
from helpers.trained_like import trained_like
from helpers.trained_like_cases import COG_SMALL
from oracle import dit_oracle

HW = dict(cog=(16, 24), wan=(32, 48), hy=(32, 32))            # latent height x width: 96 / 384 / 256 tokens a frame
TOKENS = dict(cog=96, wan=384, hy=256)
HY_VALID = (13, 20, 7)                                        # helpers/attn_far_cases.py: the valid prompt keys of sample b % 3


class PoolFamily(FarFamily):
    def __init__(self, name):
        super().__init__(name)
        small = self.inputs
        h, w = HW[name]
        if name == "cog":
            # cog_case("small") on a 16 x 24 latent (its learned positional embedding is tied to the configured size)
            from alg_amd import transformer_cogvideox
            kw = dict(COG_SMALL, sample_width=w, sample_height=h)
            ocfg = dit_oracle.DiTConfig(**kw)
            wbf = {k: v.to(BF) for k, v in trained_like(dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)).items()}
            cfg = transformer_cogvideox.CogVideoXTransformerConfig(**kw)
            self.build = lambda fp8=False: transformer_cogvideox.CogVideoXTransformer3DModel(cfg, wbf, device=DEV, fp8=fp8)
            self.ocfg, self.w32 = ocfg, {k: v.float() for k, v in wbf.items()}
            self.rope = dit_oracle.rope_tables(ocfg, h * 8, w * 8, self.frames)

            def inputs(n, seed, t):
                g = torch.Generator().manual_seed(seed)
                hs = torch.randn(n, self.frames, kw["in_channels"], h, w, generator=g).to(BF)
                ehs = torch.randn(n, 10, kw["text_embed_dim"], generator=g).to(BF)
                return dict(hs=hs.to(DEV), ehs=ehs.to(DEV), ts=torch.tensor([t] * n), t=t, frames=self.frames)

            def run(model, inp, keys=None, force=False):
                kw_ = {} if keys is None else dict(cache_keys=keys, cache_force=force)
                return model(inp["hs"], inp["ehs"], inp["ts"], image_rotary_emb=self.rope, return_dict=False, **kw_)[0].clone()

            self.inputs, self.run = inputs, run
        else:
            def inputs(n, seed, t):
                inp = small(n, seed, t)
                g = torch.Generator().manual_seed(seed + 1000)
                c = inp["x"].shape[1]
                inp["x"] = torch.randn(n, c, self.frames, h, w, generator=g).to(BF).to(DEV)
                return inp

            self.inputs = inputs

    def window_table(self, sample=0):
        F_, hw = self.frames, TOKENS[self.name]
        if self.name == "cog":
            return frame_window_ranges(F_, hw, 1, prefix=10)
        if self.name == "hy":
            return frame_window_ranges(F_, hw, 1, tail=(F_ * hw, F_ * hw + HY_VALID[sample % 3]), rows=F_ * hw + 20)
        return frame_window_ranges(F_, hw, 1)


def cog_oracle_errors(fam, inp, G, monkeypatch):
    """(window-only, pooled) relative L2 of the fp32 CPU oracle's output against its dense output, sample 0 of `inp`."""
    window = fam.window_table()
    wm, near, pooled = ranges_to_mask(window), *(ranges_to_mask(t) for t in R.near_far_pooled(window, G)[::2])
    unit = R.LOG2E / math.sqrt(64.0)
    hs, ehs, ts = inp["hs"][:1].cpu().float(), inp["ehs"][:1].cpu().float(), inp["ts"][:1]

    def forward(attention):
        with monkeypatch.context() as mp:
            if attention is not None:
                mp.setattr(torch.nn.functional, "scaled_dot_product_attention", attention)
            return dit_oracle.dit_forward(fam.ocfg, fam.w32, hs, ehs, ts, fam.rope)

    dense = forward(None)
    win = forward(lambda q, k, v: R.windowed_ref(q, k, v, wm, unit).to(q.dtype))
    pool = forward(lambda q, k, v: R.operator_ref(q, k, v, near, pooled, G, unit).to(q.dtype))
    return R.rel_l2(win, dense), R.rel_l2(pool, dense)
