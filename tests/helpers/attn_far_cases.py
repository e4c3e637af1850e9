"""The three small trained-like DiTs of helpers/attn_reuse_cases.py (Family) at latent-frame counts where a frame window of 1 is
narrower than the video -- 11 / 5 / 7 frames for CogVideoX / Wan / HunyuanVideo, the counts tests/test_gpu_sampler_ext.py uses --
with the fp32 oracle of the same inputs.  Shared by tests/test_gpu_attn_far_models.py.

    fam = FarFamily("cog"); model = fam.build(); inp = fam.inputs(n, seed, t); out = fam.run(model, inp, keys, force)
    ref = fam.oracle(inp)        the fp32 oracle's forward of the same inputs (CPU)"""
import torch

from helpers.attn_reuse_cases import BF, DEV, Family
from helpers.trained_like_cases import cog_case, hy_case, wan_case
from oracle import dit_oracle, hy_oracle, wan_oracle

FRAMES = dict(cog=11, wan=5, hy=7)


class FarFamily(Family):
    def __init__(self, name):
        super().__init__(name)
        self.frames = FRAMES[name]
        getattr(self, "_far_" + name)()

    def _far_cog(self):
        kw, ocfg, wbf, _ = cog_case("small")
        w32 = {k: v.float() for k, v in wbf.items()}
        ropes = {}

        def rope(frames):
            if frames not in ropes:
                ropes[frames] = dit_oracle.rope_tables(ocfg, 8 * 8, 12 * 8, frames)
            return ropes[frames]

        def inputs(n, seed, t, frames=None):
            frames = self.frames if frames is None else frames
            g = torch.Generator().manual_seed(seed)
            hs = torch.randn(n, frames, kw["in_channels"], 8, 12, generator=g).to(BF)
            ehs = torch.randn(n, 10, kw["text_embed_dim"], generator=g).to(BF)
            return dict(hs=hs.to(DEV), ehs=ehs.to(DEV), ts=torch.tensor([t] * n), t=t, frames=frames)

        def run(model, inp, keys=None, force=False):
            kw_ = {} if keys is None else dict(cache_keys=keys, cache_force=force)
            return model(inp["hs"], inp["ehs"], inp["ts"], image_rotary_emb=rope(inp["frames"]), return_dict=False, **kw_)[0].clone()

        def oracle(inp):
            return dit_oracle.dit_forward(ocfg, w32, inp["hs"].cpu().float(), inp["ehs"].cpu().float(), inp["ts"], rope(inp["frames"]))

        self.inputs, self.run, self.oracle = inputs, run, oracle

    def _far_wan(self):
        kw, ocfg, sd, _ = wan_case("small")

        def inputs(n, seed, t, frames=None):
            frames = self.frames if frames is None else frames
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(n, 36, frames, 16, 24, generator=g).to(BF)
            txt, img = torch.randn(n, 512, 64, generator=g).to(BF), torch.randn(n, 257, 64, generator=g).to(BF)
            return dict(x=x.to(DEV), ts=torch.tensor([float(t)] * n).to(DEV), txt=txt.to(DEV), img=img.to(DEV), t=t)

        def oracle(inp):
            return wan_oracle.wan_forward(ocfg, sd, inp["x"].cpu().float(), inp["ts"].cpu(), inp["txt"].cpu().float(),
                                          inp["img"].cpu().float())

        self.inputs, self.oracle = inputs, oracle

    def _far_hy(self):
        kw, ocfg, sd, _ = hy_case("token_replace")
        sd32 = {k: v.float() for k, v in sd.items()}

        def inputs(n, seed, t, frames=None):
            frames = self.frames if frames is None else frames
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(n, 16, frames, 16, 16, generator=g).to(BF)
            txt, pooled = torch.randn(n, 20, 64, generator=g).to(BF), torch.randn(n, 64, generator=g).to(BF)
            mask = torch.zeros(n, 20)
            for b in range(n):
                mask[b, :(13, 20, 7)[b % 3]] = 1
            return dict(x=x.to(DEV), ts=torch.tensor([float(t)] * n).to(DEV), txt=txt.to(DEV), mask=mask.to(DEV).to(BF),
                        pooled=pooled.to(DEV), t=t)

        def oracle(inp):
            return hy_oracle.hy_forward(ocfg, sd32, inp["x"].cpu().float(), inp["ts"].cpu(), inp["txt"].cpu().float(),
                                        inp["mask"].cpu().float(), inp["pooled"].cpu().float(), None)

        self.inputs, self.oracle = inputs, oracle
