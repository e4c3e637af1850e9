#!/usr/bin/env python3
"""Launch trace of the three DiTs' self-attention: every _lib.flash_attn_*, attn_lse_recall, attn_prefix_mass,
attn_rows_position_major and attn_vt_position_major call of the small Wan and HunyuanVideo set-ups of
tests/test_gpu_attn_window_models.py and the CogVideoX one of tests/test_gpu_attn_window_cogvideox.py, through every mode of the
launch ladder: window off, shared window, recall set but uncalibrated, the calibration forward, calibrated with mixed heads
(decisions forced as test_mixed_heads_forward_is_exact_to_the_dense_standard forces them), the same with attn_window_balance,
attn_window_widths (Wan; HunyuanVideo at nine frames, as five are inside a window of 2), attn_band (Wan), fp8_attention (Wan,
HunyuanVideo), and CogVideoX fp8=True with a window.

One line per launch: the wrapper, every argument by the wrapper's own parameter name with its defaults filled in (a tensor as the
workspace / calibration / band-scratch buffer its data_ptr falls in, a table as its type and the SHA-256 of its host copy), and
the profile key the launch was timed under ("-": not timed; a launch counts for the first attn* key recorded behind it).  One line
per forward with the SHA-256 of its output.  Two trees that launch alike print the same text: run it on both and diff.
usage: python scripts/probes/self_attn_launches.py [> trace.txt]      (needs the GPU)"""
import hashlib
import inspect
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
WRAPPED = ("attn_lse_recall", "attn_prefix_mass", "attn_rows_position_major", "attn_vt_position_major")


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch

    import test_gpu_attn_window_cogvideox as C
    import test_gpu_attn_window_models as M
    from alg_amd import _lib, attn_window
    from alg_amd.transformer_cogvideox import CogVideoXTransformer3DModel
    from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel
    from alg_amd.transformer_wan import WanTransformer3DModel

    DEV = M.DEV
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
    pending = []          # [wrapper, bound arguments, key] of the launches of the forward under way

    class Keys(dict):
        """model.profile: the models append their event pairs under setdefault(key, [])"""
        def setdefault(self, key, default=None):
            for rec in pending:
                if rec[2] is None:
                    rec[2] = key if key.startswith("attn") else "-"
            return dict.setdefault(self, key, default)

    def wrap(name):
        real = getattr(_lib, name)
        sig = inspect.signature(real)

        def recorded(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            pending.append([name, dict(b.arguments), None])
            return real(*a, **kw)

        setattr(_lib, name, recorded)

    for name in sorted(n for n in dir(_lib) if n.startswith("flash_attn_") or n in WRAPPED):
        if callable(getattr(_lib, name)):
            wrap(name)

    def buffers(model):
        """name -> tensor of the model's workspace, calibration buffers and band scratch (resolved behind the forward)"""
        out = {}
        for prefix, holder in (("ws", list(getattr(model, "_ws", {}).values())), ("cal", [getattr(model, "_attn_cal", None)]),
                               ("band", [getattr(model, "_band_ws", None)])):
            for h in holder:
                for k, v in (h if isinstance(h, dict) else vars(h) if h is not None else {}).items():
                    if torch.is_tensor(v) and v.is_cuda:
                        out["%s.%s" % (prefix, k)] = v
        return out

    def show(v, bufs):
        if torch.is_tensor(v):
            for n, t in bufs.items():
                if t.data_ptr() <= v.data_ptr() < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                    return n if v.data_ptr() == t.data_ptr() else "%s+%d" % (n, v.data_ptr() - t.data_ptr())
            return "tensor%s" % (tuple(v.shape),)
        host = getattr(v, "table", getattr(v, "order", None))
        if torch.is_tensor(host):
            return "%s:%s" % (type(v).__name__, sha(host))
        return repr(round(v, 9) if isinstance(v, float) else v)

    def forward(label, model, run, calibrate=False):
        del pending[:]
        model.profile = Keys()
        out = run(model, calibrate)
        torch.cuda.synchronize()
        model.profile = None
        bufs = buffers(model)
        print("== %s" % label)
        for name, args, key in pending:
            if name in ("attn_lse_recall", "attn_prefix_mass") and args["rows"] is None:
                args["rows"] = args["Sq"] - args["row0"]
            print("%s [%s] %s" % (name, key or "-", " ".join("%s=%s" % (k, show(v, bufs)) for k, v in args.items())))
        print("output %s" % sha(out), flush=True)

    def forced(name, fn):
        """attn_window.<name> replaced for one calibration forward: the decisions do not depend on the recalls' last bits"""
        class Ctx:
            def __enter__(self):
                self.real = getattr(attn_window, name)
                setattr(attn_window, name, fn)

            def __exit__(self, *exc):
                setattr(attn_window, name, self.real)
        return Ctx()

    alternate = lambda recall, thr: [h % 2 == 0 for h in range(len(recall[0]))]

    def ladder(tag, model, run):
        """the modes every model has"""
        forward(tag + " window off", model, run)
        model.attn_window = 1
        forward(tag + " shared window", model, run)
        model.attn_window_recall = 0.5
        forward(tag + " recall, uncalibrated", model, run)
        with forced("decide_heads", alternate):
            forward(tag + " calibration", model, run, calibrate=True)
        forward(tag + " mixed heads", model, run)
        model.attn_window_balance = "units"
        forward(tag + " mixed heads, balanced", model, run)
        model.attn_window_balance = False
        model.reset_attn_window_heads()

    def widths(tag, model, run):
        model.attn_window, model.attn_window_recall, model.attn_window_widths = 2, 0.5, (1, 2)
        with forced("decide_widths", lambda recall, ws, thr: [(1, 0, 2, 1)[h % 4] for h in range(len(recall[0]))]):
            forward(tag + " widths calibration", model, run, calibrate=True)
        forward(tag + " widths tables", model, run)
        model.attn_window_balance = "lanes"
        forward(tag + " widths tables, balanced", model, run)
        model.attn_window_balance, model.attn_window_widths = False, None
        model.reset_attn_window_heads()

    call = attn_window.call_transformer

    # ---- Wan
    cfg, sd, (x, t, txt, img) = M._wan_setup()
    model = WanTransformer3DModel(cfg, sd, device=DEV)
    run = lambda m, cal: call(m, False, x.to(DEV), t.to(DEV), txt.to(DEV), img.to(DEV), return_dict=False, calibrate=cal)[0].clone()
    ladder("wan", model, run)
    widths("wan", model, run)
    model.attn_window, model.attn_window_recall, model.attn_band = 1, 0.5, 2
    layouts = iter([["band", "window", "dense", "band"], ["band"] * M.HEADS])      # layer 1: no main launch
    with forced("decide_layouts", lambda rw, rb, cw, cb, thr: next(layouts)):
        forward("wan band calibration", model, run, calibrate=True)
    forward("wan band tables", model, run)
    model.attn_window_balance = "units"
    forward("wan band tables, balanced", model, run)
    model.attn_window_balance, model.attn_band, model.attn_window, model.attn_window_recall = False, 0, 0, 0.0
    model.reset_attn_window_heads()
    model.fp8_attention = True
    forward("wan fp8_attention", model, run)
    del model

    # ---- HunyuanVideo
    cfg, sd, (x, t, txt, mask, pooled) = M._hy_setup()
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    run = lambda m, cal: call(m, False, hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                              encoder_attention_mask=mask.to(DEV).to(M.BF), pooled_projections=pooled.to(DEV), return_dict=False,
                              calibrate=cal)[0].clone()
    ladder("hunyuan", model, run)
    model.attn_window, model.attn_window_recall = 0, 0.0
    model.fp8_attention = True
    forward("hunyuan fp8_attention", model, run)
    M.HY_F = 9            # (with five frames a window of 2 covers the video: the widths tests' nine)
    cfg, sd, (x, t, txt, mask, pooled) = M._hy_setup()
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    widths("hunyuan F=9", model, run)
    del model

    # ---- CogVideoX, bf16 and fp8 blocks
    for fp8 in (False, True):
        cfg, wbf, (hs, ehs, ts, rope) = C._setup()
        model = CogVideoXTransformer3DModel(cfg, wbf, device=DEV, fp8=fp8)
        run = lambda m, cal: call(m, False, hs, ehs, ts, image_rotary_emb=rope, return_dict=False, calibrate=cal)[0].clone()
        ladder("cogvideox fp8" if fp8 else "cogvideox", model, run)
        del model


if __name__ == "__main__":
    main()
