"""Test-side LoRA reference: seeded adapters in the diffusers / PEFT key grammar and the float64 merge
W + sum_i scale_i * alpha_i / r_i * B_i @ A_i.  It shares no code with alg_amd/lora.py: keys are read here again, from the
grammar's definition, so that a parsing mistake there does not cancel out."""
import torch

A_NAMES = ("lora_A.weight", "lora_down.weight")
B_NAMES = ("lora_B.weight", "lora_up.weight")


def make_adapter(state_dict, modules, rank, seed, rel_std=1.0, alpha=None, prefix="transformer.", names=("lora_A", "lora_B"),
                 dtype=torch.float32):
    """{key: tensor} for `modules` (names without ".weight") at `rank`.  A ~ N(0, 1 / K) and B ~ N(0, s^2), s chosen so that
    the delta B @ A * (alpha / rank) has `rel_std` times the standard deviation of the weight it is added to.  `alpha` = None
    writes no alpha entry (alpha = rank); values are rounded to `dtype` (what a file of that dtype holds)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for m in modules:
        w = state_dict[m + ".weight"]
        N, K = w.shape
        a = torch.randn(rank, K, generator=g) / K ** 0.5
        gain = (alpha if alpha is not None else rank) / rank
        # std(sum_r B A) = sqrt(rank) * s / sqrt(K)
        s = rel_std * w.float().std().item() * K ** 0.5 / (rank ** 0.5 * gain)
        b = torch.randn(N, rank, generator=g) * s
        out["%s%s.%s.weight" % (prefix, m, names[0])] = a.to(dtype)
        out["%s%s.%s.weight" % (prefix, m, names[1])] = b.to(dtype)
        if alpha is not None:
            out["%s%s.alpha" % (prefix, m)] = torch.tensor(float(alpha))
    return out


def read_adapter(tensors, metadata=None):
    """module -> (A float64, B float64, alpha) by the grammar: optional "transformer." prefix, lora_A | lora_down, lora_B | lora_up,
    alpha = the module's `.alpha`, else the metadata's lora_alpha, else the rank."""
    mods = {}
    for key, t in tensors.items():
        k = key[len("transformer."):] if key.startswith("transformer.") else key
        for names, slot in ((A_NAMES, "A"), (B_NAMES, "B"), (("alpha",), "alpha")):
            for n in names:
                if k.endswith("." + n):
                    mods.setdefault(k[:-len(n) - 1], {})[slot] = t.double()
    out = {}
    for m, e in mods.items():
        r = e["A"].shape[0]
        alpha = float(e["alpha"]) if "alpha" in e else float((metadata or {}).get("lora_alpha", r))
        out[m] = (e["A"], e["B"], alpha)
    return out


def merge_ref64(state_dict, adapters):
    """`adapters`: a list of (tensors, scale[, metadata]).  Returns a copy of the state dict (CPU) whose targeted weights are
    (W.double() + sum scale * alpha / r * B.double() @ A.double()) as float64 tensors; untargeted entries are the caller's."""
    out = {k: v.cpu() for k, v in state_dict.items()}
    for ad in adapters:
        tensors, scale = ad[0], ad[1]
        for m, (a, b, alpha) in read_adapter(tensors, ad[2] if len(ad) > 2 else None).items():
            key = m + ".weight"
            out[key] = out[key].double() + (scale * alpha / a.shape[0]) * (b @ a)
    return out
