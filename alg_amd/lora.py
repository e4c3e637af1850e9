"""LoRA adapters, merged at load time (an extension; the reference pipelines inherit diffusers' LoRA loader mixins).

The adapters are merged INTO THE STATE DICT, before a transformer is built from it: W <- bf16(W + sum_i scale_i * B_i @ A_i), one
launch of alg_lora_merge per targeted weight.  The constructors and forwards never hear of LoRA, so every derived form of a
weight (concatenated, packed in fragment order, e4m3, MXFP4) is made from the merged weight by the code that makes it anyway,
and "unload" is building the model without the adapter.  There is no load / unload on a built model.

Importing this module and parsing adapter files needs no GPU; only `merge_into` launches a kernel.

Adapter format: a `.safetensors` file on local disk, or a `{key: tensor}` dict (an optional "__metadata__" entry holds what the
file's header would), with diffusers / PEFT module paths and an optional leading "transformer.":
    <module>.lora_A.weight  [r, K]      <module>.lora_B.weight  [N, r]       (lora_down / lora_up are synonyms)
    <module>.alpha          scalar, optional
alpha = the module's own `.alpha`, else the file metadata's global `lora_alpha`, else r; the rank always comes from the shapes.
Everything else is refused with a ValueError that names the first offending key -- nothing is skipped silently.
"""
from __future__ import annotations

import math
import os
import re
from collections import OrderedDict, namedtuple

import torch

MAX_RANK = 512          # alg_lora_merge: the combined rank of all adapters of one weight
K_GRANULE = 8           # alg_lora_merge: K % 8 == 0

LoraSpec = namedtuple("LoraSpec", "source scale name")
LoraReport = namedtuple("LoraReport", "name scale targets ranks")
# one targeted weight: the state-dict key, A [R, K], B [N, R] and scale [R], fp32, the adapters concatenated along R in list order
MergeItem = namedtuple("MergeItem", "key a b scale")

_A_SUFFIXES = (".lora_A.weight", ".lora_down.weight")
_B_SUFFIXES = (".lora_B.weight", ".lora_up.weight")
_ALPHA_SUFFIX = ".alpha"
# original-format (non-diffusers) names: ComfyUI / kohya prefixes, HunyuanVideo's double_blocks / single_blocks / img_attn / txt_attn,
# Wan's self_attn / cross_attn / ffn.<n>
_ORIGINAL = re.compile(r"^(diffusion_model\.|lora_unet_|lora_te)|(^|\.)(double_blocks|single_blocks)\.|\.(img|txt)_(attn|mlp|mod)|"
                       r"\.(self_attn|cross_attn)\.|\.ffn\.\d+(\.|$)")


def _is_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def _one_spec(item, index):
    if isinstance(item, LoraSpec):
        source, scale, name = item
    elif isinstance(item, (str, os.PathLike)):
        source, scale, name = item, 1.0, None
    elif isinstance(item, tuple):
        if len(item) != 2:
            raise ValueError("lora: a tuple spec is (path_or_dict, scale), got %d entries" % len(item))
        source, scale, name = item[0], item[1], None
    elif isinstance(item, dict):
        unknown = sorted(set(item) - {"path", "scale", "name"})
        if "path" not in item or unknown:
            raise ValueError("lora: a dict spec is {'path': ..., 'scale': ..., 'name': ...}%s"
                             % (", got the unknown key %r" % unknown[0] if unknown else ", 'path' is missing"))
        source, scale, name = item["path"], item.get("scale", 1.0), item.get("name")
    else:
        raise ValueError("lora: a spec is a path, (path_or_dict, scale) or {'path', 'scale', 'name'}, got %r" % type(item).__name__)
    if not isinstance(source, (str, os.PathLike, dict)):
        raise ValueError("lora: the adapter is a path or a {key: tensor} dict, got %r" % type(source).__name__)
    if not _is_number(scale) or not math.isfinite(scale):
        raise ValueError("lora: the scale of an adapter is a finite number, got %r" % (scale,))
    if name is None:
        name = ("adapter%d" % index if isinstance(source, dict)
                else os.path.splitext(os.path.basename(os.fspath(source)))[0])
    return LoraSpec(source if isinstance(source, dict) else os.fspath(source), float(scale), str(name))


def parse_specs(lora):
    """`lora=` as the models, the pipelines and run.py take it -> a tuple of LoraSpec(source, scale, name).  One spec is a path,
    (path_or_dict, scale) or {"path": path_or_dict, "scale": s, "name": n}; `lora` is one spec or a list of them; None or an
    empty list is no adapter."""
    if lora is None:
        return ()
    many = isinstance(lora, list) or (isinstance(lora, tuple) and not isinstance(lora, LoraSpec)
                                      and all(isinstance(x, LoraSpec) for x in lora))     # (what this function returned)
    items = list(lora) if many else [lora]
    return tuple(_one_spec(item, i) for i, item in enumerate(items))


def read_adapter(source):
    """A `.safetensors` path or a {key: tensor} dict -> (tensors, metadata)."""
    if isinstance(source, dict):
        meta = source.get("__metadata__") or {}
        return {k: v for k, v in source.items() if k != "__metadata__"}, dict(meta)
    if not os.path.isfile(source):
        raise FileNotFoundError("lora: adapter file %s not found (adapters are read from local disk)" % source)
    from safetensors import safe_open

    with safe_open(source, framework="pt", device="cpu") as f:
        meta = dict(f.metadata() or {})
        tensors = {k: f.get_tensor(k) for k in f.keys()}
    return tensors, meta


def parse_adapter(tensors, metadata=None):
    """The key grammar: {key: tensor} -> OrderedDict module -> (A [r, K] fp32, B [N, r] fp32, alpha), in the file's key order.
    Refuses (ValueError naming the key) whatever is outside the grammar."""
    metadata = metadata or {}
    global_alpha = None
    if metadata.get("lora_alpha") is not None:
        try:
            global_alpha = float(metadata["lora_alpha"])
        except (TypeError, ValueError):
            raise ValueError("lora: the metadata's lora_alpha = %r is not a number" % (metadata["lora_alpha"],))
    parts = OrderedDict()
    for key, t in tensors.items():
        module = key[len("transformer."):] if key.startswith("transformer.") else key
        if module.startswith(("text_encoder.", "text_encoder_2.")):
            raise ValueError("lora: %r targets a text encoder; only transformer adapters are built" % key)
        if module.endswith(".bias"):
            raise ValueError("lora: %r is a bias term; adapters with biases (lora_B.bias) are not built" % key)
        if "lora_magnitude_vector" in module or module.endswith(".dora_scale"):
            raise ValueError("lora: %r is a DoRA magnitude vector; DoRA adapters are not built" % key)
        if _ORIGINAL.search(module):
            raise ValueError("lora: %r is an original-format (non-diffusers) key name; such names are not converted -- export the "
                             "adapter with diffusers / PEFT module paths" % key)
        for suffixes, slot in ((_A_SUFFIXES, "A"), (_B_SUFFIXES, "B"), ((_ALPHA_SUFFIX,), "alpha")):
            hit = [s for s in suffixes if module.endswith(s)]
            if hit:
                name = module[:-len(hit[0])]
                break
        else:
            raise ValueError("lora: %r is outside the key grammar (<module>.lora_A.weight, <module>.lora_B.weight, their "
                             "lora_down / lora_up synonyms, <module>.alpha)" % key)
        entry = parts.setdefault(name, {})
        if not name or slot in entry:
            raise ValueError("lora: %r %s" % (key, "names no module" if not name else "is the second %s of its module" % slot))
        entry[slot] = (key, t)
    out = OrderedDict()
    for name, entry in parts.items():
        for have, need in (("A", "B"), ("B", "A"), ("alpha", "A")):
            if have in entry and need not in entry:
                raise ValueError("lora: %r has no lora_%s beside it" % (entry[have][0], need))
        (ka, a), (kb, b) = entry["A"], entry["B"]
        if a.dim() != 2 or b.dim() != 2:
            bad = ka if a.dim() != 2 else kb
            raise ValueError("lora: %r is not 2-D (shape %s); only linear layers are targeted" % (bad, tuple(tensors[bad].shape)))
        if b.shape[1] != a.shape[0] or a.shape[0] < 1:
            raise ValueError("lora: %r [N, r] = %s does not fit lora_A [r, K] = %s" % (kb, tuple(b.shape), tuple(a.shape)))
        r = a.shape[0]
        alpha = float(r) if global_alpha is None else global_alpha
        if "alpha" in entry:
            kal, al = entry["alpha"]
            if al.numel() != 1:
                raise ValueError("lora: %r must be a scalar, got shape %s" % (kal, tuple(al.shape)))
            alpha = float(al.reshape(()).double())
        out[name] = (a.to(torch.float32), b.to(torch.float32), alpha)     # fp16 / bf16 / fp32 upcast exactly
    return out


def plan_merge(state_dict, specs):
    """(items, report) without touching a GPU or the state dict: a MergeItem per targeted weight, in first-appearance order, with
    the adapters' A, B and per-column scale (user scale * alpha / r) concatenated along R in list order; the report is a tuple
    of LoraReport(name, scale, targets, ranks) per adapter.  Every target is checked against the state dict."""
    specs = parse_specs(specs)
    per_key, report = OrderedDict(), []
    for spec in specs:
        tensors, meta = read_adapter(spec.source)
        modules = parse_adapter(tensors, meta)
        ranks = set()
        for module, (a, b, alpha) in modules.items():
            key = module + ".weight"
            if key not in state_dict:
                raise ValueError("lora: adapter %r targets %r, which is not in the model's state dict" % (spec.name, module))
            w = state_dict[key]
            if w.dim() != 2:
                raise ValueError("lora: adapter %r targets %r, whose weight is not 2-D (shape %s); only linear layers are merged"
                                 % (spec.name, module, tuple(w.shape)))
            if (b.shape[0], a.shape[1]) != tuple(w.shape):
                raise ValueError("lora: adapter %r, module %r: B @ A is %s, the weight is %s"
                                 % (spec.name, module, (b.shape[0], a.shape[1]), tuple(w.shape)))
            if w.shape[1] % K_GRANULE:
                raise ValueError("lora: module %r has K = %d input features; the merge kernel takes multiples of %d"
                                 % (module, w.shape[1], K_GRANULE))
            r = a.shape[0]
            ranks.add(r)
            per_key.setdefault(key, []).append((a, b, torch.full((r,), spec.scale * alpha / r, dtype=torch.float32)))
        report.append(LoraReport(spec.name, spec.scale, len(modules), tuple(sorted(ranks))))
    items = []
    for key, group in per_key.items():
        total = sum(a.shape[0] for a, _, _ in group)
        if total > MAX_RANK:
            raise ValueError("lora: the adapters of %r have a combined rank of %d, the merge kernel takes at most %d"
                             % (key[:-len(".weight")], total, MAX_RANK))
        items.append(MergeItem(key, torch.cat([a for a, _, _ in group], dim=0).contiguous(),
                               torch.cat([b for _, b, _ in group], dim=1).contiguous(), torch.cat([s for _, _, s in group])))
    return items, tuple(report)


def merge_into(state_dict, specs, device="cuda"):
    """Merge the adapters of `specs` into `state_dict` IN PLACE and return the report (plan_merge).  A targeted `<module>.weight`
    is moved to `device` in its own dtype (bf16 or fp32; anything else is upcast to fp32 exactly), merged by one alg_lora_merge
    launch and put back as a bf16 device tensor -- a bf16 weight that already lies on the device is replaced by a new tensor,
    the caller's own is left as it was; untargeted entries are neither touched nor moved.  A scale of 0 still runs and gives bf16(W)."""
    from . import _lib

    items, report = plan_merge(state_dict, specs)
    dev = torch.device(device)
    if items and dev.type != "cuda":
        raise _lib.AlgHipError("lora.merge_into runs on the GPU only (alg_lora_merge, no CPU fallback)")
    for it in items:
        w = state_dict[it.key]
        if w.dtype not in (torch.bfloat16, torch.float32):
            w = w.to(torch.float32)
        w = w.to(dev)
        if w.stride(1) != 1 or w.stride(0) % K_GRANULE or w.data_ptr() % 16:
            w = w.contiguous()
        state_dict[it.key] = _lib.lora_merge(w, it.a.to(dev), it.b.to(dev), it.scale.to(dev))
    return report


def build(cls, config, state_dict, lora, device, **ctor_kw):
    """cls(config, state_dict, device=device, **ctor_kw) with the adapters of `lora` merged into `state_dict` first (merge_into,
    in place); the report is the model's `lora_report`."""
    report = merge_into(state_dict, lora, device)
    model = cls(config, state_dict, device=device, **ctor_kw)
    model.lora_report = report
    return model
