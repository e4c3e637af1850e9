"""LoRA at load time, the part that needs no GPU: the key grammar and its refusals, the three alpha sources, how several
adapters are concatenated along R, the `lora=` spec forms, run.py's --lora, and the argument check of alg_lora_merge (a refused
call returns before any HIP call, so host or null pointers are never dereferenced)."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch
from safetensors.torch import save_file

import alg_amd
from alg_amd import _lib, lora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
Q = "blocks.0.attn1.to_q"
F2 = "blocks.0.ffn.net.2"


def state_dict():
    return {Q + ".weight": torch.zeros(24, 16, dtype=torch.bfloat16), Q + ".bias": torch.zeros(24),
            F2 + ".weight": torch.zeros(16, 40), "patch_embedding.weight": torch.zeros(24, 4, 1, 2, 2),
            "odd.weight": torch.zeros(8, 12)}


def adapter(module=Q, r=4, N=24, K=16, prefix="transformer.", names=("lora_A", "lora_B"), seed=0, alpha=None):
    g = torch.Generator().manual_seed(seed)
    d = {"%s%s.%s.weight" % (prefix, module, names[0]): torch.randn(r, K, generator=g),
         "%s%s.%s.weight" % (prefix, module, names[1]): torch.randn(N, r, generator=g)}
    if alpha is not None:
        d["%s%s.alpha" % (prefix, module)] = torch.tensor(float(alpha))
    return d


# ---- grammar ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["transformer.", ""])
@pytest.mark.parametrize("names", [("lora_A", "lora_B"), ("lora_down", "lora_up")])
def test_both_suffix_pairs_with_and_without_the_transformer_prefix(prefix, names):
    d = adapter(prefix=prefix, names=names)
    mods = lora.parse_adapter(d)
    assert list(mods) == [Q]
    a, b, alpha = mods[Q]
    assert torch.equal(a, d["%s%s.%s.weight" % (prefix, Q, names[0])]) and torch.equal(b, d["%s%s.%s.weight" % (prefix, Q, names[1])])
    assert alpha == 4.0


def test_adapters_are_upcast_exactly_and_stay_fp32():
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        d = {k: v.to(dt) for k, v in adapter().items()}
        a, b, _ = lora.parse_adapter(d)[Q]
        assert a.dtype == b.dtype == torch.float32
        assert torch.equal(a.double(), d["transformer." + Q + ".lora_A.weight"].double())


def test_alpha_sources_and_their_precedence(tmp_path):
    sd = state_dict()
    # 3. nothing: alpha = r, so the column scale is the user's scale
    items, _ = lora.plan_merge(sd, [(adapter(r=4), 0.5)])
    assert torch.equal(items[0].scale, torch.full((4,), 0.5))
    # 2. the file's metadata
    path = str(tmp_path / "meta.safetensors")
    save_file(adapter(r=4), path, metadata={"lora_alpha": "8"})
    items, _ = lora.plan_merge(sd, [(path, 0.5)])
    assert torch.equal(items[0].scale, torch.full((4,), 0.5 * 8 / 4))
    d = dict(adapter(r=4), __metadata__={"lora_alpha": "8"})         # the dict form of the same
    assert torch.equal(lora.plan_merge(sd, [(d, 0.5)])[0][0].scale, torch.full((4,), 1.0))
    # 1. the module's own alpha wins over the metadata
    path = str(tmp_path / "both.safetensors")
    save_file(adapter(r=4, alpha=2), path, metadata={"lora_alpha": "8"})
    items, _ = lora.plan_merge(sd, [(path, 0.5)])
    assert torch.equal(items[0].scale, torch.full((4,), 0.5 * 2 / 4))
    # ... module by module: F2 has none of its own and takes the metadata's
    both = dict(adapter(r=4, alpha=2), **adapter(F2, r=2, N=16, K=40))
    save_file(both, path, metadata={"lora_alpha": "8"})
    items = {it.key: it for it in lora.plan_merge(sd, [(path, 1.0)])[0]}
    assert torch.equal(items[Q + ".weight"].scale, torch.full((4,), 0.5)) and torch.equal(items[F2 + ".weight"].scale, torch.full((2,), 4.0))


def test_rank_comes_from_the_shapes():
    sd = state_dict()
    for r in (1, 3, 7):
        items, report = lora.plan_merge(sd, [(adapter(r=r, alpha=16), 1.0)])
        assert items[0].a.shape == (r, 16) and items[0].b.shape == (24, r)
        assert torch.equal(items[0].scale, torch.full((r,), 16.0 / r)) and report[0].ranks == (r,)


def test_two_adapters_concatenate_along_r_in_list_order_with_their_own_column_scales():
    sd = state_dict()
    d1 = dict(adapter(r=4, seed=1, alpha=8), **adapter(F2, r=2, N=16, K=40, seed=2))
    d2 = adapter(r=3, seed=3, prefix="")
    items, report = lora.plan_merge(sd, [{"path": d1, "scale": 1.0, "name": "style"}, (d2, 0.5)])
    by = {it.key: it for it in items}
    assert [it.key for it in items] == [Q + ".weight", F2 + ".weight"]
    q = by[Q + ".weight"]
    assert q.a.shape == (7, 16) and q.b.shape == (24, 7) and q.a.is_contiguous() and q.b.is_contiguous()
    assert torch.equal(q.a[:4], d1["transformer." + Q + ".lora_A.weight"]) and torch.equal(q.a[4:], d2[Q + ".lora_A.weight"])
    assert torch.equal(q.b[:, :4], d1["transformer." + Q + ".lora_B.weight"]) and torch.equal(q.b[:, 4:], d2[Q + ".lora_B.weight"])
    assert torch.equal(q.scale, torch.tensor([2.0] * 4 + [0.5] * 3))
    assert by[F2 + ".weight"].a.shape == (2, 40) and torch.equal(by[F2 + ".weight"].scale, torch.ones(2))
    assert report == (lora.LoraReport("style", 1.0, 2, (2, 4)), lora.LoraReport("adapter1", 0.5, 1, (3,)))
    # the other order swaps the columns
    items2, _ = lora.plan_merge(sd, [(d2, 0.5), (d1, 1.0)])
    assert torch.equal(items2[0].scale, torch.tensor([0.5] * 3 + [2.0] * 4)) and torch.equal(items2[0].a[:3], d2[Q + ".lora_A.weight"])
    # the state dict is only read
    assert all(torch.equal(v, state_dict()[k]) for k, v in sd.items())


def test_combined_rank_above_512_raises():
    sd = state_dict()
    lora.plan_merge(sd, [(adapter(r=256, seed=1), 1.0), (adapter(r=256, seed=2), 1.0)])
    with pytest.raises(ValueError, match=re.escape(Q)):
        lora.plan_merge(sd, [(adapter(r=256, seed=1), 1.0), (adapter(r=257, seed=2), 1.0)])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _with(extra):
    return dict(adapter(), **extra)


REFUSED = [
    ("outside the grammar", _with({"transformer." + Q + ".lora_C.weight": torch.zeros(4, 16)}), "transformer." + Q + ".lora_C.weight"),
    ("PEFT adapter-name infix", {"transformer." + Q + ".lora_A.default.weight": torch.zeros(4, 16)},
     "transformer." + Q + ".lora_A.default.weight"),
    ("text encoder", _with({"text_encoder.encoder.layers.0.q.lora_A.weight": torch.zeros(4, 16)}), "text_encoder.encoder.layers.0.q.lora_A.weight"),
    ("bias", _with({"transformer." + Q + ".lora_B.bias": torch.zeros(24)}), "transformer." + Q + ".lora_B.bias"),
    ("DoRA", _with({"transformer." + Q + ".lora_magnitude_vector": torch.zeros(24)}), "transformer." + Q + ".lora_magnitude_vector"),
    ("patch convolution", adapter("patch_embedding", N=24, K=16), "patch_embedding"),
    ("4-D adapter", {"patch_embedding.lora_A.weight": torch.zeros(4, 4, 1, 2, 2), "patch_embedding.lora_B.weight": torch.zeros(24, 4, 1, 1, 1)},
     "patch_embedding.lora_A.weight"),
    ("module not in the model", adapter("blocks.9.attn1.to_q"), "blocks.9.attn1.to_q"),
    ("A without B", {"transformer." + Q + ".lora_A.weight": torch.zeros(4, 16)}, "transformer." + Q + ".lora_A.weight"),
    ("B without A", {Q + ".lora_up.weight": torch.zeros(24, 4)}, Q + ".lora_up.weight"),
    ("ranks disagree", {Q + ".lora_A.weight": torch.zeros(4, 16), Q + ".lora_B.weight": torch.zeros(24, 5)}, Q + ".lora_B.weight"),
    ("K mismatch", adapter(K=24), Q),
    ("N mismatch", adapter(N=16), Q),
    ("alpha not a scalar", _with({"transformer." + Q + ".alpha": torch.zeros(4)}), "transformer." + Q + ".alpha"),
    ("K no multiple of 8", adapter("odd", N=8, K=12), "odd"),
    ("original Wan names", {"diffusion_model.blocks.0.self_attn.q.lora_A.weight": torch.zeros(4, 16)},
     "diffusion_model.blocks.0.self_attn.q.lora_A.weight"),
    ("original Wan names, no prefix", {"blocks.0.cross_attn.k.lora_down.weight": torch.zeros(4, 16)}, "blocks.0.cross_attn.k.lora_down.weight"),
    ("original Wan feed-forward", {"blocks.0.ffn.0.lora_A.weight": torch.zeros(4, 16)}, "blocks.0.ffn.0.lora_A.weight"),
    ("original Hunyuan names", {"double_blocks.0.img_attn_qkv.lora_A.weight": torch.zeros(4, 16)}, "double_blocks.0.img_attn_qkv.lora_A.weight"),
    ("original Hunyuan single blocks", {"transformer.single_blocks.3.linear1.lora_B.weight": torch.zeros(4, 16)},
     "transformer.single_blocks.3.linear1.lora_B.weight"),
    ("kohya names", {"lora_unet_blocks_0_attn1_to_q.lora_down.weight": torch.zeros(4, 16)}, "lora_unet_blocks_0_attn1_to_q.lora_down.weight"),
]


@pytest.mark.parametrize("what,tensors,offender", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_not_dropped(what, tensors, offender):
    sd = state_dict()
    with pytest.raises(ValueError, match=re.escape(offender)) as e:
        lora.plan_merge(sd, [(tensors, 1.0)])
    if what.startswith(("original", "kohya")):
        assert "original-format (non-diffusers)" in str(e.value)


def test_diffusers_names_of_the_three_models_are_inside_the_grammar():
    for m in ("transformer_blocks.0.attn1.to_out.0", "transformer_blocks.41.ff.net.0.proj", "blocks.0.attn2.add_k_proj",
              "blocks.39.ffn.net.2", "transformer_blocks.0.attn.add_q_proj", "single_transformer_blocks.0.proj_mlp",
              "single_transformer_blocks.39.attn.to_q", "condition_embedder.text_embedder.linear_1"):
        assert list(lora.parse_adapter(adapter(m))) == [m]


# ---- specs --------------------------------------------------------------------------------------------------------------------
def test_parse_specs_forms(tmp_path):
    d = adapter()
    assert lora.parse_specs(None) == () and lora.parse_specs([]) == ()
    assert lora.parse_specs("dir/style.safetensors") == (lora.LoraSpec("dir/style.safetensors", 1.0, "style"),)
    assert lora.parse_specs(tmp_path / "m.safetensors") == (lora.LoraSpec(str(tmp_path / "m.safetensors"), 1.0, "m"),)
    assert lora.parse_specs(("a.safetensors", 0.5)) == (lora.LoraSpec("a.safetensors", 0.5, "a"),)
    s = lora.parse_specs((d, 2))
    assert s[0].source is d and s[0].scale == 2.0 and s[0].name == "adapter0"
    assert lora.parse_specs({"path": "a.safetensors", "scale": 0.25, "name": "motion"}) == (lora.LoraSpec("a.safetensors", 0.25, "motion"),)
    assert lora.parse_specs({"path": d})[0] == lora.LoraSpec(d, 1.0, "adapter0")
    many = lora.parse_specs(["a.safetensors", ("b.safetensors", 0.5), {"path": d, "name": "x"}])
    assert [(m.scale, m.name) for m in many] == [(1.0, "a"), (0.5, "b"), (1.0, "x")]
    assert lora.parse_specs(many) == many                       # normalising twice changes nothing
    for bad in (3, ("a", "b"), ("a", 1.0, 2.0), {"scale": 1.0}, {"path": "a", "weight": 1.0}, ("a", float("nan")), ("a", True), (5, 1.0)):
        with pytest.raises(ValueError, match="lora"):
            lora.parse_specs(bad)
    with pytest.raises(FileNotFoundError, match="nowhere.safetensors"):
        lora.plan_merge(state_dict(), str(tmp_path / "nowhere.safetensors"))


def test_no_adapter_is_no_work_and_the_models_take_the_keyword_last():
    sd = state_dict()
    assert lora.merge_into(sd, None, "cpu") == () and lora.merge_into(sd, [], "cpu") == ()      # nothing launched, nothing moved
    with pytest.raises(_lib.AlgHipError, match="GPU only"):
        lora.merge_into(sd, [(adapter(), 1.0)], "cpu")
    from alg_amd import (CogVideoXImageToVideoPipeline, CogVideoXTransformer3DModel, HunyuanVideoImageToVideoPipeline,
                         HunyuanVideoTransformer3DModel, WanImageToVideoPipeline, WanTransformer3DModel)
    for cls in (CogVideoXTransformer3DModel, WanTransformer3DModel, HunyuanVideoTransformer3DModel):
        assert cls.lora_report == ()
        assert "lora" not in inspect.signature(cls.__init__).parameters
        p = list(inspect.signature(cls.from_synthetic).parameters)
        assert p[-1] == "lora" and inspect.signature(cls.from_synthetic).parameters["lora"].default is None
        p = inspect.signature(cls.from_pretrained).parameters
        assert list(p)[-2:] == ["lora", "_"] and p["lora"].default is None
    for pipe in (CogVideoXImageToVideoPipeline, HunyuanVideoImageToVideoPipeline):
        p = inspect.signature(pipe.from_pretrained).parameters
        assert list(p)[-2:] == ["lora", "_"] and p["lora"].default is None
    # the Wan pipeline's named keywords end with attn_band (a tested surface): it takes lora= from its trailing keywords
    src = inspect.getsource(WanImageToVideoPipeline.from_pretrained)
    assert 'lora=_.get("lora")' in src and "lora" in WanImageToVideoPipeline.from_pretrained.__doc__


# ---- run.py -------------------------------------------------------------------------------------------------------------------
def test_run_py_lora_flag(tmp_path):
    import run
    a, b = str(tmp_path / "a.safetensors"), str(tmp_path / "b.safetensors")
    save_file(adapter(seed=1), a)
    save_file(adapter(seed=2), b)
    args = run.make_parser().parse_args(["--lora", a + ":0.5", "--lora", b])
    assert args.lora == [a + ":0.5", b]
    assert run.parse_lora_args(args.lora) == [(a, 0.5), (b, 1.0)]
    assert lora.parse_specs(run.parse_lora_args(args.lora)) == (lora.LoraSpec(a, 0.5, "a"), lora.LoraSpec(b, 1.0, "b"))
    assert run.make_parser().parse_args([]).lora is None and run.parse_lora_args(None) == []
    odd = str(tmp_path / "c:2.safetensors")                      # an existing file is a path whatever it contains
    save_file(adapter(seed=3), odd)
    assert run.parse_lora_args([odd, odd + ":3"]) == [(odd, 1.0), (odd, 3.0)]
    with pytest.raises(SystemExit, match="--lora"):
        run.parse_lora_args([str(tmp_path / "missing.safetensors")])
    with pytest.raises(SystemExit, match="--lora"):
        run.parse_lora_args([a + ":fast"])
    with pytest.raises(SystemExit, match="--lora"):
        run.parse_lora_args([a + ":nan"])
    # build_pipeline reads the flag with getattr (bare namespaces have none) and refuses a missing file before anything is built
    cfg = {"model": {"path": "THUDM/CogVideoX-5b-I2V", "dtype": "bfloat16"}}
    with pytest.raises(SystemExit, match="--lora"):
        run.build_pipeline(cfg, SimpleNamespace(synthetic=True, fp8=False, lora=[str(tmp_path / "missing.safetensors")]), "cpu")
    assert 'getattr(args, "lora", None)' in inspect.getsource(run.build_pipeline)
    assert "--lora" in run.make_parser().format_help()


# ---- the C entry --------------------------------------------------------------------------------------------------------------
def test_header_exports_and_wrapper_agree_on_the_name():
    header = open(os.path.join(ROOT, "include", "alg_hip.h")).read()
    declared = set(re.findall(r"\b(alg_[a-z0-9_]+)\s*\(", header))
    assert "alg_lora_merge" in declared and "alg_lora_merge" in _lib.EXPORTS and declared == set(_lib.EXPORTS)
    assert hasattr(alg_amd.load_library(), "alg_lora_merge")
    assert list(inspect.signature(_lib.lora_merge).parameters) == ["w", "a", "b", "scale", "out"]
    src = open(os.path.join(ROOT, "alg_amd", "csrc", "lora.hip")).read()
    proto = lambda text: re.sub(r"\s+", " ", text[text.index("int alg_lora_merge("):].split(")")[0])
    strip = lambda args: [a.strip().rsplit(" ", 1)[0] for a in args.split("(")[1].split(",")]
    assert strip(proto(header)) == strip(proto(src[src.index('extern "C"'):])) and len(strip(proto(header))) == 12
    mk = open(os.path.join(ROOT, "alg_amd", "csrc", "Makefile")).read()
    assert " lora.hip " in mk.split("SRCS =")[1].split("\n")[0] and " lora " in mk.split("STRICT =")[1].split("\n")[0] + " "
    assert "alg_lora_merge" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lora.MAX_RANK == 512 and lora.K_GRANULE == 8


_BUF = ctypes.create_string_buffer(4096)
P = (ctypes.addressof(_BUF) + 255) & ~255          # a 256-byte aligned host address; never dereferenced
W, A, B, S, O = P, P + 1024, P + 1280, P + 1536, P + 2048


def _call(**kw):
    a = dict(W=W, w_dtype=_lib.ALG_BF16, ldw=16, A=A, B=B, scale=S, out=O, ldo=16, N=4, K=16, R=4)
    a.update(kw)
    lib = alg_amd.load_library()
    rc = lib.alg_lora_merge(a["W"], a["w_dtype"], a["ldw"], a["A"], a["B"], a["scale"], a["out"], a["ldo"], a["N"], a["K"], a["R"], None)
    return rc, lib.alg_last_error().decode()


INVALID = [
    ("R = 0", dict(R=0), "R=0 must be in 1..512"),
    ("R = 513", dict(R=513), "R=513 must be in 1..512"),
    ("K = 12", dict(K=12), "K=12 must be a multiple of 8"),
    ("K = 0", dict(K=0), "bad shape"),
    ("N < 0", dict(N=-1), "bad shape"),
    ("ldw < K", dict(ldw=8), "must be at least K=16"),
    ("ldo < K", dict(ldo=8), "must be at least K=16"),
    ("ldo % 8", dict(ldo=20), "multiples of 16 bytes"),
    ("fp32 ldw % 4", dict(w_dtype=_lib.ALG_F32, ldw=18), "multiples of 16 bytes"),
    ("dtype", dict(w_dtype=2), "unknown base dtype 2"),
    ("null W", dict(W=None), "null pointer"),
    ("null A", dict(A=None), "null pointer"),
    ("null B", dict(B=None), "null pointer"),
    ("null scale", dict(scale=None), "null pointer"),
    ("null out", dict(out=None), "null pointer"),
    ("W misaligned", dict(W=W + 8), "16-byte aligned"),
    ("aliasing an fp32 base", dict(w_dtype=_lib.ALG_F32, out=W), "out may alias W only as the same bf16 buffer"),
    ("aliasing with another leading dimension", dict(out=W, ldo=24), "out may alias W only as the same bf16 buffer"),
    ("partial overlap", dict(out=W + 32), "out may alias W only as the same bf16 buffer"),
    # validate-only: no pointer at all -- the shape refusals come first
    ("validate-only R = 513", dict(W=None, A=None, B=None, scale=None, out=None, R=513), "R=513 must be in 1..512"),
    ("validate-only K", dict(W=None, A=None, B=None, scale=None, out=None, K=20), "K=20 must be a multiple of 8"),
    ("validate-only ld", dict(W=None, A=None, B=None, scale=None, out=None, ldw=8), "must be at least K=16"),
    ("validate-only, shape fine", dict(W=None, A=None, B=None, scale=None, out=None), "null pointer"),
]


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")
@pytest.mark.parametrize("what,kw,text", INVALID, ids=[c[0] for c in INVALID])
def test_argument_check_refuses_before_any_launch(what, kw, text):
    rc, msg = _call(**kw)
    assert rc == EINVAL and msg.startswith("alg_lora_merge: ") and text in msg, (rc, msg)


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-path test: a lost check would launch on host pointers")
def test_checked_calls_that_launch_nothing():
    assert _call(N=0)[0] == 0                                    # nothing to do
    rc, msg = _call(out=W)                                       # in place on a bf16 base passes the check: it fails at the launch
    assert rc == -2 and "alg_lora_merge" in msg, (rc, msg)


def test_wrapper_checks_its_tensors_before_the_library():
    w = torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(_lib.AlgHipError, match="device tensor"):
        _lib.lora_merge(w, torch.zeros(2, 16), torch.zeros(4, 2), torch.ones(2))
