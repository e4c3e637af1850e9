"""HunyuanVideoTransformer3DModel(..., fp8=True): e4m3 block linears on the fp8 MFMA.

The scheme is oracle/fp8_oracle.py's (per-token / per-output-channel amax / 448, fp32 accumulation) -- this build's choice, the
reference has no fp8 -- so every accuracy statement here is about the product and its own oracle, on synthetic weights.  The floor
of a forward is the reference's execution mode (bf16 weights and activations, eager op order) with exactly the quantised linears
sent through fp8_oracle.linear (tests/_hy_fp8_floor.py: six per dual-stream block on the latent stream, five per single-stream
block on the joint rows, proj_out on the concatenated [attention | mlp] row); the bounds are the unchanged factors of
tests/_parity.py against that floor."""
import contextlib

import pytest
import torch

from _attn_fp8_floor import hy_fp8_attention
from _hy_fp8_floor import hy_fp8_linears, routed_per_forward
from _parity import assert_repeatable, check_floor, rel
from alg_amd import _lib
from alg_amd.pipeline_hunyuan_video_image2video_lowpass import HunyuanVideoImageToVideoPipeline
from alg_amd.schedulers import FlowMatchEulerDiscreteScheduler
from alg_amd.transformer_hunyuan_video import HunyuanVideoTransformer3DModel, HunyuanVideoTransformerConfig
from helpers.trained_like_cases import hy_case
from oracle import hy_oracle, loop_oracle
from oracle.sched_oracle import FlowMatchEulerOracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


# ---- 1. the fused norm + quantiser -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("D", [512, 1024, 3072])
def test_layernorm_modulate_seg_fp8_is_norm_then_quantiser(D, batch):
    """alg_layernorm_modulate_seg_fp8 == alg_layernorm_modulate_seg into bf16 + alg_quantize_fp8_rows, bytes and scales, bit for
    bit, on outputs pre-filled with a sentinel."""
    rows, eps = 229, 1e-6                                   # not a multiple of the 4 rows of a workgroup
    x_bstride, x_off = rows * D + 64, 24                    # x_bstride > rows * D, x_off != 0
    xbuf = _rand((x_off + batch * x_bstride,), 10 + D + batch, 2.0)
    xv = xbuf[x_off:].view(batch, x_bstride)[:, :rows * D].view(batch, rows, D)
    xv[0, 3] = 1.25                                         # a row of all-equal values: variance 0
    xv[batch - 1, rows - 1] *= 40.0                         # and a large one
    w, b = 1.0 + _rand((D,), 1, 0.2), _rand((D,), 2, 0.1)
    mod_bs = 8 + 12 * D                                     # per batch item: 8 unused | [2][6 D] (HunyuanVideo's token-replace layout)
    mod = _rand((batch, mod_bs), 3, 0.5)
    shift_off, scale_off = 8, 8 + D
    for seg_stride in (0, 3 * D, 6 * D):
        for seg in (0, 7, rows - 3, rows):
            for wgt, bia in ((None, None), (w, b)):         # the no-affine form the model uses | with a LayerNorm affine
                y = torch.empty(batch * rows, D, dtype=BF, device=DEV)
                _lib.layernorm_modulate_seg(xbuf, y, wgt, bia, mod, mod, mod_bs, seg_stride, batch, rows, D, seg, eps,
                                            x_bstride=x_bstride, x_off=x_off, scale_off=scale_off, shift_off=shift_off)
                q_ref = torch.empty(batch * rows, D, dtype=torch.uint8, device=DEV)
                s_ref = torch.empty(batch * rows, dtype=torch.float32, device=DEV)
                _lib.quantize_fp8_rows(y, q_ref, s_ref, batch * rows, D)
                q = torch.full((batch * rows + 2, D), 0xA5, dtype=torch.uint8, device=DEV)
                s = torch.full((batch * rows + 2,), -7.0, dtype=torch.float32, device=DEV)
                _lib.layernorm_modulate_seg_fp8(xbuf, q, s, wgt, bia, mod, mod, mod_bs, seg_stride, batch, rows, D, seg, eps,
                                                x_bstride=x_bstride, x_off=x_off, scale_off=scale_off, shift_off=shift_off)
                case = (seg_stride // D, seg, wgt is not None)
                assert torch.equal(s[:-2], s_ref), case
                assert torch.equal(q[:-2], q_ref), case
                assert (s[:-2] > 0).all() and (q[-2:] == 0xA5).all() and (s[-2:] == -7.0).all(), case
    # the two segments take different vectors: with seg_stride = 6 D the rows below the split differ from the seg_stride = 0 run
    q0, s0 = (torch.empty(batch * rows, D, dtype=torch.uint8, device=DEV), torch.empty(batch * rows, dtype=torch.float32, device=DEV))
    q6, s6 = torch.empty_like(q0), torch.empty_like(s0)
    for qq, ss, st in ((q0, s0, 0), (q6, s6, 6 * D)):
        _lib.layernorm_modulate_seg_fp8(xbuf, qq, ss, None, None, mod, mod, mod_bs, st, batch, rows, D, 7, eps,
                                        x_bstride=x_bstride, x_off=x_off, scale_off=scale_off, shift_off=shift_off)
    assert torch.equal(q0[:7], q6[:7]) and not torch.equal(q0[7:rows], q6[7:rows])


def test_layernorm_modulate_seg_fp8_refuses_bad_calls_before_any_launch():
    rows = 5
    for D in (768, 8704):
        x = _rand((rows, D), 7)
        q = torch.full((rows, D), 0x5A, dtype=torch.uint8, device=DEV)
        s = torch.full((rows,), -3.0, dtype=torch.float32, device=DEV)
        with pytest.raises(_lib.AlgHipError, match="multiple of 512"):
            _lib.layernorm_modulate_seg_fp8(x, q, s, None, None, None, None, 0, 0, 1, rows, D, 0, 1e-6)
        torch.cuda.synchronize()
        assert (q == 0x5A).all() and (s == -3.0).all()
    x = _rand((rows, 512), 8)
    q = torch.full((rows, 512), 0x5A, dtype=torch.uint8, device=DEV)
    s = torch.full((rows,), -3.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.AlgHipError, match="together"):          # scale without shift
        _lib.layernorm_modulate_seg_fp8(x, q, s, None, None, x, None, 0, 0, 1, rows, 512, 0, 1e-6)
    with pytest.raises(_lib.AlgHipError, match="bad argument"):      # a segment distance that breaks the 16-byte loads
        _lib.layernorm_modulate_seg_fp8(x, q, s, None, None, x, x, 1024, 12, 1, rows, 512, 0, 1e-6)
    torch.cuda.synchronize()
    assert (q == 0x5A).all() and (s == -3.0).all()


# ---- 2. the batched, strided quantiser ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [5, 1030])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("K", [3072, 12288, 15360, 256, 2560])
def test_quantize_fp8_rows_batched_is_the_row_quantiser_per_item(K, batch, rows):
    """Rows inside a wider, batch-strided buffer (the ws.am layout: row stride > K, a column offset, a batch stride with slack), all
    items in one launch == alg_quantize_fp8_rows on each item, bit for bit; K = 3072 / 12288 / 15360 keep the row in registers,
    256 / 2560 take the loop form.  The source, the bytes behind the last row and the scales behind the last are untouched."""
    col, rs = 64, K + 512
    bs = rows * rs + 128
    xbuf = _rand((batch * bs + 8,), 100 + K // 8 + batch + rows, 1.5)
    xv = xbuf[:batch * bs].view(batch, bs)[:, :rows * rs].view(batch, rows, rs)
    xv[batch - 1, 2, col:col + K] = 0.0                     # an all-zero row: scale 1, bytes 0
    xv[0, rows - 1, col:col + K] *= 300.0
    xv[0, 1, col + K - 1] = 77.0                            # the row maximum in the last column read
    xv[0, 1, col + K] = 9000.0                              # ... and a larger value right behind it, in a column that is not
    before = xbuf.clone()
    q = torch.full((batch * rows + 3, K), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full((batch * rows + 3,), -7.0, dtype=torch.float32, device=DEV)
    _lib.quantize_fp8_rows_batched(xbuf, q, s, batch, rows, K, bs, rs, x_off=col)
    q_ref = torch.empty(batch * rows, K, dtype=torch.uint8, device=DEV)
    s_ref = torch.empty(batch * rows, dtype=torch.float32, device=DEV)
    for b in range(batch):
        _lib.quantize_fp8_rows(xbuf, q_ref, s_ref, rows, K, x_rstride=rs, x_off=b * bs + col, q_off=b * rows * K, scale_off=b * rows)
    torch.cuda.synchronize()
    assert torch.equal(s[:-3], s_ref) and torch.equal(q[:-3], q_ref)
    assert (q[-3:] == 0xA5).all() and (s[-3:] == -7.0).all()
    assert torch.equal(xbuf, before)
    zero = (batch - 1) * rows + 2
    assert s[zero].item() == 1.0 and (q[zero] == 0).all()
    assert s[1].item() == pytest.approx(max(77.0, xv[0, 1, col:col + K].float().abs().max().item()) / 448.0, rel=1e-6)
    # the values are the source's: de-quantised they are within e4m3's half-ulp of it
    src = xv[:, :, col:col + K].reshape(batch * rows, K).float()
    deq = q[:-3].view(F8).float() * s[:-3, None]
    assert ((deq - src).abs() <= 2.0 ** -4 * src.abs() + s[:-3, None] * 2.0 ** -10).all()


def test_quantize_fp8_rows_batched_refuses_bad_calls_before_any_launch():
    x = _rand((4, 256), 9)
    q = torch.full((4, 256), 0x5A, dtype=torch.uint8, device=DEV)
    s = torch.full((4,), -3.0, dtype=torch.float32, device=DEV)
    for kw in (dict(K=12), dict(batch=-1), dict(x_rstride=260), dict(x_off=4)):
        a = dict(dict(batch=1, rows=4, K=256, x_bstride=1024, x_rstride=256, x_off=0), **kw)
        with pytest.raises(_lib.AlgHipError, match="alg_quantize_fp8_rows_batched"):
            _lib.quantize_fp8_rows_batched(x, q, s, a["batch"], a["rows"], a["K"], a["x_bstride"], a["x_rstride"], x_off=a["x_off"])
    torch.cuda.synchronize()
    assert (q == 0x5A).all() and (s == -3.0).all()


# ---- 3 - 5. the forward ------------------------------------------------------------------------------------------------------
MODES = {"token_replace": dict(image_condition_type="token_replace", guidance_embeds=False),
         "plain_guidance": dict(image_condition_type="latent_concat", guidance_embeds=True)}


def _small(mode, seed=3, **over):
    """tests/test_gpu_hunyuan_forward.py's small() config (heads 4, D = 512): -> (config, oracle config, bf16 state dict)"""
    kw = dict(num_attention_heads=4, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64,
              pooled_projection_dim=64, **MODES[mode])
    kw.update(over)
    ocfg = hy_oracle.HyConfig(**kw)
    return HunyuanVideoTransformerConfig(**kw), ocfg, hy_oracle.init_weights(ocfg, seed=seed)


def _inputs(ocfg, F, H, W, L, valid, seed, N=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 16, F, H, W, generator=g).to(BF)
    txt = torch.randn(N, L, 64, generator=g).to(BF)
    mask = torch.zeros(N, L)
    for b, v in enumerate(valid):
        mask[b, :v] = 1
    pooled = torch.randn(N, 64, generator=g).to(BF)
    guid = torch.tensor([6000.0] * N) if ocfg.guidance_embeds else None
    return x, torch.tensor([996.0] * N), txt, mask, pooled, guid


def _run(model, inputs):
    x, t, txt, mask, pooled, guid = inputs
    return model(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV),
                 encoder_attention_mask=mask.to(DEV).to(BF), pooled_projections=pooled.to(DEV),
                 guidance=None if guid is None else guid.to(DEV), return_dict=False)[0]


def _oracles(ocfg, sd, inputs, fp8_attention=False):
    """fp32 reference, bf16-eager, and the e4m3-eager floor: the bf16 oracle with the quantised linears through fp8_oracle.linear
    (and, for fp8_attention, the joint attentions through the eager restatement of that scheme: tests/_attn_fp8_floor.py)."""
    x, t, txt, mask, pooled, guid = inputs
    ref = hy_oracle.hy_forward(ocfg, {k: v.float() for k, v in sd.items()}, x.float(), t, txt.float(), mask, pooled.float(), guid)
    bf16 = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, guid, dtype=BF)
    with contextlib.ExitStack() as stack:
        stats = stack.enter_context(hy_fp8_linears(sd, BF))
        if fp8_attention:
            a_stats = stack.enter_context(hy_fp8_attention(ocfg, sd))
        e4m3 = hy_oracle.hy_forward(ocfg, sd, x, t, txt, mask, pooled, guid, dtype=BF)
    assert stats["routed"] == routed_per_forward(ocfg)
    if fp8_attention:
        assert a_stats["routed"] == ocfg.num_layers + ocfg.num_single_layers
    return ref, bf16, e4m3


CASES = {   # mode, config overrides, (F, H, W, L, valid prompt lengths)
    "token_replace": ("token_replace", {}, (3, 16, 16, 20, (13, 20))),
    "plain_guidance": ("plain_guidance", {}, (3, 16, 16, 20, (13, 20))),
    # 180 latent + 22 prompt tokens: the joint rows of a sample are not a multiple of 4 (one launch per item in the single blocks)
    "ragged_joint_rows": ("token_replace", dict(num_layers=2, num_single_layers=2), (3, 12, 20, 22, (22, 5))),
}


@pytest.mark.parametrize("fp8_attention", [False, True], ids=["bf16_attention", "fp8_attention"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fp8_forward_on_the_e4m3_floor_and_anchored_to_bf16(case, fp8_attention):
    """HIP fp8 forward vs fp32 within the unchanged factors of the e4m3-eager floor, repeatable; its distance to the bf16 model's
    output, on the same weights, is at most 1.5 x the distance of the two ORACLE runs (e4m3-eager vs bf16-eager)."""
    mode, over, shape = CASES[case]
    cfg, ocfg, sd = _small(mode, **over)
    inputs = _inputs(ocfg, *shape, seed=4)
    ref, bf16, e4m3 = _oracles(ocfg, sd, inputs, fp8_attention)
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=True, fp8_attention=fp8_attention)
    assert model.fp8 is True and model.fp8_attention is fp8_attention
    out = assert_repeatable(lambda: _run(model, inputs), times=3, what="fp8 forward " + case)
    assert out.shape == ref.shape and out.dtype == BF
    name = "hy_fp8_forward_%s%s" % (case, "_fp8_attention" if fp8_attention else "")
    e_hip, e_floor = check_floor(name, out, ref, e4m3)
    out_bf16 = _run(HunyuanVideoTransformer3DModel(cfg, sd, device=DEV), inputs)
    r, anchor = rel(out, out_bf16), rel(e4m3, bf16)
    print("%s: fp8 HIP vs fp32 %.3e (e4m3-eager floor %.3e, bf16-eager %.3e); fp8 HIP vs bf16 HIP %.3e (e4m3-eager vs bf16-eager "
          "%.3e)" % (name, e_hip, e_floor, rel(bf16, ref), r, anchor))
    assert 0 < r <= 1.5 * anchor, (r, anchor)


@pytest.mark.parametrize("fp8_attention", [False, True], ids=["bf16_attention", "fp8_attention"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fp8_forward_on_trained_like_weights(mode, fp8_attention):
    """The same forward on the trained-like profile (tests/helpers/trained_like.py: QK gains of 1 to 16, massive channels, hot
    output channels, O(1) biases), held to the e4m3-eager floor with the same factors."""
    kw, ocfg, sd, inputs = hy_case(mode)
    ref, bf16, e4m3 = _oracles(ocfg, sd, inputs, fp8_attention)
    model = HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(**kw), sd, device=DEV, fp8=True, fp8_attention=fp8_attention)
    out = assert_repeatable(lambda: _run(model, inputs), times=3, what="fp8 trained-like forward " + mode)
    name = "hy_fp8_forward_small_%s_trained_like%s" % (mode, "_fp8_attention" if fp8_attention else "")
    e_hip, e_floor = check_floor(name, out, ref, e4m3)
    print("%s: fp8 HIP vs fp32 %.3e (e4m3-eager floor %.3e, bf16-eager %.3e)" % (name, e_hip, e_floor, rel(bf16, ref)))


def _block_tensors(blocks):
    """every tensor an attribute of a block holds (directly, in a tuple or in its `packed` dict), and the PackedB copies"""
    tensors, packed = [], []
    for L in blocks:
        for name, v in vars(L).items():
            for item in (v.values() if isinstance(v, dict) else v if isinstance(v, (tuple, list)) else (v,)):
                if isinstance(item, torch.Tensor):
                    tensors.append((name, item))
                elif isinstance(item, _lib.PackedB):
                    packed.append((name, item))
    return tensors, packed


def test_fp8_flag_semantics():
    """bf16-built: flips both ways and keeps both weight sets; the first fp8 forward of a flipped model is the fp8-built model's;
    fp8-built: no bf16 or packed copy of a quantised weight, refuses a bf16 forward; all four fp8 x fp8_attention combinations run
    on one model."""
    cfg, ocfg, sd = _small("token_replace", num_layers=2, num_single_layers=2)
    inputs = _inputs(ocfg, 3, 16, 16, 20, (13, 20), seed=4)
    D, M = cfg.dim, int(cfg.dim * cfg.mlp_ratio)
    built8 = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=True)
    out8 = _run(built8, inputs)
    flip = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    assert flip.fp8 is False and not hasattr(flip.dual[0], "wqk8")
    first = _run(flip, inputs)
    assert not hasattr(flip._workspace(2, 192, 20), "q8")        # the e4m3 workspace appears with the flag only
    flip.fp8 = True
    as_fp8 = _run(flip, inputs)
    assert torch.equal(as_fp8, out8)                             # the lazily quantised model is the one built with fp8=True
    assert not torch.equal(as_fp8, first)
    assert hasattr(flip._workspace(2, 192, 20), "q8")
    flip.fp8 = False
    assert torch.equal(_run(flip, inputs), first)                # and back: the run that never flipped
    # all four combinations of the two independent flags on one model; fp8_attention alone is what it is on a plain model
    outs = {}
    for f8, f8a in ((False, False), (True, False), (False, True), (True, True)):
        flip.fp8, flip.fp8_attention = f8, f8a
        outs[f8, f8a] = _run(flip, inputs)
        assert torch.isfinite(outs[f8, f8a].float()).all()
    flip.fp8 = flip.fp8_attention = False
    assert torch.equal(outs[False, False], first) and torch.equal(outs[True, False], out8)
    assert len({tuple(o.flatten()[:4096].tolist()) for o in outs.values()}) == 4
    plain_attn8 = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8_attention=True)
    assert torch.equal(outs[False, True], _run(plain_attn8, inputs))
    both = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=True, fp8_attention=True)
    assert torch.equal(outs[True, True], _run(both, inputs))
    # what the two builds hold.  Shapes of the quantised weights: [2D, D] (Q|K), [D, D] (V, out), [M, D], [D, M], [D, D + M];
    # the prompt stream of a dual block keeps one bf16 [2D, D], two [D, D], one [M, D] and one [D, M] of its own
    shapes = {(2 * D, D), (D, D), (M, D), (D, M), (D, D + M)}
    count = lambda tensors, dt: sum(1 for _, t in tensors if t.dtype == dt and tuple(t.shape) in shapes)
    t8d, p8d = _block_tensors(built8.dual)
    t8s, p8s = _block_tensors(built8.single)
    assert not p8d and not p8s                                   # no PackedB anywhere
    assert count(t8d, BF) == 5 * len(built8.dual)                # the prompt stream's five, nothing of the latent stream
    assert count(t8s, BF) == 0
    assert count(t8d, torch.uint8) == 5 * len(built8.dual) and count(t8s, torch.uint8) == 4 * len(built8.single)
    for L, names in [(L, built8.FP8_DUAL) for L in built8.dual] + [(L, built8.FP8_SINGLE) for L in built8.single]:
        for nm in names:
            q, s = getattr(L, nm + "8")
            assert q.dtype == torch.uint8 and s.dtype == torch.float32 and s.shape == (q.shape[0],)
    tfd, pfd = _block_tensors(flip.dual)
    tfs, pfs = _block_tensors(flip.single)
    assert count(tfd, BF) == 10 * len(flip.dual) and count(tfs, BF) == 4 * len(flip.single)      # both sets are kept
    assert count(tfd, torch.uint8) == 5 * len(flip.dual) and len(pfd) == 4 * len(flip.dual) and len(pfs) == 3 * len(flip.single)
    # a model built with fp8=True has nothing to run bf16 on, and says so
    built8.fp8 = False
    try:
        with pytest.raises(_lib.AlgHipError, match="fp8=True"):
            _run(built8, inputs)
    finally:
        built8.fp8 = True
    assert torch.equal(_run(built8, inputs), out8)


def test_fp8_build_allocates_less_than_the_bf16_build():
    cfg, ocfg, sd = _small("token_replace", num_attention_heads=8, num_layers=2, num_single_layers=4)   # 1024 wide
    D = cfg.dim

    def footprint(fp8):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=fp8)
        torch.cuda.synchronize()
        return model, torch.cuda.memory_allocated() - before

    m8, b8 = footprint(True)
    del m8
    m16, b16 = footprint(False)
    quantised = cfg.num_layers * 12 * D * D + cfg.num_single_layers * 12 * D * D     # parameters of the quantised linears
    print("allocated by construction: fp8 %d bytes, bf16 %d bytes (quantised linears: %d parameters)" % (b8, b16, quantised))
    # bf16 build: 2 bytes per parameter + the packed copies (dual: 11 of the 12 D^2, single: 11 of 12) = about 3.8 bytes;
    # fp8 build: 1 byte (+ 4 per output channel).  2.8 apart up to the scales and the allocator's rounding: 2.5 is asked
    assert b16 - b8 >= 2.5 * quantised


def test_fp8_refuses_a_width_the_e4m3_path_cannot_take():
    """K % 128 == 0 is alg_gemm_fp8's contract, D % 512 == 0 the fused norm's: the constructor checks both before it touches a
    weight, and so does the flip of a model built in bf16."""
    with pytest.raises(ValueError, match="K % 128"):
        HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(num_attention_heads=4, mlp_ratio=0.125), {}, device=DEV, fp8=True)
    with pytest.raises(ValueError, match="D % 512"):
        HunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(num_attention_heads=3), {}, device=DEV, fp8=True)
    cfg, ocfg, sd = _small("token_replace", mlp_ratio=3.875)     # an MLP width of 1984 = 15.5 x 128: fine in bf16 (K % 64)
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV)
    inputs = _inputs(ocfg, 3, 16, 16, 20, (13, 20), seed=4)
    first = _run(model, inputs)
    model.fp8 = True
    with pytest.raises(ValueError, match="K % 128"):
        _run(model, inputs)
    model.fp8 = False
    assert torch.equal(_run(model, inputs), first)


def test_fp8_padded_prompt_tokens_do_not_reach_the_latents():
    """As tests/test_gpu_full_size_c345.py::test_hunyuan_13b_width_c4_token_count asks of the bf16 model: padded prompt tokens
    set to 37.0 change no latent, bit for bit -- also with a per-token scale taken over rows that hold them.

    The statement is about the e4m3 linears with the bf16 attention.  `fp8_attention` is not part of it: that flag's scheme takes
    the V^T row scales over every column of the joint sequence, padded prompt columns included (tests/helpers/attn_fp8_ref.py,
    sdpa_fp8: "the operands are quantised over the whole length first, as the models do"), so with it on a padded token moves
    the scale of V and through it the latents, with bf16 linears just as with e4m3 ones (docs/numerics.md)."""
    cfg, ocfg, sd = _small("token_replace", num_layers=2, num_single_layers=2)
    inputs = _inputs(ocfg, 3, 16, 16, 20, (13, 7), seed=4)
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=True)
    out = _run(model, inputs)
    x, t, txt, mask, pooled, guid = inputs
    txt2 = txt.clone()
    txt2[0, 13:] = 37.0
    txt2[1, 7:] = 37.0
    assert torch.equal(_run(model, (x, t, txt2, mask, pooled, guid)), out)


# ---- 7. the sampler --------------------------------------------------------------------------------------------------------
def test_alg_sampler_with_the_fp8_transformer_on_the_e4m3_loop_floor():
    """Two ALG steps (true CFG + low-pass branch: a 3-pass step) of HunyuanVideoImageToVideoPipeline with the fp8 transformer vs
    oracle/loop_oracle driving the fp32 oracle DiT; the floor is the same loop driving the e4m3-eager forward."""
    cfg, ocfg, sd = _small("token_replace", seed=7)
    sd32 = {k: v.float() for k, v in sd.items()}
    model = HunyuanVideoTransformer3DModel(cfg, sd, device=DEV, fp8=True)
    g = torch.Generator().manual_seed(8)
    lat, img = torch.randn(1, 16, 3, 16, 16, generator=g), torch.randn(1, 16, 1, 16, 16, generator=g)
    mk = lambda v: (torch.randn(1, 20, 64, generator=g).to(BF), torch.randn(1, 64, generator=g).to(BF),
                    torch.cat([torch.ones(1, v), torch.zeros(1, 20 - v)], dim=1).to(BF))
    pos, neg = mk(17), mk(9)
    alg = dict(lp_filter_type="down_up", lp_resize_factor=0.625, lp_strength_schedule_type="interval",
               schedule_interval_start_time=0.0, schedule_interval_end_time=0.6)
    loop = dict(true_cfg_scale=6.0, guidance_scale=1.0, use_low_pass_guidance=True, guidance_embeds=False, **alg)

    def oracle_dit(x, timestep, ehs, mask, pooled, guidance):
        return hy_oracle.hy_forward(ocfg, sd32, x.float(), timestep.float(), ehs.float(), mask.float(), pooled.float(), None).to(BF)

    def eager_dit(x, ts, e, m, p_, g_):
        return hy_oracle.hy_forward(ocfg, sd, x.to(BF), ts.float(), e, m.float(), p_, None, dtype=BF)

    trace_o, trace_p = [], []
    want = loop_oracle.hunyuan_denoise_loop(oracle_dit, FlowMatchEulerOracle(shift=7.0), lat, img, pos, neg, 2, trace=trace_o, **loop)
    with hy_fp8_linears(sd, BF) as stats:
        floor = loop_oracle.hunyuan_denoise_loop(eager_dit, FlowMatchEulerOracle(shift=7.0), lat, img, pos, neg, 2, **loop)
    plain = loop_oracle.hunyuan_denoise_loop(eager_dit, FlowMatchEulerOracle(shift=7.0), lat, img, pos, neg, 2, **loop)
    pipe = HunyuanVideoImageToVideoPipeline(transformer=model, scheduler=FlowMatchEulerDiscreteScheduler(shift=7.0)).to(DEV)
    d = lambda t_: t_.to(DEV)
    out = pipe(prompt_embeds=d(pos[0]), pooled_prompt_embeds=d(pos[1]), prompt_attention_mask=d(pos[2]),
               negative_prompt_embeds=d(neg[0]), negative_pooled_prompt_embeds=d(neg[1]),
               negative_prompt_attention_mask=d(neg[2]), negative_prompt=None, image_latents=d(img), latents=d(lat),
               height=128, width=128, num_frames=9, num_inference_steps=2, true_cfg_scale=6.0, guidance_scale=1.0,
               output_type="latent", use_low_pass_guidance=True, lp_filter_in_latent=True, step_trace=trace_p, **alg)
    passes = [n for _, n, _ in trace_p]
    assert passes == [n for _, n, _ in trace_o] and len(passes) == 2 and passes[0] == 3
    assert stats["routed"] == routed_per_forward(ocfg) * 2        # one batched oracle forward per step
    assert torch.equal(out.frames[:, :, :1].cpu(), img)
    assert not torch.equal(floor, plain)
    check_floor("hy_fp8_sampler_2steps", out.frames[:, :, 1:], want[:, :, 1:], floor[:, :, 1:])
