"""The encoder attention entry (alg_attn_bias; csrc/t5.hip) through its raw C ABI -- three pointers, two pitches -- on guarded
operands with exact data (tests/helpers/enc_attn_arena.py): every tower's mode (T5 / UMT5 with bias and mask, CLIP text causal,
CLIP vision at head_dim 80) at the lengths where the kernel's paths change (one row, a second workgroup of one row, the 64-key
chunk edge, L % 4 != 0, the size limits 512 and 448), the cross combinations the contract allows (causal with a mask, with a bias,
at head_dim 80), masks with tails of another length per item, holes, key 0 masked under causal and a fully masked item.  Every
case, under a friendly fill of zeros and a hostile fill of NaN outside the live elements, the friendly one twice:

  1. value: family A ("selector") is BIT FOR BIT the float64 statement of the header's contract -- the scores take levels at
     least 112 apart, p is bf16(1 / n) on the top level, and any leaked key (masked ones carry v = 2^100), a wrong bucket, head,
     diagonal or key count changes the bits; family B ("graded", a softmax that is not one-hot) holds
     |got - ref| <= (2^-9 + 2^-13) (A + |ref|) per element, derived in the helper.  The share of family B elements that differ
     from bf16(ref) is printed, not asserted on (measured when the test was written: 0 to 0.16 % per case, median 0.004 %,
     and at most 0.94 of the bound used).  A row without a surviving key is zeros, of either sign;
  2. footprint: every element of the out arena outside rows < B L, columns [0, inner) of the window still holds the canary;
     q, k, v, the table, the LUT and the mask are unchanged;
  3. fill independence: the hostile and the friendly outputs are bit-equal and finite;
  4. determinism: the second friendly run gives the same bits in the whole arena.

tests/test_enc_attn_arena_cpu.py shows on an emulation that these assertions catch the ways such a kernel goes wrong, and asserts
the conditions on the data.  The refusals at the end launch nothing."""
import pytest
import torch

from alg_amd import _lib
from helpers import enc_attn_arena as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
TABLE = E.table()


def _call_abi(call, out_full, q_off=None, k_off=None, v_off=None, batch=E.B, head_dim=None, L=None, qkv_rs=None, lut=True):
    """alg_attn_bias as include/alg_hip.h declares it; the keywords bend one argument for the refusals."""
    data = call.data
    p = _lib._p
    rc = _lib.load_library().alg_attn_bias(
        p(call.qkv, call.q_off if q_off is None else q_off), p(call.qkv, call.k_off if k_off is None else k_off),
        p(call.qkv, call.v_off if v_off is None else v_off), p(out_full, call.out_off), p(call.table), p(call.lut if lut else None),
        p(call.mask), batch, E.H, call.d if head_dim is None else head_dim, call.L if L is None else L,
        call.qkv_rs if qkv_rs is None else qkv_rs, call.out_rs, float(data.scale), int(data.causal), _lib._stream())
    _lib._check(rc, "alg_attn_bias")


@pytest.mark.parametrize("case", TABLE, ids=[E.case_id(c) for c in TABLE])
def test_encoder_attention_on_guarded_operands(case):
    data = E.make_data(case)
    ref = E.reference(data, flips=False)
    for layout in E.layouts_of(case):
        f, h = E.build(data, layout, "friendly", DEV), E.build(data, layout, "hostile", DEV)
        outs = []
        for call in (f, h, f):
            out = call.fresh_out()
            _call_abi(call, out)
            outs.append(out)
        torch.cuda.synchronize()
        report = []
        failed = E.failures(f, outs[0], h, outs[1], ref, outs[2], report)
        for cid, lay, fill, share, used in report:
            print("family B: share of elements off bf16(ref) %-28s %-8s %-8s %.6f   largest |got - ref| / bound %.3f" % (cid, lay, fill, share, used))
        assert failed == {}, (layout, failed)
        if layout == "compact":      # the wrapper passes exactly this
            out = f.fresh_out()
            _lib.attn_bias(f.qkv[f.q_off:], out[f.out_off:], f.table, f.lut, f.mask, E.B, E.H, case.L, scale=data.scale,
                           head_dim=f.d, causal=data.causal)
            torch.cuda.synchronize()
            E.assert_deterministic(f, outs[0], out)


REFUSALS = {
    "L = 0":                     ("t5", dict(L=0)),
    "L = 513 at head_dim 64":    ("t5", dict(L=513)),
    "L = 449 at head_dim 80":    ("clip_vision", dict(L=449)),
    "head_dim = 128":            ("t5", dict(head_dim=128)),
    "qkv_rstride % 8 != 0":      ("t5", dict(qkv_rs="+4")),
    "a bias table without LUT":  ("t5", dict(lut=False)),
    "k off 16 bytes":            ("t5", dict(k_off="+4")),
    "v off 16 bytes":            ("clip_vision", dict(v_off="+4")),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_bad_arguments_are_refused_before_any_launch(name):
    """Each is ALG_EINVAL by the header; `out` keeps its canary and the inputs their bits.  k and v are read 16 bytes at a time
    (the staging loop of attn_bias_kernel), so a base off that grid is refused; q is read per element and may sit anywhere."""
    mode, bend = REFUSALS[name]
    call = E.build(E.make_data(E.Case(mode, 65, "A")), "loose", "friendly", DEV)
    kw = {}
    for key, val in bend.items():
        kw[key] = getattr(call, key) + int(val) if isinstance(val, str) else val
    out = call.fresh_out()
    with pytest.raises(_lib.AlgHipError):
        _call_abi(call, out, **kw)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == E.CANARY_BITS).all())
    E.assert_inputs_unchanged(call)


def test_an_empty_batch_returns_without_touching_out():
    call = E.build(E.make_data(E.Case("t5", 65, "A")), "loose", "friendly", DEV)
    out = call.fresh_out()
    _call_abi(call, out, batch=0)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == E.CANARY_BITS).all())
    E.assert_inputs_unchanged(call)


def test_q_and_out_may_sit_on_any_element():
    """The other side of the alignment refusal: q two bytes off the 16-byte grid (out's window already starts at column 6 of a
    pitch that is no multiple of 8) computes what the aligned call computes, on q shifted by one column."""
    case = E.Case("clip_text", 65, "A")
    data = E.make_data(case)
    call = E.build(data, "loose", "friendly", DEV)
    shifted = E.Data(case, torch.roll(data.q.reshape(E.B * 65, -1), -1, dims=1).reshape(data.q.shape), data.k, data.v, None, None, None)
    shifted.q.reshape(E.B * 65, -1)[:, -1] = 0          # the first gap column behind q's window: zeros under the friendly fill
    ref = E.reference(shifted, flips=False)
    assert bool((ref.top_gap >= E.GAP).all()) and bool(E.n_is_safe(ref.n[~ref.nokey]).all())      # family A's conditions
    assert not torch.equal(ref.out, E.reference(data, flips=False).out)
    out = call.fresh_out()
    _call_abi(call, out, q_off=call.q_off + 1)
    torch.cuda.synchronize()
    E.assert_value(call, out, ref)
    E.assert_footprint(call, out)
