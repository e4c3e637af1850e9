"""The e4m3-eager floor helper (tests/_fp8_floor.py) on the CPU: it routes exactly the six block linears of every block of
oracle/dit_oracle.py through oracle/fp8_oracle.linear, nothing else, and always puts torch.nn.functional.linear back."""
import pytest
import torch
import torch.nn.functional as F

from _fp8_floor import FP8_LINEARS, fp8_linears, fp8_weight_names
from _parity import rel
from oracle import dit_oracle

BF = torch.bfloat16
SMALL = dict(num_attention_heads=8, attention_head_dim=64, in_channels=16, out_channels=8, num_layers=2,
             time_embed_dim=64, text_embed_dim=128, max_text_seq_length=10, sample_width=12, sample_height=8,
             sample_frames=9, patch_size=2)


def _case(num_layers=2):
    ocfg = dit_oracle.DiTConfig(**dict(SMALL, num_layers=num_layers))
    w32 = dit_oracle.init_weights(ocfg, seed=3, std=0.05, randomize_affine=True)
    wbf = {k: v.to(BF) for k, v in w32.items()}
    g = torch.Generator().manual_seed(1)
    hs = torch.randn(3, 3, 16, 8, 12, generator=g).to(BF)
    ehs = torch.randn(3, 10, 128, generator=g).to(BF)
    ts = torch.tensor([999, 999, 999])
    rope = dit_oracle.rope_tables(ocfg, 64, 96, 3)
    return ocfg, wbf, hs, ehs, ts, rope


def test_helper_names_the_six_block_linears_of_every_block():
    ocfg, wbf, *_ = _case(num_layers=3)
    names = fp8_weight_names(wbf)
    assert sorted(names) == sorted("transformer_blocks.%d.%s.weight" % (i, n) for i in range(3) for n in FP8_LINEARS)


def test_helper_routes_six_linears_per_layer_and_nothing_else():
    ocfg, wbf, hs, ehs, ts, rope = _case()
    with fp8_linears(wbf) as plain_count:       # counts only: how many F.linear calls the forward makes in all
        pass
    original = F.linear
    with fp8_linears(wbf) as stats:
        assert F.linear is not original
        e4m3 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    assert F.linear is original
    assert stats["weights"] == 6 * ocfg.num_layers
    assert stats["routed"] == 6 * ocfg.num_layers and plain_count["routed"] == 0
    # every other linear of the forward went to torch untouched: count them with an empty pointer set
    with fp8_linears({}) as none:
        bf16 = dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope)
    assert none["routed"] == 0 and none["other"] == stats["routed"] + stats["other"]
    # ... and an empty routing is the plain bf16-eager forward
    assert torch.equal(bf16, dit_oracle.dit_forward(ocfg, wbf, hs, ehs, ts, rope))
    ref = dit_oracle.dit_forward(ocfg, {k: v.float() for k, v in wbf.items()}, hs.float(), ehs.float(), ts, rope)
    assert e4m3.dtype == BF and not torch.equal(e4m3, bf16)
    e_fp8, e_bf16, d = rel(e4m3, ref), rel(bf16, ref), rel(e4m3, bf16)
    print("e4m3-eager vs fp32 %.3e, bf16-eager vs fp32 %.3e, e4m3-eager vs bf16-eager %.3e" % (e_fp8, e_bf16, d))
    assert e_bf16 < e_fp8 < 0.5 and d > 0


def test_helper_restores_linear_when_the_body_raises():
    ocfg, wbf, *_ = _case()
    original = F.linear
    with pytest.raises(RuntimeError, match="boom"):
        with fp8_linears(wbf):
            assert F.linear is not original
            raise RuntimeError("boom")
    assert F.linear is original
    # an error inside a routed call (shape mismatch in fp8_oracle.linear) leaves the wrapper installed until the context ends
    w = wbf["transformer_blocks.0.attn1.to_q.weight"]
    with pytest.raises(RuntimeError):
        with fp8_linears(wbf):
            F.linear(torch.zeros(2, w.shape[1] + 1, dtype=BF), w)
    assert F.linear is original
