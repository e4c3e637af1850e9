"""Test helper: attn_bias_kernel of csrc/t5.hip restated in plain torch on the flat arenas of tests/helpers/enc_attn_arena.py, with
the kernel's own addressing: per (b, h) the staging of K^T [DH][Lp] and V [Lp][DH] from k / v + (b L + j) qkv_rs + h DH with zero
fill of the key slots [L, Lp); 32 query rows per workgroup, wave w taking rows row0 + w, + 4, ...; scores per 64-key chunk with
the validity test `j < L && mask && causal`; the `lane + 64 < DH` half of q, of p v and of the store; the stores at
out + (b L + i) out_rs + h DH.  float32 arithmetic with the kernel's roundings (exact on the data of both families but for exp).

`mutant` switches on ONE way such a kernel goes wrong (MUTANTS); tests/test_enc_attn_arena_cpu.py shows that the assertions of the
arena helper catch each.  Indices a mutant pushes past a table (the bucket LUT, the mask) are clamped to the table: the emulation
reads what is there, as a kernel would read its neighbour."""
import torch

from helpers import enc_attn_arena as E

BF = torch.bfloat16
MUTANTS = (
    "bias_i_minus_j",          # bias indexed by i - j
    "bias_other_head",         # bias taken from another head's column
    "bias_table_transposed",   # bias table read as [heads][buckets]
    "mask_batch0",             # batch 0's mask used for every item
    "mask_ignored",
    "causal_strict",           # causal j < i
    "causal_ignored",
    "key_bound_Lp",            # key bound j < Lp in place of j < L
    "qk_drop_hi",              # columns >= 64 dropped in q . k at head_dim 80
    "pv_drop_hi",              # columns >= 64 dropped in p v at head_dim 80
    "kt_pair_swapped",         # the two halves of a packed K pair swapped in the transpose
    "head_off_64",             # head offset h * 64 at head_dim 80
    "last_wg_skipped",         # the last partial workgroup's rows skipped
    "tail_mod4_skipped",       # rows with i % 4 != 0 in the tail skipped
    "out_pitch_inner",         # out stored at pitch inner
    "out_rows_ge_L",           # out stored for rows >= L
)


def _rbf(x):
    return x.to(BF).float()


def emulate(call, out_full, mutant=None):
    """The call on the arenas of `call` into out_full (CPU tensors)."""
    assert mutant is None or mutant in MUTANTS
    data, d, L = call.data, call.d, call.L
    Lp, CH = (L + 63) // 64 * 64, d // 8
    nchunk, rows_per_wg = Lp >> 6, 32
    full, qkv_rs = call.qkv, call.qkv_rs
    out_rs = call.inner if mutant == "out_pitch_inner" else call.out_rs
    scale = torch.tensor(data.scale, dtype=torch.float32)
    ar = torch.arange
    for b in range(E.B):
        for h in range(E.H):
            hoff = h * (64 if mutant == "head_off_64" else d)
            # ---- staging: element e = j * CH + chunk of 8 columns; K^T [d][Lp], V [Lp][d], zeros for j >= L
            e = ar(Lp * CH)
            j, c = e // CH, (e % CH) * 8
            live = (j < L).reshape(-1, 1)
            src = (b * L + torch.where(j < L, j, 0)).reshape(-1, 1) * qkv_rs + hoff + c.reshape(-1, 1) + ar(8).reshape(1, 8)
            kv = torch.where(live, full[call.k_off + src], torch.zeros((), dtype=BF))
            vv = torch.where(live, full[call.v_off + src], torch.zeros((), dtype=BF))
            V = torch.zeros(Lp, d, dtype=BF)
            KT = torch.zeros(d, Lp, dtype=BF)
            col = c.reshape(-1, 1) + ar(8).reshape(1, 8)
            V[j.reshape(-1, 1).expand(-1, 8), col] = vv
            KT[(col ^ 1) if mutant == "kt_pair_swapped" else col, j.reshape(-1, 1).expand(-1, 8)] = kv
            # ---- the rows this (b, h) computes, in launch order
            rows = []
            for wg in range((L + rows_per_wg - 1) // rows_per_wg):
                row0 = wg * rows_per_wg
                partial = row0 + rows_per_wg > L
                row1 = row0 + rows_per_wg if mutant == "out_rows_ge_L" else min(row0 + rows_per_wg, L)
                if partial and mutant == "last_wg_skipped":
                    continue
                for wave in range(4):
                    for i in range(row0 + wave, row1, 4):
                        if not (partial and mutant == "tail_mod4_skipped" and i % 4):
                            rows.append(i)
            if not rows:
                continue
            I = torch.tensor(rows).reshape(-1, 1)
            lanes = ar(d).reshape(1, d)          # lane, and lane + 64 where lane + 64 < DH
            qv = full[call.q_off + (b * L + I) * qkv_rs + hoff + lanes].float()
            dq = 64 if mutant == "qk_drop_hi" else d
            jj = ar(Lp).reshape(1, Lp)
            s = torch.empty(len(rows), Lp)
            for ck in range(nchunk):
                s[:, ck * 64:ck * 64 + 64] = qv[:, :dq] @ KT[:dq, ck * 64:ck * 64 + 64].float()
            valid = (jj < (Lp if mutant == "key_bound_Lp" else L)).expand(len(rows), Lp).clone()
            if call.mask is not None and mutant != "mask_ignored":
                mb = 0 if mutant == "mask_batch0" else b * L
                valid &= call.mask[(mb + jj).clamp(max=call.mask.numel() - 1)] != 0
            if data.causal and mutant != "causal_ignored":
                valid &= (jj < I) if mutant == "causal_strict" else (jj <= I)
            s = _rbf(s)
            if data.scale != 1.0:
                s = _rbf(s * scale)
            if call.table is not None:
                rel = (I - jj) if mutant == "bias_i_minus_j" else (jj - I)
                bucket = call.lut[(rel + L - 1).clamp(0, call.lut.numel() - 1)].long()
                hh = (h + 1) % E.H if mutant == "bias_other_head" else h
                idx = hh * E.NB + bucket if mutant == "bias_table_transposed" else bucket * E.H + hh
                s = _rbf(s + call.table[idx].float())
            s = torch.where(valid, s, torch.tensor(-float("inf")))
            m = s.max(dim=1, keepdim=True).values
            ex = torch.where(s > -float("inf"), torch.exp(s - torch.where(m > -float("inf"), m, torch.zeros_like(m))), torch.zeros_like(s))
            tot = ex.sum(dim=1, keepdim=True)
            inv = torch.where(tot > 0, 1.0 / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(tot))
            p = _rbf(ex * inv)
            o = p[:, :L] @ V[:L].float()
            if mutant == "pv_drop_hi":
                o[:, 64:] = 0.0
            out_full[call.out_off + (b * L + I) * out_rs + hoff + lanes] = o.to(BF)
    return out_full
