#!/usr/bin/env python3
"""Generates alg_amd/csrc/attn_pipe_loop.inc: the steady-state KV loop of the d = 64 attention as ONE inline-asm statement.

Why (profiles/r3_attention_d64_mix_microbench.txt): on gfx950 matrix and vector work of DIFFERENT waves of a SIMD do not
overlap, vector work issued by the SAME wave right behind its own MFMA does -- 1 MFMA + {2 v_exp, 1 v_cvt_pk_bf16_f32, 2 v_add,
1 ds_read_b128} costs 18.3 ns of SIMD time against 16.3 ns for the MFMA alone, while the straight loop of attention.hip (QK ->
softmax -> PV, each phase on its own) spends 28.6 ns per MFMA.  (v_dot2c_f32_bf16 does NOT hide: +7 ns per MFMA; plain adds do.)

The loop is software-pipelined over KV tiles of 64: iteration t issues, per wave (32 queries; a workgroup is eight waves = one 256-query unit),
    PV(t-1): O^T += V(t-1)^T P(t-1)^T      8 MFMAs, A = V^T fragments from LDS, B = P(t-1) (registers), C/D = a[0:31]
    QK(t+1): S(t+1)^T = K(t+1) Q^T         8 MFMAs, A = K fragments from LDS,   B = Q (registers), first k-step from C = 0
    softmax(t): P(t) = bf16(exp2(S(t))), row sum     16 score pairs, ONE PAIR PER MFMA GAP: exp, exp, cvt_pk (of the previous
                                                     pair), add, add -- none of it depends on this iteration's MFMAs
Scores arrive in log2 units with the running offset at zero (attention.hip, softmax_tile_zero's common path): the statement is
entered only by waves whose offsets are all zero and leaves as soon as a tile's row sum leaves [0, 2^80) -- the exact path
(tile max, rescale) stays in C++.

Collective protocol (identical in the C++ loop around the statement, so waves of one workgroup may be in either): at the top
of iteration t   s_waitcnt vmcnt(2); s_barrier;  DMA K(t+3) -> K slot (t+3) & 3, V^T(t+2) -> V slot (t+2) & 3   (1 KiB = one
instruction per wave and tile each; the counted wait leaves the previous iteration's two in flight: two tiles of prefetch).
Iteration t reads K(t+1), V(t-1) (pipelined form) or K(t), V(t) (straight form): all resident in the 4-slot rings.

Unrolled x 4 (ring slot = t & 3 as immediates; the S / P register roles alternate with t & 1).  Entered at t = 1 (mod 4) through
a warm-up (QK(t) on its own; no PV: the caller has finished tile t-1), runs whole groups of four while t + 4 <= t_end, then
drains PV of its last tile.  Register plan (named literally, clobbered):
    v[26:57]  SA   v[58:89] SB      score tiles (sub-tile 0: +0..15, sub-tile 1: +16..31); roles alternate
    v[90:105] PA   v[106:121] PB    packed probabilities: register n = pair (S[2n], S[2n+1])
    v122 tile sum, v[123:126] exp results in flight, v127 scratch
    a[0:31]   O^T accumulators (two 32x32 tiles)
    a[32:63]  eight fragment buffers (ring, one per MFMA, read four MFMAs ahead; ds_read_b128 straight into AccVGPRs)
    a[64:79]  Q fragments (loaded by the statement: four 16-byte pieces per lane)
(hipcc grants an 8-wave workgroup 128 + 128 registers per lane: v[0:25] are the frame's, O travels in AccVGPR operands)
Operands: o0..o31 "+a" (O^T elements, moved to / from a[0:31]), l "+v" running row sum, t "+s" iteration index (in: first
iteration, = 1 mod 4; out: the iteration the caller continues with), code "=s" (0: t's top-of-iteration protocol NOT done,
caller continues normally; 1: row-sum check failed in iteration t -- its protocol, PV(t-1) and QK(t+1) are done, softmax(t)
is not: the caller redoes tile t from QK), lk0..lk3 / lv0..lv3 "v" LDS byte address of the lane's K / V^T fragment per
k-step (ring base included; slot and sub-tile are immediates), kvo0, vvo0 "+v" DMA byte offsets of this lane (row srow)
into the K / V^T panels AT TILE (t + 3) / (t + 2) of the entry iteration (advanced inside), qvo "v" byte offset of the lane's Q row, kb / vb /
qb "s" 64-bit panel bases, kstep "s" bytes per K tile, tend "s" (whole groups of four run while t + 4 <= tend; the caller guarantees t + 3 < T inside),
wk / wv "s" = LDS byte address of the K / V^T ring + wave * 1024 (DMA destination of this wave).

Offset mode (configure(8, offset=True) -> attn_pipe_off_loop.inc, ALG_ATTN_PIPE8_OFF_*; attention.hip, ALG_ATTN_PP=8): the same
8-wave statement for waves whose rows keep a NON-ZERO running offset m (first-tile scores beyond +-64 log2 units).  In the
S^T = K Q^T layout the 16 accumulator values a lane holds of a 32 x 32 block all belong to ONE query, so -m rides in as srcC of the
first QK k-step of both sub-tiles (that k-step starts from C = 0 in the zero-offset form): the scores come out of the matrix pipe as
s - m, with -m FIRST in the fp32 accumulation chain, and the softmax mix, the DMA / barrier protocol, `code` and the 2^80 exit are
unchanged -- no VALU instruction is added to the loop.  m does not change inside the statement (the lazy max stays the frame's).
One extra operand: negm "+v" = -m of the lane's query (never written: "+" so that the frame reads its m back from it and keeps no
register of its own live across the statement); the warm-up copies it into the literal block v[10:25] (16 v_mov_b32 per entry).  The block has to be ArchVGPRs: a VOP3P-MAI instruction has ONE bit for the register file of srcC and vdst together, the
scores must land in ArchVGPRs (v_exp_f32 reads no AccVGPR), so an AccVGPR srcC cannot be encoded with them.  The 16 registers come
out of the frame's share v[0:25]: the four V^T fragment addresses lv0..lv3 are dropped -- the V^T ring lies 32 KiB behind the K ring
in one LDS block, and 32768 + slot * 8192 + half * 4096 still fits the 16-bit offset field of ds_read_b128 -- which leaves nine
"v" operands (l, kvo0, vvo0, qvo, lk0..lk3, negm) for v[0:9].

(The 4-wave form of the statement, ALG_ATTN_PP=3, and three round-5 experiment knobs -- one fragment wait per two MFMAs, softmax
work in place of the s_nop behind an M0 write, row sums on the matrix pipe -- are in the history; their measurements are in
profiles/r3_attention_pipe_bench_ab.txt and docs/lab_notebook_r5.md.)
"""
import os

OACC, FR, Q = 0, 32, 64        # AccVGPRs: O^T tiles, fragment ring, Q fragments
VBASE = 26                     # first ArchVGPR of the statement (hipcc grants an 8-wave workgroup 128 + 128 registers per lane)
SA, SB, PA, PB = VBASE, VBASE + 32, VBASE + 64, VBASE + 80
TS, E0, E1, E2, E3, SCR = (VBASE + 96 + i for i in range(6))
OFFSET = False                 # offset mode (configure(8, offset=True)): -m as srcC of the first QK k-step
NEGM, V_RING = 10, 32768       # offset mode: v[10:25] = -m of the lane's query; LDS distance K ring -> V^T ring


def configure(nw=8, offset=False):
    """the 8-wave statement: zero-offset form (attn_pipe_loop.inc) or offset mode (attn_pipe_off_loop.inc).
    nw is not consulted: the statement exists in the 8-wave form only, and callers written when there was a 4-wave form, which
    put that one back with configure(4) after use, get the zero-offset 8-wave form -- what every caller configures first anyway."""
    global OFFSET
    OFFSET = offset


TILE = 8192

v = lambda i: "v%d" % i
vr = lambda i, n: "v[%d:%d]" % (i, i + n - 1)
ar = lambda i, n: "a[%d:%d]" % (i, i + n - 1)


def frag_read(buf, which, slot, half, kstep):
    """ds_read_b128 of one fragment: K (which = 'k') sub-tile `half` k-step `kstep`, or V^T d-tile `half` kv block `kstep`"""
    # address = lane part(kstep) (carries the ring base) + slot * TILE + half * 4096
    if OFFSET and which == "v":     # no lv operands: the V^T ring through the K fragment address (same lane part) + 32 KiB
        return "ds_read_b128 %s, %%[lk%d] offset:%d" % (ar(FR + 4 * buf, 4), kstep, V_RING + slot * TILE + half * 4096)
    return "ds_read_b128 %s, %%[l%s%d] offset:%d" % (ar(FR + 4 * buf, 4), which, kstep, slot * TILE + half * 4096)


def softmax_gap(S, P, n, first, last_of_tile=False):
    """VALU work of one MFMA gap: exp2 of pair n (if n < 16), pack + row sum of pair n - 1 (if n >= 1).
    Pair n lives in E0/E1 (n even) or E2/E3 (n odd) until it is packed in the next gap."""
    out = []
    ea, eb = (E0, E1) if n % 2 == 0 else (E2, E3)
    pa, pb = (E2, E3) if n % 2 == 0 else (E0, E1)   # previous pair
    if n >= 1:
        out.append("v_cvt_pk_bf16_f32 %s, %s, %s" % (v(P + n - 1), v(pa), v(pb)))
        if n - 1 == 0:
            out.append("v_add_f32 %s, %s, %s" % (v(TS), v(pa), v(pb)))
        else:
            out.append("v_add_f32 %s, %s, %s" % (v(SCR), v(pa), v(pb)))
            out.append("v_add_f32 %s, %s, %s" % (v(TS), v(TS), v(SCR)))
    if n < 16:
        out.append("v_exp_f32 %s, %s" % (v(ea), v(S + 2 * n)))
        out.append("v_exp_f32 %s, %s" % (v(eb), v(S + 2 * n + 1)))
    return out


def top_protocol(phase, spread=False):
    """top of iteration t (t & 3 == phase): all but the previous iteration's four DMAs have landed (K(t+1), V(t) and older),
    everybody is done with iteration t - 1; then this wave's share of K(t+3) and V^T(t+2) -- two tiles ahead, into the slots of
    K(t-1) / V^T(t-2): one 1 KiB piece each (eight waves stage an 8 KiB tile).
    spread: returns (head, groups) -- the four DMAs go out one per MFMA gap behind the barrier instead of as a block"""
    ks, vs = (phase + 3) & 3, (phase + 2) & 3
    head = ["s_waitcnt vmcnt(2)", "s_barrier"]
    groups = [["s_add_u32 m0, %%[wk], %d" % (ks * TILE), "s_nop 0",
               "global_load_lds_dwordx4 %[kvo0], %[kb]", "v_add_u32 %[kvo0], %[kstep], %[kvo0]"],
              ["s_add_u32 m0, %%[wv], %d" % (vs * TILE), "s_nop 0",
               "global_load_lds_dwordx4 %[vvo0], %[vb]", "v_add_u32 %[vvo0], 0x80, %[vvo0]"]]
    if spread:
        return head, groups
    return head + [ln for g in groups for ln in g]


def first_reads(phase):
    """the first four fragment reads of a full iteration at `phase`: V^T(t-1) kv blocks 0, 1 for both d-tiles.  They do not
    depend on the iteration's barrier (V^T(t-1) landed two iterations earlier), so the PREVIOUS iteration issues them behind its
    twelfth MFMA (buffers 0-3 are free from there on) and the LDS latency hides under the top-of-iteration wait + barrier."""
    vslot = (phase - 1) & 3
    return [frag_read(j, "v", vslot, half, kstep) for j, (half, kstep) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)])]


def iteration(phase, X, Y, U, W, pv=True, softmax=True, qk=True, reads_in_flight=False, prefetch_next=None, dma_groups=None,
              pre_exp=False):
    """one pipelined iteration at ring phase t & 3 == phase.  MFMA stream (16, or 8 without PV): the four PV MFMAs of kv blocks
    0, 1 first (their V^T fragments do not depend on this iteration's barrier), then QK and PV alternating, QK last."""
    kslot, vslot = (phase + 1) & 3, (phase - 1) & 3
    mf = []   # (kind, half, kstep)
    if pv:
        mf += [("v", 0, 0), ("v", 1, 0), ("v", 0, 1), ("v", 1, 1)]
        rest_v = [("v", 0, 2), ("v", 1, 2), ("v", 0, 3), ("v", 1, 3)]
    else:
        rest_v = []
    qks = [("k", s, ks) for ks in range(4) for s in range(2)] if qk else []
    # alternate: QK, PV, QK, PV, ... then the remaining QKs
    i = 0
    while rest_v or qks[i:]:
        if qks[i:]:
            mf.append(qks[i]); i += 1
        if rest_v:
            mf.append(rest_v.pop(0))
    n_m = len(mf)
    lines = []
    AHEAD = 4
    def read(j):
        kind, half, kstep = mf[j]
        return frag_read(j % 8, kind, kslot if kind == "k" else vslot, half, kstep)
    if not reads_in_flight:
        for j in range(min(AHEAD, n_m)):
            lines.append(read(j))
    pair = 1 if (softmax and pre_exp) else 0     # pre_exp: the caller has issued the two exps of pair 0 (softmax_pre)
    n_pairs = 16 if softmax else 0
    # pairs per gap: spread 17 VALU groups (16 exps + the trailing pack) over the gaps
    per_gap = max(1, 16 // n_m) if softmax else 0
    seen_first = {"k0": False, "k1": False}
    for j, (kind, half, kstep) in enumerate(mf):
        outstanding = (AHEAD if prefetch_next is not None else min(AHEAD, n_m - j)) - 1   # reads issued after read j
        lines.append("s_waitcnt lgkmcnt(%d)" % outstanding)
        fr = ar(FR + 4 * (j % 8), 4)
        if kind == "k":
            acc = vr(Y + 16 * half, 16)
            c = acc if seen_first["k%d" % half] else (vr(NEGM, 16) if OFFSET else "0")
            seen_first["k%d" % half] = True
            lines.append("v_mfma_f32_32x32x16_bf16 %s, %s, %s, %s" % (acc, fr, ar(Q + 4 * kstep, 4), c))
        else:
            acc = ar(16 * half, 16)
            lines.append("v_mfma_f32_32x32x16_bf16 %s, %s, %s, %s" % (acc, fr, vr(U + 4 * kstep, 4), acc))
        if j + AHEAD < n_m:
            lines.append(read(j + AHEAD))
        elif prefetch_next is not None and j + AHEAD - n_m < AHEAD:
            lines.append(first_reads(prefetch_next)[j + AHEAD - n_m])   # next iteration's reads 0..3 behind MFMAs 12..15
        if dma_groups and j < len(dma_groups):
            lines += dma_groups[j]                                   # one DMA per gap behind the barrier
        for g in range(per_gap):
            if softmax and pair <= 16:
                if g > 0:
                    lines.append("s_nop 1")     # the pack below reads what the two exps just above wrote (trans -> VALU use)
                lines += softmax_gap(X, W, pair, pair == 0)
                pair += 1
    while softmax and pair <= 16:
        lines.append("s_nop 1")
        lines += softmax_gap(X, W, pair, False)
        pair += 1
    return lines


def softmax_pre(S):
    """the two exps of score pair 0, issued AHEAD of the top-of-iteration wait + barrier (the scores are complete)"""
    return ["v_exp_f32 %s, %s" % (v(E0), v(S)), "v_exp_f32 %s, %s" % (v(E1), v(S + 1))]


def check_and_count(fail_label):
    """row-sum check of the iteration just issued, then t += 1"""
    return ["v_cmp_ngt_f32 vcc, 0x67800000, %s" % v(TS), "s_nop 4", "s_cbranch_vccnz %s" % fail_label,   # !(2^80 > sum)
            "v_add_f32 %%[l], %%[l], %s" % v(TS), "s_add_u32 %[t], %[t], 1"]


def emit():
    L = []
    # ---- entry: O -> a[0:31], Q fragments, constants ----
    L += ["v_accvgpr_mov_b32 a%d, %%[o%d]" % (i, i) for i in range(32)]
    L += ["global_load_dwordx4 %s, %%[qvo], %%[qb] offset:%d" % (ar(Q + 4 * ks, 4), 32 * ks) for ks in range(4)]
    roles = {1: (SA, SB, PA, PB), 2: (SB, SA, PB, PA), 3: (SA, SB, PA, PB), 0: (SB, SA, PB, PA)}
    # ---- warm-up at phase 1: top protocol, QK(t) alone into X = SA (K(t) sits in slot 1 = the "next" slot of phase 0) ----
    if OFFSET:
        L += ["v_mov_b32 %s, %%[negm]" % v(NEGM + i) for i in range(16)]   # under the latency of the Q loads
    L += ["s_waitcnt vmcnt(0) lgkmcnt(0)"]   # Q (and, once, whatever the caller had in flight)
    L += top_protocol(1)
    X, Y, U, W = roles[1]
    L += iteration(0, Y, X, U, W, pv=False, softmax=False)      # phase 0's "next" K slot is slot 1: S(t) -> SA
    L += ["s_nop 15", "s_nop 15"]                                  # S(t) complete before the first exp reads it
    L += iteration(1, X, Y, U, W, pv=False, prefetch_next=2)      # QK(t+1) -> SB under softmax(t) -> PB
    L += check_and_count("90f")
    L += ["s_branch 12f"]
    # ---- the loop: phases 1, 2, 3, 0 ----
    L += ["11:"]
    for ph in (1, 2, 3, 0):
        if ph == 2:
            L += ["12:"]
        X, Y, U, W = roles[ph]
        head, groups = top_protocol(ph, spread=True)
        L += softmax_pre(X) + head
        L += iteration(ph, X, Y, U, W, reads_in_flight=True, prefetch_next=(ph + 1) & 3, dma_groups=groups, pre_exp=True)
        L += check_and_count("90f")
    # after phase 0: t = 1 (mod 4) again.  Another whole group?  (t + 4 <= tend)
    L += ["s_add_u32 %[code], %[t], 4", "s_cmp_le_u32 %[code], %[tend]", "s_cbranch_scc1 11b"]
    # ---- drain: PV of the last tile (P in PB after phase 0: W of phase 0 = PA? roles[0] = (SB, SA, PB, PA): W = PA) ----
    X, Y, U, W = roles[0]
    L += iteration(1, Y, X, W, U, pv=True, softmax=False, qk=False, reads_in_flight=True)   # V slot (1 - 1) & 3 = slot of tile t - 1
    L += ["s_mov_b32 %[code], 0", "s_branch 99f"]
    # ---- failed row-sum check in iteration t: its MFMAs are issued; leave with code 1 ----
    L += ["90:", "s_mov_b32 %[code], 1"]
    L += ["99:", "s_nop 15", "s_nop 15"]
    L += ["v_accvgpr_mov_b32 %%[o%d], a%d" % (i, i) for i in range(32)]
    L += ["s_waitcnt lgkmcnt(0)"]
    return L


def write_form(f, tag):
    lines = emit()
    f.write("#define ALG_ATTN_PIPE%s_LOOP_ASM \\\n" % tag)
    for ln in lines:
        f.write('  "%s\\n\\t" \\\n' % ln)
    f.write('  ""\n')
    regs = ["a%d" % i for i in range(80)] + ["v%d" % i for i in range(NEGM if OFFSET else VBASE, VBASE + 102)]
    f.write("#define ALG_ATTN_PIPE%s_CLOBBERS \\\n  " % tag + ", ".join('"%s"' % r for r in regs) + '\n')
    f.write("#define ALG_ATTN_PIPE%s_O_OPERANDS(o) \\\n  " % tag +
            ", ".join('[o%d] "+a"(o[%d])' % (i, i) for i in range(32)) + '\n')
    return lines


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.environ.get("ATTN_PIPE_OUT") or os.path.join(here, "..", "alg_amd", "csrc", "attn_pipe_loop.inc")
    with open(path, "w") as f:
        f.write("// GENERATED by scripts/gen_attn_pipe.py -- do not edit.  Steady-state KV loop of the pipelined d = 64 attention.\n")
        configure()
        lines = write_form(f, "8")
        print("wrote", os.path.normpath(path), len(lines), "lines,", sum(1 for l in lines if l.startswith("v_mfma")), "MFMAs")
    path = os.environ.get("ATTN_PIPE_OFF_OUT") or os.path.join(here, "..", "alg_amd", "csrc", "attn_pipe_off_loop.inc")
    with open(path, "w") as f:
        f.write("// GENERATED by scripts/gen_attn_pipe.py -- do not edit.  The 8-wave statement of the pipelined d = 64 attention for any\n"
                "// running offset: -m is srcC of the first QK k-step (ALG_ATTN_PP=8).\n")
        configure(8, offset=True)
        lines = write_form(f, "8_OFF")
        print("wrote", os.path.normpath(path), "offset form", len(lines), "lines,", sum(1 for l in lines if l.startswith("v_mfma")), "MFMAs")
    configure()


if __name__ == "__main__":
    main()
