"""The OFFSET form of the default d = 64 statement (scripts/gen_attn_pipe.py, configure(8, offset=True) ->
alg_amd/csrc/attn_pipe_off_loop.inc, ALG_ATTN_PP=8) in the instruction-level emulator, driven the way attention.hip's frame drives
it -- next to attn_emu.run_pipe8_statement, whose problem class, LDS staging and lane maps it shares -- and a model of that frame's
control flow (which tiles a wave runs inside the statement, which in the C++ straight loop) for the path counters of
alg_attn_path_tap."""
import numpy as np

import attn_emu as H  # (puts scripts/ on the path)
import asm_emu  # noqa: E402

KVB = H.KVB


def frame_path(T, ragged, refused=()):
    """flash_attn_d64_pipe_kernel<8, true>'s loop for ONE wave: tile 0 in the straight form, entry at every t = 1 (mod 4) with
    t + 4 <= tend, whole groups of four inside, a tile in `refused` (row sum >= 2^80 inside the statement) leaves with code 1, is
    redone in the straight form, which then runs up to the next entry point.  -> (entries, tiles inside, tiles straight)."""
    tend = T - 4 if ragged else T - 3
    t, top_done, entries, inside = 0, False, 0, 0
    while True:
        tt = t + 1 if top_done else t
        ta = tt + ((1 - tt) & 3)
        if ta + 4 > tend:
            return entries, inside, T - inside
        t0 = t = ta
        entries += 1
        top_done = False
        while True:                              # the statement: iterations until a refusal or the end of the last whole group
            if t in refused:
                top_done = True
                break
            t += 1
            if (t & 3) == 1 and t + 4 > tend:
                break
        inside += t - t0


def pp4_path(T, ragged, all_zero, refused=()):
    """flash_attn_d64_pipe_kernel<8>'s (ALG_ATTN_PP=4) path of one wave: one entry at t = 1 if every row's offset snapped to zero,
    never again after a refusal."""
    tend = T - 4 if ragged else T - 3
    if not all_zero or 1 + 4 > tend:
        return 0, 0, T
    t = 1
    while True:
        if t in refused:
            break
        t += 1
        if (t & 3) == 1 and t + 4 > tend:
            break
    return 1, t - 1, T - (t - 1)


def run_pipe8_off_statement(pb, m_run, lazy_reads, lazy_dma, t0=1, mutate=None, zero_form=False):
    """The offset statement for one 256-query unit (eight waves x 32 queries), entered at t0 with the per-query running offsets
    m_run [Sq] (log2 units; float32) after tiles 0 .. t0 - 1 were folded into (l, O) against those offsets by `the frame` (numpy).
    zero_form: the SAME harness around the existing zero-offset statement (needs m_run == 0).
    -> dict(O [Sq, 64] unnormalised, l [Sq], t_exit, codes [8], scores {(wave, 'SA' | 'SB'): [32 keys.., 64 lanes] raw registers},
            probs: the packed P registers, lines)."""
    import gen_attn_pipe as GP
    assert pb.d == 64 and pb.prescaled and not pb.ragged
    GP.configure(8, offset=not zero_form)
    lines = GP.emit()
    regs = dict(SA=GP.SA, SB=GP.SB, PA=GP.PA, PB=GP.PB)
    GP.configure(8)
    if mutate is not None:
        lines = mutate(lines)
    m_run = np.asarray(m_run, dtype=np.float32)
    assert not zero_form or not m_run.any()
    T, TILE, NW = pb.T, 8192, 8
    tend = T - 3
    KL, VL = 0, 4 * TILE
    tab = {"o%d" % i: "a%d" % (80 + i) for i in range(32)}
    names_v = ["l", "kvo0", "vvo0", "qvo"] + ["lk%d" % i for i in range(4)] + (["lv%d" % i for i in range(4)] if zero_form else ["negm"])
    for i, n in enumerate(names_v):
        tab[n] = "v%d" % i
    assert len(names_v) <= (26 if zero_form else 10)          # the offset form owns v[10:25]
    for i, n in enumerate(("t", "code", "kstep", "tend", "wk", "wv")):
        tab[n] = "s%d" % i
    for i, n in enumerate(("kb", "vb", "qb")):
        tab[n] = "s[%d:%d]" % (8 + 2 * i, 9 + 2 * i)
    m = asm_emu.Machine(asm_emu.bind(lines, tab), n_waves=NW, gmem=pb.gmem, lazy_reads=lazy_reads, lazy_dma=lazy_dma)
    qf, kf, vf = pb.q.astype(np.float64), pb.k.astype(np.float64), pb.v.astype(np.float64)
    s_all = qf @ kf.T                                      # log2 units already
    with np.errstate(all="ignore"):
        e_all = np.exp2(s_all - m_run.astype(np.float64)[:, None])
    probs = lambda t: H.bf16_round(e_all[:, t * KVB:(t + 1) * KVB]).astype(np.float64)
    fsum = lambda t: e_all[:, t * KVB:(t + 1) * KVB].astype(np.float32).astype(np.float64).sum(axis=1)
    O, l = np.zeros((pb.Sq, 64)), np.zeros(pb.Sq)
    for t in range(t0):
        O += probs(t) @ vf[t * KVB:(t + 1) * KVB]
        l += fsum(t)

    def stage8(which, tile):
        for wave in range(NW):
            tid = wave * 64 + np.arange(64)
            row, slot = tid >> 3, (tid & 7) ^ ((tid >> 4) & 7)
            for ln in range(64):
                if which == "k":
                    src = pb.KOFF + ((tile * KVB + row[ln]) * pb.k_rs + slot[ln] * 8) * 2
                    dst = KL + (tile & 3) * TILE + wave * 1024 + ln * 16
                else:
                    src = pb.VOFF + (row[ln] * pb.vt_rs + slot[ln] * 8 + tile * KVB) * 2
                    dst = VL + (tile & 3) * TILE + wave * 1024 + ln * 16
                m.lds[dst:dst + 16] = pb.gmem[src:src + 16]
    for t in range(t0 - 1, t0 + 3):
        stage8("k", t)
    for t in range(t0 - 1, t0 + 2):
        stage8("v", t)

    def sset(w, name, val):
        r = asm_emu.parse_reg(tab[name])
        w.s[r[1]] = np.uint32(int(val) & 0xFFFFFFFF)
        if r[2] == 2:
            w.s[r[1] + 1] = np.uint32(int(val) >> 32)

    def vset(w, name, arr):
        a = np.asarray(arr)
        w.v[asm_emu.parse_reg(tab[name])[1]] = a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64).astype(np.uint32)
    for w in m.waves:
        lane = np.arange(64)
        l31, h2, tid = lane & 31, lane >> 5, w.id * 64 + lane
        q_row = w.id * 32 + l31
        srow, sslot = tid >> 3, (tid & 7) ^ ((tid >> 4) & 7)
        sset(w, "t", t0), sset(w, "tend", tend), sset(w, "kstep", KVB * pb.k_rs * 2)
        sset(w, "wk", KL + w.id * 1024), sset(w, "wv", VL + w.id * 1024)
        sset(w, "kb", pb.KOFF), sset(w, "vb", pb.VOFF), sset(w, "qb", pb.QOFF)
        vset(w, "qvo", (q_row * pb.q_rs + h2 * 8) * 2)
        vset(w, "l", np.where(h2 == 0, l[q_row], 0.0).astype(np.float32))
        if not zero_form:
            vset(w, "negm", (np.float32(0.0) - m_run[q_row]).astype(np.float32))        # the frame's 0.0f - m_run
        for ks in range(4):
            fl = l31 * 128 + (((2 * ks + h2) ^ ((l31 >> 1) & 7)) * 16)
            vset(w, "lk%d" % ks, KL + fl)
            if zero_form:
                vset(w, "lv%d" % ks, VL + fl)
        vset(w, "kvo0", (((t0 + 3) * KVB + srow) * pb.k_rs + sslot * 8) * 2)
        vset(w, "vvo0", (srow * pb.vt_rs + sslot * 8 + (t0 + 2) * KVB) * 2)
        for i in range(32):
            dt, e = i >> 4, i & 15
            drow = dt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2
            w.a[80 + i] = O[q_row, drow].astype(np.float32).view(np.uint32)
    with np.errstate(all="ignore"):
        m.run()
    t_exit = int(m.waves[0].s[asm_emu.parse_reg(tab["t"])[1]])
    t_exits = [int(w.s[asm_emu.parse_reg(tab["t"])[1]]) for w in m.waves]
    codes = [int(w.s[asm_emu.parse_reg(tab["code"])[1]]) for w in m.waves]
    O2, l2 = np.zeros((pb.Sq, 64), dtype=np.float32), np.zeros((pb.Sq, 2), dtype=np.float32)
    raw = {}
    for w in m.waves:
        lane = np.arange(64)
        l31, h2 = lane & 31, lane >> 5
        q_row = w.id * 32 + l31
        l2[q_row, h2] = w.v[asm_emu.parse_reg(tab["l"])[1]].view(np.float32)
        for i in range(32):
            dt, e = i >> 4, i & 15
            drow = dt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2
            O2[q_row, drow] = w.a[80 + i].view(np.float32)
        for name, base in regs.items():
            n = 32 if name[0] == "S" else 16
            raw[(w.id, name)] = np.stack([w.v[base + i].copy() for i in range(n)])
    return dict(O=O2, l=l2, t_exit=t_exit, t_exits=t_exits, codes=codes, raw=raw, lines=lines, probs=probs, fsum=fsum, vf=vf)


def finish(pb, r):
    """the frame's tail in numpy (tiles t_exit .. T - 1 against the same offsets) and the normalisation -> [Sq, 64] float64"""
    O2, l2 = r["O"].astype(np.float64), r["l"].astype(np.float64).sum(axis=1)
    for t in range(r["t_exit"], pb.T):
        O2 = O2 + r["probs"](t) @ r["vf"][t * KVB:(t + 1) * KVB]
        l2 = l2 + r["fsum"](t)
    return O2 / l2[:, None]


def score_tile(r, wave, name):
    """a wave's S register block (32 registers x 64 lanes, as left by the statement) -> scores [32 queries, 64 keys] float32:
    sub-tile `sub` register e of lane (l31, h2) <-> key 32 sub + (e & 3) + 8 (e >> 2) + 4 h2 of query l31"""
    regs = r["raw"][(wave, name)].view(np.float32)
    out = np.zeros((32, 64), dtype=np.float32)
    for sub in range(2):
        for e in range(16):
            for h2 in range(2):
                out[:, 32 * sub + (e & 3) + 8 * (e >> 2) + 4 * h2] = regs[16 * sub + e, 32 * h2:32 * h2 + 32]
    return out


def prob_tile(r, wave, name):
    """a wave's packed P block (16 registers: register n = the bf16 pair of score registers 2n, 2n + 1) -> [32 queries, 64 keys]"""
    regs = r["raw"][(wave, name)]
    lo = asm_emu.bf16_to_f32((regs & 0xFFFF).astype(np.uint16))
    hi = asm_emu.bf16_to_f32((regs >> 16).astype(np.uint16))
    out = np.zeros((32, 64), dtype=np.float32)
    for n in range(16):
        for half, vals in ((0, lo), (1, hi)):
            sreg = 2 * n + half
            sub, e = sreg >> 4, sreg & 15
            for h2 in range(2):
                out[:, 32 * sub + (e & 3) + 8 * (e >> 2) + 4 * h2] = vals[n, 32 * h2:32 * h2 + 32]
    return out
