// Flash attention forward, head_dim 128, the LONG self-attention form of the Wan / HunyuanVideo DiTs: 64 queries per wave, one
// wave per SIMD, the steady-state KV loop ONE generated asm statement (round 5).
//
// Why 64 queries per wave: every K / V^T fragment read from LDS feeds TWO MFMAs (the wave's two 32-query halves) and a 64-key
// tile is staged once per 256 queries with four waves -- half the LDS instructions and half the L2 -> LDS traffic per FLOP of the
// 32-query kernels (attention128_pipe.hip, attention128.hip).  Round 4 shipped that idea with the MFMAs and fragment reads as
// separate inline-asm statements and everything between them scheduled by hipcc: 1280-1320 TFLOP/s at 62 % matrix-pipe busy, and
// a three-round hunt for a register hipcc recycled in the shadow of an MFMA it cannot see (profiles/r4_attention128_q64_probe.txt).
// Round 5 replaces that body by the construction of the 32-query statements: scripts/gen_attn_q64.py emits the whole steady
// state -- per 64-key tile and wave 64 MFMAs (PV(t-1) and QK(t+1)), 32 fragment reads, the 8 DMA pieces of the wave and the 224
// VALU instructions of softmax(t), each at a fixed place between two MFMAs -- as attn128_q64_loop.inc, and NO compiler-scheduled
// instruction sits between the first and the last MFMA of the statement (the hazard class of round 4 cannot occur: the statement
// ends behind s_nops that cover its last MFMA).  The generated text is checked on the CPU by an instruction-level emulator under
// the weakest memory ordering the ISA allows (tests/test_attn_q64_statement_cpu.py).
//
// This file is the frame, and everything in it is plain C++ the compiler sees whole: workgroup -> (head, q block) order, operand
// layouts and swizzles of attention128_pipe.hip, O as eight f32x16 values (handed to the statement as "+a" operands), a C++
// tile body for tile 0 (where the lazy running max is established), the last one or two tiles (the masked one) and any tile the statement
// refuses (row sum outside [0, 2^80): exact max / rescale), all under the statement's collective protocol
//     top of iteration t:  s_waitcnt vmcnt(8); s_barrier; DMA K(t+3) -> K slot (t+3) & 3, V^T(t+2) -> V slot (t+2) & 3
// so the waves of a workgroup may be inside or outside the statement independently.  A wave that left the statement RE-ENTERS
// it at the next t = 1 (mod 4) (round 4's single-statement kernels stayed outside for good).
//
// The same frame serves alg_flash_attn_d128_ranges (opt-in frame-window attention, alg_amd/attn_window.py): there a workgroup runs
// the key ranges of its row of a device table one after the other, each as a panel of its own, with one drain of the ring between
// two of them.  alg_flash_attn_d128_ranges_heads is the same instantiation with a table row per (head, q
// block) and an optional output of the log2-domain log-sum-exp of the visited keys (the recall policy of attn_window.py).
// alg_flash_attn_d128_ranges_order is that launch with its workgroups in an order the host computed (attn_window.balanced_order):
// workgroup b runs the unit order[b] and computes what it computes in the other entries.
// alg_flash_attn_d128_ranges_prefix is an instantiation of its own (PREFIX): the same frame over a table of up to 12 segments,
// which writes the log-sum-exp of the keys visited SO FAR behind every segment (the one-pass calibration of attn_window.py).
//
// DEFAULT for non-causal, ungrouped attention over at least ATTN128_Q64_POLICY_TILES KV tiles; ALG_ATTN128_Q64=0 switches it off
// (the 32-query pipelined kernel takes over), =2 takes every call of at least ATTN128_Q64_MIN_TILES tiles (tests).  That decision
// is attn128_plan's (attention128.hip); this file holds the kernel, its launch step and the ranged entries, which are checked
// and planned by the same two functions (attention128_host.h).
#include "attention128_host.h"
#include "attn128_q64_loop.inc"

namespace alg {
namespace a128q {

constexpr int NW = 4;
constexpr int QW = 64;                   // queries per wave
constexpr int KVB = 64;
constexpr int TILE = 16384;              // K tile = V^T tile
constexpr int LDS_BYTES = 8 * TILE;      // 4 K slots + 4 V^T slots

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

struct P {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* vt;
  bf16_t* o;
  int batch, heads, Sq, Skv, q_blocks;
  int64_t q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs;
  float scale_log2;
  uint64_t* clk;   // clock tap (calibrate.hip: alg_attn_clock_tap) or NULL
  int clk_slots;
  int use_statement;   // 0: every tile through the C++ tile body (ALG_ATTN128_Q64=3: tests of the frame on its own)
  const int32_t* ranges;   // RANGES: device table [q_blocks][max_ranges][2] of (begin, end) key indices (alg_flash_attn_d128_ranges)
  int max_ranges;
  // RANGES, alg_flash_attn_d128_ranges_heads only (0 and NULL from the other entries; the dense instantiation reads neither)
  int head_rows;           // q_blocks when the table has a leading head dimension ([heads][q_blocks][max_ranges][2]), else 0
  float* lse;              // fp32 [batch][heads][Sq]: log2-domain log-sum-exp of the scaled scores over the visited keys, or NULL
  // RANGES, alg_flash_attn_d128_ranges_order only (NULL and 0 from every other entry; the dense instantiation reads neither)
  const int32_t* order;    // device int32 [order_len]: the unit bh * q_blocks + qb workgroup b runs (negative: it exits), or NULL
  int order_len;           // = the grid
  // PREFIX, alg_flash_attn_d128_ranges_prefix only (NULL from every other entry; no other instantiation reads it)
  float* lse_prefix;       // fp32 [batch][heads][max_ranges][Sq]: entry i = the log-sum-exp over the keys of the segments 0 .. i
};

// RANGES = false: every key of the panel, ONE segment [0, Skv) -- the dense kernel.  RANGES = true: the workgroup's 256 queries
// visit the key ranges of their row of p.ranges one after the other; each range is a SEGMENT the frame runs exactly as the dense
// kernel runs a panel of that length whose K / V^T start at `begin` (prime the ring, tile 0 in C++, the statement from t = 1, the
// tail in C++), with O, the running max and the row sum carried from segment to segment.  PREFIX (with RANGES): behind every
// segment of the row, visited or skipped, the log-sum-exp of the keys visited so far goes to p.lse_prefix -- the epilogue's value,
// taken from the running state, which it leaves as it is.  An instantiation of its own: <true, false> keeps its code.
template <bool RANGES, bool PREFIX = false>
__global__ __launch_bounds__(NW * 64) void flash_attn_d128_q64_kernel(const P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const k_ring = smem;
  char* const v_ring = smem + 4 * TILE;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int nbh = p.batch * p.heads;
  int bh, qb;
  bool ordered = false;
  if constexpr (RANGES) ordered = p.order != nullptr;
  if (ordered) {
    // the launch order is data the host computed (attn_window.balanced_order): one wave-uniform load.  Defensive read: whatever
    // the table holds, the workgroup runs a unit of this launch or none
    const int bid = blockIdx.x;
    if (bid >= p.order_len) return;
    const int u = __builtin_amdgcn_readfirstlane(p.order[bid]);
    if (u < 0 || u >= nbh * p.q_blocks) return;
    bh = u / p.q_blocks;
    qb = u - bh * p.q_blocks;
  } else {
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int slot = idx / p.q_blocks;
    qb = idx - slot * p.q_blocks;
    bh = slot * 8 + xcd;
    if (bh >= nbh) return;
  }
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int Sq = p.Sq;
  const bool tap = p.clk != nullptr && (blockIdx.x & 63) == 0 && (int)(blockIdx.x >> 6) < p.clk_slots && wave == 0;   // clock tap: see attention.hip
  uint64_t tap_c0 = 0, tap_r0 = 0;
  if (tap) {
    tap_c0 = __builtin_readcyclecounter();
    tap_r0 = wall_clock64();
  }
  const bf16_t* Q = p.q + (int64_t)b * p.q_bs + h * 128;
  const bf16_t* const K0 = p.k + (int64_t)b * p.k_bs + h * 128;
  const bf16_t* const VT0 = p.vt + (int64_t)b * p.vt_bs + (int64_t)h * 128 * p.vt_rs;
  // the segment in hand: its first key's K row / V^T column, its length, and what follows from the length.  Everything below that
  // says Skv, T, ragged or tend means the SEGMENT's (RANGES = false: the panel's, set once)
  const bf16_t* K = K0;
  const bf16_t* VT = VT0;
  int Skv = p.Skv;
  int seg_begin = 0;   // the segment's first key: what the V^T rows have left behind a column is counted from the row's start
  int T = (Skv + KVB - 1) / KVB;
  bool ragged = (Skv & (KVB - 1)) != 0;
  const float c = p.scale_log2;
  // O^T of the wave's two query halves: tile (qh, dt) = oa[4 qh + dt], lane (q = l31, h2) register e <-> d = 32 dt + (e & 3) + 8 (e >> 2) + 4 h2
  f32x16 oa[8];
#pragma unroll
  for (int i = 0; i < 128; ++i) oa[i >> 4][i & 15] = 0.0f;
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};

  // everything lane-derived is rebuilt from a freshly laundered lane id by each phase (in front of, inside the operand set-up of,
  // and behind the statement): none of it is live across the statement, whose literal registers leave the compiler v[0:51]
  struct LaneCtx {
    int l31, h2, tid, k_row, k_slot, v_row, v_slot, q_row, k_row_off, k_sw, v_row_off, v_sw;
  };
  auto make_ctx = [&](int lane) -> LaneCtx {
    LaneCtx x;
    x.l31 = lane & 31, x.h2 = lane >> 5, x.tid = wave * 64 + lane;
    x.k_row = x.tid >> 4, x.k_slot = (x.tid & 15) ^ ((x.tid >> 4) & 15);      // + 16 rows per DMA piece
    x.v_row = x.tid >> 3, x.v_slot = (x.tid & 7) ^ ((x.tid >> 4) & 7);        // + 32 d-rows per DMA piece
    x.q_row = qb * (NW * QW) + wave * QW + x.l31;                              // query of half 0; half 1: + 32
    x.k_row_off = x.l31 * 256, x.k_sw = x.l31 & 15;
    x.v_row_off = x.l31 * 128, x.v_sw = (x.l31 >> 1) & 7;
    return x;
  };
  auto fresh_lane = [&]() -> int {
    int z = 0;
    asm volatile("" : "+s"(z));
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
  };
  auto stage_k = [&](const LaneCtx& x, int t) {
    const int kv0 = min(t, T - 1) * KVB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16_t* ks = K + (int64_t)min(kv0 + x.k_row + 16 * i, Skv - 1) * p.k_rs + x.k_slot * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)ks, (lptr_t)(k_ring + (t & 3) * TILE + (i * 4 + wave) * 1024), 16, 0, 0);
    }
  };
  auto stage_v = [&](const LaneCtx& x, int t) {
    const int kv0 = min(t, T - 1) * KVB;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(VT + (int64_t)(x.v_row + 32 * i) * p.vt_rs + x.v_slot * 8 + kv0),
                                       (lptr_t)(v_ring + (t & 3) * TILE + (i * 4 + wave) * 1024), 16, 0, 0);
  };
  // ONE tile in the straight form: protocol (unless done), S = K Q^T for both query halves, lazy softmax with the exact path in
  // line, O += V^T P^T.  Builtin MFMAs on C++ values: hipcc sees every hazard.  Runs tile 0, the tail and refused tiles only.
  auto straight_tile = [&](const LaneCtx& x, int t, bool top_done) {
    if (!top_done) {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // all but the previous iteration's eight DMAs
      __syncthreads();
      stage_k(x, t + 3);   // (past the end: clamped sources; the DMA count per iteration must not depend on t)
      stage_v(x, t + 2);
    }
    const char* Ks = k_ring + (t & 3) * TILE + x.k_row_off;
    const char* Vs = v_ring + (t & 3) * TILE + x.v_row_off;
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      bf16x8 qf[8];
      const bf16_t* qp = Q + (int64_t)min(x.q_row + 32 * qh, Sq - 1) * p.q_rs + x.h2 * 8;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
      f32x16 s[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) s[sub][e] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const bf16x8 kf = *(const bf16x8*)(Ks + sub * 8192 + (((2 * ks + x.h2) ^ x.k_sw) * 16));
          s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[sub], 0, 0, 0);
        }
      if (ragged && t == T - 1) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int kv = t * KVB + sub * 32 + (e & 3) + 8 * (e >> 2) + 4 * x.h2;
            if (kv >= Skv) s[sub][e] = -INFINITY;
          }
      }
      bf16x8 pf[4];
      auto probs = [&](float mc) -> float {
        float psum = 0.0f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float p0 = __builtin_amdgcn_exp2f(s[sub][8 * g + 2 * j] * c - mc);
              const float p1 = __builtin_amdgcn_exp2f(s[sub][8 * g + 2 * j + 1] * c - mc);
              pk.u[j] = pack_bf2(p0, p1);
              psum += p0 + p1;       // fp32 sums of the unrounded probabilities, as inside the statement
            }
            pf[sub * 2 + g] = pk.v;
          }
        return psum;
      };
      float psum = probs(m_run[qh] * c);
      if (__any(!(psum < ALG_LAZY_SUM_LIMIT))) {  // 2^80; also inf / NaN (tile 0: m = -inf)
        float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, s[0][e]), s[1][e]);
        {
          const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
          mt = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
        }
        const float m_new = fmaxf(m_run[qh], mt);
        const float alpha = __builtin_amdgcn_exp2f((m_run[qh] - m_new) * c);
        m_run[qh] = m_new;
        l_run[qh] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oa[4 * qh + dt] *= alpha;
        psum = probs(m_run[qh] * c);
      }
      l_run[qh] += psum;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 vf = *(const bf16x8*)(Vs + dt * 4096 + (((2 * kk + x.h2) ^ x.v_sw) * 16));
          oa[4 * qh + dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[kk], oa[4 * qh + dt], 0, 0, 0);
        }
    }
  };

  bool visited = !RANGES;   // a segment has run: the ring holds its tiles and its clamped prefetches may still be in flight
  // PREFIX: what the epilogue writes as lse, from the state behind segment `seg` (once per query: both h2 lanes hold l_tot and
  // the same m_run); -inf while no key has been visited.  Called at the top of the NEXT segment's iteration
  auto snapshot = [&](int seg) {
    const LaneCtx x = make_ctx(fresh_lane());
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      const float l_tot = l_run[qh] + __shfl_xor(l_run[qh], 32, 64);
      const int q_row = x.q_row + 32 * qh;
      if (q_row < Sq && x.h2 == 0)
        p.lse_prefix[((int64_t)bh * p.max_ranges + seg) * Sq + q_row] =
            visited ? m_run[qh] * c + __builtin_amdgcn_logf(l_tot) : -INFINITY;
    }
  };
  for (int seg = 0; seg < (RANGES ? p.max_ranges : 1); ++seg) {
  if constexpr (PREFIX) {
    if (seg > 0) snapshot(seg - 1);   // ONE site: a skipped segment comes by here as well; the last one is the epilogue's
  }
  if constexpr (RANGES) {
    // defensive read: whatever the table holds, the segment lies inside the panel and starts on the dense kernel's tile grid
    // (the bit-2/3 column permutation and the 16-byte alignment of the V^T DMA hold for begin % 64 == 0 only)
    const int32_t* r = p.ranges + ((int64_t)(h * p.head_rows + qb) * p.max_ranges + seg) * 2;   // (h, head_rows: wave-uniform)
    const int begin = __builtin_amdgcn_readfirstlane(min(max(r[0], 0), p.Skv)) & ~(KVB - 1);
    const int end = __builtin_amdgcn_readfirstlane(min(max(r[1], 0), p.Skv));
    if (end <= begin) continue;
    if (visited) {
      // hand-over of the ring: this wave's DMAs of the previous segment have landed, and no wave still reads its last tiles
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    visited = true;
    K = K0 + (int64_t)begin * p.k_rs;
    VT = VT0 + begin;
    Skv = end - begin;
    seg_begin = begin;
    T = (Skv + KVB - 1) / KVB;
    ragged = (Skv & (KVB - 1)) != 0;
  }
  // the statement runs iterations t < tend: QK(t + 1) must not touch the masked (ragged) last tile.  Its DMA of K(t + 3) / V^T(t + 2)
  // reaches past the end in the last iterations: the buffer descriptors' num_records end the panel, such pieces fetch nothing
  const int tend = ragged ? T - 2 : T - 1;
  int t = 1;
  bool top_done = false;
  {
    const LaneCtx x = make_ctx(fresh_lane());
    stage_k(x, 0);
    stage_k(x, 1);
    stage_v(x, 0);
    stage_v(x, 0);       // (filler: eight DMAs per batch)
    stage_k(x, 2);       // the batch "iteration -1" would have issued: K(2), V(1)
    stage_v(x, 1);
    straight_tile(x, 0, false);     // tile 0: establishes the running max of both query halves
  }
  for (;;) {
    if (p.use_statement && (t & 3) == 1 && t < tend && __all(m_run[0] > -3.0e38f && m_run[1] > -3.0e38f)) {
      const LaneCtx x = make_ctx(fresh_lane());
      auto sreg = [](int v) -> int { return __builtin_amdgcn_readfirstlane(v); };
      auto uniform64 = [](const void* ptr) -> uint64_t {
        const uint64_t v = (uint64_t)(uintptr_t)ptr;
        return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
      };
      const uint32_t kl = (uint32_t)(uintptr_t)(lptr_t)k_ring, vl = (uint32_t)(uintptr_t)(lptr_t)v_ring;
      int lk[8], lv[4];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) lk[ks] = kl + x.k_row_off + (((2 * ks + x.h2) ^ x.k_sw) * 16);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) lv[kk] = vl + x.v_row_off + (((2 * kk + x.h2) ^ x.v_sw) * 16);
      // DMA: the lane's byte offset inside a tile (constant) against raw buffer descriptors whose base is the tile the statement
      // fetches first -- K(t + 3), V^T(t + 2) -- and whose num_records is what is left of this (batch, head) panel from there
      // (0 once the tile lies past the end: the statement prefetches past the last tile it computes, and such pieces fetch nothing)
      int kvo[4], vvo[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        kvo[i] = (int)(((int64_t)(x.k_row + 16 * i) * p.k_rs + x.k_slot * 8) * 2);
        vvo[i] = (int)(((int64_t)(x.v_row + 32 * i) * p.vt_rs + x.v_slot * 8) * 2);
      }
      const int64_t k_tile_bytes = (int64_t)KVB * p.k_rs * 2;
      const int64_t k_left = ((int64_t)(Skv - 1) * p.k_rs + 128) * 2 - (int64_t)(t + 3) * k_tile_bytes;
      const int64_t v_left = (int64_t)128 * p.vt_rs * 2 - ((int64_t)seg_begin + (int64_t)(t + 2) * KVB) * 2;
      const uint64_t kt = uniform64((const char*)K + (int64_t)(t + 3) * k_tile_bytes);
      const uint64_t vtb = uniform64((const char*)VT + (int64_t)(t + 2) * KVB * 2);
      const int kd0 = sreg((int)(uint32_t)kt), kd1 = sreg((int)(uint32_t)(kt >> 32) & 0xffff), kd2 = sreg((int)(uint32_t)(k_left > 0 ? k_left : 0));
      const int vd0 = sreg((int)(uint32_t)vtb), vd1 = sreg((int)(uint32_t)(vtb >> 32) & 0xffff), vd2 = sreg((int)(uint32_t)(v_left > 0 ? v_left : 0));
      const int d3 = sreg(0x00020000);
      const int qvo0 = (int)(((int64_t)min(x.q_row, Sq - 1) * p.q_rs + x.h2 * 8) * 2);
      const int qvo1 = (int)(((int64_t)min(x.q_row + 32, Sq - 1) * p.q_rs + x.h2 * 8) * 2);
      const uint64_t qbs = uniform64(Q);
      const int kstep = sreg((int)k_tile_bytes), tend_s = sreg(tend);
      const int wk = sreg((int)kl + wave * 1024), wv = sreg((int)vl + wave * 1024);
      const float c_s = __builtin_bit_cast(float, sreg(__builtin_bit_cast(int, c)));
      const float negmc0 = -m_run[0] * c, negmc1 = -m_run[1] * c;
      int ts = sreg(t), code;
      asm volatile(ALG_ATTN128_Q64_LOOP_ASM
                   : ALG_ATTN128_Q64_O_OPERANDS(oa), [l0] "+v"(l_run[0]), [l1] "+v"(l_run[1]), [t] "+s"(ts), [code] "=&s"(code)
                   : [lk0] "v"(lk[0]), [lk1] "v"(lk[1]), [lk2] "v"(lk[2]), [lk3] "v"(lk[3]), [lk4] "v"(lk[4]), [lk5] "v"(lk[5]),
                     [lk6] "v"(lk[6]), [lk7] "v"(lk[7]), [lv0] "v"(lv[0]), [lv1] "v"(lv[1]), [lv2] "v"(lv[2]), [lv3] "v"(lv[3]),
                     [kvo0] "v"(kvo[0]), [kvo1] "v"(kvo[1]), [kvo2] "v"(kvo[2]), [kvo3] "v"(kvo[3]), [vvo0] "v"(vvo[0]),
                     [vvo1] "v"(vvo[1]), [vvo2] "v"(vvo[2]), [vvo3] "v"(vvo[3]),
                     [qvo0] "v"(qvo0), [qvo1] "v"(qvo1), [negmc0] "v"(negmc0), [negmc1] "v"(negmc1), [c] "s"(c_s),
                     [kd0] "s"(kd0), [kd1] "s"(kd1), [kd2] "s"(kd2), [kd3] "s"(d3), [vd0] "s"(vd0), [vd1] "s"(vd1), [vd2] "s"(vd2),
                     [vd3] "s"(d3), [qb] "s"(qbs), [kstep] "s"(kstep), [tend] "s"(tend_s), [wk] "s"(wk), [wv] "s"(wv)
                   : "memory", "vcc", "scc", ALG_ATTN128_Q64_CLOBBERS);
      t = ts;
      top_done = code != 0;   // 1: iteration t's protocol is done, softmax(t) is not: tile t is redone below
    }
    if (t >= T) break;
    const LaneCtx x = make_ctx(fresh_lane());
    straight_tile(x, t, top_done);   // a tile behind the statement, or one it refused (then back into it at the next t = 1 mod 4)
    top_done = false;
    ++t;
  }
  }   // segments

  const LaneCtx x = make_ctx(fresh_lane());
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    const float l_tot = l_run[qh] + __shfl_xor(l_run[qh], 32, 64);
    const float inv = visited ? 1.0f / l_tot : 0.0f;   // (a block the table leaves without a key writes zeros)
    const int q_row = x.q_row + 32 * qh;
    if (q_row < Sq) {
      bf16_t* op = p.o + (int64_t)b * p.o_bs + (int64_t)q_row * p.o_rs + h * 128;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = dt * 32 + 8 * g + 4 * x.h2;
          uint2 v;
          v.x = pack_bf2(oa[4 * qh + dt][4 * g] * inv, oa[4 * qh + dt][4 * g + 1] * inv);
          v.y = pack_bf2(oa[4 * qh + dt][4 * g + 2] * inv, oa[4 * qh + dt][4 * g + 3] * inv);
          *(uint2*)(op + d) = v;
        }
    }
    if constexpr (RANGES) {
      // sum over the visited keys of 2^(c s) = 2^(c m_run) l_tot: once per query (both h2 lanes hold l_tot and the same m_run)
      if (p.lse != nullptr && q_row < Sq && x.h2 == 0)
        p.lse[(int64_t)bh * Sq + q_row] = visited ? m_run[qh] * c + __builtin_amdgcn_logf(l_tot) : -INFINITY;
    }
    if constexpr (PREFIX) {   // the prefix behind the last segment: the lse above, to its place
      if (q_row < Sq && x.h2 == 0)
        p.lse_prefix[((int64_t)bh * p.max_ranges + p.max_ranges - 1) * Sq + q_row] =
            visited ? m_run[qh] * c + __builtin_amdgcn_logf(l_tot) : -INFINITY;
    }
  }
  if (tap && x.l31 == 0 && x.h2 == 0) {
    uint64_t* cp = p.clk + (size_t)(blockIdx.x >> 6) * 4;   // one workgroup owns a slot (block / 64 < slots)
    cp[0] = tap_c0, cp[1] = tap_r0, cp[2] = __builtin_readcyclecounter(), cp[3] = wall_clock64();
  }
}

}  // namespace a128q

// The launch step of the Q64 route, for the dense and the ranged instantiations: `entry` names the caller in the opt-in's
// message, `what` in the launch's.  The ranged parts of `a` are NULL / 0 from a dense call, whose instantiation reads none of them.
template <bool RANGES, bool PREFIX>
static int launch_q64(const char* entry, const char* what, const Attn128Args& a, const Attn128Plan& pl) {
  using namespace a128q;
  static_assert(NW * QW == ATTN128_Q64_ROWS && KVB == ATTN128_KVB, "the plan's tile sizes are the kernel's");
  static PerDeviceOnce attr_set;
  const int rc = opt_in_lds(attr_set, {(const void*)flash_attn_d128_q64_kernel<RANGES, PREFIX>}, LDS_BYTES, entry);
  if (rc != ALG_OK) return rc;
  P p;
  attn128_fill(p, a, pl.q_blocks);
  p.clk = clock_tap_for(a.stream, &p.clk_slots);
  p.use_statement = pl.use_statement;
  p.ranges = a.ranges;
  p.max_ranges = a.max_ranges;
  p.head_rows = a.table_heads == 1 ? 0 : p.q_blocks;
  p.lse = a.lse;
  p.order = a.order;
  p.order_len = a.order ? a.order_len : 0;
  p.lse_prefix = a.lse_prefix;
  hipLaunchKernelGGL((flash_attn_d128_q64_kernel<RANGES, PREFIX>), dim3((unsigned)pl.grid), dim3(NW * 64), LDS_BYTES, a.stream, p);
  return check_launch(what);
}

// (the three instantiations are named in the order the object has always held them -- dense, PREFIX, ranged: hipcc emits kernels
// as a file names them)
int launch_d128_q64(const Attn128Args& a, const Attn128Plan& pl) {
  return launch_q64<false, false>("alg_flash_attn_d128 (64-query kernel)", "alg_flash_attn_d128", a, pl);
}

}  // namespace alg

using namespace alg;

// Each block of 256 queries attends to its row of a table of key ranges (include/alg_hip.h).  This kernel is the only one that
// takes a table: attn128_plan routes a ranged call nowhere else, and of ALG_ATTN128_Q64 only the value 3 (statement off) is
// honoured here.
static int ranges_entry(const char* entry, Attn128Form form, const Attn128Args& a) {
  const int rc = attn128_check(a, entry, form);
  if (rc != ALG_OK) return rc;
  const Attn128Plan pl = attn128_plan(a);
  if (!pl.within_limits) {
    set_error("%s: operands beyond 31-bit byte offsets inside one (batch, head), or grid too large", entry);
    return ALG_ELIMIT;
  }
  return form == Attn128Form::PREFIX ? launch_q64<true, true>(entry, entry, a, pl) : launch_q64<true, false>(entry, entry, a, pl);
}

extern "C" int alg_flash_attn_d128_ranges(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq,
                                          int Skv, int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride,
                                          int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride,
                                          float scale, const int32_t* kv_ranges, int max_ranges, void* stream) {
  return ranges_entry("alg_flash_attn_d128_ranges", Attn128Form::RANGES,
                      {q, k, vt, o, batch, heads, Sq, Skv, q_bstride, q_rstride, k_bstride, k_rstride, vt_bstride, vt_rstride, o_bstride,
                       o_rstride, scale, 1, 0, (hipStream_t)stream, kv_ranges, max_ranges, 1, nullptr, nullptr, 0, nullptr});
}

// The same launch with a table row per (head, q block) when table_heads == heads, and the log-sum-exp output (include/alg_hip.h).
extern "C" int alg_flash_attn_d128_ranges_heads(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq,
                                                int Skv, int64_t q_bstride, int64_t q_rstride, int64_t k_bstride,
                                                int64_t k_rstride, int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride,
                                                int64_t o_rstride, float scale, const int32_t* kv_ranges, int max_ranges,
                                                int table_heads, float* lse, void* stream) {
  return ranges_entry("alg_flash_attn_d128_ranges_heads", Attn128Form::RANGES,
                      {q, k, vt, o, batch, heads, Sq, Skv, q_bstride, q_rstride, k_bstride, k_rstride, vt_bstride, vt_rstride, o_bstride,
                       o_rstride, scale, 1, 0, (hipStream_t)stream, kv_ranges, max_ranges, table_heads, lse, nullptr, 0, nullptr});
}

// The same launch in the order a device table gives: workgroup b runs the unit order[b] (include/alg_hip.h).  Every workgroup
// computes what it computes in alg_flash_attn_d128_ranges_heads, so O and lse are that entry's bit for bit, for every order.
extern "C" int alg_flash_attn_d128_ranges_order(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq,
                                                int Skv, int64_t q_bstride, int64_t q_rstride, int64_t k_bstride,
                                                int64_t k_rstride, int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride,
                                                int64_t o_rstride, float scale, const int32_t* kv_ranges, int max_ranges,
                                                int table_heads, float* lse, const int32_t* order, int order_len, void* stream) {
  return ranges_entry("alg_flash_attn_d128_ranges_order", Attn128Form::RANGES_ORDER,
                      {q, k, vt, o, batch, heads, Sq, Skv, q_bstride, q_rstride, k_bstride, k_rstride, vt_bstride, vt_rstride, o_bstride,
                       o_rstride, scale, 1, 0, (hipStream_t)stream, kv_ranges, max_ranges, table_heads, lse, order, order_len, nullptr});
}

// The same launch over a table of up to 12 segments, with the log-sum-exp of the keys visited so far written behind every segment
// (include/alg_hip.h).  The last prefix is what alg_flash_attn_d128_ranges_heads writes as lse for the same table, bit for bit.
extern "C" int alg_flash_attn_d128_ranges_prefix(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq,
                                                 int Skv, int64_t q_bstride, int64_t q_rstride, int64_t k_bstride,
                                                 int64_t k_rstride, int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride,
                                                 int64_t o_rstride, float scale, const int32_t* kv_ranges, int max_segments,
                                                 int table_heads, float* lse_prefix, void* stream) {
  return ranges_entry("alg_flash_attn_d128_ranges_prefix", Attn128Form::PREFIX,
                      {q, k, vt, o, batch, heads, Sq, Skv, q_bstride, q_rstride, k_bstride, k_rstride, vt_bstride, vt_rstride, o_bstride,
                       o_rstride, scale, 1, 0, (hipStream_t)stream, kv_ranges, max_segments, table_heads, nullptr, nullptr, 0,
                       lse_prefix});
}

namespace alg {
namespace a128q {

// Recall of a window (alg_attn_lse_recall): per panel the mean over the rows [row0, row0 + rows) of 2^(lse_part - lse_full), the
// fraction of a query's softmax mass that lies on the keys `lse_part` was taken over.  One workgroup per panel, two levels, both
// in a fixed order and in double: each lane sums its rows (stride 4 x 1024), then the lanes are summed (as vae.hip: gn_final).
constexpr int RECALL_THREADS = 1024;

__device__ inline float recall_term(float part, float full) {
  return part == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(part - full);
}

__global__ __launch_bounds__(RECALL_THREADS) void lse_recall_kernel(const float* __restrict__ part, const float* __restrict__ full,
                                                                    double* __restrict__ out, int Sq, int row0, int rows) {
  __shared__ double red[RECALL_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * Sq + row0;
  part += base, full += base;
  double acc = 0.0;
  // float4 where the panel's first row is 16-byte aligned in both buffers (workgroup-uniform); scalars otherwise and for the tail
  const bool vec = (((uintptr_t)part | (uintptr_t)full) & 15) == 0;
  const int rows4 = vec ? rows & ~3 : 0;
  for (int i = (int)threadIdx.x * 4; i < rows4; i += RECALL_THREADS * 4) {
    const float4 a = *(const float4*)(part + i), b = *(const float4*)(full + i);
    acc += ((double)recall_term(a.x, b.x) + (double)recall_term(a.y, b.y)) +
           ((double)recall_term(a.z, b.z) + (double)recall_term(a.w, b.w));
  }
  for (int i = rows4 + (int)threadIdx.x; i < rows; i += RECALL_THREADS) acc += (double)recall_term(part[i], full[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < RECALL_THREADS / 64; ++w) tot += red[w];
    out[blockIdx.x] = tot / (double)rows;
  }
}

// Softmax mass per segment (alg_attn_prefix_mass): workgroup (panel, i) forms the mean over the rows [row0, row0 + rows) of
// 2^(P_i - P_last) - 2^(P_(i-1) - P_last) from the prefixes [panels][segments][Sq] of alg_flash_attn_d128_ranges_prefix.  The
// exponentials are taken in double (the masses of a row add up to exactly 2^0 minus what cancels, and a sum of them over the
// segments of a width is compared against one); the reduction is lse_recall_kernel's: per lane in row order, then the lanes.
__device__ inline double prefix_term(float pre, float last) {
  return pre == -INFINITY ? 0.0 : exp2((double)pre - (double)last);
}

__global__ __launch_bounds__(RECALL_THREADS) void prefix_mass_kernel(const float* __restrict__ prefix, double* __restrict__ out,
                                                                     int segments, int Sq, int row0, int rows) {
  __shared__ double red[RECALL_THREADS / 64];
  const int panel = blockIdx.x / segments, i = blockIdx.x - panel * segments;
  const float* const last = prefix + ((int64_t)panel * segments + segments - 1) * Sq + row0;
  const float* const cur = prefix + ((int64_t)panel * segments + i) * Sq + row0;
  const float* const prev = i > 0 ? cur - Sq : nullptr;    // P_(-1) = -inf
  double acc = 0.0;
  for (int r = (int)threadIdx.x; r < rows; r += RECALL_THREADS) {
    const float l = last[r];
    acc += prefix_term(cur[r], l) - (prev ? prefix_term(prev[r], l) : 0.0);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < RECALL_THREADS / 64; ++w) tot += red[w];
    out[blockIdx.x] = tot / (double)rows;
  }
}

}  // namespace a128q
}  // namespace alg

extern "C" int alg_attn_prefix_mass(const float* lse_prefix, double* out, int panels, int segments, int Sq, int row0, int rows,
                                    void* stream) {
  if (!lse_prefix || !out || ((uintptr_t)lse_prefix & 3) || ((uintptr_t)out & 7)) {
    set_error("alg_attn_prefix_mass: lse_prefix must be a 4-byte and out an 8-byte aligned device pointer");
    return ALG_EINVAL;
  }
  if (panels <= 0 || segments < 1 || segments > 12 || Sq <= 0 || row0 < 0 || rows <= 0 || (int64_t)row0 + rows > Sq ||
      (int64_t)panels * segments > 0x7fffffff) {
    set_error("alg_attn_prefix_mass: bad argument (panels=%d segments=%d Sq=%d row0=%d rows=%d: segments in 1..12, the rows "
              "inside [0, Sq))", panels, segments, Sq, row0, rows);
    return ALG_EINVAL;
  }
  hipLaunchKernelGGL(a128q::prefix_mass_kernel, dim3((unsigned)(panels * segments)), dim3(a128q::RECALL_THREADS), 0,
                     (hipStream_t)stream, lse_prefix, out, segments, Sq, row0, rows);
  return check_launch("alg_attn_prefix_mass");
}

extern "C" int alg_attn_lse_recall(const float* lse_part, const float* lse_full, double* out, int panels, int Sq, int row0,
                                   int rows, void* stream) {
  if (!lse_part || !lse_full || !out || ((uintptr_t)lse_part & 3) || ((uintptr_t)lse_full & 3) || ((uintptr_t)out & 7)) {
    set_error("alg_attn_lse_recall: lse_part / lse_full must be 4-byte and out 8-byte aligned device pointers");
    return ALG_EINVAL;
  }
  if (panels <= 0 || Sq <= 0 || row0 < 0 || rows <= 0 || (int64_t)row0 + rows > Sq) {
    set_error("alg_attn_lse_recall: bad argument (panels=%d Sq=%d row0=%d rows=%d: the rows must lie inside [0, Sq))", panels, Sq,
              row0, rows);
    return ALG_EINVAL;
  }
  hipLaunchKernelGGL(a128q::lse_recall_kernel, dim3((unsigned)panels), dim3(a128q::RECALL_THREADS), 0, (hipStream_t)stream,
                     lse_part, lse_full, out, Sq, row0, rows);
  return check_launch("alg_attn_lse_recall");
}
