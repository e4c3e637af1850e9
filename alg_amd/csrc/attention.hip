// Flash attention forward (full softmax, no mask), head_dim 64, bf16 in/out, fp32 accumulate, for the
// joint [text; video] sequence of the video DiT (17,776 tokens at the north-star config).
//
// Wave-level formulation (64-wide waves, v_mfma_f32_32x32x16_bf16):
//   S^T = K Q^T   : A = K tile rows (kv), B = Q^T.  In the 32x32 C layout a lane then owns ONE query column
//                   (q = lane & 31) and 16 kv rows per sub-tile, so the softmax running max / sum / rescale
//                   are per-lane scalars; the two half-waves own complementary kv rows and exchange only the
//                   tile max (one cross-lane op per KV tile).
//   O^T = V^T P^T : A = V^T (rows = d), B = P^T taken straight from the S^T accumulators (exp -> bf16 pack),
//                   no LDS round trip for P.  The contraction index order of B is whatever the C layout hands
//                   out (kv = 16g + 8(j>>2) + 4h + (j&3)); V^T is stored by its producer GEMM with index bits
//                   2 and 3 swapped so one ds_read_b128 yields the matching A fragment.
// Workgroup = 8 waves x 32 queries = 256 queries of one (batch, head); KV tiles of 64 stream through an LDS
// ring with 16-byte global_load_lds; the bank swizzle sits on the source address (same scheme as gemm.hip).
// Workgroups are ordered so that one XCD works on one head at a time (K/V of a head = 4.5 MB, re-read by the
// 70 query blocks of that head out of the XCD's L2).
//
// Ten kernels are built from this file:
//   flash_attn_d64_kernel<SM>               the straight loop (QK^T -> softmax -> PV per tile), SM = one of three softmax forms:
//       Softmax::EXACT      exact running max; the O / l rescale is skipped (exactly: alpha == 1) when no lane's max grew;
//                           fp32 row sums of the unrounded probabilities.  ALG_ATTN_VARIANT=1: the reference of the parity tests
//       Softmax::LAZY       (DEFAULT, ALG_ATTN_VARIANT=33) lazy running max (softmax_tile_lazy): no tile max in the common path,
//                           the exact max / rescale path runs only when a row sum leaves [0, 2^80); row sums by
//                           v_dot2c_f32_bf16 from the packed P pairs (the bf16-rounded probabilities the PV MFMA uses)
//       Softmax::PRESCALED  the form behind alg_flash_attn_d64_ex(ALG_ATTN_Q_PRESCALED): Q was scaled by scale * log2(e) where it
//                           was produced (alg_qk_norm_rope_scaled: no extra rounding), the offset is snapped to zero when the
//                           first tile's max allows it, p = exp2(s) with no per-score fma (softmax_tile_zero); ALG_ATTN_PP=0
//   flash_attn_d64_kernel<LAZY | PRESCALED, SPLIT>   the same loops over one KV chunk of a split-KV tail unit (plan_tail)
//   flash_attn_d64_merge_kernel             merges the chunk results of the tail
//   flash_attn_d64_pipe_kernel<OFF, false>  PRESCALED with the steady-state loop as one generated asm statement: OFF = false
//                                           (DEFAULT, ALG_ATTN_PP=4) for waves whose offsets are zero, OFF = true (ALG_ATTN_PP=8)
//                                           for any offset.  (ALG_ATTN_PP=7 is attention64_m16.hip.)
//   flash_attn_d64_pipe_kernel<OFF, true>   the same two frames over the key ranges of a table, one range after the other
//                                           (alg_flash_attn_d64_ranges: the opt-in frame window, off by default)
//   flash_attn_d64_pipe_kernel<OFF, true, true>  ... that also write the log-sum-exp of the visited keys from an exact row sum
//                                           (alg_flash_attn_d64_ranges_heads with an lse pointer: the calibration forward)
//                                           Every RANGES = true instantiation also takes an optional launch-order table
//                                           (alg_flash_attn_d64_ranges_order): workgroup b runs the unit order[b]
//
// Measured and removed (the sources are in the history, the records in profiles/r1_*, profiles/r3_attention_d64_pingpong.txt,
// profiles/r3_attention_pipe_bench_ab.txt and docs/lab_notebook_r*.md).  MI355X, C2 shape (2 x 48 heads x 17,776 tokens),
// TFLOP/s: straight loop without the rescale skip 875; QK^T of tile t+1 under the softmax of tile t, K one tile ahead through a
// 3-slot ring 830; "lean" softmax 867 / 861; 4-wave workgroups 836; 64 queries per wave 804 / 599 (8 / 4 waves); two KV tiles
// per barrier 899 / 893 (with s_setprio); 16-wave workgroups 860; peeled ragged tile + packed fma / row sums 880; explicitly
// staged fragments 865; "duo" (two 32-query streams per wave) 835 / 875, with the lazy softmax 995 / 1044 -- against 860-915
// for EXACT and 990-1027 for LAZY on the same boxes.  Dot2 row sums alone: 925 -> 945; Q pre-scaled in registers: +2 % at one
// more bf16 rounding of q.  Ping-pong of the two waves of a SIMD over workgroup barriers (ALG_ATTN_PP=1/2, bit-identical to
// PRESCALED): 1097 / 1096 against 1103-1111 at the same clock and power -- the phase order across waves is not what limits
// the kernel.  The 4-wave form of the asm statement (ALG_ATTN_PP=3): 1114-1130 against 1164-1170 for the 8-wave one (half the
// L2 -> LDS traffic per MFMA).  Ablations of the straight loop (ms per 2-sample launch): full 8.75 | no DMA 7.62 | no LDS reads 6.76 | neither 6.10
// | no barrier 8.62 | no exp2 7.95 | no DMA/LDS/exp2 5.30 (MFMA floor at the sustained clock ~3.9).
// All of them sat at 1225-1330 W with the clock pulled down to 1.9-2.2 GHz (profiles/r1_power_and_issue_rates.txt): the kernel
// is bound by energy per FLOP under the package power cap, so variants that only remove stalls or issue slots gain clock, not
// time.
#include <stdlib.h>

#include "common.h"
#include "attn_pipe_loop.inc"
#include "attn_pipe_off_loop.inc"

namespace alg {

constexpr int ATT_THREADS = 512;
constexpr int QB = 256;   // queries per workgroup
constexpr int KVB = 64;   // kv rows per tile
constexpr int ATT_TILE = KVB * 64 * 2;     // 8 KiB (K tile; V^T tile is the same size)

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

struct AttnP {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* vt;
  bf16_t* o;
  int batch, heads, S, q_blocks;
  int64_t q_bs, q_rs, vt_bs, vt_rs, o_bs, o_rs;
  float scale_log2;  // scale * log2(e)
  // split-KV tail (see alg_flash_attn_d64): the last `tail_units` (head, q block) units of every XCD are cut into
  // `tail_split` KV chunks of `tail_tiles` KV tiles each; chunk results go to a workspace and are merged by a second kernel
  int unit0, tail_units, tail_split, tail_tiles;
  float* ws_o;   // [8 * tail_units][tail_split][q rows per block][64] fp32, unnormalised
  float* ws_ml;  // [8 * tail_units][tail_split][q rows per block][2]: running max (raw score units), row sum
  int prio;      // 1: the younger half of an 8-wave workgroup (waves 4-7) runs at s_setprio 1 (ALG_ATTN_PRIO, A/B knob)
  uint64_t* clk;   // clock tap (calibrate.hip: alg_attn_clock_tap) or NULL: {cycles, wall} at start / end of every 64th workgroup
  int clk_slots;
  uint64_t* path;  // path counters (calibrate.hip: alg_attn_path_tap) or NULL: {statement entries, tiles inside, tiles straight}
  // flash_attn_d64_pipe_kernel<OFF, RANGES = true> only (alg_flash_attn_d64_ranges, alg_flash_attn_d64_ranges_heads); the dense
  // instantiations read none of them
  const int32_t* ranges;   // device table [q_blocks][max_ranges][2] of (begin, end) key indices, or [heads][q_blocks][max_ranges][2]
  int max_ranges;
  int use_statement;       // 0: every tile through the C++ tile body (ALG_ATTN_PP=0: the frame on its own)
  int head_rows;           // q_blocks when the table has a leading head dimension ([heads][q_blocks][max_ranges][2]), else 0
  float* lse;              // fp32 [batch][heads][S]: log2-domain log-sum-exp of the (pre-scaled) scores over the visited keys, or NULL
  // alg_flash_attn_d64_ranges_order only (NULL and 0 from every other entry)
  const int32_t* order;    // device int32 [order_len]: the unit bh * q_blocks + qb workgroup b runs (negative: it exits), or NULL
  int order_len;           // = the grid
};

struct Frag {
  int row_off;  // l31 * 128
  int sw;       // (l31 >> 1) & 7
  int h2;
};

// S^T sub-tiles of one 64-row K tile: s[sub] = K[sub] Q^T
__device__ __forceinline__ void qk_tile(const char* Ks, const bf16x8 (&qf)[4], const Frag f, f32x16 (&s)[2]) {
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
    for (int e = 0; e < 16; ++e) s[sub][e] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 kf = *(const bf16x8*)(Ks + f.row_off + sub * 4096 + (((2 * ks + f.h2) ^ f.sw) * 16));
      s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[sub], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ void mask_tail(f32x16 (&s)[2], int kv0, int S, int h2) {
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kv = kv0 + sub * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2;
      if (kv >= S) s[sub][e] = -INFINITY;
    }
}

template <bool B>
struct BoolC { static constexpr bool value = B; };

// online softmax of one tile's scores -> bf16 P fragments; updates m, l and rescales O when needed (Softmax::EXACT): exact
// running max, the rescale skipped when no lane's max grew, fp32 row sums
__device__ __forceinline__ void softmax_tile(const f32x16 (&s)[2], float c, float& m_run, float& l_run,
                                             f32x16 (&o_acc)[2], bf16x8 (&pf)[4]) {
  float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
  for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, s[0][e]), s[1][e]);
  mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
  const bool grow = mt > m_run;
  if (__any(grow)) {
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o_acc[dt][e] *= alpha;
  }
  const float mc = m_run * c;
  float psum = 0.0f;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = s[sub][8 * g + 2 * j] * c - mc, x1 = s[sub][8 * g + 2 * j + 1] * c - mc;
        const float p0 = __builtin_amdgcn_exp2f(x0), p1 = __builtin_amdgcn_exp2f(x1);
        pk.u[j] = pack_bf2(p0, p1);
        psum += p0 + p1;  // the row sum uses the unrounded fp32 probabilities (as the math SDPA path does)
      }
      pf[sub * 2 + g] = pk.v;
    }
  l_run += psum;
}

// Lazy running max (Softmax::LAZY).  Softmax is invariant to the subtracted offset, and fp32 / bf16 keep their relative
// precision at any magnitude, so the offset only has to keep exp2 inside the exponent range: the probabilities are formed
// against the CURRENT m (no tile max: 23 VALU instructions saved per tile) and the exact path -- tile max, grow m, rescale
// O and l, recompute -- runs only when a tile's row sum leaves [0, 2^80) (inf on the first tile, where m = -inf; NaN if
// a masked score meets m = -inf).  m is then always a max actually seen, so nothing that matters can underflow.  The row sum
// comes from v_dot2c_f32_bf16 on the packed P pairs (one instruction per two scores instead of two adds): it sums the
// bf16-rounded probabilities -- the values the PV MFMA actually uses.
__device__ __forceinline__ void softmax_tile_lazy(const f32x16 (&s)[2], float c, float& m_run, float& l_run,
                                                  f32x16 (&o_acc)[2], bf16x8 (&pf)[4]) {
  typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
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
          psum = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2v, pk.u[j]), __builtin_bit_cast(bf2v, 0x3f803f80u),
                                                 psum, false);
        }
        pf[sub * 2 + g] = pk.v;
      }
    return psum;
  };
  float psum = probs(m_run * c);
  if (__any(!(psum < ALG_LAZY_SUM_LIMIT))) {  // 2^80; also true for inf and NaN
    float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
    for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, s[0][e]), s[1][e]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o_acc[dt][e] *= alpha;
    psum = probs(m_run * c);
  }
  l_run += psum;
}

// Softmax::PRESCALED: Q is pre-scaled, so the scores arrive in log2 units and the only per-score VALU work left in the common path
// is exp2, the bf16 pack and the dot2 row sum: the offset is SNAPPED TO ZERO whenever the first tile's max lies in
// (-64, 64) (probabilities then span 2^-64 .. 2^64 at most before the lazy rescale threshold trips: harmless for fp32 /
// bf16), and p = exp2(s) needs no subtraction at all.  Rows whose scores are further out keep a non-zero offset and take
// the subtracting path; the exact max / rescale path is the lazy one of softmax_tile_lazy.
//
// EXACT (flash_attn_d64_pipe_kernel<OFF, true, LSE = true> only): *dl also accumulates (fp32 sum of the UNROUNDED probabilities) -
// (the dot2 sum of the bf16-rounded ones), rescaled with l_run: l_run + *dl is the row sum a log-sum-exp wants, while l_run, the
// probabilities and O -- everything the output is made of -- are computed exactly as without it.
template <bool EXACT = false>
__device__ __forceinline__ void softmax_tile_zero(const f32x16 (&s)[2], float& m_run, float& l_run, f32x16 (&o_acc)[2],
                                                  bf16x8 (&pf)[4], float* dl = nullptr) {
  typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
  float esum = 0.0f;   // EXACT: the unrounded sum of the last probs() pass
  auto probs = [&](auto sub_c, float m) -> float {
    constexpr bool SUB = decltype(sub_c)::value;
    float psum = 0.0f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x0 = s[sub][8 * g + 2 * j], x1 = s[sub][8 * g + 2 * j + 1];
          const float p0 = __builtin_amdgcn_exp2f(SUB ? x0 - m : x0);
          const float p1 = __builtin_amdgcn_exp2f(SUB ? x1 - m : x1);
          pk.u[j] = pack_bf2(p0, p1);
          psum = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2v, pk.u[j]), __builtin_bit_cast(bf2v, 0x3f803f80u),
                                                 psum, false);
          if constexpr (EXACT) esum += p0, esum += p1;
        }
        pf[sub * 2 + g] = pk.v;
      }
    return psum;
  };
  float psum;
  if (__all(m_run == 0.0f))
    psum = probs(BoolC<false>{}, 0.0f);
  else
    psum = probs(BoolC<true>{}, m_run);
  if (__any(!(psum < ALG_LAZY_SUM_LIMIT))) {  // 2^80; also inf (first tile: m = -inf) and NaN
    float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
    for (int e = 1; e < 16; ++e) mt = fmaxf(fmaxf(mt, s[0][e]), s[1][e]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    float m_new = fmaxf(m_run, mt);
    if (m_run == -INFINITY && fabsf(m_new) < 64.0f) m_new = 0.0f;  // first tile: snap the offset to zero when it is safe
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o_acc[dt][e] *= alpha;
    if constexpr (EXACT) *dl *= alpha, esum = 0.0f;   // (the first pass's sum may be inf / NaN: it is dropped like psum)
    psum = probs(BoolC<true>{}, m_run);
  }
  l_run += psum;
  if constexpr (EXACT) *dl += esum - psum;
}

// O^T += V^T P^T for one 64-row tile
__device__ __forceinline__ void pv_tile(const char* Vs, const bf16x8 (&pf)[4], const Frag f, f32x16 (&o_acc)[2]) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // kk = sub*2 + g : kv block [16 kk, 16 kk + 16)
      const bf16x8 vf = *(const bf16x8*)(Vs + f.row_off + dt * 4096 + (((2 * kk + f.h2) ^ f.sw) * 16));
      o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[kk], o_acc[dt], 0, 0, 0);
    }
}

// the three softmax forms (header comment): softmax_tile, softmax_tile_lazy, softmax_tile_zero
enum class Softmax { EXACT, LAZY, PRESCALED };

template <Softmax SM, bool SPLIT = false>
__global__ __launch_bounds__(ATT_THREADS, 4) void flash_attn_d64_kernel(const AttnP p) {
  static_assert(!SPLIT || SM != Softmax::EXACT, "the split-KV tail is built on the lazy forms");
  __shared__ __attribute__((aligned(16))) char smem[4 * ATT_TILE];   // two K slots, two V^T slots
  char* const k_ring = smem;
  char* const v_ring = smem + 2 * ATT_TILE;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h2 = lane >> 5;

  // ---- workgroup -> (batch*head, q block): XCD x walks heads x, x+8, ... ----
  const int nbh = p.batch * p.heads;
  int bh, qb;
  int part = 0, chunk = 0;  // SPLIT: workspace slot of this (unit, chunk)
  {
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    int idx = bid >> 3;
    if (SPLIT) {  // the tail launch: block j of an XCD = chunk j % split of tail unit j / split
      chunk = idx % p.tail_split;
      const int u = idx / p.tail_split;
      part = xcd * p.tail_units + u;
      idx = p.unit0 + u;
    }
    const int slot = idx / p.q_blocks;
    qb = idx - slot * p.q_blocks;
    bh = slot * 8 + xcd;
    if (bh >= nbh) return;
  }
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int S = p.S;
  const bf16_t* Q = p.q + (int64_t)b * p.q_bs + h * 64;
  const bf16_t* K = p.k + (int64_t)b * p.q_bs + h * 64;
  const bf16_t* VT = p.vt + (int64_t)b * p.vt_bs + (int64_t)h * 64 * p.vt_rs;

  // ---- Q^T fragments (B operand): lane (q = l31, h2) holds Q[q][16 ks + 8 h2 .. +8] ----
  const int q_row = qb * QB + wave * 32 + l31;
  bf16x8 qf[4];
  {
    const bf16_t* qp = Q + (int64_t)min(q_row, S - 1) * p.q_rs + h2 * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }

  // ---- DMA sources: one 16-B piece of K and of V^T per thread per tile ----
  // per-lane base pointers for tile 0; a tile adds a wave-uniform byte offset (scalar multiply), and the row clamp
  // (rows >= S re-read row S-1, masked later) only exists on the last, ragged tile
  const int srow = tid >> 3;                        // K: kv row, V^T: d row
  const int sslot = (tid & 7) ^ ((tid >> 4) & 7);   // (row >> 1) & 7
  // (one-element arrays filled by a one-trip loop, the shape the code had when a workgroup could have four waves: as plain
  // scalars hipcc folds the address arithmetic earlier and schedules the prologue of three of the kernels differently)
  const bf16_t* k_src[1];
  const bf16_t* v_src[1];
#pragma unroll
  for (int i = 0; i < 1; ++i) {
    k_src[i] = K + (int64_t)min(srow, S - 1) * p.q_rs + sslot * 8;
    v_src[i] = VT + (int64_t)srow * p.vt_rs + sslot * 8;
  }
  const int64_t k_tile_stride = (int64_t)KVB * p.q_rs;
  const int last_tile = (S + KVB - 1) / KVB - 1;
  const bool ragged_src = (S & (KVB - 1)) != 0;
  auto stage_k = [&](int slot, int kv0) {
    const int t = kv0 / KVB;
    const bf16_t* ks = k_src[0] + t * k_tile_stride;
    if (ragged_src && t == last_tile) ks = K + (int64_t)min(kv0 + srow, S - 1) * p.q_rs + sslot * 8;
    __builtin_amdgcn_global_load_lds((gptr_t)ks, (lptr_t)(k_ring + slot * ATT_TILE + wave * 1024), 16, 0, 0);
  };
  auto stage_v = [&](int slot, int kv0) {
    __builtin_amdgcn_global_load_lds((gptr_t)(v_src[0] + kv0), (lptr_t)(v_ring + slot * ATT_TILE + wave * 1024), 16, 0, 0);
  };

  Frag f;
  f.row_off = l31 * 128;
  f.sw = (l31 >> 1) & 7;
  f.h2 = h2;

  f32x16 o_acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o_acc[i][e] = 0.0f;
  float m_run = -INFINITY;   // running max of raw scores (this lane's query)
  float l_run = 0.0f;        // this half-wave's share of the running sum
  const float c = p.scale_log2;
  const int n_tiles = (S + KVB - 1) / KVB;
  const bool ragged = (S & (KVB - 1)) != 0;
  // static priority for the second-dispatched half (guide T5, static form): it loses VALU arbitration to the older half on
  // every segment otherwise; one s_setprio, no per-cluster flips (the condition is provably wave-uniform: readfirstlane)
  if (p.prio && wave >= 4) __builtin_amdgcn_s_setprio(1);

  // SPLIT: this workgroup owns KV tiles [t0, t1) of its unit only
  const int t0 = SPLIT ? min(chunk * p.tail_tiles, n_tiles) : 0;
  const int t1 = SPLIT ? min(t0 + p.tail_tiles, n_tiles) : n_tiles;
  if (!SPLIT || t0 < t1) {
    stage_k(t0 & 1, t0 * KVB);
    stage_v(t0 & 1, t0 * KVB);
  }
  for (int t = t0; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < t1) {
      stage_k((t + 1) & 1, (t + 1) * KVB);
      stage_v((t + 1) & 1, (t + 1) * KVB);
    }
    f32x16 s[2];
    qk_tile(k_ring + (t & 1) * ATT_TILE, qf, f, s);
    if (ragged && t == n_tiles - 1) mask_tail(s, t * KVB, S, h2);
    bf16x8 pf[4];
    if (SM == Softmax::PRESCALED)
      softmax_tile_zero(s, m_run, l_run, o_acc, pf);
    else if (SM == Softmax::LAZY)
      softmax_tile_lazy(s, c, m_run, l_run, o_acc, pf);
    else
      softmax_tile(s, c, m_run, l_run, o_acc, pf);
    pv_tile(v_ring + (t & 1) * ATT_TILE, pf, f, o_acc);
  }

  // ---- finish: combine the half-waves' sums, normalise, store O[q][d] ----
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (SPLIT) {  // partial result of this KV chunk: unnormalised O, running max, row sum
    const int64_t row = ((int64_t)part * p.tail_split + chunk) * QB + wave * 32 + l31;
    float* wo = p.ws_o + row * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(float4*)(wo + dt * 32 + 8 * g + 4 * h2) =
            make_float4(o_acc[dt][4 * g], o_acc[dt][4 * g + 1], o_acc[dt][4 * g + 2], o_acc[dt][4 * g + 3]);
    if (h2 == 0) *(float2*)(p.ws_ml + row * 2) = make_float2(m_run, l_tot);
    return;
  }
  const float inv = 1.0f / l_tot;
  if (q_row < S) {
    bf16_t* op = p.o + (int64_t)b * p.o_bs + (int64_t)q_row * p.o_rs + h * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = dt * 32 + 8 * g + 4 * h2;
        uint2 v;
        v.x = pack_bf2(o_acc[dt][4 * g] * inv, o_acc[dt][4 * g + 1] * inv);
        v.y = pack_bf2(o_acc[dt][4 * g + 2] * inv, o_acc[dt][4 * g + 3] * inv);
        *(uint2*)(op + d) = v;
      }
  }
}

// Merge of the split-KV tail: O = sum_c 2^((m_c - M) c) O_c / sum_c 2^((m_c - M) c) l_c.  One thread = 4 output values.
__global__ __launch_bounds__(256) void flash_attn_d64_merge_kernel(const AttnP p) {
  constexpr int QBR = 256;  // query rows per unit (8 waves x 32)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)8 * p.tail_units * QBR * 16;
  if (e >= total) return;
  const int d4 = (int)(e & 15);
  const int row = (int)((e >> 4) % QBR);
  const int part = (int)(e / (16 * QBR));
  const int xcd = part / p.tail_units, u = part - xcd * p.tail_units;
  const int idx = p.unit0 + u;
  const int slot = idx / p.q_blocks, qb = idx - slot * p.q_blocks;
  const int bh = slot * 8 + xcd;
  const int q_row = qb * QBR + row;
  if (bh >= p.batch * p.heads || q_row >= p.S) return;
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int64_t base = (int64_t)part * p.tail_split * QBR + row;
  float M = -INFINITY;
  for (int c = 0; c < p.tail_split; ++c) M = fmaxf(M, p.ws_ml[(base + (int64_t)c * QBR) * 2]);
  float L = 0.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < p.tail_split; ++c) {
    const int64_t r = base + (int64_t)c * QBR;
    const float2 ml = *(const float2*)(p.ws_ml + r * 2);
    if (ml.y == 0.0f) continue;  // empty chunk
    const float w = __builtin_amdgcn_exp2f((ml.x - M) * p.scale_log2);
    const float4 o = *(const float4*)(p.ws_o + r * 64 + d4 * 4);
    L += w * ml.y;
    acc.x += w * o.x, acc.y += w * o.y, acc.z += w * o.z, acc.w += w * o.w;
  }
  const float inv = 1.0f / L;
  uint2 v;
  v.x = pack_bf2(acc.x * inv, acc.y * inv);
  v.y = pack_bf2(acc.z * inv, acc.w * inv);
  *(uint2*)(p.o + (int64_t)b * p.o_bs + (int64_t)q_row * p.o_rs + h * 64 + d4 * 4) = v;
}

// ---------------------------------------------------------------------------------------------------------------
// Pipelined form (ALG_ATTN_PP=4, the default main launch of the pre-scaled call): the steady-state KV loop is ONE generated asm statement (attn_pipe_loop.inc,
// scripts/gen_attn_pipe.py) in which every MFMA is followed, in program order of the SAME wave, by the softmax work of one
// score pair and one fragment read -- the only arrangement in which matrix and vector work overlap on this part
// (profiles/r3_attention_d64_mix_microbench.txt).  This kernel is the frame around it: the same workgroup -> (head, q block)
// map, Q / K / V^T layouts and finish as flash_attn_d64_kernel<PRESCALED>, a C++ loop that runs tile 0 (where the running offset is
// established and snapped to zero), the last few tiles (ragged tail) and any tile on which the statement bails out (row sum
// outside [0, 2^80): the exact max / rescale path), all under the statement's collective protocol:
//     top of iteration t:  s_waitcnt vmcnt(2); s_barrier; DMA K(t+3) -> K slot (t+3) & 3, V^T(t+2) -> V slot (t+2) & 3
// so that the waves of a workgroup may be inside or outside the statement independently.  The straight form of an iteration
// reads K(t), V^T(t); the pipelined form K(t+1), V^T(t-1): four-slot rings keep all of them resident.
// Row sums are plain fp32 adds of the unrounded probabilities inside the statement (v_dot2c does not hide behind an MFMA),
// the bf16-rounded dot2 sums of softmax_tile_zero outside it.
// ---------------------------------------------------------------------------------------------------------------
//
// OFF (ALG_ATTN_PP=8): the offset form of the statement (attn_pipe_off_loop.inc).  The scores leave the matrix pipe as
// s - m -- the wave hands in -m of each lane's query and the statement makes it srcC of the first QK k-step -- so a wave enters
// whatever its rows' offsets are (the first-tile snap to zero stays: rows that snap under 4 still do), and after a refused tile
// (code 1: the exact path in C++, which may move m) it runs the straight form up to the next t = 1 (mod 4) with t + 4 <= tend
// and enters again with the new offset.  One loop, one copy of the straight body and of the statement.
//
// One 256-query unit per 8-wave workgroup, as in flash_attn_d64_kernel.  hipcc grants such a workgroup 128 + 128 registers per
// lane: the statement lives in v[26:127] (OFF: v[10:127]) and a[0:79] and takes O in AccVGPR operands.
//
// RANGES (alg_flash_attn_d64_ranges, the opt-in frame-window attention of alg_amd/attn_window.py; as in attention128_q64.hip):
// false = every key of the panel, ONE segment [0, S) known when the kernel starts -- the dense kernel, the segment loop folds away.
// true = the workgroup's 256 queries attend to the key ranges of their row of p.ranges, one after the other.  A segment
// [begin, end) is a panel of its own: K and V^T advanced to its first key, the six priming DMAs, tile 0 in C++, the statement
// under the frame's own entry rule, the tail in C++ -- with O, the running offset and the row sum carried from segment to segment
// and nothing else.  softmax_tile_zero treats a finite offset on a segment's tile 0 like any later tile (it snaps only while the
// offset is -inf), and the statements only run iterations whose K(t + 3) is a whole tile of the SEGMENT, so with the frame's
// clamps no DMA leaves [begin, round_up(end, 64)): inside the V^T pitch attn64_check demands.  Between segments the ring is
// handed over by s_waitcnt vmcnt(0) + one workgroup barrier; inside a segment the DMA count per iteration stays constant (the
// counted vmcnt(2) wait relies on it).  Everything a segment adds is wave-uniform and lives in SGPRs: nothing new is live across
// the statement in vector registers (LaneCtx below).
//
// LSE (RANGES only; alg_flash_attn_d64_ranges_heads with an lse pointer -- the host picks the instantiation): the epilogue also
// writes the log2-domain log-sum-exp of the visited keys, m_run + log2(row sum).  The frame's own row sum l_run is a sum of
// bf16-ROUNDED probabilities wherever the C++ tile body ran (each off by up to 2^-8), so these instantiations carry one more
// per-lane value, dl = (exact fp32 sum) - (rounded sum) over those tiles (softmax_tile_zero<EXACT>; the statements add unrounded
// probabilities themselves and never rescale, so dl passes them unchanged), and take log2(l + dl).  O is bit for bit what the
// LSE = false instantiation writes; the four LSE = false instantiations have no trace of any of this.
template <bool OFF, bool RANGES, bool LSE = false>
__global__ __launch_bounds__(ATT_THREADS) void flash_attn_d64_pipe_kernel(const AttnP p) {
  static_assert(RANGES || !LSE, "the LSE output exists on the ranged instantiations only");
  __shared__ __attribute__((aligned(16))) char smem[8 * ATT_TILE];
  char* const k_ring = smem;
  char* const v_ring = smem + 4 * ATT_TILE;
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
    const int xcd = bid & 7;
    const int idx = bid >> 3;
    const int slot = idx / p.q_blocks;
    qb = idx - slot * p.q_blocks;
    bh = slot * 8 + xcd;
    if (bh >= nbh) return;
  }
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int Sq = p.S;   // the panel's rows: what the query clamp and the store mean by S
  const bf16_t* Q = p.q + (int64_t)b * p.q_bs + h * 64;
  // the segment in hand: its first key's K row / V^T column, its length, and what follows from the length.  Everything below
  // that says K, VT, S, T or ragged means the SEGMENT's (RANGES = false: the panel's, set once)
  const bf16_t* K = p.k + (int64_t)b * p.q_bs + h * 64;
  const bf16_t* VT = p.vt + (int64_t)b * p.vt_bs + (int64_t)h * 64 * p.vt_rs;
  int S = p.S;
  int T = (S + KVB - 1) / KVB;
  bool ragged = (S & (KVB - 1)) != 0;
  // clock tap (bench.py: the shader clock THIS kernel ran at): scalar reads of two counters, wave 0 of every 64th workgroup
  const bool tap = p.clk != nullptr && (blockIdx.x & 63) == 0 && (int)(blockIdx.x >> 6) < p.clk_slots && wave == 0;
  uint64_t tap_c0 = 0, tap_r0 = 0;
  if (tap) {
    tap_c0 = __builtin_readcyclecounter();
    tap_r0 = wall_clock64();
  }
  f32x16 oa[2];
#pragma unroll
  for (int i = 0; i < 32; ++i) oa[i >> 4][i & 15] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;
  float dl = 0.0f;   // LSE only

  // Everything lane-derived is rebuilt from a lane id (LaneCtx): the C++ loops in front of and behind the statement each build
  // their own from a freshly laundered id, so that none of it is live across the statement (values that are compete with its
  // 32 O operands for v[0:63], and hipcc then parks them in AccVGPRs beyond a79: 328 registers, one wave per SIMD)
  struct LaneCtx {
    int lane, l31, h2, tid, srow, sslot, q_row;
    Frag f;
  };
  auto make_ctx = [&](int lane) -> LaneCtx {
    LaneCtx c;
    c.lane = lane, c.l31 = lane & 31, c.h2 = lane >> 5, c.tid = wave * 64 + lane;
    c.srow = c.tid >> 3, c.sslot = (c.tid & 7) ^ ((c.tid >> 4) & 7);
    c.q_row = qb * QB + wave * 32 + c.l31;
    c.f.row_off = c.l31 * 128, c.f.sw = (c.l31 >> 1) & 7, c.f.h2 = c.h2;
    return c;
  };
  auto fresh_lane = [&]() -> int {
    int z = 0;
    asm volatile("" : "+s"(z));
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
  };
  // (one-trip loops, the shape the staging had when a workgroup could have four waves: without them hipcc folds the address
  // arithmetic earlier and schedules the DMA issue of both kernels differently)
  auto stage_k = [&](const LaneCtx& c, int t) {
#pragma unroll
    for (int i = 0; i < 1; ++i) {
      const bf16_t* ks = K + (int64_t)min(t * KVB + c.srow, S - 1) * p.q_rs + c.sslot * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)ks, (lptr_t)(k_ring + (t & 3) * ATT_TILE + wave * 1024), 16, 0, 0);
    }
  };
  auto stage_v = [&](const LaneCtx& c, int t) {
#pragma unroll
    for (int i = 0; i < 1; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(VT + (int64_t)c.srow * p.vt_rs + c.sslot * 8 + min(t, T - 1) * KVB),
                                       (lptr_t)(v_ring + (t & 3) * ATT_TILE + wave * 1024), 16, 0, 0);
  };
  // iterations [t, t_end) in the straight form: protocol (unless the first one's is already done), QK(t) -> softmax -> PV(t)
  auto straight = [&](const LaneCtx& c, int t, int t_end, bool top_done) {
    bf16x8 qf[4];
    const bf16_t* qp = Q + (int64_t)min(c.q_row, Sq - 1) * p.q_rs + c.h2 * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
    for (; t < t_end; ++t) {
      if (!top_done) {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // all but the previous iteration's DMAs (two per wave)
        __syncthreads();
        stage_k(c, t + 3);   // past the end the source rows are clamped (K) / lie in the padded pitch (V^T): the DMA count per
        stage_v(c, t + 2);   // iteration must not depend on t, the counted wait above relies on it
      }
      top_done = false;
      f32x16 s[2];
      qk_tile(k_ring + (t & 3) * ATT_TILE, qf, c.f, s);
      if (ragged && t == T - 1) mask_tail(s, t * KVB, S, c.h2);
      bf16x8 pf[4];
      if constexpr (LSE) softmax_tile_zero<true>(s, m_run, l_run, oa, pf, &dl);
      else softmax_tile_zero(s, m_run, l_run, oa, pf);
      pv_tile(v_ring + (t & 3) * ATT_TILE, pf, c.f, oa);
    }
  };

  int n_ent = 0, n_in = 0;   // path counters: statement entries, tiles run inside the statement
  int n_tiles = 0;           // ... and the tiles of the segments run
  bool visited = !RANGES;    // a segment has run: the ring holds its tiles and its clamped prefetches may still be in flight
  LaneCtx c;                 // the context of the last C++ loop, which the finish shares
  // (a do-while: its condition is a constant for RANGES = false, and the dense kernels are compiled as if there were no loop)
  int seg = 0;
  do {
  if constexpr (RANGES) {
    // defensive read: whatever the table holds, the segment lies inside the panel and starts on the dense kernel's tile grid
    // (the bit-2/3 column permutation and the 16-byte alignment of the V^T DMA hold for begin % 64 == 0 only)
    const int32_t* r = p.ranges + ((int64_t)(h * p.head_rows + qb) * p.max_ranges + seg) * 2;   // (h, head_rows: wave-uniform)
    const int begin = __builtin_amdgcn_readfirstlane(min(max(r[0], 0), Sq)) & ~(KVB - 1);
    const int end = __builtin_amdgcn_readfirstlane(min(max(r[1], 0), Sq));
    if (end <= begin) continue;
    if (visited) {
      // hand-over of the ring: this wave's DMAs of the previous segment have landed, and no wave still reads its last tiles
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    visited = true;
    K = p.k + (int64_t)b * p.q_bs + h * 64 + (int64_t)begin * p.q_rs;
    VT = p.vt + (int64_t)b * p.vt_bs + (int64_t)h * 64 * p.vt_rs + begin;
    S = end - begin;
    T = (S + KVB - 1) / KVB;
    ragged = (S & (KVB - 1)) != 0;
  }
  n_tiles += T;
  // the statement only runs iterations t whose DMA target K(t + 3) is a whole tile (its sources are not clamped) and whose
  // tile t + 1 needs no mask
  const int tend = ragged ? T - 4 : T - 3;
  // wave-uniform operands of the statement travel in SGPRs.  (The per-lane address set-up in front of each statement is written
  // out in both branches below on purpose: computed by one shared lambda, hipcc allocates the frame around the statements
  // differently -- see LaneCtx above.)
  auto sreg = [](int v) -> int { return __builtin_amdgcn_readfirstlane(v); };
  auto uniform64 = [](const void* ptr) -> uint64_t {
    const uint64_t v = (uint64_t)(uintptr_t)ptr;
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  };
  int t = OFF ? 0 : 1;
  bool top_done = false;
  {
    const LaneCtx c = make_ctx(fresh_lane());
    stage_k(c, 0);
    stage_k(c, 1);
    stage_v(c, 0);
    stage_v(c, 0);       // (filler: four DMAs per batch)
    stage_k(c, 2);       // the batch "iteration -1" would have issued: K(2), V(1)
    stage_v(c, 1);
    if constexpr (!OFF) straight(c, 0, 1, false);     // tile 0: establishes the running offset (snapped to zero when its scores allow)
  }
  if constexpr (OFF) {
    for (;;) {
      // straight form up to the next entry point: the smallest ta = 1 (mod 4) behind the tile that has to be (re)done here -- tile 0
      // (establishes the offset, snapped to zero when its scores allow) or a tile the statement refused -- or to the end
      const int tt = top_done ? t + 1 : t;
      const int ta = tt + ((1 - tt) & 3);
      const bool enter = ta + 4 <= tend;
      {
        const LaneCtx c = make_ctx(fresh_lane());
        straight(c, t, enter ? ta : T, top_done);
      }
      if (!enter) break;
      t = ta;
      const LaneCtx c = make_ctx(fresh_lane());
      // (no V^T fragment addresses: the statement reads the V^T ring through lk + 4 * ATT_TILE -- v_ring = k_ring + 32 KiB above)
      const uint32_t kl = (uint32_t)(uintptr_t)(lptr_t)k_ring, vl = (uint32_t)(uintptr_t)(lptr_t)v_ring;
      const int lk0 = kl + c.f.row_off + (((0 + c.h2) ^ c.f.sw) * 16), lk1 = kl + c.f.row_off + (((2 + c.h2) ^ c.f.sw) * 16);
      const int lk2 = kl + c.f.row_off + (((4 + c.h2) ^ c.f.sw) * 16), lk3 = kl + c.f.row_off + (((6 + c.h2) ^ c.f.sw) * 16);
      int kvo0 = (int)(((int64_t)((t + 3) * KVB + c.srow) * p.q_rs + c.sslot * 8) * 2);
      int vvo0 = (int)(((int64_t)c.srow * p.vt_rs + c.sslot * 8 + (t + 2) * KVB) * 2);
      const int qvo = (int)(((int64_t)min(c.q_row, Sq - 1) * p.q_rs + c.h2 * 8) * 2);
      const uint64_t kb = uniform64(K), vb = uniform64(VT), qbs = uniform64(Q);
      const int kstep = sreg((int)(KVB * p.q_rs * 2)), tend_s = sreg(tend);
      const int wk = sreg((int)kl + wave * 1024), wv = sreg((int)vl + wave * 1024);
      int ts = sreg(t), code;
      float negm = 0.0f - m_run;   // (+0 for a snapped row: the first k-step then starts from what the zero-offset form starts from)
      float o[32];
#pragma unroll
      for (int i = 0; i < 32; ++i) o[i] = oa[i >> 4][i & 15];
      asm volatile(ALG_ATTN_PIPE8_OFF_LOOP_ASM
                   : ALG_ATTN_PIPE8_OFF_O_OPERANDS(o), [l] "+v"(l_run), [t] "+s"(ts), [code] "=&s"(code), [kvo0] "+v"(kvo0),
                     [vvo0] "+v"(vvo0), [negm] "+v"(negm)
                   : [lk0] "v"(lk0), [lk1] "v"(lk1), [lk2] "v"(lk2), [lk3] "v"(lk3), [qvo] "v"(qvo), [kb] "s"(kb), [vb] "s"(vb),
                     [qb] "s"(qbs), [kstep] "s"(kstep), [tend] "s"(tend_s), [wk] "s"(wk), [wv] "s"(wv)
                   : "memory", "vcc", "scc", ALG_ATTN_PIPE8_OFF_CLOBBERS);
#pragma unroll
      for (int i = 0; i < 32; ++i) oa[i >> 4][i & 15] = o[i];
      m_run = 0.0f - negm;   // (travels through the statement in its operand: nothing of the frame's is live across it)
      n_ent += 1, n_in += ts - t;
      t = ts;
      top_done = code != 0;   // 1: iteration t's protocol is done, softmax(t) is not: tile t is redone at the top of the loop
    }
  } else if ((!RANGES || p.use_statement) && 1 + 4 <= tend && __all(m_run == 0.0f)) {
    const LaneCtx c = make_ctx(fresh_lane());
    const uint32_t kl = (uint32_t)(uintptr_t)(lptr_t)k_ring, vl = (uint32_t)(uintptr_t)(lptr_t)v_ring;
    const int fl0 = c.f.row_off + (((0 + c.h2) ^ c.f.sw) * 16), fl1 = c.f.row_off + (((2 + c.h2) ^ c.f.sw) * 16);
    const int fl2 = c.f.row_off + (((4 + c.h2) ^ c.f.sw) * 16), fl3 = c.f.row_off + (((6 + c.h2) ^ c.f.sw) * 16);
    const int lk0 = kl + fl0, lk1 = kl + fl1, lk2 = kl + fl2, lk3 = kl + fl3;
    const int lv0 = vl + fl0, lv1 = vl + fl1, lv2 = vl + fl2, lv3 = vl + fl3;
    int kvo0 = (int)(((int64_t)((t + 3) * KVB + c.srow) * p.q_rs + c.sslot * 8) * 2);
    int vvo0 = (int)(((int64_t)c.srow * p.vt_rs + c.sslot * 8 + (t + 2) * KVB) * 2);
    const int qvo = (int)(((int64_t)min(c.q_row, Sq - 1) * p.q_rs + c.h2 * 8) * 2);
    const uint64_t kb = uniform64(K), vb = uniform64(VT), qbs = uniform64(Q);
    const int kstep = sreg((int)(KVB * p.q_rs * 2)), tend_s = sreg(tend);
    const int wk = sreg((int)kl + wave * 1024), wv = sreg((int)vl + wave * 1024);
    int ts = sreg(t), code;
    float o[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) o[i] = oa[i >> 4][i & 15];
    asm volatile(ALG_ATTN_PIPE8_LOOP_ASM
                 : ALG_ATTN_PIPE8_O_OPERANDS(o), [l] "+v"(l_run), [t] "+s"(ts), [code] "=&s"(code), [kvo0] "+v"(kvo0),
                   [vvo0] "+v"(vvo0)
                 : [lk0] "v"(lk0), [lk1] "v"(lk1), [lk2] "v"(lk2), [lk3] "v"(lk3), [lv0] "v"(lv0), [lv1] "v"(lv1),
                   [lv2] "v"(lv2), [lv3] "v"(lv3), [qvo] "v"(qvo), [kb] "s"(kb), [vb] "s"(vb), [qb] "s"(qbs),
                   [kstep] "s"(kstep), [tend] "s"(tend_s), [wk] "s"(wk), [wv] "s"(wv)
                 : "memory", "vcc", "scc", ALG_ATTN_PIPE8_CLOBBERS);
#pragma unroll
    for (int i = 0; i < 32; ++i) oa[i >> 4][i & 15] = o[i];
    n_ent += 1, n_in += ts - t;
    t = ts;
    top_done = code != 0;   // 1: iteration t's protocol is done, softmax(t) is not: tile t is redone below
  }
  if constexpr (!OFF) {
    c = make_ctx(fresh_lane());
    straight(c, t, T, top_done);   // the tiles behind the statement (or all of them but tile 0)
  }
  } while (RANGES && ++seg < p.max_ranges);   // segments
  if constexpr (OFF || RANGES) c = make_ctx(fresh_lane());

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = !RANGES || visited ? 1.0f / l_tot : 0.0f;   // (a block the table leaves without a key writes zeros)
  if (c.q_row < Sq) {
    bf16_t* op = p.o + (int64_t)b * p.o_bs + (int64_t)c.q_row * p.o_rs + h * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = dt * 32 + 8 * g + 4 * c.h2;
        uint2 v;
        v.x = pack_bf2(oa[dt][4 * g] * inv, oa[dt][4 * g + 1] * inv);
        v.y = pack_bf2(oa[dt][4 * g + 2] * inv, oa[dt][4 * g + 3] * inv);
        *(uint2*)(op + d) = v;
      }
  }
  if constexpr (LSE) {
    // sum over the visited keys of 2^s = 2^m_run (l_tot + dl_tot) (Q is pre-scaled: the scores are in log2 units): once per query
    // -- both h2 lanes hold the sums, and the same m_run (softmax_tile_zero folds the tile max across the halves before it moves
    // the offset)
    const float dl_tot = dl + __shfl_xor(dl, 32, 64);
    if (p.lse != nullptr) {   // uniform
      if (c.q_row < Sq && c.h2 == 0)
        p.lse[(int64_t)bh * Sq + c.q_row] = visited ? m_run + __builtin_amdgcn_logf(l_tot + dl_tot) : -INFINITY;
    }
  }
  if (tap && c.lane == 0) {
    uint64_t* cp = p.clk + (size_t)(blockIdx.x >> 6) * 4;   // one workgroup owns a slot (block / 64 < slots)
    cp[0] = tap_c0, cp[1] = tap_r0, cp[2] = __builtin_readcyclecounter(), cp[3] = wall_clock64();
  }
  if (p.path != nullptr) {   // uniform
    if (c.lane == 0) {
      unsigned long long* pc = (unsigned long long*)p.path;
      atomicAdd(pc + 0, (unsigned long long)n_ent);
      atomicAdd(pc + 1, (unsigned long long)n_in);
      atomicAdd(pc + 2, (unsigned long long)(n_tiles - n_in));
    }
  }
}


// Workgroup-count quantisation (measured, scripts/attn_tail_probe.py): every XCD runs 64 workgroups at a time (32 CUs x
// 2), a workgroup takes ~0.64 ms at S = 17,776, and a 2-sample C2 launch is 840 units per XCD = 13.125 rounds: the
// fourteenth round keeps 8 of 64 slots busy and costs 1.5-5 % of the launch depending on the box.  When the last round is at most 1/4 full its units
// are cut along KV instead: tail_units x split chunk-workgroups fill the slots, then one small merge kernel.
struct TailPlan {
  int units, split, tiles;
};
static TailPlan plan_tail(int nbh, int q_blocks, int n_tiles) {
  TailPlan t = {0, 0, 0};
  if (!opt(OPT_ATTN_SPLIT_TAIL)) return t;  // ALG_ATTN_SPLIT_TAIL=0: single launch (parity tests: batch-shape bit-identity)
  if (nbh % 8) return t;  // heads spread unevenly over the XCDs: a different imbalance, not this one
  const int slots = 64;
  const int per_xcd = nbh / 8 * q_blocks;
  const int r = per_xcd % slots;
  if (per_xcd < slots || r == 0 || r > 16 || n_tiles < 64) return t;  // fuller last rounds gain little
  t.units = r;
  t.split = (r * 8) % slots == 0 ? 8 : 16;
  t.tiles = (n_tiles + t.split - 1) / t.split;
  return t;
}

// The launch plan of one call: pure, a function of the shape, the flags and the option table only.
// ALG_ATTN_VARIANT: 33 = the default (LAZY), 1 = the exact-running-max reference the parity tests compare it with (capi.hip
// accepts only {1, 33}); ALG_ATTN_Q_PRESCALED calls have one form.  The split-KV tail is built on the two lazy forms.
struct Attn64Plan {
  Softmax form;
  int q_blocks;      // 256-query units per (batch, head)
  TailPlan tail;     // units == 0: a single launch
  int64_t ws_bytes;  // workspace the tail needs: [8 * units][split][256 rows] x (64 O values + max + row sum) fp32
};
static Attn64Plan attn64_plan(int batch, int heads, int S, int flags) {
  Attn64Plan pl;
  pl.form = (flags & ALG_ATTN_Q_PRESCALED) ? Softmax::PRESCALED : opt(OPT_ATTN_VARIANT) == 1 ? Softmax::EXACT : Softmax::LAZY;
  pl.q_blocks = (S + QB - 1) / QB;
  pl.tail = TailPlan{0, 0, 0};
  if (pl.form != Softmax::EXACT) pl.tail = plan_tail(batch * heads, pl.q_blocks, (S + KVB - 1) / KVB);
  pl.ws_bytes = (int64_t)8 * pl.tail.units * pl.tail.split * QB * 66 * (int64_t)sizeof(float);
  return pl;
}

static int attn64_check(const void* q, const void* k, const void* vt, const void* o, int batch, int heads, int S, int64_t q_bs,
                        int64_t q_rs, int64_t vt_bs, int64_t vt_rs, int64_t o_bs, int64_t o_rs) {
  if (!q || !k || !vt || !o || batch <= 0 || heads <= 0 || S <= 0) {
    set_error("alg_flash_attn_d64: bad argument (batch=%d heads=%d S=%d)", batch, heads, S);
    return ALG_EINVAL;
  }
  if (q_rs % 8 || q_bs % 8 || vt_rs % 8 || vt_bs % 8 || o_rs % 4 || o_bs % 4 || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) ||
      ((uintptr_t)vt & 15) || ((uintptr_t)o & 7)) {
    set_error("alg_flash_attn_d64: q/k/vt need 16-byte aligned rows (strides %% 8 == 0), o 8-byte aligned");
    return ALG_EINVAL;
  }
  if (vt_rs < (int64_t)((S + KVB - 1) / KVB) * KVB) {
    set_error("alg_flash_attn_d64: vt row stride %lld must cover S rounded up to %d", (long long)vt_rs, KVB);
    return ALG_EINVAL;
  }
  return ALG_OK;
}

// attention64_m16.hip: the 8-wave statement kernel on v_mfma_f32_16x16x32_bf16 as the main launch (ALG_ATTN_PP=7); 1 = not covered
int flash_attn_d64_m16(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S, int q_blocks,
                       int64_t q_bs, int64_t q_rs, int64_t vt_bs, int64_t vt_rs, int64_t o_bs, int64_t o_rs, unsigned blocks,
                       hipStream_t stream);

// `blocks` workgroups of the straight loop in the plan's softmax form: over whole units, or (split) over the KV chunks of the
// tail units.  (The seven instantiations are named in this and the next function in the order the code object has always
// had them; hipcc emits kernels in the order a file names them, and their order moves the code of some of them.)
static void attn64_launch_straight(Softmax form, bool split, unsigned blocks, const AttnP& p, hipStream_t s);

// Main launch of `blocks` workgroups (the whole grid, or the units in front of the split-KV tail) in the plan's softmax form.
// ALG_OK: launched.  For PRESCALED, ALG_ATTN_PP picks the kernel: 4 (default) = the pipelined kernel (asm steady-state loop, every
// MFMA followed by one score pair of the softmax), 8 = the same statement for any running offset (waves return to it after a
// refused tile), 7 = attention64_m16.hip (the statement on 16x16x32 MFMAs; a call it declines -- fewer than 12 KV tiles, 31-bit
// offsets, V^T pitch -- runs 4), 0 = the straight loop (same softmax, fp32 summation order differs).
static int attn64_launch(Softmax form, unsigned blocks, const AttnP& p, hipStream_t s) {
  int pp = form == Softmax::PRESCALED ? opt(OPT_ATTN_PP) : 0;
  if (pp == 7) {
    const int rq = flash_attn_d64_m16(p.q, p.k, p.vt, p.o, p.batch, p.heads, p.S, p.q_blocks, p.q_bs, p.q_rs, p.vt_bs, p.vt_rs,
                                      p.o_bs, p.o_rs, blocks, s);
    if (rq != 1) return rq;
  }
  // the pipelined statements address K / V^T / Q with 31-bit byte offsets from the (batch, head) panel bases
  if (pp >= 3 && ((int64_t)(p.S + 4 * KVB) * p.q_rs * 2 >= (1ll << 31) || (int64_t)65 * p.vt_rs * 2 >= (1ll << 31))) pp = 0;
  switch (pp) {
    case 4:
    case 7: hipLaunchKernelGGL((flash_attn_d64_pipe_kernel<false, false>), dim3(blocks), dim3(ATT_THREADS), 0, s, p); break;
    case 8: hipLaunchKernelGGL((flash_attn_d64_pipe_kernel<true, false>), dim3(blocks), dim3(ATT_THREADS), 0, s, p); break;
    default: attn64_launch_straight(form, false, blocks, p, s); break;
  }
  return ALG_OK;
}

static void attn64_launch_straight(Softmax form, bool split, unsigned blocks, const AttnP& p, hipStream_t s) {
  const dim3 g(blocks), blk(ATT_THREADS);
  switch (form) {
    case Softmax::PRESCALED:
      if (!split) hipLaunchKernelGGL(flash_attn_d64_kernel<Softmax::PRESCALED>, g, blk, 0, s, p);
      else hipLaunchKernelGGL((flash_attn_d64_kernel<Softmax::PRESCALED, true>), g, blk, 0, s, p);
      break;
    case Softmax::LAZY:
      if (!split) hipLaunchKernelGGL(flash_attn_d64_kernel<Softmax::LAZY>, g, blk, 0, s, p);
      else hipLaunchKernelGGL((flash_attn_d64_kernel<Softmax::LAZY, true>), g, blk, 0, s, p);
      break;
    case Softmax::EXACT:   // (attn64_plan puts no tail on it)
      hipLaunchKernelGGL(flash_attn_d64_kernel<Softmax::EXACT>, g, blk, 0, s, p);
      break;
  }
}

// The ranged launch (alg_flash_attn_d64_ranges): pre-scaled Q, one launch over whole units in the dense grid order.  ALG_ATTN_PP
// picks the frame: 4 and 7 the zero-offset statement, 8 the any-offset one; 0, or operands beyond the statements' 31-bit byte
// offsets (the rule of attn64_launch), the zero-offset frame with the statement switched off -- every tile through the C++ tile
// body.  (Named behind the seven dense instantiations: the code object keeps their order.)
static void attn64_launch_ranges(unsigned blocks, AttnP& p, hipStream_t s) {
  int pp = opt(OPT_ATTN_PP);
  if (pp >= 3 && ((int64_t)(p.S + 4 * KVB) * p.q_rs * 2 >= (1ll << 31) || (int64_t)65 * p.vt_rs * 2 >= (1ll << 31))) pp = 0;
  p.use_statement = pp >= 3;
  if (p.lse == nullptr) {
    if (pp == 8) hipLaunchKernelGGL((flash_attn_d64_pipe_kernel<true, true>), dim3(blocks), dim3(ATT_THREADS), 0, s, p);
    else hipLaunchKernelGGL((flash_attn_d64_pipe_kernel<false, true>), dim3(blocks), dim3(ATT_THREADS), 0, s, p);
  } else {   // the LSE output: the instantiations that also carry the exact row sum (named last: the others keep their order)
    if (pp == 8) hipLaunchKernelGGL((flash_attn_d64_pipe_kernel<true, true, true>), dim3(blocks), dim3(ATT_THREADS), 0, s, p);
    else hipLaunchKernelGGL((flash_attn_d64_pipe_kernel<false, true, true>), dim3(blocks), dim3(ATT_THREADS), 0, s, p);
  }
}

}  // namespace alg

using namespace alg;

extern "C" int alg_flash_attn_d64(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                  int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                  int64_t o_bstride, int64_t o_rstride, float scale, void* stream) {
  return alg_flash_attn_d64_ex(q, k, vt, o, batch, heads, S, q_bstride, q_rstride, vt_bstride, vt_rstride, o_bstride,
                               o_rstride, scale, 0, nullptr, 0, stream);
}

// Bytes of the split-KV workspace the launch plan of (batch, heads, S) uses (0: the plan is a single launch).  The library
// never allocates: the caller owns the buffer and passes it to alg_flash_attn_d64_ex.
extern "C" int64_t alg_flash_attn_d64_workspace_bytes(int batch, int heads, int S, int flags) {
  if (batch <= 0 || heads <= 0 || S <= 0) return 0;
  return attn64_plan(batch, heads, S, flags).ws_bytes;
}

extern "C" int alg_flash_attn_d64_ex(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                     int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                     int64_t o_bstride, int64_t o_rstride, float scale, int flags, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  const int rc = attn64_check(q, k, vt, o, batch, heads, S, q_bstride, q_rstride, vt_bstride, vt_rstride, o_bstride, o_rstride);
  if (rc != ALG_OK) return rc;
  const Attn64Plan pl = attn64_plan(batch, heads, S, flags);
  hipStream_t s = (hipStream_t)stream;
  AttnP p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.vt = (const bf16_t*)vt; p.o = (bf16_t*)o;
  p.batch = batch; p.heads = heads; p.S = S; p.q_blocks = pl.q_blocks;
  p.q_bs = q_bstride; p.q_rs = q_rstride; p.vt_bs = vt_bstride; p.vt_rs = vt_rstride;
  p.o_bs = o_bstride; p.o_rs = o_rstride;
  p.scale_log2 = (flags & ALG_ATTN_Q_PRESCALED) ? 1.0f : scale * 1.4426950408889634f;  // m is in log2 units already
  p.prio = 0;
  p.clk = clock_tap_for(s, &p.clk_slots);
  p.path = path_tap_for(s);
  p.unit0 = p.tail_units = p.tail_split = p.tail_tiles = 0;
  p.ws_o = p.ws_ml = nullptr;
  p.ranges = nullptr, p.max_ranges = 0, p.use_statement = 1, p.head_rows = 0, p.lse = nullptr;
  p.order = nullptr, p.order_len = 0;
  const int nbh = batch * heads;
  // the split-KV tail runs only in a caller-provided workspace (alg_flash_attn_d64_workspace_bytes); without one the whole
  // problem is a single launch (same rows up to fp32 summation order in the tail units)
  const TailPlan& tp = pl.tail;
  if (!tp.units || !workspace || ((uintptr_t)workspace & 15) || workspace_bytes < pl.ws_bytes) {
    const int r = attn64_launch(pl.form, (unsigned)((int64_t)((nbh + 7) / 8) * 8 * p.q_blocks), p, s);
    return r != ALG_OK ? r : check_launch("alg_flash_attn_d64");
  }
  p.unit0 = nbh / 8 * p.q_blocks - tp.units, p.tail_units = tp.units, p.tail_split = tp.split, p.tail_tiles = tp.tiles;
  const size_t rows = (size_t)8 * tp.units * tp.split * QB;
  p.ws_o = (float*)workspace, p.ws_ml = p.ws_o + rows * 64;
  const int r = attn64_launch(pl.form, (unsigned)(8 * p.unit0), p, s);
  if (r != ALG_OK) return r;
  attn64_launch_straight(pl.form, true, (unsigned)(8 * tp.units * tp.split), p, s);
  const int64_t merge = (int64_t)8 * tp.units * QB * 16;
  hipLaunchKernelGGL(flash_attn_d64_merge_kernel, dim3((unsigned)((merge + 255) / 256)), dim3(256), 0, s, p);
  return check_launch("alg_flash_attn_d64");
}

// Each block of 256 queries attends to its row of a table of key ranges (include/alg_hip.h): pre-scaled Q only (the
// ALG_ATTN_Q_PRESCALED form of alg_flash_attn_d64_ex), ONE launch -- no split-KV tail, no workspace.  Both entries run this:
// `what` names the caller in the error text.
static int ranges64_entry(const char* what, const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                          int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride,
                          int64_t o_rstride, const int32_t* kv_ranges, int max_ranges, int table_heads, float* lse,
                          const int32_t* order, int order_len, bool ordered, void* stream) {
  const int rc = attn64_check(q, k, vt, o, batch, heads, S, q_bstride, q_rstride, vt_bstride, vt_rstride, o_bstride, o_rstride);
  if (rc != ALG_OK) {
    set_error("%s: the operands fail the checks of alg_flash_attn_d64 (batch=%d heads=%d S=%d; q/k/vt "
              "16-byte aligned rows, o 8-byte aligned, vt row stride %lld covering S rounded up to %d)",
              what, batch, heads, S, (long long)vt_rstride, KVB);
    return rc;
  }
  if (!kv_ranges || ((uintptr_t)kv_ranges & 3) || max_ranges < 1 || max_ranges > 4) {
    set_error("%s: kv_ranges must be a 4-byte aligned device table and max_ranges in 1..4 (got %p, %d)", what,
              (const void*)kv_ranges, max_ranges);
    return ALG_EINVAL;
  }
  if (table_heads != 1 && table_heads != heads) {
    set_error("%s: table_heads must be 1 (one table for every head) or heads = %d, got %d", what, heads, table_heads);
    return ALG_EINVAL;
  }
  if ((uintptr_t)lse & 3) {
    set_error("%s: lse must be 4-byte aligned (got %p)", what, (const void*)lse);
    return ALG_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  AttnP p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.vt = (const bf16_t*)vt; p.o = (bf16_t*)o;
  p.batch = batch; p.heads = heads; p.S = S; p.q_blocks = (S + QB - 1) / QB;
  p.q_bs = q_bstride; p.q_rs = q_rstride; p.vt_bs = vt_bstride; p.vt_rs = vt_rstride;
  p.o_bs = o_bstride; p.o_rs = o_rstride;
  p.scale_log2 = 1.0f;
  p.prio = 0;
  p.clk = clock_tap_for(s, &p.clk_slots);
  p.path = path_tap_for(s);
  p.unit0 = p.tail_units = p.tail_split = p.tail_tiles = 0;
  p.ws_o = p.ws_ml = nullptr;
  p.ranges = kv_ranges, p.max_ranges = max_ranges;
  p.head_rows = table_heads == 1 ? 0 : p.q_blocks;
  p.lse = lse;
  p.order = nullptr, p.order_len = 0;
  int64_t grid = (int64_t)((batch * heads + 7) / 8) * 8 * p.q_blocks;
  if (grid > 0x7fffffff) {
    set_error("%s: grid too large (batch=%d heads=%d S=%d)", what, batch, heads, S);
    return ALG_EINVAL;
  }
  if (ordered) {   // alg_flash_attn_d64_ranges_order: the order table is the grid (the other entries pass NULL)
    const int64_t units = (int64_t)batch * heads * p.q_blocks;
    if (!order || ((uintptr_t)order & 3) || order_len <= 0 || order_len % 8 || (int64_t)order_len < units) {
      set_error("%s: order must be a 4-byte aligned device int32[order_len] with order_len a multiple of 8 and at least "
                "batch * heads * q_blocks = %lld (got %p, %d)", what, (long long)units, (const void*)order, order_len);
      return ALG_EINVAL;
    }
    p.order = order, p.order_len = order_len;
    grid = order_len;
  }
  attn64_launch_ranges((unsigned)grid, p, s);
  return check_launch(what);
}

extern "C" int alg_flash_attn_d64_ranges(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                         int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                         int64_t o_bstride, int64_t o_rstride, const int32_t* kv_ranges, int max_ranges,
                                         void* stream) {
  return ranges64_entry("alg_flash_attn_d64_ranges", q, k, vt, o, batch, heads, S, q_bstride, q_rstride, vt_bstride, vt_rstride,
                        o_bstride, o_rstride, kv_ranges, max_ranges, 1, nullptr, nullptr, 0, false, stream);
}

// The same launch with a table row per (head, q block) when table_heads == heads, and the log-sum-exp output (include/alg_hip.h).
extern "C" int alg_flash_attn_d64_ranges_heads(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                               int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                               int64_t o_bstride, int64_t o_rstride, const int32_t* kv_ranges, int max_ranges,
                                               int table_heads, float* lse, void* stream) {
  return ranges64_entry("alg_flash_attn_d64_ranges_heads", q, k, vt, o, batch, heads, S, q_bstride, q_rstride, vt_bstride,
                        vt_rstride, o_bstride, o_rstride, kv_ranges, max_ranges, table_heads, lse, nullptr, 0, false, stream);
}

// The same launch in the order a device table gives: workgroup b runs the unit order[b] (include/alg_hip.h).  Every workgroup
// computes what it computes in alg_flash_attn_d64_ranges_heads, so O and lse are that entry's bit for bit, for every order.
extern "C" int alg_flash_attn_d64_ranges_order(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                               int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                               int64_t o_bstride, int64_t o_rstride, const int32_t* kv_ranges, int max_ranges,
                                               int table_heads, float* lse, const int32_t* order, int order_len, void* stream) {
  return ranges64_entry("alg_flash_attn_d64_ranges_order", q, k, vt, o, batch, heads, S, q_bstride, q_rstride, vt_bstride,
                        vt_rstride, o_bstride, o_rstride, kv_ranges, max_ranges, table_heads, lse, order, order_len, true, stream);
}
