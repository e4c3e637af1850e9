// Flash attention forward, head_dim 128, OCP e4m3 operands on v_mfma_scale_f32_32x32x64_f8f6f4 (both formats e4m3, every E8M0
// block scale 2^0: a plain K = 64 fp8 contraction at twice the bf16 rate, as gemm_kernel.h issues it).  Opt-in: nothing calls
// this kernel unless the host asks for it; alg_flash_attn_d128 is untouched.
//
// Scope: non-causal, ungrouped, separate Sq / Skv, ragged last tile, strides and offsets as alg_flash_attn_d128, bf16 output.
//
// Formulation: S^T = K Q^T as in the bf16 kernels, so a lane owns ONE query (lane & 31) and half of a tile's keys (lane >> 5), and
// the softmax state is per lane.  With 64 queries per wave (attention128_q64.hip) a 64-key x 128 K tile costs two K = 64 MFMAs per
// 32-key sub-tile and query half (the bf16 kernel: eight K = 16), O^T += V^T P^T one MFMA per 32-row d-tile and query half (four).
//
// Scales.
//   * Q: one fp32 scale per (batch, token, head).  A lane owns one query, so the scale folds into the lane's scale_log2 factor.
//   * K: one fp32 scale per (batch, head).  It folds into the same factor: NO instruction in the loop.  Anything finer (per key
//     block, per token) is a v_mul_f32 per score -- 32 per lane, tile and query half -- in a loop whose VALU work (32 fma, 32 exp2,
//     32 adds, 16 conversions per tile and half) is already what the matrix pipe waits for.  e4m3 is a floating-point format, so a
//     coarse scale costs no relative precision for the normal range (2^-6 .. 448 of the head's amax / 448: fifteen binades); only
//     keys more than 2^15 below the largest |k| of their head lose bits.
//   * V^T: one fp32 scale per (batch, head, channel) row; it multiplies the accumulator rows in the epilogue.
//
// P in registers.  The accumulator of S^T holds, in lane (q, h2) register e of sub-tile sub, key 32 sub + 8 (e >> 2) + 4 h2 + (e & 3).
// Converted to e4m3 four at a time, a lane's 32 probabilities of a 64-key tile ARE its 32-byte B operand (byte 16 sub + e).  The A
// operand pairs byte j of lane (d, h2) with byte j of lane (q, h2), so V^T has to hold, at column 64 t + 32 h2 + 16 sub + e of row
// d, key 64 t + 32 sub + 8 (e >> 2) + 4 h2 + (e & 3): alg_quantize_fp8_vt writes that order (the role ALG_GEMM_PERMUTE_COLS plays
// for the bf16 kernels).  Padding columns up to the next multiple of 64 are zero (they meet p = 0: anything but the NaN byte does).
//
// Overflow.  The bf16 kernels' lazy running max lets a probability reach 2^80; e4m3 ends at 448 and v_cvt_pk_fp8_f32 must not be
// relied on to saturate.  Probabilities are formed as exp2(s c - m c + 3) -- a fixed P scale of 2^3 -- and the exact path (tile
// max, grow m, rescale O and l) runs whenever a LANE's sum over its 32 values of the tile is not <= 448 (also inf / NaN: tile 0).
// Every term is non-negative, so each converted value is <= 448 on the lazy path; on the exact path each is <= 2^3 and the lane sum
// is <= 256, so the trigger cannot fire twice for one tile.  2^3 is the largest power of two for which a flat tile (32 values at
// the maximum) does not trip the trigger again right after an exact step.  With it, probabilities down to 2^-9 of the running
// offset are normal e4m3 numbers, down to 2^-12 subnormal, and anything below 2^-13 contributes to l (fp32, unrounded) but
// not to O.  The scale cancels in O / l.
//
// Host side: the entry fills the operand struct of the bf16 entries (attention128_host.h) and reads top to bottom as they do --
// check (the shared predicates at the e4m3 row modulus, around this entry's own messages), plan (one kernel), launch.
#include <type_traits>

#include "attention128_host.h"
#include "row_ops.h"

namespace alg {
namespace a128f8 {

constexpr int NW = 4;
constexpr int QW = 64;                   // queries per wave
constexpr int KVB = 64;
constexpr int TILE = 8192;               // K tile (64 keys x 128 B) = V^T tile (128 rows x 64 B)
constexpr int LDS_BYTES = 8 * TILE;      // 4 K slots + 4 V^T slots
constexpr float P_SHIFT = 3.0f;          // log2 of the P scale
constexpr float P_LIMIT = 448.0f;        // e4m3 maximum

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef int i8v __attribute__((ext_vector_type(8)));
typedef int i4v __attribute__((ext_vector_type(4)));

struct P {
  const uint8_t* q;
  const uint8_t* k;
  const uint8_t* vt;
  const float* q_scale;
  const float* k_scale;
  const float* vt_scale;
  bf16_t* o;
  int batch, heads, Sq, Skv, q_blocks;
  int64_t q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs;
  float scale_log2;
};

__device__ __forceinline__ i8v cat(const i4v l, const i4v h) { return i8v{l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]}; }

__global__ __launch_bounds__(NW * 64) void flash_attn_d128_fp8_kernel(const P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const k_ring = smem;
  char* const v_ring = smem + 4 * TILE;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int nbh = p.batch * p.heads;
  int bh, qb;
  {
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int slot = idx / p.q_blocks;
    qb = idx - slot * p.q_blocks;
    bh = slot * 8 + xcd;
    if (bh >= nbh) return;
  }
  const int b = bh / p.heads, h = bh - b * p.heads;
  const int Sq = p.Sq, Skv = p.Skv;
  const uint8_t* Q = p.q + (int64_t)b * p.q_bs + h * 128;
  const uint8_t* K = p.k + (int64_t)b * p.k_bs + h * 128;
  const uint8_t* VT = p.vt + (int64_t)b * p.vt_bs + (int64_t)h * 128 * p.vt_rs;
  const int T = (Skv + KVB - 1) / KVB;
  const bool ragged = (Skv & (KVB - 1)) != 0;
  const int lane = threadIdx.x & 63, l31 = lane & 31, h2 = lane >> 5, tid = threadIdx.x;
  // DMA: 16 bytes per lane, 4 KiB per instruction of the workgroup, two instructions per tile.  Chunk ci = 256 i + tid of the tile
  // lands at byte 16 ci; the source is chosen so that row r keeps its logical 16-byte chunk c at slot c ^ swizzle(r).
  const int k_row = tid >> 3, k_chunk = (tid & 7) ^ ((tid >> 3) & 7);          // + 32 keys per piece
  const int v_row = tid >> 2, v_chunk = (tid & 3) ^ ((tid >> 3) & 3);          // + 64 d-rows per piece
  auto stage_k = [&](int t) {
    const int kv0 = min(t, T - 1) * KVB;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint8_t* ks = K + (int64_t)min(kv0 + k_row + 32 * i, Skv - 1) * p.k_rs + k_chunk * 16;
      __builtin_amdgcn_global_load_lds((gptr_t)ks, (lptr_t)(k_ring + (t & 3) * TILE + (i * 4 + wave) * 1024), 16, 0, 0);
    }
  };
  auto stage_v = [&](int t) {
    const int kv0 = min(t, T - 1) * KVB;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(VT + (int64_t)(v_row + 64 * i) * p.vt_rs + v_chunk * 16 + kv0),
                                       (lptr_t)(v_ring + (t & 3) * TILE + (i * 4 + wave) * 1024), 16, 0, 0);
  };
  stage_k(0);
  stage_k(1);
  stage_v(0);
  stage_v(0);       // (filler: four DMAs per batch)
  stage_k(2);       // the batch "iteration -1" would have issued: K(2), V(1)
  stage_v(1);

  // the lane's two queries: 128 e4m3 bytes each, bytes 64 kp + 32 h2 .. + 32 are the B operand of MFMA kp
  i8v qf[2][2];
  float c[2];
  const int q_row0 = qb * (NW * QW) + wave * QW + l31;
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    const int qr = min(q_row0 + 32 * qh, Sq - 1);
    const uint8_t* qp = Q + (int64_t)qr * p.q_rs + h2 * 32;
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) qf[qh][kp] = cat(*(const i4v*)(qp + kp * 64), *(const i4v*)(qp + kp * 64 + 16));
    c[qh] = p.scale_log2 * p.q_scale[((int64_t)b * Sq + qr) * p.heads + h] * p.k_scale[bh];
  }
  // O^T of the wave's two query halves: tile (qh, dt) = oa[4 qh + dt], lane (q = l31, h2) register e <-> d = 32 dt + (e & 3) + 8 (e >> 2) + 4 h2
  f32x16 oa[8];
#pragma unroll
  for (int i = 0; i < 128; ++i) oa[i >> 4][i & 15] = 0.0f;
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};
  const int k_off = l31 * 128, k_sw = l31 & 7;          // rows l31 and l31 + 32 share the swizzle
  const int v_off = l31 * 64, v_sw = (l31 >> 1) & 3;    // rows l31 + 32 dt likewise

  // One tile.  The two query halves are staggered by hand so that every batch of MFMAs has softmax VALU work of the OTHER half
  // next to it in the same basic block (an MFMA runs 16 passes in the background once issued; a wave issues in order, so overlap
  // needs VALU instructions BETWEEN the MFMAs -- the source order below is pinned with sched_barrier fences):
  //     QK(0) | QK(1) + probabilities(0) | [exact path 0] | PV(0) + probabilities(1) | [exact path 1] | PV(1)
  // LAST: the ragged last tile (keys >= Skv masked); a template argument so that the steady-state body has no branch for it.
  auto tile = [&](int t, auto last_tag) {
    constexpr bool LAST = decltype(last_tag)::value;
    // collective protocol of attention128_q64.hip: everything but the previous iteration's four DMAs has landed, every wave is
    // past its reads of the slots restaged now -- K slot (t + 3) & 3 was read in iteration t - 1, V^T slot (t + 2) & 3 in t - 2
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __syncthreads();
    stage_k(t + 3);   // (past the end: clamped sources; the DMA count per iteration must not depend on t)
    stage_v(t + 2);
    const char* Ks = k_ring + (t & 3) * TILE + k_off;
    const char* Vs = v_ring + (t & 3) * TILE + v_off;
    i8v kf[2][2], vf[4];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        const int c0 = 4 * kp + 2 * h2;
        kf[sub][kp] = cat(*(const i4v*)(Ks + sub * 4096 + ((c0 ^ k_sw) * 16)), *(const i4v*)(Ks + sub * 4096 + (((c0 + 1) ^ k_sw) * 16)));
      }
    f32x16 s[2][2];
    i8v pf[2];
    float psum[2];
    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // (an inline constant: no VALU)
    auto qk_mfma = [&](int qh, int i) {       // MFMA i of the four of S^T(qh): sub-tile i >> 1, d half i & 1
      const int sub = i >> 1;
      s[qh][sub] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[sub][i & 1], qf[qh][i & 1], (i & 1) ? s[qh][sub] : zero, 0, 0, 0,
                                                                   0x7f7f7f7f, 0, 0x7f7f7f7f);
    };
    auto pv_mfma = [&](int qh, int dt) {
      oa[4 * qh + dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf[dt], pf[qh], oa[4 * qh + dt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    };
    // a quarter of a half's probabilities: sub-tile i >> 1, registers 8 (i & 1) .. + 8 -- 8 fma, 8 exp2, 4 conversions, 8 adds
    auto probs_quarter = [&](int qh, int i, float off, float sum) -> float {     // off = 3 - m c
      const float cq = c[qh];
      const int sub = i >> 1;
#pragma unroll
      for (int g = 2 * (i & 1); g < 2 * (i & 1) + 2; ++g) {
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[j] = fmaf(s[qh][sub][4 * g + j], cq, off);
          if (LAST && t * KVB + sub * 32 + 8 * g + 4 * h2 + j >= Skv) x[j] = -INFINITY;
        }
        const float p0 = __builtin_amdgcn_exp2f(x[0]), p1 = __builtin_amdgcn_exp2f(x[1]);
        const float p2 = __builtin_amdgcn_exp2f(x[2]), p3 = __builtin_amdgcn_exp2f(x[3]);
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, w, true);
        pf[qh][sub * 4 + g] = w;
        sum += (p0 + p1) + (p2 + p3);       // fp32 sums of the unrounded probabilities
      }
      return sum;
    };
    auto probs = [&](int qh, float off) {
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) sum = probs_quarter(qh, i, off, sum);
      psum[qh] = sum;
    };
    auto exact = [&](int qh) {                // tile max, grow the offset, rescale O and l, redo the probabilities (every one <= 2^3)
      float mt = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const bool dead = LAST && t * KVB + sub * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2 >= Skv;
          mt = fmaxf(mt, dead ? -INFINITY : s[qh][sub][e]);
        }
      {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
        mt = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
      }
      const float m_new = fmaxf(m_run[qh], mt);
      const float alpha = __builtin_amdgcn_exp2f((m_run[qh] - m_new) * c[qh]);
      m_run[qh] = m_new;
      l_run[qh] *= alpha;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oa[4 * qh + dt] *= alpha;
      probs(qh, P_SHIFT - m_run[qh] * c[qh]);
    };
    // The order below is pinned (sched_barrier: nothing crosses): one MFMA, then a quarter of the other half's softmax.
    auto fence = []() { __builtin_amdgcn_sched_barrier(0); };
#pragma unroll
    for (int i = 0; i < 4; ++i) qk_mfma(0, i);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)   // (behind the last use of the K fragments of half 0's MFMAs; half 1's follow)
      vf[dt] = cat(*(const i4v*)(Vs + dt * 2048 + (((2 * h2) ^ v_sw) * 16)), *(const i4v*)(Vs + dt * 2048 + (((2 * h2 + 1) ^ v_sw) * 16)));
    {
      const float off = P_SHIFT - m_run[0] * c[0];
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fence();
        qk_mfma(1, i);
        fence();
        sum = probs_quarter(0, i, off, sum);
      }
      fence();
      psum[0] = sum;
    }
    if (__any(!(psum[0] <= P_LIMIT))) exact(0);               // a value above the e4m3 range is possible; also inf / NaN (tile 0: m = -inf)
    l_run[0] += psum[0];
    {
      const float off = P_SHIFT - m_run[1] * c[1];
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fence();
        pv_mfma(0, i);
        fence();
        sum = probs_quarter(1, i, off, sum);
      }
      fence();
      psum[1] = sum;
    }
    if (__any(!(psum[1] <= P_LIMIT))) exact(1);
    l_run[1] += psum[1];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) pv_mfma(1, dt);
  };
  for (int t = 0; t < T - 1; ++t) tile(t, std::false_type{});
  if (ragged)
    tile(T - 1, std::true_type{});
  else
    tile(T - 1, std::false_type{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped prefetches past the last tile: nothing may land after the workgroup ends

  const float* vs = p.vt_scale + (int64_t)bh * 128;
#pragma unroll
  for (int qh = 0; qh < 2; ++qh) {
    const float l_tot = l_run[qh] + __shfl_xor(l_run[qh], 32, 64);
    const float inv = 1.0f / l_tot;
    const int q_row = q_row0 + 32 * qh;
    if (q_row < Sq) {
      bf16_t* op = p.o + (int64_t)b * p.o_bs + (int64_t)q_row * p.o_rs + h * 128;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = dt * 32 + 8 * g + 4 * h2;
          const float4 sc = *(const float4*)(vs + d);
          uint2 v;
          v.x = pack_bf2(oa[4 * qh + dt][4 * g] * sc.x * inv, oa[4 * qh + dt][4 * g + 1] * sc.y * inv);
          v.y = pack_bf2(oa[4 * qh + dt][4 * g + 2] * sc.z * inv, oa[4 * qh + dt][4 * g + 3] * sc.w * inv);
          *(uint2*)(op + d) = v;
        }
    }
  }
}

// ---- producers -----------------------------------------------------------------------------------------------------------------
// The quantiser (amax8, e4m3_scale, e4m3x8) is row_ops.h's: the arithmetic of alg_quantize_fp8_rows

// K with one scale per (batch, head).  Pass 1: amax bits (non-negative floats order as unsigned integers) into scale[] by atomic
// max; pass 2 turns them into scales; pass 3 converts.  16 lanes per (token, head) row of 128.
constexpr int KH_TOKENS = 64;   // tokens per workgroup of passes 1 and 3
__global__ __launch_bounds__(256) void khead_amax_kernel(const bf16_t* __restrict__ x, int64_t x_bs, int64_t x_rs, unsigned* amax_bits,
                                                         int heads, int S) {
  const int b = blockIdx.y, s0 = blockIdx.x * KH_TOKENS;
  const int s1 = min(s0 + KH_TOKENS, S);
  const int per_row = heads * 16;
  for (int hc = threadIdx.x; hc < per_row; hc += 256) {   // one thread keeps one 8-channel column of one head over the tokens
    float amax = 0.0f;
    for (int s = s0; s < s1; ++s) amax = amax8(*(const uint4*)(x + (int64_t)b * x_bs + (int64_t)s * x_rs + hc * 8), amax);
    atomicMax(amax_bits + b * heads + (hc >> 4), __float_as_uint(amax));
  }
}
__global__ void khead_scale_kernel(float* scale, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float amax = scale[i];
    scale[i] = e4m3_scale(amax);
  }
}
__global__ __launch_bounds__(256) void khead_quant_kernel(const bf16_t* __restrict__ x, int64_t x_bs, int64_t x_rs,
                                                          uint8_t* __restrict__ q, int64_t q_bs, int64_t q_rs,
                                                          const float* __restrict__ scale, int heads, int S) {
  const int b = blockIdx.y, s0 = blockIdx.x * KH_TOKENS;
  const int s1 = min(s0 + KH_TOKENS, S);
  const int per_row = heads * 16;
  for (int hc = threadIdx.x; hc < per_row; hc += 256) {
    const float inv = 1.0f / scale[b * heads + (hc >> 4)];
    for (int s = s0; s < s1; ++s)
      *(uint2*)(q + (int64_t)b * q_bs + (int64_t)s * q_rs + hc * 8) =
          e4m3x8(*(const uint4*)(x + (int64_t)b * x_bs + (int64_t)s * x_rs + hc * 8), inv);
  }
}

// V^T: one wave per (batch, head, channel) row.  Output column 64 t + 32 h2 + 16 sub + 4 g + j holds key 64 t + 32 sub + 8 g + 4 h2 + j,
// so eight consecutive output bytes (fixed t, h2, sub, g in {2 g', 2 g' + 1}) are keys base + {0..3} and base + 8 + {0..3},
// base = 64 t + 32 sub + 16 g' + 4 h2.  In a source written with ALG_GEMM_PERMUTE_COLS (index bits 2 and 3 swapped) those are the
// eight consecutive columns 64 t + 32 sub + 16 g' + 8 h2 .. + 8: one 16-byte load.  A source in natural order takes two 8-byte loads.
template <bool SRC_PERM>
__global__ __launch_bounds__(256) void vt_quant_kernel(const bf16_t* __restrict__ x, int64_t x_bs, int64_t x_rs,
                                                       uint8_t* __restrict__ q, int64_t q_bs, int64_t q_rs, float* __restrict__ scale,
                                                       int rows, int Skv) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (row >= rows) return;
  const bf16_t* xr = x + (int64_t)b * x_bs + (int64_t)row * x_rs;
  uint8_t* qr = q + (int64_t)b * q_bs + (int64_t)row * q_rs;
  const int cols = (Skv + 63) & ~63;
  // the eight values behind output bytes o8 .. o8 + 7, keys >= Skv as zero
  auto fetch = [&](int o8) -> uint4 {
    const int t = o8 >> 6, h2 = (o8 >> 5) & 1, sub = (o8 >> 4) & 1, gp = (o8 >> 3) & 1;
    const int key0 = 64 * t + 32 * sub + 16 * gp + 4 * h2;    // keys key0 + {0..3}, key0 + 8 + {0..3}
    uint2 a, c;
    if (SRC_PERM) {
      const uint4 v = *(const uint4*)(xr + 64 * t + 32 * sub + 16 * gp + 8 * h2);
      a = make_uint2(v.x, v.y), c = make_uint2(v.z, v.w);
    } else {
      a = *(const uint2*)(xr + key0), c = *(const uint2*)(xr + key0 + 8);
    }
    uint32_t u[4] = {a.x, a.y, c.x, c.y};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = key0 + (i >> 1) * 8 + (i & 1) * 2;
      if (key >= Skv) u[i] = 0;
      else if (key + 1 >= Skv) u[i] &= 0xffffu;
    }
    return make_uint4(u[0], u[1], u[2], u[3]);
  };
  float amax = 0.0f;
  for (int o8 = lane * 8; o8 < cols; o8 += 512) amax = amax8(fetch(o8), amax);
  const float sc = e4m3_scale(xor_max<64>(amax));
  const float inv = 1.0f / sc;
  if (lane == 0) scale[(int64_t)b * rows + row] = sc;
  for (int o8 = lane * 8; o8 < cols; o8 += 512) *(uint2*)(qr + o8) = e4m3x8(fetch(o8), inv);
}

}  // namespace a128f8
}  // namespace alg

using namespace alg;

extern "C" int alg_flash_attn_d128_fp8(const void* q, const float* q_scale, const void* k, const float* k_scale, const void* vt,
                                       const float* vt_scale, void* o, int batch, int heads, int Sq, int Skv, int64_t q_bstride,
                                       int64_t q_rstride, int64_t k_bstride, int64_t k_rstride, int64_t vt_bstride,
                                       int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale, int kv_group,
                                       int causal, void* stream) {
  using namespace a128f8;
  static_assert(KVB == ATTN128_KVB, "the pitch check's tile is the kernel's");
  const Attn128Args a{q, k, vt, o, batch, heads, Sq, Skv, q_bstride, q_rstride, k_bstride, k_rstride, vt_bstride, vt_rstride,
                      o_bstride, o_rstride, scale, kv_group, causal, (hipStream_t)stream};
  // ---- check: the predicates of attn128_check at the e4m3 row modulus, around this entry's own messages and order
  if (attn128_bad_argument(a) || !q_scale || !k_scale || !vt_scale) {
    set_error("alg_flash_attn_d128_fp8: bad argument (batch=%d heads=%d Sq=%d Skv=%d)", batch, heads, Sq, Skv);
    return ALG_EINVAL;
  }
  if (kv_group != 1 || causal) {
    set_error("alg_flash_attn_d128_fp8: grouped-query (kv_group=%d) and causal (%d) attention are not covered: use alg_flash_attn_d128_ex",
              kv_group, causal);
    return ALG_EINVAL;
  }
  if (attn128_misaligned(a, 16) || ((uintptr_t)vt_scale & 15) || ((uintptr_t)q_scale & 3) || ((uintptr_t)k_scale & 3)) {
    set_error("alg_flash_attn_d128_fp8: q/k/vt need 16-byte aligned rows (strides %% 16 == 0), vt_scale 16-byte, o 8-byte aligned");
    return ALG_EINVAL;
  }
  if (attn128_pitch_short(vt_rstride, Skv)) {
    set_error("alg_flash_attn_d128_fp8: vt row stride %lld must cover Skv = %d rounded up to %d", (long long)vt_rstride, Skv, KVB);
    return ALG_EINVAL;
  }
  // ---- plan: one kernel, 256 queries per workgroup
  const int q_blocks = attn128_q_blocks(a, NW * QW);
  const int64_t grid = attn128_grid(a, q_blocks);
  // ---- launch
  static PerDeviceOnce attr_set;
  const int rc = opt_in_lds(attr_set, {(const void*)flash_attn_d128_fp8_kernel}, LDS_BYTES, "alg_flash_attn_d128_fp8");
  if (rc != ALG_OK) return rc;
  if (grid > 0x7fffffff) {
    set_error("alg_flash_attn_d128_fp8: grid too large");
    return ALG_ELIMIT;
  }
  P p;
  attn128_fill(p, a, q_blocks);
  p.q_scale = q_scale; p.k_scale = k_scale; p.vt_scale = vt_scale;
  hipLaunchKernelGGL(flash_attn_d128_fp8_kernel, dim3((unsigned)grid), dim3(NW * 64), LDS_BYTES, a.stream, p);
  return check_launch("alg_flash_attn_d128_fp8");
}

extern "C" int alg_quantize_fp8_khead(const void* x, int64_t x_bstride, int64_t x_rstride, void* q, int64_t q_bstride,
                                      int64_t q_rstride, float* scale, int batch, int heads, int S, int scale_given,
                                      void* stream) {
  using namespace a128f8;
  if (!x || !q || !scale || batch <= 0 || heads <= 0 || S <= 0 || x_rstride % 8 || x_bstride % 8 || q_rstride % 8 || q_bstride % 8 ||
      ((uintptr_t)x & 15) || ((uintptr_t)q & 7) || ((uintptr_t)scale & 3) || x_rstride < (int64_t)heads * 128 ||
      q_rstride < (int64_t)heads * 128) {
    set_error("alg_quantize_fp8_khead: bad argument (batch=%d heads=%d S=%d; x 16-byte, q 8-byte aligned rows of heads * 128)", batch,
              heads, S);
    return ALG_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((S + KH_TOKENS - 1) / KH_TOKENS), (unsigned)batch), blk(256);
  if (!scale_given) {
    if (hipMemsetAsync(scale, 0, sizeof(float) * (size_t)batch * heads, s) != hipSuccess) {
      set_error("alg_quantize_fp8_khead: hipMemsetAsync failed");
      return ALG_ELAUNCH;
    }
    hipLaunchKernelGGL(khead_amax_kernel, grid, blk, 0, s, (const bf16_t*)x, x_bstride, x_rstride, (unsigned*)scale, heads, S);
    hipLaunchKernelGGL(khead_scale_kernel, dim3((unsigned)((batch * heads + 255) / 256)), blk, 0, s, scale, batch * heads);
  }
  hipLaunchKernelGGL(khead_quant_kernel, grid, blk, 0, s, (const bf16_t*)x, x_bstride, x_rstride, (uint8_t*)q, q_bstride, q_rstride,
                     (const float*)scale, heads, S);
  return check_launch("alg_quantize_fp8_khead");
}

extern "C" int alg_quantize_fp8_vt(const void* x, int64_t x_bstride, int64_t x_rstride, void* q, int64_t q_bstride, int64_t q_rstride,
                                   float* scale, int batch, int rows, int Skv, int src_permuted, void* stream) {
  using namespace a128f8;
  const int64_t cols = ((int64_t)Skv + 63) & ~63ll;
  if (!x || !q || !scale || batch <= 0 || rows <= 0 || Skv <= 0 || x_rstride % 8 || x_bstride % 8 || q_rstride % 8 || q_bstride % 8 ||
      ((uintptr_t)x & 15) || ((uintptr_t)q & 7) || ((uintptr_t)scale & 3) || x_rstride < cols || q_rstride < cols) {
    set_error("alg_quantize_fp8_vt: bad argument (batch=%d rows=%d Skv=%d; both row strides must cover Skv rounded up to 64)", batch,
              rows, Skv);
    return ALG_EINVAL;
  }
  const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)batch), blk(256);
  if (src_permuted)
    hipLaunchKernelGGL(vt_quant_kernel<true>, grid, blk, 0, (hipStream_t)stream, (const bf16_t*)x, x_bstride, x_rstride, (uint8_t*)q,
                       q_bstride, q_rstride, scale, rows, Skv);
  else
    hipLaunchKernelGGL(vt_quant_kernel<false>, grid, blk, 0, (hipStream_t)stream, (const bf16_t*)x, x_bstride, x_rstride, (uint8_t*)q,
                       q_bstride, q_rstride, scale, rows, Skv);
  return check_launch("alg_quantize_fp8_vt");
}
