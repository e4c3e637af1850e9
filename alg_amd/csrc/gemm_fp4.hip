// OCP MXFP4 (e2m1 elements, one E8M0 scale per 32 along K) operands on v_mfma_scale_f32_32x32x64_f8f6f4 with both format
// selectors at FP4 and the real block scales in the scale operands + the row quantiser that feeds it.  A kernel of its own
// (the bf16 / e4m3 template of gemm_kernel.h is not touched): 128 x 128 tile, 4 waves as 2 x 2, each 2 x 2 blocks of 32 x 32,
// k-tiles of 256 elements = 128 bytes per row (schedule 6's staging width: a lane's 16-byte fragment is 32 e2m1 values = one
// MX block = one operand of the K = 64 instruction).  Correctness first: one LDS buffer, the next k-tile waits in registers
// while the current one is multiplied; tuning is left for later.
//
// alg_gemm_fp4_q4out is the same kernel with an MXFP4 output (Q4): the epilogue's bf16 values are quantised where they are, as
// alg_quantize_mxfp4_rows would quantise the bf16 tensor, and only the e2m1 bytes + the E8M0 scales are stored.
#include "common.h"
#include "row_ops.h"

namespace alg {
namespace {
constexpr int FT = 128;        // tile rows (M) and columns (N)
constexpr int FKB = 128;       // bytes of one operand row per k-tile (256 e2m1 values, 8 scale bytes)
typedef int i8v __attribute__((ext_vector_type(8)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));   // native vectors: the staging registers stay registers
typedef unsigned u2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void unpack_bf4(const uint2 v, float (&f)[4]) {
  f[0] = __uint_as_float(v.x << 16);
  f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16);
  f[3] = __uint_as_float(v.y & 0xffff0000u);
}

// Operand lane map of the instruction with FP4 data (checked with exact integer data, tests/test_gpu_mxfp4.py): lane l holds
// row l & 31, k = 32 (l >> 5) + j for j = 0..31 in the first four of its eight operand registers, element 2i in the low nibble
// of byte i; the lane's scale operand (byte 0, opsel 0) is the E8M0 scale of exactly those 32 values.
// Q4 (alg_gemm_fp4_q4out): C is [batch][M][N / 2] e2m1 bytes, out_scales [batch][M][N / 32] E8M0 bytes
template <int ACT, bool RES, bool Q4>
__global__ __launch_bounds__(256) void gemm_fp4_kernel(const alg_gemm_args p, const int m_tiles, const int n_tiles,
                                                       uint8_t* __restrict__ out_scales, const int64_t out_scales_bs) {
  __shared__ __attribute__((aligned(16))) char lds[2][FT * FKB];   // A rows, B rows: row r chunk c at r * 128 + ((c ^ (r & 7)) * 16)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, l31 = lane & 31, h = lane >> 5;
  const int per = m_tiles * n_tiles;
  const int b = blockIdx.x / per, rem = blockIdx.x - b * per;
  const int m0 = (rem % m_tiles) * FT, n0 = (rem / m_tiles) * FT;
  const int64_t lda_b = p.lda >> 1, ldb_b = p.ldb >> 1, sc_ld = p.K >> 5;
  const char* Ab = (const char*)p.A + (int64_t)b * (p.strideA >> 1);
  const char* Bb = (const char*)p.B + (int64_t)b * (p.strideB >> 1);
  const uint8_t* As = (const uint8_t*)p.a_scale + (int64_t)b * p.strideAScale;
  const uint8_t* Bs = (const uint8_t*)p.b_scale + (int64_t)b * p.strideBScale;

  // staging: thread t moves chunk t & 7 of rows (t >> 3) + 32 i; edge tiles clamp the row (their results are never stored)
  const int sc = tid & 7, sr = tid >> 3;
  const char* ga[4];
  const char* gb[4];
  int lo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = sr + 32 * i;
    const int ra = m0 + r < p.M ? m0 + r : p.M - 1, rb = n0 + r < p.N ? n0 + r : p.N - 1;
    ga[i] = Ab + ra * lda_b + sc * 16;
    gb[i] = Bb + rb * ldb_b + sc * 16;
    lo[i] = r * FKB + ((sc ^ (r & 7)) * 16);
  }
  // fragments: the lane's rows of the wave's 2 x 2 blocks, and the scale bytes of those rows (8 per k-tile)
  int fa[2], fb[2];
  const uint8_t* ka[2];
  const uint8_t* kb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    fa[t] = wm * 64 + t * 32 + l31;
    fb[t] = wn * 64 + t * 32 + l31;
    const int ra = m0 + fa[t] < p.M ? m0 + fa[t] : p.M - 1, rb = n0 + fb[t] < p.N ? n0 + fb[t] : p.N - 1;
    ka[t] = As + ra * sc_ld;
    kb[t] = Bs + rb * sc_ld;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.0f;

  u4v va[4], vb[4];
  u2v sa[2], sb[2];
  auto fetch = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      va[i] = *(const u4v*)(ga[i] + (int64_t)kt * FKB);
      vb[i] = *(const u4v*)(gb[i] + (int64_t)kt * FKB);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sa[t] = *(const u2v*)(ka[t] + kt * 8);
      sb[t] = *(const u2v*)(kb[t] + kt * 8);
    }
  };
  // the lane's 16-byte chunk ch of tile row `row` as the instruction's operand (FP4 reads the first four registers)
  auto frag = [](const char* base, int row, int ch) -> i8v {
    const u4v x = *(const u4v*)(base + row * FKB + ((ch ^ (row & 7)) * 16));
    return i8v{(int)x.x, (int)x.y, (int)x.z, (int)x.w, 0, 0, 0, 0};
  };
  // scale byte 2 ks + h of the row's eight, in byte 0 of the scale operand (opsel 0)
  auto sbyte = [](const u2v s8, int ks, int sh) -> int { return (int)(((ks < 2 ? s8.x : s8.y) >> sh) & 0xffu); };
  const int nk = p.K >> 8;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();   // everybody is done reading the previous k-tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(u4v*)(lds[0] + lo[i]) = va[i];
      *(u4v*)(lds[1] + lo[i]) = vb[i];
    }
    const u2v ca[2] = {sa[0], sa[1]}, cb[2] = {sb[0], sb[1]};
    __syncthreads();
    fetch(kt + 1 < nk ? kt + 1 : kt);   // (the last round re-reads its own tile: no branch around loads in flight)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int ch = 2 * ks + h, sh = 8 * (ch & 3);   // the lane's 16-byte chunk = MX block of this k-step
      // B first: C^T blocks, so a lane owns four consecutive output columns of one row per register quad
      const i8v a0 = frag(lds[0], fa[0], ch), a1 = frag(lds[0], fa[1], ch), b0 = frag(lds[1], fb[0], ch), b1 = frag(lds[1], fb[1], ch);
      const int as0 = sbyte(ca[0], ks, sh), as1 = sbyte(ca[1], ks, sh), bs0 = sbyte(cb[0], ks, sh), bs1 = sbyte(cb[1], ks, sh);
      acc[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b0, a0, acc[0][0], 4, 4, 0, bs0, 0, as0);
      acc[0][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b1, a0, acc[0][1], 4, 4, 0, bs1, 0, as0);
      acc[1][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b0, a1, acc[1][0], 4, 4, 0, bs0, 0, as1);
      acc[1][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b1, a1, acc[1][1], 4, 4, 0, bs1, 0, as1);
    }
  }

  // ---- epilogue: the arithmetic of the bf16 / e4m3 kernel's element-exact path (gemm_kernel.h), 64-bit offsets ----
  const bf16_t* bias = (const bf16_t*)p.bias;
  if constexpr (Q4) {
    // MXFP4 output (N % 32 == 0, no residual).  An MX block of an output row -- the 32 columns of one (mt, nt) -- lives in the lane
    // pair (l, l + 32): lane half h holds columns 8 g + 4 h + i.  One half exchange gives both lanes the block's amax; a second
    // one moves the halves' bytes so that the lower lane holds bytes 0-7 of the block's sixteen and the upper lane bytes 8-15:
    // one 8-byte store per lane and block.  Every lane runs the exchanges; only the stores are guarded.
    uint8_t* Cq = (uint8_t*)p.C + (int64_t)b * (p.strideC >> 1);
    uint8_t* Sq = out_scales + (int64_t)b * out_scales_bs;
    const int64_t ldc_b = p.ldc >> 1, ldsc = p.N >> 5;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int row = m0 + fa[mt];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int nb = n0 + wn * 64 + nt * 32;            // the block's first column: wave-uniform
        const int nbc = nb < p.N ? nb : p.N - 32;         // (a block past N reads the last block's bias and stores nothing)
        float v[4][4];
        float amax = 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float bv[4] = {0.f, 0.f, 0.f, 0.f};
          if (bias) unpack_bf4(*(const uint2*)(bias + nbc + 8 * g + 4 * h), bv);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float x = rbf(acc[mt][nt][4 * g + i] + bv[i]);   // nn.Linear returns a bf16 tensor
            if (ACT != ALG_ACT_NONE) x = rbf(act_apply(x, ACT));
            v[g][i] = x;
            amax = fmaxf(amax, fabsf(x));
          }
        }
        {
          const unsigned am = __float_as_uint(amax);
          const auto r = __builtin_amdgcn_permlane32_swap(am, am, false, false);   // r[0] | r[1]: own, the other half's
          amax = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
        }
        const int e = mxfp4_scale_byte(amax);
        // lo: this half's two bytes of column groups 0 and 1, hi: of groups 2 and 3
        const unsigned lo = e2m1_pack(v[0], e) | (e2m1_pack(v[1], e) << 16), hi = e2m1_pack(v[2], e) | (e2m1_pack(v[3], e) << 16);
        // the upper lanes' lo <-> the lower lanes' hi: a lower lane then holds groups 0, 1 of both halves, an upper lane groups 2, 3
        const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
        const unsigned h0 = r[0], h1 = r[1];   // the lane's two groups as half 0 and as half 1 hold them
        uint2 o;
        o.x = (h0 & 0xffffu) | (h1 << 16);
        o.y = (h0 >> 16) | (h1 & 0xffff0000u);
        if (row < p.M && nb < p.N) {
          *(uint2*)(Cq + row * ldc_b + (nb >> 1) + 8 * h) = o;
          if (h == 0) Sq[row * ldsc + (nb >> 5)] = (uint8_t)e;
        }
      }
    }
    return;
  }
  const bf16_t* R = RES ? (const bf16_t*)p.R + (int64_t)b * p.strideR : nullptr;
  const bf16_t* gate = (RES && p.gate) ? (const bf16_t*)p.gate + (int64_t)b * p.strideGate : nullptr;
  const int64_t gate_seg = (p.flags & ALG_GEMM_GATE_SEG_STRIDE) ? p.gate_seg_stride : p.N;
  const bool gate_f32 = RES && p.gate && (p.flags & ALG_GEMM_GATE_F32);
  bf16_t* Cb = (bf16_t*)p.C + (int64_t)b * p.strideC;
  const bool n_vec = (p.N & 3) == 0;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int row = m0 + fa[mt];
    if (row >= p.M) continue;
    const int64_t gseg = row >= p.seg_split ? gate_seg : 0;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + nt * 32 + 8 * g + 4 * h;
        if (n_vec) {
          if (n >= p.N) continue;
          float bv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {1.f, 1.f, 1.f, 1.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
          if (bias) unpack_bf4(*(const uint2*)(bias + n), bv);
          if (RES && gate) {
            if (gate_f32) {
              const float4 g4 = *(const float4*)((const float*)p.gate + (int64_t)b * p.strideGate + gseg + n);
              gv[0] = g4.x, gv[1] = g4.y, gv[2] = g4.z, gv[3] = g4.w;
            } else {
              unpack_bf4(*(const uint2*)(gate + gseg + n), gv);
            }
          }
          if (RES) unpack_bf4(*(const uint2*)(R + row * p.ldr + n), rv);
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float x = rbf(acc[mt][nt][4 * g + i] + bv[i]);   // nn.Linear returns a bf16 tensor
            if (ACT != ALG_ACT_NONE) x = rbf(act_apply(x, ACT));
            if (RES) x = gate_f32 ? rv[i] + gv[i] * x : rv[i] + rbf(gv[i] * x);
            v[i] = x;
          }
          uint2 o;
          o.x = pack_bf2(v[0], v[1]);
          o.y = pack_bf2(v[2], v[3]);
          *(uint2*)(Cb + row * p.ldc + n) = o;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int nn = n + i;
            if (nn >= p.N) continue;
            float x = rbf(acc[mt][nt][4 * g + i] + (bias ? bf2f(bias[nn]) : 0.0f));
            if (ACT != ALG_ACT_NONE) x = rbf(act_apply(x, ACT));
            if (RES) {
              if (gate_f32) {
                x = bf2f(R[row * p.ldr + nn]) + ((const float*)p.gate)[(int64_t)b * p.strideGate + gseg + nn] * x;
              } else {
                x = bf2f(R[row * p.ldr + nn]) + rbf((gate ? bf2f(gate[gseg + nn]) : 1.0f) * x);
              }
            }
            Cb[row * p.ldc + nn] = f2bf(x);
          }
        }
      }
  }
}

// (the block quantiser, mxfp4_quantize8: row_ops.h -- eight bf16 values per lane, four lanes share an MX block)
__global__ __launch_bounds__(256) void quantize_mxfp4_rows_kernel(const bf16_t* __restrict__ x, int64_t x_rs, uint8_t* __restrict__ q,
                                                                  uint8_t* __restrict__ scales, int64_t rows, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* xr = x + row * x_rs;
  uint8_t* qr = q + row * (int64_t)(K >> 1);
  uint8_t* sr = scales + row * (int64_t)(K >> 5);
  // K % 32 == 0: the four lanes of a block are inside K together
  for (int c = lane * 8; c < K; c += 512) mxfp4_quantize8(*(const uint4*)(xr + c), qr + (c >> 1), sr + (c >> 5), lane);
}

template <int ACT, bool RES>
int launch_fp4(const alg_gemm_args* a, int m_tiles, int n_tiles, unsigned nwg, hipStream_t s) {
  hipLaunchKernelGGL((gemm_fp4_kernel<ACT, RES, false>), dim3(nwg), dim3(256), 0, s, *a, m_tiles, n_tiles, (uint8_t*)nullptr,
                     (int64_t)0);
  return check_launch("alg_gemm_fp4");
}
template <int ACT>
int launch_fp4_q4out(const alg_gemm_args* a, int m_tiles, int n_tiles, unsigned nwg, uint8_t* out_scales, int64_t out_scales_bs,
                     hipStream_t s) {
  hipLaunchKernelGGL((gemm_fp4_kernel<ACT, false, true>), dim3(nwg), dim3(256), 0, s, *a, m_tiles, n_tiles, out_scales, out_scales_bs);
  return check_launch("alg_gemm_fp4_q4out");
}
}  // namespace
}  // namespace alg

using namespace alg;

// The refusals both entries share, each written once; `entry` is the name the messages carry.  q4out: C holds e2m1 bytes (the
// output-side rules are alg_gemm_fp4_q4out's own, below).
static int gemm_fp4_check(const alg_gemm_args* a, const char* entry, bool q4out) {
  if (!a || !a->A || !a->B || !a->C || !a->a_scale || !a->b_scale) {
    set_error("%s: null argument (A, B, C, a_scale and b_scale are required)", entry);
    return ALG_EINVAL;
  }
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0 || a->K % 256) {
    set_error("%s: bad shape M=%d N=%d K=%d batch=%d (K %% 256 == 0)", entry, a->M, a->N, a->K, a->batch);
    return ALG_EINVAL;
  }
  if (a->flags & (ALG_GEMM_B_PACKED11 | ALG_GEMM_BIAS_PER_ROW | ALG_GEMM_PERMUTE_COLS)) {
    set_error("%s: ALG_GEMM_B_PACKED11, ALG_GEMM_BIAS_PER_ROW and ALG_GEMM_PERMUTE_COLS are not built for MXFP4 operands (flags=%d)",
              entry, a->flags);
    return ALG_EINVAL;
  }
  if (a->conv_wp || a->conv_cin_log2 || a->conv_hpwp || a->conv_kw) {
    set_error("%s: convolution addressing is not built for MXFP4 operands", entry);
    return ALG_EINVAL;
  }
  if (a->lda % 32 || a->ldb % 32 || a->strideA % 32 || a->strideB % 32 || a->lda < a->K || a->ldb < a->K || a->strideA < 0 ||
      a->strideB < 0 || ((uintptr_t)a->A & 15) || ((uintptr_t)a->B & 15)) {
    set_error("%s: A/B must be 16-byte aligned with lda/ldb >= K and lda/ldb/strides multiples of 32 elements (16 bytes)", entry);
    return ALG_EINVAL;
  }
  if (((uintptr_t)a->a_scale & 7) || ((uintptr_t)a->b_scale & 7) || (a->strideAScale & 7) || (a->strideBScale & 7) ||
      a->strideAScale < 0 || a->strideBScale < 0) {
    set_error("%s: a_scale / b_scale (E8M0 bytes, [rows][K/32]) must be 8-byte aligned with batch strides multiples of 8 bytes", entry);
    return ALG_EINVAL;
  }
  if (a->act < ALG_ACT_NONE || a->act > ALG_ACT_SILU) {
    set_error("%s: unknown activation %d", entry, a->act);
    return ALG_EINVAL;
  }
  if ((a->R && a->act != ALG_ACT_NONE) || (a->gate && !a->R)) {
    set_error("%s: an activation cannot be combined with the residual epilogue, and a gate needs a residual", entry);
    return ALG_EINVAL;
  }
  if (!q4out && (a->N & 3) == 0) {   // 8-byte epilogue accesses
    const bool bad = (a->ldc & 3) || (a->strideC & 3) || ((uintptr_t)a->C & 7) || (a->bias && ((uintptr_t)a->bias & 7)) ||
                     (a->R && ((a->ldr & 3) || (a->strideR & 3) || ((uintptr_t)a->R & 7))) ||
                     (a->gate && ((a->strideGate & 3) || ((a->flags & ALG_GEMM_GATE_SEG_STRIDE) && (a->gate_seg_stride & 3)) ||
                                  ((uintptr_t)a->gate & ((a->flags & ALG_GEMM_GATE_F32) ? 15 : 7))));
    if (bad) {
      set_error("%s: C/bias/R/gate must be 8-byte aligned with ldc/ldr/strides multiples of 4 elements", entry);
      return ALG_EINVAL;
    }
  }
  const int64_t nwg = (int64_t)((a->M + FT - 1) / FT) * ((a->N + FT - 1) / FT) * a->batch;
  if (nwg > 0x7fffffff) {
    set_error("%s: grid too large", entry);
    return ALG_ELIMIT;
  }
  return ALG_OK;
}

extern "C" int alg_gemm_fp4(const alg_gemm_args* a, void* stream) {
  if (const int rc = gemm_fp4_check(a, "alg_gemm_fp4", false)) return rc;
  const int m_tiles = (a->M + FT - 1) / FT, n_tiles = (a->N + FT - 1) / FT;
  const unsigned nwg = (unsigned)((int64_t)m_tiles * n_tiles * a->batch);
  hipStream_t s = (hipStream_t)stream;
  if (a->R) return launch_fp4<ALG_ACT_NONE, true>(a, m_tiles, n_tiles, nwg, s);
  if (a->act == ALG_ACT_GELU_TANH) return launch_fp4<ALG_ACT_GELU_TANH, false>(a, m_tiles, n_tiles, nwg, s);
  if (a->act == ALG_ACT_SILU) return launch_fp4<ALG_ACT_SILU, false>(a, m_tiles, n_tiles, nwg, s);
  return launch_fp4<ALG_ACT_NONE, false>(a, m_tiles, n_tiles, nwg, s);
}

// [p, p + the bytes batch items of `rows` rows at these strides span), for the overlap refusals
static bool fp4_spans_overlap(const void* p, int64_t bstride, int64_t rstride, int64_t row_bytes, const void* q, int64_t q_bstride,
                              int64_t q_rstride, int64_t q_row_bytes, int batch, int rows) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  const uintptr_t p1 = p0 + (uintptr_t)((batch - 1) * bstride + (rows - 1) * rstride + row_bytes);
  const uintptr_t q1 = q0 + (uintptr_t)((batch - 1) * q_bstride + (rows - 1) * q_rstride + q_row_bytes);
  return p0 < q1 && q0 < p1;
}

extern "C" int alg_gemm_fp4_q4out(const alg_gemm_args* a, void* out_scales, int64_t out_scales_bstride, void* stream) {
  static const char* const entry = "alg_gemm_fp4_q4out";
  if (const int rc = gemm_fp4_check(a, entry, true)) return rc;
  if (a->N % 32) {
    set_error("%s: N=%d must be a multiple of 32 (whole MX blocks along the output row)", entry, a->N);
    return ALG_EINVAL;
  }
  if (a->R || a->gate) {
    set_error("%s: the residual epilogue (R, gate) has no MXFP4 output", entry);
    return ALG_EINVAL;
  }
  if (a->act != ALG_ACT_NONE && a->act != ALG_ACT_GELU_TANH) {
    set_error("%s: activation %d is not built for the MXFP4 output (ALG_ACT_NONE, ALG_ACT_GELU_TANH)", entry, a->act);
    return ALG_EINVAL;
  }
  if (a->ldc % 32 || a->strideC % 32 || a->ldc < a->N || a->strideC < 0 || ((uintptr_t)a->C & 15) ||
      (a->bias && ((uintptr_t)a->bias & 7))) {
    set_error("%s: C (e2m1 bytes) must be 16-byte aligned with ldc >= N and ldc / strideC multiples of 32 elements; bias 8-byte aligned",
              entry);
    return ALG_EINVAL;
  }
  if (!out_scales || ((uintptr_t)out_scales & 7) || (out_scales_bstride & 7) || out_scales_bstride < 0) {
    set_error("%s: out_scales (E8M0 bytes, [batch][M][N/32]) must be given, 8-byte aligned, its batch stride a multiple of 8 bytes",
              entry);
    return ALG_EINVAL;
  }
  // workgroups read A and its scales while others store C and out_scales
  if (fp4_spans_overlap(a->A, a->strideA >> 1, a->lda >> 1, a->K >> 1, a->C, a->strideC >> 1, a->ldc >> 1, a->N >> 1, a->batch, a->M) ||
      fp4_spans_overlap(a->a_scale, a->strideAScale, a->K >> 5, a->K >> 5, out_scales, out_scales_bstride, a->N >> 5, a->N >> 5,
                        a->batch, a->M)) {
    set_error("%s: C overlaps A (or out_scales overlaps a_scale): the output needs buffers of its own", entry);
    return ALG_EINVAL;
  }
  const int m_tiles = (a->M + FT - 1) / FT, n_tiles = (a->N + FT - 1) / FT;
  const unsigned nwg = (unsigned)((int64_t)m_tiles * n_tiles * a->batch);
  hipStream_t s = (hipStream_t)stream;
  if (a->act == ALG_ACT_GELU_TANH)
    return launch_fp4_q4out<ALG_ACT_GELU_TANH>(a, m_tiles, n_tiles, nwg, (uint8_t*)out_scales, out_scales_bstride, s);
  return launch_fp4_q4out<ALG_ACT_NONE>(a, m_tiles, n_tiles, nwg, (uint8_t*)out_scales, out_scales_bstride, s);
}

extern "C" int alg_quantize_mxfp4_rows(const void* x, int64_t x_rstride, void* q, void* scales, int64_t rows, int K, void* stream) {
  if (rows < 0 || K <= 0 || K % 32 || x_rstride % 8 || x_rstride < K || (rows + 3) / 4 > 0x7fffffff) {
    set_error("alg_quantize_mxfp4_rows: bad shape rows=%lld K=%d x_rstride=%lld (K %% 32 == 0, x_rstride >= K and %% 8 == 0)",
              (long long)rows, K, (long long)x_rstride);
    return ALG_EINVAL;
  }
  if (rows == 0) return ALG_OK;
  if (!x || !q || !scales || ((uintptr_t)x & 15) || ((uintptr_t)q & 3)) {
    set_error("alg_quantize_mxfp4_rows: null or misaligned pointer (x 16-byte, q 4-byte aligned)");
    return ALG_EINVAL;
  }
  hipLaunchKernelGGL(quantize_mxfp4_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, x_rstride, (uint8_t*)q, (uint8_t*)scales, rows, K);
  return check_launch("alg_quantize_mxfp4_rows");
}
