// OCP MXFP4 (e2m1 elements, one E8M0 scale per 32 along K) operands on v_mfma_scale_f32_32x32x64_f8f6f4 with both format
// selectors at FP4 and the real block scales in the scale operands + the row quantiser that feeds it.  A kernel of its own
// (the bf16 / e4m3 template of gemm_kernel.h is not touched): 128 x 128 tile, 4 waves as 2 x 2, each 2 x 2 blocks of 32 x 32,
// k-tiles of 256 elements = 128 bytes per row (schedule 6's staging width: a lane's 16-byte fragment is 32 e2m1 values = one
// MX block = one operand of the K = 64 instruction).  Correctness first: one LDS buffer, the next k-tile waits in registers
// while the current one is multiplied; tuning is left for later.
#include "common.h"

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
template <int ACT, bool RES>
__global__ __launch_bounds__(256) void gemm_fp4_kernel(const alg_gemm_args p, const int m_tiles, const int n_tiles) {
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

// Eight bf16 values (one 16-byte load) of an MX block: four lanes share a block.
__device__ __forceinline__ void mxfp4_quantize8(const uint4 v, uint8_t* __restrict__ q4, uint8_t* __restrict__ scale, int lane) {
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
  float f[8];
  float amax = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = __uint_as_float(u[k] << 16);
    f[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
    amax = fmaxf(amax, fmaxf(fabsf(f[2 * k]), fabsf(f[2 * k + 1])));
  }
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  // E8M0 byte: floor(log2(amax)) - 2 clamped to [-127, 127], + 127.  floor(log2) of a normal number is its exponent field - 127;
  // a subnormal amax (field 0) lies below 2^-126 and clamps to byte 0 like field 1 and 2 do.  A zero block writes 127.
  const int ef = (int)(__float_as_uint(amax) >> 23);
  const int e = amax > 0.0f ? (ef > 2 ? ef - 2 : 0) : 127;
  const float inv = __uint_as_float((uint32_t)(254 - e) << 23);   // 2^(127 - e): e <= 252, so a normal number
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float a = fabsf(f[k]) * inv;   // exact (a power of two), or underflows far below the first tie point
    // nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating: one compare per boundary
    const uint32_t code = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                          (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
    out |= (code | ((__float_as_uint(f[k]) >> 28) & 8u)) << (4 * k);
  }
  *(uint32_t*)q4 = out;
  if ((lane & 3) == 0) *scale = (uint8_t)e;
}

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
  hipLaunchKernelGGL((gemm_fp4_kernel<ACT, RES>), dim3(nwg), dim3(256), 0, s, *a, m_tiles, n_tiles);
  return check_launch("alg_gemm_fp4");
}
}  // namespace
}  // namespace alg

using namespace alg;

extern "C" int alg_gemm_fp4(const alg_gemm_args* a, void* stream) {
  if (!a || !a->A || !a->B || !a->C || !a->a_scale || !a->b_scale) {
    set_error("alg_gemm_fp4: null argument (A, B, C, a_scale and b_scale are required)");
    return ALG_EINVAL;
  }
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0 || a->K % 256) {
    set_error("alg_gemm_fp4: bad shape M=%d N=%d K=%d batch=%d (K %% 256 == 0)", a->M, a->N, a->K, a->batch);
    return ALG_EINVAL;
  }
  if (a->flags & (ALG_GEMM_B_PACKED11 | ALG_GEMM_BIAS_PER_ROW | ALG_GEMM_PERMUTE_COLS)) {
    set_error("alg_gemm_fp4: ALG_GEMM_B_PACKED11, ALG_GEMM_BIAS_PER_ROW and ALG_GEMM_PERMUTE_COLS are not built for MXFP4 operands (flags=%d)",
              a->flags);
    return ALG_EINVAL;
  }
  if (a->conv_wp || a->conv_cin_log2 || a->conv_hpwp || a->conv_kw) {
    set_error("alg_gemm_fp4: convolution addressing is not built for MXFP4 operands");
    return ALG_EINVAL;
  }
  if (a->lda % 32 || a->ldb % 32 || a->strideA % 32 || a->strideB % 32 || a->lda < a->K || a->ldb < a->K || a->strideA < 0 ||
      a->strideB < 0 || ((uintptr_t)a->A & 15) || ((uintptr_t)a->B & 15)) {
    set_error("alg_gemm_fp4: A/B must be 16-byte aligned with lda/ldb >= K and lda/ldb/strides multiples of 32 elements (16 bytes)");
    return ALG_EINVAL;
  }
  if (((uintptr_t)a->a_scale & 7) || ((uintptr_t)a->b_scale & 7) || (a->strideAScale & 7) || (a->strideBScale & 7) ||
      a->strideAScale < 0 || a->strideBScale < 0) {
    set_error("alg_gemm_fp4: a_scale / b_scale (E8M0 bytes, [rows][K/32]) must be 8-byte aligned with batch strides multiples of 8 bytes");
    return ALG_EINVAL;
  }
  if (a->act < ALG_ACT_NONE || a->act > ALG_ACT_SILU) {
    set_error("alg_gemm_fp4: unknown activation %d", a->act);
    return ALG_EINVAL;
  }
  if ((a->R && a->act != ALG_ACT_NONE) || (a->gate && !a->R)) {
    set_error("alg_gemm_fp4: an activation cannot be combined with the residual epilogue, and a gate needs a residual");
    return ALG_EINVAL;
  }
  if ((a->N & 3) == 0) {   // 8-byte epilogue accesses
    const bool bad = (a->ldc & 3) || (a->strideC & 3) || ((uintptr_t)a->C & 7) || (a->bias && ((uintptr_t)a->bias & 7)) ||
                     (a->R && ((a->ldr & 3) || (a->strideR & 3) || ((uintptr_t)a->R & 7))) ||
                     (a->gate && ((a->strideGate & 3) || ((a->flags & ALG_GEMM_GATE_SEG_STRIDE) && (a->gate_seg_stride & 3)) ||
                                  ((uintptr_t)a->gate & ((a->flags & ALG_GEMM_GATE_F32) ? 15 : 7))));
    if (bad) {
      set_error("alg_gemm_fp4: C/bias/R/gate must be 8-byte aligned with ldc/ldr/strides multiples of 4 elements");
      return ALG_EINVAL;
    }
  }
  const int m_tiles = (a->M + FT - 1) / FT, n_tiles = (a->N + FT - 1) / FT;
  const int64_t nwg = (int64_t)m_tiles * n_tiles * a->batch;
  if (nwg > 0x7fffffff) {
    set_error("alg_gemm_fp4: grid too large");
    return ALG_ELIMIT;
  }
  hipStream_t s = (hipStream_t)stream;
  if (a->R) return launch_fp4<ALG_ACT_NONE, true>(a, m_tiles, n_tiles, (unsigned)nwg, s);
  if (a->act == ALG_ACT_GELU_TANH) return launch_fp4<ALG_ACT_GELU_TANH, false>(a, m_tiles, n_tiles, (unsigned)nwg, s);
  if (a->act == ALG_ACT_SILU) return launch_fp4<ALG_ACT_SILU, false>(a, m_tiles, n_tiles, (unsigned)nwg, s);
  return launch_fp4<ALG_ACT_NONE, false>(a, m_tiles, n_tiles, (unsigned)nwg, s);
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
