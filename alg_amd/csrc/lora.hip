// LoRA merge at load time (an extension: the reference pipelines inherit diffusers' LoRA loader mixins; alg_amd/lora.py):
//   t[n, r]   = double(scale[r]) * double(B[n, r])                  exact: two fp32 factors
//   acc[n, k] = fma(t[n, r], double(A[r, k]), acc)  r = 0 .. R-1 ascending, from acc = 0, in double (the ONE fused statement)
//   out[n, k] = bf16_rne(double(W[n, k]) + acc[n, k])               one rounding, from the double sum straight to bf16
// W is bf16 or fp32 (an fp32 checkpoint is rounded once: never to bf16 before the delta is added, never through fp32 after it),
// A, B and scale stay fp32 from the file to the kernel: an fp16, bf16 or fp32 adapter file is upcast exactly and no adapter is
// ever rounded.  Several adapters are concatenated along R by the host, each column with its own scale.
//
// Why double: with an fp32 chain the absolute error is an fp32 ulp of the OPERANDS per step, which is several bf16 steps of an
// element where W and the delta cancel to 2^-13 of their size or less (measured: up to 8 steps on single elements of 133,640).
// In double the result is within one bf16 step of bf16(float64 merge) everywhere.  The vector fp64 FMA runs at half the fp32
// rate on gfx950, and this runs once per model load.
//
// The chain of an output element is a function of its own operands alone -- r ascending, whatever the tile, the grid or the place
// of the row in the matrix -- so a slice merged alone gives the bits of the full merge and every rank of a multi-GPU run agrees.
// No MFMA (a bf16 MFMA would round A and t), no atomics, no split along R.
//
// A workgroup of 256 threads owns 64 rows x 128 columns, a thread 4 rows x 8 columns (one 16-byte bf16 store per row); A (fp32)
// and t (double) are staged through LDS 32 rank columns at a time.  Every element of out is read (as W) and written by the same
// thread, the read first: out may be W itself.  Bytes between K and a leading dimension are neither read nor written.
#include "common.h"
#include "row_ops.h"

namespace alg {

constexpr int LM_THREADS = 256;
constexpr int LM_ROWS = 64, LM_COLS = 128;   // the workgroup's tile
constexpr int LM_RC = 32;                    // rank columns staged per round
constexpr int LM_TPITCH = LM_ROWS + 2;       // doubles per rank column of the t tile (keeps the 16-byte reads aligned)
constexpr int LM_MAX_R = 512;

struct LoraMergeArgs {
  const void* W;
  int w_dtype;
  int64_t ldw;
  const float *A, *B, *scale;
  void* out;
  int64_t ldo;
  int N, K, R;
};

struct LoraMergePlan {
  int col_tiles;
  int64_t blocks;
};

template <typename WT>
__device__ __forceinline__ void lm_load8(const WT* p, float (&w)[8]);
template <>
__device__ __forceinline__ void lm_load8<bf16_t>(const bf16_t* p, float (&w)[8]) {
  unpack8(*(const uint4*)p, w);
}
template <>
__device__ __forceinline__ void lm_load8<float>(const float* p, float (&w)[8]) {
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
  w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}

// double -> bf16, round to nearest even ONCE: the double is first rounded to fp32 "to odd" (truncate, then set the last bit if
// anything was lost), which keeps every tie and every side of a tie of the 8-bit target visible to the final fp32 -> bf16 RNE
__device__ __forceinline__ float lm_round_to_odd(double x) {
  float f = (float)x;
  if ((double)f != x) {
    uint32_t u = __float_as_uint(f);
    if (fabs((double)f) > fabs(x)) u -= 1;   // back towards zero: the magnitude's bit pattern is monotonic
    f = __uint_as_float(u | 1u);
  }
  return f;
}

// W and out carry no __restrict__: they may be the same buffer
template <typename WT>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(const WT* W, int64_t ldw, const float* __restrict__ A,
                                                                const float* __restrict__ B, const float* __restrict__ scale,
                                                                bf16_t* out, int64_t ldo, int N, int K, int R, int col_tiles) {
  __shared__ __attribute__((aligned(16))) float sA[LM_RC][LM_COLS];
  __shared__ __attribute__((aligned(16))) double sT[LM_RC][LM_TPITCH];
  const int tid = threadIdx.x;
  const int cg = tid & 15, rg = tid >> 4;
  const int n0 = (int)(blockIdx.x / col_tiles) * LM_ROWS, k0 = (int)(blockIdx.x % col_tiles) * LM_COLS;

  double acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

  for (int r0 = 0; r0 < R; r0 += LM_RC) {
    const int rn = R - r0 < LM_RC ? R - r0 : LM_RC;
    // A tile: rn x 128 floats, 16 bytes per thread and trip (K % 8 == 0: a 4-column piece is inside the row or outside it)
    for (int idx = tid; idx < rn * (LM_COLS / 4); idx += LM_THREADS) {
      const int r = idx / (LM_COLS / 4), c = (idx % (LM_COLS / 4)) * 4;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (k0 + c < K) v = *(const float4*)(A + (int64_t)(r0 + r) * K + k0 + c);
      *(float4*)&sA[r][c] = v;
    }
    // t tile: 64 rows x rn, stored rank-major so that a thread reads its four rows in one piece
    for (int idx = tid; idx < LM_ROWS * LM_RC; idx += LM_THREADS) {
      const int r = idx % LM_RC, row = idx / LM_RC;
      if (r < rn) {
        double t = 0.0;
        if (n0 + row < N) t = (double)scale[r0 + r] * (double)B[(int64_t)(n0 + row) * R + r0 + r];
        sT[r][row] = t;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < rn; ++r) {
      const float4 a0 = *(const float4*)&sA[r][cg * 8], a1 = *(const float4*)&sA[r][cg * 8 + 4];
      const double2 t01 = *(const double2*)&sT[r][rg * 4], t23 = *(const double2*)&sT[r][rg * 4 + 2];
      const double a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const double t[4] = {t01.x, t01.y, t23.x, t23.y};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = fma(t[i], a[j], acc[i][j]);
    }
    __syncthreads();
  }

  const int k = k0 + cg * 8;
  if (k >= K) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + rg * 4 + i;
    if (n >= N) break;
    float w[8];
    lm_load8<WT>(W + (int64_t)n * ldw + k, w);
    uint4 o;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lm_round_to_odd((double)w[j] + acc[i][j]);
    o.x = pack_bf2(v[0], v[1]);
    o.y = pack_bf2(v[2], v[3]);
    o.z = pack_bf2(v[4], v[5]);
    o.w = pack_bf2(v[6], v[7]);
    *(uint4*)(out + (int64_t)n * ldo + k) = o;
  }
}

// the refusals, each written once, in a fixed order: shape first (a validate-only call passes null pointers), then pointers
static int lora_merge_check(const LoraMergeArgs& a) {
  if (a.N < 0 || a.K <= 0) {
    set_error("alg_lora_merge: bad shape N=%d K=%d", a.N, a.K);
    return ALG_EINVAL;
  }
  if (a.R < 1 || a.R > LM_MAX_R) {
    set_error("alg_lora_merge: R=%d must be in 1..%d (the combined rank of all adapters of one weight)", a.R, LM_MAX_R);
    return ALG_EINVAL;
  }
  if (a.K % 8) {
    set_error("alg_lora_merge: K=%d must be a multiple of 8 (bf16 rows move in 16-byte pieces)", a.K);
    return ALG_EINVAL;
  }
  if (a.w_dtype != ALG_F32 && a.w_dtype != ALG_BF16) {
    set_error("alg_lora_merge: unknown base dtype %d (ALG_F32 or ALG_BF16)", a.w_dtype);
    return ALG_EINVAL;
  }
  if (a.ldw < a.K || a.ldo < a.K) {
    set_error("alg_lora_merge: leading dimensions ldw=%lld ldo=%lld must be at least K=%d", (long long)a.ldw, (long long)a.ldo, a.K);
    return ALG_EINVAL;
  }
  if (a.ldo % 8 || a.ldw % (a.w_dtype == ALG_BF16 ? 8 : 4)) {
    set_error("alg_lora_merge: leading dimensions ldw=%lld ldo=%lld must be multiples of 16 bytes", (long long)a.ldw,
              (long long)a.ldo);
    return ALG_EINVAL;
  }
  if (!a.W || !a.A || !a.B || !a.scale || !a.out) {
    set_error("alg_lora_merge: null pointer");
    return ALG_EINVAL;
  }
  if (((uintptr_t)a.W | (uintptr_t)a.A | (uintptr_t)a.out) & 15 || ((uintptr_t)a.B | (uintptr_t)a.scale) & 3) {
    set_error("alg_lora_merge: W, A and out must be 16-byte aligned, B and scale 4-byte aligned");
    return ALG_EINVAL;
  }
  if (a.N == 0) return ALG_OK;
  // out may be W itself (bf16, same leading dimension); any other overlap is refused
  const int64_t wsize = a.w_dtype == ALG_BF16 ? 2 : 4;
  const uintptr_t w0 = (uintptr_t)a.W, w1 = w0 + (uintptr_t)(((int64_t)(a.N - 1) * a.ldw + a.K) * wsize);
  const uintptr_t o0 = (uintptr_t)a.out, o1 = o0 + (uintptr_t)(((int64_t)(a.N - 1) * a.ldo + a.K) * 2);
  if (w0 < o1 && o0 < w1 && !(w0 == o0 && a.w_dtype == ALG_BF16 && a.ldw == a.ldo)) {
    set_error("alg_lora_merge: out may alias W only as the same bf16 buffer with ldw == ldo (an fp32 base is merged out of place)");
    return ALG_EINVAL;
  }
  return ALG_OK;
}

static int lora_merge_plan(const LoraMergeArgs& a, LoraMergePlan* pl) {
  pl->col_tiles = (a.K + LM_COLS - 1) / LM_COLS;
  pl->blocks = (int64_t)pl->col_tiles * ((a.N + LM_ROWS - 1) / LM_ROWS);
  if (pl->blocks > 0x7fffffff) {
    set_error("alg_lora_merge: N=%d K=%d is more than one launch covers", a.N, a.K);
    return ALG_ELIMIT;
  }
  return ALG_OK;
}

}  // namespace alg

using namespace alg;

extern "C" int alg_lora_merge(const void* W, int w_dtype, int64_t ldw, const float* A, const float* B, const float* scale,
                              void* out, int64_t ldo, int N, int K, int R, void* stream) {
  const LoraMergeArgs a = {W, w_dtype, ldw, A, B, scale, out, ldo, N, K, R};
  int rc = lora_merge_check(a);
  if (rc != ALG_OK) return rc;
  if (N == 0) return ALG_OK;
  LoraMergePlan pl;
  rc = lora_merge_plan(a, &pl);
  if (rc != ALG_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (w_dtype == ALG_BF16)
    hipLaunchKernelGGL(lora_merge_kernel<bf16_t>, dim3((unsigned)pl.blocks), dim3(LM_THREADS), 0, s, (const bf16_t*)W, ldw, A, B,
                       scale, (bf16_t*)out, ldo, N, K, R, pl.col_tiles);
  else
    hipLaunchKernelGGL(lora_merge_kernel<float>, dim3((unsigned)pl.blocks), dim3(LM_THREADS), 0, s, (const float*)W, ldw, A, B,
                       scale, (bf16_t*)out, ldo, N, K, R, pl.col_tiles);
  return check_launch("alg_lora_merge");
}
