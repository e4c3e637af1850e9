// Pooled far-field attention (alg_amd/attn_pool.py): the keys outside the frame window are attended to at 1 / G of their
// resolution -- every group of G consecutive keys, aligned to G on the absolute key index, becomes ONE pooled key bf16(mean k) with
// the pooled value bf16(mean v), and the far launch's log-sum-exp is shifted by log2 G so that a pooled key weighs as G keys.
//   alg_attn_pool_k           K rows [S][row stride] -> [S / G] pooled rows, rows up to the next multiple of 64 zero
//   alg_attn_pool_vt          V^T [rows][S padded to 64] -> [rows][S / G padded to 64] along the key axis, the attention kernels'
//                             column permutation (index bits 2 and 3 swapped: perm23 of attn_layout.hip) on both sides
//   alg_attn_merge_lse_shift  alg_attn_merge_lse (attn_far.hip) with a shift added to the far log-sum-exp
// The mean: an fp32 sum over the G rows in ascending key order, the exact scale 1 / G (G is a power of two), ONE rounding to
// bf16.  Both pooling kernels are memory-bound and written that way: 16-byte accesses on both sides, a capped grid with a
// grid-stride loop, every output element a function of its own operands alone.  No atomics, no LDS, no scratch.
#include "common.h"
#include "row_ops.h"

namespace alg {

// attn_far.hip
int merge_lse_entry(const char* what, void* o, const float* lse, const void* o_far, const float* lse_far, int batch, int heads,
                    int head_dim, int Sq, int64_t o_bstride, int64_t o_rstride, int64_t far_bstride, int64_t far_rstride,
                    float far_shift, float* lse_out, void* stream);

namespace pool {

constexpr int THREADS = 256;

// ---- K rows ------------------------------------------------------------------------------------------------------------------
// One item = 16 bytes (8 bf16) of one destination row: v = ((b * P_pad + p) * vpr + c), consecutive lanes walk a row.
template <int G>
__global__ __launch_bounds__(THREADS) void k_kernel(const uint4* __restrict__ src, int64_t src_bvs, int64_t src_rvs,
                                                    uint4* __restrict__ dst, int64_t dst_bvs, int64_t dst_rvs, int P, int P_pad,
                                                    int vpr, int64_t nvec) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < nvec; v += stride) {
    const int c = (int)(v % vpr);
    const int64_t t = v / vpr;
    const int p = (int)(t % P_pad);
    const int64_t b = t / P_pad;
    uint4 out = make_uint4(0, 0, 0, 0);          // rows [P, P_pad): padding
    if (p < P) {
      const uint4* s = src + b * src_bvs + (int64_t)p * G * src_rvs + c;
      float acc[8], x[8];
      unpack8(s[0], acc);
#pragma unroll
      for (int g = 1; g < G; ++g) {
        unpack8(s[g * src_rvs], x);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += x[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] *= 1.0f / G;
      out = pack8(acc);
    }
    dst[b * dst_bvs + (int64_t)p * dst_rvs + c] = out;
  }
}

// ---- V^T ---------------------------------------------------------------------------------------------------------------------
// One item = one 16-column block of one destination row (two 16-byte stores): its pooled keys 16 kb .. 16 kb + 15 are the means
// of the source keys [16 kb G, 16 (kb + 1) G), G source blocks of 16 columns (two 16-byte loads each).  Inside a block of 16 the
// storage chunk 0 holds the keys {0..3, 8..11} and chunk 1 the keys {4..7, 12..15}, source and destination alike.  A source
// block is read only if it begins below P * G (then it lies inside S rounded up to 16, inside the source pitch); what it holds
// behind P * G feeds pooled keys >= P only, and those are written as zero whatever was read.
template <int G>
__global__ __launch_bounds__(THREADS) void vt_kernel(const bf16_t* __restrict__ src, int64_t src_bs, int64_t src_rs,
                                                     bf16_t* __restrict__ dst, int64_t dst_bs, int64_t dst_rs, int rows, int P,
                                                     int blocks, int64_t items) {
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < items; i += stride) {
    const int kb = (int)(i % blocks);
    const int64_t t = i / blocks;
    const int r = (int)(t % rows);
    const int64_t b = t / rows;
    const bf16_t* const s_row = src + b * src_bs + (int64_t)r * src_rs;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int key0 = (kb * G + j) * 16;
      if (key0 >= P * G) continue;
      float c0[8], c1[8], l[16];
      unpack8(*(const uint4*)(s_row + key0), c0);
      unpack8(*(const uint4*)(s_row + key0 + 8), c1);
#pragma unroll
      for (int k = 0; k < 4; ++k) l[k] = c0[k], l[8 + k] = c0[4 + k], l[4 + k] = c1[k], l[12 + k] = c1[4 + k];
#pragma unroll
      for (int k = 0; k < 16; ++k) {   // ascending key order inside every group, the sum seeded by the group's first key (as in
        if ((16 * j + k) % G == 0) acc[(16 * j + k) / G] = l[k];   // k_kernel: a group of -0.0 pools to -0.0)
        else acc[(16 * j + k) / G] += l[k];
      }
    }
    float o0[8], o1[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = kb * 16 + k < P ? acc[k] * (1.0f / G) : 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) o0[k] = acc[k], o0[4 + k] = acc[8 + k], o1[k] = acc[4 + k], o1[4 + k] = acc[12 + k];
    bf16_t* const d = dst + b * dst_bs + (int64_t)r * dst_rs + kb * 16;
    *(uint4*)d = pack8(o0);
    *(uint4*)(d + 8) = pack8(o1);
  }
}

static bool group_ok(int G) { return G == 2 || G == 4 || G == 8; }

}  // namespace pool
}  // namespace alg

using namespace alg;

extern "C" int alg_attn_pool_k(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst, int64_t dst_bstride,
                               int64_t dst_rstride, int batch, int heads, int head_dim, int S, int group, void* stream) {
  if (!src || !dst || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) {
    set_error("alg_attn_pool_k: src / dst must be 16-byte aligned device pointers");
    return ALG_EINVAL;
  }
  if (batch < 1 || heads < 1 || (head_dim != 64 && head_dim != 128) || !pool::group_ok(group) || S < group) {
    set_error("alg_attn_pool_k: bad argument (batch=%d heads=%d head_dim=%d S=%d group=%d: head_dim is 64 or 128, group 2, 4 or 8, "
              "S holds at least one group)", batch, heads, head_dim, S, group);
    return ALG_EINVAL;
  }
  const int64_t row = (int64_t)heads * head_dim;
  const int P = S / group, P_pad = (P + 63) & ~63;
  if (src_rstride < row || dst_rstride < row || (src_rstride & 7) || (dst_rstride & 7) || (src_bstride & 7) || (dst_bstride & 7) ||
      src_bstride < 0 || dst_bstride < 0 ||
      (batch > 1 && (src_bstride < (int64_t)(S - 1) * src_rstride + row || dst_bstride < (int64_t)(P_pad - 1) * dst_rstride + row))) {
    set_error("alg_attn_pool_k: bad strides (src %lld / %lld, dst %lld / %lld: multiples of 8 elements, a row stride >= heads * "
              "head_dim = %lld, batch strides that hold S = %d source rows and S / group rounded up to 64 = %d pooled rows)",
              (long long)src_bstride, (long long)src_rstride, (long long)dst_bstride, (long long)dst_rstride, (long long)row, S, P_pad);
    return ALG_EINVAL;
  }
  const int vpr = (int)(row / 8);
  const int64_t nvec = (int64_t)batch * P_pad * vpr;
  const dim3 grid(grid_for(nvec)), block(pool::THREADS);
  hipStream_t s = (hipStream_t)stream;
#define ALG_POOL_K(G_)                                                                                                            \
  hipLaunchKernelGGL(pool::k_kernel<G_>, grid, block, 0, s, (const uint4*)src, src_bstride / 8, src_rstride / 8, (uint4*)dst,      \
                     dst_bstride / 8, dst_rstride / 8, P, P_pad, vpr, nvec)
  if (group == 2) ALG_POOL_K(2);
  else if (group == 4) ALG_POOL_K(4);
  else ALG_POOL_K(8);
#undef ALG_POOL_K
  return check_launch("alg_attn_pool_k");
}

extern "C" int alg_attn_pool_vt(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst, int64_t dst_bstride,
                                int64_t dst_rstride, int batch, int heads, int head_dim, int S, int group, void* stream) {
  if (!src || !dst || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) {
    set_error("alg_attn_pool_vt: src / dst must be 16-byte aligned device pointers");
    return ALG_EINVAL;
  }
  if (batch < 1 || heads < 1 || (head_dim != 64 && head_dim != 128) || !pool::group_ok(group) || S < group) {
    set_error("alg_attn_pool_vt: bad argument (batch=%d heads=%d head_dim=%d S=%d group=%d: head_dim is 64 or 128, group 2, 4 or 8, "
              "S holds at least one group)", batch, heads, head_dim, S, group);
    return ALG_EINVAL;
  }
  const int64_t rows = (int64_t)heads * head_dim, S_pad = ((int64_t)S + 63) & ~63LL;
  const int P = S / group, P_pad = (P + 63) & ~63;
  if (rows > 0x7fffffffLL) {
    set_error("alg_attn_pool_vt: heads * head_dim = %lld is beyond what one launch addresses", (long long)rows);
    return ALG_ELIMIT;
  }
  if (src_rstride < S_pad || dst_rstride < P_pad || (src_rstride & 7) || (dst_rstride & 7) || (src_bstride & 7) || (dst_bstride & 7) ||
      src_bstride < 0 || dst_bstride < 0 || (batch > 1 && (src_bstride < rows * src_rstride || dst_bstride < rows * dst_rstride))) {
    set_error("alg_attn_pool_vt: bad strides (src %lld / %lld, dst %lld / %lld: multiples of 8 elements, a source row stride >= S "
              "rounded up to 64 = %lld, a destination row stride >= S / group rounded up to 64 = %d, batch strides that hold heads * "
              "head_dim rows)", (long long)src_bstride, (long long)src_rstride, (long long)dst_bstride, (long long)dst_rstride,
              (long long)S_pad, P_pad);
    return ALG_EINVAL;
  }
  const int blocks = P_pad / 16;
  const int64_t items = (int64_t)batch * rows * blocks;
  const dim3 grid(grid_for(items)), block(pool::THREADS);
  hipStream_t s = (hipStream_t)stream;
#define ALG_POOL_VT(G_)                                                                                                           \
  hipLaunchKernelGGL(pool::vt_kernel<G_>, grid, block, 0, s, (const bf16_t*)src, src_bstride, src_rstride, (bf16_t*)dst,           \
                     dst_bstride, dst_rstride, (int)rows, P, blocks, items)
  if (group == 2) ALG_POOL_VT(2);
  else if (group == 4) ALG_POOL_VT(4);
  else ALG_POOL_VT(8);
#undef ALG_POOL_VT
  return check_launch("alg_attn_pool_vt");
}

extern "C" int alg_attn_merge_lse_shift(void* o, const float* lse, const void* o_far, const float* lse_far, int batch, int heads,
                                        int head_dim, int Sq, int64_t o_bstride, int64_t o_rstride, int64_t far_bstride,
                                        int64_t far_rstride, float far_lse_shift, float* lse_out, void* stream) {
  if (!(far_lse_shift == far_lse_shift) || far_lse_shift - far_lse_shift != 0.0f) {
    set_error("alg_attn_merge_lse_shift: far_lse_shift must be finite");
    return ALG_EINVAL;
  }
  return merge_lse_entry("alg_attn_merge_lse_shift", o, lse, o_far, lse_far, batch, heads, head_dim, Sq, o_bstride, o_rstride,
                         far_bstride, far_rstride, far_lse_shift, lse_out, stream);
}
