// Layout moves for the position-major band attention (alg_amd/attn_window.py: position_band_ranges): the selected heads of Q, K
// and O between the frame-major token order s = f * HW + p and the position-major order pi(s) = p * F + f
// (alg_attn_rows_position_major), and the same reordering of V^T's key axis (alg_attn_vt_position_major).  Pure moves: no
// arithmetic, every value keeps its bits.  Both are memory-bound and written that way: 16-byte global accesses on both sides, a
// grid capped at a few resident rounds with a grid-stride loop, no atomics.
#include "common.h"

namespace alg {
namespace layout {

constexpr int THREADS = 256;
constexpr int BLOCKS_PER_CU = 8;

// ---- rows ------------------------------------------------------------------------------------------------------------------
// One item = 16 bytes (8 bf16) of one head slice of one row; items are numbered in the order of the DESTINATION (row, head slot,
// chunk), so a wave writes whole head slices (128 or 256 contiguous bytes) of consecutive rows and reads whole head slices.
// wide: the [rows][all heads] tensor, head slice at head_list[j] * hd; compact: [rows][n_sel heads], head slice at j * hd.
__global__ __launch_bounds__(THREADS) void rows_kernel(const bf16_t* __restrict__ src, int64_t src_bs, int64_t src_rs,
                                                       bf16_t* __restrict__ dst, int64_t dst_bs, int64_t dst_rs,
                                                       const int32_t* __restrict__ head_list, int n_sel, int hd_log2, int frames,
                                                       int hw, int inverse, int64_t items) {
  const int S = frames * hw;
  const int cpr_log2 = hd_log2 - 3;                      // 16-byte chunks per head slice: 8 or 16
  const int64_t per_batch = ((int64_t)S * n_sel) << cpr_log2;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * THREADS) {
    const int b = (int)(i / per_batch);
    const uint32_t r = (uint32_t)(i - (int64_t)b * per_batch);     // < S * n_sel * 16 <= 2^31 (checked on the host)
    const int c = (int)(r & ((1u << cpr_log2) - 1));
    const uint32_t t = r >> cpr_log2;
    const int row = (int)(t / (uint32_t)n_sel), j = (int)(t - (uint32_t)row * (uint32_t)n_sel);
    const int head = head_list[j];
    int64_t so, d_o;
    if (!inverse) {   // row is pi(s) = p * F + f: the compact destination's row; the source row is s = f * HW + p
      const int p = row / frames, f = row - p * frames;
      so = (int64_t)b * src_bs + (int64_t)(f * hw + p) * src_rs + ((int64_t)head << hd_log2);
      d_o = (int64_t)b * dst_bs + (int64_t)row * dst_rs + ((int64_t)j << hd_log2);
    } else {          // row is s: the wide destination's row; the source row is pi(s)
      const int f = row / hw, p = row - f * hw;
      so = (int64_t)b * src_bs + (int64_t)(p * frames + f) * src_rs + ((int64_t)j << hd_log2);
      d_o = (int64_t)b * dst_bs + (int64_t)row * dst_rs + ((int64_t)head << hd_log2);
    }
    *(uint4*)(dst + d_o + c * 8) = *(const uint4*)(src + so + c * 8);
  }
}

// ---- V^T -------------------------------------------------------------------------------------------------------------------
// Per (batch, selected row) the key axis is an [F][HW] matrix transposed to [HW][F], with the attention kernels' column
// permutation (index bits 2 and 3 swapped) on both sides.  One task = TILE consecutive destination columns of one row, built in
// LDS in LOGICAL destination order: the source columns that land in the tile are, per frame f, one run of positions
// [pa, pb], read as aligned 16-byte chunks (coalesced along the run) and scattered into the tile element by element; the tile
// then leaves as 16-byte chunks in storage order.  The LDS size does not depend on F or HW.  The element scatter
// (ds_write_b16, lane stride 8 F elements) has bank conflicts; it stays under the time the 2 x 16 KiB of HBM traffic per task
// take (profiles/attn_layout_resources.txt).
constexpr int TILE = 8192;                               // destination columns per task: 16 KiB of LDS, a multiple of 64

__device__ __forceinline__ int perm23(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

__global__ __launch_bounds__(THREADS) void vt_kernel(const bf16_t* __restrict__ src, int64_t src_bs, int64_t src_rs,
                                                     bf16_t* __restrict__ dst, int64_t dst_bs, int64_t dst_rs,
                                                     const int32_t* __restrict__ head_list, int n_sel, int hd_log2, int frames,
                                                     int hw, int tiles, int64_t tasks) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[TILE];
  const int S = frames * hw, S_pad = (S + 63) & ~63;
  const int rows = n_sel << hd_log2;
  for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
    const int t = (int)(task % tiles);
    const int64_t br = task / tiles;
    const int row = (int)(br % rows), b = (int)(br / rows);
    const int j = row >> hd_log2;
    const bf16_t* const s_row = src + (int64_t)b * src_bs + (((int64_t)head_list[j] << hd_log2) + (row & ((1 << hd_log2) - 1))) * src_rs;
    bf16_t* const d_row = dst + (int64_t)b * dst_bs + (int64_t)row * dst_rs;
    const int L0 = t * TILE;                              // the tile holds the destination columns [L0, L0 + width)
    const int width = min(TILE, S_pad - L0);
    const int L1 = min(L0 + width, S);                    // ... of which [L0, L1) carry keys, the rest is padding: zero
    if (L1 < L0 + width) {
      for (int x = (int)threadIdx.x * 8; x < width; x += THREADS * 8) *(uint4*)(tile + x) = make_uint4(0, 0, 0, 0);
      __syncthreads();
    }
    if (L1 > L0) {
      const int pa = L0 / frames, pb = (L1 - 1) / frames;             // the positions whose keys land in [L0, L1)
      const int nch = 2 * (((pb - pa) >> 4) + 2);                      // 16-byte chunks per frame: covers any alignment of the run
      const int n_items = frames * nch;
      for (int i = (int)threadIdx.x; i < n_items; i += THREADS) {
        const int f = i / nch, c = i - f * nch;
        const int lo = f * hw + pa, hi = f * hw + pb;                  // logical source columns of frame f, inclusive
        const int col0 = ((lo >> 4) << 4) + c * 8;                     // storage column of this chunk
        if (col0 > (hi | 15)) continue;                                // behind the run's last 16-column block
        const uint4 v = *(const uint4*)(s_row + col0);                 // col0 + 7 <= hi | 15 < S rounded up to 16 <= src_rs
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int s = perm23(col0 + e);                              // the key this storage column holds
          if (s < lo || s > hi) continue;
          const int at = (s - f * hw) * frames + f - L0;               // its destination column pi(s), relative to the tile
          if (at >= 0 && at < L1 - L0) tile[at] = (bf16_t)(w[e >> 1] >> ((e & 1) * 16));
        }
      }
    }
    __syncthreads();
    // out: storage chunk m of the tile = the logical columns 16 k + {0..3, 8..11} (m even) or 16 k + {4..7, 12..15} (m odd)
    for (int m = (int)threadIdx.x; m < width / 8; m += THREADS) {
      const int base = (m >> 1) * 16 + (m & 1) * 4;
      const uint2 a = *(const uint2*)(tile + base), c2 = *(const uint2*)(tile + base + 8);
      *(uint4*)(d_row + L0 + m * 8) = make_uint4(a.x, a.y, c2.x, c2.y);
    }
    __syncthreads();
  }
}

static int hd_log2_of(int head_dim) { return head_dim == 64 ? 6 : head_dim == 128 ? 7 : -1; }

static unsigned capped_grid(int64_t blocks) {
  const int64_t cap = (int64_t)device_cus() * BLOCKS_PER_CU;
  return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace layout
}  // namespace alg

using namespace alg;

extern "C" int alg_attn_rows_position_major(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst,
                                            int64_t dst_bstride, int64_t dst_rstride, const int32_t* head_list, int n_sel,
                                            int head_dim, int batch, int frames, int hw, int inverse, void* stream) {
  const int hl2 = layout::hd_log2_of(head_dim);
  if (!src || !dst || !head_list || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)head_list & 3)) {
    set_error("alg_attn_rows_position_major: src / dst must be 16-byte and head_list 4-byte aligned device pointers");
    return ALG_EINVAL;
  }
  if (hl2 < 0 || n_sel < 1 || batch < 1 || frames < 1 || hw < 1 || (inverse != 0 && inverse != 1)) {
    set_error("alg_attn_rows_position_major: bad argument (head_dim=%d n_sel=%d batch=%d frames=%d hw=%d inverse=%d: head_dim is 64 "
              "or 128, the counts are >= 1, inverse is 0 or 1)", head_dim, n_sel, batch, frames, hw, inverse);
    return ALG_EINVAL;
  }
  const int64_t S = (int64_t)frames * hw, slice = (int64_t)n_sel * head_dim;
  if (S * n_sel * 16 > 0x7fffffffLL) {
    set_error("alg_attn_rows_position_major: frames * hw * n_sel = %lld is beyond what one launch addresses", (long long)(S * n_sel));
    return ALG_ELIMIT;
  }
  if (src_rstride < slice || dst_rstride < slice || (src_rstride & 7) || (dst_rstride & 7) || (src_bstride & 7) || (dst_bstride & 7) ||
      (batch > 1 && (src_bstride < (S - 1) * src_rstride + slice || dst_bstride < (S - 1) * dst_rstride + slice))) {
    set_error("alg_attn_rows_position_major: bad strides (src %lld / %lld, dst %lld / %lld: multiples of 8 elements, a row stride "
              ">= n_sel * head_dim = %lld, a batch stride that holds frames * hw rows)", (long long)src_bstride,
              (long long)src_rstride, (long long)dst_bstride, (long long)dst_rstride, (long long)slice);
    return ALG_EINVAL;
  }
  const int64_t items = (int64_t)batch * S * n_sel * (head_dim / 8);
  const unsigned grid = layout::capped_grid((items + layout::THREADS - 1) / layout::THREADS);
  hipLaunchKernelGGL(layout::rows_kernel, dim3(grid), dim3(layout::THREADS), 0, (hipStream_t)stream, (const bf16_t*)src, src_bstride,
                     src_rstride, (bf16_t*)dst, dst_bstride, dst_rstride, head_list, n_sel, hl2, frames, hw, inverse, items);
  return check_launch("alg_attn_rows_position_major");
}

extern "C" int alg_attn_vt_position_major(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst,
                                          int64_t dst_bstride, int64_t dst_rstride, const int32_t* head_list, int n_sel,
                                          int head_dim, int batch, int frames, int hw, void* stream) {
  const int hl2 = layout::hd_log2_of(head_dim);
  if (!src || !dst || !head_list || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)head_list & 3)) {
    set_error("alg_attn_vt_position_major: src / dst must be 16-byte and head_list 4-byte aligned device pointers");
    return ALG_EINVAL;
  }
  if (hl2 < 0 || n_sel < 1 || batch < 1 || frames < 1 || hw < 1) {
    set_error("alg_attn_vt_position_major: bad argument (head_dim=%d n_sel=%d batch=%d frames=%d hw=%d: head_dim is 64 or 128, the "
              "counts are >= 1)", head_dim, n_sel, batch, frames, hw);
    return ALG_EINVAL;
  }
  const int64_t S = (int64_t)frames * hw, S_pad = (S + 63) & ~63LL, rows = (int64_t)n_sel * head_dim;
  if (S_pad > 0x7fffffffLL - layout::TILE || rows > 0x7fffffffLL) {
    set_error("alg_attn_vt_position_major: frames * hw = %lld is beyond what one launch addresses", (long long)S);
    return ALG_ELIMIT;
  }
  if (src_rstride < S_pad || dst_rstride < S_pad || (src_rstride & 7) || (dst_rstride & 7) || (src_bstride & 7) || (dst_bstride & 7) ||
      (batch > 1 && (src_bstride < rows * src_rstride || dst_bstride < rows * dst_rstride))) {
    set_error("alg_attn_vt_position_major: bad strides (src %lld / %lld, dst %lld / %lld: multiples of 8 elements, a row stride "
              ">= frames * hw rounded up to 64 = %lld, a batch stride that holds n_sel * head_dim rows)", (long long)src_bstride,
              (long long)src_rstride, (long long)dst_bstride, (long long)dst_rstride, (long long)S_pad);
    return ALG_EINVAL;
  }
  const int tiles = (int)((S_pad + layout::TILE - 1) / layout::TILE);
  const int64_t tasks = (int64_t)batch * rows * tiles;
  hipLaunchKernelGGL(layout::vt_kernel, dim3(layout::capped_grid(tasks)), dim3(layout::THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)src, src_bstride, src_rstride, (bf16_t*)dst, dst_bstride, dst_rstride, head_list, n_sel, hl2,
                     frames, hw, tiles, tasks);
  return check_launch("alg_attn_vt_position_major");
}
