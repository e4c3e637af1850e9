// Step cache ("first-block cache") probe: ONE pass over one sample's hidden state behind block 0 of a DiT.
//   x0 = hidden state in front of block 0 (the caller's copy, `keep`), x1 = behind it, r_prev = the residual of the last forward
//   r        = bf16_rne(float(x1) - float(x0))                                       all rows
//   a       += |float(r) - float(r_prev)|,  b += |float(r_prev)|                     token rows [tok0, tok0 + tok_rows) only
//   r_prev  <- r  (in place: the thread that read an element writes it),  keep <- x1 (the copy the tail needs)
// HBM-bound: three reads and two writes of rows * D bf16, 16 bytes per lane and access.
//
// The sums are deterministic and do not depend on how the grid is scheduled: the grid is a function of the shape alone, a
// thread adds the eight terms of a vector in fp32 (a chain of 8) and everything above that in double in a fixed order -- lanes
// by shuffle, the waves of a block through LDS, one partial pair per block into the caller's workspace, and a second launch of
// one block sums the workspace.  No atomics.
#include "common.h"
#include "row_ops.h"

namespace alg {

constexpr int SC_THREADS = 256;
constexpr int64_t SC_MAX_BLOCKS = 2048;   // 8 resident blocks on each of 256 compute units; a constant: the sums are the same on any device

inline int64_t sc_blocks(int64_t nvec) {
  const int64_t want = (nvec + SC_THREADS - 1) / SC_THREADS;
  return want < 1 ? 1 : (want > SC_MAX_BLOCKS ? SC_MAX_BLOCKS : want);
}

// one 8-element vector: returns r packed, adds this vector's terms (fp32, chain of 8) to the double accumulators
__device__ __forceinline__ uint4 probe8(const uint4 vx0, const uint4 vx1, const uint4 vrp, bool counted, double& a, double& b) {
  float x0[8], x1[8], rp[8], r[8];
  unpack8(vx0, x0);
  unpack8(vx1, x1);
  unpack8(vrp, rp);
  float sa = 0.0f, sb = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    r[k] = rbf(__fsub_rn(x1[k], x0[k]));
    sa = __fadd_rn(sa, fabsf(__fsub_rn(r[k], rp[k])));
    sb = __fadd_rn(sb, fabsf(rp[k]));
  }
  if (counted) {
    a += (double)sa;
    b += (double)sb;
  }
  uint4 o;
  o.x = pack_bf2(r[0], r[1]); o.y = pack_bf2(r[2], r[3]); o.z = pack_bf2(r[4], r[5]); o.w = pack_bf2(r[6], r[7]);
  return o;
}

// keep / x1 / r are three distinct buffers (the launcher's contract), each element is read and written by one thread
__global__ __launch_bounds__(SC_THREADS) void step_cache_probe_kernel(uint4* __restrict__ keep, const uint4* __restrict__ x1,
                                                                      uint4* __restrict__ r, int64_t nvec, int64_t v0, int64_t v1,
                                                                      double* __restrict__ partial) {
  const int64_t stride = (int64_t)gridDim.x * SC_THREADS;
  double a = 0.0, b = 0.0;
  // two vectors per trip: six 16-byte loads in flight per lane before the first store
  for (int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; i < nvec; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < nvec;
    const uint4 k0 = keep[i], y0 = x1[i], p0 = r[i];
    uint4 k1 = k0, y1 = y0, p1 = p0;
    if (two) {
      k1 = keep[j];
      y1 = x1[j];
      p1 = r[j];
    }
    r[i] = probe8(k0, y0, p0, i >= v0 && i < v1, a, b);
    keep[i] = y0;
    if (two) {
      r[j] = probe8(k1, y1, p1, j >= v0 && j < v1, a, b);
      keep[j] = y1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  __shared__ double wa[SC_THREADS / 64], wb[SC_THREADS / 64];
  if ((threadIdx.x & 63) == 0) {
    wa[threadIdx.x >> 6] = a;
    wb[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = wa[0], sb = wb[0];
#pragma unroll
    for (int w = 1; w < SC_THREADS / 64; ++w) {
      sa += wa[w];
      sb += wb[w];
    }
    partial[2 * blockIdx.x] = sa;
    partial[2 * blockIdx.x + 1] = sb;
  }
}

// sums[0..1] = the partial pairs of `blocks` workgroups, added in a fixed order in double (blocks == 0: zeros)
__global__ __launch_bounds__(SC_THREADS) void step_cache_sum_kernel(const double* __restrict__ partial, int blocks,
                                                                    double* __restrict__ sums) {
  __shared__ double sa[SC_THREADS], sb[SC_THREADS];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < blocks; i += SC_THREADS) {
    a += partial[2 * i];
    b += partial[2 * i + 1];
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int w = SC_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sa[threadIdx.x] += sa[threadIdx.x + w];
      sb[threadIdx.x] += sb[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[0] = sa[0];
    sums[1] = sb[0];
  }
}

}  // namespace alg

using namespace alg;

extern "C" int64_t alg_step_cache_workspace_bytes(int rows, int D) {
  if (rows < 0 || D <= 0 || D % 8) {
    set_error("alg_step_cache_workspace_bytes: bad argument (rows=%d D=%d; D must be a positive multiple of 8)", rows, D);
    return ALG_EINVAL;
  }
  return sc_blocks((int64_t)rows * D / 8) * 2 * (int64_t)sizeof(double);
}

extern "C" int alg_step_cache_probe(void* keep, const void* x1, void* r, int rows, int D, int tok0, int tok_rows,
                                    void* workspace, double* sums, void* stream) {
  if (!keep || !x1 || !r || !workspace || !sums) {
    set_error("alg_step_cache_probe: null pointer");
    return ALG_EINVAL;
  }
  if (rows < 0 || D <= 0 || D % 8) {
    set_error("alg_step_cache_probe: bad argument (rows=%d D=%d; D must be a positive multiple of 8)", rows, D);
    return ALG_EINVAL;
  }
  if (tok0 < 0 || tok_rows < 0 || (int64_t)tok0 + tok_rows > rows) {
    set_error("alg_step_cache_probe: token rows [%d, %d + %d) leave the %d rows of the sample", tok0, tok0, tok_rows, rows);
    return ALG_EINVAL;
  }
  if (((uintptr_t)keep | (uintptr_t)x1 | (uintptr_t)r) & 15 || ((uintptr_t)workspace | (uintptr_t)sums) & 7) {
    set_error("alg_step_cache_probe: keep, x1 and r must be 16-byte aligned, workspace and sums 8-byte aligned");
    return ALG_EINVAL;
  }
  if (keep == x1 || keep == r || x1 == r) {
    set_error("alg_step_cache_probe: keep, x1 and r must be three distinct buffers");
    return ALG_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t vrow = D / 8, nvec = (int64_t)rows * vrow;
  int blocks = 0;
  if (nvec > 0) {
    blocks = (int)sc_blocks(nvec);
    hipLaunchKernelGGL(step_cache_probe_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, s, (uint4*)keep, (const uint4*)x1,
                       (uint4*)r, nvec, (int64_t)tok0 * vrow, ((int64_t)tok0 + tok_rows) * vrow, (double*)workspace);
  }
  hipLaunchKernelGGL(step_cache_sum_kernel, dim3(1), dim3(SC_THREADS), 0, s, (const double*)workspace, blocks, sums);
  return check_launch("alg_step_cache_probe");
}
