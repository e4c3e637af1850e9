// Far-field attention reuse (alg_amd/attn_far.py): two partial attentions over DISJOINT key sets, each with the log2-domain
// log-sum-exp of the keys it visited (what the _ranges_heads entries write), combine into the exact attention over the union.
//   o (the near partial, fresh) and o_far (cached): bf16 [batch][Sq][heads * head_dim], lse / lse_far: fp32 [batch][heads][Sq]
//   a = lse, f = lse_far, m = max(a, f), wa = exp2(a - m), wf = exp2(f - m)
//   o = bf16((wa * o + wf * o_far) / (wa + wf))      fp32, one rounding;   lse_out = m + log2(wa + wf)
// A side that carries no mass (its lse is -inf, or its weight underflows to 0) leaves the other side's BITS: the row of o is not
// written at all, or is a copy of the far row.
// HBM-bound: one 16-byte read of each operand and one 16-byte write per lane and vector; the lanes of one (b, q, head) read the
// same two LSEs.  A capped grid with a grid-stride loop; every output element is a function of its own operands alone, so the
// result does not depend on the grid.  No atomics, no LDS, no scratch.
#include "common.h"
#include "row_ops.h"

namespace alg {

constexpr int AF_THREADS = 256;

template <int HD>
__global__ __launch_bounds__(AF_THREADS) void attn_merge_lse_kernel(uint4* __restrict__ o, const float* __restrict__ lse,
                                                                    const uint4* __restrict__ o_far, const float* __restrict__ lse_far,
                                                                    int heads, int Sq, int64_t nvec, int64_t o_bvs, int64_t o_rvs,
                                                                    int64_t far_bvs, int64_t far_rvs, float* __restrict__ lse_out,
                                                                    float far_shift) {
  constexpr int VPH = HD / 8;   // 16-byte vectors per head
  const int64_t stride = (int64_t)gridDim.x * AF_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * AF_THREADS + threadIdx.x; v < nvec; v += stride) {
    // v = ((b * Sq + q) * heads + h) * VPH + c: consecutive lanes walk a row of o
    const int c = (int)(v % VPH);
    int64_t t = v / VPH;
    const int h = (int)(t % heads);
    t /= heads;
    const int q = (int)(t % Sq);
    const int64_t b = t / Sq;
    const int64_t li = (b * heads + h) * Sq + q;
    // far_shift (alg_attn_merge_lse_shift: every far key stands for 2^far_shift keys); 0 leaves the far LSE's bits
    const float a = lse[li], f = far_shift != 0.0f ? lse_far[li] + far_shift : lse_far[li];
    const float m = fmaxf(a, f);
    float wa = 0.0f, wf = 0.0f;   // both -inf: nothing to merge, o keeps its bits
    if (m != -INFINITY) {
      wa = exp2f(a - m);
      wf = exp2f(f - m);
    }
    if (lse_out != nullptr && c == 0) lse_out[li] = (m == -INFINITY) ? -INFINITY : m + log2f(wa + wf);
    if (wf == 0.0f) continue;     // the far side carries nothing: the row of o is not touched
    const int64_t oi = b * o_bvs + (int64_t)q * o_rvs + h * VPH + c;
    const uint4 vf = o_far[b * far_bvs + (int64_t)q * far_rvs + h * VPH + c];
    if (wa == 0.0f) {             // the near side carries nothing: the far row's bits
      o[oi] = vf;
      continue;
    }
    float x[8], y[8];
    unpack8(o[oi], x);
    unpack8(vf, y);
    const float den = wa + wf;
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (wa * x[k] + wf * y[k]) / den;
    o[oi] = pack8(x);
  }
}

// Both entries run this (alg_attn_merge_lse_shift lives in attn_pool.hip): `what` names the caller in the error text.
int merge_lse_entry(const char* what, void* o, const float* lse, const void* o_far, const float* lse_far, int batch, int heads,
                    int head_dim, int Sq, int64_t o_bstride, int64_t o_rstride, int64_t far_bstride, int64_t far_rstride,
                    float far_shift, float* lse_out, void* stream) {
  if (batch <= 0 || heads <= 0 || Sq <= 0) {
    set_error("%s: bad argument (batch=%d heads=%d Sq=%d must be positive)", what, batch, heads, Sq);
    return ALG_EINVAL;
  }
  if (head_dim != 64 && head_dim != 128) {
    set_error("%s: head_dim=%d (64 or 128)", what, head_dim);
    return ALG_EINVAL;
  }
  const int64_t row = (int64_t)heads * head_dim;
  if (o_rstride < row || far_rstride < row || o_rstride % 8 || far_rstride % 8) {
    set_error("%s: row strides o=%lld far=%lld must be multiples of 8 elements and at least heads * head_dim = %lld", what,
              (long long)o_rstride, (long long)far_rstride, (long long)row);
    return ALG_EINVAL;
  }
  if (o_bstride < 0 || far_bstride < 0 || o_bstride % 8 || far_bstride % 8 ||
      (batch > 1 && (o_bstride < (Sq - 1) * o_rstride + row || far_bstride < (Sq - 1) * far_rstride + row))) {
    set_error("%s: batch strides o=%lld far=%lld must be multiples of 8 elements and hold the Sq=%d rows of a sample", what,
              (long long)o_bstride, (long long)far_bstride, Sq);
    return ALG_EINVAL;
  }
  if (!o || !lse || !o_far || !lse_far) {
    set_error("%s: null pointer", what);
    return ALG_EINVAL;
  }
  if (((uintptr_t)o | (uintptr_t)o_far) & 15 || ((uintptr_t)lse | (uintptr_t)lse_far | (uintptr_t)lse_out) & 3) {
    set_error("%s: o and o_far must be 16-byte aligned, lse, lse_far and lse_out 4-byte aligned", what);
    return ALG_EINVAL;
  }
  const int64_t nvec = (int64_t)batch * Sq * (row / 8);
  const dim3 grid(grid_for(nvec)), block(AF_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (head_dim == 64)
    hipLaunchKernelGGL(attn_merge_lse_kernel<64>, grid, block, 0, s, (uint4*)o, lse, (const uint4*)o_far, lse_far, heads, Sq, nvec,
                       o_bstride / 8, o_rstride / 8, far_bstride / 8, far_rstride / 8, lse_out, far_shift);
  else
    hipLaunchKernelGGL(attn_merge_lse_kernel<128>, grid, block, 0, s, (uint4*)o, lse, (const uint4*)o_far, lse_far, heads, Sq, nvec,
                       o_bstride / 8, o_rstride / 8, far_bstride / 8, far_rstride / 8, lse_out, far_shift);
  return check_launch(what);
}

}  // namespace alg

using namespace alg;

extern "C" int alg_attn_merge_lse(void* o, const float* lse, const void* o_far, const float* lse_far, int batch, int heads,
                                  int head_dim, int Sq, int64_t o_bstride, int64_t o_rstride, int64_t far_bstride,
                                  int64_t far_rstride, float* lse_out, void* stream) {
  return merge_lse_entry("alg_attn_merge_lse", o, lse, o_far, lse_far, batch, heads, head_dim, Sq, o_bstride, o_rstride, far_bstride,
                         far_rstride, 0.0f, lse_out, stream);
}
