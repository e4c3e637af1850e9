// bf16 ping-pong GEMM with convolution addressing of the A operand (see gemm_kernel.h, CONV): plain and residual epilogues.
#include "gemm_kernel.h"

namespace alg {
int launch_gemm_p6_conv(const alg_gemm_args* a, int m_tiles, int n_tiles, int64_t nwg, hipStream_t s) {
  static PerDeviceOnce attr_set;
  const int rc = opt_in_lds(attr_set,
                            {(const void*)gemm_bf16_kernel<ALG_ACT_NONE, true, 6, 4, false, true>,
                             (const void*)gemm_bf16_kernel<ALG_ACT_NONE, false, 6, 4, false, true>},
                            GEMM_LDS, "alg_conv_cl_bf16");
  if (rc != ALG_OK) return rc;
  const dim3 grid(gemm_grid(nwg)), block(512);
  const int gm = gemm_group_m(6);
  if (a->R)
    hipLaunchKernelGGL((gemm_bf16_kernel<ALG_ACT_NONE, true, 6, 4, false, true>), grid, block, GEMM_LDS, s, *a, m_tiles,
                       n_tiles, gm, GemmNoPair{});
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<ALG_ACT_NONE, false, 6, 4, false, true>), grid, block, GEMM_LDS, s, *a, m_tiles,
                       n_tiles, gm, GemmNoPair{});
  return check_launch("alg_conv_cl_bf16");
}
}  // namespace alg
