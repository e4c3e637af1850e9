// Host path of the row-norm entries (norm.hip: alg_layernorm_modulate, _seg, _fp8, _seg_fp8; wan.hip: alg_layernorm_mod_f32,
// _fp8, alg_rmsnorm_rope, _fp8; hunyuan.hip: alg_headnorm_rope, _fp8).  Each of these entries fills ONE operand struct of its
// family and then runs
//     *_check   -- the family's refusals, each written once, in a fixed order; the entry's name is passed in
//     *_plan    -- the two LayerNorm families (LnModArgs in norm.hip, LnF32Args in wan.hip): which kernel the call runs, with how
//                  many rows per wave and which grid -- a pure function of the shape, of which parameters are there and how
//                  they are aligned, and of the device's CU count
//     launch    -- dispatch_iters picks the instantiation; no launch step decides anything
// What the families share is here: the plan's shape, the limit of one launch, the width dispatch, the failed launch's message,
// and the operands and refusals of the two norm + rope pairs (their kernels need no plan: one row, or one head vector, per unit).
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace alg {

// a *_check's third answer: batch * rows == 0, nothing to do (pointers may be null) -- the entry returns ALG_OK
constexpr int ROW_EMPTY = 1;

// one launch covers 2^31 - 1 workgroups
inline bool row_blocks_fit(int64_t blocks) { return blocks <= 0x7fffffff; }
inline int row_elimit(const char* entry, const char* what, int64_t n) {
  set_error("%s: %s = %lld is more than one launch covers", entry, what, (long long)n);
  return ALG_ELIMIT;
}

enum class RowRoute { ONE_ROW, MANY_ROWS, GENERIC };
struct RowPlan {
  RowRoute route;
  int rpw;         // rows per wave (1 unless MANY_ROWS)
  unsigned grid;   // workgroups of four waves
};
inline RowPlan row_plan_one(RowRoute route, int64_t total) { return {route, 1, (unsigned)((total + 3) / 4)}; }

// "<entry> (<route>, rpw=<n>, grid=<g>): launch failed: ..."
inline int row_check_launch(const char* entry, const RowPlan& pl) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return ALG_OK;
  static const char* const route[] = {"one row per wave", "many rows", "generic width"};
  set_error("%s (%s, rpw=%d, grid=%u): launch failed: %s", entry, route[(int)pl.route], pl.rpw, pl.grid, hipGetErrorString(e));
  return ALG_ELAUNCH;
}

// The widths a kernel family is instantiated for, as ITERS = D / 512.  dispatch_iters calls f(std::integral_constant<int, I>)
// for the I that equals `iters`; false: this width is not instantiated, nothing was called.
template <int... I>
using IterSet = std::integer_sequence<int, I...>;
template <int... I>
constexpr bool has_iters(int iters, IterSet<I...>) { return ((iters == I) || ...); }
template <int... I, class F>
inline bool dispatch_iters(int iters, IterSet<I...>, F&& f) {
  return ((iters == I && (f(std::integral_constant<int, I>{}), true)) || ...);
}

// ---- RMSNorm + rope over a whole row (alg_rmsnorm_rope, wan.hip) and per 128-wide head (alg_headnorm_rope, hunyuan.hip), and
// their e4m3 twins ----
// Filled field by field (value-initialise, then name what the entry has): a twin adds its q8 fields, the per-head form its
// batch strides.  The kernel's own arguments (eps, rope_tokens, the stream) stay with the entry.
struct NormRopeArgs {
  bool per_head;              // true: `heads` 128-wide vectors per row, batch-strided; false: one norm over D, rows contiguous
  bool fp8;                   // the twin: x is only read, q8 (+ scale or head_scale) is written
  const void* x;
  const void* weight;
  const float *cos_tab, *sin_tab;
  int64_t x_rstride, x_bstride;
  int batch, rows;
  int width;                  // D, or heads
  const void* q8;
  int64_t q8_rstride, q8_bstride;
  const float *scale, *head_scale;
};
inline int64_t norm_rope_total(const NormRopeArgs& a) { return (int64_t)a.batch * a.rows; }
// what a wave (rows) or sixteen lanes (head vectors) own, saturating; a workgroup takes four rows or sixteen head vectors
inline int64_t norm_rope_units(const NormRopeArgs& a) {
  const int64_t total = norm_rope_total(a);
  if (!a.per_head) return total;
  return total > INT64_MAX / a.width ? INT64_MAX : total * a.width;
}
inline int64_t norm_rope_blocks(const NormRopeArgs& a) {
  const int64_t units = norm_rope_units(a), per = a.per_head ? 16 : 4;
  return units / per + (units % per != 0);
}

inline int norm_rope_check(const NormRopeArgs& a, const char* entry) {
  const bool tables_bad = a.cos_tab && !a.sin_tab;
  bool bad;
  if (a.per_head) {
    const int64_t elems = (int64_t)a.width * 128;
    bad = a.batch < 0 || a.rows < 0 || a.width <= 0 || a.x_rstride % 8 || a.x_bstride % 8 || a.x_rstride < elems || tables_bad ||
          (a.fp8 && (a.q8_rstride % 8 || a.q8_bstride % 8 || a.q8_rstride < elems));
  } else {
    bad = a.batch < 0 || a.rows < 0 || a.width <= 0 || a.width % 512 || a.x_rstride % 8 || tables_bad ||
          (a.fp8 && (a.q8_rstride % 8 || a.q8_rstride < a.width));
  }
  if (bad) {
    const char* unit = a.per_head ? "heads" : "D";
    if (a.fp8)
      set_error("%s: bad shape batch=%d rows=%d %s=%d strides=%lld / %lld", entry, a.batch, a.rows, unit, a.width,
                (long long)a.x_rstride, (long long)a.q8_rstride);
    else
      set_error("%s: bad shape batch=%d rows=%d %s=%d stride=%lld", entry, a.batch, a.rows, unit, a.width, (long long)a.x_rstride);
    return ALG_EINVAL;
  }
  if (norm_rope_total(a) == 0) return ROW_EMPTY;
  if (!a.fp8 && (!a.x || !a.weight)) {
    set_error("%s: null pointer", entry);
    return ALG_EINVAL;
  }
  if (a.fp8 && (!a.x || !a.weight || !a.q8 || (!a.scale && !a.head_scale) || ((uintptr_t)a.x & 15) || ((uintptr_t)a.q8 & 7))) {
    set_error("%s: null or misaligned pointer (x 16-byte, q8 8-byte; scale or head_scale is needed)", entry);
    return ALG_EINVAL;
  }
  if (!row_blocks_fit(norm_rope_blocks(a)))
    return row_elimit(entry, a.per_head ? "batch * rows * heads" : "batch * rows", norm_rope_units(a));
  return ALG_OK;
}

}  // namespace alg
