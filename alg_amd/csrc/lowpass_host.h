// Host path of the low-pass filters (lowpass.hip, lowpass_v2.hip, lowpass_v3.hip, lowpass_big.hip): alg_down_up and
// alg_gaussian_blur fill ONE LowpassArgs and then run
//     lowpass_check   -- the refusals of both entries, each written once, in a fixed order (lowpass.hip); what depends on the
//                        route -- the global-memory passes' limit and workspace, the tables' alignment -- follows the plan
//                        (lowpass_check_route)
//     lowpass_plan    -- which kernel the call runs, with how many threads, which instantiation and how much LDS: a pure
//                        function of the operands, the device's CU count and ALG_LOWPASS_PATH (lowpass.hip)
//     launch_lowpass_* -- one per route: opts in to the kernel's LDS (opt_in_lds, common.h), launches, check_launch
// No launch step decides whether it takes a call, and the two workspace queries ask the plan's first question.
#pragma once
#include "common.h"
#include "lowpass_tabs.h"

namespace alg {

enum class LowpassFilter { DOWN_UP, GAUSSIAN };

struct LowpassArgs {
  LowpassFilter filter;
  const void* in;
  void* out;
  int64_t planes;
  int H, W, dtype;
  hipStream_t stream;
  int device;                // current_device_slot() of the call, looked up once by the entry: CU count, opt-ins, occupancy
  void* workspace;           // the global-memory passes' intermediates (alg_*_workspace_bytes); unused by the other routes
  int64_t workspace_bytes;
  // DOWN_UP
  int h1, w1;
  int round_mid;             // 1 only for bf16 with round_intermediate set: fp32 has no tensor dtype to round through
  const void* tables;        // alg_lowpass_tables_build's blob, or NULL: the kernels that build their taps per plane
  // GAUSSIAN
  int ksize;
  float sigma;
};

// lowpass.hip, lowpass_v2.hip, lowpass_v3.hip, lowpass_big.hip
enum class LowpassRoute { PLANE, PERSISTENT, BLOCKED, GLOBAL };

struct LowpassPlan {
  LowpassRoute route;
  int threads;          // per workgroup
  int variant;          // the instantiation: PERSISTENT 16-byte prefetch registers per thread (1..4); BLOCKED the tap count K of
                        // a gaussian (3..19), the down-tap bucket of a down_up (5, 7, 9, 11); 0 elsewhere
  size_t lds;           // dynamic LDS bytes per workgroup (GLOBAL: 0)
  int64_t workspace;    // bytes of caller workspace the route needs (GLOBAL only, else 0)
  // the grid: PLANE one workgroup per plane; GLOBAL one thread per output.  The two persistent routes launch
  // min(planes, cus * workgroups resident per CU): PERSISTENT knows the residents from LDS and its launch bounds
  // (wgs_per_cu), BLOCKED asks the runtime in its launch step (wgs_per_cu = 0)
  int cus, wgs_per_cu;
  bool within_limits;   // false: ALG_ELIMIT (GLOBAL only: more than 65,535 planes or rows)
};

constexpr size_t LOWPASS_LDS_CAP = 160 * 1024;   // a CU's LDS; every kernel of the family is opted in to it once per device

// the opt-in of one kernel instantiation (`once` is that instantiation's own); `who` = lowpass_who().  Once it is made on
// the call's device this is one load: the filters are launch-bound at one video, and a device lookup costs as much as the plan
inline int lowpass_opt_in(PerDeviceOnce& once, const void* kernel, const char* who, const LowpassArgs& a) {
  if (device_done(once, a.device)) return ALG_OK;
  return opt_in_lds(once, {kernel}, (int)LOWPASS_LDS_CAP, who);
}

// "<entry> (<route name>)": what a launch or opt-in failure carries
inline const char* lowpass_who(const LowpassArgs& a, LowpassRoute r) {
  static const char* const who[2][4] = {
      {"alg_down_up (plane-per-workgroup kernel)", "alg_down_up (persistent-grid kernel)",
       "alg_down_up (register-blocked kernel)", "alg_down_up (global-memory passes)"},
      {"alg_gaussian_blur (plane-per-workgroup kernel)", "alg_gaussian_blur (persistent-grid kernel)",
       "alg_gaussian_blur (register-blocked kernel)", "alg_gaussian_blur (global-memory passes)"}};
  return who[a.filter == LowpassFilter::GAUSSIAN][(int)r];
}

inline size_t lowpass_esize(const LowpassArgs& a) { return a.dtype == ALG_F32 ? 4 : 2; }
// the 16-byte loads and stores of the two persistent routes
inline bool lowpass_misaligned(const LowpassArgs& a) { return ((uintptr_t)a.in & 15) || ((uintptr_t)a.out & 15); }
inline unsigned lowpass_persistent_grid(const LowpassArgs& a, const LowpassPlan& pl, int wgs_per_cu) {
  const int64_t slots = (int64_t)pl.cus * wgs_per_cu;
  return (unsigned)(a.planes < slots ? a.planes : slots);
}

int lowpass_check(const LowpassArgs& a, const char* entry);                    // lowpass.hip
int lowpass_check_route(const LowpassArgs& a, const LowpassPlan& pl, int option, const char* entry);
LowpassPlan lowpass_plan(const LowpassArgs& a, int cus, int option);           // lowpass.hip
// What each kernel family covers: pure, next to the limits they encode.  true = the plan's route, threads, variant, lds and
// wgs_per_cu are filled in.  lowpass_plan asks BLOCKED first, then PERSISTENT, and plans PLANE when both decline.
bool lowpass_blocked_covers(const LowpassArgs& a, int cus, int option, LowpassPlan* pl);   // lowpass_v3.hip
bool lowpass_persistent_covers(const LowpassArgs& a, int cus, LowpassPlan* pl);            // lowpass_v2.hip
// The global-memory passes' side of the plan (lowpass_big.hip): their workspace and the limit of their 3-D grids
int64_t lowpass_global_bytes(const LowpassArgs& a);
bool lowpass_global_grid_fits(const LowpassArgs& a);

int launch_lowpass_persistent(const LowpassArgs& a, const LowpassPlan& pl);    // lowpass_v2.hip
int launch_lowpass_blocked(const LowpassArgs& a, const LowpassPlan& pl);       // lowpass_v3.hip
int launch_lowpass_global(const LowpassArgs& a, const LowpassPlan& pl);        // lowpass_big.hip

}  // namespace alg
