// Host path of the d = 128 attention entries (attention128.hip, attention128_pipe.hip, attention128_q64.hip,
// attention128_fp8.hip): every extern "C" entry fills ONE Attn128Args and then runs
//     attn128_check  -- the refusals, each written once, in a fixed order (attention128.hip)
//     attn128_plan   -- which kernel the call runs, with which grid: a pure function of the shape and the options
//     launch_*       -- one per kernel: fills that kernel's P, opts in to its LDS (opt_in_lds, common.h) and launches
// Nothing below the entries takes the operands one by one, and no launch step decides whether it takes a call.
#pragma once
#include "common.h"

namespace alg {

struct Attn128Args {
  const void* q;
  const void* k;
  const void* vt;
  void* o;
  int batch, heads, Sq, Skv;
  int64_t q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs;   // strides in elements
  float scale;
  int kv_group, causal;
  hipStream_t stream;
  // what the ranged entries add (alg_flash_attn_d128_ranges*); NULL / 0 from every other entry
  const int32_t* ranges;   // the table: marks the call as a ranged one
  int max_ranges, table_heads;
  float* lse;
  const int32_t* order;
  int order_len;
  float* lse_prefix;
};

// Which refusals an entry has (attn128_check) -- the ranged forms differ in the table's cap and in the optional parts they take
enum class Attn128Form { DENSE, RANGES, RANGES_ORDER, PREFIX };

enum class Attn128Route { BASE, PIPE, Q64 };   // attention128.hip, attention128_pipe.hip, attention128_q64.hip

struct Attn128Plan {
  Attn128Route route;
  int q_blocks;         // blocks of the route's queries per workgroup along Sq
  int64_t grid;         // workgroups: (batch, head) slots rounded up to the 8 XCDs x q_blocks, or the ranged call's order table
  bool use_statement;   // Q64 only: false = every tile through the frame's C++ body (ALG_ATTN128_Q64=3)
  bool within_limits;   // false: ALG_ELIMIT (the grid beyond 2^31 - 1; a ranged call also when attn128_fits fails)
};

constexpr int ATTN128_KVB = 64;                                         // keys per tile, every kernel
constexpr int ATTN128_BASE_ROWS = 256, ATTN128_PIPE_ROWS = 128, ATTN128_Q64_ROWS = 256;   // queries per workgroup
constexpr int ATTN128_PIPE_MIN_TILES = 12;      // what the pipelined kernel takes
constexpr int ATTN128_Q64_MIN_TILES = 8;        // what the 64-query kernel can take (ALG_ATTN128_Q64=2, 3)
constexpr int ATTN128_Q64_POLICY_TILES = 64;    // what it takes by default: 4,096 keys and more

// ---- the predicates of the refusals (the dual and the e4m3 entry word their own messages around them) ----
inline bool attn128_bad_argument(const Attn128Args& a) {
  return !a.q || !a.k || !a.vt || !a.o || a.batch <= 0 || a.heads <= 0 || a.Sq <= 0 || a.Skv <= 0;
}
// 16-byte rows of q / k / vt: strides % 8 for bf16, % 16 for e4m3; o is bf16 in both
inline bool attn128_misaligned(const Attn128Args& a, int mod) {
  return a.q_rs % mod || a.q_bs % mod || a.k_rs % mod || a.k_bs % mod || a.vt_rs % mod || a.vt_bs % mod || a.o_rs % 4 ||
         a.o_bs % 4 || ((uintptr_t)a.q & 15) || ((uintptr_t)a.k & 15) || ((uintptr_t)a.vt & 15) || ((uintptr_t)a.o & 7);
}
// a V^T row covers whole 64-key tiles: the DMA of the last tile reads to its end
inline bool attn128_pitch_short(int64_t vt_rs, int Skv) {
  return vt_rs < (int64_t)((Skv + ATTN128_KVB - 1) / ATTN128_KVB) * ATTN128_KVB;
}
// 31-bit BYTE offsets inside one (batch, head) for the DMA's lane offsets of the pipelined and the 64-query kernel
inline bool attn128_fits(const Attn128Args& a) {
  return (int64_t)(a.Skv + 64) * a.k_rs * 2 < (1ll << 31) && (int64_t)129 * a.vt_rs * 2 < (1ll << 31) &&
         (int64_t)a.Sq * a.q_rs * 2 < (1ll << 31);
}

inline int attn128_q_blocks(const Attn128Args& a, int rows) { return (a.Sq + rows - 1) / rows; }
inline int64_t attn128_grid(const Attn128Args& a, int q_blocks) { return (int64_t)((a.batch * a.heads + 7) / 8) * 8 * q_blocks; }

// The fields every kernel's P starts with (a128::P, a128p::P, a128q::P; a128f8::P has them around its scales).  The P structs
// themselves stay as they are: they are the kernarg layout.
template <class P>
inline void attn128_fill(P& p, const Attn128Args& a, int q_blocks) {
  p.q = (decltype(p.q))a.q; p.k = (decltype(p.k))a.k; p.vt = (decltype(p.vt))a.vt; p.o = (decltype(p.o))a.o;
  p.batch = a.batch; p.heads = a.heads; p.Sq = a.Sq; p.Skv = a.Skv;
  p.q_blocks = q_blocks;
  p.q_bs = a.q_bs; p.q_rs = a.q_rs; p.k_bs = a.k_bs; p.k_rs = a.k_rs;
  p.vt_bs = a.vt_bs; p.vt_rs = a.vt_rs; p.o_bs = a.o_bs; p.o_rs = a.o_rs;
  p.scale_log2 = a.scale * 1.4426950408889634f;
}

int attn128_check(const Attn128Args& a, const char* entry, Attn128Form form);   // attention128.hip
Attn128Plan attn128_plan(const Attn128Args& a);                                 // attention128.hip
int launch_d128_pipe(const Attn128Args& a, const Attn128Plan& pl);              // attention128_pipe.hip
int launch_d128_q64(const Attn128Args& a, const Attn128Plan& pl);               // attention128_q64.hip (the dense form)

}  // namespace alg
