/*
 * alg_hip.h -- C ABI of libalg_hip.so, the MI355X (gfx950) native hot path of the ALG sampler.
 *
 * The reference (choi403/ALG) has no native/FFI layer of its own: its hot path is PyTorch ops called
 * from Python.  Each entry point below therefore cites the reference *call site* it replaces
 * (paths relative to the reference checkout).  Abbreviations:
 *   lp:  lp_utils.py            cog: pipeline_cogvideox_image2video_lowpass.py
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); the library never allocates, frees or caches
 *     device memory: scratch space is a `workspace` argument sized by the matching alg_*_workspace_bytes()
 *     query, precomputed tables are a caller-owned blob filled by an explicit alg_*_build() call
 *   - enqueue-only on `stream` (a hipStream_t, may be NULL = default stream); no internal sync, no blocking
 *     copy: every entry point is legal inside a hipGraph stream capture
 *   - in/out may not alias unless stated
 *   - return 0 on success, negative ALG_E* on failure; message via alg_last_error() (thread local)
 *   - dtype codes: ALG_F32 = 0, ALG_BF16 = 1
 */
#ifndef ALG_HIP_H
#define ALG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALG_F32 0
#define ALG_BF16 1

#define ALG_OK 0
#define ALG_EINVAL (-1)   /* bad argument (shape, dtype, alignment, null pointer) */
#define ALG_ELAUNCH (-2)  /* HIP launch / runtime error */
#define ALG_ELIMIT (-3)   /* shape exceeds what the kernel supports (e.g. plane does not fit LDS) */

#define ALG_VERSION 110

int alg_version(void);
const char* alg_last_error(void);

/* Run-time options.  The library reads its ALG_* environment variables ONCE, when it is loaded; no launch path calls getenv.
 * A host that changes one of them afterwards calls alg_reload_env() (host-only, no GPU work; not to be called while another
 * thread is inside the library).  The default build knows seven, each selecting between bit-identical or documented-equivalent
 * schedules (README.md "Run-time options"): ALG_ATTN_SPLIT_TAIL, ALG_ATTN_PP (4 = the 8-wave pipelined statement on v_mfma_f32_32x32x16_bf16, 7 = the same construction on
 * v_mfma_f32_16x16x32_bf16 -- a call it declines (fewer than 12 KV tiles, 31-bit offsets, V^T pitch) runs the default, 4 --, 8 = statement 4 for any running
 * softmax offset: -m enters the fp32 accumulation as srcC of the first QK k-step and a wave returns to the statement after a
 * refused tile; bit-identical to 4 while every offset snaps to zero --, 0 = the straight loop), ALG_ATTN_VARIANT, ALG_ATTN128_PIPE,
 * ALG_ATTN128_Q64 (1 = the 64-queries-per-wave d = 128 kernel from 4,096 keys on, the default; 2 = for every call it can
 * take; 0 = off: the escape hatch back to the 32-query pipelined kernel), ALG_GEMM_PIPE, ALG_LOWPASS_PATH.  A value must be
 * a whole decimal integer the build knows; anything else (including "off", "1x", an empty string) leaves the default in
 * place.
 *
 * ALG_ATTN128_*: how a d = 128 call is routed.  Every entry checks its arguments, then plans, then launches; the plan is a pure
 * function of the shape and these two options (KV tiles = ceil(Skv / 64)):
 *   - causal or kv_group != 1, or an operand beyond 31-bit byte offsets inside one (batch, head) -- (Skv + 64) * k_rstride * 2,
 *     129 * vt_rstride * 2 or Sq * q_rstride * 2 reaches 2^31 --: the base kernel (attention128.hip);
 *   - otherwise ALG_ATTN128_Q64 = 1 from 64 KV tiles on, = 2 or 3 from 8 on: the 64-query kernel (3: its generated statement
 *     off, every tile through the C++ frame; tests), unless its grid exceeds 2^31 - 1;
 *   - otherwise ALG_ATTN128_PIPE = 1 from 12 KV tiles on: the pipelined 32-query kernel, unless its grid exceeds 2^31 - 1;
 *   - otherwise the base kernel, whose own grid overflow is ALG_ELIMIT "grid too large".
 * alg_flash_attn_d128_dual always runs the base kernel; the alg_flash_attn_d128_ranges* entries always run the 64-query frame
 * (of the option they honour only the value 3) and return ALG_ELIMIT where it cannot address the operands.
 * The 64-query, the pipelined and the e4m3 kernel need more than 64 KiB of LDS and opt in to it once per device.  A failed
 * opt-in is ALG_ELAUNCH with the message "<entry>: hipFuncSetAttribute(<bytes> B LDS): <HIP's text>" from every entry -- it is
 * never answered by running another kernel.  <entry> is the C entry's name, except for the dense entries, whose two routes both
 * ask for 131,072 B and are named "alg_flash_attn_d128 (64-query kernel)" and "alg_flash_attn_d128 (pipelined kernel)".
 * (While routing was "try the kernel, 1 = not covered", a failed opt-in sent a dense call on to the next kernel without a word,
 * a ranged call got ALG_ELIMIT, and alg_flash_attn_d128_fp8 said "cannot reserve <bytes> bytes of LDS".) */
void alg_reload_env(void);

/* ------------------------------------------------------------------------------------------------
 * Low-pass filters on [planes, H, W] contiguous planes (a 4-D/5-D tensor viewed per (H, W) plane,
 * lp:31-37).  Planes resident in LDS: one workgroup per plane for small calls, a persistent grid of
 * register-blocked workgroups from 128 planes up (all bit-identical; planes beyond LDS size run
 * through global-memory passes).
 *
 * Both entries check their arguments, then plan, then launch.  The plan is a pure function of the operands, the device's
 * compute units (CUs; 256 on an MI355X) and ALG_LOWPASS_PATH, and the two workspace queries answer from its first rule:
 *   - "global-memory passes" (lowpass_big.hip): a plane whose plane-per-workgroup kernel would need more than 160 KiB of
 *     LDS, a blur of more than 255 taps, every call under ALG_LOWPASS_PATH=4.  The only route that needs `workspace`; more
 *     than 65,535 planes or rows (H, or h1 of a down_up) is ALG_ELIMIT;
 *   - ALG_LOWPASS_PATH=1, or a down_up call with tables = NULL: the "plane-per-workgroup kernel" (lowpass.hip);
 *   - otherwise the "register-blocked kernel" (lowpass_v3.hip) unless ALG_LOWPASS_PATH=2: at least CUs / 2 planes (=3: any
 *     count) of even W and H * W a multiple of four, `in` and `out` 16-byte aligned; a blur of 3..19 taps with ksize / 2 + 1
 *     below H and W; a down_up whose way back has 3 taps along both axes and whose way down has at most 11 along W and 64
 *     along H; a plane that fits the kernel's own LDS layout and 8 prefetch loads per thread;
 *   - otherwise the "persistent-grid kernel" (lowpass_v2.hip): more than 2 * CUs planes whose byte size is a multiple of 16
 *     and at most 64 KiB, `in` and `out` 16-byte aligned, inside its LDS layout (a down_up also: H * w1 a multiple of four,
 *     at most 64 taps along W);
 *   - otherwise the plane-per-workgroup kernel.
 * No kernel is tried and fallen back from.  Every kernel of the family is opted in to 160 KiB of LDS once per device; a failed
 * opt-in or launch is ALG_ELAUNCH and names the route: "<entry> (<route name>): hipFuncSetAttribute(<bytes> B LDS): <HIP's
 * text>" or "<entry> (<route name>): launch failed: <HIP's text>", e.g. "alg_down_up (register-blocked kernel): ...".
 * ---------------------------------------------------------------------------------------------- */

/* lp:49-54  F.interpolate(bilinear, antialias) to (h1, w1) then back to (H, W).
 * h1, w1 are computed by the caller exactly as lp:51-52 (Python banker's rounding).
 * round_intermediate != 0 rounds the (h1, w1) intermediate to bf16 (the reference's two separate
 * interpolate calls each return a tensor of the input dtype); only meaningful for ALG_BF16. */
int alg_down_up(const void* in, void* out, int64_t planes, int H, int W, int h1, int w1, int dtype,
                int round_intermediate, const void* tables, void* workspace, int64_t workspace_bytes, void* stream);

/* The antialias tap tables of one (H, W) -> (h1, w1) -> (H, W) shape (lp:51-54: the weights F.interpolate(antialias=True)
 * derives per output index), as a blob the caller owns: alg_lowpass_tables_bytes() sizes it, alg_lowpass_tables_build()
 * fills it with one tiny kernel on `stream`, alg_down_up(tables=...) reads it on any later call of that shape (ordered
 * after the build on the stream, as usual).  tables = NULL is legal: alg_down_up then uses the kernels that derive the
 * taps per plane (identical bits, lower throughput on many-plane batches). */
int64_t alg_lowpass_tables_bytes(int H, int W, int h1, int w1);
int alg_lowpass_tables_build(void* tables, int64_t bytes, int H, int W, int h1, int w1, void* stream);

/* Scratch bytes alg_down_up needs for this call (0 for planes that fit LDS -- every latent-sized plane; pixel-sized planes
 * run through global-memory passes with fp32 intermediates in `workspace`). */
int64_t alg_down_up_workspace_bytes(int64_t planes, int H, int W, int h1, int w1);

/* lp:40-47  torchvision gaussian_blur(kernel_size=[k,k], sigma=[s,s]): reflect pad k/2, separable
 * correlation with g = exp(-0.5 (x/s)^2)/sum.  ksize must be odd (any size: more than 255 taps run through the global-memory
 * passes), ksize/2 < min(H, W), sigma > 0.  Weights are fp32 for every dtype (torchvision builds them in the image dtype:
 * for bf16 tensors see DESIGN.md section 2, "Rounding semantics"). */
int alg_gaussian_blur(const void* in, void* out, int64_t planes, int H, int W, int ksize, float sigma, int dtype,
                      void* workspace, int64_t workspace_bytes, void* stream);
int64_t alg_gaussian_blur_workspace_bytes(int64_t planes, int H, int W, int ksize);   /* 0 for LDS-sized planes */

/* ------------------------------------------------------------------------------------------------
 * cog:1091-1123  noise_pred.float(); chunk; CFG combine; CogVideoXDDIMScheduler.step (v-prediction,
 * eta = 0); cast back -- one fused elementwise pass, latents updated IN PLACE.
 *   n_pass = 3: u0 + g*(text - u)   (pred = [uncond_init, uncond, text], cog:1099-1102)
 *   n_pass = 2: u  + g*(text - u)   (cog:1096-1097)
 *   n_pass = 1: pred                (no CFG)
 *   x0 = sqrt_alpha_t * x - sqrt_beta_t * v ;  x <- coef_a * x + coef_b * x0
 * pred: [n_pass, numel] of pred_dtype;  latents: [numel] of lat_dtype.
 * ---------------------------------------------------------------------------------------------- */
int alg_cfg_ddim_step(const void* pred, int pred_dtype, void* latents, int lat_dtype, int n_pass, int64_t numel,
                      float guidance_scale, float sqrt_alpha_t, float sqrt_beta_t, float coef_a, float coef_b,
                      void* stream);

/* wan:919-924, hy:1254-1261  CFG combine in the prediction dtype (no .float()): out = u0 + g*(text - u), every
 * intermediate rounded to `dtype`.  pred [n_pass, numel] (n_pass 2 or 3), out [numel]. */
int alg_cfg_combine(const void* pred, void* out, int dtype, int n_pass, int64_t numel, float guidance_scale,
                    void* stream);

/* CFG residual reuse across steps (an extension: alg_amd/cfg_reuse.py; the reference has none).  A two-pass step keeps
 * delta = text - uncond (STORE); a later step that ran the conditional pass alone rebuilds the unconditional prediction from it
 * (REUSE) and goes on with the arithmetic of the plain entry.  All three entries check, plan, launch: a mode outside {0, 1}, a
 * dtype code the entry does not know, a negative numel, a null pointer, or a pointer that is not aligned to its element size
 * (alg_cfg_delta_drift: a and b to 16 bytes, work and out to 8) is ALG_EINVAL before anything is launched; numel == 0 is ALG_OK
 * without a launch (and without a look at the pointers). */
#define ALG_CFG_DELTA_STORE 0
#define ALG_CFG_DELTA_REUSE 1

/* alg_cfg_ddim_step with the delta; delta: fp32 [numel]; latents: [numel] of lat_dtype, updated IN PLACE.
 *   STORE: pred [2, numel] = [uncond, text].  latents get the bits alg_cfg_ddim_step(n_pass = 2) gives them, and
 *          delta[e] = float(text[e]) - float(uncond[e])  (one fp32 subtraction: the value the combine forms anyway)
 *   REUSE: pred [1, numel] = [text].  u' = float(text) - delta (fp32), then the n_pass = 2 update on (u', text):
 *          v = u' + g * (text - u');  x0 = sqrt_alpha_t * x - sqrt_beta_t * v;  x <- coef_a * x + coef_b * x0
 * The dtype pairs and the two paths of alg_cfg_ddim_step: 8 elements per lane and trip when numel % 8 == 0 and pred, delta and
 * latents are 16-byte aligned, one element otherwise; a grid of at most 2,048 blocks with a grid-stride loop. */
int alg_cfg_ddim_step_delta(const void* pred, int pred_dtype, float* delta, void* latents, int lat_dtype, int mode, int64_t numel,
                            float guidance_scale, float sqrt_alpha_t, float sqrt_beta_t, float coef_a, float coef_b,
                            void* stream);

/* alg_cfg_combine with the delta (the Wan / HunyuanVideo loops, and the fp32 combine in front of CogVideoX's DPM step): every
 * intermediate is rounded to `dtype` (rnd), and delta [numel] has that dtype; out [numel].
 *   STORE: pred [2, numel].  out has the bits of alg_cfg_combine(n_pass = 2), delta = rnd(text - uncond), that kernel's d
 *   REUSE: pred [1, numel].  u' = rnd(text - delta), then out = u' + rnd(g * rnd(text - u')) */
int alg_cfg_combine_delta(const void* pred, void* delta, void* out, int dtype, int mode, int64_t numel, float guidance_scale,
                          void* stream);

/* The drift of the delta (the diagnostic of cfg_reuse_drift): out[0] = sum |float(a) - float(b)|, out[1] = sum |float(b)| over
 * a (new), b (cached): [numel] of `dtype` (ALG_F32 or ALG_BF16), 16-byte aligned; numel needs no alignment.  DEVICE doubles,
 * deterministic, alg_attn_drift's scheme: the elements go in groups of 8, the terms of a group are added in fp32 (a chain of 8),
 * everything above in double in a fixed order that depends on numel alone (a capped grid with a grid-stride loop, one partial
 * pair per block into `work`, a second launch of one block sums them); no atomics.  The last group of a numel that is no
 * multiple of 8 is read element by element and filled with zeros, so its chain has numel % 8 terms that count.  A NaN in a
 * reaches out[0] only.  work: alg_cfg_delta_drift_workspace_bytes(numel) bytes, 8-byte aligned.  numel == 0 launches nothing
 * and leaves out as it is. */
int64_t alg_cfg_delta_drift_workspace_bytes(int64_t numel);
int alg_cfg_delta_drift(const void* a, const void* b, int dtype, int64_t numel, void* work, double* out, void* stream);

/* out = sum_i coefs[i] * xs[i]  (1..4 terms, each ALG_F32 or ALG_BF16).  Rounding follows torch eager: every product
 * is rounded to its tensor's dtype, the running sum is fp32, left to right, unfused; cast to out_dtype at the end.
 * Covers FlowMatchEulerDiscreteScheduler.step (hy:1265-1269: sample + (sigma_next - sigma) * v) and UniPC's
 * convert_model_output (wan:927: sample - sigma * v).
 * xs, coefs, dtypes are HOST arrays; the pointers inside xs are device pointers. */
int alg_lincomb(const void* const* xs, const float* coefs, const int* dtypes, int n_terms, void* out, int out_dtype,
                int64_t numel, void* stream);

/* Step cache ("first-block cache", an extension: the reference has none) -- the probe behind block 0 of a DiT, one call per
 * sample.  keep = the caller's copy of the hidden state in front of block 0 (x0), x1 = the hidden state behind it, r = the
 * residual the last forward left (r_prev); all [rows][D] bf16, three distinct buffers, 16-byte aligned, D % 8 == 0.
 *   r_new = bf16(float(x1) - float(x0))                                               every row
 *   a = sum |float(r_new) - float(r_prev)|,  b = sum |float(r_prev)|                  rows [tok0, tok0 + tok_rows) only
 * and in the same pass r <- r_new, keep <- x1 (the copy the cached tail is taken against).  sums[0] = a, sums[1] = b: DEVICE
 * doubles, deterministic (no atomics: eight fp32 terms per 16-byte vector, everything above in double in a fixed order that
 * depends on (rows, D) alone).  workspace: alg_step_cache_workspace_bytes(rows, D) bytes, 8-byte aligned.  rows == 0 writes
 * zeros.  The decision (a < threshold * b) is the host's: alg_amd/step_cache.py. */
int64_t alg_step_cache_workspace_bytes(int rows, int D);
int alg_step_cache_probe(void* keep, const void* x1, void* r, int rows, int D, int tok0, int tok_rows, void* workspace,
                         double* sums, void* stream);

/* Attention-reuse drift (an extension: alg_amd/attn_reuse.py) -- how far a layer's attention output moved from its cached copy.
 * a (new), b (cached): bf16 [rows][cols], row strides in ELEMENTS (multiples of 8, at least cols), cols % 8 == 0, 16-byte aligned.
 *   out[0] = sum |float(a) - float(b)|,  out[1] = sum |float(b)|
 * DEVICE doubles, deterministic (no atomics: eight fp32 terms per 16-byte vector, everything above in double in a fixed order
 * that depends on (rows, cols) alone: a capped grid with a grid-stride loop, one partial pair per block into `work`, a second
 * launch of one block sums them).  A NaN in a reaches out[0] only.  work: alg_attn_drift_workspace_bytes(rows, cols) bytes,
 * 8-byte aligned.  rows == 0 writes zeros (a and b are not read then and may be null).  Bytes between cols and a row stride are
 * not read.  Every refusal is ALG_EINVAL before anything is launched. */
int64_t alg_attn_drift_workspace_bytes(int rows, int cols);
int alg_attn_drift(const void* a, const void* b, int rows, int cols, int64_t a_rstride, int64_t b_rstride, void* work, double* out,
                   void* stream);

/* Far-field attention reuse (an extension: alg_amd/attn_far.py) -- the merge of two partial attentions over DISJOINT key sets.
 * o: bf16 [batch][Sq][heads * head_dim], batch and row strides in ELEMENTS, IN PLACE: the near partial on entry, the merged
 * attention on return; o_far: the same shape with its own strides; lse, lse_far, lse_out: fp32 [batch][heads][Sq], contiguous, the
 * log2-domain log-sum-exp of the keys each partial visited, exactly as alg_flash_attn_d64_ranges_heads and
 * alg_flash_attn_d128_ranges_heads write it.  head_dim: 64 or 128.  For every (b, h, q), with a = lse and f = lse_far:
 *   f == -inf               the row of o keeps its BITS (it is not written)
 *   a == -inf, f finite     the row of o becomes the far row's bits
 *   otherwise               m = max(a, f), wa = exp2(a - m), wf = exp2(f - m),
 *                           o = bf16_rne((wa * o + wf * o_far) / (wa + wf))   in fp32, no contraction: ONE rounding to bf16
 *                           a weight that underflows to 0 gives the other side's bits, as above
 *   lse_out (may be NULL)   m + log2(wa + wf); -inf when both are; it may be lse itself
 * Every output element is a function of its own operands alone (16-byte accesses, a capped grid with a grid-stride loop, vector
 * stores only, no atomics, no scratch): run-to-run bit-identical.  Enqueue-only, allocation-free.  Bytes between heads * head_dim and
 * a row stride are neither read nor written.  ALG_EINVAL before anything is launched: batch, heads or Sq < 1; head_dim not 64 / 128;
 * a row stride below heads * head_dim or not a multiple of 8; a batch stride that is not a multiple of 8 or (batch > 1) does not
 * hold a sample's rows; a null pointer (except lse_out); o or o_far not 16-byte aligned, an lse not 4-byte aligned. */
int alg_attn_merge_lse(void* o, const float* lse, const void* o_far, const float* lse_far, int batch, int heads, int head_dim, int Sq,
                       int64_t o_bstride, int64_t o_rstride, int64_t far_bstride, int64_t far_rstride, float* lse_out, void* stream);

/* Pooled far-field attention (an extension: alg_amd/attn_pool.py) -- the far-side operands at 1 / group of their resolution.
 * Every group of `group` (2, 4 or 8) consecutive keys, aligned to `group` on the absolute key index, becomes one pooled key: the
 * fp32 sum of its rows in ascending key order, times the exact 1 / group, rounded ONCE to bf16.  P = S / group (floor) pooled
 * keys; keys behind P * group are not read into any of them; the pooled keys P .. P_pad - 1, P_pad = P rounded up to 64, are
 * written as zero.  head_dim: 64 or 128; strides in ELEMENTS.
 *   alg_attn_pool_k   src: bf16 [batch][S][heads * head_dim] rows (a row stride >= heads * head_dim: the K half of a Q|K buffer),
 *                     dst: bf16 [batch][P_pad][heads * head_dim]; bytes between heads * head_dim and a row stride are neither
 *                     read nor written
 *   alg_attn_pool_vt  src: bf16 V^T [batch][heads * head_dim][>= S rounded up to 64], dst: [batch][heads * head_dim][>= P_pad],
 *                     pooled along the key axis; in both, the keys of every 16 columns are stored with index bits 2 and 3
 *                     swapped, as the attention entries expect them.  Source columns behind S rounded up to 16 are not read,
 *                     destination columns behind P_pad not written
 * Memory-bound: 16-byte accesses on both sides, a capped grid with a grid-stride loop, vector stores only, no atomics, no
 * scratch; run-to-run bit-identical.  Enqueue-only, allocation-free.  ALG_EINVAL before anything is launched: a null or not
 * 16-byte aligned pointer; batch or heads < 1; head_dim not 64 / 128; group not 2 / 4 / 8; S < group; a stride that is not a
 * multiple of 8, a row stride below what is stated above, a batch stride (batch > 1) that does not hold a sample. */
int alg_attn_pool_k(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst, int64_t dst_bstride, int64_t dst_rstride,
                    int batch, int heads, int head_dim, int S, int group, void* stream);
int alg_attn_pool_vt(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst, int64_t dst_bstride, int64_t dst_rstride,
                     int batch, int heads, int head_dim, int S, int group, void* stream);

/* alg_attn_merge_lse with far_lse_shift (finite) added to every far log-sum-exp before the merge: far keys that each stand for
 * 2^far_lse_shift keys (the pooled keys above: log2 group).  An lse_far of -inf stays -inf: the row of o keeps its bits.  With
 * far_lse_shift == 0 the result is alg_attn_merge_lse's bit for bit.  lse_far itself is not written. */
int alg_attn_merge_lse_shift(void* o, const float* lse, const void* o_far, const float* lse_far, int batch, int heads, int head_dim,
                             int Sq, int64_t o_bstride, int64_t o_rstride, int64_t far_bstride, int64_t far_rstride,
                             float far_lse_shift, float* lse_out, void* stream);

/* LoRA merge at load time (an extension; the reference pipelines inherit diffusers' LoRA loader mixins; alg_amd/lora.py merges
 * the adapters into the state dict BEFORE a transformer is built from it, so no forward path knows about them):
 *   t[n, r]   = double(scale[r]) * double(B[n, r])                exact
 *   acc[n, k] = fma(t[n, r], double(A[r, k]), acc)                r = 0 .. R-1 ascending, from acc = 0, in double
 *   out[n, k] = bf16_rne(double(W[n, k]) + acc[n, k])             ONE rounding, from the double sum straight to bf16
 * (double, not fp32: where W and the delta cancel, an fp32 chain is several bf16 steps away from the float64 merge; this is
 * within one step everywhere, and it runs once per model load)
 * W: [N][K] of w_dtype (ALG_BF16 or ALG_F32: an fp32 checkpoint is not rounded to bf16 before the delta is added), leading
 * dimension ldw; A: [R][K] fp32 and B: [N][R] fp32, both contiguous; scale: [R] fp32, one entry per rank column (several adapters
 * are concatenated along R by the caller, each column carrying its user_scale * alpha / r; B is never pre-scaled); out: bf16
 * [N][K], leading dimension ldo.  out may be W itself when W is bf16 and ldw == ldo; any other overlap of the two is refused.
 * 1 <= R <= 512; K % 8 == 0; N and R need no alignment (N == 0: nothing is launched); ldw, ldo >= K and multiples of 16
 * bytes; W, A and out 16-byte aligned.  Bytes between K and a leading dimension are neither read nor written.
 * The chain of one output element is a function of its own operands alone (vector fp64 FMA, no MFMA, no atomics): the result
 * does not depend on the tile, the grid or where a row lies in the matrix -- a slice merged alone has the bits of the full
 * merge, and every rank of a multi-GPU run produces the same weights.
 * Check, plan, launch: the shape refusals come first (a validate-only call may pass null pointers), then null or misaligned
 * pointers and the aliasing rule, all ALG_EINVAL before anything is launched; more workgroups (64 x 128 outputs each) than one
 * launch covers is ALG_ELIMIT. */
int alg_lora_merge(const void* W, int w_dtype, int64_t ldw, const float* A, const float* B, const float* scale, void* out,
                   int64_t ldo, int N, int K, int R, void* stream);

/* wan:877-889, hy:1146-1160, 1230  CFG batch assembly in one launch (replaces cat([latents]*n) + cat(dim) + .to()):
 *   out[i, o, a, r] = a < A0 ? src0[i][o*s0_ostride + a*R + r] : src1[i][o*s1_ostride + (a1_off + a - A0)*R + r]
 * for i < n (<= 16), o < O, a < A0 + A1, r < R, cast to out_dtype.  src0 / src1 are HOST arrays of n device pointers
 * (one per output sample -- repeat a pointer to duplicate a sample across CFG passes).
 *   Wan    (channel concat [latents | condition]):      O=1, A0=16, A1=20, R=F*H*W
 *   Hunyuan (first-frame token replace [cond | lat 1:]): O=C, A0=cond frames, A1=F-1, R=H*W, a1_off=1 */
int alg_concat_cast(const void* const* src0, int dtype0, const void* const* src1, int dtype1, int n, int64_t O,
                    int64_t A0, int64_t A1, int64_t R, int64_t s0_ostride, int64_t s1_ostride, int64_t a1_off,
                    void* out, int out_dtype, void* stream);

/* wan:927  UniPCMultistepScheduler (bh1/bh2, predict_x0, solver_order <= 2) predictor or corrector update on fp32:
 *   out = (r*x - c*m0) - k * ( [m1] rho0*((m1 - m0)/rk)  +  [m_new] rho_new*(m_new - m0) )
 * m1 / m_new may be NULL (order-1 predictor: both NULL; order-1 corrector: m1 NULL). */
int alg_unipc_update(const float* x, const float* m0, const float* m1, const float* m_new, float* out,
                     int64_t numel, float r, float c, float k, float rk, float rho0, float rho_new, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Video-DiT forward building blocks (cog:1082-1090 self.transformer(...); the arithmetic is
 * diffusers' CogVideoXTransformer3DModel -- see DESIGN.md).  All activations bf16, fp32 accumulate.
 * ---------------------------------------------------------------------------------------------- */

#define ALG_ACT_NONE 0
#define ALG_ACT_GELU_TANH 1
#define ALG_ACT_SILU 2

#define ALG_GEMM_BIAS_PER_ROW 1   /* bias indexed by output row (used for the transposed V projection) */
#define ALG_GEMM_PERMUTE_COLS 4   /* store column n at n with bits 2 and 3 swapped (MFMA k-order for V^T) */
#define ALG_GEMM_GATE_SEG_STRIDE 16 /* gate[1] sits gate_seg_stride elements after gate[0] instead of N */
#define ALG_GEMM_B_PACKED11 32     /* B is NOT [N][K] but the panel alg_pack_b_p11 wrote from it (ldb ignored, strideB must be 0): the call runs
                                     GEMM schedule 11 -- 1 x 4 waves, the weight fetched straight into registers in MFMA-fragment order --
                                     under every ALG_GEMM_PIPE.  Accepted by alg_gemm_bf16 and by either problem of alg_gemm_bf16_pair /
                                     _pair_qk (that problem then runs as its own alg_gemm_bf16 call); alg_gemm_fp8 and the convolution
                                     addressing refuse it (ALG_EINVAL) */
#define ALG_GEMM_GATE_F32 8       /* gate is float32 and C = bf16(R + gate * bf16(acc + bias)) with ONE final rounding
                                     (WanTransformerBlock: (x.float() + out * gate_msa).type_as(x)) */

typedef struct alg_gemm_args {
  const void* A;      /* [batch][M][K] bf16, row stride lda, batch stride strideA (elements) */
  const void* B;      /* [batch][N][K] bf16 (nn.Linear weight layout), ldb, strideB (0 = shared)  */
  void* C;            /* [batch][M][N] bf16, ldc, strideC */
  const void* bias;   /* [N] (or [M] with BIAS_PER_ROW) bf16, may be NULL */
  const void* R;      /* residual [batch][M][N] bf16 (ldr, strideR), may be NULL; may alias C   */
  const void* gate;   /* [batch][2][N] bf16: gate[0] for rows < seg_split, gate[1] otherwise; NULL = 1 */
  int64_t lda, ldb, ldc, ldr;
  int64_t strideA, strideB, strideC, strideR, strideGate;
  int32_t M, N, K, batch;
  int32_t seg_split;
  int32_t act;        /* ALG_ACT_* applied to (acc + bias) */
  int32_t flags;      /* ALG_GEMM_* */
  int64_t gate_seg_stride; /* with ALG_GEMM_GATE_SEG_STRIDE: elements between gate[0] and gate[1] (default N; 0 = one gate) */
  int32_t perm_col0;  /* with ALG_GEMM_PERMUTE_COLS: output column n is joint column perm_col0 + n of a wider permuted row
                         (C points at joint column 0); 0 for a stand-alone V^T */
  int32_t conv_cin_log2; /* implicit-GEMM convolution (alg_conv_bf16 sets these; 0 = plain GEMM): log2 of the channels per tap */
  const float* a_scale; /* alg_gemm_fp8 only: one scale per row of A, [batch][M] at batch stride strideAScale */
  const float* b_scale; /* alg_gemm_fp8 only: one scale per row of B, [batch][N] at batch stride strideBScale (0 = shared) */
                        /* alg_gemm_fp4 reinterprets both pointers as E8M0 BYTE arrays, [batch][M][K/32] and [batch][N][K/32] row-major
                           (one scale per 32 elements along K), with strideAScale / strideBScale in bytes */
  int64_t strideAScale, strideBScale;
  int32_t conv_wp;   /* rows of A between vertically adjacent taps (padded width) */
  int32_t conv_hpwp; /* rows of A between temporally adjacent taps (padded height * padded width) */
  int32_t conv_kw;   /* taps along x: 3, or 4 when one A row holds two neighbouring voxels (lda = 2 * channels) */
  int32_t reserved1;
} alg_gemm_args;

/* C = R + gate * act(A @ B^T + bias)   (bias optional; either act or the residual(+gate) form).  K % 64 == 0, lda/ldb % 8 == 0,
 * A and B 16-byte aligned.  M and N are arbitrary (edge tiles clamp loads and guard stores).
 * C, R, gate and a column bias: with N % 4 == 0 the epilogue moves whole quads, so C, R, a bf16 gate and the column bias are 8-byte
 * aligned, a float32 gate (ALG_GEMM_GATE_F32) 16-byte aligned, and every pitch -- ldc, ldr, strideC, strideR, strideGate, and
 * gate_seg_stride under ALG_GEMM_GATE_SEG_STRIDE -- is a multiple of 4 elements (0 included); a call that breaks this is ALG_EINVAL
 * before any launch and writes no C.  With N % 4 != 0 every access is a single element: nothing beyond the element size is
 * required.  (16-byte aligned C / R / gate with pitches in multiples of 8, N % 8 == 0 and perm_col0 % 16 == 0 is the fast path;
 * the result does not depend on which store loop a call takes: tests/test_gpu_gemm_operands.py.) */
int alg_gemm_bf16(const alg_gemm_args* args, void* stream);

/* Packs an nn.Linear weight W [N][K] (bf16, row pitch ldb elements) for GEMM schedule 11 (ALG_GEMM_B_PACKED11): per (256-row tile of W,
 * 64-deep k-tile) 32 KiB in MFMA-fragment order, rows past N zero.  alg_pack_b_p11_bytes(N, K) = ceil(N / 256) * (K / 64) * 32768 is the
 * size of `packed` (caller-owned, 16-byte aligned).  K % 64 == 0, K >= 128.  Done once when a model is loaded; the reference's
 * nn.Linear weights (e.g. the attn1.to_q / ff.net.* tensors behind /root/reference/pipeline_cogvideox_image2video_lowpass.py:1082) keep
 * their values -- only the order in memory changes. */
int64_t alg_pack_b_p11_bytes(int N, int K);
int alg_pack_b_p11(const void* w, void* packed, int N, int K, int64_t ldb, void* stream);

/* Two independent alg_gemm_bf16 calls as ONE persistent launch when both are plain (no residual, gate, activation or
 * convolution addressing, a row-major B; the Q|K and V^T projections of a DiT block, cog:1082-1090, read the same activations):
 * the tiles of `b` follow the tiles of `a` in the tile list, so the two launches' partial last rounds become one.  Every output
 * element is computed exactly as by the two separate calls (bit-identical); calls the pair form cannot take run one after the
 * other -- among them a problem with a packed B (ALG_GEMM_B_PACKED11), which runs on schedule 11 as its alg_gemm_bf16 call
 * would.  Every argument check of alg_gemm_bf16 runs on both problems before anything is launched: a bad call writes no C.
 * C of one problem must not alias an operand of the other. */
int alg_gemm_bf16_pair(const alg_gemm_args* a, const alg_gemm_args* b, void* stream);

/* alg_gemm_bf16_pair with the CogVideoX block's per-head QK LayerNorm + rotary embedding (alg_qk_norm_rope_scaled; diffusers
 * CogVideoXAttnProcessor2_0: norm_q / norm_k / apply_rotary_emb, cog:1082-1090) applied to problem `qk` inside its store loop:
 * qk->C is the [batch][S][2][heads][64] tensor (M = S, N = ldc = 2*heads*64, strideC = S*N), written ONCE in its final
 * form.  Bit-identical to alg_gemm_bf16_pair followed by alg_qk_norm_rope_scaled(qk->C, ..., qk->batch, qk->M, heads,
 * text_len, eps, q_scale) -- which is exactly what runs when the fused form cannot take the call (heads % 4 != 0, schedule 6,
 * a pair the persistent launch cannot take, e.g. a packed B in either problem). */
typedef struct alg_qk_norm_rope_args {
  const void *wq, *bq, *wk, *bk;      /* [64] bf16 LayerNorm weight / bias of norm_q and norm_k */
  const float *cos_tab, *sin_tab;      /* [S - text_len][64] float32, or both NULL (no rotary embedding) */
  int32_t heads, text_len;
  float eps, q_scale;                  /* q_scale: see alg_qk_norm_rope_scaled (1 = plain) */
} alg_qk_norm_rope_args;
int alg_gemm_bf16_pair_qk(const alg_gemm_args* qk, const alg_gemm_args* vt, const alg_qk_norm_rope_args* e, void* stream);

/* BASELINE config 5 (fp8 weights on the CDNA4 fp8 MFMA): same contract and epilogues with A and B holding OCP e4m3 bytes
 * (lda / ldb / strides in elements = bytes) and per-row float32 scales: C = epilogue(a_scale[m] * b_scale[n] * (A @ B^T)).
 * K % 128 == 0.  Operands come from alg_quantize_fp8_rows (activations: per token, weights: per output channel).  B is always
 * row-major: ALG_GEMM_B_PACKED11 is refused with ALG_EINVAL before anything is launched. */
int alg_gemm_fp8(const alg_gemm_args* args, void* stream);

/* Row-wise dynamic quantisation to OCP e4m3: scale[r] = max|x[r]| / 448 (1 if the row is zero), q = e4m3(x / scale).
 * x: rows of K bf16 at stride x_rstride (elements); q: rows of K bytes, contiguous; scale: [rows] float32. */
int alg_quantize_fp8_rows(const void* x, int64_t x_rstride, void* q, float* scale, int64_t rows, int K, void* stream);
/* OCP MXFP4 operands (MX v1.0: e2m1 elements, one E8M0 scale per block of 32 consecutive elements along K) on
 * v_mfma_scale_f32_32x32x64_f8f6f4 with both format selectors at FP4 and the block scales in the instruction's scale operands:
 * the contract and epilogues of alg_gemm_fp8 -- C = R + gate * act((A @ B^T) + bias), A and B already scaled by their blocks --
 * with A [batch][M][K/2 bytes] and B [batch][N][K/2 bytes] holding packed e2m1 (element 2i in the LOW nibble of byte i; lda /
 * ldb / strideA / strideB count ELEMENTS, two per byte, each a multiple of 32 = 16 bytes, A and B 16-byte aligned) and a_scale /
 * b_scale reinterpreted as the E8M0 byte arrays [batch][rows][K/32] (8-byte aligned; strideAScale / strideBScale in bytes,
 * multiples of 8, 0 = shared).  K % 256 == 0; M and N arbitrary (edge tiles clamp loads and guard stores); bias, ALG_ACT_*,
 * residual (may alias C), bf16 / fp32 gate with seg_split, strideGate and ALG_GEMM_GATE_SEG_STRIDE, batch strides as in
 * alg_gemm_bf16.  A scale byte of 0xFF (NaN) is outside the contract.  ALG_GEMM_B_PACKED11, ALG_GEMM_BIAS_PER_ROW,
 * ALG_GEMM_PERMUTE_COLS and the convolution addressing are refused with ALG_EINVAL before anything is launched. */
int alg_gemm_fp4(const alg_gemm_args* args, void* stream);

/* Row-wise quantisation to OCP MXFP4, the operand form of alg_gemm_fp4 (activations: per token; weights, once at load: per
 * output channel).  Per block of 32 consecutive elements of a row:
 *   scale byte (E8M0)  e = clamp(floor(log2(amax)) - 2, -127, 127) + 127; an all-zero block writes 127; 0xFF is never written;
 *   elements           x * 2^-(e - 127) rounded to nearest, ties to even, onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6
 *                      (codes 0..7, bit 3 = the input's sign bit, kept also where the value rounds to zero);
 *   packing            two elements per byte, element 2i in the low nibble of byte i.
 * x: rows of K bf16 at stride x_rstride (elements, >= K, % 8 == 0), 16-byte aligned; q: [rows][K/2] bytes, contiguous, 4-byte
 * aligned; scales: [rows][K/32] bytes, contiguous.  K % 32 == 0.  NaN and Inf inputs are outside the contract (an Inf block
 * would need the scale 2^126 and saturate, a NaN compares false everywhere and becomes a signed zero).  A bad call is ALG_EINVAL
 * before any launch. */
int alg_quantize_mxfp4_rows(const void* x, int64_t x_rstride, void* q, void* scales, int64_t rows, int K, void* stream);

/* alg_gemm_fp4 with an MXFP4 output, for a GEMM whose result is the next MXFP4 GEMM's A operand: instead of bf16, C receives
 * [batch][M][N/2] packed e2m1 bytes (ldc / strideC count ELEMENTS, multiples of 32, ldc >= N; C 16-byte aligned) and out_scales
 * the E8M0 bytes [batch][M][N/32] (rows contiguous, 8-byte aligned, out_scales_bstride in bytes, a multiple of 8) -- bit for
 * bit what alg_gemm_fp4 into a bf16 C followed by alg_quantize_mxfp4_rows writes: the quantiser sees the bf16-rounded epilogue
 * value act((A @ B^T) + bias), which never reaches memory.  N % 32 == 0; M arbitrary; ALG_ACT_NONE or ALG_ACT_GELU_TANH; no
 * residual and no gate; C must not overlap A, nor out_scales a_scale (workgroups read A while others store).  Those and
 * everything alg_gemm_fp4 refuses are ALG_EINVAL before any launch.  The pointer is a parameter: alg_gemm_args keeps its layout. */
int alg_gemm_fp4_q4out(const alg_gemm_args* args, void* out_scales, int64_t out_scales_bstride, void* stream);

/* The same quantiser on rows that sit inside a wider, batch-strided bf16 buffer, all batch items in ONE launch: row r of item b
 * starts at x + b * x_bstride + r * x_rstride (elements, both % 8 == 0; a column offset goes through the pointer); q is
 * [batch * rows][K] contiguous, scale [batch * rows].  Bit-identical to alg_quantize_fp8_rows on each item.  K = 3072, 12288 and
 * 15360 (HunyuanVideo's D, M and D + M) keep the row in registers and read it once; every other K % 8 == 0 takes the two-pass form.
 * x 16-byte, q 8-byte aligned; a bad call is ALG_EINVAL before any launch. */
int alg_quantize_fp8_rows_batched(const void* x, int64_t x_bstride, int64_t x_rstride, void* q, float* scale, int batch, int rows,
                                  int K, void* stream);

/* Full (unmasked) softmax attention, head_dim 64.
 *   q, k : bf16, element (b, s, h, d) at  base + b*q_bstride + s*q_rstride + h*64 + d   (same strides for k)
 *   vt   : bf16 V transposed, element (b, h, d, s') at base + b*vt_bstride + (h*64+d)*vt_rstride + perm(s'),
 *          perm = swap of index bits 2 and 3 (what alg_gemm_bf16 + ALG_GEMM_PERMUTE_COLS writes);
 *          columns >= S up to the next multiple of 64 must be readable and finite (zero)
 *   o    : bf16, element (b, s, h, d) at base + b*o_bstride + s*o_rstride + h*64 + d
 * softmax(q k^T * scale) v, fp32 accumulate, P rounded to bf16 before P@V. */
int alg_flash_attn_d64(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                       int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                       int64_t o_bstride, int64_t o_rstride, float scale, void* stream);

/* flags = ALG_ATTN_Q_PRESCALED: q already carries scale * log2(e) (alg_qk_norm_rope_scaled); `scale` is ignored and the
 * scores come out of the MFMA in log2 units.  flags = 0 is alg_flash_attn_d64.
 * workspace: when the (head, query-block) units of a launch leave the last round of workgroups nearly empty (C2: 840 units
 * per XCD on 64 slots), the last units are cut along KV into a second launch whose fp32 partials live in `workspace`
 * (alg_flash_attn_d64_workspace_bytes; 0 = this shape is one launch).  workspace = NULL (what alg_flash_attn_d64 passes)
 * runs everything as one launch: same result up to the fp32 summation order of those last units. */
#define ALG_ATTN_Q_PRESCALED 1
int alg_flash_attn_d64_ex(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                          int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                          int64_t o_bstride, int64_t o_rstride, float scale, int flags, void* workspace,
                          int64_t workspace_bytes, void* stream);
int64_t alg_flash_attn_d64_workspace_bytes(int batch, int heads, int S, int flags);

/* alg_flash_attn_d64_ex(ALG_ATTN_Q_PRESCALED) (the same layouts, strides and alignment; q carries scale * log2(e)) in which each
 * block of 256 queries attends to a short list of key ranges instead of to all keys: the primitive under the opt-in frame window
 * of the CogVideoX self-attention (alg_amd/attn_window.py).  One launch in the dense grid order: no split-KV tail, no workspace.
 *   kv_ranges : DEVICE table int32 [q_blocks][max_ranges][2] of (begin, end) key indices, q_blocks = ceil(S / 256); one table
 *               serves every batch item and head of the launch.  max_ranges is 1..4.
 *   A table is valid when in each block the used entries come first, sorted and disjoint, begin % 64 == 0, begin < end <= S,
 *   unused trailing entries are (0, 0), and every block has at least one key.
 * o[q] = softmax of the log2-unit scores restricted to the union of the ranges of q's block, times v, with the numerics of the
 * dense entry's single launch: a range [begin, end) is computed exactly as that launch computes a panel of end - begin keys whose
 * k / vt start at key `begin`, with the running offset, the row sum and the fp32 accumulator carried from range to range.  vt's
 * padding rule holds per range: the columns up to the next multiple of 64 behind `end` are read and multiplied by p = 0 (finite
 * values).
 * The kernel reads the table defensively -- begin / end clamped into [0, S], begin rounded down to a multiple of 64, empty
 * entries skipped, a block left without a key writes zeros -- so no table content makes it read outside the panels; a null or
 * misaligned table and max_ranges outside 1..4 are ALG_EINVAL before any launch.  ALG_ATTN_PP picks the kernel as it does for
 * the dense entry: 4 and 7 the zero-offset statement, 8 the any-offset one, 0 (or operands beyond the statements' 31-bit byte
 * offsets) the same frame with the statement switched off. */
int alg_flash_attn_d64_ranges(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                              int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                              int64_t o_bstride, int64_t o_rstride, const int32_t* kv_ranges, int max_ranges, void* stream);

/* alg_flash_attn_d64_ranges with (a) a table row per head and (b) an optional log-sum-exp output: the d = 64 twin of
 * alg_flash_attn_d128_ranges_heads below, the primitive under CogVideoX's per-head frame window chosen by recall
 * (alg_amd/attn_window.py: head_window_ranges, decide_heads).  Same kernel, same operands and checks, same defensive reading of the
 * table, the same choice by ALG_ATTN_PP, one launch; alg_flash_attn_d64_ranges IS this entry with table_heads == 1 and lse == NULL.
 *   kv_ranges   : DEVICE table int32 [table_heads][q_blocks][max_ranges][2].  table_heads is 1 (one table for every head, the
 *                 layout above) or `heads` (the workgroup of (b, h, q block) reads row h * q_blocks + q block; one table serves
 *                 every batch item).  Any other value is ALG_EINVAL.  Each head's slice obeys the rules above.
 *   lse         : NULL, or DEVICE fp32 [batch][heads][S], contiguous, 4-byte aligned (else ALG_EINVAL).  When given, the kernel
 *                 also writes once per query  lse[b][h][q] = log2( sum over the VISITED keys j of 2^(q.k_j) )  -- q is pre-scaled,
 *                 so the scores are in log2 units and no factor is applied -- as m + log2(l) from the kernel's own running offset
 *                 and row sum.  o is bit for bit what it is without lse.
 *                 Numerics: the d = 64 frames sum the bf16-ROUNDED probabilities in their C++ tile body (fdot2 over the packed P,
 *                 round to nearest), where the d = 128 kernel keeps an fp32 sum of the unrounded ones; that sum alone would put up
 *                 to one bf16 rounding, 2^-8 relative, into l (5.6e-3 into lse).  A launch with lse therefore runs instantiations
 *                 of the kernel that also carry, per query, the difference between the fp32 sum of the unrounded probabilities
 *                 and the rounded sum over those tiles, and lse is taken from their total: it has fp32 accuracy, like the d = 128
 *                 entry's (docs/numerics.md), at the price of two more additions per score pair in the C++ tile body of that
 *                 launch only.  A launch without lse runs the kernels of alg_flash_attn_d64_ranges.  alg_attn_lse_recall takes the
 *                 lse of either entry.
 * A block the table leaves without a key writes zeros to o and -inf to lse. */
int alg_flash_attn_d64_ranges_heads(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                    int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                    int64_t o_bstride, int64_t o_rstride, const int32_t* kv_ranges, int max_ranges, int table_heads,
                                    float* lse, void* stream);

/* alg_flash_attn_d64_ranges_heads in a launch order the host computed: the d = 64 twin of alg_flash_attn_d128_ranges_order below
 * (alg_amd/attn_window.py: LaunchOrder, balanced_order).  Same kernel, operands, checks and defensive reading of the table, one
 * launch of order_len workgroups.
 *   order     : DEVICE int32 [order_len], 4-byte aligned.  Entry b is the unit workgroup b runs, bh * q_blocks + qb with
 *               bh = b_item * heads + h and q_blocks = ceil(S / 256), or a negative value for a workgroup that exits at once.
 *   order_len : a multiple of 8, at least batch * heads * q_blocks (entries 8 i + x share dispatch lane x, as blocks 8 i + x of the
 *               other entries do).
 * A null or misaligned order, an order_len that is no multiple of 8 or smaller than batch * heads * q_blocks are ALG_EINVAL before
 * any launch.  The kernel reads the entry defensively: a value outside [0, batch * heads * q_blocks) makes the workgroup exit, so no
 * content of `order` makes it read or write outside the operands.  The order has to hold every unit exactly once for o (and lse) to
 * be complete -- a unit that is missing leaves its rows unwritten, one that occurs twice is computed twice with the same bits;
 * attn_window.LaunchOrder validates that on the host.  Every workgroup computes exactly what the workgroup of that unit computes in
 * alg_flash_attn_d64_ranges_heads: o and lse are that entry's BIT FOR BIT for every valid order; only the time differs.
 * Enqueue-only and allocation-free. */
int alg_flash_attn_d64_ranges_order(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int S,
                                    int64_t q_bstride, int64_t q_rstride, int64_t vt_bstride, int64_t vt_rstride,
                                    int64_t o_bstride, int64_t o_rstride, const int32_t* kv_ranges, int max_ranges, int table_heads,
                                    float* lse, const int32_t* order, int order_len, void* stream);

/* wan:910-917 (WanTransformer3DModel self- and cross-attention, head_dim 128; diffusers WanAttnProcessor SDPA)
 * Same contract as alg_flash_attn_d64 with head_dim 128 and separate query / key lengths:
 *   q : element (b, s, h, d) at q + b*q_bstride + s*q_rstride + h*128 + d,  s < Sq
 *   k : likewise with k_bstride / k_rstride, s < Skv
 *   vt: V transposed, element (b, h, d, s) at vt + b*vt_bstride + (h*128 + d)*vt_rstride + perm(s), perm swaps index
 *       bits 2 and 3 (what alg_gemm_bf16 writes with ALG_GEMM_PERMUTE_COLS); vt_rstride >= Skv rounded up to 64 and the
 *       padding columns must hold finite values (they are multiplied by p = 0)
 *   o : element (b, s, h, d) at o + b*o_bstride + s*o_rstride + h*128 + d */
int alg_flash_attn_d128(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq, int Skv,
                        int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride, int64_t vt_bstride,
                        int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale, void* stream);

/* The same kernel with grouped-query attention (kv_group query heads share one K / V head; k and vt then hold heads / kv_group
 * heads) and an optional causal mask (query i sees keys 0..i; needs Sq == Skv): the Llama-3 tower of HunyuanVideo's prompt
 * encoder (reference pipeline_hunyuan_video_image2video_lowpass.py:282-420, transformers LlavaForConditionalGeneration). */
int alg_flash_attn_d128_ex(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq, int Skv,
                           int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride, int64_t vt_bstride,
                           int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale, int kv_group, int causal,
                           void* stream);

/* alg_flash_attn_d128 (non-causal, ungrouped, bf16; the same layouts, strides and alignment) in which each block of 256 queries
 * attends to a short list of key ranges instead of to all keys: the primitive under the opt-in frame window of the Wan and
 * HunyuanVideo self-attention (alg_amd/attn_window.py).  Always the 64-queries-per-wave kernel (attention128_q64.hip), any Skv.
 *   kv_ranges : DEVICE table int32 [q_blocks][max_ranges][2] of (begin, end) key indices, q_blocks = ceil(Sq / 256); one table
 *               serves every batch item and head of the launch.  max_ranges is 1..4.
 *   A table is valid when in each block the used entries come first, sorted and disjoint, begin % 64 == 0, begin < end <= Skv,
 *   unused trailing entries are (0, 0), and every block has at least one key.
 * o[q] = softmax(scale * q k^T restricted to the union of the ranges of q's block) v, with the numerics of alg_flash_attn_d128: a
 * range [begin, end) is computed exactly as that entry computes a panel of end - begin keys whose k / vt start at key `begin`, with
 * the running max, the row sum and the fp32 accumulator carried from range to range.  vt's padding rule holds per range: the
 * columns up to the next multiple of 64 behind `end` are read and multiplied by p = 0 (finite values).
 * The kernel reads the table defensively -- begin / end clamped into [0, Skv], begin rounded down to a multiple of 64, empty
 * entries skipped, a block left without a key writes zeros -- so no table content makes it read outside the panels; a null or
 * misaligned table and max_ranges outside 1..4 are ALG_EINVAL before any launch.  ALG_ATTN128_Q64=3 runs it with the generated
 * statement switched off (tests); the other values of that variable do not route this entry anywhere else. */
int alg_flash_attn_d128_ranges(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq, int Skv,
                               int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride, int64_t vt_bstride,
                               int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale, const int32_t* kv_ranges,
                               int max_ranges, void* stream);

/* alg_flash_attn_d128_ranges with (a) a table row per head and (b) an optional log-sum-exp output: the primitives under the
 * per-head frame window chosen by recall (alg_amd/attn_window.py: head_window_ranges, decide_heads).  Same kernel, same operands,
 * same defensive reading of the table, and with table_heads == 1 and lse == NULL the bits of alg_flash_attn_d128_ranges.
 *   kv_ranges   : DEVICE table int32 [table_heads][q_blocks][max_ranges][2].  table_heads is 1 (one table for every head, the
 *                 layout above) or `heads` (the workgroup of (b, h, q block) reads row h * q_blocks + q block; one table serves
 *                 every batch item).  Any other value is ALG_EINVAL.  Each head's slice obeys the rules above.
 *   lse         : NULL, or DEVICE fp32 [batch][heads][Sq], contiguous, 4-byte aligned (else ALG_EINVAL).  When given, the kernel
 *                 also writes once per query  lse[b][h][q] = log2( sum over the VISITED keys j of 2^(c * q.k_j) ),
 *                 c = scale * log2(e): the log2-domain log-sum-exp of the scaled scores, from the kernel's own running max and
 *                 fp32 row sum (m * c + log2(l); docs/numerics.md).  o is bit for bit what it is without lse.
 * A block the table leaves without a key writes zeros to o and -inf to lse. */
int alg_flash_attn_d128_ranges_heads(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq, int Skv,
                                     int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride,
                                     int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale,
                                     const int32_t* kv_ranges, int max_ranges, int table_heads, float* lse, void* stream);

/* alg_flash_attn_d128_ranges_heads in a launch order the host computed (alg_amd/attn_window.py: LaunchOrder, balanced_order).  The
 * other ranged entries map workgroup b to the unit (bh = (b >> 3) / q_blocks * 8 + (b & 7), qb = (b >> 3) % q_blocks): heads dealt
 * to the eight dispatch lanes by bh % 8, units head-major.  With a per-head table a dense head's units cost several times a
 * windowed head's, and that order neither starts the long units first nor evens out the lanes.  Here workgroup b runs unit
 * order[b].  Same kernel, operands, checks and defensive reading of the table; one launch of order_len workgroups.
 *   order     : DEVICE int32 [order_len], 4-byte aligned.  Entry b is bh * q_blocks + qb with bh = b_item * heads + h and
 *               q_blocks = ceil(Sq / 256), or a negative value for a workgroup that exits at once.
 *   order_len : a multiple of 8, at least batch * heads * q_blocks (entries 8 i + x share dispatch lane x).
 * A null or misaligned order, an order_len that is no multiple of 8 or smaller than batch * heads * q_blocks are ALG_EINVAL before
 * any launch; an order_len beyond the 31-bit grid is ALG_ELIMIT.  The kernel reads the entry defensively: a value outside
 * [0, batch * heads * q_blocks) makes the workgroup exit, so no content of `order` makes it read or write outside the operands.
 * The order has to hold every unit exactly once for o (and lse) to be complete -- a missing unit leaves its rows unwritten, one
 * that occurs twice is computed twice with the same bits; attn_window.LaunchOrder validates that on the host.  Every workgroup
 * computes exactly what the workgroup of that unit computes in alg_flash_attn_d128_ranges_heads: o and lse are that entry's BIT FOR
 * BIT for every valid order; only the time differs.  No workgroup talks to another: the order is data.  Enqueue-only and
 * allocation-free. */
int alg_flash_attn_d128_ranges_order(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq, int Skv,
                                     int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride,
                                     int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale,
                                     const int32_t* kv_ranges, int max_ranges, int table_heads, float* lse, const int32_t* order,
                                     int order_len, void* stream);

/* alg_flash_attn_d128_ranges_heads over a table of up to 12 SEGMENTS that writes, instead of one lse, the log-sum-exp of the keys
 * visited SO FAR behind every segment: the one-pass calibration of the per-head window width (alg_amd/attn_window.py:
 * frame_profile_segments, decide_widths).  Same frame, operands, checks, defensive reading of the table and shape limits; an
 * instantiation of its own, so the kernels of the other entries are what they were.
 *   kv_ranges    : DEVICE table int32 [table_heads][q_blocks][max_segments][2], max_segments in 1..12 (the other entries: 1..4).
 *                  The kernel visits a row's segments in table order; empty entries (end <= begin) may stand ANYWHERE and are
 *                  skipped.
 *   lse_prefix   : DEVICE fp32 [batch][heads][max_segments][Sq], contiguous, 4-byte aligned, not NULL (else ALG_EINVAL).  Behind
 *                  segment i, visited or skipped, the kernel writes once per query
 *                      lse_prefix[b][h][i][q] = log2( sum over the keys j of the segments 0 .. i of 2^(c * q.k_j) )
 *                  from its running max and fp32 row sum (m * c + log2(l)), -inf while no key has been visited.
 * o is written from the final state as in the other entries.  lse_prefix[b][h][max_segments - 1] is BIT FOR BIT the lse of
 * alg_flash_attn_d128_ranges_heads for the same table, and o is that entry's o (for tables that entry takes).  When the segments
 * of every row partition [0, Skv) the launch is the dense attention: the exact softmax over all keys in another fp32 summation
 * grouping than alg_flash_attn_d128's (docs/numerics.md).  Enqueue-only and allocation-free. */
int alg_flash_attn_d128_ranges_prefix(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int Sq, int Skv,
                                      int64_t q_bstride, int64_t q_rstride, int64_t k_bstride, int64_t k_rstride,
                                      int64_t vt_bstride, int64_t vt_rstride, int64_t o_bstride, int64_t o_rstride, float scale,
                                      const int32_t* kv_ranges, int max_segments, int table_heads, float* lse_prefix,
                                      void* stream);

/* Softmax mass per segment from the prefixes of alg_flash_attn_d128_ranges_prefix, fp32 [panels][segments][Sq] with panels = batch *
 * heads.  With P_i = lse_prefix[p][i][q], P_last = P_(segments - 1) and P_(-1) = -inf:
 *   out[p][i] = mean over q in [row0, row0 + rows) of exp2(P_i - P_last) - exp2(P_(i-1) - P_last),  exp2(-inf - x) being 0
 * i.e. the fraction of the softmax mass of panel p's queries that lies on the keys of segment i.  out is DEVICE double
 * [panels][segments], 8-byte aligned.  One launch; double exp2 and double accumulation in a fixed two-level order (per lane in
 * row order, then across the lanes of the (panel, segment)'s workgroup), no atomics: run-to-run bit-identical.  segments in 1..12,
 * 0 <= row0, rows >= 1, row0 + rows <= Sq, else ALG_EINVAL. */
int alg_attn_prefix_mass(const float* lse_prefix, double* out, int panels, int segments, int Sq, int row0, int rows, void* stream);

/* Recall of a key subset from two lse outputs of alg_flash_attn_d128_ranges_heads or of alg_flash_attn_d64_ranges_heads (it knows
 * nothing of the head dimension) over the same queries (lse_part: the subset, lse_full: all keys), both fp32 [panels][Sq] with
 * panels = batch * heads:
 *   out[p] = mean over q in [row0, row0 + rows) of exp2f(lse_part[p][q] - lse_full[p][q]),  a term being 0 where lse_part is -inf
 * i.e. the fraction of the softmax mass of panel p's queries that lies on the subset.  out is DEVICE double [panels], 8-byte
 * aligned.  One launch for all panels; fp32 exp2, double accumulation in a fixed two-level order (per lane, then across the lanes
 * of the panel's workgroup): run-to-run bit-identical.  0 <= row0, rows >= 1, row0 + rows <= Sq, else ALG_EINVAL. */
int alg_attn_lse_recall(const float* lse_part, const float* lse_full, double* out, int panels, int Sq, int row0, int rows,
                        void* stream);

/* Layout moves under the position-major band attention (alg_amd/attn_window.py: position_band_ranges; attn_layout.hip).  A video
 * latent's tokens lie frame by frame, s = f * hw + p; in the position-major order pi(s) = p * frames + f the keys "the same and the
 * neighbouring positions in every frame" are ONE contiguous run, which alg_flash_attn_d128_ranges takes.  Both entries are pure
 * moves of bf16 (or any 2-byte) elements, bit-exact, for the heads named by
 *   head_list : DEVICE int32 [n_sel], 4-byte aligned: DISTINCT head indices of the wide tensor, in any order (the kernels do not
 *               check its contents: alg_amd/attn_window.py: HeadList validates them before the upload).
 * head_dim (hd) is 64 or 128; S = frames * hw.  Strides in elements, multiples of 8; src / dst 16-byte aligned.  Null or
 * misaligned pointers, head_dim, n_sel / batch / frames / hw < 1, inverse outside {0, 1} and strides that cannot hold the
 * tensors are ALG_EINVAL before any launch.  16-byte accesses, a capped grid with a grid-stride loop, no atomics; enqueue-only
 * and allocation-free.
 *
 * alg_attn_rows_position_major: Q, K (inside a [Q | K] buffer: a base offset and the row stride) and O.
 *   inverse = 0 (gather into a compact buffer):  dst[b][pi(s)][j*hd + d] = src[b][s][head_list[j]*hd + d]
 *   inverse = 1 (scatter back):                  dst[b][s][head_list[j]*hd + d] = src[b][pi(s)][j*hd + d]
 *   Element (b, row, c) of either tensor is at base + b*bstride + row*rstride + c.  inverse = 1 writes the selected heads' slices
 *   only: every other byte of dst keeps its value.  Row strides >= n_sel * hd.
 *
 * alg_attn_vt_position_major: V^T, whose key axis carries perm (index bits 2 and 3 swapped: ALG_GEMM_PERMUTE_COLS).
 *   dst[b][j*hd + d][perm(pi(s))] = src[b][head_list[j]*hd + d][perm(s)]  for s < S;  the columns S .. S rounded up to 64 of dst
 *   are written as ZERO.  Row strides >= S rounded up to 64; the columns of src up to S rounded up to 16 are read.  The key axis
 *   is transposed through LDS, so reads and writes both go out as whole 16-byte chunks along a row. */
int alg_attn_rows_position_major(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst, int64_t dst_bstride,
                                 int64_t dst_rstride, const int32_t* head_list, int n_sel, int head_dim, int batch, int frames,
                                 int hw, int inverse, void* stream);
int alg_attn_vt_position_major(const void* src, int64_t src_bstride, int64_t src_rstride, void* dst, int64_t dst_bstride,
                               int64_t dst_rstride, const int32_t* head_list, int n_sel, int head_dim, int batch, int frames,
                               int hw, void* stream);

/* Opt-in e4m3 form of alg_flash_attn_d128 on v_mfma_scale_f32_32x32x64_f8f6f4 (attention128_fp8.hip): non-causal, ungrouped
 * (kv_group != 1 or causal != 0 is ALG_EINVAL), separate Sq / Skv, ragged last tile, bf16 output; strides in elements = bytes.
 *   q  : OCP e4m3, element (b, s, h, d) at q + b*q_bstride + s*q_rstride + h*128 + d;  q_scale: float32 [batch][Sq][heads]
 *        (what alg_quantize_fp8_rows writes for rows of 128 of a contiguous [batch][Sq][heads * 128] tensor)
 *   k  : likewise with k_bstride / k_rstride;  k_scale: float32 [batch][heads], ONE scale per (batch, head) (alg_quantize_fp8_khead)
 *   vt : OCP e4m3 V transposed in the kernel's key order (alg_quantize_fp8_vt): element (b, h, d, s) at
 *        vt + b*vt_bstride + (h*128 + d)*vt_rstride + 64*(s / 64) + perm(s % 64),  perm(32 sub + 8 g + 4 h2 + j) = 32 h2 + 16 sub + 4 g + j
 *        (sub, h2 < 2; g, j < 4); vt_rstride >= Skv rounded up to 64 and the padding columns must not hold the e4m3 NaN byte
 *        (they are multiplied by p = 0; alg_quantize_fp8_vt writes zeros);
 *        vt_scale: float32 [batch][heads * 128], one scale per row
 *   o  : bf16, element (b, s, h, d) at o + b*o_bstride + s*o_rstride + h*128 + d
 * o = softmax(scale * (q_scale q)(k_scale k)^T) (vt_scale vt)^T with fp32 accumulation, P rounded to e4m3 at a fixed scale of 2^3
 * (docs/numerics.md).  q / k / vt 16-byte aligned with strides % 16 == 0, vt_scale 16-byte, o 8-byte aligned (strides % 4 == 0). */
int alg_flash_attn_d128_fp8(const void* q, const float* q_scale, const void* k, const float* k_scale, const void* vt,
                            const float* vt_scale, void* o, int batch, int heads, int Sq, int Skv, int64_t q_bstride,
                            int64_t q_rstride, int64_t k_bstride, int64_t k_rstride, int64_t vt_bstride, int64_t vt_rstride,
                            int64_t o_bstride, int64_t o_rstride, float scale, int kv_group, int causal, void* stream);

/* K operand of alg_flash_attn_d128_fp8: x bf16 (b, s, h, d) at x + b*x_bstride + s*x_rstride + h*128 + d becomes e4m3 bytes at
 * q + b*q_bstride + s*q_rstride + h*128 + d with ONE scale per (batch, head): scale[b*heads + h] = max|x| / 448 over the head's
 * S x 128 values (1 if all zero), q = e4m3(clamp(x * (1 / scale))) -- the arithmetic of alg_quantize_fp8_rows at that granularity.
 * scale_given != 0: scale[] is an INPUT (a bound known beforehand; values beyond it saturate at +-448) and only the conversion runs.
 * x 16-byte, q 8-byte aligned; strides % 8 == 0. */
int alg_quantize_fp8_khead(const void* x, int64_t x_bstride, int64_t x_rstride, void* q, int64_t q_bstride, int64_t q_rstride,
                           float* scale, int batch, int heads, int S, int scale_given, void* stream);

/* alg_rmsnorm_rope / alg_headnorm_rope in front of alg_flash_attn_d128_fp8: the same arguments and arithmetic, but x is only
 * read and the result goes out as OCP e4m3 -- q8 element (row, c) at q8 + row*q8_rstride + c (alg_rmsnorm_rope_fp8; row counts
 * through the batch) or (b, tok, c) at q8 + b*q8_bstride + tok*q8_rstride + c (alg_headnorm_rope_fp8) -- bit for bit what a
 * quantiser pass makes of the bf16 tensor the bf16 kernel writes, without that tensor going through memory:
 *   head_scale == NULL: one scale per (token, head) = max|head vector| / 448 (1 if zero), written to scale[row*heads + head]
 *                       (alg_headnorm_rope_fp8: scale[b*scale_bstride + tok*heads + head]): alg_quantize_fp8_rows on rows of 128;
 *   head_scale != NULL: float32 [batch][heads], the scale of (b, head) is READ from it and `scale` is not touched:
 *                       alg_quantize_fp8_khead with scale_given = 1.
 * x 16-byte, q8 8-byte aligned; q8_rstride % 8 == 0. */
int alg_rmsnorm_rope_fp8(const void* x, const void* weight, const float* cos_tab, const float* sin_tab, int64_t x_rstride,
                         int batch, int rows, int D, float eps, void* q8, int64_t q8_rstride, float* scale,
                         const float* head_scale, void* stream);
int alg_headnorm_rope_fp8(const void* x, const void* weight, const float* cos_tab, const float* sin_tab, int64_t x_rstride,
                          int64_t x_bstride, int batch, int rows, int heads, int rope_tokens, float eps, void* q8,
                          int64_t q8_rstride, int64_t q8_bstride, float* scale, int64_t scale_bstride, const float* head_scale,
                          void* stream);

/* V^T operand of alg_flash_attn_d128_fp8: `rows` (= heads * 128) bf16 rows per batch at x + b*x_bstride + r*x_rstride become e4m3
 * rows at q + b*q_bstride + r*q_rstride in the kernel's key order (see above), scale[b*rows + r] = max|x[r][s < Skv]| / 448 (1 if
 * zero).  src_permuted = 1: x holds key s at the column alg_gemm_bf16 + ALG_GEMM_PERMUTE_COLS writes (index bits 2 and 3
 * swapped), 0: at column s.  Columns Skv .. Skv rounded up to 64 of x are never used (they must be readable) and are written as
 * ZERO.  Both row strides >= Skv rounded up to 64 and % 8 == 0; x 16-byte, q 8-byte aligned. */
int alg_quantize_fp8_vt(const void* x, int64_t x_bstride, int64_t x_rstride, void* q, int64_t q_bstride, int64_t q_rstride,
                        float* scale, int batch, int rows, int Skv, int src_permuted, void* stream);

/* Two key / value sets for the same queries, the two attention outputs added: the image + text cross-attention of the Wan I2V DiT
 * (wan:910-917 calls WanTransformer3DModel; its attention processor computes sdpa(q, k_img, v_img) + sdpa(q, k, v) on bf16 tensors)
 * as ONE launch -- o = bf16(bf16(attn(q, k, vt)) + bf16(attn(q, k2, vt2))), bit for bit what two alg_flash_attn_d128 calls and
 * alg_lincomb give.  Layouts as alg_flash_attn_d128; both sets are meant to be short (encoder tokens). */
int alg_flash_attn_d128_dual(const void* q, const void* k, const void* vt, int Skv, int64_t k_bstride, int64_t k_rstride,
                             int64_t vt_bstride, int64_t vt_rstride, const void* k2, const void* vt2, int Skv2, int64_t k2_bstride,
                             int64_t k2_rstride, int64_t vt2_bstride, int64_t vt2_rstride, void* o, int batch, int heads, int Sq,
                             int64_t q_bstride, int64_t q_rstride, int64_t o_bstride, int64_t o_rstride, float scale, void* stream);

/* Llama rotary embedding ("rotate_half" form) in place on x [rows][heads][128] bf16 (row stride x_rstride elements):
 * x' = x * cos[pos[r]] + rotate_half(x) * sin[pos[r]], every product and the sum rounded to bf16 like the eager graph;
 * cos / sin: fp32 tables [positions][128]; pos: int32 [rows]. */
int alg_rope_half(void* x, const float* cos_tab, const float* sin_tab, const int* pos, int64_t rows, int heads,
                  int64_t x_rstride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Text encoders of the conditioning front-end (transformers T5EncoderModel, cog:228-268 `_get_t5_prompt_embeds`;
 * UMT5EncoderModel, wan:185-234 `_get_t5_prompt_embeds`): the small kernels around alg_gemm_bf16
 * ------------------------------------------------------------------------------------------------ */

/* out[r][:] = table[ids[r]][:]  (nn.Embedding; ids int64, clamped into [0, vocab)), rows of D bf16, D % 8 == 0. */
int alg_embed_rows(const int64_t* ids, const void* table, void* out, int64_t n, int D, int vocab, void* stream);

/* T5LayerNorm: y = bf16( bf16(x * rsqrt(mean(x^2) + eps)) * weight ), variance in fp32, no mean subtraction, no bias. */
int alg_t5_layernorm(const void* x, const void* weight, void* y, int64_t rows, int D, float eps, void* stream);

/* T5Attention / CLIPAttention (eager graph; head_dim 64 with L <= 512, or 80 with L <= 448): for batch b, head h
 *   s = bf16(q k^T) [* scale -> bf16]  + bias_table[rel_bucket[j - i + L - 1]][h] -> bf16;  masked keys (key_mask[b][j]
 *   == 0) get probability 0, and with `causal` keys j > i too (CLIPTextModel);  p = bf16(softmax_fp32(s));  out = bf16(p v)
 * q / k / v: element (b, i, h, d) at ptr + (b*L + i)*qkv_rstride + h*head_dim + d (three pointers into one fused QKV buffer);
 * out likewise with out_rstride; bias_table: [buckets][heads] bf16 (relative_attention_bias.weight) or NULL;
 * rel_bucket: int32 [2L - 1], the bucket of relative position (key - query); key_mask: int32 [batch][L] or NULL.
 * A query row without a surviving key (all of its keys masked or causally excluded) is written as zeros (either sign), where
 * the eager graph gives NaN.  Masked k / v rows are read and multiplied by p = 0: they must be finite.  Nothing outside
 * out[(b*L + i)*out_rstride + [0, heads*head_dim)] is written.
 * ALG_EINVAL before any launch: L <= 0, L above the limit, another head_dim, qkv_rstride % 8 != 0, a bias_table without
 * rel_bucket, k or v not 16-byte aligned (they are read 16 bytes at a time; q and out may sit on any element).  batch == 0
 * returns ALG_OK and touches nothing. */
int alg_attn_bias(const void* q, const void* k, const void* v, void* out, const void* bias_table, const int* rel_bucket,
                  const int* key_mask, int batch, int heads, int head_dim, int L, int64_t qkv_rstride, int64_t out_rstride,
                  float scale, int causal, void* stream);

/* CLIPTextModel's `quick_gelu` (hy:421-452 `text_encoder_2`): x = bf16(x * bf16(sigmoid(bf16(1.702 x)))), in place. */
int alg_quick_gelu(void* x, int64_t numel, void* stream);

/* out = bf16(a * b) (T5DenseGatedActDense: gelu_new(wi_0 x) * wi_1 x). */
int alg_mul_bf16(const void* a, const void* b, void* out, int64_t numel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * AutoencoderKLCogVideoX decoder (diffusers; call site cog:428-433 `frames = self.vae.decode(latents).sample`)
 * Activations are channels-last bf16 over a padded grid (Hp, Wp) = (H + 2, W + 2):
 *   padded  [T + 2][Hp][Wp][C]  zero borders, frames 0 and 1 repeat frame 0 (causal padding)  -- convolution input
 *   virtual [T][Hp][Wp][C]      rows with y >= H or x >= W are don't-care                      -- convolution output
 * ------------------------------------------------------------------------------------------------ */

/* CogVideoXCausalConv3d (kt = 3: 3x3x3, first frame repeated twice in front, zero spatial padding) and the upsamplers'
 * Conv2d 3x3 (kt = 1), as one implicit-GEMM launch on the MFMA GEMM kernel:
 *   x : padded input [frames + kt - 1][Hp][Wp][Cin], readable for 2*Wp + 2 rows past its end
 *   w : [Cout][kt*9][Cin] bf16 (tap-major (dt, dy, dx), channels innermost);  bias: [Cout] or NULL
 *   y : virtual output [frames][Hp][Wp][Cout];  res: optional residual in y's layout, y = res + conv (may alias y)
 * Output row r of frame t is the sum over (dt, dy, dx, c) of x[(t + dt)*Hp*Wp + r + dy*Wp + dx][c] * w[o][(dt, dy, dx)][c],
 * accumulated in fp32; y = bf16(sum + bias), and with a residual y = bf16(res + bf16(sum + bias)) -- the convolution's bf16
 * result, then the add, as two torch ops round.  Rows with y < H and x < W never read x's slack or res's don't-care rows.
 * Cin a power of two >= 64 (pad thinner inputs with zero channels), Cout % 4 == 0.
 * mode ALG_CONV_PAIR (Cout <= 128; the GEMM tile is 256 columns wide): one GEMM row produces TWO neighbouring voxels, so a
 * 128-channel convolution fills the tile: w is then [2*Cout][kt*3*4][Cin] with rows [0, Cout) = the kernel at dx 0..2
 * (dx 3 zero) and rows [Cout, 2*Cout) = the kernel at dx 1..3 (dx 0 zero), bias is [2*Cout] (the bias twice), Hp*Wp must
 * be even, and x must be readable for 2*Wp + 3 rows past its end.  Same results, 4/3 of the useful MFMA work instead of 2x.
 * mode ALG_CONV_STRIDE2 (kt = 1; CogVideoXDownsample3D: pad (0,1,0,1) + Conv2d k3 s2 p0): x is the padded input of the
 * [H][W] activation (H, W even), y has (H/2)*Wp rows per frame -- output (Y, X) at row Y*Wp + X, i.e. at the INPUT's pitch
 * (alg_vae_repitch moves it to the standard layout of the half-resolution level). */
#define ALG_CONV_PLAIN 0
#define ALG_CONV_PAIR 1
#define ALG_CONV_STRIDE2 2
int alg_conv_cl_bf16(const void* x, const void* w, const void* bias, const void* res, void* y, int frames, int Hp,
                     int Wp, int Cin, int Cout, int kt, int mode, void* stream);

typedef struct alg_vae_geom {
  int32_t frames, H, W, C;     /* activation extent; C a power of two in [128, 2048] (32 groups) */
  int32_t first_len, seg_len;  /* GroupNorm segments in frames: [0, first_len), then seg_len each -- the published decoder
                                  normalises each batch of latent frames (3 first, then 2) on its own */
  int32_t lat_first_single;    /* frame t came from latent frame (t ? 1 + (t-1)/lat_rate : 0) if set, else t/lat_rate */
  int32_t lat_rate, lat_scale; /* temporal and spatial upsampling factors relative to the latent */
  int32_t lat_h, lat_w;        /* latent grid (the conditioning tensor is padded: [L + 2][lat_h + 2][lat_w + 2][2C]) */
} alg_vae_geom;

/* GroupNorm(32 groups) statistics of a virtual-layout activation per (segment, group): stats[seg][32][2] = (mean, rstd).
 * Deterministic (fixed-order partial sums, final reduction in double).  workspace: alg_vae_groupnorm_workspace() bytes. */
int64_t alg_vae_groupnorm_workspace(const alg_vae_geom* g);
int alg_vae_groupnorm_stats(const void* x, const alg_vae_geom* g, float eps, void* workspace, float* stats, void* stream);

/* CogVideoXSpatialNorm3D (+ SiLU): out = act(GroupNorm(x) * conv_y(zq) + conv_b(zq)), virtual -> padded.  zyb holds
 * [conv_y(zq) | conv_b(zq)] (2C channels) at latent resolution in the padded latent layout; each tensor op rounds to bf16
 * as the eager reference does. */
int alg_vae_spatial_norm(const void* x, const float* stats, const void* gamma, const void* beta, const void* zyb,
                         void* out, const alg_vae_geom* g, int silu, void* stream);

/* The encoder's plain GroupNorm (+ SiLU), virtual -> padded: same kernel without the conditioning (lat_* ignored). */
int alg_vae_group_norm(const void* x, const float* stats, const void* gamma, const void* beta, void* out,
                       const alg_vae_geom* g, int silu, void* stream);

/* virtual -> padded copy (zero borders, causal frames), for convolutions that read an un-normalised activation. */
int alg_vae_pad(const void* x, void* out, int frames, int H, int W, int C, void* stream);

/* Rows written at another pitch (ALG_CONV_STRIDE2: src_rows rows per frame, src_wp per line) -> the standard virtual
 * layout [frames][H + 2][W + 2][C]. */
int alg_vae_repitch(const void* x, void* out, int frames, int H, int W, int C, int src_rows, int src_wp, void* stream);

/* virtual [frames][H+2][W+2][C] -> planes [C][frames][H][W] bf16 (the encoder's moments, `AutoencoderKLCogVideoX.encode`). */
int alg_vae_unpack_planes(const void* x, void* out, int frames, int H, int W, int C, void* stream);

/* CogVideoXUpsample3D nearest-neighbour part: virtual [T][H+2][W+2][C] -> padded [frames_out][2H+2][2W+2][C] (no time
 * padding, the convolution that follows is 2-D); compress_time doubles every frame but the first (first_single) . */
int alg_vae_upsample(const void* x, void* out, int frames_out, int H, int W, int C, int compress_time, int first_single,
                     void* stream);

/* cog:429-430: z element (c, l, y, x) at z + c*c_stride + l*frame_stride + y*w + x, times `scale` (1 / scaling_factor,
 * one bf16 rounding) -> padded [frames + 2][h + 2][w + 2][64] with channels >= `channels` zero. */
int alg_vae_pack_latent(const void* z, int64_t c_stride, int64_t frame_stride, void* out, int frames, int h, int w,
                        int channels, float scale, void* stream);

/* virtual [frames][H+2][W+2][4] (RGB + pad channel) -> bf16 [3][frames][H][W] (decode().sample) or, with to_uint8, the
 * writer's uint8 [frames][H][W][3] (VideoProcessor.postprocess_video + run:121-125). */
int alg_vae_unpack_video(const void* x, void* out, int frames, int H, int W, int to_uint8, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HunyuanVideo DiT building blocks (diffusers HunyuanVideoTransformer3DModel; call site hy:1243-1252)
 * ------------------------------------------------------------------------------------------------ */

/* HunyuanVideoAttnProcessor2_0 qk norm (RMSNorm over each 128-wide head, weight [128]) + rotary embedding, in place:
 * row r of batch b = heads*128 bf16 at x + b*x_bstride + r*x_rstride; rope = x*cos + rot(x)*sin on interleaved pairs
 * with fp32 tables [rope_tokens][128], applied to rows r < rope_tokens only (latent tokens; text tokens follow them). */
int alg_headnorm_rope(void* x, const void* weight, const float* cos_tab, const float* sin_tab, int64_t x_rstride,
                      int64_t x_bstride, int batch, int rows, int heads, int rope_tokens, float eps, void* stream);

/* HunyuanVideoTokenRefiner pooled prompt: out[b][d] = mean over the first valid[b] tokens of x[b][.][d] (bf16). */
int alg_masked_mean(const void* x, const int* valid, void* out, int batch, int L, int D, void* stream);

/* y = silu(x) on bf16 (AdaLayerNormZero: linear(silu(emb))). */
int alg_silu(const void* x, void* y, int64_t numel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Wan 2.1 DiT building blocks (diffusers WanTransformer3DModel; call site wan:910-917)
 * ------------------------------------------------------------------------------------------------ */

/* WanTransformerBlock norm1/norm2/norm3, norm_out:  y = bf16( FP32LayerNorm(x) [* weight + bias] [* (1 + scale[b]) +
 * shift[b]] ), the whole chain in fp32.  x, y: [batch][rows][D] bf16 contiguous; weight/bias: [D] float32 or NULL;
 * scale/shift: float32 vectors of batch b at scale + b*mod_bstride (NULL = no modulation).  Register-resident rows when
 * D % 512 == 0 (D/512 in {1,2,3,4,6,8,10,12}), a strided three-pass kernel otherwise. */
int alg_layernorm_mod_f32(const void* x, void* y, const float* weight, const float* bias, const float* scale,
                          const float* shift, int64_t mod_bstride, int batch, int rows, int D, float eps, void* stream);

/* The same norm feeding an fp8 GEMM: instead of the bf16 tensor, writes what alg_quantize_fp8_rows would make of it
 * (q8: [batch*rows][D] OCP e4m3 bytes, q8_scale: [batch*rows] float32 = amax / 448 of the bf16-rounded row), bit for bit,
 * without the bf16 round trip through HBM.  D % 512 == 0 only. */
int alg_layernorm_mod_f32_fp8(const void* x, void* q8, float* q8_scale, const float* weight, const float* bias,
                              const float* scale, const float* shift, int64_t mod_bstride, int batch, int rows, int D,
                              float eps, void* stream);

/* WanAttnProcessor norm_q / norm_k (RMSNorm across all heads) + rotary embedding, in place:
 *   x = rope( bf16( bf16(x * rsqrt(mean(x^2) + eps)) * weight ) ),  x: [batch*rows] rows of D bf16 at stride x_rstride;
 * rope multiplies the interleaved pairs (2j, 2j+1) of every 128-wide head by cos/sin[token][j] (fp32 tables [rows][64],
 * token = row % rows); cos_tab NULL = no rope (cross-attention q, text / image k). */
int alg_rmsnorm_rope(void* x, const void* weight, const float* cos_tab, const float* sin_tab, int64_t x_rstride,
                     int batch, int rows, int D, float eps, void* stream);

/* out[l][b][j][d] = table[l][j][d] + float(vec[b][(vec_per_j ? j*D : 0) + d]):  (scale_shift_table + temb.float()) of
 * every block in one launch (J = 6, vec = timestep_proj), and of the output head (J = 2, vec = temb). */
int alg_wan_modulation(const float* table, const void* vec, float* out, int layers, int batch, int J, int D,
                       int vec_per_j, void* stream);

/* Conv3d(kernel = stride = (1, ph, pw)) patch gather: out[n][(f, gy, gx)][c*ph*pw + py*pw + px] = in[n][c][f][..][..],
 * row length Kpad >= C*ph*pw (zero padded so the patch-embed GEMM sees K % 64 == 0). */
int alg_patchify3d(const void* in, void* out, int n, int C, int F, int H, int W, int ph, int pw, int Kpad, void* stream);

/* proj_out rows (row stride ldin) -> [n][C][F][H][W] bf16; the row holds (py*pw + px)*C + c (Wan, channel_major = 0) or
 * c*ph*pw + py*pw + px (HunyuanVideo, channel_major = 1). */
int alg_unpatchify3d(const void* in, int64_t ldin, void* out, int n, int C, int F, int H, int W, int ph, int pw,
                     int channel_major, void* stream);

/* Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) in float32: out[n][dim] = [cos | sin]. */
int alg_timestep_embedding_f32(const float* t, float* out, int n, int dim, void* stream);

/* float32 linear for the modules diffusers keeps in fp32 (time_embedder): y = act(x W^T + b), x [M][K], W [N][K];
 * act 0 none, 1 SiLU.  Any of y (fp32), y_bf16 (= bf16(y)), y_silu_bf16 (= bf16(silu(bf16(y)))) may be NULL. */
int alg_linear_f32(const float* x, const float* W, const float* b, float* y, void* y_bf16, void* y_silu_bf16, int M,
                   int N, int K, int act, void* stream);

/* exact (erf) GELU in place on bf16 (WanImageEmbedding feed-forward). */
int alg_gelu_erf(void* x, int64_t numel, void* stream);

/* y = LayerNorm(x; weight, bias, eps) * (1 + scale[seg]) + shift[seg]       (CogVideoXLayerNormZero / AdaLayerNorm)
 * x, y: [batch][rows][D] bf16, rows contiguous, batch strides x_bstride / y_bstride (elements);
 * weight/bias: [D] bf16 (may be NULL);
 * scale/shift: [batch][2][D] bf16 at batch stride mod_bstride (seg 0 = rows < seg_split, seg 1 = the rest),
 * NULL = plain LayerNorm.  D % 512 == 0, D <= 8192. */
int alg_layernorm_modulate(const void* x, void* y, const void* weight, const void* bias, const void* scale,
                           const void* shift, int64_t mod_bstride, int batch, int rows, int D, int64_t x_bstride,
                           int64_t y_bstride, int seg_split, float eps, void* stream);
/* same with an explicit distance (elements) between the two segments' vectors (seg_stride = D above; 0 = one vector for
 * all rows).  HunyuanVideo token_replace: rows < seg_split (first-frame tokens) take the timestep-0 modulation. */
int alg_layernorm_modulate_seg(const void* x, void* y, const void* weight, const void* bias, const void* scale,
                               const void* shift, int64_t mod_bstride, int64_t seg_stride, int batch, int rows, int D,
                               int64_t x_bstride, int64_t y_bstride, int seg_split, float eps, void* stream);

/* alg_layernorm_modulate in front of an fp8 GEMM: the same arguments and arithmetic, but instead of y it writes
 * q8 [batch * rows][D] OCP e4m3 bytes (contiguous) and q8_scale [batch * rows] float32 -- bit for bit what
 * alg_quantize_fp8_rows makes of the bf16 y (amax / 448 per row), without the bf16 row going through memory.
 * x 16-byte aligned, q8 8-byte aligned.  D % 512 == 0, D <= 8192; anything else is ALG_EINVAL before any launch. */
int alg_layernorm_modulate_fp8(const void* x, void* q8, float* q8_scale, const void* weight, const void* bias,
                               const void* scale, const void* shift, int64_t mod_bstride, int batch, int rows, int D,
                               int64_t x_bstride, int seg_split, float eps, void* stream);
/* alg_layernorm_modulate_seg in front of an fp8 GEMM: the explicit distance between the two segments' vectors (seg_stride,
 * elements, % 8 == 0; 0 = one vector for all rows), otherwise alg_layernorm_modulate_fp8 -- bit for bit alg_layernorm_modulate_seg
 * into bf16 followed by alg_quantize_fp8_rows.  HunyuanVideo's latent / joint rows with token-replace modulation. */
int alg_layernorm_modulate_seg_fp8(const void* x, void* q8, float* q8_scale, const void* weight, const void* bias,
                                   const void* scale, const void* shift, int64_t mod_bstride, int64_t seg_stride, int batch,
                                   int rows, int D, int64_t x_bstride, int seg_split, float eps, void* stream);
/* alg_layernorm_modulate in front of an MXFP4 GEMM: the arguments and arithmetic of alg_layernorm_modulate_fp8, but it writes
 * q4 [batch * rows][D / 2] packed e2m1 bytes and q4_scales [batch * rows][D / 32] E8M0 bytes (both contiguous) -- bit for bit
 * what alg_quantize_mxfp4_rows makes of the bf16 y, without the bf16 row going through memory.  x 16-byte aligned, q4 4-byte
 * aligned.  D % 512 == 0, D <= 8192; anything else is ALG_EINVAL before any launch. */
int alg_layernorm_modulate_mxfp4(const void* x, void* q4, void* q4_scales, const void* weight, const void* bias,
                                 const void* scale, const void* shift, int64_t mod_bstride, int batch, int rows, int D,
                                 int64_t x_bstride, int seg_split, float eps, void* stream);

/* In place on qk: [batch][S][2][heads][64] bf16 (q then k per token):
 * per-head LayerNorm(64) with (wq,bq) / (wk,bk), then RoPE (cos/sin fp32 [S - text_len][64], interleaved-pair
 * convention) on tokens >= text_len. */
int alg_qk_norm_rope(void* qk, const void* wq, const void* bq, const void* wk, const void* bk, const float* cos_tab,
                     const float* sin_tab, int batch, int S, int heads, int text_len, float eps, void* stream);

/* The same with Q multiplied by q_scale inside its last rounding (K untouched): q_scale = softmax_scale * log2(e) lets
 * alg_flash_attn_d64_ex(ALG_ATTN_Q_PRESCALED) form its probabilities as exp2(score) with no per-score multiply. */
int alg_qk_norm_rope_scaled(void* qk, const void* wq, const void* bq, const void* wk, const void* bk, const float* cos_tab,
                            const float* sin_tab, int batch, int S, int heads, int text_len, float eps, float q_scale,
                            void* stream);

/* Patch gather for the patch-embed GEMM (cog:1060-1070 batch assembly folded in, no materialised cat):
 * out[n][(f, gy, gx)][c*p*p + py*p + px]; channels [0, C) come from latents (sample stride lat_bstride, 0 =
 * broadcast), channels [C, 2C) from cond[n] (cond_ptrs: n device pointers to [F][C][H][W] tensors). */
int alg_patchify(const void* latents, int64_t lat_bstride, const void* const* cond_ptrs, void* out, int n_samples,
                 int frames, int C, int H, int W, int p, void* stream);

/* proj_out rows [n][(f,gy,gx)][c*p*p + py*p + px] -> [n][F][C][H][W] bf16. */
int alg_unpatchify(const void* in, void* out, int n_samples, int frames, int C, int H, int W, int p, void* stream);

/* CogVideoX 1.5 (`patch_size_t`; CogVideoXPatchEmbed's Linear over (c, t, py, px) and the matching unpatchify): frames
 * are folded in groups of p_t: out[n][(f / p_t, gy, gx)][((c*p_t + f % p_t)*p + py)*p + px];  p_t = 1 is the above. */
int alg_patchify_t(const void* latents, int64_t lat_bstride, const void* const* cond_ptrs, void* out, int n_samples,
                   int frames, int C, int H, int W, int p, int p_t, void* stream);
int alg_unpatchify_t(const void* in, void* out, int n_samples, int frames, int C, int H, int W, int p, int p_t,
                     void* stream);

/* Timesteps(dim, flip_sin_to_cos, freq_shift=0): out [n][dim] bf16 sinusoid of t[n] (fp32 timesteps). */
int alg_timestep_embedding(const float* t, void* out, int n, int dim, int flip_sin_to_cos, void* stream);

/* ---- Wan 2.1 VAE (diffusers AutoencoderKLWan; reference pipeline_wan_image2video_lowpass.py:426-430 encode, :959 decode) ----
 * Its convolutions are alg_conv_cl_bf16 / alg_gemm_bf16 launches; these two are the kernels specific to it. */

/* WanRMS_norm (+ the SiLU that follows it in every residual block): y[r][c] = act(x[r][c] * sqrt(C) / max(||x[r][:C]||_2,
 * 1e-12) * gamma[c]) for c < C and 0 for the padding channels C <= c < Cp.  x, y: [rows][Cp] bf16, gamma: [Cp] bf16. */
int alg_rms_norm_rows(const void* x, const void* gamma, void* y, int64_t rows, int C, int Cp, int silu, void* stream);

/* Row softmax of the VAE mid-block attention over scores split in two bf16 matrices (hi = -neg_hi, lo): p[r][j] =
 * softmax_j((lo - neg_hi) * scale), zero in the padding columns cols <= j < ld.  All three [rows][ld] bf16. */
int alg_softmax_hilo(const void* neg_hi, const void* lo, void* p, int64_t rows, int cols, int64_t ld, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Box calibration for the benchmark line (no reference call site: the reference times nothing, readme.md:1-170; SURVEY 8d asks
 * for rooflines measured on the box).  csrc/calibrate.hip.
 * ---------------------------------------------------------------------------------------------- */

/* One launch of a register-only v_mfma_f32_32x32x16_bf16 loop on pseudo-random bf16 operands: `blocks` workgroups of 256
 * threads (0 = two per CU, i.e. two waves per SIMD); every wave issues 32 * iters MFMAs = 32 * iters * 32768 FLOP.  The caller
 * brackets the launch with events.  clocks (optional): uint64 [blocks][4] = {shader cycles, constant-rate ticks} at the start and
 * at the end of each workgroup.  Returns the number of workgroups launched (> 0) or a negative ALG_E* code. */
int alg_calib_mfma_bf16(float* sink, int iters, unsigned seed, int blocks, uint64_t* clocks, void* stream);

/* Rate of the constant counter of the clock taps in kHz (100,000 on MI355X); 0 when unknown. */
int alg_wall_clock_khz(void);

/* While `buffer` is non-NULL, every launch of the pipelined d = 64 attention and of the 64-query d = 128 attention has one lane
 * of each workgroup whose index is a multiple of 64 -- the first `slots` of them: one workgroup owns a slot -- store {shader
 * cycles, constant-rate ticks} at its start and end into buffer[block / 64][4] (uint64): d cycles / d ticks = the shader clock
 * that kernel ran at.  Results are unaffected.  A launch on a CAPTURING stream never takes the tap (the pointer would be baked
 * into the graph and outlive the buffer).  Host-only call; NULL (the default) switches the taps off; the caller keeps the
 * buffer alive until it has done so. */
void alg_attn_clock_tap(uint64_t* buffer, int slots);

/* Path counters of the pipelined d = 64 attention (ALG_ATTN_PP 4 and 8).  While `buffer` (device memory, three uint64, zeroed by
 * the caller) is non-NULL, every wave of every launch adds at its end, with atomicAdd from one lane: buffer[0] += entries into the
 * asm statement, buffer[1] += KV tiles run inside the statement, buffer[2] += KV tiles run in the C++ straight loop (tile 0, the
 * tail, refused tiles and the tiles up to the next entry point).  Per wave [1] + [2] = the number of KV tiles.  Results are
 * unaffected; with no buffer the cost is one uniform branch per wave.  Capture rule, lifetime and threading as
 * alg_attn_clock_tap.  Host-only call; NULL (the default) switches the counters off. */
void alg_attn_path_tap(uint64_t* buffer);

#ifdef __cplusplus
}
#endif
#endif /* ALG_HIP_H */
