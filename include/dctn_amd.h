/*
 * dctn_amd — C-ABI of the MI355X (gfx950) kernel library for dctn's hot path.
 *
 * Drop-in boundary.  The reference (philip-bl/dctn) is pure Python: it has no FFI for this path;
 * its arithmetic is delegated to opt_einsum -> torch.einsum.  The entry points below are what a
 * binding for this path binds (ctypes stub: INTEGRATION.md); each one names the reference
 * function whose arithmetic it replaces (file:line relative to the reference repository).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes and element strides; no torch / C++ types.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream).  No allocation, no synchronisation, no host<->device copies inside: calls can be
 *     captured into a hipGraph.  Scratch memory is supplied by the caller (`*_workspace_bytes`).
 *   - return value: 0 on success, negative DCTN_ERR_* otherwise (dctn_strerror()).  The Python
 *     host layer turns shape errors into AssertionError like the reference's `assert`s.
 *   - dtype codes: DCTN_F32 / DCTN_F64 / DCTN_BF16 (bf16 storage, fp32 accumulation).
 *   - re-entrant.  Nothing a call computes depends on process state beyond the device's geometry (CU count, LDS per
 *     CU: asked once, dctn_device_limits()); there are no setters; the one mutable global is the diagnostic name
 *     returned by dctn_last_kernel().
 */
#ifndef DCTN_AMD_H
#define DCTN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { DCTN_F32 = 0, DCTN_F64 = 1, DCTN_BF16 = 2, DCTN_DTYPE_MASK = 0xFF };
/* OR-ed into the `dtype` argument of the dctn_convsbs_* entry points (any other bit above DCTN_DTYPE_MASK:
 * DCTN_ERR_UNSUPPORTED): strings with every bond <= 4 run on the matrix-core sweep instead of the register-resident
 * sweep that is their default (cross-check of the two kernel families; same results to f32 rounding) */
enum { DCTN_SBS_MATRIX_CORE_SWEEP = 1 << 8 };
/* OR-ed in the same way: the backward runs on the wide family (convsbs_wide.hip: dCore GEMMs over HBM partial records,
 * the family every string whose core gradients do not fit one workgroup's LDS falls to) for any string it covers; the
 * forward ignores the bit (cross-check of the wide family against the generic sweep on strings both take) */
enum { DCTN_SBS_WIDE_SWEEP = 1 << 9 };

enum {
  DCTN_OK = 0,
  DCTN_ERR_BAD_SHAPE = -1,    /* sizes inconsistent (reference: AssertionError) */
  DCTN_ERR_BAD_DTYPE = -2,    /* unknown dtype code */
  DCTN_ERR_UNSUPPORTED = -3,  /* valid request no kernel of this build covers */
  DCTN_ERR_WORKSPACE = -4,    /* workspace missing or too small */
  DCTN_ERR_LAUNCH = -5,       /* HIP reported a launch error */
  DCTN_ERR_NULL = -6          /* required pointer is NULL */
};
/* positive success codes of the entry points that document them */
enum {
  DCTN_SAVED = 1,             /* dctn_eps_fwd_save / dctn_convsbs_fwd: the forward also WROTE the buffer a following
                                 *_bwd_saved call reads; DCTN_OK (0) = forward done, buffer untouched */
  DCTN_PARTIAL = 2            /* DCTN_OPT_MAIN_KERNEL_ONLY was honoured: only the dominant kernel ran, the
                                 gradients are NOT complete */
};

/* `policy` argument of the EPS entry points: one DCTN_PREC_* value (precision policy for float32 tensors on the
 * MFMA paths), optionally OR-ed with DCTN_OPT_* flags.  A workspace query and the call it sizes take the same policy. */
enum {
  DCTN_PREC_EXACT = 0, /* f32 in / f32 accumulate (v_mfma_f32_32x32x2_f32 or VALU fma) */
  DCTN_PREC_BF16 = 1,  /* operands rounded to bf16, f32 accumulate (v_mfma_f32_32x32x16_bf16) */
  /* bf16x3 ("high"): each f32 operand value is hi + lo, two bf16 values (hi = bf16_rn(v), lo = bf16_rn(v - hi)), each
   * product hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, f32 accumulate (relative error ~3 * 2^-18 per product).
   * It PERMITS the faster arithmetic and does not force it: float32 calls whose shape the bf16x3 large-core family
   * (DCTN_EPS_FAMILY_BIGCORE_BF16X3) plans run bf16x3, forward and backward; every other shape, dtype and entry point
   * runs exactly as under DCTN_PREC_EXACT - the same kernels and the same bits (the register-resident exact-f32 family
   * and its fused head, the two-halves path, float64, the generic kernels). */
  DCTN_PREC_SPLIT = 2,
  DCTN_PREC_MASK = 0xFF
};
enum {
  /* float32 shapes that both exact-f32 families cover run on the two-halves GEMM path instead of the LDS-streamed
   * large-core kernels (cross-check of the two designs; same results to f32 rounding) */
  DCTN_OPT_F32_PREFER_HALVES = 1 << 8,
  /* two-halves path: bound its per-chunk buffers to 256 KiB instead of 1 GiB, so that small inputs take many
   * chunks (tests of the chunk loop; results identical) */
  DCTN_OPT_SMALL_CHUNKS = 1 << 9,
  /* measurement only: dctn_eps_bwd / dctn_eps_head_bwd on the register-resident family launch their dominant
   * kernel (per-workgroup partial sums) and skip the small reduction kernel, so that the kernel can be timed
   * alone; the gradients are NOT written and the call returns DCTN_PARTIAL (2), not DCTN_OK.  One exception:
   * dctn_eps_head_bwd with DCTN_OPT_HEAD_FEATURES_BLOCKED4 forms the head weight gradient on spare waves of that
   * dominant kernel, so there the kernel also writes d_weight (and its time includes that product) */
  DCTN_OPT_MAIN_KERNEL_ONLY = 1 << 10,
  /* dctn_eps_fwd / dctn_eps_bwd on the generic kernels whatever the shape: one lane per window walks the core rows
   * one factor digit after the other, no matrix cores, no Khatri-Rao halves - the independent evaluation order
   * behind `eps_one_by_one` (dctn/eps.py:43-63), which the reference's tests use to cross-check `eps` */
  DCTN_OPT_GENERIC_KERNELS = 1 << 11,
  /* dctn_eps_head_fwd / dctn_eps_head_bwd only: `features` in the sample-blocked layout "blocked4" instead of
   * row-major (see dctn_eps_head_fwd); every other entry point returns DCTN_ERR_UNSUPPORTED for it */
  DCTN_OPT_HEAD_FEATURES_BLOCKED4 = 1 << 12,
  DCTN_OPT_ALL = (1 << 8) | (1 << 9) | (1 << 10) | (1 << 11) | (1 << 12)   /* any other bit above DCTN_PREC_MASK: DCTN_ERR_UNSUPPORTED */
};

int dctn_version(void);
const char* dctn_strerror(int code);
/* name of the kernel family the last successful call dispatched to
 * (diagnostics / tests: proves which HIP path ran; process-wide, last writer wins) */
const char* dctn_last_kernel(void);

/* the device geometry every plan of the library assumes: CUs and LDS bytes per CU of the current device, asked once
 * per process (gfx950 values where the runtime cannot say).  The environment variable DCTN_DEVICE_LIMITS="cus,lds"
 * can only lower them: tests run the plans of a smaller device (a partitioned card) with it. */
int dctn_device_limits(int* cus, int* lds_bytes);

/* ------------------------------------------------------------------------------------------
 * EPS — replaces dctn/eps.py:19-40 `eps(core, input)` (and :43-63 `eps_one_by_one`, same result)
 *   x    : (C, B, H, W, Q) with element strides x_strides[5]
 *   core : (Q,)*(K*K*C) + (O,) contiguous == row-major matrix (Q^(K*K*C), O); factor index
 *          n = pos*C + ch, pos row-major over (dh, dw)  (dctn/align.py:31-32,41-45)
 *   out  : (B, H-K+1, W-K+1, O) contiguous
 *   workspace : scratch of dctn_eps_fwd_workspace_bytes() bytes (0 for most shapes; the large-core
 *          family splits its row tiles over the grid and sums the slices in a fixed order)
 * ------------------------------------------------------------------------------------------ */
/* Which kernel family the forward (and backward) of a shape runs on, for a contiguous input: callers use
 * it to route bf16 tensors with large cores through float32 (the exact-f32 matrix-core family; bf16
 * storage, f32 arithmetic) instead of the generic kernels — see dctn_amd/eps.py.  -1 = invalid shape. */
#define DCTN_EPS_FAMILY_GENERIC 0
#define DCTN_EPS_FAMILY_Q2REG 1        /* bf16 MFMA, Q = 2, N in {8, 9} */
#define DCTN_EPS_FAMILY_BIGCORE_F32 2  /* exact f32 MFMA, LDS-streamed core */
#define DCTN_EPS_FAMILY_HALVES 3       /* two-halves GEMM path: f64 MFMA, and f32 MFMA for shapes 1 and 2 leave */
#define DCTN_EPS_FAMILY_Q2REG_F32 4    /* exact f32 MFMA, register-resident core: Q = 2, N in {8, 9}, O <= 4 */
#define DCTN_EPS_FAMILY_BIGCORE_BF16X3 5  /* DCTN_PREC_SPLIT float32 only: bf16x3 MFMA, LDS-streamed core (the shapes of
                                           * family 2 whose every product the bf16x3 plans take); under that policy
                                           * every other shape answers what it answers under DCTN_PREC_EXACT */
int dctn_eps_family(int C, int B, int H, int W, int Q, int K, int O, int dtype, int policy);
size_t dctn_eps_fwd_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O,
                                    int dtype, int policy);
int dctn_eps_fwd(const void* x, const int64_t x_strides[5], const void* core, void* out,
                 void* workspace, size_t workspace_bytes,
                 int C, int B, int H, int W, int Q, int K, int O,
                 int dtype, int policy, void* stream);

/* Forward whose output is only needed for its statistics - replaces the `transform_in_slices(...)` +
 * `output.std(unbiased=False)` of dctn/eps.py:163-181 `make_eps_unit_empirical_output_std` (and the statistics of
 * dctn/eps_plus_linear.py:161-196): stats[0] += sum y, stats[1] += sum y^2 over every value of eps(core, x), in
 * float64, values as the output tensor would hold them (rounded to the storage dtype).  `stats`: two float64 on the
 * device, ACCUMULATED (the caller zeroes them once and feeds slice after slice; count = B*H'*W'*O per call).
 * The register-resident family folds the sums into the forward kernel's epilogue and stores nothing; the other
 * families write the slice into `workspace` (dctn_eps_fwd_stats_workspace_bytes) and reduce it in a second pass -
 * the output of the whole data set is never materialised either way. */
size_t dctn_eps_fwd_stats_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O,
                                          int dtype, int policy);
int dctn_eps_fwd_stats(const void* x, const int64_t x_strides[5], const void* core, void* stats,
                       void* workspace, size_t workspace_bytes,
                       int C, int B, int H, int W, int Q, int K, int O,
                       int dtype, int policy, void* stream);

/* Autograd of the above (reference: torch autograd through the 4 path steps, dctn/training.py:81).
 *   dY    : (B, H', W', O) contiguous
 *   dX    : (C, B, H, W, Q) contiguous, or NULL when the input needs no gradient
 *   dCore : same layout as core, or NULL
 *   Both are OVERWRITTEN (not accumulated).  `workspace` must hold dctn_eps_bwd_workspace_bytes().
 */
size_t dctn_eps_bwd_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O,
                                    int dtype, int policy, int need_dx, int need_dcore);
int dctn_eps_bwd(const void* x, const int64_t x_strides[5], const void* core, const void* dY,
                 void* dX, void* dCore, void* workspace, size_t workspace_bytes,
                 int C, int B, int H, int W, int Q, int K, int O,
                 int dtype, int policy, void* stream);

/* Training forward / backward that keep the forward's GEMM result - what the reference's autograd does: torch saves
 * the result G of path step (0,1) (dctn/eps.py:25-30, `core . K-R_0`) and its backward runs TWO GEMMs of that size
 * (d core, d K-R_0) plus a product of G with dY; without the buffer dctn_eps_bwd has to run the forward GEMM a third
 * time.  Only the input gradient needs it (dCore does not): pass it when dX will be asked for.
 *   dctn_eps_saved_bytes : size of the buffer for this shape, 0 when the shape's kernel family keeps nothing
 *                          (register-resident and generic families: nothing to save; also beyond 16 GiB)
 *   dctn_eps_fwd_save    : dctn_eps_fwd + fills `saved`.  Returns DCTN_SAVED (1) when `saved` was written,
 *                          DCTN_OK (0) when the forward ran but kept nothing (then call dctn_eps_bwd), < 0 on error
 *   dctn_eps_bwd_saved   : dctn_eps_bwd reading `saved` as written by dctn_eps_fwd_save for the SAME x, core, shape,
 *                          dtype and policy.  Same outputs as dctn_eps_bwd to rounding (the sums run in another order).
 * large-core float32 family: Z[(b,o)][w] float32 in row-quad-major order, B*H'*W' * Q^n1 * O * 4 bytes (cfg3a layer 2:
 * 416 MB); two-halves family: both Khatri-Rao halves and Z in the storage dtype. */
size_t dctn_eps_saved_bytes(int C, int B, int H, int W, int Q, int K, int O, int dtype, int policy);
int dctn_eps_fwd_save(const void* x, const int64_t x_strides[5], const void* core, void* out,
                      void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                      int C, int B, int H, int W, int Q, int K, int O,
                      int dtype, int policy, void* stream);
int dctn_eps_bwd_saved(const void* x, const int64_t x_strides[5], const void* core, const void* dY,
                       const void* saved, size_t saved_bytes,
                       void* dX, void* dCore, void* workspace, size_t workspace_bytes,
                       int C, int B, int H, int W, int Q, int K, int O,
                       int dtype, int policy, void* stream);

/* Forward of (EPS layer -> "b h w q -> b (h w q)" -> nn.Linear), the tail of EPSesPlusLinear.forward (reference:
 * dctn/eps_plus_linear.py:144-147), as ONE kernel: a workgroup holds all window positions of a few samples, so the
 * head's sum over (position, output) closes inside the workgroup - no second launch, no re-read of the features.
 *   features : OVERWRITTEN (the layer's output; the backward reads it), F = H'*W'*O features per sample, in one of
 *              two layouts chosen by the policy:
 *              row-major (default): (B, F) contiguous;
 *              "blocked4" (DCTN_OPT_HEAD_FEATURES_BLOCKED4): features[((j * F) + f) * 4 + i] = feature f of sample
 *              4 j + i, ceil(B / 4) * 4 * F values, the samples past B written as zeros.  Only the bf16 register family
 *              takes it, for the shapes whose backward forms dW as one product over the samples (N = 9, O = 4, vector
 *              input layout, ceil(B / 4) * 4 * F * 2 < 2^31 bytes); every other shape, the float32 family and
 *              DCTN_OPT_SMALL_CHUNKS return DCTN_ERR_UNSUPPORTED before any launch
 *   logits   : (B, Cout) contiguous, OVERWRITTEN = features @ head_weight^T + head_bias, products of the stored
 *              (bf16-rounded) features with the bf16 weight, float32 sums (the same bits in both layouts)
 * bfloat16, contiguous x, the register-resident family with O in {2, 4}, Cout <= 16 and at most 768 window positions
 * per sample; DCTN_ERR_UNSUPPORTED otherwise (the caller then runs dctn_eps_fwd + dctn_linear_head_fwd). */
int dctn_eps_head_fwd(const void* x, const int64_t x_strides[5], const void* core, const void* head_weight,
                      const void* head_bias, void* features, void* logits,
                      int C, int B, int H, int W, int Q, int K, int O, int Cout,
                      int dtype, int policy, void* stream);

/* Backward of (EPS layer -> "b h w q -> b (h w q)" -> nn.Linear), the tail of
 * EPSesPlusLinear.forward (reference: dctn/eps_plus_linear.py:144-147), in one pass over x: the
 * kernel forms dY[b,h,w,o] = sum_c dLogits[b,c] * head_weight[c, (h*W'+w)*O + o] on the fly, so the
 * gradient of the features is never written to or read from HBM, and accumulates the head's own
 * gradients beside dCore.
 *   features    : the layer's forward output (input of the linear head), row-major (B, H'*W'*O) contiguous, or
 *                 "blocked4" as dctn_eps_head_fwd wrote it under DCTN_OPT_HEAD_FEATURES_BLOCKED4 (the same bit in
 *                 `policy`; honoured on the same shapes, DCTN_ERR_UNSUPPORTED before any launch elsewhere)
 *   dLogits     : (B, Cout) contiguous;  head_weight : (Cout, H'*W'*O) contiguous
 *   dCore       : same layout as core;  dWeight : like head_weight, or NULL;  dBias : (Cout), or NULL
 *   all three OVERWRITTEN; `workspace` must hold dctn_eps_head_bwd_workspace_bytes().
 * bfloat16 (register-resident bf16 family) and float32 (register-resident exact-f32 family, O in {2, 4}, Cout <= 16);
 * the layer's input gets no gradient.  Returns DCTN_ERR_UNSUPPORTED for shapes outside those two families (the
 * caller then composes dctn_linear_head_bwd or library GEMMs with dctn_eps_bwd; there is no CPU fallback). */
size_t dctn_eps_head_bwd_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O, int Cout,
                                         int dtype, int policy);
int dctn_eps_head_bwd(const void* x, const int64_t x_strides[5], const void* features,
                      const void* dLogits, const void* head_weight, void* dCore, void* dWeight,
                      void* dBias, void* workspace, size_t workspace_bytes,
                      int C, int B, int H, int W, int Q, int K, int O, int Cout,
                      int dtype, int policy, void* stream);

/* ------------------------------------------------------------------------------------------
 * ConvSBS — replaces dctn/conv_sbs.py:258-304 `ConvSBS.forward`
 *   x         : (C, B, H, W, q) with element strides x_strides[5] (channel c = x[c])
 *   n_cores   : number of cores in the string (string order)
 *   cores[c]  : device pointer to core c, shape (out_sizes[c], bond_sizes[c],
 *               bond_sizes[(c+1)%n], q, ..., q [C times]) contiguous (dctn/conv_sbs_spec.py:24-27,65-80)
 *   pos_h/pos_w : position of core c inside the window (min must be 0, dctn/align.py:18-19)
 *   out       : (B, H-max_h, W-max_w, prod(out_sizes)) contiguous, out dims in string order
 * ------------------------------------------------------------------------------------------ */
size_t dctn_convsbs_workspace_bytes(int n_cores, const int* out_sizes, const int* bond_sizes,
                                    int C, int B, int H, int W, int q,
                                    const int* pos_h, const int* pos_w, int dtype, int backward);
int dctn_convsbs_fwd(const void* x, const int64_t x_strides[5], const void* const* cores,
                     void* out, int n_cores, const int* out_sizes, const int* bond_sizes,
                     const int* pos_h, const int* pos_w,
                     int C, int B, int H, int W, int q,
                     void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* dX (C,B,H,W,q contiguous) and dCores[c] (same layout as cores[c]) are OVERWRITTEN; either
 * dX or the whole dCores array may be NULL. */
int dctn_convsbs_bwd(const void* x, const int64_t x_strides[5], const void* const* cores,
                     const void* dY, void* dX, void* const* dCores,
                     int n_cores, const int* out_sizes, const int* bond_sizes,
                     const int* pos_h, const int* pos_w,
                     int C, int B, int H, int W, int q,
                     void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* A training forward can leave its forward states for the backward instead of having the backward recompute them
 * (the backward's own forward sweep is a quarter of its time): pass dctn_convsbs_fwd a workspace of at least
 * dctn_convsbs_saved_states_bytes(...) bytes (0: this string always recomputes - rings, many-valued cores, bonds above
 * 16, float64 / bf16).  dctn_convsbs_fwd then returns DCTN_SAVED (1) when it WROTE the states - hand that buffer,
 * untouched, to dctn_convsbs_bwd_saved - and DCTN_OK (0) when the forward ran on a kernel that keeps nothing (the
 * buffer is then uninitialised: call dctn_convsbs_bwd).  NULL / too small saved_states: exactly dctn_convsbs_bwd.  Replaces nothing in the reference (autograd keeps every intermediate there, dctn/conv_sbs.py:268-303). */
size_t dctn_convsbs_saved_states_bytes(int n_cores, const int* out_sizes, const int* bond_sizes, int C, int B, int H,
                                       int W, int q, const int* pos_h, const int* pos_w, int dtype);
int dctn_convsbs_bwd_saved(const void* x, const int64_t x_strides[5], const void* const* cores,
                           const void* dY, void* dX, void* const* dCores, int n_cores,
                           const int* out_sizes, const int* bond_sizes, const int* pos_h,
                           const int* pos_w, int C, int B, int H, int W, int q, void* workspace,
                           size_t workspace_bytes, const void* saved_states, size_t saved_states_bytes, int dtype,
                           void* stream);

/* Several strings of one layer at once - replaces the loop of `ManyConvSBS.forward` (dctn/conv_sbs.py:367-370: every
 * string contracts the same input) for layers whose strings are all nine-core strings of one bond <= 4 over the same
 * window positions (the reference's layers: two snakes through one 3 x 3 window, mnist.py:189-252): ONE forward launch,
 * ONE backward launch (+ the small reduction), dX written once, already summed over the strings.  Since version 401
 * also layers of TWO strings of the band family (largest bond 5..16, same band geometry: the bond-16 layer of
 * mnist.py:224-242): one forward launch, one backward launch + one tail kernel that sums the strings' shares of dX.
 *   cores / dCores : n_strings * n_cores pointers, string-major;  out_sizes, bond_sizes, pos_h, pos_w likewise
 *   outs / dYs     : one (B, H', W', prod(out_sizes of the string)) tensor per string
 * DCTN_ERR_UNSUPPORTED for any other layer: call dctn_convsbs_fwd / _bwd per string (and add the dX). */
size_t dctn_convsbs_many_workspace_bytes(int n_strings, int n_cores, const int* out_sizes, const int* bond_sizes,
                                         int C, int B, int H, int W, int q, const int* pos_h, const int* pos_w, int dtype);
int dctn_convsbs_many_fwd(const void* x, const int64_t x_strides[5], const void* const* cores, void* const* outs,
                          int n_strings, int n_cores, const int* out_sizes, const int* bond_sizes,
                          const int* pos_h, const int* pos_w, int C, int B, int H, int W, int q, int dtype, void* stream);
int dctn_convsbs_many_bwd(const void* x, const int64_t x_strides[5], const void* const* cores, const void* const* dYs,
                          void* dX, void* const* dCores, int n_strings, int n_cores,
                          const int* out_sizes, const int* bond_sizes, const int* pos_h, const int* pos_w,
                          int C, int B, int H, int W, int q, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * logmatmulexp — replaces dctn/logmatmulexp.py:5-14 (and the checkpointed :17-22; nothing of
 * size Theta*R*I is ever materialised here, forward or backward).
 *   batched: logA (batch, Theta, R), logB (batch, R, I), out (batch, Theta, I), all contiguous;
 *   the reference's strictly 2-D call is batch == 1.  stride_*_batch in elements (0 = broadcast).
 * ------------------------------------------------------------------------------------------ */
/* Products that are not tiny run as "exp -> GEMM on the matrix cores -> log" (one exp per input
 * element, float32 MFMA) and need scratch: `workspace` of dctn_logmatmulexp_workspace_bytes() bytes
 * (0 = this shape uses the direct kernels; workspace may then be NULL).  With workspace == NULL the
 * direct kernels are always used.  Results keep torch.logsumexp semantics either way: output tiles
 * / batch elements where the factored form is not safe are recomputed by the direct kernels. */
size_t dctn_logmatmulexp_workspace_bytes(int64_t batch, int Theta, int R, int I,
                                         int64_t strideA_batch, int64_t strideB_batch, int dtype);
int dctn_logmatmulexp_fwd(const void* logA, const void* logB, void* out,
                          void* workspace, size_t workspace_bytes,
                          int64_t batch, int Theta, int R, int I,
                          int64_t strideA_batch, int64_t strideB_batch,
                          int dtype, void* stream);
/* dA / dB are OVERWRITTEN; either may be NULL.  With a broadcast operand (stride 0) its
 * gradient is summed over the batch. */
int dctn_logmatmulexp_bwd(const void* logA, const void* logB, const void* out, const void* dOut,
                          void* dA, void* dB,
                          void* workspace, size_t workspace_bytes,
                          int64_t batch, int Theta, int R, int I,
                          int64_t strideA_batch, int64_t strideB_batch,
                          int dtype, void* stream);

/* Left fold over L square log-matrices per window — the loop
 * `reduce(logmatmulexp, matrices)` of small_experiments/logmatmulexp_benchmark/benchmark.py:30,
 * batched over windows (BASELINE config 5).
 *   mats : (Wn, L, D, D) contiguous;  out : (Wn, D, D)
 * Backward recomputes the prefix folds; `workspace` holds dctn_logmatmulexp_fold_workspace_bytes(). */
size_t dctn_logmatmulexp_fold_workspace_bytes(int64_t Wn, int L, int D, int dtype, int backward);
int dctn_logmatmulexp_fold_fwd(const void* mats, void* out, int64_t Wn, int L, int D,
                               int dtype, void* stream);
int dctn_logmatmulexp_fold_bwd(const void* mats, const void* dOut, void* dMats,
                               void* workspace, size_t workspace_bytes,
                               int64_t Wn, int L, int D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Linear classifier head — replaces `self.linear(features)` of dctn/eps_plus_linear.py:147
 * (nn.Linear(H'*W'*Q, 10)) for skinny outputs.
 *   feat (B, F), weight (Cout, F), bias (Cout), out (B, Cout), all contiguous;
 *   float32, float64 and bf16 (float32 accumulation; float64 for float64), Cout <= 16, any F.  bf16 with F % 8 == 0 and
 *   16-byte aligned pointers runs the vectorised matrix-core kernels, everything else the scalar streaming kernels
 *   (DCTN_ERR_UNSUPPORTED only for Cout > 16: the host layer then uses the framework's library GEMM).
 *   Backward: dFeat (B, F), dWeight (Cout, F), dBias (Cout) are OVERWRITTEN; dFeat may be NULL;
 *   dWeight and dBias are produced together (dBias may be NULL).
 * ------------------------------------------------------------------------------------------ */
int dctn_linear_head_fwd(const void* feat, const void* weight, const void* bias, void* out,
                         int64_t B, int F, int Cout, int dtype, void* stream);
size_t dctn_linear_head_bwd_workspace_bytes(int64_t B, int F, int Cout, int dtype);
int dctn_linear_head_bwd(const void* feat, const void* weight, const void* dOut, void* dFeat,
                         void* dWeight, void* dBias, void* workspace, size_t workspace_bytes,
                         int64_t B, int F, int Cout, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Window statistics of the input feature map (reference: calc_scaling_factor,
 * dctn/dataset_loading.py:79-94 = make_windows (dctn/align.py:49-61) + RankOneTensorsBatch
 * .mean_over_batch / .var_over_batch (dctn/rank_one_tensor.py:53-100)).  For the rank-one tensor
 * T_w = (x)_n x_n[w,:] of every K x K window w of x (C,B,H,W,Q):
 *   sums[0] = sum_w sum(T_w)   = sum_w prod_n sum_q x_n[w,q]
 *   sums[1] = sum_w ||T_w||^2  = sum_w prod_n sum_q x_n[w,q]^2
 * `sums`: two float64 values on the device, OVERWRITTEN.  The K*K-fold window tensor of the
 * reference is never materialised.
 * ------------------------------------------------------------------------------------------ */
int dctn_window_stats(const void* x, const int64_t x_strides[5], void* sums,
                      int C, int B, int H, int W, int Q, int K, int dtype, void* stream);

/* The feature map itself on the device - replaces `phi_cos_sin_squared_1` as applied to the whole data set in
 * dctn/dataset_loading.py:33-36,63 (u -> (2 sin^2(pi u / 2), 2 cos^2(pi u / 2)), float32 arithmetic like the reference's):
 *   dctn_phi_window_stats : the two sums of dctn_window_stats straight from the RAW images (B, H, W) float32 contiguous,
 *       phi applied once per pixel inside the kernel: neither the expanded (1, B, H, W, 2) tensor nor the K*K stacked
 *       window copies of calc_scaling_factor (dataset_loading.py:79-94) exist.  sums: two float64, OVERWRITTEN.
 *       DCTN_ERR_UNSUPPORTED for images whose per-pixel table does not fit LDS (beyond ~97 x 97).
 *   dctn_phi_expand       : x[0, b, h, w, :] = scale * phi(images[b, h, w]) written once in the model's dtype
 *       (`dtype` of x: f32 / f64 / bf16), the scaling factor folded in; n_pixels = B * H * W. */
int dctn_phi_window_stats(const void* images, void* sums, int B, int H, int W, int K, void* stream);
int dctn_phi_expand(const void* images, void* x, int64_t n_pixels, float scale, int dtype, void* stream);

/* Statistics of a byte-resident data set, from the bytes (version 517; dctn_amd/csrc/byte_stats.hip): what the reference's
 * colour loader computes from the EXPANDED training tensor (dctn/dataset_loading.py:351-352 and calc_scaling_factor, :79-94)
 * for the sources that keep the data set on the device as uint8.  Nothing of the data set's size is expanded.
 *   dctn_byte_histogram : src (n_pixels, channels) interleaved uint8, channels 1 .. 4, ANY byte alignment;
 *       counts int64 [channels][256] (8-byte aligned), OVERWRITTEN: counts[c][v] = the pixels whose channel c holds v.
 *       Workgroups count in 32-bit LDS counters - the plan bounds a workgroup's share to 2^31 + 6 pixels, so none wraps -
 *       and add them with 64-bit integer atomics: the result is exact and the same in any order.
 *   dctn_byte_window_stats : the two sums of dctn_window_stats (C = 1) for the tensor that a 256-row table per channel
 *       expands the bytes to, without it.  src (n, H, W, channels) interleaved uint8, any alignment; tu double
 *       [channels][256][2]: for byte value v in channel c the sum t and the sum of squares u of the features that byte
 *       produces; t0, u0: the same of the columns no byte feeds (a constant channel).  A pixel's pair is
 *       t = t0 + sum_c tu[c][byte_c].t (channels ascending), u likewise; a window's two terms are the products of t and of
 *       u over its K x K pixels; sums (two float64, OVERWRITTEN) = {sum_w prod t, sum_w prod u}.
 *       One workgroup per image; each STORES its pair of partial sums into workspace[image], and the workgroup that draws
 *       the last ticket adds the n pairs in one fixed order (no workgroup waits, no float atomic): two launches on the same
 *       input leave the SAME BITS, whatever the number of CUs.
 *       workspace: dctn_byte_window_stats_workspace_bytes of n bytes exactly, 8-byte aligned, any previous content.
 *       DCTN_ERR_UNSUPPORTED, before any launch, when the table plus the image's pairs (16 (256 channels + H W) bytes and
 *       80 more) exceed what a workgroup of this device may claim (15/16 of dctn_device_limits' LDS), or a float64 or
 *       int64 buffer is off its 8-byte alignment.  Checks in the library's order: NULL, shape (n_pixels, n < 1, channels
 *       outside 1 .. 4, K < 1, H or W < K), unsupported; no argument carries a dtype. */
int dctn_byte_histogram(const void* src, int64_t n_pixels, int channels, void* counts, void* stream);
size_t dctn_byte_window_stats_workspace_bytes(int64_t n);
int dctn_byte_window_stats(const void* src, int64_t n, int H, int W, int channels, const void* tu, double t0, double u0,
                           int K, void* workspace, void* sums, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tail of a training iteration (reference: dctn/training.py:77-84 with
 * F.cross_entropy, the L2 regularisers of dctn/eps_plus_linear.py:149-159 and torch.optim.SGD).
 *   dctn_ce_loss_fwd : loss[0] (float32, OVERWRITTEN) = mean_b ( logsumexp(logits[b,:]) - logits[b, labels[b]] )
 *   dctn_ce_loss_bwd : dlogits = (softmax(logits) - onehot(labels)) * dloss[0] / B, dtype of logits
 *   dctn_sgd_l2_step : over one flat parameter buffer (n values; the first n_reg are regularised):
 *                      g = grads + 2*l2*w (regularised prefix), buf = first_step ? g : momentum*buf + g,
 *                      w -= lr*buf; sq_sum (optional, float32 array of dctn_sgd_l2_num_partials(n) slots,
 *                      OVERWRITTEN): slot b = workgroup b's part of the sum of w^2 over the prefix BEFORE the
 *                      update; their sum is the regulariser's value / its coefficient (stored, not
 *                      accumulated: no fill launch and no atomics in the iteration).
 *                      momentum_buf is float32 whatever the parameter dtype.  The arithmetic is float32 and
 *                      the result is rounded back into the parameter's own cell: NO float32 copy of a bf16
 *                      parameter is kept (dctn_sgd_l2_step_master below keeps one).
 *   dctn_sgd_l2_step_master (version 501) : the same step for bf16 parameters with a float32 master copy.
 *                      master (float32, n values) is READ and OVERWRITTEN: the update above runs on it, and
 *                      sq_sum is the MASTER's sum of w^2 before the update.  params (bf16, n values) is
 *                      OVERWRITTEN with the new master value rounded to nearest even and is NEVER READ.
 *                      grads are bf16.  The master values are, bit for bit, what dctn_sgd_l2_step leaves in
 *                      float32 parameters given the same gradients.  Same validation and return codes.
 * logits (B, C) contiguous, labels int64; dtypes DCTN_F32 / DCTN_BF16.  Rows labelled -100 (F.cross_entropy's default
 * ignore_index) add nothing to the loss, get a zero gradient row and do not count in the mean (n = the other rows; n = 0:
 * NaN, as torch).  Any other label outside [0, C) makes the loss and that sample's gradient row NaN (F.cross_entropy
 * raises on it).
 * ------------------------------------------------------------------------------------------ */
int dctn_ce_loss_fwd(const void* logits, const void* labels, void* loss, int64_t B, int C, int dtype, void* stream);
/* forward that also leaves dlogits_unit = (softmax - onehot) / n (logits' dtype): the backward for an incoming gradient of 1,
 * so that a caller who knows its gradient seed is 1 needs no second kernel */
int dctn_ce_loss_fwd_grad(const void* logits, const void* labels, void* loss, void* dlogits_unit,
                          int64_t B, int C, int dtype, void* stream);
int dctn_ce_loss_bwd(const void* logits, const void* labels, const void* dloss, void* dlogits,
                     int64_t B, int C, int dtype, void* stream);
int dctn_sgd_l2_num_partials(int64_t n);
int dctn_sgd_l2_step(void* params, const void* grads, void* momentum_buf, void* sq_sum, int64_t n, int64_t n_reg,
                     float lr, float momentum, float l2, int first_step, int dtype, void* stream);
int dctn_sgd_l2_step_master(void* master, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                            int64_t n, int64_t n_reg, float lr, float momentum, float l2, int first_step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Adam (torch.optim.Adam: coupled weight decay, amsgrad = False, maximize = False) plus the same L2 regulariser, as
 * ONE launch per step over the flat parameter buffer.  Per element, in float32 arithmetic (the parameter is widened,
 * updated and rounded back into its own cell; dctn_adam_l2_step STORES no float32 copy of a bf16 parameter, so an
 * update below half an ulp of the bf16 value is lost - dctn_adam_l2_step_master keeps that copy):
 *   g = grads + weight_decay*w (+ 2*l2*w on the regularised prefix),
 *   m = beta1*m + (1-beta1)*g,  v = beta2*v + (1-beta2)*g*g,
 *   w -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)         t = number of this step, from 1.
 * exp_avg / exp_avg_sq are float32 whatever the parameter dtype (DCTN_F32 / DCTN_BF16).  sq_sum: as dctn_sgd_l2_step
 * (optional, dctn_adam_l2_num_partials(n) float32 slots, OVERWRITTEN, sum of w^2 over the prefix BEFORE the update).
 * The step count and the learning rate live on the DEVICE, so that a captured graph that holds this launch advances
 * t on every replay and follows a learning rate changed between replays.  `state`: dctn_adam_state_bytes() = 16
 * bytes, 16-byte aligned, laid out as
 *   int32  steps_done   number of steps taken so far (0 before the first); the launch computes with t = steps_done + 1
 *                       and leaves steps_done + 1 here
 *   float  lr           read by every launch; the caller may overwrite it in stream order between launches
 *   uint32 ticket       0 between launches (workgroups count themselves out on it; the last one resets it)
 *   uint32 reserved     0
 * The caller creates the block once (zeroes + lr) and may read or write it in stream order between launches.
 * beta1^t and beta2^t are formed from t in the kernel (no running products).
 *
 * dctn_adam_l2_step_master (version 501): the same launch for bf16 parameters with a float32 master copy.
 *   master : float32, n values, READ and OVERWRITTEN - the step above runs on it (weight decay, the 2*l2*w term and
 *            sq_sum all see the master value; sq_sum is the MASTER's sum of w^2 before the update)
 *   params : bf16, n values, OVERWRITTEN with the new master value rounded to nearest even; NEVER READ
 *   grads  : bf16;  exp_avg / exp_avg_sq / sq_sum / state and the partial and state sizes: as above
 * The master values, the moments and t are, bit for bit, what dctn_adam_l2_step leaves in float32 parameters given
 * the same gradients.  Same validation and return codes (no dtype argument: the dtypes are fixed).
 * ------------------------------------------------------------------------------------------ */
size_t dctn_adam_state_bytes(void);
int dctn_adam_l2_num_partials(int64_t n);
int dctn_adam_l2_step(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, void* sq_sum, void* state,
                      int64_t n, int64_t n_reg, double beta1, double beta2, float eps, float weight_decay, float l2,
                      int dtype, void* stream);
int dctn_adam_l2_step_master(void* master, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                             void* sq_sum, void* state, int64_t n, int64_t n_reg, double beta1, double beta2, float eps,
                             float weight_decay, float l2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient guard (version 505; reference: the stop-on-NaN-loss hook every run installs, new_runner.py:544, and
 * torch.nn.utils.clip_grad_norm_): ONE launch in front of the optimizer step forms the squared norm of the flat gradient
 * buffer and leaves a decision on the DEVICE that the guarded step kernels obey - the host reads nothing per iteration,
 * and a captured graph that holds the two launches halts and clips on its own.
 *
 * dctn_grad_guard_check : grads (n values, DCTN_F32 / DCTN_BF16) are summed as g*g in FLOAT64 (the square of a float32
 *   value cannot overflow a double, so the sum is non-finite exactly when some element is); one partial sum per workgroup
 *   is STORED into `partials` (dctn_grad_guard_num_partials of n float64 slots, OVERWRITTEN, nothing of their previous
 *   content is used), and the workgroup that finishes last adds them in one fixed order: the same bits from run to run.
 *   No workgroup waits for another.  loss_or_null: optional float32 device scalar; a non-finite loss counts like a
 *   non-finite gradient.  `guard`: dctn_grad_guard_state_bytes = 32 bytes, 16-byte aligned, laid out as
 *     float  max_norm    clip threshold; +inf = never clip.  The caller writes it, in stream order between launches
 *     float  last_norm   (float)sqrt(sum) of the last launch (may be inf / NaN)
 *     uint32 halted      latch: 1 once a launch saw a non-finite sum or loss; ONLY the caller clears it
 *     int32  bad_step    value of `seen` at the launch that set the latch; -1 before
 *     uint32 seen        launches so far (this launch adds 1)
 *     uint32 clipped     launches whose coefficient was below 1
 *     uint32 ticket      0 between launches (workgroups count themselves out on it; the last one resets it)
 *     float  coef        the decision for the step that follows: its gradient multiplier
 *   The caller creates the block once: {max_norm, 0, 0, -1, 0, 0, 0, 0}.  With apply = the latch was clear before this
 *   launch, and sum and loss are finite:
 *     apply     : coef = min(1, (float)((double)max_norm / ((double)last_norm + 1e-6)))   (clip_grad_norm_'s coefficient)
 *     otherwise : coef = 0, the latch is set, and bad_step is written if the latch was clear
 *
 * The guarded steps (the `guard` argument follows `state` / `sq_sum`; everything else as the unguarded entry points,
 * which are unchanged): every workgroup reads `halted` and `coef` first.  Halted: the launch writes NOTHING - no
 * parameter, master value, moment, momentum or sq_sum slot, and the Adam step count does not advance.  Otherwise each
 * gradient is replaced by one rounded float32 product g * coef (a bf16 gradient is widened first and not rounded back)
 * in front of the step's arithmetic: the clip applies to the gradient as it stands in the buffer; weight_decay * w and
 * 2 * l2 * w are added after it - clip_grad_norm_ followed by Adam(weight_decay) / SGD.  With coef = 1 the results are,
 * bit for bit, the unguarded step's.  dctn_grad_guard_check must run before every guarded step, on the same stream.
 * Return codes: DCTN_ERR_NULL, DCTN_ERR_BAD_SHAPE (n < 1, ...), DCTN_ERR_BAD_DTYPE as the unguarded steps.
 * ------------------------------------------------------------------------------------------ */
size_t dctn_grad_guard_state_bytes(void);
int dctn_grad_guard_num_partials(int64_t n);
int dctn_grad_guard_check(const void* grads, int64_t n, int dtype, const void* loss_or_null, void* partials, void* guard,
                          void* stream);
int dctn_adam_l2_step_guarded(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, void* sq_sum, void* state,
                              const void* guard, int64_t n, int64_t n_reg, double beta1, double beta2, float eps,
                              float weight_decay, float l2, int dtype, void* stream);
int dctn_adam_l2_step_master_guarded(void* master, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                                     void* sq_sum, void* state, const void* guard, int64_t n, int64_t n_reg,
                                     double beta1, double beta2, float eps, float weight_decay, float l2, void* stream);
int dctn_sgd_l2_step_guarded(void* params, const void* grads, void* momentum_buf, void* sq_sum, const void* guard,
                             int64_t n, int64_t n_reg, float lr, float momentum, float l2, int first_step, int dtype,
                             void* stream);
int dctn_sgd_l2_step_master_guarded(void* master, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                                    const void* guard, int64_t n, int64_t n_reg, float lr, float momentum, float l2,
                                    int first_step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Learning-rate schedule (version 510): the optimizer launch itself evaluates a table of knots at the device step
 * count, so that a replayed graph - and each of the K iterations inside one launch - steps with its own rate, with no
 * host write and no further graph node.
 *
 * `schedule`: dctn_lr_schedule_bytes = 784 bytes, 16-byte aligned, laid out as
 *   int32  n_knots        1..64
 *   float  scale          multiplies every value; 1.0f leaves the bits alone
 *   int32  reserved[2]    0
 *   int32  k[64]          strictly increasing step indices, k[0] >= 0
 *   float  lr[64]         the rate at each knot (finite, >= 0)
 *   int32  hold[64]       1: lr[i] holds on [k[i], k[i+1]); 0: linear from lr[i] to lr[i+1]
 * Slots at and past n_knots are never used, whatever they hold.  The caller writes the block in stream order between
 * launches; the launches only read it.
 *
 * The value at s = steps_done, the 0-based index of the step being taken (the first step uses the value at 0):
 *   lr[0] for s < k[0];  lr[n-1] for s >= k[n-1];  lr[i] on a hold segment;  on a linear segment the float32 rounding of
 *     (double)lr[i] + ((double)lr[i+1] - (double)lr[i]) * ((double)(s - k[i]) / (double)(k[i+1] - k[i]))
 *   with one float64 division, one multiplication and one addition, each rounded on its own (no FMA contraction);
 *   the value is then multiplied by `scale` as one rounded float32 product.
 * dctn_lr_schedule_value runs exactly this arithmetic on the HOST over a host copy of the block (no device, no stream).
 * It validates the block - n_knots in 1..64, k[0] >= 0 and k strictly increasing, every used lr and the scale finite and
 * >= 0, step >= 0 - and returns DCTN_ERR_BAD_SHAPE otherwise; the step entry points below do not read the block on the
 * host and validate nothing of it.
 *
 * dctn_adam_l2_step_scheduled : dctn_adam_l2_step with the rate taken from `schedule` instead of state->lr (which the
 *   launch does not read).  master_or_null: null, or the float32 master copy of bf16 parameters (dtype must then be
 *   DCTN_BF16; as dctn_adam_l2_step_master).  guard_or_null: null, or the guard block (as the guarded steps:
 *   dctn_grad_guard_check ran in front).  The launch leaves steps_done + 1 AND the rate it used in the state block, so
 *   state->lr reports the rate of the step just taken.  A halted guarded launch writes nothing: steps_done stays, and
 *   with it the schedule's position.  Given lr = the schedule's value, every result is, bit for bit, what the
 *   unscheduled entry points leave.
 * dctn_sgd_l2_step_scheduled : dctn_sgd_l2_step with a device state block of the same 16 bytes
 *   {int32 steps_done, float lr, uint32 ticket, uint32 reserved} (zeroes before the first step): first_step is
 *   steps_done == 0 read on the device, the rate comes from `schedule`, and the launch leaves steps_done + 1 and the
 *   rate it used.  master_or_null / guard_or_null as above.
 * Return codes, decided on the host before any launch: DCTN_ERR_NULL, DCTN_ERR_BAD_SHAPE, DCTN_ERR_BAD_DTYPE as the
 * unscheduled steps.  No workspace; the calls only enqueue and can be captured.  These launches do not report to
 * dctn_last_kernel.
 * ------------------------------------------------------------------------------------------ */
size_t dctn_lr_schedule_bytes(void);
int dctn_lr_schedule_value(const void* host_block, int64_t step, float* out);
int dctn_adam_l2_step_scheduled(void* master_or_null, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                                void* sq_sum, void* state, const void* guard_or_null, const void* schedule, int64_t n,
                                int64_t n_reg, double beta1, double beta2, float eps, float weight_decay, float l2,
                                int dtype, void* stream);
int dctn_sgd_l2_step_scheduled(void* master_or_null, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                               void* state, const void* guard_or_null, const void* schedule, int64_t n, int64_t n_reg,
                               float momentum, float l2, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter groups (version 511): one optimizer launch obeys a table that gives every parameter of the flat buffer its
 * own rate multiplier, weight decay, frozen flag and step count (the reference freezes cores with requires_grad = False
 * and torch.optim.Adam then skips them: new_runner.py:443-444, :496-498).
 *
 * `groups`: dctn_param_groups_bytes = 1552 bytes, 16-byte aligned, laid out as
 *   int32   n_segments        1..64
 *   int32   reserved[3]       0
 *   int64   end[64]           exclusive element index where a segment ends; strictly increasing; the last used one is n
 *   float   lr_scale[64]      multiplies the rate; 1.0f leaves the bits alone
 *   float   weight_decay[64]  the segment's coupled weight decay (of the SGD steps only dctn_sgd_flat_step_decay uses it)
 *   uint32  flags[64]         bit 0: frozen
 *   int32   steps[64]         steps the segment has taken; the launch advances it
 * One segment is one parameter, in flat order: elements [end[s-1], end[s]), end[-1] = 0.  Slots at and past n_segments
 * are never used, whatever they hold.  The caller writes the block in stream order between launches.  The regularised
 * set stays the prefix n_reg (it may end inside a segment) and l2 stays one scalar.
 *
 * Semantics:
 *   The rate of a segment is ONE rounded float32 product rate * lr_scale, where rate is state->lr, or with a schedule
 *     its value at the GLOBAL steps_done.  lr_scale == 1.0f leaves the bits unchanged.
 *   Adam's bias corrections use the SEGMENT's count steps + 1 (torch.optim.Adam's per-parameter state["step"]), formed
 *     in float64 exactly as the ungrouped step forms them from steps_done + 1.
 *   SGD's first step (the momentum buffer takes the gradient) is steps == 0 of the segment.
 *   A frozen segment: no element of params, master, exp_avg, exp_avg_sq or momentum_buf is stored to, its gradient is
 *     not read, and its steps does not advance.  Its w * w still goes into sq_sum where it lies under n_reg (the
 *     reference's regulariser sums every core whatever requires_grad says; only the gradient term is dropped).
 *   The launch writes steps + 1 for every unfrozen segment, beside steps_done + 1 (the GLOBAL count of launches that
 *     were not halted); with a schedule state->lr gets the global rate, before any segment's scale.
 *   A halted guarded launch writes nothing and advances nothing.
 *   When every segment has lr_scale 1 and one weight_decay, none is frozen and every count equals steps_done, the
 *     launch leaves the ungrouped launch's bits (with that weight_decay) in every buffer, the sq_sum slots included.
 *
 * dctn_adam_l2_step_grouped : dctn_adam_l2_step_scheduled's arguments with `groups` behind the schedule and without
 *   weight_decay (the table holds it).  master_or_null / guard_or_null as there; schedule_or_null: null reads state->lr.
 * dctn_sgd_l2_step_grouped : dctn_sgd_l2_step_scheduled's arguments with `groups` behind the schedule.  It always takes
 *   the 16-byte state block; with schedule_or_null null it reads state->lr, as the Adam step does.
 * dctn_param_groups_check : HOST only, over a host copy of the block: n_segments in 1..64, end[0] >= 1 and strictly
 *   increasing with end[n_segments-1] == n, every used lr_scale and weight_decay finite and >= 0, no flag bit but bit 0,
 *   steps >= 0; DCTN_ERR_BAD_SHAPE otherwise.
 * The step entry points do not read the block on the host and validate nothing of it.  A malformed table may give a
 * wrong update; it never gives an access outside the buffers: the kernels keep the segment index inside the used
 * slots (n_segments clamped to 1..64), let the last used segment reach to n, and index elements only by i < n.
 * Return codes as the scheduled steps.  No workspace; the calls only enqueue and can be captured.  These launches do
 * not report to dctn_last_kernel.
 * ------------------------------------------------------------------------------------------ */
size_t dctn_param_groups_bytes(void);
int dctn_param_groups_check(const void* host_block, int64_t n);
int dctn_adam_l2_step_grouped(void* master_or_null, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                              void* sq_sum, void* state, const void* guard_or_null, const void* schedule_or_null,
                              void* groups, int64_t n, int64_t n_reg, double beta1, double beta2, float eps, float l2,
                              int dtype, void* stream);
int dctn_sgd_l2_step_grouped(void* master_or_null, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                             void* state, const void* guard_or_null, const void* schedule_or_null, void* groups,
                             int64_t n, int64_t n_reg, float momentum, float l2, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One description of a flat-optimizer step (version 512).  Master weights, the guard, the schedule and the group table
 * are four options that do not depend on one another; dctn_flat_step_t names every buffer and block of a step once, an
 * option that is off is a NULL pointer, and one entry point per optimizer takes it.  The twelve dctn_adam_l2_step* /
 * dctn_sgd_l2_step* entry points above are conveniences over these two: each fills the struct and launches the same
 * kernel with the same arguments.
 *
 * dctn_flat_step_t: dctn_flat_step_bytes() = 88 bytes on the HOST, read during the call only (the caller may keep one
 * for the life of an optimizer and rewrite `grads` per step).  Every pointer in it is a DEVICE pointer:
 *   void*       params    n values of `dtype`; with `master` they are bf16, OVERWRITTEN and never read
 *   void*       master    NULL, or the float32 master copy of bf16 parameters (dtype must then be DCTN_BF16)
 *   const void* grads     n values of `dtype`
 *   void*       sq_sum    NULL, or dctn_*_l2_num_partials(n) float32 slots, OVERWRITTEN
 *   void*       state     the 16-byte step block {steps_done, lr, ticket, reserved}.  Adam: required.  SGD: required
 *                         with a schedule or a group table, and not looked at otherwise
 *   const void* guard     NULL, or the 32-byte guard block: the step obeys it (dctn_grad_guard_check ran in front)
 *   const void* schedule  NULL, or the 784-byte schedule block: the rate is its value at steps_done, not state->lr
 *   void*       groups    NULL, or the 1552-byte group table.  Adam then takes every segment's weight decay from it
 *                         and ignores its weight_decay argument
 *   int64_t     n, n_reg  elements of the flat buffer; the first n_reg are regularised
 *   float       l2        the regulariser's coefficient
 *   int         dtype     DCTN_F32 / DCTN_BF16
 * dctn_adam_flat_step : the struct plus exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay (dctn_adam_l2_step's).
 * dctn_sgd_flat_step  : the struct plus momentum_buf, lr, momentum, first_step (dctn_sgd_l2_step's).  With a schedule or
 *   a group table lr and first_step are not used: both are read from the step block on the device.
 * Return codes, decided on the host before any launch: DCTN_ERR_NULL (the struct, or a required pointer), then
 * DCTN_ERR_BAD_SHAPE (n < 1, n_reg outside 0..n; Adam: a beta outside [0, 1)), then DCTN_ERR_BAD_DTYPE (a dtype that is
 * neither DCTN_F32 nor DCTN_BF16, or a master copy beside one that is not DCTN_BF16).  The semantics of every option are
 * stated with its block above.  No workspace; the calls only enqueue and can be captured.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  void *params, *master;
  const void* grads;
  void* sq_sum;
  void* state;
  const void *guard, *schedule;
  void* groups;
  int64_t n, n_reg;
  float l2;
  int dtype;
} dctn_flat_step_t;
size_t dctn_flat_step_bytes(void);
int dctn_adam_flat_step(const dctn_flat_step_t* step, void* exp_avg, void* exp_avg_sq, double beta1, double beta2,
                        float eps, float weight_decay, void* stream);
int dctn_sgd_flat_step(const dctn_flat_step_t* step, void* momentum_buf, float lr, float momentum, int first_step,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * A weight average (EMA) inside the flat step (version 514): the fifth option of a flat step, independent of the other
 * four.  A float32 buffer `ema` of n values sits beside the flat parameter buffer.  In the launch that updates the
 * parameters, every element the step stores to also updates its average from the value the optimizer KEEPS for that
 * element: with a master copy the float32 master value; without one the parameter as stored, rounded to `dtype` and
 * widened again.  The update is three float32 operations, each rounded on its own (no FMA), so numpy float32 gives the
 * same bits:
 *     ema = ema + omd * (w_new - ema)
 * omd is one float32 per launch: omd = (float)(1.0 - d_u), formed in float64; d_u = decay, or with the warm-up flag
 * d_u = min(decay, (1 + u) / (10 + u)) (one float64 division), u = the block's count of updates done so far.
 *
 * The block: dctn_weight_ema_bytes() = 32 bytes, 16-byte aligned, on the DEVICE:
 *   float   decay        in [0, 1); the caller writes it in stream order between launches
 *   uint32  flags        bit 0: warm-up
 *   int32   updates      updates done so far; the launch advances it
 *   float   last_omd     the weight the last update used; 0 before the first
 *   int32   reserved[4]  0
 * The launch reads decay, flags and updates beside steps_done (no load depends on another); the workgroup that draws the
 * last ticket of the step block writes updates + 1 and last_omd.
 *
 * With the other options: a halted guarded launch writes nothing - ema, updates and last_omd stay.  A frozen segment's
 * ema is not stored to, exactly as its moments are not.  decay == 0 makes omd == 1; the three operations still run.  The
 * step itself is unchanged: with or without the average every other buffer, block and sq_sum slot holds the same bits.
 * SGD: with an average the 16-byte step block is required, as with a schedule or a group table; the rate (state->lr
 * without a schedule) and first_step = (steps_done == 0) are read from it on the device, and the launch advances it.
 *
 * dctn_weight_ema_t: 16 bytes on the HOST, read during the call only; both members are DEVICE pointers.
 * dctn_adam_flat_step_ema / dctn_sgd_flat_step_ema: dctn_adam_flat_step / dctn_sgd_flat_step with the average;
 *   ema_or_null == NULL is exactly those.  Return codes in their order: DCTN_ERR_NULL also for a given dctn_weight_ema_t
 *   with a null member and, for SGD, a missing step block; then shape; then dtype.  Nothing of the block is validated: a
 *   bad block gives a wrong average, never an access outside the n floats.
 * dctn_weight_ema_weight: HOST only, over a host copy of the block: the kernels' float64 arithmetic for the launch at
 *   `updates`.  DCTN_ERR_NULL for a null pointer; DCTN_ERR_BAD_SHAPE for a decay outside [0, 1) or not finite, unknown
 *   flag bits, a negative count (the block's or the argument; the argument is also at most 2^31 - 1).
 * dctn_weight_ema_apply: ONE launch: stash[i] = params[i], then params[i] = (dtype)ema[i] with the round-to-nearest-even
 *   cast of the step kernels.  It never touches a master copy.  dctn_weight_ema_restore copies params back from stash.
 *   stash: n values of `dtype`.  DCTN_ERR_NULL, then n < 1: DCTN_ERR_BAD_SHAPE, then DCTN_ERR_BAD_DTYPE.
 * All of these only enqueue and can be captured.  None reports to dctn_last_kernel.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  void* ema;
  void* block;
} dctn_weight_ema_t;
size_t dctn_weight_ema_bytes(void);
int dctn_weight_ema_weight(const void* host_block, int64_t updates, float* one_minus_decay);
int dctn_adam_flat_step_ema(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* exp_avg,
                            void* exp_avg_sq, double beta1, double beta2, float eps, float weight_decay, void* stream);
int dctn_sgd_flat_step_ema(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* momentum_buf,
                           float lr, float momentum, int first_step, void* stream);
int dctn_weight_ema_apply(void* params, void* stash, const void* ema, int64_t n, int dtype, void* stream);
int dctn_weight_ema_restore(void* params, const void* stash, int64_t n, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RMSprop on the flat path, and weight decay for the flat SGD (version 515): with dctn_adam_flat_step the four
 * optimizers the reference's training scripts build (new_runner.py:496-498, mnist.py:466-476).
 *
 * dctn_rmsprop_flat_step: torch.optim.RMSprop(lr, alpha, eps, weight_decay, momentum, centered=False) plus the fused L2
 * term, ONE launch over the flat buffer described by a dctn_flat_step_t.  Per element, in float32, every product-sum one
 * fused multiply-add in this order (g after the guard's clip, one rounded product g * coef):
 *     g   = fma(wd, w, g)
 *     g   = fma(2 * l2, w, g)                      below n_reg; sq_sum takes w * w
 *     sq  = fma(alpha, sq, (oma * g) * g)          oma = (float)(1.0 - alpha), formed in double
 *     avg = sqrt(sq) + eps                         correctly rounded square root and division
 *     buf = fma(momentum, buf, g / avg);  w = fma(-rate, buf, w)        with a momentum buffer
 *                                         w = fma(-rate, g / avg, w)    without one
 * There is no first-step case: square_avg and the buffer start from zeros, as torch's.
 *   square_avg            n float32 values, read and written
 *   momentum_buf_or_null  n float32 values, required when momentum > 0.  momentum == 0: no buffer exists; the pointer
 *                         is not looked at and the launch moves nothing for it
 *   state                 the 16-byte step block, REQUIRED: the rate is read from it (or, with a schedule, evaluated at
 *                         its steps_done and left in it), and the launch advances steps_done as dctn_adam_flat_step's
 *   sq_sum                NULL, or dctn_rmsprop_num_partials(n) float32 slots, OVERWRITTEN
 * Master copy, guard, schedule, group table and weight average mean what they mean for dctn_adam_flat_step_ema, Adam's
 * per-segment bias corrections aside: a segment steps with rate * lr_scale and its own weight decay, a frozen one is not
 * touched (its squares still count in sq_sum) and its `steps` does not advance.  With a group table the weight_decay
 * argument is ignored.
 * Return codes, decided on the host before any launch: DCTN_ERR_NULL (the struct, params, grads, square_avg or state; a
 * given dctn_weight_ema_t with a null member; momentum > 0 without a buffer), then DCTN_ERR_BAD_SHAPE (n < 1, n_reg
 * outside 0..n, alpha outside [0, 1) or not finite, momentum < 0, eps < 0, weight_decay < 0), then DCTN_ERR_BAD_DTYPE
 * (a dtype that is neither DCTN_F32 nor DCTN_BF16, or a master copy beside one that is not DCTN_BF16).
 *
 * dctn_sgd_flat_step_decay: dctn_sgd_flat_step_ema with torch.optim.SGD's coupled weight decay, g = fma(wd, w, g) in
 * front of the 2 * l2 * w term and the momentum.  With a group table every segment takes the table's weight_decay and
 * the argument is ignored.  weight_decay == 0 leaves the bits of dctn_sgd_flat_step_ema (it launches other kernels).
 * Return codes: dctn_sgd_flat_step_ema's, and weight_decay < 0 (or NaN) is DCTN_ERR_BAD_SHAPE.
 * Both only enqueue and can be captured.  Neither reports to dctn_last_kernel.
 * ------------------------------------------------------------------------------------------ */
int dctn_rmsprop_flat_step(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* square_avg,
                           void* momentum_buf_or_null, double alpha, float eps, float weight_decay, float momentum,
                           void* stream);
int dctn_rmsprop_num_partials(int64_t n);
int dctn_sgd_flat_step_decay(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* momentum_buf,
                             float lr, float momentum, float weight_decay, int first_step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring(reference: dctn/evaluation.py:7-22): one launch per batch ADDS to acc = three float64 values
 * {sum of the rows' cross-entropies, number of correct rows, number of rows}.  logits (B, C) contiguous, DCTN_F32 /
 * DCTN_BF16; labels int64.  Per row a max-shifted log-sum-exp with float32 exponentials; the row's sum, its
 * logarithm and the sums over the rows are float64, in a fixed order: the same bits from run to run (the float32
 * logarithm of gfx950 is low by about 0.4 ulp on average for such sums, which would add up over a batch); a row is correct when its label equals the LOWEST index among the
 * row's maxima (torch.argmax).  Rows labelled -100 are skipped and not counted; any other label outside [0, C) makes
 * sum_loss NaN and counts as a wrong row.  acc is read and written in stream order (no atomics, no fill per batch);
 * the caller zeroes it once.
 * ------------------------------------------------------------------------------------------ */
int dctn_ce_score_accumulate(const void* logits, const void* labels, void* acc, int64_t B, int C, int dtype,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Step trace (version 509): ONE launch at the end of a training iteration writes one 64-byte record into a ring on the
 * DEVICE and advances a device counter, so that a captured graph which holds the launch - once, or K times for K
 * iterations per graph launch - fills consecutive slots on its replays and the host reads nothing per iteration.
 *
 * `head`: dctn_step_trace_head_bytes() = 16 bytes, 16-byte aligned, laid out as
 *   uint32 records_done   records written so far; the launch reads seq = records_done and leaves records_done + 1
 *   uint32 ticket         0 (the launch is one workgroup and draws no ticket; the word is kept for a split form)
 *   uint32 reserved[2]    0
 * The caller zeroes it once and may read or write it in stream order between launches.
 * `ring`: capacity records of dctn_step_trace_record_bytes() = 64 bytes, 16-byte aligned; capacity >= 1 may be any
 * number, not only a power of two.  The launch writes slot seq % capacity.  (seq is 32 bits: when it wraps, the slot jumps
 * for a capacity that is no power of two.)
 *
 * Record (little-endian, EVERY byte of the 64 written by every launch; a field whose block is absent is 0):
 *   offset  0  uint32 seq
 *           4  uint32 present         DCTN_TRACE_HAS_REG | _GUARD | _ADAM | _SOURCE: which optional blocks were given
 *           8  float  loss            the bits of loss[0] (float32 device scalar)
 *          12  float  reg             the bits of reg_or_null[0] (float32 device scalar)
 *          16  int32  rows            rows of the batch whose label is not -100
 *          20  int32  correct         of those, the rows whose label equals the LOWEST index among the row's maxima
 *          24  float  grad_norm       guard block: last_norm   } the block of dctn_grad_guard_check (32 bytes) as it
 *          28  float  coef            guard block: coef        } stands when the launch runs: placed after the
 *          32  uint32 halted          guard block: halted      } optimizer step, it shows this iteration's check
 *          36  int32  bad_step        guard block: bad_step    }
 *          40  int32  opt_steps_done  Adam block (16 bytes, dctn_adam_l2_step): steps_done, after the step
 *          44  float  lr              Adam block: lr
 *          48  uint32 batches_done    batch source block (16 bytes, dctn_batch_draw): batches_done as read (after the
 *                                     iteration's draw: the number of this batch + 1)
 *          52  12 bytes of zero
 * rows / correct follow dctn_ce_score_accumulate's rules exactly: logits (B, C) contiguous, DCTN_F32 / DCTN_BF16, labels
 * int64; rows labelled -100 are skipped; any other label outside [0, C) counts as a wrong row; the maximum of a row is
 * taken with fmaxf, so a NaN logit is never the maximum and a row of nothing but NaN is a wrong row.  Integer counts: the
 * record is the same bits from run to run.
 *
 * Buffer contract: `head` (records_done) and the one addressed slot are written, with vector stores; nothing else is.
 * Logits, labels, loss, reg and the three state blocks are only read.  No workgroup waits for another.  The call
 * allocates nothing and synchronises nothing: it only enqueues and can be captured.  Return codes, decided on the host
 * before any launch: DCTN_ERR_NULL (logits, labels, loss, head, ring); DCTN_ERR_BAD_SHAPE (B < 1, C < 1, capacity < 1);
 * DCTN_ERR_BAD_DTYPE.  No workspace.  This launch does not report to dctn_last_kernel.
 * ------------------------------------------------------------------------------------------ */
#define DCTN_TRACE_HAS_REG 1
#define DCTN_TRACE_HAS_GUARD 2
#define DCTN_TRACE_HAS_ADAM 4
#define DCTN_TRACE_HAS_SOURCE 8
size_t dctn_step_trace_head_bytes(void);
size_t dctn_step_trace_record_bytes(void);
int dctn_step_trace_record(const void* logits, const void* labels, const void* loss, const void* reg_or_null,
                           const void* guard_or_null, const void* adam_state_or_null, const void* batch_state_or_null,
                           void* head, void* ring, int capacity, int64_t B, int C, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Component dropout of the EPS cores (version 502; reference: dctn/eps_plus_linear.py:139-143, `mask * core / p` with
 * mask ~ Bernoulli(p) per component of every core): ONE launch each way for all cores of a model, and a mask that is
 * stored nowhere - a pure function of (seed, draw, core number, element index).
 *
 * Mask definition (normative; dctn_amd/dropout.py `expected_keep` restates it in Python).  The generator is
 * Philox4x32-10: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; the key (k0, k1) grows by (0x9E3779B9, 0xBB67AE85)
 * after every round; one round maps the counter (c0, c1, c2, c3) to
 *   (hi(M1*c2) ^ c1 ^ k0,  lo(M1*c2),  hi(M0*c0) ^ c3 ^ k1,  lo(M0*c0)).
 * Element e of the s-th core of a call (s = its index in the pointer arrays), under draw d and the 64-bit seed:
 *   counter = (e >> 2, 0, d, s),  key = (seed & 0xFFFFFFFF, seed >> 32),  word = output word (e & 3);
 *   the element is KEPT iff word < T,  T = min(floor(p * 2^32), 2^32 - 1), formed in double from the value of p as
 *   the tensor dtype stores it (the bfloat16 "0.9" is 0.8984375 - the probability the reference's bernoulli() sees too).
 * fwd : out = keep ? core / p : 0        bwd : d_core = keep ? d_out / p : 0        mask : keep ? 1 : 0
 * One division in float32 (double for DCTN_F64), rounded once to the tensor dtype.  For finite inputs fwd compares
 * equal to the reference's `mask * core / p` evaluated in the tensor dtype (a dropped value is +0 here and a zero of
 * either sign there; bfloat16 is rounded once here as there, since mask * core is exact).  A NON-FINITE dropped
 * component gives 0 here where the reference's 0 * inf gives NaN.
 *
 * Arguments.  cores / out / d_out / d_core / mask: HOST arrays of n_cores device pointers, numel: HOST array of their
 * element counts (contiguous tensors of `dtype`: DCTN_F32 / DCTN_F64 / DCTN_BF16, aligned to their element size; a core
 * whose bases are 16-byte aligned (bf16: 8) moves in vector accesses).  1 <= n_cores <= 8 (more: DCTN_ERR_UNSUPPORTED);
 * 1 <= numel[i] < 2^34 (DCTN_ERR_BAD_SHAPE: e >> 2 is one 32-bit counter word).  p: DEVICE pointer to one value of
 * `dtype`, 0 < p <= 1.  d_core[i] may be the same pointer as d_out[i] (in place); no other overlap is allowed.  In
 * dctn_core_dropout_bwd a core whose d_out[i] and d_core[i] are both NULL is skipped (a frozen core); it keeps its number.
 *
 * `state`: dctn_core_dropout_state_bytes() = 16 bytes on the device, 16-byte aligned, laid out as
 *   uint32 seed_lo, uint32 seed_hi   the seed; read by every forward launch
 *   uint32 draws_done                number of forward launches so far; a launch draws with d = draws_done as read at
 *                                    its start and leaves d + 1 here
 *   uint32 ticket                    0 between launches (workgroups count themselves out on it; the last one resets it)
 * The caller creates the block once (seed, 0, 0) and may read or write it in stream order between launches.  `record`:
 * 16 bytes on the device, 4-byte aligned; the forward OVERWRITES it with {seed_lo, seed_hi, d, 0}; the backward and the
 * mask kernel read it and `p` and nothing else of the state - they never touch the block.  No entry point reads the
 * device on the host: every call only enqueues, so a captured graph that holds the forward draws d, d + 1, ... on its
 * replays, and its backward node follows through the record.
 *
 * Buffer contract: out / d_core / mask are fully OVERWRITTEN (every element, whatever they held - NaN included),
 * nothing outside them, the record and (fwd) the block is written, and no result depends on what an output held
 * before (in-place bwd reads d_out, which is then the output, by definition).  No workspace.
 * dctn_last_kernel(): core_dropout_{fwd,bwd,mask}_{f32,f64,bf16}.
 * ------------------------------------------------------------------------------------------ */
size_t dctn_core_dropout_state_bytes(void);
int dctn_core_dropout_fwd(const void* const* cores, void* const* out, const int64_t* numel, int n_cores, const void* p,
                          void* state, void* record, int dtype, void* stream);
int dctn_core_dropout_bwd(const void* const* d_out, void* const* d_core, const int64_t* numel, int n_cores, const void* p,
                          const void* record, int dtype, void* stream);
int dctn_core_dropout_mask(void* const* mask, const int64_t* numel, int n_cores, const void* p, const void* record,
                           int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident batch source (version 503; reference: the train DataLoader of dctn/dataset_loading.py:69-70, 282-286,
 * 319-325 - __getitem__ per sample, collate_quantum, pinning and a copy).  ONE launch picks the samples of a batch, moves
 * them into the model's input layout and dtype and advances a device counter; the epoch order is stored nowhere - a pure
 * function of (seed, epoch, position).
 *
 * Order definition (normative; dctn_amd/batches.py `round_keys` / `order_at` restate it in Python).  Position i of epoch
 * e over n samples (1 <= n < 2^31) under the 64-bit seed maps to a sample through a bijection on [0, 2^b),
 * b = max(2, bit length of n - 1), applied again while the value is >= n (cycle walking: i < n lies on a cycle of the
 * bijection, so the walk comes back below n; the result is a bijection on [0, n)).
 *   round keys  K[0..5] = the first six words of Philox4x32-10(counter (0, 0, e, TAG), key) followed by
 *               Philox4x32-10(counter (1, 0, e, TAG), key), TAG = 0x53485546, key = (seed & 0xFFFFFFFF, seed >> 32) - the
 *               generator of the dropout section above, whose counters keep c3 below 8
 *   mix32(h)    h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16      (32-bit arithmetic)
 *   one pass    wl = b / 2, wr = b - wl;  L = v >> wr, R = v & (2^wr - 1);
 *               six times, j = 0..5:  (L, R) = (R, L ^ (mix32(R ^ K[j]) & (2^wl - 1))), then wl and wr change places;
 *               result (L << wr) | R
 * Batch k (the device counter) with global batch G and S = n / G batches per epoch (the remainder of an epoch is dropped):
 * epoch e = k / S; the launch of a rank whose shard starts at rank_offset takes positions (k % S) * G + rank_offset + j,
 * j < local_batch.  With DCTN_BATCH_IDENTITY_ORDER in `flags` the sample IS the position (a sequential pass).
 * DCTN_BATCH_PAD_TAIL (version 504; only together with DCTN_BATCH_IDENTITY_ORDER) makes that pass cover ALL n samples with
 * batches of one fixed shape: S = ceil(n / G), the positions are the same expression with this S, and a slot whose position
 * is >= n is padding: its x row is the row of sample n - 1 (fully written, finite), y[j] = -100 (the label
 * dctn_ce_score_accumulate and dctn_ce_loss_* skip) and indices[j] = -1.  Slots with a position below n are exactly what the
 * identity order gives without the flag.  S draws that start at k = 0 (mod S) walk every sample once and leave the counter
 * at 0 (mod S) again.  S * G exceeds n by up to G - 1; G <= n < 2^31 keeps every position below 2^32.  The counter word
 * means a different S with and without the flag: one block serves one of the two forms.  The flag selects instantiations
 * of their own (same kernel names): a draw without it runs code that holds no trace of it.
 *
 * dctn_batch_draw   : sample numbers from `state`; the launch draws batch k = batches_done as read at its start and
 *                     leaves k + 1.  It only enqueues and never reads the device on the host: a captured graph that holds
 *                     it draws k, k + 1, ... on its replays.
 * dctn_batch_gather : the same data movement for `count` sample numbers given as a DEVICE int64 array; reads no state and
 *                     takes no ticket (sequential evaluation passes, eager use).  Every number must lie in [0, n): the
 *                     caller's contract, not checked.
 * Source kinds (`row_len`, `width` describe the geometry):
 *   DCTN_BATCH_SRC_U8_TABLE : src = raw uint8 intensities (n, P), P = row_len pixels (what torchvision's `.data` holds);
 *       table = (256, Q) values of `dtype`, Q = width, 1 <= Q <= 4 (phi, the scale and the cast, folded in by the caller);
 *       x = (1, local_batch, P, Q):  x[0, j, p, :] = table[src[s_j, p], :].  The workgroup stages the table in LDS; four
 *       pixels move per 32-bit load when P % 4 == 0 and src is 4-byte aligned (and x 16-byte aligned; 8 for bf16 with
 *       odd Q), pixel by pixel otherwise.
 *   DCTN_BATCH_SRC_ROWS     : src = features already expanded, (C, n, R) values of `dtype`, R = row_len, C = width <= 4;
 *       x = (C, local_batch, R):  x[c, j, :] = src[c, s_j, :] (16-byte accesses when both bases and R * sizeof allow);
 *       table is ignored (may be NULL).
 * Both write y[j] = labels[s_j] and indices[j] = s_j (int64; labels: n int64 values).  dtype: DCTN_F32 / F64 / BF16; all
 * tensors contiguous and aligned to their element size.
 *
 * `state`: dctn_batch_state_bytes() = 16 bytes on the device, 16-byte aligned, laid out as
 *   uint32 seed_lo, uint32 seed_hi   the seed; read by every draw
 *   uint32 batches_done              number of draws so far (a 32-bit counter: it wraps after 2^32 batches)
 *   uint32 ticket                    0 between launches (workgroups count themselves out on it; the last one resets it)
 * The caller creates the block once (seed, 0, 0) and may read or write it in stream order between launches; ranks that
 * hold the same block and pass their own rank_offset draw disjoint shards of the same global batch.
 *
 * Buffer contract: x, y, indices are fully OVERWRITTEN (every element, whatever they held), nothing outside them is
 * touched; src, table, labels and sample_idx are never written; of the block only batches_done and ticket change.
 * Return codes, all decided on the host before any launch: DCTN_ERR_NULL; DCTN_ERR_BAD_SHAPE (n < 1, n >= 2^31,
 * global_batch > n or < 1, local_batch / count < 1, rank_offset + local_batch > global_batch, row_len or width < 1, an
 * unknown src_kind or flag, DCTN_BATCH_PAD_TAIL without DCTN_BATCH_IDENTITY_ORDER); DCTN_ERR_BAD_DTYPE;
 * DCTN_ERR_UNSUPPORTED (width > 4).  No workspace.
 * dctn_last_kernel(): batch_{draw,gather}_{u8,rows}_{f32,f64,bf16}.
 * ------------------------------------------------------------------------------------------ */
/* DCTN_BATCH_SRC_COLOUR (version 513) is the colour source below: dctn_batch_call_t names it; dctn_batch_draw and
 * dctn_batch_gather refuse it (DCTN_ERR_BAD_SHAPE), as they refuse an unknown kind. */
enum { DCTN_BATCH_SRC_U8_TABLE = 0, DCTN_BATCH_SRC_ROWS = 1, DCTN_BATCH_SRC_COLOUR = 2 };
enum { DCTN_BATCH_IDENTITY_ORDER = 1 };   /* `flags` of dctn_batch_draw */
/* `flags` of dctn_batch_draw, version 504: with DCTN_BATCH_IDENTITY_ORDER only.  A macro beside the enum, not a member of
 * it: tests/test_host_batches.py takes every `DCTN_BATCH_x = n` of this header for the complete list of the version 503
 * constants; tests/test_host_eval_pass.py reads this line and holds dctn_amd/_lib.py to it. */
#define DCTN_BATCH_PAD_TAIL 2
size_t dctn_batch_state_bytes(void);
int dctn_batch_draw(const void* src, const void* table, const void* labels, void* x, void* y, void* indices, void* state,
                    int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset, int64_t row_len, int width,
                    int src_kind, int flags, int dtype, void* stream);
int dctn_batch_gather(const void* src, const void* table, const void* labels, const void* sample_idx, void* x, void* y,
                      void* indices, int64_t n, int64_t count, int64_t row_len, int width, int src_kind, int dtype,
                      void* stream);

/* Raw colour images (version 506; reference: get_cifar10_colored_data_loaders, dctn/dataset_loading.py:331-389 -
 * to_tensor, the optional per-channel centring and scaling, the optional constant channel, the per-channel nu).  Every
 * value of that pipeline is a function of one byte and its channel, so one 256-row table per channel holds them all
 * (dctn_amd/batches.py `colour_table`).  A third source form with entry points of its own: the `src_kind` argument of
 * dctn_batch_draw / dctn_batch_gather keeps its two values.
 *   src   = (n, P, C) uint8, the channels interleaved (what torchvision's CIFAR10 `.data` holds), P = pixels,
 *           C = src_channels;
 *   table = (W, 256) values of `dtype`, W = width: row c is channel c's table;
 *   x     = (1, local_batch, P, W):  x[0, j, p, c] = table[c][src[s_j, p, c]]  for c < C,
 *                                    x[0, j, p, c] = table[c][0]               for C <= c < W (the constant channel).
 * 1 <= C <= 4 and W = C or C + 1 with W <= 4.  The byte offset of a row is 64-bit: n * P * C may pass 4 GiB.
 * The workgroup stages the table in LDS, planar as it is given.  A lane moves four pixels per step - C 32-bit loads, 4 W
 * elements in 16-byte stores (8-byte ones for bf16 with odd W) - when P % 4 == 0, src is 4-byte aligned and x is aligned
 * to that store width; pixel by pixel otherwise.  Same results either way.
 * dctn_batch_draw_cols / dctn_batch_gather_cols are dctn_batch_draw / dctn_batch_gather in everything else: the order
 * definition, the 16-byte `state` block and how a draw advances it, both flags (padding slots read sample n - 1 and
 * report the label -100 and the index -1), sharding by rank_offset, y and indices, the buffer contract (x, y, indices
 * fully overwritten, nothing else written but batches_done and ticket) and the return-code rules: DCTN_ERR_NULL (any
 * pointer; the table is always needed); DCTN_ERR_BAD_SHAPE (as above, with pixels, src_channels or width < 1);
 * DCTN_ERR_BAD_DTYPE; DCTN_ERR_UNSUPPORTED (src_channels > 4, width > 4, width < src_channels,
 * width > src_channels + 1).  No workspace.
 * dctn_last_kernel(): colour_{draw,gather}_{f32,f64,bf16}. */
int dctn_batch_draw_cols(const void* src, const void* table, const void* labels, void* x, void* y, void* indices,
                         void* state, int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset,
                         int64_t pixels, int src_channels, int width, int flags, int dtype, void* stream);
int dctn_batch_gather_cols(const void* src, const void* table, const void* labels, const void* sample_idx, void* x, void* y,
                           void* indices, int64_t n, int64_t count, int64_t pixels, int src_channels, int width, int dtype,
                           void* stream);

/* On-device augmentation of the two byte-resident sources (version 507): a random shift (pad and crop) and a horizontal
 * flip of the BYTES of every drawn sample, before the table lookup.  The reference has no augmentation (its README notes
 * that the model overfits CIFAR-10); these are torchvision's RandomCrop(padding = m, fill) and RandomHorizontalFlip in
 * distribution.
 *
 * Definition (normative; dctn_amd/batches.py `augment_params` / `augment_bytes` restate it in Python).  k is the batch
 * counter read at the launch's start, S = n / G the batches per epoch, e = k / S the epoch.  Slot j of the launch has the
 * GLOBAL position g = (k % S) * G + rank_offset + j - the position the order definition above maps to the sample s_j
 * (with DCTN_BATCH_IDENTITY_ORDER s_j = g).  The parameters of the slot:
 *   w = Philox4x32-10(counter (g, 0, e, DCTN_AUG_TAG), key (seed & 0xFFFFFFFF, seed >> 32)), DCTN_AUG_TAG = 0x41554731
 *       (disjoint from the order's 0x53485546 and from dropout's c3 < 8);
 *   with m = max_shift:  dy = (int)(((uint64)w[0] * (2 m + 1)) >> 32) - m,  dx the same expression on w[1],
 *                        flip = (aug_flags & DCTN_AUG_HFLIP) ? w[2] >> 31 : 0.
 * Output for image height H = height, width Wd = width_px, wf = flip ? Wd - 1 - w : w:
 *   grey   (dctn_batch_draw_aug):       x[0, j, h, w, :] = table[b, :]
 *   colour (dctn_batch_draw_cols_aug):  x[0, j, h, w, c] = table[c][b_c] for c < C, table[C][0] for the constant column
 * where b (b_c) is the source byte of sample s_j at row h + dy, column wf + dx (channel c) when that lies inside the
 * image, and the fill byte otherwise: one fill byte per source channel, packed in `fill` with channel c in bits
 * 8 c .. 8 c + 7.  This equals padding the byte image by m with the fill on every side, cropping an H x Wd window at
 * (m + dy, m + dx), flipping it horizontally, and then applying the unaugmented per-byte pipeline; the fill is in the
 * byte domain so that the result is bit for bit "augment the bytes, then expand".  The parameters depend on the global
 * position, never on the rank or the number of ranks: the global batch does not depend on how it is sharded.  y, indices,
 * the `state` block, the ticket and the counter advance are those of the unaugmented draw; there is no new device state,
 * so {"seed", "batches_done"} repeats the augmentations too, and a captured launch augments every replay differently.
 * The 32-bit words are mapped by multiply-high: the bias of a value is below 2^-32 * (2 m + 1).
 *
 * Arguments: those of dctn_batch_draw (without src_kind: the source is the uint8 one) and dctn_batch_draw_cols, with
 * row_len / pixels replaced by height, width_px, and max_shift, aug_flags, fill added.  src = (n, H, Wd) or
 * (n, H, Wd, C) uint8; x = (1, local_batch, H, Wd, width).  `flags` accepts DCTN_BATCH_IDENTITY_ORDER only: an evaluation
 * pass is not augmented, so DCTN_BATCH_PAD_TAIL is DCTN_ERR_BAD_SHAPE like an unknown bit.  There is no augmented gather.
 * Return codes, decided on the host before any launch, in this order: DCTN_ERR_NULL; DCTN_ERR_BAD_SHAPE (the rules of the
 * unaugmented draws with height, width_px or their product outside [1, 2^31); max_shift < 0 or >= 2^15; an unknown bit
 * in aug_flags; fill bits above the source channels); DCTN_ERR_BAD_DTYPE; DCTN_ERR_UNSUPPORTED (the width rules of the
 * unaugmented draws; a sample of more than 13 KiB, H * Wd * C rounded up to 16 bytes: a wave keeps its sample in LDS -
 * 64 x 64 x 3 fits).  Buffer contract as above; no workspace.
 * dctn_last_kernel(): aug_draw_{u8,cols}_{f32,f64,bf16}. */
#define DCTN_AUG_TAG 0x41554731u
enum { DCTN_AUG_HFLIP = 1 };   /* `aug_flags` */
int dctn_batch_draw_aug(const void* src, const void* table, const void* labels, void* x, void* y, void* indices, void* state,
                        int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset, int64_t height,
                        int64_t width_px, int width, int flags, int dtype, int max_shift, int aug_flags, uint32_t fill,
                        void* stream);
int dctn_batch_draw_cols_aug(const void* src, const void* table, const void* labels, void* x, void* y, void* indices,
                             void* state, int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset,
                             int64_t height, int64_t width_px, int src_channels, int width, int flags, int dtype,
                             int max_shift, int aug_flags, uint32_t fill, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One description of a batch-source launch (version 513).  The three source kinds, the two operations and the augmentation
 * are one data movement with options; dctn_batch_call_t names every buffer, shape and option of a launch once, and one
 * entry point per operation takes it - two, because a draw advances the state block and a gather has none.  The six entry
 * points above are conveniences over these two: each fills the struct and launches the same kernel with the same
 * arguments.  Everything said above about the order, the state block, the kinds, the augmentation and the buffer contract
 * holds here word for word.
 *
 * dctn_batch_call_t: dctn_batch_call_bytes() = 160 bytes on the HOST, read during the call only (the caller may keep one
 * for the life of a source and rewrite x, y, indices per launch; a captured launch holds no reference to it).  Every
 * pointer in it is a DEVICE pointer:
 *   const void* src          the data set, laid out as its kind says
 *   const void* table        the kind's table; DCTN_BATCH_SRC_ROWS ignores it (may be NULL)
 *   const void* labels       n int64 values
 *   const void* sample_idx   gather: `count` int64 sample numbers.  A draw ignores it
 *   void *x, *y, *indices    the outputs, fully overwritten
 *   void*       state        draw: the 16-byte block.  A gather ignores it
 *   int64_t n                samples of the data set
 *   int64_t global_batch, rank_offset   draw: G and the first position of this launch's shard.  A gather ignores them
 *   int64_t count            this launch's samples: the local_batch of a draw, the length of sample_idx of a gather
 *   int64_t row_len          pixels P of a sample (U8_TABLE, COLOUR), elements R of a row (ROWS)
 *   int64_t height, width_px augmented draws: the image's H and Wd, and row_len must equal H * Wd.  Ignored otherwise
 *   int src_kind             DCTN_BATCH_SRC_U8_TABLE, DCTN_BATCH_SRC_ROWS or DCTN_BATCH_SRC_COLOUR
 *   int src_channels         COLOUR: C.  Ignored by the other kinds (U8_TABLE has one source channel)
 *   int width                U8_TABLE: table columns Q;  ROWS: channels C;  COLOUR: output columns W
 *   int flags                draw: DCTN_BATCH_IDENTITY_ORDER, DCTN_BATCH_PAD_TAIL.  A gather ignores it
 *   int dtype                DCTN_F32 / DCTN_F64 / DCTN_BF16
 *   int augment              0: the plain kernels.  Not 0: the augmented ones - also with max_shift = 0 and no flip, which
 *                            moves the bytes unchanged through the augmented kernel.  Draws of U8_TABLE and COLOUR only
 *   int max_shift, aug_flags; uint32_t fill    the augmentation's arguments.  Ignored when augment is 0
 * Return codes, all decided on the host before any launch, in this order:
 *   DCTN_ERR_NULL         the struct; src, labels, x, y, indices; state (draw) or sample_idx (gather)
 *   DCTN_ERR_BAD_SHAPE    an unknown src_kind; augment with a gather or with DCTN_BATCH_SRC_ROWS
 *   DCTN_ERR_NULL         table, unless the kind is DCTN_BATCH_SRC_ROWS - only the kind says whether there is one, so it is
 *                         looked at in front of the table; the older entry points answered in this order and still do
 *   DCTN_ERR_BAD_SHAPE    every shape rule stated above: n, count, row_len outside [1, 2^31); width or src_channels < 1;
 *                         a draw's global_batch, rank_offset and flags (an augmented draw accepts the identity order
 *                         only); an augmented draw's height, width_px, their product against row_len, max_shift,
 *                         aug_flags and fill
 *   DCTN_ERR_BAD_DTYPE
 *   DCTN_ERR_UNSUPPORTED  width > 4; COLOUR: src_channels > 4 or width outside src_channels .. src_channels + 1; an
 *                         augmented sample of more than 13 KiB
 * No workspace; the calls only enqueue and can be captured.  dctn_last_kernel(): the names stated with each kind above.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void *src, *table, *labels;
  const void* sample_idx;
  void *x, *y, *indices;
  void* state;
  int64_t n, global_batch, count, rank_offset;
  int64_t row_len;
  int64_t height, width_px;
  int src_kind;
  int src_channels, width, flags, dtype;
  int augment;
  int max_shift, aug_flags;
  uint32_t fill;
} dctn_batch_call_t;
size_t dctn_batch_call_bytes(void);
int dctn_batch_draw_call(const dctn_batch_call_t* call, void* stream);
int dctn_batch_gather_call(const dctn_batch_call_t* call, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-run snapshots (version 508; the reference's runner only has --load-model-state): everything a training run keeps
 * on the device - the flat parameter buffer, the moments, the float32 master copy and the 16- / 32-byte state blocks of
 * the optimizer, the gradient guard, the dropout and the batch source - gathered into ONE contiguous arena by one launch
 * at one point of the stream, and put back in place by one launch.  dctn_amd/checkpoint.py is the host side.
 *
 * Layout (normative).  Region r of a call (r = its index in the pointer array) has bytes[r] >= 1 bytes and starts in the
 * arena at the sum of the earlier lengths, each rounded up to a multiple of 16; the arena's size is that sum over all
 * regions, which the arena-size query returns (0 for a NULL table, a count outside 1 .. 16 or a length < 1).  The
 * gather writes every byte of the arena: the bytes between a region's end and the next multiple of 16 are ZERO.
 *
 * Digest (normative; dctn_amd/checkpoint.py `digest` restates it in Python).  A region's bytes, zero-padded to a multiple
 * of 16, read as little-endian uint32 words w_0 .. w_(m-1):  s1 = sum of w_i,  s2 = sum of (i + 1) * w_i,  both mod 2^64.
 * Integer sums: every summation order gives the same bits.  `digests` receives {uint64 s1, uint64 s2} per region, 16
 * bytes each, in table order.  The gather digests what it READ from the regions, the scatter what it READ from the arena
 * (the region's bytes there; the arena's padding does not enter), so a host that recomputes the digest of the bytes it
 * received, or sent, checks the whole way.
 *
 * Arguments.  srcs / dsts: HOST array of n_regions device pointers, each a multiple of 4 (DCTN_ERR_UNSUPPORTED otherwise:
 * a bf16 view at an odd element); a region whose address is a multiple of 16 moves in 16-byte accesses, any other in
 * dwords; the last bytes[r] % 4 bytes move as a short and / or a byte, and no access reaches past a region's last byte.
 * bytes: HOST array of the lengths.  1 <= n_regions <= 16 as the max-regions query returns (more:
 * DCTN_ERR_UNSUPPORTED; the caller makes several calls).  arena: device, 16-byte aligned; arena_bytes must be exactly the
 * padded sum (DCTN_ERR_BAD_SHAPE).  digests: device, 8-byte aligned, 16 * n_regions bytes.  Regions must not overlap
 * each other or the arena.  The table travels by value in the kernel argument: the calls read no host memory after they
 * return and no device memory on the host, they only enqueue (a zeroing launch for the digest cells, then the one copy
 * launch: the cells are summed with 64-bit vector atomics, no workgroup waits for another) and can be captured.
 *
 * Buffer contract.  gather: the arena (all arena_bytes) and the 16 * n_regions digest bytes are fully OVERWRITTEN,
 * whatever they held; the regions are only read.  scatter: every byte of every region and the digest bytes are
 * OVERWRITTEN, nothing past a region's last byte is written, the arena is only read.  Nothing else is touched.  No
 * workspace.  Return codes, decided on the host before any launch: DCTN_ERR_NULL (table, an entry, arena, digests);
 * DCTN_ERR_BAD_SHAPE (n_regions < 1, a length < 1, arena_bytes off); DCTN_ERR_UNSUPPORTED (n_regions > 16, alignment).
 * These launches do not report to dctn_last_kernel.
 * ------------------------------------------------------------------------------------------ */
int dctn_state_max_regions(void);
size_t dctn_state_arena_bytes(const int64_t* bytes, int n_regions);
int dctn_state_gather(const void* const* srcs, const int64_t* bytes, int n_regions, void* arena, size_t arena_bytes,
                      void* digests, void* stream);
int dctn_state_scatter(const void* arena, void* const* dsts, const int64_t* bytes, int n_regions, void* digests,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * The tail of the ConvSBS classifier and the statistics of its strings' outputs (version 518; dctn_amd/csrc/sbs_tail.hip;
 * host side: dctn_amd/mnist_model.py, dctn_amd/tensor_stats.py).  Dtypes: DCTN_F32 / DCTN_F64 only.  None of the three
 * reports to dctn_last_kernel.  Return codes, decided on the host before any launch, in the project's order:
 * DCTN_ERR_NULL, DCTN_ERR_BAD_SHAPE, DCTN_ERR_BAD_DTYPE, DCTN_ERR_UNSUPPORTED (then DCTN_ERR_WORKSPACE where there is one).
 *
 * dctn_position_mean_fwd : the reference's einops.reduce(result, "b h w l -> b l", "mean") (mnist.py:263).  y: (B, P, L)
 *   contiguous, the final string's (B, H', W', L); out: (B, L), OVERWRITTEN.  out[b, l] = the sum over p in FLOAT64, divided by
 *   P in float64, rounded once to `dtype`.  B >= 1 (and < 2^31), P >= 1: DCTN_ERR_BAD_SHAPE otherwise; 1 <= L <= 64:
 *   DCTN_ERR_UNSUPPORTED otherwise.  One workgroup per sample with R L threads, R = 256 / L: thread t owns label t % L and
 *   the positions t / L, t / L + R, ...; the R partial sums of a label are added in that order.  Grid and summation order are
 *   a function of (P, L) alone, never of B or of the device: a sample's row has the same bits in whatever batch it sits.
 * dctn_position_mean_bwd : dy[b, p, l] = dlogits[b, l] / P, divided in float64 and rounded once; dy (B, P, L) is
 *   OVERWRITTEN.  The same limits and codes.
 *
 * dctn_tensor_stats : the moments of up to 8 tensors in ONE launch.  tensors / counts: HOST arrays of n_tensors device
 *   pointers (contiguous values of `dtype`, aligned to their element size; a 16-byte aligned pointer is read four elements
 *   per access - the record does not depend on which form ran) and element counts.  1 <= n_tensors <= 8 and every count
 *   >= 1: DCTN_ERR_BAD_SHAPE otherwise.  records: device, 8-byte aligned, n_tensors records of
 *   dctn_tensor_stats_record_bytes() = 64 bytes, laid out as
 *        0  int64    n          all elements
 *        8  double   sum        } over the FINITE elements only, in float64 (a float32 value and its square are exact
 *       16  double   sum_sq     } in a double)
 *       24  double   sum_abs    }
 *       32  float    min_abs    +Inf if the tensor has no finite element
 *       36  float    max_abs    0 if it has none
 *       40  uint32   nonfinite  NaN and +-Inf elements
 *       44  uint32   seq        advanced by one by every launch
 *       48  uint32   ticket     0 between launches
 *       52  uint32   reserved[3]
 *   The records must be ZERO before the first launch and are the caller's to read after any launch; every launch
 *   overwrites all fields but `reserved`.  workspace: device, 8-byte aligned, dctn_tensor_stats_workspace_bytes(n_tensors)
 *   bytes (too small: DCTN_ERR_WORKSPACE); it need not be initialised and nothing of it is kept between launches.
 *   Tensor i is read by min(256, ceil(count / 4096)) workgroups of 1024 threads; each stores its partial sums into its
 *   own slots of the workspace and draws the tensor's ticket; the workgroup that draws the last one adds the slots in
 *   index order, writes the record and puts the ticket back to 0.  No workgroup waits for another, and the record's bits
 *   are a function of the tensor's values alone.  Capturable: the launch reads no host state but its arguments.
 * ------------------------------------------------------------------------------------------ */
int dctn_position_mean_fwd(const void* y, void* out, int64_t B, int64_t P, int L, int dtype, void* stream);
int dctn_position_mean_bwd(const void* dlogits, void* dy, int64_t B, int64_t P, int L, int dtype, void* stream);
size_t dctn_tensor_stats_record_bytes(void);
size_t dctn_tensor_stats_workspace_bytes(int n_tensors);
int dctn_tensor_stats(const void* const* tensors, const int64_t* counts, int n_tensors, void* records, void* workspace,
                      size_t workspace_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Histograms of up to 8 tensors in ONE launch over a table of bin edges (version 519; dctn_amd/csrc/tensor_hist.hip;
 * host side: dctn_amd/tensor_hist.py) - the reference's log_dumb_histogram (mnist.py:537-553) over TensorBoard's bucket
 * set, or any other table.  Dtypes: DCTN_F32 / DCTN_F64, one per call.  None of the three reports to dctn_last_kernel.
 *
 * dctn_tensor_hist : tensors / counts: HOST arrays of n_tensors device pointers (contiguous values of `dtype`, aligned
 *   to their element size; a 16-byte aligned pointer is read four elements per access - the block does not depend on
 *   which form ran) and element counts.  edges: DEVICE, 8-byte aligned, n_edges float64 values, STRICTLY INCREASING and
 *   finite (the caller's duty: the library cannot read them).  blocks: DEVICE, 8-byte aligned, n_tensors blocks of
 *   dctn_tensor_hist_block_bytes(n_edges) = 80 + 8 (n_edges - 1) bytes each, one after the other, laid out as
 *        0  uint64   total      every element seen
 *        8  uint64   below      finite and < edges[0]
 *       16  uint64   above      finite and > edges[n_edges - 1]
 *       24  uint64   nan
 *       32  uint64   pos_inf
 *       40  uint64   neg_inf
 *       48  uint64   max_key    key(largest finite value); 0: no finite value yet
 *       56  uint64   min_key_c  ~key(smallest finite value); 0: no finite value yet
 *       64  uint32   calls      launches so far, recorded or not
 *       68  uint32   recorded   launches that counted
 *       72  uint32   ticket     0 between launches
 *       76  uint32   reserved
 *       80  uint64   counts[n_edges - 1]
 *   key(v), for the float64 bits b of v: ~b if the sign bit is set, b | 2^63 otherwise - unsigned order is value order,
 *   and no finite value has key 0 or ~0.  A block must be ZERO before its first launch: all zero is a valid empty block.
 *   Semantics, those of numpy.histogram(v.astype(float64), bins=edges): a finite v counts in bin i when
 *   edges[i] <= v < edges[i + 1]; the last bin is closed on the right; a float32 value is widened exactly and compared
 *   in float64; -0.0 is 0.0 (in min / max too).  The bin is found by a binary search of comparisons against the table.
 *   A launch ADDS to what the block holds, if it is recorded: it is iff calls % period == 0 for the `calls` it finds; a
 *   launch that is not reads no element.  Either way it leaves calls + 1 and ticket 0.  Everything accumulated is an
 *   integer sum or a max: the block's bits are a function of the values of the recorded launches alone.  Tensor i is
 *   read by min(256, ceil(count / 4096)) workgroups of 1024 threads; no workgroup waits for another.  Capturable: the
 *   launch reads no host state but its arguments; the blocks it reads and writes are device state, so a replay goes on
 *   where the last launch stopped.  The tensors and the table are only read; nothing outside the blocks is written; no
 *   workspace.
 *   Return codes, decided on the host before any launch, in the project's order: DCTN_ERR_NULL (an array, an entry,
 *   edges, blocks); DCTN_ERR_BAD_SHAPE (n_tensors outside 1..8, a count < 1, n_edges outside 2..2048, period < 1);
 *   DCTN_ERR_BAD_DTYPE (bf16 or anything else); DCTN_ERR_UNSUPPORTED (a count above 2^39; edges or blocks not 8-byte
 *   aligned).
 * dctn_tensor_hist_reset : zeroes counts, counters, keys and `recorded` of n_tensors blocks and KEEPS `calls`, so the
 *   period's phase survives a read.  One small launch on `stream`, between launches of dctn_tensor_hist; not meant to be
 *   captured.  DCTN_ERR_NULL; DCTN_ERR_BAD_SHAPE (n_tensors < 1, n_edges outside 2..2048); DCTN_ERR_UNSUPPORTED
 *   (n_tensors > 65535, alignment).
 * ------------------------------------------------------------------------------------------ */
size_t dctn_tensor_hist_block_bytes(int n_edges);   /* 0 for n_edges < 2 */
int dctn_tensor_hist(const void* const* tensors, const int64_t* counts, int n_tensors, const void* edges, int n_edges,
                     void* blocks, int period, int dtype, void* stream);
int dctn_tensor_hist_reset(void* blocks, int n_tensors, int n_edges, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sum and squared Frobenius norm of the tensor each of up to 16 ConvSBS strings REPRESENTS, in ONE launch, from the
 * cores alone (version 520; dctn_amd/csrc/tt_stats.hip; host side: dctn_amd/tt_stats.py) - what the reference logs per
 * string every 20 iterations as mean_of_tt_tensor / std_of_tt_tensor (dctn/conv_sbs_statistics_logging.py, from
 * ConvSBS.mean() and ConvSBS.var() ** 0.5).  Dtypes: DCTN_F32 / DCTN_F64, one per call; all arithmetic is float64 (a
 * float32 element is widened exactly).  None of the three reports to dctn_last_kernel.
 *
 * dctn_tt_string_t : one string.  Core c is (out_sizes[c], l_c, r_c, q, ..., q) contiguous, q repeated C times, with
 *   l_c = bond_sizes[c] and r_c = bond_sizes[(c + 1) % n_cores]: the bonds are taken cyclically, so bond_sizes[0] == 1 is an
 *   open chain and anything larger a ring.  P = q^C; the slices A_c[o, p] are l_c x r_c.  `reserved` is ignored.
 * dctn_tt_stats : cores: HOST array of the strings' device pointers, string-major (the n_cores of string 0, then those
 *   of string 1, ...), each aligned to its element size.  strings: HOST array of n_strings descriptors.  Per string
 *        sum     = tr(S_0 S_1 ... S_{N-1}),                              S_c    = sum_{o,p} A_c[o, p]
 *        sq_norm = sum_{i,j < l_0} (F_{N-1} o ... o F_0)(e_i e_j^T)[i, j],   F_c(V) = sum_{o,p} A_c[o, p]^T V A_c[o, p]
 *   the sum of all elements of the represented tensor and its squared Frobenius norm.  Limits: 1 <= n_cores <= 16,
 *   every bond <= 32 (non-uniform bonds included), P <= 256, any out size >= 1 as long as a core has fewer than 2^31
 *   elements.  block: DEVICE, 8-byte aligned, dctn_tt_stats_block_bytes(n_strings, capacity) =
 *   32 + capacity (16 + 16 n_strings) bytes, laid out as
 *        0  uint32   calls        launches so far, recorded or not
 *        4  uint32   recorded     launches that wrote a row
 *        8  uint32   ticket       0 between launches
 *       12  uint32   reserved[5]
 *       32  rows[capacity], each
 *             0  uint32   call      the `calls` value the row was taken at
 *             4  uint32   seq       the `recorded` value it got, written last
 *             8  uint64   reserved
 *            16  { double sum, double sq_norm } [n_strings]
 *   The block must be ZERO before the first launch.  A launch is RECORDED iff calls % period == 0 for the `calls` it
 *   finds; a recorded launch writes row recorded % capacity (a ring: the oldest row is overwritten); a launch that is not
 *   recorded reads no core and writes nothing but the header.  Either way it leaves calls + 1 and ticket 0.
 *   workspace: DEVICE, 8-byte aligned, dctn_tt_stats_workspace_bytes(strings, n_strings) bytes = 16 per workgroup; it need
 *   not be initialised and nothing of it is kept between launches.  A string owns bond_sizes[0] workgroups of 256
 *   threads (an open chain: one); each stores its two partial values into its own slot and draws the ticket; the
 *   workgroup that draws the launch's last one adds every string's slots in index order, writes the row and advances the
 *   header.  No workgroup waits for another.  Grid and every summation order are functions of the string's own shape: a
 *   string's 16 bytes do not depend on how many strings the launch holds, on its place among them, on the device or on
 *   what the workspace held.  Capturable: the launch reads no host state but its arguments (the descriptors and pointers
 *   travel in the kernel's argument); the block is device state, so a replay goes on where the last launch stopped.  The
 *   cores are only read; nothing outside the block and the workspace is written.
 *   Return codes, decided on the host before any launch, in the project's order: DCTN_ERR_NULL (cores, strings, block, or
 *   an entry of cores); DCTN_ERR_BAD_SHAPE (n_strings outside 1..16; n_cores, C, q, an out size or a bond < 1;
 *   n_cores > 16; capacity < 1; period < 1); DCTN_ERR_BAD_DTYPE (bf16 or anything else); DCTN_ERR_UNSUPPORTED (a bond
 *   above 32, P above 256, a core of 2^31 elements or more; a misaligned core, block or workspace); DCTN_ERR_WORKSPACE
 *   (workspace NULL or too small).
 * dctn_tt_stats_block_bytes : 0 for n_strings outside 1..16 or capacity < 1.
 * dctn_tt_stats_workspace_bytes : 0 for NULL, n_strings outside 1..16 or a string dctn_tt_stats would refuse.
 * ------------------------------------------------------------------------------------------ */
typedef struct dctn_tt_string_t {
  int n_cores, C, q, reserved;
  int out_sizes[16];
  int bond_sizes[16];
} dctn_tt_string_t;
size_t dctn_tt_stats_block_bytes(int n_strings, int capacity);
size_t dctn_tt_stats_workspace_bytes(const dctn_tt_string_t* strings, int n_strings);
int dctn_tt_stats(const void* const* cores, const dctn_tt_string_t* strings, int n_strings, void* block, int capacity, int period,
                  void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sum, sum of squares, largest magnitude and non-finite count of every parameter and of its gradient, for up to 64
 * parameters in ONE launch over the two flat buffers of a flat optimizer (version 521; dctn_amd/csrc/param_stats.hip;
 * host side: dctn_amd/param_stats.py) - what the reference logs per parameter and iteration through
 * add_weights_and_grads_logging (mnist.py:535: a norm of each parameter and of its gradient) and log_parameters_stats
 * (dctn/training.py:247: mean and std).  Dtypes: DCTN_F32 / DCTN_F64 / DCTN_BF16, one per call; all arithmetic is float64
 * (a bfloat16 or float32 element and its square are exact there).  None of the three reports to dctn_last_kernel.
 *
 * dctn_param_stats : params: DEVICE, n values of `dtype`.  master_or_null: DEVICE, n float32 values (DCTN_BF16 only);
 *   when given, the WEIGHT statistics are taken from it and params is not read.  grads: DEVICE, n values of `dtype`.
 *   ends: HOST array of n_segments exclusive segment ends, strictly increasing, ends[n_segments - 1] = n: segment s is the
 *   elements ends[s - 1] .. ends[s] - 1 of every buffer (ends[-1] = 0).  1 <= n_segments <= 64, a segment has fewer than
 *   2^31 elements.  block: DEVICE, 8-byte aligned, dctn_param_stats_block_bytes(n_segments, capacity) =
 *   32 + capacity (16 + 64 n_segments) bytes, laid out as
 *        0  uint32   calls        launches so far, recorded or not
 *        4  uint32   recorded     launches that wrote a row
 *        8  uint32   ticket       0 between launches
 *       12  uint32   reserved[5]
 *       32  rows[capacity], each
 *             0  uint32   call      the `calls` value the row was taken at
 *             4  uint32   seq       the `recorded` value it got, written last
 *             8  uint64   reserved
 *            16  { double w_sum, w_sum_sq, w_max_abs; uint64 w_nonfinite;
 *                  double g_sum, g_sum_sq, g_max_abs; uint64 g_nonfinite } [n_segments]
 *   sum and sum_sq run over the FINITE elements only; max_abs is their largest magnitude, 0 when the segment has no
 *   finite element (-0.0 counts as 0); nonfinite counts NaN and +-Inf.
 *   The block must be ZERO before the first launch.  A launch is RECORDED iff calls % period == 0 for the `calls` it
 *   finds; a recorded launch writes row recorded % capacity (a ring: the oldest row is overwritten); a launch that is not
 *   recorded reads no element and writes nothing but the header.  Either way it leaves calls + 1 and ticket 0.
 *   workspace: DEVICE, 8-byte aligned, dctn_param_stats_workspace_bytes(ends, n_segments) bytes = 64 per workgroup; it
 *   need not be initialised and nothing of it is kept between launches.
 *   The plan: a segment of c elements owns min(64, ceil(c / 8192)) workgroups of 256 threads.  The segment is cut into
 *   groups of four consecutive elements counted from the SEGMENT's first element; thread j of the segment's 256 W threads
 *   (workgroup-major) owns the groups j, j + 256 W, ... and adds their elements in index order.  A whole group is loaded in
 *   one access per buffer when its address allows (16 bytes of float32, 8 of bfloat16, two 16-byte accesses of float64)
 *   and element by element otherwise.  A workgroup reads its part of both buffers in one pass, reduces in a fixed tree
 *   (lanes by shuffles at distances 32 .. 1, the four waves through LDS in index order), stores its eight partial values
 *   into its own 64-byte slot and draws the ticket; the workgroup that draws the launch's last one adds every segment's
 *   slots in index order, writes the row and advances the header.  No workgroup waits for another.
 *   A segment's 64 bytes are a function of its own values alone: they do not depend on its offset in the flat buffer (and
 *   so the alignment of its first element, or whether a group was loaded in one access), on the other segments of the
 *   launch or its place among them, on the device's CU count or on what the workspace held.  Capturable: the launch reads
 *   no host state but its arguments (the ends travel in the kernel's argument); the block is device state, so a replay
 *   goes on where the last launch stopped.  The three buffers are only read; nothing outside the block and the workspace
 *   is written.
 *   Return codes, decided on the host before any launch, in the project's order: DCTN_ERR_NULL (params, grads, ends or
 *   block); DCTN_ERR_BAD_SHAPE (n_segments < 1; ends not strictly increasing or the first < 1; capacity < 1; period < 1);
 *   DCTN_ERR_BAD_DTYPE (anything but the three); DCTN_ERR_UNSUPPORTED (n_segments > 64; a segment of 2^31 elements or
 *   more; params, grads or the master copy not aligned to its element size; block or workspace not 8-byte aligned; a
 *   master copy with a dtype other than DCTN_BF16); DCTN_ERR_WORKSPACE (workspace NULL or too small).
 * dctn_param_stats_block_bytes : 0 for n_segments outside 1..64 or capacity < 1.
 * dctn_param_stats_workspace_bytes : 0 for NULL, n_segments outside 1..64 or ends dctn_param_stats would refuse.
 * ------------------------------------------------------------------------------------------ */
size_t dctn_param_stats_block_bytes(int n_segments, int capacity);
size_t dctn_param_stats_workspace_bytes(const int64_t* ends, int n_segments);
int dctn_param_stats(const void* params, const void* master_or_null, const void* grads, const int64_t* ends, int n_segments,
                     void* block, int capacity, int period, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The batch monitor (version 522; dctn_amd/csrc/batch_monitor.hip; host side: dctn_amd/batch_monitor.py): what the
 * reference's hooks read off the BATCH, in ONE launch - the input statistics (mnist.py:298-311, :571-591: mean and std of
 * the quantum batch, std_of_coordinates_of_windows of its K x K windows as rank-one tensors), the whole model's output
 * (mnist.py:555-569: signed min, max, mean, std of the logits, the histogram of softmax(logits, dim=1)) and the per-sample
 * confidence (new_runner.py:512-531: the probability each sample gives its true class, beside the sample indices).  All
 * arithmetic is float64.  None of the three reports to dctn_last_kernel.
 *
 * dctn_batch_monitor_t: on the HOST, read during the call only.  Every pointer in it is a DEVICE pointer; the five inputs
 * are only read:
 *   x        contiguous (C, B, H, W, Q) values of x_dtype
 *   logits   contiguous (B, L) values of logits_dtype (chosen independently of x_dtype)
 *   y        B int64 labels
 *   indices  B int64 sample numbers, or NULL
 *   edges    n_edges float64 values, strictly increasing (the caller's duty, as for dctn_tensor_hist), 2 <= n_edges <= 2048
 *   block    8-byte aligned, dctn_batch_monitor_block_bytes(B, n_edges, capacity) bytes; all-zero is a valid empty block
 *   workspace, workspace_bytes   8-byte aligned, EXACTLY dctn_batch_monitor_workspace_bytes(B) = 40 B bytes; it may hold
 *            anything before the launch and nothing of it is kept
 *   K        the window size; 0 turns the window sums off.  period >= 1, capacity >= 1, 1 <= L <= 1024, B >= 1,
 *            B * L < 2^32, B <= 2^31 - 2.  DCTN_F32 / DCTN_F64 / DCTN_BF16 for either dtype.
 * The block, with R = 112 + 8 ceil((n_edges - 1) / 2) + 24 B the bytes of a row:
 *        0  uint32   calls        launches so far, recorded or not
 *        4  uint32   recorded     launches that wrote a row
 *        8  uint32   ticket       0 between launches
 *       12  uint32   reserved[5]
 *       32  rows[capacity], R bytes each
 *             0  uint32   call          the `calls` value the row was taken at
 *             4  uint32   seq           the `recorded` value it got, written last
 *             8  uint32   rows          samples with 0 <= y < L
 *            12  uint32   correct       those of `rows` whose prediction equals y
 *            16  uint32   bad_rows      samples whose logits hold a non-finite value
 *            20  uint32   z_nonfinite   non-finite logits
 *            24  uint64   x_nonfinite   non-finite elements of x
 *            32  double   x_sum, x_sum_sq          over the FINITE elements of x
 *            48  double   win_sum, win_sq          win_sum = sum over b and the (H-K+1)(W-K+1) windows of the product over
 *                                                  (dh, dw, c) of sum_q x[c, b, h+dh, w+dw, q]; win_sq the same with x^2.
 *                                                  Non-finite values are NOT filtered out of these two: one NaN or Inf in a
 *                                                  sample makes them non-finite.  Both 0 when K == 0.
 *            64  double   z_sum, z_sum_sq, z_min, z_max   over the FINITE logits; +inf / -inf when there is none
 *            96  uint32   below, above, nan, reserved     probabilities outside the table; nan: L for every bad row
 *           112  uint32   counts[n_edges - 1]             then 4 zero bytes when n_edges - 1 is odd
 *                int64    label[B]      y as given
 *                int64    index[B]      indices as given, -1 where indices is NULL
 *                float    p_true[B]     NaN when y is outside [0, L) or the row is bad
 *                int32    pred[B]       the argmax, the lowest index among equal maxima; -1 for a bad row
 *   The softmax, for a row without a non-finite logit, in float64: m = max_j z_j, e_j = exp(z_j - m), S = sum_j e_j in
 *   increasing j, p_j = e_j / S.  Every p_j is binned as numpy.histogram bins it (bin i: edges[i] <= p < edges[i + 1], the
 *   last bin closed on the right); p_true is p_y rounded to float32.  A bad row adds L to `nan` and nothing to `counts`.
 *   A launch is RECORDED iff calls % period == 0 for the `calls` it finds; a recorded launch writes row recorded % capacity
 *   completely (a ring) with seq = recorded and call = calls, then leaves recorded + 1; a launch that is not recorded reads
 *   no element and writes nothing but the header.  Either way it leaves calls + 1 and ticket 0.
 *   The plan: B + 1 workgroups of 256 threads, a function of B alone.  Workgroup b < B reads sample b of x once, stages its
 *   (sum_q x, sum_q x^2) pairs in LDS (K > 0), forms every window product from them, reduces in a fixed tree (lanes by
 *   shuffles at distances 32 .. 1, the four waves in index order) and stores five values into its 40-byte slot; workgroup B
 *   takes the logits, one thread per row, adds the rows' values in row order and writes its piece of the row directly; the
 *   workgroup that draws the launch's last ticket adds the slots in sample order.  No workgroup waits for another.  The
 *   same values leave the same row bytes (apart from call / seq) on every launch, device and CU count.  Capturable: the
 *   launch reads no host state but its arguments.  Nothing outside the block and the workspace is written.
 *   Return codes, decided on the host before any launch, in the project's order: DCTN_ERR_NULL (the struct, x, logits, y,
 *   edges, block or workspace); DCTN_ERR_BAD_SHAPE (B, C, H, W or Q < 1; K < 0, K > H or K > W; L outside 1..1024;
 *   n_edges outside 2..2048; period or capacity < 1); DCTN_ERR_BAD_DTYPE (either dtype not one of the three);
 *   DCTN_ERR_UNSUPPORTED (B * L >= 2^32 or B > 2^31 - 2; x or logits not aligned to its element, y, indices, edges, block
 *   or workspace not 8-byte aligned; workspace_bytes not exactly the size above; the LDS of a workgroup - 10 416 bytes plus
 *   the larger of 16 C H W (K > 0) and 4 (n_edges + 2) rounded up to 16 - above 15/16 of what dctn_device_limits reports).
 * dctn_batch_monitor_block_bytes : 32 + capacity R; 0 for B outside 1..2^31 - 2, n_edges outside 2..2048 or capacity < 1.
 * dctn_batch_monitor_workspace_bytes : 40 B; 0 for B outside 1..2^31 - 2.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void *x, *logits, *y, *indices, *edges;
  void *block, *workspace;
  size_t workspace_bytes;
  int64_t B;
  int C, H, W, Q, K, L, n_edges, period, capacity, x_dtype, logits_dtype, reserved;
} dctn_batch_monitor_t;
size_t dctn_batch_monitor_block_bytes(int64_t B, int n_edges, int capacity);
size_t dctn_batch_monitor_workspace_bytes(int64_t B);
int dctn_batch_monitor(const dctn_batch_monitor_t* monitor, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tensor-network inner product of two stacks of EPS cores - replaces the contractions of
 * dctn/epses_composition.py:21-58 `inner_product` (Gram of the first pair of cores over their input legs:
 * dctn/eps.py:106-112 `contract_on_input_dims`; that matrix absorbed into every input leg of the next core:
 * the N-operand einsum at :46-56; the closing dot product: dctn/eps.py:120-123), which the reference evaluates
 * every training iteration (dctn/eps_plus_linear.py:156-159).  Forward and backward are compositions of two
 * primitives over a contiguous tensor viewed as (pre, q, post):
 *   dctn_mode_product : out[pre, j, post] = sum_i in[pre, i, post] * M[i, j]      M: (q, q2) contiguous
 *   dctn_fiber_gram   : out[i, j] = sum_(pre, post) A[pre, i, post] * B[pre, j, post]     out: (qa, qb)
 * (Gram of two (rows, O) matrices: post = 1; dot product: qa = qb = 1.)  q, q2, qa, qb <= 32.  Outputs are
 * OVERWRITTEN, in the tensors' dtype (f32 / f64 / bf16 storage with f32 accumulation); sums are combined in a
 * fixed order (no atomics).  `out` must not alias `in`.
 * ------------------------------------------------------------------------------------------ */
int dctn_mode_product(const void* in, const void* M, void* out, int64_t pre, int q, int q2, int64_t post,
                      int dtype, void* stream);
size_t dctn_fiber_gram_workspace_bytes(int64_t pre, int qa, int qb, int64_t post, int dtype);
int dctn_fiber_gram(const void* A, const void* B, void* out, void* workspace, size_t workspace_bytes,
                    int64_t pre, int qa, int qb, int64_t post, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Latency-first gradient all-reduce over peer-mapped buffers (the reference has no
 * collective; the build's one collective is the mean of the parameter gradients, 58 KB .. 7.5 MB: latency-bound).
 * One-shot direct algorithm for the ranks of ONE node: every rank owns an uncached device block (flag lines + two
 * staging buffers), exported once as an IPC handle and mapped by every peer; per step ONE kernel per rank copies the
 * rank's values to its staging buffer, publishes its step number to every peer, waits (bounded, ~2 s) for theirs,
 * then sums every rank's staging buffer in rank order (float32 / float64 accumulation) and writes the (scaled)
 * result over `buf` in place: bitwise identical on all ranks.  Replayable from a HIP graph (the step counter lives
 * in device memory).  dctn_ar_create / _connect / _status / _destroy allocate, map or synchronise and are NOT
 * capturable; dctn_ar_allreduce only enqueues.  Host-side pairing: dctn_amd/ddp.py `DirectAllReducer`.
 *   create(world <= 16, rank, max_bytes)  -> opaque state;  export -> dctn_ar_handle_bytes() bytes for the peers;
 *   connect(handles of ALL ranks, rank-major);  allreduce(buf, n elements, dtype, average);
 *   status: 0 = every wait completed, r + 1 = a wait for rank r timed out (the results of that step are invalid).
 * Two-shot form for large buckets (version 402): rank r reduces chunk r only (reads (P - 1) N / P bytes), leaves it in
 * its result area and publishes a second flag; every rank copies the other chunks from their owners ((P - 1) N / P
 * more) instead of reading (P - 1) N bytes - bitwise the one-shot values.  dctn_ar_allreduce picks it for world >= 4
 * and >= 512 KiB; dctn_ar_allreduce_algo(..., algorithm: 0 = that rule, 1 = one-shot, 2 = two-shot) forces a form.
 * ------------------------------------------------------------------------------------------ */
size_t dctn_ar_handle_bytes(void);
int dctn_ar_create(int world, int rank, size_t max_bytes, void** state_out);
int dctn_ar_export(void* state, void* handle_out);
int dctn_ar_connect(void* state, const void* handles);
int dctn_ar_allreduce(void* state, void* buf, int64_t n, int dtype, int average, void* stream);
int dctn_ar_allreduce_algo(void* state, void* buf, int64_t n, int dtype, int average, int algorithm, void* stream);
int dctn_ar_status(void* state);
int dctn_ar_destroy(void* state);

#ifdef __cplusplus
}
#endif
#endif /* DCTN_AMD_H */
