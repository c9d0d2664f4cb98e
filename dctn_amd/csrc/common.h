// Shared helpers for the dctn_amd HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dctn_amd.h"

typedef __bf16 bf16_t;

template <typename S> struct AccOf { typedef float type; };
template <> struct AccOf<double> { typedef double type; };

#define DCTN_WAVE 64

// Store policy of the two buffers a register-family EPS step hands from one kernel to the next (eps_mfma.hip,
// eps_q2f32.hip): the `aux` operand of their 16-byte buffer stores.  0 = plain (the line stays dirty in the XCD's L2
// until the write-back at the end of the kernel), 16 = sc1, 17 = sc0 sc1 (written through, the line is dropped: the
// next kernel reads it from the memory side).  Build-time switches of the comparison in DESIGN 4.1.
//   DCTN_WT_FEATURES: the forward's feature buffer (blocked4 block store in bf16, the 16-byte row store in float32)
//   DCTN_WT_TILES:    the dCore kernels' partial tiles
#ifndef DCTN_WT_FEATURES
#define DCTN_WT_FEATURES 16
#endif
#ifndef DCTN_WT_TILES
#define DCTN_WT_TILES 0
#endif

// Build-time switches of the fused bf16 head forward's prologue and step loop (eps_fwd_head_q2reg_t_k, eps_mfma.hip), one
// per item of the comparison in DESIGN 4.1; none of them touches a floating-point operation.  1 = on, 0 = the form before; the defaults are what won its own A/B.
//   DCTN_FWD_ARGS_ONCE:    every kernel argument is read in the one scalar round at entry and kept in registers
//   DCTN_FWD_EARLY_WINDOW: the first group's step counter is set in front of the barrier that publishes the core (one
//                          workgroup barrier fewer), a wave's first window goes out behind the core's loads
//   DCTN_FWD_POS_TABLE:    a step reads its lane's offsets from a table in LDS that the workgroup fills once, and splits
//                          its ticket into (sample, position group) by a multiply-shift
#ifndef DCTN_FWD_ARGS_ONCE
#define DCTN_FWD_ARGS_ONCE 0   // built and measured: it does not beat its twin (NOTEBOOK round 13)
#endif
#ifndef DCTN_FWD_EARLY_WINDOW
#define DCTN_FWD_EARLY_WINDOW 1
#endif
#ifndef DCTN_FWD_POS_TABLE
#define DCTN_FWD_POS_TABLE 1
#endif

// The device's geometry, asked once per process (capi.hip); gfx950 defaults when the runtime cannot say
struct DctnDev { int cus; int lds; };   // CUs, LDS bytes per CU
const DctnDev& dctn_dev();
int dctn_lds_wg_max();   // LDS bytes one workgroup's plan may claim: 15/16 of a CU's (150 of 160 KiB on gfx950)
// workgroups resident at once: cus * clamp(lds / lds_bytes, lo, hi); lds_bytes == 0 -> cus * hi
long long dctn_resident_wgs(size_t lds_bytes, int lo, int hi);
// the dynamic-LDS opt-in of a kernel: false when `bytes` exceeds a CU's LDS or the runtime refuses
bool dctn_lds_optin(const void* fn, size_t bytes);

#define DCTN_CHECK_LAUNCH()                                   \
  do {                                                        \
    if (hipGetLastError() != hipSuccess) return DCTN_ERR_LAUNCH; \
  } while (0)

// name of the kernel family the last call dispatched to
void dctn_set_last_kernel(const char* name);

// Zero `bytes` bytes on the stream with a kernel.  Not hipMemsetAsync: recorded into a
// torch HIP graph, a memset node zero-filled on the first replay and wrote garbage on the later ones
// (tools/memset_capture_check.py, ROCm 7.2 + torch 2.10; the same node replays correctly from a plain HIP program,
// tools/probes/memset_graph.hip) - accumulators that start from zero must not depend on it.
int dctn_zero_async(void* ptr, size_t bytes, hipStream_t st);

static inline long long ipow_ll(long long b, int e) {
  long long r = 1;
  for (int i = 0; i < e; ++i) r *= b;
  return r;
}

static inline size_t dtype_size(int dtype) {
  return dtype == DCTN_F64 ? 8 : (dtype == DCTN_F32 ? 4 : 2);
}
// bytes of the type a dtype accumulates in: bf16 storage accumulates in float32
static inline size_t acc_size(int dtype) { return dtype == DCTN_F64 ? 8 : 4; }

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

template <typename T>
__device__ __forceinline__ T wave_reduce_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Philox4x32-10 (include/dctn_amd.h states it): the generator of the dropout masks (core_dropout.hip) and of the round
// keys of the batch order (batch_source.hip)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// -------------------------------------------------------------------------------- EPS shapes
struct EpsP {
  int C, B, H, W, Q, K, O, N, Ho, Wo;
  long long Wn;    // B*Ho*Wo windows
  long long R;     // Q^N core rows
  long long s[5];  // element strides of x
  int m, LO, NH;   // low split: last m factors, LO = Q^m, NH = N-m high factors
  long long HI;    // Q^NH
  int bits;        // bits per packed digit in the dCore kernel
  int opts;        // DCTN_OPT_* flags of the call's policy argument (0 from the workspace queries' defaults)
};

int eps_fill_params(EpsP& p, const int64_t x_strides[5], int C, int B, int H, int W, int Q, int K,
                    int O, int policy = 0);

// generic (any shape, f32/f64/bf16-storage) kernels — eps_generic.hip
int eps_fwd_generic(const void* x, const void* core, void* out, void* ws, size_t ws_bytes, EpsP p, int dtype,
                    hipStream_t st);
size_t eps_bwd_generic_workspace(const EpsP& p, int dtype, int need_dx, int need_dcore);
int eps_bwd_generic(const void* x, const void* core, const void* dY, void* dX, void* dCore,
                    void* ws, size_t ws_bytes, EpsP p, int dtype, hipStream_t st);

int eps_gather_dx_launch(const void* gxw, void* dX, const EpsP& p, int dtype, hipStream_t st);

// MFMA family "bigcore" (exact f32, LDS-streamed core) — eps_bigcore.hip
size_t eps_fwd_bigcore_workspace(const EpsP& p, int dtype, int precision);
// zsave (optional): room of eps_bigcore_saved_bytes() for the forward GEMM result Z, which eps_bwd_dx_bigcore then
// reads instead of running its third GEMM (0 bytes: the shape keeps nothing)
size_t eps_bigcore_saved_bytes(const EpsP& p, int dtype, int precision);
int eps_fwd_bigcore(const void* x, const void* core, void* out, void* ws, size_t ws_bytes,
                    const EpsP& p, int dtype, int precision, hipStream_t st, void* zsave = nullptr);
size_t eps_bwd_dcore_bigcore_workspace(const EpsP& p, int dtype, int precision);
int eps_bwd_dcore_bigcore(const void* x, const void* dY, void* dCore, const EpsP& p, int dtype,
                          int precision, hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0);
size_t eps_bwd_dfactor_bigcore_workspace(const EpsP& p, int dtype, int precision);
int eps_bwd_dx_bigcore(const void* x, const void* core, const void* dY, void* dX, void* ws,
                       size_t ws_bytes, const EpsP& p, int dtype, int precision, hipStream_t st,
                       const void* zsaved = nullptr, size_t zsaved_bytes = 0);

// bf16x3 large-core family (DCTN_PREC_SPLIT float32: the bigcore kernels on three bf16 products) — eps_bigcore_bf16x3.hip
bool eps_bf16x3_covers(const EpsP& p, int dtype, int precision);
size_t eps_fwd_bf16x3_workspace(const EpsP& p, int dtype, int precision);
size_t eps_bf16x3_saved_bytes(const EpsP& p, int dtype, int precision);
int eps_fwd_bf16x3(const void* x, const void* core, void* out, void* ws, size_t ws_bytes, const EpsP& p, int dtype,
                   int precision, hipStream_t st, void* zsave = nullptr);
size_t eps_bwd_dfactor_bf16x3_workspace(const EpsP& p, int dtype, int precision);
int eps_bwd_dx_bf16x3(const void* x, const void* core, const void* dY, void* dX, void* ws, size_t ws_bytes, const EpsP& p,
                      int dtype, int precision, hipStream_t st, const void* zsaved = nullptr, size_t zsaved_bytes = 0);
size_t eps_bwd_dcore_bf16x3_workspace(const EpsP& p, int dtype, int precision);
int eps_bwd_dcore_bf16x3(const void* x, const void* dY, void* dCore, const EpsP& p, int dtype, int precision,
                         hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0);

// register-resident exact-float32 family for Q = 2, N in {8, 9}, O <= 4 (cfg2 in the reference's own dtype) — eps_q2f32.hip
bool eps_q2f32_covers(const EpsP& p, int dtype, int precision);
int eps_fwd_q2f32(const void* x, const void* core, void* out, const EpsP& p, int dtype, int precision, hipStream_t st);
size_t eps_bwd_q2f32_workspace(const EpsP& p, int dtype, int precision);
int eps_bwd_q2f32(const void* x, const void* dY, void* dCore, void* ws, size_t ws_bytes, const EpsP& p, int dtype,
                  int precision, hipStream_t st);
int eps_head_fwd_q2f32(const void* x, const void* core, const void* head_w, const void* bias, void* feat, void* logits,
                       const EpsP& p, int Cout, int dtype, int precision, hipStream_t st);
size_t eps_head_bwd_q2f32_workspace(const EpsP& p, int Cout, int dtype, int precision);
int eps_head_bwd_q2f32(const void* x, const void* feat, const void* dLogits, const void* head_w, void* dCore, void* dW,
                       void* dBias, void* ws, size_t ws_bytes, const EpsP& p, int Cout, int dtype, int precision,
                       hipStream_t st);

// which family the forward of a shape dispatches to (dctn_eps_family)
bool eps_mfma_covers(const EpsP& p, int dtype, int precision);
bool eps_bigcore_covers(const EpsP& p, int dtype, int precision);

// two-halves GEMM path on the 16x16x4 matrix instructions — eps_halves.hip: float64 (v_mfma_f64_16x16x4_f64),
// and float32 (v_mfma_f32_16x16x4_f32) for shapes the other float32 families leave (odd Q, ...)
bool eps_halves_wanted(const EpsP& p, int dtype);
size_t eps_fwd_halves_workspace(const EpsP& p, int dtype);
// saved (optional): room of eps_halves_saved_bytes() for the forward's halves and GEMM result, which eps_bwd_halves
// then reads instead of rebuilding them
size_t eps_halves_saved_bytes(const EpsP& p, int dtype);
int eps_fwd_halves(const void* x, const void* core, void* out, void* ws, size_t ws_bytes, const EpsP& p, int dtype,
                   hipStream_t st, void* saved = nullptr);
size_t eps_bwd_halves_workspace(const EpsP& p, int dtype, int need_dx, int need_dcore);
int eps_bwd_halves(const void* x, const void* core, const void* dY, void* dX, void* dCore, void* ws, size_t ws_bytes,
                   const EpsP& p, int dtype, hipStream_t st, const void* saved = nullptr, size_t saved_bytes = 0);

// MFMA kernels for power-of-two Q — eps_mfma.hip.  Return DCTN_ERR_UNSUPPORTED when the shape
// is outside the family so that the dispatcher can take the generic kernels.
// stats (optional): float64 {sum y, sum y^2}, accumulated; out may then be NULL (nothing stored)
int eps_fwd_mfma(const void* x, const void* core, void* out, const EpsP& p, int dtype,
                 int precision, hipStream_t st, double* stats = nullptr);
// {sum y, sum y^2} of n stored values, accumulated into float64 stats[2] — window_stats.hip
int eps_out_stats(const void* y, long long n, int dtype, double* stats, hipStream_t st);
size_t eps_bwd_mfma_workspace(const EpsP& p, int dtype, int precision, int need_dx, int need_dcore);
int eps_bwd_mfma(const void* x, const void* core, const void* dY, void* dX, void* dCore, void* ws,
                 size_t ws_bytes, const EpsP& p, int dtype, int precision, hipStream_t st);
int eps_head_fwd_mfma(const void* x, const void* core, const void* head_w, const void* bias, void* feat, void* logits,
                      const EpsP& p, int Cout, int dtype, int precision, hipStream_t st);
size_t eps_head_bwd_mfma_workspace(const EpsP& p, int Cout, int dtype, int precision);
int eps_head_bwd_mfma(const void* x, const void* feat, const void* dLogits, const void* head_w, void* dCore,
                      void* dW, void* dBias, void* ws, size_t ws_bytes, const EpsP& p, int Cout, int dtype,
                      int precision, hipStream_t st);

// -------------------------------------------------------------------------------- ConvSBS strings
// One string as the C-ABI describes it: n cores with their output sizes, left bonds (bond_sizes[0] closes a ring) and
// window positions, over an input of C channels, (B, H, W) pixels and q values per pixel.  The entry points build it once;
// every family plans from it.  For the several-strings entry points the arrays hold the strings one after the other.
struct SbsShape {
  int n;
  const int *out_sizes, *bond_sizes, *pos_h, *pos_w;
  int C, B, H, W, q, dtype;
};
// string i of a several-strings shape
static inline SbsShape sbs_string(SbsShape many, int i) {
  many.out_sizes += i * many.n;
  many.bond_sizes += i * many.n;
  many.pos_h += i * many.n;
  many.pos_w += i * many.n;
  return many;
}

// Generic sweep (any string, f32 / f64 / bf16 storage) — convsbs_generic.hip
// the shape checks every entry point makes before it asks a family (cores optional: every pointer non-NULL)
int convsbs_check_shape(const SbsShape& sh, const void* const* cores);
int convsbs_fwd_generic(const void* x, const int64_t xs[5], const void* const* cores, void* out, const SbsShape& sh, hipStream_t st);
// The backward in two calls.  The plan checks the workspace, plans the LDS and opts the kernel in (DCTN_ERR_UNSUPPORTED:
// nothing written, the wide family takes the string), carves the workspace and zero-fills the accumulators; the run is the
// sweep, the dX gather and the bf16 conversion.  Between the two the entry point tries the matrix-core backward.
// states [element][window] | gxw: per-window d/d(pixel features) [n C q][windows] | acc: bf16 storage's float32 accumulators |
// partials: the matrix-core backward's records (NULL: the tail is too short for partial_bytes)
struct SbsBwdPlan { void *states, *gxw; unsigned char* acc; float* partials; size_t partial_bytes; };
size_t convsbs_bwd_generic_workspace(const SbsShape& sh, bool* lds_fits = nullptr);   // lds_fits: the plan's LDS answer with core gradients
int convsbs_bwd_generic_plan(SbsBwdPlan& pl, const SbsShape& sh, void* const* dCores, void* ws, size_t ws_bytes, hipStream_t st);
int convsbs_bwd_generic_run(const SbsBwdPlan& pl, const void* x, const int64_t xs[5], const void* const* cores,
                            const void* dY, void* dX, void* const* dCores, const SbsShape& sh, hipStream_t st);
// dX from per-window gradients in the gxw layout: every family that writes them gathers here
int convsbs_gather_dx(const SbsShape& sh, const void* gxw, void* dX, hipStream_t st);

// MFMA ConvSBS sweep (open chain, uniform bond) — convsbs_mfma.hip
// its share of the generic backward's workspace: state elements per window (0: bonds outside the family), bytes of its records
long long convsbs_mfma_state_elems(const SbsShape& sh);
size_t convsbs_mfma_partial_bytes(const SbsShape& sh);
// save_states (optional): room of convsbs_saved_states_bytes(...) for the forward states a following backward takes over
size_t convsbs_saved_states_bytes(const SbsShape& sh);
int convsbs_fwd_mfma(const void* x, const int64_t xs[5], const void* const* cores, void* out, const SbsShape& sh,
                     hipStream_t st, float* save_states = nullptr);
int convsbs_bwd_mfma(const void* x, const int64_t xs[5], const void* const* cores, const void* dY, float* states, float* gxw,
                     float* const* dcores, const SbsShape& sh, hipStream_t st, float* partials = nullptr,
                     size_t partial_bytes = 0, const float* saved_states = nullptr);
// Band-owning backward for bonds 5..16 (two roles per SIMD, nothing kept by the forward) - convsbs_band.hip.  Strings it
// covers keep no forward states (convsbs_saved_states_bytes returns 0 for them); `ws` holds the per-workgroup dCore
// records and the partial sums of the pixel rows two bands share (convsbs_band_bwd_workspace; 0 = outside the family).
bool convsbs_band_covers(const SbsShape& sh);
size_t convsbs_band_bwd_workspace(const SbsShape& sh);
int convsbs_fwd_band(const void* x, const int64_t xs[5], const void* const* cores, void* out, const SbsShape& sh,
                     hipStream_t st);
int convsbs_bwd_band(const void* x, const int64_t xs[5], const void* const* cores, const void* dY, void* dX,
                     float* const* dcores, const SbsShape& sh, hipStream_t st, void* ws, size_t ws_bytes);
// Wide backward for strings whose core gradients do not fit one workgroup's LDS (any bond, f32 / f64 / bf16 storage) -
// convsbs_wide.hip.  GEMMs over HBM buffers of window chunks, fixed-order partial records, no atomics.  The per-window input
// gradients land at the START of `ws` in the generic sweep's gxw layout ([n C q][windows]; dX, when wanted, is gathered
// from them by convsbs_gather_dx).  convsbs_wide_bwd_workspace: 0 = outside the family.
size_t convsbs_wide_bwd_workspace(const SbsShape& sh);
int convsbs_bwd_wide(const void* x, const int64_t xs[5], const void* const* cores, const void* dY, void* dX,
                     void* const* dcores, const SbsShape& sh, hipStream_t st, void* ws, size_t ws_bytes);

// Register-resident sweep for small bonds (every bond <= 4, float32 open chains, at most one two-valued core,
// q^C <= 4) - convsbs_reg.hip.  The backward writes dX itself (no per-window gradients, no gather launch) and needs
// `ws` only for its per-workgroup dCore records (convsbs_reg_bwd_workspace; 0 = the string is outside the family).
size_t convsbs_reg_bwd_workspace(const SbsShape& sh);
int convsbs_fwd_reg(const void* x, const int64_t xs[5], const void* const* cores, void* out, const SbsShape& sh,
                    hipStream_t st);
int convsbs_bwd_reg(const void* x, const int64_t xs[5], const void* const* cores, const void* dY, void* dX,
                    float* const* dcores, const SbsShape& sh, hipStream_t st, void* ws, size_t ws_bytes);
// several uniform strings of one layer in one launch each way (DCTN_ERR_UNSUPPORTED: run them one by one)
// The same for strings of the band family (bonds 5..16): blockIdx.y = string, one tail kernel for all strings.
size_t convsbs_many_band_bwd_workspace(int ns, const SbsShape& sh);
int convsbs_many_fwd_band(const void* x, const int64_t xs[5], const void* const* cores, void* const* outs, int ns,
                          const SbsShape& sh, hipStream_t st);
int convsbs_many_bwd_band(const void* x, const int64_t xs[5], const void* const* cores, const void* const* dYs, void* dX,
                          float* const* dcores, int ns, const SbsShape& sh, hipStream_t st, void* ws, size_t ws_bytes);
size_t convsbs_many_reg_bwd_workspace(int ns, const SbsShape& sh);
int convsbs_many_fwd_reg(const void* x, const int64_t xs[5], const void* const* cores, void* const* outs, int ns,
                         const SbsShape& sh, hipStream_t st);
int convsbs_many_bwd_reg(const void* x, const int64_t xs[5], const void* const* cores, const void* const* dYs, void* dX,
                         float* const* dcores, int ns, const SbsShape& sh, hipStream_t st, void* ws, size_t ws_bytes);
