// C-ABI entry points (include/dctn_amd.h): argument validation + dispatch to kernel families.
#include "common.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

// The library's process-wide state.  g_last_kernel, its only mutable global: a diagnostic pointer to a string literal
// naming the kernel family of the last successful call (relaxed atomic, last writer wins: autograd runs backward on its
// own thread, so a thread-local would hide the backward's kernels from the caller).  No entry point reads it to decide
// anything.  dctn_dev(): the device's CU count and LDS per CU, set once on first use, which every plan and launch reads.
static std::atomic<const char*> g_last_kernel{"none"};
void dctn_set_last_kernel(const char* name) { g_last_kernel.store(name, std::memory_order_relaxed); }

const DctnDev& dctn_dev() {
  static const DctnDev d = [] {
    DctnDev r{256, 160 * 1024};   // gfx950 (MI355X)
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess) {
      if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) r.cus = v;
      if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && v >= 64 * 1024) r.lds = v;
    }
    // test hook: DCTN_DEVICE_LIMITS="cus,lds_bytes" runs the plans of a smaller device (a partitioned card) on this one;
    // it only lowers the values, so no kernel asks for more than the card has
    int cus = 0, lds = 0;
    const char* lim = getenv("DCTN_DEVICE_LIMITS");
    if (lim && sscanf(lim, "%d,%d", &cus, &lds) == 2) {
      if (cus > 0 && cus < r.cus) r.cus = cus;
      if (lds > 0 && lds < r.lds) r.lds = lds;
    }
    return r;
  }();
  return d;
}

int dctn_lds_wg_max() { return dctn_dev().lds / 16 * 15; }

long long dctn_resident_wgs(size_t lds_bytes, int lo, int hi) {
  long long per_cu = lds_bytes ? (long long)dctn_dev().lds / (long long)lds_bytes : hi;
  if (per_cu < lo) per_cu = lo;
  if (per_cu > hi) per_cu = hi;
  return (long long)dctn_dev().cus * per_cu;
}

bool dctn_lds_optin(const void* fn, size_t bytes) {
  return bytes <= (size_t)dctn_dev().lds &&
         hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

namespace {
__global__ __launch_bounds__(256) void dctn_zero_k(unsigned* __restrict__ p, size_t words) {
  const size_t n4 = words / 4;
  uint4* p4 = reinterpret_cast<uint4*>(p);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) p4[i] = uint4{0u, 0u, 0u, 0u};
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += stride) p[i] = 0u;
}
__global__ __launch_bounds__(256) void dctn_zero_words_k(unsigned* __restrict__ p, size_t words) {   // 4-byte aligned only
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += stride) p[i] = 0u;
}
__global__ __launch_bounds__(256) void dctn_zero_bytes_k(unsigned char* __restrict__ p, size_t bytes) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < bytes; i += stride) p[i] = 0;
}
}  // namespace

int dctn_zero_async(void* ptr, size_t bytes, hipStream_t st) {
  if (bytes == 0) return DCTN_OK;
  if (!ptr) return DCTN_ERR_NULL;
  if ((bytes & 3) || ((uintptr_t)ptr & 3)) {   // odd sizes (bf16 tails): byte by byte
    size_t bb = (bytes + 255) / 256;
    if (bb > 2048) bb = 2048;
    hipLaunchKernelGGL(dctn_zero_bytes_k, dim3((unsigned)bb), dim3(256), 0, st, (unsigned char*)ptr, bytes);
    return hipGetLastError() == hipSuccess ? DCTN_OK : DCTN_ERR_LAUNCH;
  }
  const size_t words = bytes / 4;
  size_t blocks = (words / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  if (((uintptr_t)ptr & 15) == 0)
    hipLaunchKernelGGL(dctn_zero_k, dim3((unsigned)blocks), dim3(256), 0, st, (unsigned*)ptr, words);
  else
    hipLaunchKernelGGL(dctn_zero_words_k, dim3((unsigned)blocks), dim3(256), 0, st, (unsigned*)ptr, words);
  return hipGetLastError() == hipSuccess ? DCTN_OK : DCTN_ERR_LAUNCH;
}

static bool dtype_ok(int dtype) { return dtype == DCTN_F32 || dtype == DCTN_F64 || dtype == DCTN_BF16; }

// the EpsP of a query: no tensor, so the strides of a contiguous-like dummy
static bool eps_query_params(EpsP& p, int C, int B, int H, int W, int Q, int K, int O, int policy) {
  const int64_t dummy[5] = {0, 0, 0, 0, 1};
  return eps_fill_params(p, dummy, C, B, H, W, Q, K, O, policy) == DCTN_OK;
}

// ---------------------------------------------------------------------------------------------- EPS routing
// Which family takes a (shape, dtype, policy), decided in ONE place (DESIGN.md "EPS routing").  Every entry point and
// every query below reads the route; no other function asks a family whether it covers a shape.
enum { EPS_NO_FAMILY = -1 };
enum EpsSavedLayout {
  EPS_SAVED_NONE = 0,   // the family keeps nothing
  EPS_SAVED_Z,       // large-core families: the GEMM result Z, row-quad-major
  EPS_SAVED_HALVES   // two-halves path: P0 | P1 | Z
};

struct EpsRoute {
  int precision;        // what every family but bf16x3 is called with: DCTN_PREC_SPLIT runs them as DCTN_PREC_EXACT
  // the forward: the family that takes the call (fwd[0]: what dctn_eps_family answers), then what a run-time decline of
  // a launcher falls to, in order; EPS_NO_FAMILY ends the list.  A forward that was handed room for the saved buffer
  // starts at fwd[fwd_saving]
  int fwd[6], fwd_saving;
  int saved_layout;     // how the backward of this shape reads a saved buffer; a forward family keeps only in this layout
  size_t saved_bytes;   // its size; 0: the shape keeps nothing
  // the backward: a register-resident family computes dCore in a launch of its own at the head of the workspace
  // (EPS_NO_FAMILY: none), without / with a saved buffer; `bwd` computes dX and what is left, in fall-through order
  int dcore_reg, dcore_reg_saved;
  int bwd[4];
};

static void eps_list(int* out, int a, int b = EPS_NO_FAMILY, int c = EPS_NO_FAMILY) {
  out[0] = a, out[1] = b, out[2] = c, out[3] = EPS_NO_FAMILY;
}

static int eps_saved_layout_of(int family) {
  if (family == DCTN_EPS_FAMILY_BIGCORE_F32 || family == DCTN_EPS_FAMILY_BIGCORE_BF16X3) return EPS_SAVED_Z;
  return family == DCTN_EPS_FAMILY_HALVES ? EPS_SAVED_HALVES : EPS_SAVED_NONE;
}

static EpsRoute eps_route(const EpsP& p, int dtype, int policy) {
  const int precision = policy & DCTN_PREC_MASK;
  EpsRoute r = {};   // (nothing saved, the forward with room starts where the plain one does)
  r.precision = precision == DCTN_PREC_SPLIT ? DCTN_PREC_EXACT : precision;
  r.dcore_reg = r.dcore_reg_saved = EPS_NO_FAMILY;
  if (p.opts & DCTN_OPT_GENERIC_KERNELS) {   // short-circuits everything
    eps_list(r.fwd, DCTN_EPS_FAMILY_GENERIC);
    eps_list(r.bwd, DCTN_EPS_FAMILY_GENERIC);
    return r;
  }
  const bool q2reg = eps_mfma_covers(p, dtype, r.precision), q2f32 = eps_q2f32_covers(p, dtype, r.precision);
  const bool halves = eps_halves_wanted(p, dtype);
  // DCTN_OPT_F32_PREFER_HALVES sends float32 shapes that both exact families cover to the two-halves path
  const bool prefer_halves = (p.opts & DCTN_OPT_F32_PREFER_HALVES) && dtype == DCTN_F32 && halves;
  const bool bigcore = eps_bigcore_covers(p, dtype, r.precision) && !prefer_halves;
  // DCTN_PREC_SPLIT: the bf16x3 large-core family takes the float32 shapes it plans among those that run on the exact
  // large-core family under DCTN_PREC_EXACT; every other call runs as under DCTN_PREC_EXACT.  It never runs half a call:
  // nothing follows it in the lists
  if (precision == DCTN_PREC_SPLIT && bigcore && !q2reg && !q2f32 && eps_bf16x3_covers(p, dtype, precision)) {
    eps_list(r.fwd, DCTN_EPS_FAMILY_BIGCORE_BF16X3);
    eps_list(r.bwd, DCTN_EPS_FAMILY_BIGCORE_BF16X3);
    r.saved_layout = EPS_SAVED_Z;
    r.saved_bytes = eps_bf16x3_saved_bytes(p, dtype, precision);   // (the exact family's layout and size)
    return r;
  }
  // the forward walks this order from the first family that covers the shape; the launchers before it would decline
  const int order[5] = {DCTN_EPS_FAMILY_Q2REG, DCTN_EPS_FAMILY_Q2REG_F32, DCTN_EPS_FAMILY_BIGCORE_F32, DCTN_EPS_FAMILY_HALVES,
                        DCTN_EPS_FAMILY_GENERIC};
  const bool covers[5] = {q2reg, q2f32, bigcore, halves, true};
  r.saved_layout = bigcore ? EPS_SAVED_Z : EPS_SAVED_HALVES;
  r.saved_bytes = bigcore ? eps_bigcore_saved_bytes(p, dtype, r.precision) : eps_halves_saved_bytes(p, dtype);
  int n = 0;
  for (int i = 0; i < 5; ++i)
    if ((n > 0 || covers[i]) && !(order[i] == DCTN_EPS_FAMILY_BIGCORE_F32 && prefer_halves)) r.fwd[n++] = order[i];
  r.fwd[n] = EPS_NO_FAMILY;
  // the register-resident exact-f32 family keeps nothing for a backward: a training forward whose caller brought room for
  // Z skips it and runs on the large-core family, whose backward reads Z
  r.fwd_saving = r.fwd[0] == DCTN_EPS_FAMILY_Q2REG_F32 && r.saved_layout == EPS_SAVED_Z && r.saved_bytes > 0;
  // dCore of the register-resident shapes on their own family (the exact-f32 one only where the forward ran there too:
  // without a saved buffer); dX, and dCore of every other shape, on the family whose layout the saved buffer has.  A
  // two-halves launcher that declines falls to the large-core launchers, which take what they plan, then the generic ones
  r.dcore_reg = q2reg ? DCTN_EPS_FAMILY_Q2REG : q2f32 ? DCTN_EPS_FAMILY_Q2REG_F32 : EPS_NO_FAMILY;
  r.dcore_reg_saved = q2reg ? DCTN_EPS_FAMILY_Q2REG : EPS_NO_FAMILY;
  if (r.saved_layout == EPS_SAVED_HALVES)
    eps_list(r.bwd, DCTN_EPS_FAMILY_HALVES, DCTN_EPS_FAMILY_BIGCORE_F32, DCTN_EPS_FAMILY_GENERIC);
  else
    eps_list(r.bwd, DCTN_EPS_FAMILY_BIGCORE_F32, DCTN_EPS_FAMILY_GENERIC);
  return r;
}

// one family's forward; keep: room for what the family keeps for the backward, or NULL
static int eps_fwd_family(int family, const void* x, const void* core, void* out, void* ws, size_t ws_bytes, const EpsP& p,
                          int dtype, const EpsRoute& r, hipStream_t st, void* keep) {
  switch (family) {
    case DCTN_EPS_FAMILY_BIGCORE_BF16X3: return eps_fwd_bf16x3(x, core, out, ws, ws_bytes, p, dtype, DCTN_PREC_SPLIT, st, keep);
    case DCTN_EPS_FAMILY_Q2REG: return eps_fwd_mfma(x, core, out, p, dtype, r.precision, st);
    case DCTN_EPS_FAMILY_Q2REG_F32: return eps_fwd_q2f32(x, core, out, p, dtype, r.precision, st);
    case DCTN_EPS_FAMILY_BIGCORE_F32: return eps_fwd_bigcore(x, core, out, ws, ws_bytes, p, dtype, r.precision, st, keep);
    case DCTN_EPS_FAMILY_HALVES: return eps_fwd_halves(x, core, out, ws, ws_bytes, p, dtype, st, keep);
  }
  return eps_fwd_generic(x, core, out, ws, ws_bytes, p, dtype, st);
}

// ---------------------------------------------------------------------------------------------- fused head
// The prologue of the two head calls: the feature-layout bit is the head's own (eps_fill_params refuses it), so it is
// stripped for the shape and set again for the launchers
static int eps_head_params(EpsP& p, const int64_t x_strides[5], int C, int B, int H, int W, int Q, int K, int O, int Cout,
                           int dtype, int policy) {
  if (!dtype_ok(dtype)) return DCTN_ERR_BAD_DTYPE;
  if (Cout < 1) return DCTN_ERR_BAD_SHAPE;
  const int blk = policy & DCTN_OPT_HEAD_FEATURES_BLOCKED4;
  const int rc = eps_fill_params(p, x_strides, C, B, H, W, Q, K, O, policy & ~blk);
  p.opts |= blk;
  return rc;
}

// the head's two families in order: the bf16 register family, then (given its return code: whether) the float32 one,
// which knows row-major features only
static bool eps_head_next(const EpsP& p, int rc) {
  return rc == DCTN_ERR_UNSUPPORTED && !(p.opts & DCTN_OPT_HEAD_FEATURES_BLOCKED4);
}

extern "C" {

int dctn_version(void) { return 522; }   // callers only check that a library answers (>= 100)

const char* dctn_last_kernel(void) { return g_last_kernel.load(std::memory_order_relaxed); }

int dctn_device_limits(int* cus, int* lds_bytes) {
  if (!cus || !lds_bytes) return DCTN_ERR_NULL;
  *cus = dctn_dev().cus;
  *lds_bytes = dctn_dev().lds;
  return DCTN_OK;
}

const char* dctn_strerror(int code) {
  switch (code) {
    case DCTN_OK: return "ok";
    case DCTN_ERR_BAD_SHAPE: return "inconsistent shape";
    case DCTN_ERR_BAD_DTYPE: return "unknown dtype code";
    case DCTN_ERR_UNSUPPORTED: return "shape/dtype not covered by any kernel of this build";
    case DCTN_ERR_WORKSPACE: return "workspace missing or too small";
    case DCTN_ERR_LAUNCH: return "HIP launch error";
    case DCTN_ERR_NULL: return "required pointer is NULL";
  }
  return "unknown error";
}

// The workspace queries answer a maximum over what the fall-through order may reach, not the first family's need.  The two
// forward queries never looked at DCTN_OPT_GENERIC_KERNELS (they size for the families the flag bypasses); kept.
size_t dctn_eps_fwd_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O, int dtype,
                                    int policy) {
  EpsP p;
  if (!eps_query_params(p, C, B, H, W, Q, K, O, policy & ~DCTN_OPT_GENERIC_KERNELS)) return 0;
  const EpsRoute r = eps_route(p, dtype, policy);
  if (r.fwd[0] == DCTN_EPS_FAMILY_BIGCORE_BF16X3) return eps_fwd_bf16x3_workspace(p, dtype, policy & DCTN_PREC_MASK) + 256;
  const size_t a = eps_fwd_bigcore_workspace(p, dtype, r.precision), b = eps_fwd_halves_workspace(p, dtype);
  return std::max(a, b) + 256;
}

int dctn_eps_family(int C, int B, int H, int W, int Q, int K, int O, int dtype, int policy) {
  EpsP p;
  if (!dtype_ok(dtype) || !eps_query_params(p, C, B, H, W, Q, K, O, policy)) return -1;
  return eps_route(p, dtype, policy).fwd[0];
}

// forward with an optional buffer for what the backward would otherwise recompute; *kept = 1 when it was written
static int eps_fwd_impl(const void* x, const int64_t x_strides[5], const void* core, void* out, void* saved,
                        size_t saved_bytes, int* kept, void* workspace, size_t workspace_bytes, int C, int B, int H, int W,
                        int Q, int K, int O, int dtype, int policy, void* stream) {
  if (kept) *kept = 0;
  if (!x || !core || !out || !x_strides) return DCTN_ERR_NULL;
  if (!dtype_ok(dtype)) return DCTN_ERR_BAD_DTYPE;
  EpsP p;
  int rc = eps_fill_params(p, x_strides, C, B, H, W, Q, K, O, policy);
  if (rc != DCTN_OK) return rc;
  const EpsRoute r = eps_route(p, dtype, policy);
  const bool room = saved && r.saved_bytes > 0 && saved_bytes >= r.saved_bytes;
  for (const int* f = r.fwd + (room ? r.fwd_saving : 0);; ++f) {
    // a family keeps the buffer only where the backward will read it as ITS layout: a shape the large-core family claims
    // but then declines falls to the two-halves path with nothing kept
    const bool keep = room && eps_saved_layout_of(*f) == r.saved_layout;
    rc = eps_fwd_family(*f, x, core, out, workspace, workspace_bytes, p, dtype, r, (hipStream_t)stream, keep ? saved : nullptr);
    if (rc == DCTN_OK && keep && kept) *kept = 1;
    // run-time declines: the runtime refuses a launcher's LDS opt-in, a bf16 core is not 16-byte aligned, the two-halves
    // path has too little workspace
    const bool declined = rc == DCTN_ERR_UNSUPPORTED || (rc == DCTN_ERR_WORKSPACE && *f == DCTN_EPS_FAMILY_HALVES);
    if (!declined || f[1] == EPS_NO_FAMILY) return rc;
  }
}

int dctn_eps_fwd(const void* x, const int64_t x_strides[5], const void* core, void* out,
                 void* workspace, size_t workspace_bytes, int C, int B, int H, int W, int Q, int K,
                 int O, int dtype, int policy, void* stream) {
  return eps_fwd_impl(x, x_strides, core, out, nullptr, 0, nullptr, workspace, workspace_bytes, C, B, H, W, Q, K, O, dtype,
                      policy, stream);
}

size_t dctn_eps_saved_bytes(int C, int B, int H, int W, int Q, int K, int O, int dtype, int policy) {
  EpsP p;
  if (!dtype_ok(dtype) || !eps_query_params(p, C, B, H, W, Q, K, O, policy)) return 0;
  const EpsRoute r = eps_route(p, dtype, policy);
  // a shape of the bf16 register family keeps nothing: its forward has no GEMM result.  (Only after a run-time decline of
  // that launcher does its forward reach a family that keeps, for a caller that brought a buffer all the same.)
  return r.fwd[0] == DCTN_EPS_FAMILY_Q2REG ? 0 : r.saved_bytes;
}

int dctn_eps_fwd_save(const void* x, const int64_t x_strides[5], const void* core, void* out, void* saved,
                      size_t saved_bytes, void* workspace, size_t workspace_bytes, int C, int B, int H, int W, int Q,
                      int K, int O, int dtype, int policy, void* stream) {
  int kept = 0;
  const int rc = eps_fwd_impl(x, x_strides, core, out, saved, saved_bytes, &kept, workspace, workspace_bytes, C, B, H, W, Q,
                              K, O, dtype, policy, stream);
  return rc != DCTN_OK ? rc : (kept ? DCTN_SAVED : DCTN_OK);
}

size_t dctn_eps_fwd_stats_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O, int dtype, int policy) {
  EpsP p;
  if (!eps_query_params(p, C, B, H, W, Q, K, O, policy & ~DCTN_OPT_GENERIC_KERNELS)) return 0;
  if (eps_route(p, dtype, policy).fwd[0] == DCTN_EPS_FAMILY_Q2REG) return 256;   // in-kernel epilogue: no scratch
  return align256((size_t)p.Wn * O * dtype_size(dtype)) + dctn_eps_fwd_workspace_bytes(C, B, H, W, Q, K, O, dtype, policy) + 256;
}

int dctn_eps_fwd_stats(const void* x, const int64_t x_strides[5], const void* core, void* stats, void* workspace,
                       size_t workspace_bytes, int C, int B, int H, int W, int Q, int K, int O, int dtype, int policy,
                       void* stream) {
  if (!x || !core || !stats || !x_strides) return DCTN_ERR_NULL;
  if (!dtype_ok(dtype)) return DCTN_ERR_BAD_DTYPE;
  EpsP p;
  int rc = eps_fill_params(p, x_strides, C, B, H, W, Q, K, O, policy);
  if (rc != DCTN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  // bf16 register family: the statistics are an epilogue of the forward kernel, nothing is stored.  (Like its workspace
  // query this never looked at DCTN_OPT_GENERIC_KERNELS: the launcher is asked directly and declines other shapes.)
  rc = eps_fwd_mfma(x, core, nullptr, p, dtype, policy & DCTN_PREC_MASK, st, (double*)stats);
  if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  // other families: the slice's output goes to scratch (cache resident for the slice sizes of eps.py:126-137) and one
  // reduction pass folds it into the running sums
  const size_t out_bytes = align256((size_t)p.Wn * O * dtype_size(dtype));
  if (!workspace || workspace_bytes < out_bytes) return DCTN_ERR_WORKSPACE;
  unsigned char* ws = (unsigned char*)workspace;
  rc = dctn_eps_fwd(x, x_strides, core, ws, ws + out_bytes, workspace_bytes - out_bytes, C, B, H, W, Q, K, O, dtype, policy,
                    stream);
  if (rc != DCTN_OK) return rc;
  return eps_out_stats(ws, p.Wn * O, dtype, (double*)stats, st);
}

size_t dctn_eps_bwd_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O, int dtype,
                                    int policy, int need_dx, int need_dcore) {
  EpsP p;
  if (!eps_query_params(p, C, B, H, W, Q, K, O, policy)) return 0;
  const EpsRoute r = eps_route(p, dtype, policy);
  if (r.bwd[0] == DCTN_EPS_FAMILY_BIGCORE_BF16X3) {
    const size_t a = need_dx ? eps_bwd_dfactor_bf16x3_workspace(p, dtype, policy & DCTN_PREC_MASK) : 0;
    const size_t b = need_dcore ? eps_bwd_dcore_bf16x3_workspace(p, dtype, policy & DCTN_PREC_MASK) : 0;
    return std::max(a, b) + 256;
  }
  // [register family's dCore | the rest]
  const size_t a = align256(eps_bwd_mfma_workspace(p, dtype, r.precision, need_dx, need_dcore)) +
                   align256(need_dcore ? eps_bwd_q2f32_workspace(p, dtype, r.precision) : 0);
  size_t b = std::max(eps_bwd_generic_workspace(p, dtype, need_dx, need_dcore),
                      eps_bwd_halves_workspace(p, dtype, need_dx, need_dcore));
  if (need_dx) b = std::max(b, eps_bwd_dfactor_bigcore_workspace(p, dtype, r.precision));
  if (need_dcore) b = std::max(b, eps_bwd_dcore_bigcore_workspace(p, dtype, r.precision));
  return a + b + 256;
}

int dctn_eps_head_fwd(const void* x, const int64_t x_strides[5], const void* core, const void* head_weight,
                      const void* head_bias, void* features, void* logits, int C, int B, int H, int W, int Q, int K, int O,
                      int Cout, int dtype, int policy, void* stream) {
  if (!x || !core || !head_weight || !head_bias || !features || !logits || !x_strides) return DCTN_ERR_NULL;
  EpsP p;
  int rc = eps_head_params(p, x_strides, C, B, H, W, Q, K, O, Cout, dtype, policy);
  if (rc != DCTN_OK) return rc;
  const int precision = policy & DCTN_PREC_MASK;
  hipStream_t st = (hipStream_t)stream;
  rc = eps_head_fwd_mfma(x, core, head_weight, head_bias, features, logits, p, Cout, dtype, precision, st);
  if (!eps_head_next(p, rc)) return rc;
  return eps_head_fwd_q2f32(x, core, head_weight, head_bias, features, logits, p, Cout, dtype, precision, st);
}

size_t dctn_eps_head_bwd_workspace_bytes(int C, int B, int H, int W, int Q, int K, int O, int Cout, int dtype,
                                         int policy) {
  EpsP p;
  const int precision = policy & DCTN_PREC_MASK;
  if (!eps_query_params(p, C, B, H, W, Q, K, O, policy & ~DCTN_OPT_HEAD_FEATURES_BLOCKED4)) return 0;
  const size_t a = eps_head_bwd_mfma_workspace(p, Cout, dtype, precision), b = eps_head_bwd_q2f32_workspace(p, Cout, dtype, precision);
  return (a > b ? a : b) + 256;
}

int dctn_eps_head_bwd(const void* x, const int64_t x_strides[5], const void* features, const void* dLogits,
                      const void* head_weight, void* dCore, void* dWeight, void* dBias, void* workspace,
                      size_t workspace_bytes, int C, int B, int H, int W, int Q, int K, int O, int Cout,
                      int dtype, int policy, void* stream) {
  if (!x || !features || !dLogits || !head_weight || !dCore || !x_strides) return DCTN_ERR_NULL;
  EpsP p;
  int rc = eps_head_params(p, x_strides, C, B, H, W, Q, K, O, Cout, dtype, policy);
  if (rc != DCTN_OK) return rc;
  const int precision = policy & DCTN_PREC_MASK;
  hipStream_t st = (hipStream_t)stream;
  rc = eps_head_bwd_mfma(x, features, dLogits, head_weight, dCore, dWeight, dBias, workspace, workspace_bytes, p, Cout, dtype,
                         precision, st);
  if (!eps_head_next(p, rc)) return rc;
  return eps_head_bwd_q2f32(x, features, dLogits, head_weight, dCore, dWeight, dBias, workspace, workspace_bytes, p, Cout, dtype,
                            precision, st);
}

// ---------------------------------------------------------------------------------------------- EPS backward
static int eps_bwd_impl(const void* x, const int64_t x_strides[5], const void* core, const void* dY, const void* saved,
                        size_t saved_bytes, void* dX, void* dCore, void* workspace, size_t workspace_bytes, int C, int B,
                        int H, int W, int Q, int K, int O, int dtype, int policy, void* stream) {
  if (!x || !core || !dY || !x_strides) return DCTN_ERR_NULL;
  if (!dtype_ok(dtype)) return DCTN_ERR_BAD_DTYPE;
  if (!dX && !dCore) return DCTN_OK;
  EpsP p;
  int rc = eps_fill_params(p, x_strides, C, B, H, W, Q, K, O, policy);
  if (rc != DCTN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const EpsRoute r = eps_route(p, dtype, policy);
  unsigned char* ws = (unsigned char*)workspace;
  size_t ws_bytes = workspace_bytes;
  // dCore on a register-resident family, in the first (256-byte aligned) part of the workspace
  const int reg = saved ? r.dcore_reg_saved : r.dcore_reg;
  if (dCore && reg != EPS_NO_FAMILY) {
    const size_t w = align256(reg == DCTN_EPS_FAMILY_Q2REG ? eps_bwd_mfma_workspace(p, dtype, r.precision, 0, 1)
                                                           : eps_bwd_q2f32_workspace(p, dtype, r.precision));
    if (!ws || ws_bytes < w) return DCTN_ERR_WORKSPACE;
    rc = reg == DCTN_EPS_FAMILY_Q2REG ? eps_bwd_mfma(x, core, dY, nullptr, dCore, ws, w, p, dtype, r.precision, st)
                                      : eps_bwd_q2f32(x, dY, dCore, ws, w, p, dtype, r.precision, st);
    if (rc == DCTN_OK) dCore = nullptr;
    else if (rc != DCTN_ERR_UNSUPPORTED) return rc;
    ws += w;
    ws_bytes -= w;
  }
  // dX and what is left of dCore, in the rest of the workspace
  for (const int* f = r.bwd; dX || dCore; ++f) {
    switch (*f) {
      case DCTN_EPS_FAMILY_BIGCORE_BF16X3:
        // (dCore's slices are summed before dX uses the same workspace: stream order)
        if (dCore) {
          rc = eps_bwd_dcore_bf16x3(x, dY, dCore, p, dtype, DCTN_PREC_SPLIT, st, ws, ws_bytes);
          if (rc != DCTN_OK) return rc;
        }
        if (dX) {
          rc = eps_bwd_dx_bf16x3(x, core, dY, dX, ws, ws_bytes, p, dtype, DCTN_PREC_SPLIT, st, saved, saved_bytes);
          if (rc != DCTN_OK) return rc == DCTN_ERR_UNSUPPORTED ? DCTN_ERR_LAUNCH : rc;
        }
        return DCTN_OK;
      case DCTN_EPS_FAMILY_HALVES:   // both gradients on the two-halves GEMM path
        rc = eps_bwd_halves(x, core, dY, dX, dCore, ws, ws_bytes, p, dtype, st, saved, saved_bytes);
        if (rc != DCTN_ERR_UNSUPPORTED && rc != DCTN_ERR_WORKSPACE) return rc;
        break;
      case DCTN_EPS_FAMILY_BIGCORE_F32:
        if (dCore) {
          // (its per-chunk slices use the workspace before dX does: the sum kernel is done with them by then)
          rc = eps_bwd_dcore_bigcore(x, dY, dCore, p, dtype, r.precision, st, ws, ws_bytes);
          if (rc == DCTN_OK) dCore = nullptr;
          else if (rc != DCTN_ERR_UNSUPPORTED) return rc;
        }
        if (dX) {
          rc = eps_bwd_dx_bigcore(x, core, dY, dX, ws, ws_bytes, p, dtype, r.precision, st, saved, saved_bytes);
          if (rc == DCTN_OK) dX = nullptr;
          else if (rc != DCTN_ERR_UNSUPPORTED && rc != DCTN_ERR_WORKSPACE) return rc;
        }
        break;
      default:
        return eps_bwd_generic(x, core, dY, dX, dCore, ws, ws_bytes, p, dtype, st);
    }
  }
  return DCTN_OK;
}

int dctn_eps_bwd(const void* x, const int64_t x_strides[5], const void* core, const void* dY,
                 void* dX, void* dCore, void* workspace, size_t workspace_bytes, int C, int B,
                 int H, int W, int Q, int K, int O, int dtype, int policy, void* stream) {
  return eps_bwd_impl(x, x_strides, core, dY, nullptr, 0, dX, dCore, workspace, workspace_bytes, C, B, H, W, Q, K, O, dtype,
                      policy, stream);
}

int dctn_eps_bwd_saved(const void* x, const int64_t x_strides[5], const void* core, const void* dY, const void* saved,
                       size_t saved_bytes, void* dX, void* dCore, void* workspace, size_t workspace_bytes, int C, int B,
                       int H, int W, int Q, int K, int O, int dtype, int policy, void* stream) {
  if (!saved) return DCTN_ERR_NULL;
  return eps_bwd_impl(x, x_strides, core, dY, saved, saved_bytes, dX, dCore, workspace, workspace_bytes, C, B, H, W, Q, K,
                      O, dtype, policy, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- ConvSBS routing
// Every entry point walks its families top to bottom (DESIGN.md "ConvSBS routing"): DCTN_ERR_UNSUPPORTED = nothing written, ask the next.
// bonds 5..16 go to the band family, except that under DCTN_SBS_MATRIX_CORE_SWEEP bonds up to 8 stay on the matrix-core
// sweep (the tests hold both against the oracle)
static bool band_family_first(const SbsShape& sh, int dtype_flags) {
  int largest = 0;
  for (int c = 0; c < sh.n; ++c) largest = sh.bond_sizes[c] > largest ? sh.bond_sizes[c] : largest;
  return !((dtype_flags & DCTN_SBS_MATRIX_CORE_SWEEP) && largest <= 8);
}

constexpr int SBS_FLAGS = DCTN_SBS_MATRIX_CORE_SWEEP | DCTN_SBS_WIDE_SWEEP;

extern "C" {

size_t dctn_convsbs_workspace_bytes(int n_cores, const int* out_sizes, const int* bond_sizes, int C, int B, int H, int W, int q,
                                    const int* pos_h, const int* pos_w, int dtype_flags, int backward) {
  const int dtype = dtype_flags & DCTN_DTYPE_MASK;   // (the query covers every family: flags only select among them)
  if (!out_sizes || !bond_sizes || !pos_h || !pos_w) return 0;
  const SbsShape sh{n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype};
  if (convsbs_check_shape(sh, nullptr) != DCTN_OK) return 0;
  if (!backward) return 256;
  bool fits = false;
  size_t m = std::max({convsbs_bwd_generic_workspace(sh, &fits), convsbs_reg_bwd_workspace(sh), convsbs_band_bwd_workspace(sh)});
  // the wide family: where the generic sweep's LDS plan declines the string, or where the flag forces it
  if ((dtype_flags & DCTN_SBS_WIDE_SWEEP) || !fits) m = std::max(m, convsbs_wide_bwd_workspace(sh));
  return m + 256;
}

size_t dctn_convsbs_saved_states_bytes(int n_cores, const int* out_sizes, const int* bond_sizes, int C, int B, int H,
                                       int W, int q, const int* pos_h, const int* pos_w, int dtype_flags) {
  if (!out_sizes || !bond_sizes || !pos_h || !pos_w) return 0;
  return convsbs_saved_states_bytes({n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype_flags & DCTN_DTYPE_MASK});
}

int dctn_convsbs_fwd(const void* x, const int64_t x_strides[5], const void* const* cores, void* out, int n_cores,
                     const int* out_sizes, const int* bond_sizes, const int* pos_h, const int* pos_w, int C, int B, int H, int W,
                     int q, void* workspace, size_t workspace_bytes, int dtype_flags, void* stream) {
  if (!x || !x_strides || !cores || !out || !out_sizes || !bond_sizes || !pos_h || !pos_w) return DCTN_ERR_NULL;
  if (dtype_flags & ~(DCTN_DTYPE_MASK | SBS_FLAGS)) return DCTN_ERR_UNSUPPORTED;
  const SbsShape sh{n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype_flags & DCTN_DTYPE_MASK};
  int rc = convsbs_check_shape(sh, cores);
  if (rc != DCTN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  // a workspace of dctn_convsbs_saved_states_bytes(...) bytes: the forward leaves its states there for
  // dctn_convsbs_bwd_saved (a training forward); anything smaller: plain forward
  // small bonds: the register-resident sweep (keeps nothing: its backward recomputes the chain in registers)
  if (!(dtype_flags & DCTN_SBS_MATRIX_CORE_SWEEP)) {
    rc = convsbs_fwd_reg(x, x_strides, cores, out, sh, st);
    if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  }
  // bonds 5..16: the band family's forward (nothing kept: its backward recomputes the chain in registers)
  if (band_family_first(sh, dtype_flags)) {
    rc = convsbs_fwd_band(x, x_strides, cores, out, sh, st);
    if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  }
  const size_t sb = convsbs_saved_states_bytes(sh);
  float* save = (sb > 0 && workspace && workspace_bytes >= sb) ? (float*)workspace : nullptr;
  rc = convsbs_fwd_mfma(x, x_strides, cores, out, sh, st, save);
  // the caller learns whether the states were WRITTEN: only the matrix-core sweep writes them, and it can still decline
  // a string the size query accepted (its LDS plan); the generic sweep below leaves the buffer untouched
  if (rc == DCTN_OK) return save ? DCTN_SAVED : DCTN_OK;
  if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  return convsbs_fwd_generic(x, x_strides, cores, out, sh, st);
}

int dctn_convsbs_bwd(const void* x, const int64_t x_strides[5], const void* const* cores, const void* dY, void* dX,
                     void* const* dCores, int n_cores, const int* out_sizes, const int* bond_sizes, const int* pos_h,
                     const int* pos_w, int C, int B, int H, int W, int q, void* workspace, size_t workspace_bytes,
                     int dtype_flags, void* stream) {
  return dctn_convsbs_bwd_saved(x, x_strides, cores, dY, dX, dCores, n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H,
                                W, q, workspace, workspace_bytes, nullptr, 0, dtype_flags, stream);
}

int dctn_convsbs_bwd_saved(const void* x, const int64_t x_strides[5], const void* const* cores, const void* dY, void* dX,
                           void* const* dCores, int n_cores, const int* out_sizes, const int* bond_sizes, const int* pos_h,
                           const int* pos_w, int C, int B, int H, int W, int q, void* workspace, size_t workspace_bytes,
                           const void* saved_states, size_t saved_states_bytes, int dtype_flags, void* stream) {
  if (!x || !x_strides || !cores || !dY || !out_sizes || !bond_sizes || !pos_h || !pos_w) return DCTN_ERR_NULL;
  if (dtype_flags & ~(DCTN_DTYPE_MASK | SBS_FLAGS)) return DCTN_ERR_UNSUPPORTED;
  const SbsShape sh{n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype_flags & DCTN_DTYPE_MASK};
  if (saved_states) {   // only what the forward of this very shape can have written
    const size_t sb = convsbs_saved_states_bytes(sh);
    if (sb == 0 || saved_states_bytes < sb) saved_states = nullptr;
  }
  if (!dX && !dCores) return DCTN_OK;
  int rc = convsbs_check_shape(sh, cores);
  if (rc != DCTN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (dtype_flags & DCTN_SBS_WIDE_SWEEP) {   // forced: the wide family for every string it covers
    rc = convsbs_bwd_wide(x, x_strides, cores, dY, dX, dCores, sh, st, workspace, workspace_bytes);
    if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  }
  if (sh.dtype == DCTN_F32 && band_family_first(sh, dtype_flags)) {   // (true whenever the register family is tried)
    for (int c = 0; dCores && c < n_cores; ++c)
      if (!dCores[c]) return DCTN_ERR_NULL;
    if (!(dtype_flags & DCTN_SBS_MATRIX_CORE_SWEEP)) {
      rc = convsbs_bwd_reg(x, x_strides, cores, dY, dX, (float* const*)dCores, sh, st, workspace, workspace_bytes);
      if (rc != DCTN_ERR_UNSUPPORTED) return rc;
    }
    // bonds 5..16: the band-owning backward (recomputes the chain; no saved states, no helper launches)
    rc = convsbs_bwd_band(x, x_strides, cores, dY, dX, (float* const*)dCores, sh, st, workspace, workspace_bytes);
    if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  }
  // the generic sweep's plan declines only for its LDS, before it writes anything: the wide family takes those strings
  SbsBwdPlan plan;
  rc = convsbs_bwd_generic_plan(plan, sh, dCores, workspace, workspace_bytes, st);
  if (rc == DCTN_ERR_UNSUPPORTED) return convsbs_bwd_wide(x, x_strides, cores, dY, dX, dCores, sh, st, workspace, workspace_bytes);
  if (rc != DCTN_OK) return rc;
  // float32 strings of the matrix-core family: its sweep, in the planned workspace with the accumulators already zero
  // (a dX-only backward stays on the generic sweep)
  if (sh.dtype == DCTN_F32 && dCores) {
    rc = convsbs_bwd_mfma(x, x_strides, cores, dY, (float*)plan.states, dX ? (float*)plan.gxw : nullptr, (float* const*)dCores,
                          sh, st, plan.partials, plan.partial_bytes, (const float*)saved_states);
    if (rc == DCTN_OK) return dX ? convsbs_gather_dx(sh, plan.gxw, dX, st) : DCTN_OK;
    if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  }
  return convsbs_bwd_generic_run(plan, x, x_strides, cores, dY, dX, dCores, sh, st);
}

// ---- several strings of one layer (ManyConvSBS, dctn/conv_sbs.py:314-370) in one launch each way
size_t dctn_convsbs_many_workspace_bytes(int n_strings, int n_cores, const int* out_sizes, const int* bond_sizes, int C, int B,
                                         int H, int W, int q, const int* pos_h, const int* pos_w, int dtype) {
  if (!out_sizes || !bond_sizes || !pos_h || !pos_w) return 0;
  const SbsShape sh{n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype & DCTN_DTYPE_MASK};
  const size_t a = convsbs_many_reg_bwd_workspace(n_strings, sh);
  return a > 0 ? a : convsbs_many_band_bwd_workspace(n_strings, sh);
}

int dctn_convsbs_many_fwd(const void* x, const int64_t x_strides[5], const void* const* cores, void* const* outs,
                          int n_strings, int n_cores, const int* out_sizes, const int* bond_sizes, const int* pos_h,
                          const int* pos_w, int C, int B, int H, int W, int q, int dtype, void* stream) {
  if (!x || !x_strides || !cores || !outs || !out_sizes || !bond_sizes || !pos_h || !pos_w) return DCTN_ERR_NULL;
  if (n_strings < 1 || n_cores < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype & ~DCTN_DTYPE_MASK) return DCTN_ERR_UNSUPPORTED;
  for (int i = 0; i < n_strings * n_cores; ++i)
    if (!cores[i]) return DCTN_ERR_NULL;
  const SbsShape sh{n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype};
  const int rc = convsbs_many_fwd_reg(x, x_strides, cores, outs, n_strings, sh, (hipStream_t)stream);
  if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  return convsbs_many_fwd_band(x, x_strides, cores, outs, n_strings, sh, (hipStream_t)stream);
}

int dctn_convsbs_many_bwd(const void* x, const int64_t x_strides[5], const void* const* cores, const void* const* dYs, void* dX,
                          void* const* dCores, int n_strings, int n_cores, const int* out_sizes, const int* bond_sizes,
                          const int* pos_h, const int* pos_w, int C, int B, int H, int W, int q, void* workspace,
                          size_t workspace_bytes, int dtype, void* stream) {
  if (!x || !x_strides || !cores || !dYs || !out_sizes || !bond_sizes || !pos_h || !pos_w) return DCTN_ERR_NULL;
  if (n_strings < 1 || n_cores < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype & ~DCTN_DTYPE_MASK) return DCTN_ERR_UNSUPPORTED;
  if (!dX && !dCores) return DCTN_OK;
  for (int i = 0; i < n_strings * n_cores; ++i)
    if (!cores[i] || (dCores && !dCores[i])) return DCTN_ERR_NULL;
  const SbsShape sh{n_cores, out_sizes, bond_sizes, pos_h, pos_w, C, B, H, W, q, dtype};
  const int rc = convsbs_many_bwd_reg(x, x_strides, cores, dYs, dX, (float* const*)dCores, n_strings, sh, (hipStream_t)stream,
                                      workspace, workspace_bytes);
  if (rc != DCTN_ERR_UNSUPPORTED) return rc;
  return convsbs_many_bwd_band(x, x_strides, cores, dYs, dX, (float* const*)dCores, n_strings, sh, (hipStream_t)stream, workspace,
                               workspace_bytes);
}

}  // extern "C"
