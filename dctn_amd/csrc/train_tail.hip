// The tail of a training iteration: everything around the contraction
// path that the reference's loop runs per iteration (dctn/training.py:77-84) — cross-entropy on the
// (batch, classes) logits, the L2 regulariser (dctn/eps_plus_linear.py:149-159,
// dctn/epses_composition.py:144-146) and the optimizer update — is a few kilobytes of data, but as
// library calls it is ~30 launches of 4-5 us each, 3x the time of the forward + backward kernels of
// BASELINE config 2.  Three kernels replace them:
//   ce_fwd_k   : mean cross-entropy of bf16/f32 logits (max-shifted log-sum-exp, float32; rows labelled -100 are skipped
//                and do not count in the mean, as F.cross_entropy's default ignore_index)
//   ce_bwd_k   : dLogits = (softmax - onehot) * dLoss / n, in the logits' dtype
//   SgdRule    : SGD with momentum as a rule of flat_step_k (flat_step.h), over ONE flat buffer holding all parameters:
//                g += 2 * l2 * w on the regularised prefix, buf = momentum * buf + g, w -= lr * buf; the regulariser's
//                value sum w^2 is left as one partial sum per workgroup (float32 arithmetic; the result is rounded back
//                into the parameter's cell)
#include "flat_step.h"

namespace {

constexpr long long DCTN_CE_IGNORE = -100;   // torch.nn.functional.cross_entropy's default ignore_index

// Number of rows that count in the mean: every workgroup scans all labels itself (8 bytes per row out of L2; the mean's
// divisor is needed before the first gradient row is written, and a workgroup cannot wait for the others)
__device__ __forceinline__ float ce_count_valid(const long long* __restrict__ labels, long long B, float* red) {
  float n = 0.f;
  for (long long b = threadIdx.x; b < B; b += blockDim.x) n += labels[b] != DCTN_CE_IGNORE ? 1.f : 0.f;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  float total = 0.f;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) total += red[k];
  __syncthreads();   // `red` is reused by the caller
  return total;
}

// SINGLE: the whole batch in one workgroup of 1024 threads — the result is stored, not accumulated, so no fill
// precedes the kernel (one graph node instead of two; these kernels are launch-latency, not work)
template <typename S, bool SINGLE>
__global__ __launch_bounds__(SINGLE ? 1024 : 256) void ce_fwd_k(const S* __restrict__ logits,
                                                                const long long* __restrict__ labels,
                                                                float* __restrict__ loss, S* __restrict__ dunit,
                                                                long long B, int C) {
  // dunit (optional): (softmax - onehot) / n, the gradient of the mean loss for an incoming gradient of 1; n = the number
  // of rows whose label is not DCTN_CE_IGNORE (F.cross_entropy's default ignore_index): such rows add nothing to the loss,
  // get a zero gradient row and do not count in the mean
  __shared__ float red[16];
  const float n_valid = ce_count_valid(labels, B, red);
  float part = 0.f;
  for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (long long)gridDim.x * blockDim.x) {
    const S* row = logits + b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, (float)row[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf((float)row[c] - m);
    const long long y = labels[b];
    // any OTHER label outside [0, C) poisons the loss and its row of the gradient with NaN: F.cross_entropy raises /
    // device-asserts on such labels; a plausible-looking number would hide the bug
    const bool skip = y == DCTN_CE_IGNORE, valid = y >= 0 && y < C;
    part += skip ? 0.f : valid ? (m + logf(s)) - (float)row[y] : __builtin_nanf("");
    if (dunit) {
      const float inv = 1.f / s, scale = skip ? 0.f : valid ? 1.f / n_valid : __builtin_nanf("");
      for (int c = 0; c < C; ++c)
        dunit[b * C + c] = (S)((expf((float)row[c] - m) * inv - (c == y ? 1.f : 0.f)) * scale);
    }
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) total += red[k];
    if (SINGLE)
      loss[0] = total / n_valid;   // (no row counted: 0 / 0 = NaN, as torch)
    else
      atomicAdd(loss, total / n_valid);
  }
}

template <typename S>
__global__ __launch_bounds__(256) void ce_bwd_k(const S* __restrict__ logits, const long long* __restrict__ labels,
                                                const float* __restrict__ dloss, S* __restrict__ dlogits, long long B,
                                                int C) {
  __shared__ float red[16];
  const float scale = dloss[0] / ce_count_valid(labels, B, red);
  for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (long long)gridDim.x * blockDim.x) {
    const S* row = logits + b * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, (float)row[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf((float)row[c] - m);
    const float inv = 1.f / s;
    const long long y = labels[b];
    const float rs = y == DCTN_CE_IGNORE ? 0.f : (y >= 0 && y < C) ? scale : __builtin_nanf("");   // ignored: zero row; invalid: NaN row
    for (int c = 0; c < C; ++c) {
      const float p = expf((float)row[c] - m) * inv;
      dlogits[b * C + c] = (S)((p - (c == y ? 1.f : 0.f)) * rs);
    }
  }
}

struct SgdCoef {
  float lr, momentum, two_l2;   // lr, first_step: of a launch without a step block, zeros otherwise
  int first_step;
};
// DECAY (the pack ends with an SgdDecay by value): torch.optim.SGD's coupled weight decay, g = fmaf(wd, w, g), in front of
// the 2 * l2 * w term and the momentum - Adam's order, and torch's.  Without the member the gradient keeps its bits.
// With a group table every segment takes its own decay from the table and the member's value is not looked at.
struct SgdDecay {
  float wd;
};

// torch.optim.SGD(momentum, dampening = 0) as a rule of flat_step_k (flat_step.h): one state array, the momentum buffer;
// workgroups of 256 threads, at most 1024 of them, no vector form.  The step block is optional: a pack without a
// schedule, a group table or an average takes `lr` and `first_step` from the launch, touches no step block and draws no
// ticket - the plain kernel is the fastest of the family because of it.  With a step block the first step is
// steps_done == 0, with a table the SEGMENT's steps == 0 (torch's `momentum_buffer is None`).
struct SgdRule {
  using Coef = SgdCoef;
  static constexpr int THREADS = 256, MAX_BLOCKS = 1024;
  static constexpr bool HAS_VEC = false, STATE_ALWAYS = false;
  static constexpr SecondState SECOND = SecondState::never;
  struct Segment {
    float lr, wd;
    bool first, frozen;
  };
  static __device__ __forceinline__ Segment segment(const Coef&, float rate, int steps, float wd, bool frozen) {
    return Segment{rate, wd, steps == 0, frozen};
  }
  template <typename... G> static __device__ __forceinline__ float launch_wd(const Coef&, G... pack) {
    if constexpr (pack_has_v<SgdDecay, G...>) return pack_get<SgdDecay>(pack...).wd; else return 0.f;
  }
  // torch.optim.SGD: the first step copies g - the buffer is written and not read
  static __device__ __forceinline__ bool skips_state_read(const Segment& sg) { return sg.first; }
  template <typename... G>
  static __device__ __forceinline__ float elem(float wi, float gi, float& buf, float&, bool, bool reg, const Coef& k,
                                               const Segment& sg, float& part) {
    if constexpr (pack_has_v<SgdDecay, G...>) gi = fmaf(sg.wd, wi, gi);
    if (reg) {
      gi = fmaf(k.two_l2, wi, gi);
      part = fmaf(wi, wi, part);
    }
    buf = sg.first ? gi : fmaf(k.momentum, buf, gi);
    return fmaf(-sg.lr, buf, wi);
  }
};

unsigned blocks_for(long long n) { return flat_step_blocks_for<SgdRule>(n); }   // the cross-entropy kernels' grid, too

// Validates and launches.  With a schedule, a group table or an average the rate and first_step come from the step block
// on the device: the block is required, and the two launch arguments are zeros whatever the caller passed.
int sgd_step(const dctn_flat_step_t& d, void* momentum_buf, float lr, float momentum, int first_step, void* stream,
             const dctn_weight_ema_t* ema = nullptr, const float* decay = nullptr) {
  const bool on_device = d.schedule || d.groups || ema;
  if (const int rc = flat_step_check(d, ema, {momentum_buf, on_device ? d.state : &d})) return rc;
  if (decay && !(*decay >= 0.f)) return DCTN_ERR_BAD_SHAPE;
  const SgdCoef k{on_device ? 0.f : lr, momentum, 2.f * d.l2, on_device ? 0 : first_step};
  const FlatStepLaunch<SgdRule> a{d, momentum_buf, nullptr, k, (hipStream_t)stream, ema};
  return decay ? flat_step_run(a, SgdDecay{*decay}) : flat_step_run(a);
}


}  // namespace

extern "C" {

static int ce_fwd_launch(const void* logits, const void* labels, void* loss, void* dunit, int64_t B, int C, int dtype,
                         hipStream_t st) {
  if (!logits || !labels || !loss) return DCTN_ERR_NULL;
  if (B < 1 || C < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  if (B <= 8192) {   // one workgroup, no fill
    if (dtype == DCTN_F32)
      hipLaunchKernelGGL((ce_fwd_k<float, true>), dim3(1), dim3(1024), 0, st, (const float*)logits, (const long long*)labels, (float*)loss, (float*)dunit, (long long)B, C);
    else
      hipLaunchKernelGGL((ce_fwd_k<bf16_t, true>), dim3(1), dim3(1024), 0, st, (const bf16_t*)logits, (const long long*)labels, (float*)loss, (bf16_t*)dunit, (long long)B, C);
    DCTN_CHECK_LAUNCH();
    return DCTN_OK;
  }
  if (dctn_zero_async(loss, sizeof(float), st) != DCTN_OK) return DCTN_ERR_LAUNCH;
  const dim3 g(blocks_for(B)), b(256);
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL((ce_fwd_k<float, false>), g, b, 0, st, (const float*)logits, (const long long*)labels, (float*)loss, (float*)dunit, (long long)B, C);
  else
    hipLaunchKernelGGL((ce_fwd_k<bf16_t, false>), g, b, 0, st, (const bf16_t*)logits, (const long long*)labels, (float*)loss, (bf16_t*)dunit, (long long)B, C);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

int dctn_ce_loss_fwd(const void* logits, const void* labels, void* loss, int64_t B, int C, int dtype, void* stream) {
  return ce_fwd_launch(logits, labels, loss, nullptr, B, C, dtype, (hipStream_t)stream);
}

int dctn_ce_loss_fwd_grad(const void* logits, const void* labels, void* loss, void* dlogits_unit, int64_t B, int C,
                          int dtype, void* stream) {
  if (!dlogits_unit) return DCTN_ERR_NULL;
  return ce_fwd_launch(logits, labels, loss, dlogits_unit, B, C, dtype, (hipStream_t)stream);
}

int dctn_ce_loss_bwd(const void* logits, const void* labels, const void* dloss, void* dlogits, int64_t B, int C,
                     int dtype, void* stream) {
  if (!logits || !labels || !dloss || !dlogits) return DCTN_ERR_NULL;
  if (B < 1 || C < 1) return DCTN_ERR_BAD_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(blocks_for(B)), b(256);
  switch (dtype) {
    case DCTN_F32: hipLaunchKernelGGL(ce_bwd_k<float>, g, b, 0, st, (const float*)logits, (const long long*)labels, (const float*)dloss, (float*)dlogits, (long long)B, C); break;
    case DCTN_BF16: hipLaunchKernelGGL(ce_bwd_k<bf16_t>, g, b, 0, st, (const bf16_t*)logits, (const long long*)labels, (const float*)dloss, (bf16_t*)dlogits, (long long)B, C); break;
    default: return DCTN_ERR_BAD_DTYPE;
  }
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

int dctn_sgd_l2_num_partials(int64_t n) { return n < 1 ? 0 : (int)blocks_for(n); }

int dctn_sgd_flat_step(const dctn_flat_step_t* step, void* momentum_buf, float lr, float momentum, int first_step,
                       void* stream) {
  if (!step) return DCTN_ERR_NULL;
  return sgd_step(*step, momentum_buf, lr, momentum, first_step, stream);
}

// ema_or_null == NULL is dctn_sgd_flat_step
int dctn_sgd_flat_step_ema(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* momentum_buf,
                           float lr, float momentum, int first_step, void* stream) {
  if (!step) return DCTN_ERR_NULL;
  return sgd_step(*step, momentum_buf, lr, momentum, first_step, stream, ema_or_null);
}

// dctn_sgd_flat_step_ema with torch.optim.SGD's coupled weight decay: the DECAY kernels, for any weight_decay >= 0.  With
// a group table every segment's decay comes from the table and the argument is not used
int dctn_sgd_flat_step_decay(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* momentum_buf,
                             float lr, float momentum, float weight_decay, int first_step, void* stream) {
  if (!step) return DCTN_ERR_NULL;
  return sgd_step(*step, momentum_buf, lr, momentum, first_step, stream, ema_or_null, &weight_decay);
}

// The six entry points older than the descriptor: each fills one and takes sgd_step.  An entry point that requires a
// block answers its null pointer itself; the _scheduled / _grouped forms have no lr and first_step to pass
int dctn_sgd_l2_step(void* params, const void* grads, void* momentum_buf, void* sq_sum, int64_t n, int64_t n_reg,
                     float lr, float momentum, float l2, int first_step, int dtype, void* stream) {
  const dctn_flat_step_t d = {params, nullptr, grads, sq_sum, nullptr, nullptr, nullptr, nullptr, n, n_reg, l2, dtype};
  return sgd_step(d, momentum_buf, lr, momentum, first_step, stream);
}

int dctn_sgd_l2_step_master(void* master, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                            int64_t n, int64_t n_reg, float lr, float momentum, float l2, int first_step, void* stream) {
  if (!master) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master, grads, sq_sum, nullptr, nullptr, nullptr, nullptr, n, n_reg, l2, DCTN_BF16};
  return sgd_step(d, momentum_buf, lr, momentum, first_step, stream);
}

int dctn_sgd_l2_step_guarded(void* params, const void* grads, void* momentum_buf, void* sq_sum, const void* guard,
                             int64_t n, int64_t n_reg, float lr, float momentum, float l2, int first_step, int dtype,
                             void* stream) {
  if (!guard) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, nullptr, grads, sq_sum, nullptr, guard, nullptr, nullptr, n, n_reg, l2, dtype};
  return sgd_step(d, momentum_buf, lr, momentum, first_step, stream);
}

int dctn_sgd_l2_step_master_guarded(void* master, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                                    const void* guard, int64_t n, int64_t n_reg, float lr, float momentum, float l2,
                                    int first_step, void* stream) {
  if (!master || !guard) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master, grads, sq_sum, nullptr, guard, nullptr, nullptr, n, n_reg, l2, DCTN_BF16};
  return sgd_step(d, momentum_buf, lr, momentum, first_step, stream);
}

int dctn_sgd_l2_step_scheduled(void* master_or_null, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                               void* state, const void* guard_or_null, const void* schedule, int64_t n, int64_t n_reg,
                               float momentum, float l2, int dtype, void* stream) {
  if (!schedule) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master_or_null, grads, sq_sum, state, guard_or_null, schedule, nullptr,
                              n, n_reg, l2, dtype};
  return sgd_step(d, momentum_buf, 0.f, momentum, 0, stream);
}

// The grouped form always takes the 16-byte step block: without a schedule the rate is state->lr, as Adam's
int dctn_sgd_l2_step_grouped(void* master_or_null, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                             void* state, const void* guard_or_null, const void* schedule_or_null, void* groups,
                             int64_t n, int64_t n_reg, float momentum, float l2, int dtype, void* stream) {
  if (!groups) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master_or_null, grads, sq_sum, state, guard_or_null, schedule_or_null, groups,
                              n, n_reg, l2, dtype};
  return sgd_step(d, momentum_buf, 0.f, momentum, 0, stream);
}

}  // extern "C"
