// The reference's documented recipe trains with Adam (new_runner.py:496-498: Adam(model.parameters(), lr, weight_decay))
// and scores with cross-entropy + accuracy per batch (dctn/evaluation.py:7-22).  Two kernels beside train_tail.hip's:
//   AdamRule   : torch.optim.Adam (coupled weight decay) as a rule of flat_step_k (flat_step.h): one update + the L2
//                regulariser over ONE flat parameter buffer.  The step count t and the learning rate are read from a
//                16-byte device block, and the launch itself advances t: a captured graph replays the same node and
//                still gets t, t+1, t+2, ...
//   ce_score_k : adds one batch's {sum of cross-entropies, correct rows, rows} to three float64 values
#include "flat_step.h"

#include <cmath>

namespace {

constexpr long long DCTN_CE_IGNORE = -100;   // torch.nn.functional.cross_entropy's default ignore_index

struct AdamCoef {
  double ln_b1, ln_b2;        // ln(beta): 1 - beta^t = -expm1(t * ln beta), formed in the kernel from t
  float b1, omb1, b2, omb2;   // beta, 1 - beta (formed in double on the host, then rounded once)
  float eps, wd, two_l2;
};

// torch.optim.Adam (coupled weight decay) as a rule of flat_step_k (flat_step.h): two state arrays, exp_avg and
// exp_avg_sq; workgroups of 1024 threads, at most 256 of them (the ticket: 1024 workgroups of 256 threads took 17.7 us
// over 1.9 M parameters where the same stream without a ticket, plain SGD, takes 5.7 us); a vector form.
struct AdamRule {
  using Coef = AdamCoef;
  static constexpr int THREADS = 1024, MAX_BLOCKS = 256;
  static constexpr bool HAS_VEC = true, STATE_ALWAYS = true;
  static constexpr SecondState SECOND = SecondState::always;
  struct Segment {
    float step, bc2_sqrt, wd;
    bool frozen;
  };
  // The two bias corrections in float64, once per workgroup and segment, rounded once - what torch's host arithmetic
  // gives.  In float32 the difference 1 - beta2^t cancels: at t = 1 it is 0.001 with the absolute error of 0.999, a
  // relative 6e-5 in every update of the first steps.  (From t itself, not as running products, which drift.)  Without a
  // table t is steps_done + 1 on lane 0; with one it is the segment's own count + 1 on that segment's lane
  // (torch.optim.Adam's per-parameter state["step"]).
  static __device__ __forceinline__ Segment segment(const Coef& k, float rate, int steps, float wd, bool frozen) {
    const int t = steps + 1;
    return Segment{(float)((double)rate / -expm1((double)t * k.ln_b1)), (float)sqrt(-expm1((double)t * k.ln_b2)), wd, frozen};
  }
  template <typename... G> static __device__ __forceinline__ float launch_wd(const Coef& k, G...) { return k.wd; }
  static __device__ __forceinline__ bool skips_state_read(const Segment&) { return false; }
  template <typename... G>
  static __device__ __forceinline__ float elem(float wi, float gi, float& m, float& v, bool, bool reg, const Coef& k,
                                               const Segment& sg, float& part) {
    gi = fmaf(sg.wd, wi, gi);
    if (reg) {
      gi = fmaf(k.two_l2, wi, gi);
      part = fmaf(wi, wi, part);
    }
    m = fmaf(k.b1, m, k.omb1 * gi);
    v = fmaf(k.b2, v, (k.omb2 * gi) * gi);
    const float denom = sqrtf(v) / sg.bc2_sqrt + k.eps;
    return fmaf(-sg.step, m / denom, wi);
  }
};

// Validates and launches.  master_first: the _scheduled / _grouped entry points answer a master copy beside a dtype
// that is not bf16 in front of every other check; everywhere else it is part of the dtype check, the last one
int adam_step(const dctn_flat_step_t& d, void* exp_avg, void* exp_avg_sq, double beta1, double beta2, float eps,
              float weight_decay, void* stream, bool master_first = false, const dctn_weight_ema_t* ema = nullptr) {
  if (master_first && d.master && d.dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  if (const int rc = flat_step_check(d, ema, {exp_avg, exp_avg_sq, d.state})) return rc;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return DCTN_ERR_BAD_SHAPE;   // torch raises ValueError
  AdamCoef k;
  k.b1 = (float)beta1, k.omb1 = (float)(1.0 - beta1), k.b2 = (float)beta2, k.omb2 = (float)(1.0 - beta2);
  k.ln_b1 = std::log(beta1), k.ln_b2 = std::log(beta2);   // beta = 0: -inf, and 1 - beta^t = -expm1(-inf) = 1
  k.eps = eps, k.wd = d.groups ? 0.f : weight_decay, k.two_l2 = 2.f * d.l2;   // a table carries every segment's decay
  return flat_step_run(FlatStepLaunch<AdamRule>{d, exp_avg, exp_avg_sq, k, (hipStream_t)stream, ema});
}

__device__ __forceinline__ float ld_f32(const float* p) { return *p; }
__device__ __forceinline__ float ld_f32(const bf16_t* p) { return (float)*p; }

// ONE workgroup of 16 waves for any batch: the three sums have one fixed order, so the result is the same bits from
// run to run, and nothing needs a fill or a float atomic (scoring batches are 1e3 .. 1e4 rows of ~10 classes: a few
// hundred KB at most, launch latency).  A row belongs to P = min(64, next power of two >= C) neighbouring lanes; lane j of
// them holds classes j, j + P, ...; maximum, sum of exponentials and the lowest index of a maximum are closed by xor
// butterflies.  The exponentials are float32 (as ce_fwd_k's); everything that accumulates is float64, like `acc`.
template <typename S>
__global__ __launch_bounds__(1024) void ce_score_k(const S* __restrict__ logits, const long long* __restrict__ labels,
                                                   double* __restrict__ acc, long long B, int C, int P) {
  __shared__ double red[3][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (P - 1);
  const int rows_per_wave = 64 / P;
  double loss = 0.0, correct = 0.0, rows = 0.0;   // only a row's first lane adds to them
  // (wave-uniform trip count: the shuffles below need every lane of the wave)
  for (long long r0 = (long long)wave * rows_per_wave; r0 < B; r0 += 16LL * rows_per_wave) {
    const long long b = r0 + lane / P;
    const bool live = b < B;
    const S* row = logits + (live ? b : 0) * C;
    float m = -INFINITY;
    for (int c = sub; c < C; c += P) m = fmaxf(m, ld_f32(row + c));
    for (int off = P >> 1; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    double s = 0.0;   // float32 exponentials, summed in float64
    int first = 0x7fffffff;   // lowest class index that holds the maximum: torch.argmax's answer on ties
    for (int c = sub; c < C; c += P) {
      const float x = ld_f32(row + c);
      s += (double)expf(x - m);
      if (x == m && c < first) first = c;
    }
    for (int off = P >> 1; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      first = min(first, __shfl_xor(first, off, 64));
    }
    if (live && sub == 0) {
      const long long y = labels[b];
      if (y != DCTN_CE_IGNORE) {
        const bool valid = y >= 0 && y < C;
        // log-softmax's order, -((x_y - m) - log s); x_y - m is small and (nearly) exact in float32.  The logarithm is
        // taken in float64, one per row: this device's float32 log is low by 0.3 - 0.5 ulp on average for arguments
        // in [2, 10] (measured against float64: -7.6e-8 on [5, 10]), a bias that adds up over the rows of a batch
        loss += valid ? log(s) - (double)(ld_f32(row + (valid ? y : 0)) - m) : (double)__builtin_nanf("");
        correct += valid && y == (long long)first ? 1.0 : 0.0;
        rows += 1.0;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    loss += __shfl_down(loss, off, 64);
    correct += __shfl_down(correct, off, 64);
    rows += __shfl_down(rows, off, 64);
  }
  if (lane == 0) red[0][wave] = loss, red[1][wave] = correct, red[2][wave] = rows;
  __syncthreads();
  if (threadIdx.x < 3) {   // stream order makes the read-modify-write safe: one workgroup, one launch at a time
    double total = 0.0;
    for (int k = 0; k < 16; ++k) total += red[threadIdx.x][k];
    acc[threadIdx.x] += total;
  }
}

// The averaged weights in place of the live ones, for a scoring pass: stash = params, then params = (S)ema with the
// step kernels' round-to-nearest-even cast.  A master copy is never touched.
template <typename S>
__global__ __launch_bounds__(256) void weight_ema_apply_k(S* __restrict__ w, S* __restrict__ stash,
                                                          const float* __restrict__ em, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    stash[i] = w[i];
    w[i] = (S)em[i];
  }
}
template <typename S>
__global__ __launch_bounds__(256) void weight_ema_restore_k(S* __restrict__ w, const S* __restrict__ stash, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    w[i] = stash[i];
}
unsigned ema_copy_blocks_for(long long n) {
  long long b = (n + 255) / 256;
  if (b > 1024) b = 1024;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

size_t dctn_adam_state_bytes(void) { return sizeof(StepStateBlock); }

size_t dctn_flat_step_bytes(void) { return sizeof(dctn_flat_step_t); }

int dctn_adam_l2_num_partials(int64_t n) { return n < 1 ? 0 : (int)flat_step_blocks_for<AdamRule>(n); }

int dctn_adam_flat_step(const dctn_flat_step_t* step, void* exp_avg, void* exp_avg_sq, double beta1, double beta2,
                        float eps, float weight_decay, void* stream) {
  if (!step) return DCTN_ERR_NULL;
  return adam_step(*step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream);
}

// The six entry points older than the descriptor: each fills one and takes adam_step.  An entry point that requires a
// block answers its null pointer itself (in front of the master / dtype check of the _scheduled / _grouped forms)
int dctn_adam_l2_step(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, void* sq_sum, void* state,
                      int64_t n, int64_t n_reg, double beta1, double beta2, float eps, float weight_decay, float l2,
                      int dtype, void* stream) {
  const dctn_flat_step_t d = {params, nullptr, grads, sq_sum, state, nullptr, nullptr, nullptr, n, n_reg, l2, dtype};
  return adam_step(d, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream);
}

int dctn_adam_l2_step_master(void* master, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                             void* sq_sum, void* state, int64_t n, int64_t n_reg, double beta1, double beta2, float eps,
                             float weight_decay, float l2, void* stream) {
  if (!master) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master, grads, sq_sum, state, nullptr, nullptr, nullptr, n, n_reg, l2, DCTN_BF16};
  return adam_step(d, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream);
}

int dctn_adam_l2_step_guarded(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, void* sq_sum, void* state,
                              const void* guard, int64_t n, int64_t n_reg, double beta1, double beta2, float eps,
                              float weight_decay, float l2, int dtype, void* stream) {
  if (!guard) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, nullptr, grads, sq_sum, state, guard, nullptr, nullptr, n, n_reg, l2, dtype};
  return adam_step(d, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream);
}

int dctn_adam_l2_step_master_guarded(void* master, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                                     void* sq_sum, void* state, const void* guard, int64_t n, int64_t n_reg,
                                     double beta1, double beta2, float eps, float weight_decay, float l2, void* stream) {
  if (!master || !guard) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master, grads, sq_sum, state, guard, nullptr, nullptr, n, n_reg, l2, DCTN_BF16};
  return adam_step(d, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream);
}

int dctn_adam_l2_step_scheduled(void* master_or_null, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                                void* sq_sum, void* state, const void* guard_or_null, const void* schedule, int64_t n,
                                int64_t n_reg, double beta1, double beta2, float eps, float weight_decay, float l2,
                                int dtype, void* stream) {
  if (!schedule) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master_or_null, grads, sq_sum, state, guard_or_null, schedule, nullptr,
                              n, n_reg, l2, dtype};
  return adam_step(d, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream, true);
}

// The table carries every segment's weight decay: the launch has no weight_decay argument
int dctn_adam_l2_step_grouped(void* master_or_null, void* params, const void* grads, void* exp_avg, void* exp_avg_sq,
                              void* sq_sum, void* state, const void* guard_or_null, const void* schedule_or_null,
                              void* groups, int64_t n, int64_t n_reg, double beta1, double beta2, float eps, float l2,
                              int dtype, void* stream) {
  if (!groups) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master_or_null, grads, sq_sum, state, guard_or_null, schedule_or_null, groups,
                              n, n_reg, l2, dtype};
  return adam_step(d, exp_avg, exp_avg_sq, beta1, beta2, eps, 0.f, stream, true);
}

size_t dctn_weight_ema_bytes(void) { return sizeof(WeightEmaBlock); }

// Host only: validates a HOST copy of the block and forms the weight of the launch at `updates` with the kernels' function
int dctn_weight_ema_weight(const void* host_block, int64_t updates, float* one_minus_decay) {
  if (!host_block || !one_minus_decay) return DCTN_ERR_NULL;
  const WeightEmaBlock& b = *(const WeightEmaBlock*)host_block;
  if (!(std::isfinite(b.decay) && b.decay >= 0.f && b.decay < 1.f)) return DCTN_ERR_BAD_SHAPE;
  if ((b.flags & ~DCTN_EMA_WARMUP) != 0u) return DCTN_ERR_BAD_SHAPE;
  if (b.updates < 0 || updates < 0 || updates > 0x7fffffffLL) return DCTN_ERR_BAD_SHAPE;
  *one_minus_decay = weight_ema_omd(b.decay, b.flags, (int)updates);
  return DCTN_OK;
}

// ema_or_null == NULL is dctn_adam_flat_step
int dctn_adam_flat_step_ema(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* exp_avg,
                            void* exp_avg_sq, double beta1, double beta2, float eps, float weight_decay, void* stream) {
  if (!step) return DCTN_ERR_NULL;
  return adam_step(*step, exp_avg, exp_avg_sq, beta1, beta2, eps, weight_decay, stream, false, ema_or_null);
}

int dctn_weight_ema_apply(void* params, void* stash, const void* ema, int64_t n, int dtype, void* stream) {
  if (!params || !stash || !ema) return DCTN_ERR_NULL;
  if (n < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  const dim3 grid(ema_copy_blocks_for(n)), block(256);
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL(weight_ema_apply_k<float>, grid, block, 0, (hipStream_t)stream, (float*)params, (float*)stash, (const float*)ema, (long long)n);
  else
    hipLaunchKernelGGL(weight_ema_apply_k<bf16_t>, grid, block, 0, (hipStream_t)stream, (bf16_t*)params, (bf16_t*)stash, (const float*)ema, (long long)n);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

int dctn_weight_ema_restore(void* params, const void* stash, int64_t n, int dtype, void* stream) {
  if (!params || !stash) return DCTN_ERR_NULL;
  if (n < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  const dim3 grid(ema_copy_blocks_for(n)), block(256);
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL(weight_ema_restore_k<float>, grid, block, 0, (hipStream_t)stream, (float*)params, (const float*)stash, (long long)n);
  else
    hipLaunchKernelGGL(weight_ema_restore_k<bf16_t>, grid, block, 0, (hipStream_t)stream, (bf16_t*)params, (const bf16_t*)stash, (long long)n);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

size_t dctn_param_groups_bytes(void) { return sizeof(ParamGroupBlock); }

// Host only: validates a HOST copy of the table for a flat buffer of n elements
int dctn_param_groups_check(const void* host_block, int64_t n) {
  if (!host_block) return DCTN_ERR_NULL;
  const ParamGroupBlock& b = *(const ParamGroupBlock*)host_block;
  if (n < 1 || b.n_segments < 1 || b.n_segments > DCTN_PG_MAX_SEGMENTS) return DCTN_ERR_BAD_SHAPE;
  for (int i = 0; i < b.n_segments; ++i) {
    if (b.end[i] <= (i > 0 ? b.end[i - 1] : 0)) return DCTN_ERR_BAD_SHAPE;   // no empty segment
    if (!(std::isfinite(b.lr_scale[i]) && b.lr_scale[i] >= 0.f)) return DCTN_ERR_BAD_SHAPE;
    if (!(std::isfinite(b.weight_decay[i]) && b.weight_decay[i] >= 0.f)) return DCTN_ERR_BAD_SHAPE;
    if ((b.flags[i] & ~DCTN_PG_FROZEN) != 0u || b.steps[i] < 0) return DCTN_ERR_BAD_SHAPE;
  }
  if (b.end[b.n_segments - 1] != (long long)n) return DCTN_ERR_BAD_SHAPE;
  return DCTN_OK;
}

size_t dctn_lr_schedule_bytes(void) { return sizeof(LrScheduleBlock); }

// Host only: validates a HOST copy of the block and evaluates it with the function the kernels run
int dctn_lr_schedule_value(const void* host_block, int64_t step, float* out) {
  if (!host_block || !out) return DCTN_ERR_NULL;
  const LrScheduleBlock& b = *(const LrScheduleBlock*)host_block;
  if (step < 0 || b.n_knots < 1 || b.n_knots > DCTN_LR_MAX_KNOTS) return DCTN_ERR_BAD_SHAPE;
  if (!(std::isfinite(b.scale) && b.scale >= 0.f)) return DCTN_ERR_BAD_SHAPE;
  for (int i = 0; i < b.n_knots; ++i) {
    if (b.k[i] < 0 || (i > 0 && b.k[i] <= b.k[i - 1])) return DCTN_ERR_BAD_SHAPE;
    if (!(std::isfinite(b.lr[i]) && b.lr[i] >= 0.f)) return DCTN_ERR_BAD_SHAPE;
  }
  *out = lr_schedule_value_host(b, (long long)step);
  return DCTN_OK;
}

int dctn_ce_score_accumulate(const void* logits, const void* labels, void* acc, int64_t B, int C, int dtype,
                             void* stream) {
  if (!logits || !labels || !acc) return DCTN_ERR_NULL;
  if (B < 1 || C < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  hipStream_t st = (hipStream_t)stream;
  int P = 1;
  while (P < C && P < 64) P <<= 1;
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL(ce_score_k<float>, dim3(1), dim3(1024), 0, st, (const float*)logits, (const long long*)labels, (double*)acc, (long long)B, C, P);
  else
    hipLaunchKernelGGL(ce_score_k<bf16_t>, dim3(1), dim3(1024), 0, st, (const bf16_t*)logits, (const long long*)labels, (double*)acc, (long long)B, C, P);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
