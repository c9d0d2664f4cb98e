// The tail of a training iteration: everything around the contraction
// path that the reference's loop runs per iteration (dctn/training.py:77-84) — cross-entropy on the
// (batch, classes) logits, the L2 regulariser (dctn/eps_plus_linear.py:149-159,
// dctn/epses_composition.py:144-146) and the optimizer update — is a few kilobytes of data, but as
// library calls it is ~30 launches of 4-5 us each, 3x the time of the forward + backward kernels of
// BASELINE config 2.  Three kernels replace them:
//   ce_fwd_k   : mean cross-entropy of bf16/f32 logits (max-shifted log-sum-exp, float32; rows labelled -100 are skipped
//                and do not count in the mean, as F.cross_entropy's default ignore_index)
//   ce_bwd_k   : dLogits = (softmax - onehot) * dLoss / n, in the logits' dtype
//   sgd_l2_k   : over ONE flat buffer holding all parameters: g += 2 * l2 * w on the regularised
//                prefix, buf = momentum * buf + g, w -= lr * buf; the regulariser's value
//                sum w^2 is left as one partial sum per workgroup (float32 arithmetic; the result is rounded back
//                into the parameter's cell).  MASTER form (bf16 parameters): the step runs on a float32 master
//                copy, which is read and written; the bf16 cell only receives the rounded result.  DECAY form:
//                torch.optim.SGD's coupled weight decay, g += wd * w, in front of the 2 * l2 * w term
#include "common.h"
#include "grad_guard.h"
#include "lr_schedule.h"
#include "param_groups.h"
#include "weight_ema.h"

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

// The arithmetic of one element; every product-sum is an explicit fmaf (the contraction the compiler chose for the
// plain expressions), so that every instantiation of the kernel produces the same bits
__device__ __forceinline__ float sgd_elem(float wi, float gi, float* __restrict__ buf, bool reg, float lr, float momentum,
                                          float two_l2, int first_step, float& part) {
  if (reg) {
    gi = fmaf(two_l2, wi, gi);
    part = fmaf(wi, wi, part);
  }
  const float bi = first_step ? gi : fmaf(momentum, *buf, gi);   // torch.optim.SGD: the first step copies g
  *buf = bi;
  return fmaf(-lr, bi, wi);
}

// DECAY (the pack ends with an SgdDecay by value): torch.optim.SGD's coupled weight decay, g = fmaf(wd, w, g), in front of
// the 2 * l2 * w term and the momentum - Adam's order, and torch's.  Without the member the gradient keeps its bits.
struct SgdDecay {
  float wd;
};
template <bool DECAY> __device__ __forceinline__ float sgd_decayed(float gi, float wi, float wd) {
  if constexpr (DECAY) return fmaf(wd, wi, gi); else return gi;
}
// The grouped form's LDS copy of the segments' decays exists only in the DECAY instantiations
template <bool DECAY> __device__ __forceinline__ float* sgd_seg_wd() {
  if constexpr (DECAY) {
    __shared__ float seg_wd[DCTN_PG_MAX_SEGMENTS];
    return seg_wd;
  } else {
    return nullptr;
  }
}

// MASTER (S = bf16_t): the weight comes from and goes back to the float32 array `wm`; `w` gets its bf16 rounding and is
// not read, and `wm` and the sq_sum slots are the float instantiation's bits.  Without MASTER `wm` is unused (null).
// GUARD: the step obeys a gradient guard's decision (grad_guard.hip, launched in front of this kernel), as
// adam_l2_k's guarded form does: lane 0 of every workgroup reads `halted` and `coef` before anything else; halted, the
// workgroup returns at once and writes no parameter, master value, momentum or sq_sum slot; otherwise every gradient is
// replaced by ONE rounded float32 product g * coef in front of sgd_elem (the 2 * l2 * w term comes after the clip).
// The guard block is a trailing parameter PACK, empty in the unguarded instantiations, and the rest is behind
// `if constexpr`: those compile to what they did.
// SCHED (the pack also holds a StepStateBlock* and a const LrScheduleBlock*): the launch arguments `lr` and `first_step`
// are not used.  The 16-byte step block is adam_l2_k's, with the same ticket: wave 0 loads steps_done and the table, one
// knot per lane, finds the segment with a ballot (lr_schedule.h) and publishes the rate and first_step = (steps_done
// == 0) through LDS, together with the guard's decision when there is one; the workgroup that draws the last ticket
// writes steps_done + 1 and the rate it used.  A halted guarded step returns before the ticket: steps_done stays, and
// the schedule holds its place.
// GROUPED (the pack ends with a ParamGroupBlock*, and always holds a StepStateBlock*): the launch obeys a parameter-group
// table (param_groups.h states the semantics).  Wave 0 loads the table, one segment per lane, beside steps_done and the
// rate - state->lr, or the schedule's value at the GLOBAL steps_done - and publishes every segment's end, rate (one
// rounded product rate * lr_scale), first_step = (the SEGMENT's steps == 0) and frozen flag through LDS.  Every lane
// walks a cursor over the ends as its elements increase.  A frozen element only adds w * w below n_reg: its gradient
// and momentum are not read and nothing of it is stored.  The table's weight_decay is used by the DECAY form only: there
// every segment takes its own decay from the table and the pack's value is not looked at.
// EMA (the pack ends with a WeightEma, and always holds a StepStateBlock*): every element the step stores to also moves
// its average, from the value the step keeps for it (weight_ema.h).  Lane 0 loads the block's three cells beside
// steps_done and publishes the launch's weight; the last ticket writes updates + 1 and that weight.  Without a schedule
// or a group table the rate is state->lr and first_step is steps_done == 0, as the grouped form reads them.
template <typename S, bool MASTER, bool GUARD, bool SCHED, bool EMA, bool DECAY>
__device__ __forceinline__ void sgd_grouped_body(S* __restrict__ w, float* __restrict__ wm, const S* __restrict__ g,
                                                 float* __restrict__ buf, float* __restrict__ sq_sum, long long n,
                                                 long long n_reg, float momentum, float l2, const GradGuardBlock* guard,
                                                 StepStateBlock* state, const LrScheduleBlock* sched,
                                                 ParamGroupBlock* groups, WeightEma ema) {
  __shared__ float red[4];
  __shared__ float decision[EMA ? 3 : 2];             // halted, coef; EMA: the launch's weight
  __shared__ long long seg_end[DCTN_PG_MAX_SEGMENTS];
  __shared__ float seg_lr[DCTN_PG_MAX_SEGMENTS];
  __shared__ int seg_first[DCTN_PG_MAX_SEGMENTS], seg_frozen[DCTN_PG_MAX_SEGMENTS];
  __shared__ int seg_count;
  [[maybe_unused]] float* const seg_wd = sgd_seg_wd<DECAY>();
  int steps_done = 0, my_steps = 0;
  float rate = 0.f;
  bool my_live = false;   // wave 0: this lane's segment is in use and not frozen
  [[maybe_unused]] WeightEmaLane ema_lane{0, 0.f};   // lane 0
  if (threadIdx.x < 64) {   // wave 0, every lane
    const int lane = threadIdx.x;
    const ParamGroupLane sg = param_group_lane_load(groups, lane);
    if constexpr (EMA) {
      if (lane == 0) decision[2] = (ema_lane = weight_ema_lane_load(ema.block)).omd;
    }
    if constexpr (SCHED) {
      const LrScheduleLane knot = lr_schedule_lane_load(sched, lane);
      steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      rate = lr_schedule_wave_value(knot, lane, steps_done);
    } else {
      steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      rate = __hip_atomic_load(&state->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (GUARD) {
      if (lane == 0) {
        decision[0] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
        decision[1] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    my_steps = sg.steps;
    my_live = lane < sg.n_segments && (sg.flags & DCTN_PG_FROZEN) == 0u;
    seg_end[lane] = sg.end;
    seg_lr[lane] = __fmul_rn(rate, sg.lr_scale);
    seg_first[lane] = sg.steps == 0 ? 1 : 0;
    if constexpr (DECAY) seg_wd[lane] = sg.weight_decay;
    seg_frozen[lane] = (sg.flags & DCTN_PG_FROZEN) != 0u ? 1 : 0;
    if (lane == 0) seg_count = sg.n_segments;
  }
  __syncthreads();
  float coef = 1.f;
  if constexpr (GUARD) {
    if (decision[0] != 0.f) return;   // the whole workgroup, before any store and before the ticket
    coef = decision[1];
  }
  [[maybe_unused]] float omd = 0.f;
  [[maybe_unused]] float* __restrict__ em = nullptr;
  if constexpr (EMA) omd = decision[2], em = ema.values;
  const int n_seg = seg_count;
  ParamGroupCursor cur{0, param_group_end(seg_end, 0, n_seg)};
  float lr = seg_lr[0];
  int first_step = seg_first[0];
  bool frozen = seg_frozen[0] != 0;
  [[maybe_unused]] float wd = 0.f;
  if constexpr (DECAY) wd = seg_wd[0];
  float part = 0.f;
  const float two_l2 = 2.f * l2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (param_group_advance(cur, i, seg_end, n_seg)) {
      lr = seg_lr[cur.seg], first_step = seg_first[cur.seg], frozen = seg_frozen[cur.seg] != 0;
      if constexpr (DECAY) wd = seg_wd[cur.seg];
    }
    if (frozen) {
      if (i < n_reg) {
        const float wi = MASTER ? wm[i] : (float)w[i];
        part = fmaf(wi, wi, part);
      }
      continue;
    }
    const float w0 = MASTER ? wm[i] : (float)w[i];
    const float wi = sgd_elem(w0, sgd_decayed<DECAY>(clipped<GUARD>((float)g[i], coef), w0, wd), buf + i, i < n_reg, lr,
                              momentum, two_l2, first_step, part);
    w[i] = (S)wi;
    if (MASTER) wm[i] = wi;
    if constexpr (EMA) em[i] = weight_ema_elem(em[i], weight_ema_kept<S, MASTER>(wi), omd);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x < 64) {   // wave 0: lane 0 draws the ticket, every lane hears the answer
    unsigned drawn = 0u;
    if (threadIdx.x == 0) {
      if (sq_sum) sq_sum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
      // the ticket of adam_l2_k; the wait covers this wave's loads of steps_done, the rate and the table
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      drawn = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    drawn = __shfl(drawn, 0, 64);
    if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
      if (my_live) groups->steps[threadIdx.x] = my_steps + 1;
      if (threadIdx.x == 0) {
        state->steps_done = steps_done + 1;
        if constexpr (SCHED) state->lr = rate;   // the GLOBAL rate of this step, before any segment's scale
        if constexpr (EMA) weight_ema_advance(ema.block, ema_lane);
        state->ticket = 0u;
      }
    }
  }
}

template <typename S, bool MASTER, typename... G>
__global__ __launch_bounds__(256) void sgd_l2_k(S* __restrict__ w, float* __restrict__ wm, const S* __restrict__ g,
                                                float* __restrict__ buf, float* __restrict__ sq_sum, long long n,
                                                long long n_reg, float lr, float momentum, float l2, int first_step,
                                                G... guard_block) {
  // G holds a const GradGuardBlock* (GUARD), a StepStateBlock* and a const LrScheduleBlock* (SCHED), a ParamGroupBlock*
  // (GROUPED, with the StepStateBlock* whether or not there is a schedule), in that order, or nothing: the plain kernel,
  // parameter for parameter
  // and behind them a WeightEma (EMA, always with the StepStateBlock*): the average's values and block
  // and last an SgdDecay (DECAY): the weight decay, with or without any of the others
  constexpr bool DECAY = pack_has_v<SgdDecay, G...>;
  [[maybe_unused]] float wd = 0.f;
  if constexpr (DECAY) wd = pack_get<SgdDecay>(guard_block...).wd;
  constexpr bool GUARD = pack_has_v<const GradGuardBlock*, G...>, SCHED = pack_has_v<const LrScheduleBlock*, G...>;
  constexpr bool EMA = pack_has_v<WeightEma, G...>;
  [[maybe_unused]] WeightEma ema{nullptr, nullptr};
  if constexpr (EMA) ema = pack_get<WeightEma>(guard_block...);
  if constexpr (pack_has_v<ParamGroupBlock*, G...>) {   // GROUPED: a body of its own; the rest of this one is untouched
    const GradGuardBlock* guard = nullptr;
    const LrScheduleBlock* sched = nullptr;
    if constexpr (GUARD) guard = pack_get<const GradGuardBlock*>(guard_block...);
    if constexpr (SCHED) sched = pack_get<const LrScheduleBlock*>(guard_block...);
    sgd_grouped_body<S, MASTER, GUARD, SCHED, EMA, DECAY>(w, wm, g, buf, sq_sum, n, n_reg, momentum, l2, guard,
                                                   pack_get<StepStateBlock*>(guard_block...), sched,
                                                   pack_get<ParamGroupBlock*>(guard_block...), ema);
    return;
  }
  __shared__ float red[4];
  float coef = 1.f;
  int steps_done = 0;
  [[maybe_unused]] float omd = 0.f;
  [[maybe_unused]] WeightEmaLane ema_lane{0, 0.f};   // thread 0
  // (The EMA prologue repeats the SCHED prologue below with one more published value and the state->lr branch.  The
  // repetition is deliberate: the SCHED text stays as it was, so the instantiations without an average stay the same
  // machine code.)
  if constexpr (EMA) {   // the step block is there with or without a schedule; lane 0 also loads the average's block
    __shared__ float published[5];   // rate, first_step, halted, coef, the average's weight
    if (threadIdx.x < 64) {   // wave 0, every lane: the schedule's ballot needs them all
      StepStateBlock* state = pack_get<StepStateBlock*>(guard_block...);
      float rate;
      if constexpr (SCHED) {
        const LrScheduleLane knot = lr_schedule_lane_load(pack_get<const LrScheduleBlock*>(guard_block...), threadIdx.x);
        steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rate = lr_schedule_wave_value(knot, threadIdx.x, steps_done);
      } else {
        steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rate = __hip_atomic_load(&state->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (threadIdx.x == 0) {
        published[0] = rate, published[1] = steps_done == 0 ? 1.f : 0.f;
        published[4] = (ema_lane = weight_ema_lane_load(ema.block)).omd;
        if constexpr (GUARD) {
          const GradGuardBlock* guard = pack_get<const GradGuardBlock*>(guard_block...);
          published[2] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
          published[3] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    __syncthreads();
    if constexpr (GUARD) {
      if (published[2] != 0.f) return;   // the whole workgroup, before any store and before the ticket
      coef = published[3];
    }
    lr = published[0], first_step = published[1] != 0.f ? 1 : 0, omd = published[4];
  } else if constexpr (SCHED) {
    __shared__ float published[4];   // rate, first_step, halted, coef
    if (threadIdx.x < 64) {   // wave 0, every lane: the ballot needs them all
      const LrScheduleLane knot = lr_schedule_lane_load(pack_get<const LrScheduleBlock*>(guard_block...), threadIdx.x);
      steps_done = __hip_atomic_load(&pack_get<StepStateBlock*>(guard_block...)->steps_done, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
      const float rate = lr_schedule_wave_value(knot, threadIdx.x, steps_done);
      if (threadIdx.x == 0) {
        published[0] = rate, published[1] = steps_done == 0 ? 1.f : 0.f;
        if constexpr (GUARD) {
          const GradGuardBlock* guard = pack_get<const GradGuardBlock*>(guard_block...);
          published[2] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
          published[3] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    __syncthreads();
    if constexpr (GUARD) {
      if (published[2] != 0.f) return;   // the whole workgroup, before any store and before the ticket
      coef = published[3];
    }
    lr = published[0], first_step = published[1] != 0.f ? 1 : 0;
  } else if constexpr (GUARD) {
    __shared__ float decision[2];
    if (threadIdx.x == 0) {
      const GradGuardBlock* guard = pack_get<const GradGuardBlock*>(guard_block...);
      decision[0] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
      decision[1] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (decision[0] != 0.f) return;   // the whole workgroup, before any store
    coef = decision[1];
  }
  [[maybe_unused]] float* __restrict__ em = nullptr;
  if constexpr (EMA) em = ema.values;
  float part = 0.f;
  const float two_l2 = 2.f * l2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float w0 = MASTER ? wm[i] : (float)w[i];
    const float wi = sgd_elem(w0, sgd_decayed<DECAY>(clipped<GUARD>((float)g[i], coef), w0, wd), buf + i, i < n_reg, lr,
                              momentum, two_l2, first_step, part);
    w[i] = (S)wi;
    if (MASTER) wm[i] = wi;
    if constexpr (EMA) em[i] = weight_ema_elem(em[i], weight_ema_kept<S, MASTER>(wi), omd);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  // one slot per workgroup, stored (not accumulated): no fill before the kernel, no atomics, a fixed summation order;
  // the caller adds the dctn_sgd_l2_num_partials(n) slots when it wants the regulariser's value
  if (threadIdx.x == 0 && sq_sum) sq_sum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if constexpr (SCHED || EMA) {
    if (threadIdx.x == 0) {
      // The ticket of adam_l2_k: it orders every workgroup's read of steps_done before the last workgroup's write of it.
      // The wait makes sure this lane's load of steps_done has returned before the ticket is drawn.
      StepStateBlock* state = pack_get<StepStateBlock*>(guard_block...);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      const unsigned drawn = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
        state->steps_done = steps_done + 1;
        if constexpr (SCHED) state->lr = lr;   // without a schedule (EMA alone) the cell is the host's
        if constexpr (EMA) weight_ema_advance(ema.block, ema_lane);
        state->ticket = 0u;
      }
    }
  }
}

unsigned blocks_for(long long n) {
  long long b = (n + 255) / 256;
  if (b > 1024) b = 1024;
  return (unsigned)(b < 1 ? 1 : b);
}

// One step as the host sees it: the descriptor (include/dctn_amd.h) and what only SGD has
struct SgdStep {
  const dctn_flat_step_t& d;
  void* momentum_buf;
  float lr, momentum;
  int first_step;
  hipStream_t st;
  const dctn_weight_ema_t* ema;   // null: no average
  const float* decay;             // null: the kernels without weight decay
};

// The one launcher.  sgd_l2_k is built for the packs that hold the step block exactly when they hold a schedule, a
// group table or an average; sgd_step hands the block over in no other case, so the packs left out are never asked for.
template <typename S, bool MASTER, typename... G> void sgd_launch(const SgdStep& a, G... pack) {
  if constexpr (pack_has_v<StepStateBlock*, G...> ==
                (pack_has_v<const LrScheduleBlock*, G...> || pack_has_v<ParamGroupBlock*, G...> ||
                 pack_has_v<WeightEma, G...>)) {
    const dctn_flat_step_t& d = a.d;
    hipLaunchKernelGGL((sgd_l2_k<S, MASTER, G...>), dim3(blocks_for(d.n)), dim3(256), 0, a.st, (S*)d.params,
                       (float*)d.master, (const S*)d.grads, (float*)a.momentum_buf, (float*)d.sq_sum, (long long)d.n,
                       (long long)d.n_reg, a.lr, a.momentum, d.l2, a.first_step, pack...);
  }
}

// The pack is the optional blocks the step has, in the order sgd_l2_k expects: guard, step state, schedule, group table,
// and the average (a pair by value) and the weight decay (by value) behind them
template <typename S, bool MASTER> void sgd_dispatch(const SgdStep& a, StepStateBlock* state) {
  with_blocks([&](auto... pack) {
    const auto decayed = [&](auto... full) {
      if (a.decay) sgd_launch<S, MASTER>(a, full..., SgdDecay{*a.decay});
      else sgd_launch<S, MASTER>(a, full...);
    };
    if (a.ema) decayed(pack..., WeightEma{(float*)a.ema->ema, (WeightEmaBlock*)a.ema->block});
    else decayed(pack...);
  }, (const GradGuardBlock*)a.d.guard, state, (const LrScheduleBlock*)a.d.schedule, (ParamGroupBlock*)a.d.groups);
}

// Validates and launches.  With a schedule, a group table or an average the rate and first_step come from the step block
// on the device: the block is required, and the two launch arguments are zeros whatever the caller passed.
int sgd_step(const dctn_flat_step_t& d, void* momentum_buf, float lr, float momentum, int first_step, void* stream,
             const dctn_weight_ema_t* ema = nullptr, const float* decay = nullptr) {
  const bool on_device = d.schedule || d.groups || ema;
  if (!d.params || !d.grads || !momentum_buf || (on_device && !d.state)) return DCTN_ERR_NULL;
  if (ema && (!ema->ema || !ema->block)) return DCTN_ERR_NULL;
  if (d.n < 1 || d.n_reg < 0 || d.n_reg > d.n) return DCTN_ERR_BAD_SHAPE;
  if (decay && !(*decay >= 0.f)) return DCTN_ERR_BAD_SHAPE;
  if ((d.dtype != DCTN_F32 && d.dtype != DCTN_BF16) || (d.master && d.dtype != DCTN_BF16)) return DCTN_ERR_BAD_DTYPE;
  const SgdStep a{d, momentum_buf, on_device ? 0.f : lr, momentum, on_device ? 0 : first_step, (hipStream_t)stream, ema,
                  decay};
  StepStateBlock* state = on_device ? (StepStateBlock*)d.state : nullptr;
  if (d.master) sgd_dispatch<bf16_t, true>(a, state);
  else if (d.dtype == DCTN_F32) sgd_dispatch<float, false>(a, state);
  else sgd_dispatch<bf16_t, false>(a, state);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
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

// The grouped form always takes the 16-byte step block: without a schedule the rate is state->lr, as adam_l2_k's
int dctn_sgd_l2_step_grouped(void* master_or_null, void* params, const void* grads, void* momentum_buf, void* sq_sum,
                             void* state, const void* guard_or_null, const void* schedule_or_null, void* groups,
                             int64_t n, int64_t n_reg, float momentum, float l2, int dtype, void* stream) {
  if (!groups) return DCTN_ERR_NULL;
  const dctn_flat_step_t d = {params, master_or_null, grads, sq_sum, state, guard_or_null, schedule_or_null, groups,
                              n, n_reg, l2, dtype};
  return sgd_step(d, momentum_buf, 0.f, momentum, 0, stream);
}

}  // extern "C"
