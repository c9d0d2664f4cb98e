// The reference's documented recipe trains with Adam (new_runner.py:496-498: Adam(model.parameters(), lr, weight_decay))
// and scores with cross-entropy + accuracy per batch (dctn/evaluation.py:7-22).  Two kernels beside train_tail.hip's:
//   adam_l2_k  : torch.optim.Adam (coupled weight decay) + the L2 regulariser over ONE flat parameter buffer, like
//                sgd_l2_k.  The step count t and the learning rate are read from a 16-byte device block, and the
//                launch itself advances t: a captured graph replays the same node and still gets t, t+1, t+2, ...
//                MASTER form (bf16 parameters): the step runs on a float32 master copy, which is read and written;
//                the bf16 cell only receives the rounded result and is never read.
//   ce_score_k : adds one batch's {sum of cross-entropies, correct rows, rows} to three float64 values
#include "common.h"
#include "grad_guard.h"
#include "lr_schedule.h"
#include "param_groups.h"
#include "weight_ema.h"

#include <cmath>

namespace {

constexpr long long DCTN_CE_IGNORE = -100;   // torch.nn.functional.cross_entropy's default ignore_index

// (not merged with lr_schedule.h's StepStateBlock: the type is in the mangled name of every adam_l2_k instantiation)
struct AdamState {   // include/dctn_amd.h documents this layout: it is part of the ABI
  int steps_done;
  float lr;
  unsigned ticket;
  unsigned reserved;
};

struct AdamCoef {
  double ln_b1, ln_b2;        // ln(beta): 1 - beta^t = -expm1(t * ln beta), formed in the kernel from t
  float b1, omb1, b2, omb2;   // beta, 1 - beta (formed in double on the host, then rounded once)
  float eps, wd, two_l2;
};

// The arithmetic of one element; every product-sum is an explicit fmaf so that the vector and the scalar form of the
// kernel (and any later instantiation) produce the same bits whatever the compiler would contract on its own
__device__ __forceinline__ float adam_elem(float wi, float gi, float& m, float& v, bool reg, const AdamCoef& k,
                                           float step, float bc2_sqrt, float& part) {
  gi = fmaf(k.wd, wi, gi);
  if (reg) {
    gi = fmaf(k.two_l2, wi, gi);
    part = fmaf(wi, wi, part);
  }
  m = fmaf(k.b1, m, k.omb1 * gi);
  v = fmaf(k.b2, v, (k.omb2 * gi) * gi);
  const float denom = sqrtf(v) / bc2_sqrt + k.eps;
  return fmaf(-step, m / denom, wi);
}

__device__ __forceinline__ void load4(const float* p, float (&x)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
}
__device__ __forceinline__ void store4(float* p, const float (&x)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
}
__device__ __forceinline__ void load4(const bf16_t* p, float (&x)[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);   // bf16 -> f32 is the upper half of the word
  x[0] = __uint_as_float(t.x << 16), x[1] = __uint_as_float(t.x & 0xffff0000u);
  x[2] = __uint_as_float(t.y << 16), x[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ unsigned bf16_bits(float x) {
  return __builtin_bit_cast(unsigned short, (bf16_t)x);   // the same round-to-nearest-even cast as the scalar form
}
__device__ __forceinline__ void store4(bf16_t* p, const float (&x)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(bf16_bits(x[0]) | (bf16_bits(x[1]) << 16), bf16_bits(x[2]) | (bf16_bits(x[3]) << 16));
}

// VEC: four elements per lane and access (16 bytes of exp_avg / exp_avg_sq, 16 or 8 of the parameters) when every
// pointer is aligned for it; the tail of n and the unaligned case take one element per lane.
// MASTER (S = bf16_t): the weight comes from and goes back to the float32 array `wm`; `w` gets its bf16 rounding and is
// not read.  adam_elem sees the same float32 values in the same order as the float instantiation does, so `wm`, the
// moments and the sq_sum slots are that instantiation's bits.  Without MASTER `wm` is unused (null).
// Workgroups of 1024 threads, at most 256 of them: the ticket at the end is one atomic per workgroup on ONE address,
// and those serialise at about 12 ns each (measured: 1024 workgroups of 256 threads took 17.7 us over 1.9 M
// parameters where the same stream without a ticket, sgd_l2_k, takes 5.7 us).
// GUARD: the step obeys a gradient guard's decision (grad_guard.hip, launched in front of this kernel).  Lane 0 of every
// workgroup reads `halted` and `coef` from the guard block before anything else.  Halted: the workgroup returns at once
// - it writes no parameter, master value, moment or sq_sum slot and draws no ticket, so steps_done does not advance.
// Otherwise every gradient is replaced by ONE rounded float32 product g * coef (a bf16 gradient is widened first and
// not rounded back) in front of adam_elem: the clip applies to the gradient as it stands in the buffer, and weight
// decay and the 2 * l2 * w term come after it.  coef == 1 leaves g's bits, so an unclipped guarded step is the
// unguarded one.  The guard block is a trailing parameter PACK, empty in the unguarded instantiations, and everything
// else of it is behind `if constexpr`: those compile to what they did.
// SCHED (the pack also holds a const LrScheduleBlock*): the rate is not read from state->lr but evaluated from the
// schedule block at step steps_done (lr_schedule.h).  Wave 0 loads the table, one knot per lane, together with
// steps_done - no load of it depends on another, so the table adds no memory round trip in front of the element loop -
// finds the segment with a ballot, and lane 0 publishes step and bc2_sqrt as in the other forms.  The workgroup that
// draws the last ticket writes the rate it used to state->lr beside steps_done: the block reports the rate of the step
// just taken.  A halted guarded step returns before the ticket, so the schedule holds its place with steps_done.
// GROUPED (the pack ends with a ParamGroupBlock*): the launch obeys a parameter-group table (param_groups.h states the
// semantics).  Wave 0 loads the table, one segment per lane, beside steps_done and the rate - no load depends on
// another - and every lane forms ITS segment's step size and second correction from the segment's own count, in the
// float64 expressions of the ungrouped kernel's lane 0, and publishes them with the segment's end, weight decay and
// frozen flag through LDS.  Every lane of the workgroup then walks a cursor over the ends as its elements increase.  A
// vector of four elements that lies inside one segment takes the vector path with that segment's constants (nothing is
// loaded but w for a frozen one, and only below n_reg); a vector that straddles an end is done element by element,
// each with its own segment's constants and its own stores.  adam_elem sees the values the ungrouped kernel would give
// it, in the same order per lane, so with an all-default table every buffer and sq_sum slot holds the ungrouped bits.
struct AdamSegment {
  float step, bc2_sqrt, wd;
  bool frozen;
};

template <typename S, bool MASTER, bool GUARD, bool EMA>
__device__ __forceinline__ void adam_grouped_elem(long long i, S* __restrict__ w, float* __restrict__ wm,
                                                  const S* __restrict__ g, float* __restrict__ ea,
                                                  float* __restrict__ eas, bool reg, const AdamCoef& k,
                                                  const AdamSegment& sg, float coef, float& part,
                                                  float* __restrict__ em, float omd) {
  if (sg.frozen) {   // only the regulariser's value: no gradient read, no store
    if (reg) {
      const float wi = MASTER ? wm[i] : (float)w[i];
      part = fmaf(wi, wi, part);
    }
    return;
  }
  AdamCoef ks = k;
  ks.wd = sg.wd;
  float m = ea[i], v = eas[i];
  const float wi = adam_elem(MASTER ? wm[i] : (float)w[i], clipped<GUARD>((float)g[i], coef), m, v, reg, ks, sg.step,
                             sg.bc2_sqrt, part);
  w[i] = (S)wi;
  if (MASTER) wm[i] = wi;
  ea[i] = m, eas[i] = v;
  if constexpr (EMA) em[i] = weight_ema_elem(em[i], weight_ema_kept<S, MASTER>(wi), omd);
}

template <typename S, bool VEC, bool MASTER, bool GUARD, bool SCHED, bool EMA>
__device__ __forceinline__ void adam_grouped_body(S* __restrict__ w, float* __restrict__ wm, const S* __restrict__ g,
                                                  float* __restrict__ ea, float* __restrict__ eas,
                                                  float* __restrict__ sq_sum, AdamState* __restrict__ state, long long n,
                                                  long long n_reg, const AdamCoef& k, const GradGuardBlock* guard,
                                                  const LrScheduleBlock* sched, ParamGroupBlock* groups,
                                                  WeightEma ema) {
  __shared__ float red[16];
  __shared__ float decision[EMA ? 3 : 2];             // halted, coef; EMA: the launch's weight
  __shared__ long long seg_end[DCTN_PG_MAX_SEGMENTS];
  __shared__ float seg_step[DCTN_PG_MAX_SEGMENTS], seg_bc2[DCTN_PG_MAX_SEGMENTS], seg_wd[DCTN_PG_MAX_SEGMENTS];
  __shared__ int seg_frozen[DCTN_PG_MAX_SEGMENTS];
  __shared__ int seg_count;
  int t = 0, my_steps = 0;
  float lr = 0.f;
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
      t = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
      lr = lr_schedule_wave_value(knot, lane, t - 1);
    } else {
      t = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
      lr = __hip_atomic_load(&state->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (GUARD) {
      if (lane == 0) {
        decision[0] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
        decision[1] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // the segment's rate: one rounded product; its corrections from ITS count, as lane 0 of the ungrouped kernel
    const float rate = __fmul_rn(lr, sg.lr_scale);
    const int ts = sg.steps + 1;
    my_steps = sg.steps;
    my_live = lane < sg.n_segments && (sg.flags & DCTN_PG_FROZEN) == 0u;
    seg_end[lane] = sg.end;
    seg_step[lane] = (float)((double)rate / -expm1((double)ts * k.ln_b1));
    seg_bc2[lane] = (float)sqrt(-expm1((double)ts * k.ln_b2));
    seg_wd[lane] = sg.weight_decay;
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
  AdamSegment sg{seg_step[0], seg_bc2[0], seg_wd[0], seg_frozen[0] != 0};
  auto follow = [&](ParamGroupCursor& c, AdamSegment& s, long long i) {
    if (param_group_advance(c, i, seg_end, n_seg))
      s = AdamSegment{seg_step[c.seg], seg_bc2[c.seg], seg_wd[c.seg], seg_frozen[c.seg] != 0};
  };
  float part = 0.f;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
  const long long n_vec = VEC ? (n & ~3LL) : 0;
  if (VEC) {
    for (long long i = tid * 4; i < n_vec; i += nthr * 4) {
      follow(cur, sg, i);
      if (i + 3 < cur.end) {   // the four elements share a segment
        if (sg.frozen) {
          if (i < n_reg) {
            float wi[4];
            if (MASTER) load4(wm + i, wi); else load4(w + i, wi);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (i + e < n_reg) part = fmaf(wi[e], wi[e], part);
          }
          continue;
        }
        AdamCoef ks = k;
        ks.wd = sg.wd;
        float wi[4], gi[4], mi[4], vi[4];
        [[maybe_unused]] float ei[4];
        if (MASTER) load4(wm + i, wi); else load4(w + i, wi);
        load4(g + i, gi), load4(ea + i, mi), load4(eas + i, vi);
        if constexpr (EMA) load4(em + i, ei);
#pragma unroll
        for (int e = 0; e < 4; ++e) gi[e] = clipped<GUARD>(gi[e], coef);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          wi[e] = adam_elem(wi[e], gi[e], mi[e], vi[e], i + e < n_reg, ks, sg.step, sg.bc2_sqrt, part);
        store4(ea + i, mi), store4(eas + i, vi), store4(w + i, wi);
        if (MASTER) store4(wm + i, wi);
        if constexpr (EMA) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ei[e] = weight_ema_elem(ei[e], weight_ema_kept<S, MASTER>(wi[e]), omd);
          store4(em + i, ei);
        }
      } else {   // an end inside the vector: element by element, each with its own segment's constants and stores
        for (int e = 0; e < 4; ++e) {
          follow(cur, sg, i + e);
          adam_grouped_elem<S, MASTER, GUARD, EMA>(i + e, w, wm, g, ea, eas, i + e < n_reg, k, sg, coef, part, em, omd);
        }
      }
    }
  }
  for (long long i = n_vec + tid; i < n; i += nthr) {
    follow(cur, sg, i);
    adam_grouped_elem<S, MASTER, GUARD, EMA>(i, w, wm, g, ea, eas, i < n_reg, k, sg, coef, part, em, omd);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x < 64) {   // wave 0: lane 0 draws the ticket, every lane hears the answer
    unsigned drawn = 0u;
    if (threadIdx.x == 0) {
      float total = 0.f;
      for (int j = 0; j < 16; ++j) total += red[j];
      if (sq_sum) sq_sum[blockIdx.x] = total;
      // the ticket of the ungrouped kernel; the wait covers this wave's loads of steps_done, the rate and the table
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      drawn = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    drawn = __shfl(drawn, 0, 64);
    if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
      if (my_live) groups->steps[threadIdx.x] = my_steps + 1;
      if (threadIdx.x == 0) {
        state->steps_done = t;
        if constexpr (SCHED) state->lr = lr;   // the GLOBAL rate of this step, before any segment's scale
        if constexpr (EMA) weight_ema_advance(ema.block, ema_lane);
        state->ticket = 0u;
      }
    }
  }
}

template <typename S, bool VEC, bool MASTER, typename... G>
__global__ __launch_bounds__(1024) void adam_l2_k(S* __restrict__ w, float* __restrict__ wm, const S* __restrict__ g,
                                                 float* __restrict__ ea, float* __restrict__ eas,
                                                 float* __restrict__ sq_sum, AdamState* __restrict__ state, long long n,
                                                 long long n_reg, AdamCoef k, G... guard_block) {
  // G holds a const GradGuardBlock* (GUARD), a const LrScheduleBlock* (SCHED), a ParamGroupBlock* (GROUPED), any of them
  // in that order, or nothing: the plain kernel, parameter for parameter
  // and behind them a WeightEma (EMA, weight_ema.h): the average's values and block
  constexpr bool GUARD = pack_has_v<const GradGuardBlock*, G...>, SCHED = pack_has_v<const LrScheduleBlock*, G...>;
  constexpr bool EMA = pack_has_v<WeightEma, G...>;
  [[maybe_unused]] WeightEma ema{nullptr, nullptr};
  if constexpr (EMA) ema = pack_get<WeightEma>(guard_block...);
  if constexpr (pack_has_v<ParamGroupBlock*, G...>) {   // GROUPED: a body of its own; the rest of this one is untouched
    const GradGuardBlock* guard = nullptr;
    const LrScheduleBlock* sched = nullptr;
    if constexpr (GUARD) guard = pack_get<const GradGuardBlock*>(guard_block...);
    if constexpr (SCHED) sched = pack_get<const LrScheduleBlock*>(guard_block...);
    adam_grouped_body<S, VEC, MASTER, GUARD, SCHED, EMA>(w, wm, g, ea, eas, sq_sum, state, n, n_reg, k, guard, sched,
                                                         pack_get<ParamGroupBlock*>(guard_block...), ema);
    return;
  }
  __shared__ float red[16];
  constexpr int OMD = GUARD ? 4 : 2;   // EMA: the launch's weight, behind the other published values
  __shared__ float scale[OMD + (EMA ? 1 : 0)];
  [[maybe_unused]] WeightEmaLane ema_lane{0, 0.f};   // thread 0
  if constexpr (GUARD) {
    if (threadIdx.x == 0) {
      const GradGuardBlock* guard = pack_get<const GradGuardBlock*>(guard_block...);
      scale[2] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
      scale[3] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // lane 0 of every workgroup reads the step count and the learning rate BEFORE it takes the workgroup's ticket below;
  // the one write of the launch to steps_done happens after the last ticket is drawn, so no workgroup can see the new
  // value
  int t = 0;
  float lr = 0.f;
  if constexpr (SCHED) {
    if (threadIdx.x < 64) {   // wave 0, every lane: the ballot needs them all
      const LrScheduleLane knot = lr_schedule_lane_load(pack_get<const LrScheduleBlock*>(guard_block...), threadIdx.x);
      t = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
      lr = lr_schedule_wave_value(knot, threadIdx.x, t - 1);
    }
  }
  if (threadIdx.x == 0) {
    if constexpr (!SCHED) {
      t = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
      lr = __hip_atomic_load(&state->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (EMA) scale[OMD] = (ema_lane = weight_ema_lane_load(ema.block)).omd;
    // The two bias corrections in float64, once per workgroup, rounded once - what torch's host arithmetic gives.  In
    // float32 the difference 1 - beta2^t cancels: at t = 1 it is 0.001 with the absolute error of 0.999, a relative
    // 6e-5 in every update of the first steps.  (From t itself, not as running products, which drift.)
    scale[0] = (float)((double)lr / -expm1((double)t * k.ln_b1));
    scale[1] = (float)sqrt(-expm1((double)t * k.ln_b2));
  }
  __syncthreads();
  const float step = scale[0], bc2_sqrt = scale[1];
  float coef = 1.f;
  if constexpr (GUARD) {
    if (scale[2] != 0.f) return;   // the whole workgroup, before any store and before the ticket
    coef = scale[3];
  }
  [[maybe_unused]] float omd = 0.f;
  [[maybe_unused]] float* __restrict__ em = nullptr;
  if constexpr (EMA) omd = scale[OMD], em = ema.values;
  float part = 0.f;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
  const long long n_vec = VEC ? (n & ~3LL) : 0;
  if (VEC) {
    for (long long i = tid * 4; i < n_vec; i += nthr * 4) {
      float wi[4], gi[4], mi[4], vi[4];
      [[maybe_unused]] float ei[4];
      if (MASTER) load4(wm + i, wi); else load4(w + i, wi);
      load4(g + i, gi), load4(ea + i, mi), load4(eas + i, vi);
      if constexpr (EMA) load4(em + i, ei);
#pragma unroll
      for (int e = 0; e < 4; ++e) gi[e] = clipped<GUARD>(gi[e], coef);
#pragma unroll
      for (int e = 0; e < 4; ++e) wi[e] = adam_elem(wi[e], gi[e], mi[e], vi[e], i + e < n_reg, k, step, bc2_sqrt, part);
      store4(ea + i, mi), store4(eas + i, vi), store4(w + i, wi);
      if (MASTER) store4(wm + i, wi);
      if constexpr (EMA) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ei[e] = weight_ema_elem(ei[e], weight_ema_kept<S, MASTER>(wi[e]), omd);
        store4(em + i, ei);
      }
    }
  }
  for (long long i = n_vec + tid; i < n; i += nthr) {
    float m = ea[i], v = eas[i];
    const float wi = adam_elem(MASTER ? wm[i] : (float)w[i], clipped<GUARD>((float)g[i], coef), m, v, i < n_reg, k, step,
                               bc2_sqrt, part);
    w[i] = (S)wi;
    if (MASTER) wm[i] = wi;
    ea[i] = m, eas[i] = v;
    if constexpr (EMA) em[i] = weight_ema_elem(em[i], weight_ema_kept<S, MASTER>(wi), omd);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    // one slot per workgroup, stored (not accumulated), as sgd_l2_k
    float total = 0.f;
    for (int j = 0; j < 16; ++j) total += red[j];
    if (sq_sum) sq_sum[blockIdx.x] = total;
    // The ticket.  It orders one thing only: every workgroup's read of steps_done before the last workgroup's write of
    // it.  No data passes between workgroups, so no release / acquire of the parameter stores is needed (the kernel
    // boundary publishes those); the wait makes sure this lane's two state loads have returned before the ticket is
    // drawn, and the writer below acts on the value its own ticket returned.
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
      state->steps_done = t;
      if constexpr (SCHED) state->lr = lr;   // the rate this step used (no workgroup of a scheduled launch reads it)
      if constexpr (EMA) weight_ema_advance(ema.block, ema_lane);
      state->ticket = 0u;
    }
  }
}

unsigned adam_blocks_for(long long n) {   // one vector access of every lane per workgroup, up to one workgroup per CU
  long long b = (n + 4095) / 4096;
  if (b > 256) b = 256;
  return (unsigned)(b < 1 ? 1 : b);
}

// One step as the host sees it: the descriptor (include/dctn_amd.h) and what only Adam has
struct AdamStep {
  const dctn_flat_step_t& d;
  void *exp_avg, *exp_avg_sq;
  AdamCoef k;
  hipStream_t st;
  const dctn_weight_ema_t* ema;   // null: no average
};

// The one launcher, for every pack: the vector or the scalar kernel by alignment
template <typename S, bool MASTER, typename... G> void adam_launch(const AdamStep& a, G... pack) {
  const dctn_flat_step_t& d = a.d;
  const size_t esz = sizeof(S);
  const bool vec = ((uintptr_t)d.params | (uintptr_t)d.grads) % (4 * esz) == 0 &&
                   ((uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq | (uintptr_t)d.master | (uintptr_t)(a.ema ? a.ema->ema : nullptr)) % 16 == 0;
  const auto kernel = vec ? adam_l2_k<S, true, MASTER, G...> : adam_l2_k<S, false, MASTER, G...>;
  hipLaunchKernelGGL(kernel, dim3(adam_blocks_for(d.n)), dim3(1024), 0, a.st, (S*)d.params, (float*)d.master,
                     (const S*)d.grads, (float*)a.exp_avg, (float*)a.exp_avg_sq, (float*)d.sq_sum, (AdamState*)d.state,
                     (long long)d.n, (long long)d.n_reg, a.k, pack...);
}

// The pack is the optional blocks the step has, in the order adam_l2_k expects: guard, schedule, group table, and the
// average (a pair by value) behind them
template <typename S, bool MASTER> void adam_dispatch(const AdamStep& a) {
  with_blocks([&](auto... pack) {
    if (a.ema) adam_launch<S, MASTER>(a, pack..., WeightEma{(float*)a.ema->ema, (WeightEmaBlock*)a.ema->block});
    else adam_launch<S, MASTER>(a, pack...);
  }, (const GradGuardBlock*)a.d.guard, (const LrScheduleBlock*)a.d.schedule, (ParamGroupBlock*)a.d.groups);
}

// Validates and launches.  master_first: the _scheduled / _grouped entry points answer a master copy beside a dtype
// that is not bf16 in front of every other check; everywhere else it is part of the dtype check, the last one
int adam_step(const dctn_flat_step_t& d, void* exp_avg, void* exp_avg_sq, double beta1, double beta2, float eps,
              float weight_decay, void* stream, bool master_first = false, const dctn_weight_ema_t* ema = nullptr) {
  const bool master_dtype = d.master && d.dtype != DCTN_BF16;   // a master copy goes with bf16 parameters
  if (master_first && master_dtype) return DCTN_ERR_BAD_DTYPE;
  if (!d.params || !d.grads || !exp_avg || !exp_avg_sq || !d.state) return DCTN_ERR_NULL;
  if (ema && (!ema->ema || !ema->block)) return DCTN_ERR_NULL;
  if (d.n < 1 || d.n_reg < 0 || d.n_reg > d.n) return DCTN_ERR_BAD_SHAPE;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return DCTN_ERR_BAD_SHAPE;   // torch raises ValueError
  if ((d.dtype != DCTN_F32 && d.dtype != DCTN_BF16) || master_dtype) return DCTN_ERR_BAD_DTYPE;
  AdamCoef k;
  k.b1 = (float)beta1, k.omb1 = (float)(1.0 - beta1), k.b2 = (float)beta2, k.omb2 = (float)(1.0 - beta2);
  k.ln_b1 = std::log(beta1), k.ln_b2 = std::log(beta2);   // beta = 0: -inf, and 1 - beta^t = -expm1(-inf) = 1
  k.eps = eps, k.wd = d.groups ? 0.f : weight_decay, k.two_l2 = 2.f * d.l2;   // a table carries every segment's decay
  const AdamStep a{d, exp_avg, exp_avg_sq, k, (hipStream_t)stream, ema};
  if (d.master) adam_dispatch<bf16_t, true>(a);
  else if (d.dtype == DCTN_F32) adam_dispatch<float, false>(a);
  else adam_dispatch<bf16_t, false>(a);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
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

size_t dctn_adam_state_bytes(void) { return sizeof(AdamState); }

size_t dctn_flat_step_bytes(void) { return sizeof(dctn_flat_step_t); }

int dctn_adam_l2_num_partials(int64_t n) { return n < 1 ? 0 : (int)adam_blocks_for(n); }

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
