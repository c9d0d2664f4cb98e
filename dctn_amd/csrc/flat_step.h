// The one step kernel of the flat optimizers, and its host side.  FlatAdam (adam_score.hip), FlatSGD (train_tail.hip) and
// FlatRMSprop (rmsprop_step.hip) each give it a RULE - what differs between optimizers and nothing else - and get
// flat_step_k<Rule, ...>: one update over ONE flat parameter buffer plus the L2 regulariser, whose value sum w^2 is left
// as one partial sum per workgroup.  DESIGN 4.11i describes the skeleton and the rule interface.
//
// A rule is a struct of
//   Coef          the coefficients, passed by value
//   Segment       what an element's segment decides (the rate, the weight decay, ...; a member `frozen`), and
//   segment()     how a lane of wave 0 forms it from the rate, the segment's count of steps taken and its weight decay
//   elem()        the arithmetic of one element, every product-sum an explicit fmaf: the vector and the scalar form, and
//                 every instantiation, give the same bits whatever the compiler would contract on its own
//   launch_wd()   the weight decay of a launch without a group table
//   THREADS, MAX_BLOCKS, HAS_VEC   the geometry: threads per workgroup, the workgroup cap, whether a vector form exists
//   SECOND        whether there is a second float32 state array beside the first: always, never, or when the launch gives
//                 one (a branch that is uniform over the launch, not a template flag)
//   STATE_ALWAYS  false: packs without a schedule, a table or an average touch no step block - the rate and the first
//                 step are Coef's `lr` and `first_step`, and the launch draws no ticket and issues no atomic
//   skips_state_read()   true for a segment whose elements write the first state array without reading it
// elem() and launch_wd() see the types of the pack, so a rule may have pack members of its own behind the skeleton's
// (SGD's SgdDecay).
#pragma once

#include "common.h"
#include "grad_guard.h"
#include "lr_schedule.h"
#include "param_groups.h"
#include "weight_ema.h"

#include <initializer_list>

enum class SecondState { never, always, if_given };

#if defined(__HIPCC__)
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
// Four elements as they come from memory, not yet looked at: a load whose result is unpacked at once makes the compiler
// wait for it there, and the early loads of flat_step_k must stay in flight across the prologue and the barrier
__device__ __forceinline__ float4 raw4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint2 raw4(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ void unpack4(const float4& t, float (&x)[4]) { x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w; }
__device__ __forceinline__ void unpack4(const uint2& t, float (&x)[4]) {
  x[0] = __uint_as_float(t.x << 16), x[1] = __uint_as_float(t.x & 0xffff0000u);
  x[2] = __uint_as_float(t.y << 16), x[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ unsigned bf16_bits(float x) {
  return __builtin_bit_cast(unsigned short, (bf16_t)x);   // the same round-to-nearest-even cast as the scalar form
}
__device__ __forceinline__ void store4(bf16_t* p, const float (&x)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(bf16_bits(x[0]) | (bf16_bits(x[1]) << 16), bf16_bits(x[2]) | (bf16_bits(x[3]) << 16));
}

// The workgroup's sq_sum slot from its waves' sums.  Each geometry keeps the order it always had - four waves in pairs,
// sixteen one after the other - or the slots change bits.
template <int WAVES> __device__ __forceinline__ float flat_step_slot(const float* red) {
  if constexpr (WAVES == 4) {
    return (red[0] + red[1]) + (red[2] + red[3]);
  } else {
    float total = 0.f;
    for (int j = 0; j < WAVES; ++j) total += red[j];
    return total;
  }
}

// S: the parameters' type.  VEC: four elements per lane and access when every pointer is aligned for it; the tail of n
// and the unaligned case take one element per lane.  MASTER (S = bf16_t): the step runs on the float32 array `wm`, which
// is read and written; `w` gets its rounding and is not read, and `wm`, the state arrays and the sq_sum slots are the
// float instantiation's bits.  Without MASTER `wm` is unused (null).  `s0`, `s1`: the rule's float32 state arrays.
// G, the trailing pack, holds a const GradGuardBlock* (GUARD), a const LrScheduleBlock* (SCHED), a ParamGroupBlock*
// (GROUPED) and a WeightEma by value (EMA), any of them in that order, found by type (step_pack.h), and behind them what
// the rule adds; the headers of the four state the semantics.  One body serves every pack: everything of an option is
// behind `if constexpr`, and a launch without a table is one segment.
//   prologue : wave 0, every lane (the schedule's ballot needs them all).  All loads - steps_done, the rate or the
//              schedule's knot, the lane's segment of the table, the guard's decision, the average's block - are
//              independent of one another and go out together.  A lane then forms its segment's constants - with a table
//              from the segment's own count and ONE rounded product rate * lr_scale, without one lane 0 from steps_done
//              and the rate as it is - and publishes them through LDS.  A pack without any of the four has no prologue
//              and no barrier (STATE_ALWAYS false only).
//   halted   : the whole workgroup returns after the barrier, before any store and before the ticket: steps_done does
//              not advance and a schedule holds its place.  Otherwise every gradient is replaced by ONE rounded float32
//              product g * coef in front of the rule's arithmetic (grad_guard.h); coef == 1 leaves g's bits.
//   elements : without a table every element has the launch's one segment; with one every lane walks a cursor over the
//              segments' ends as its elements increase (param_groups.h).  A vector inside one segment takes the vector
//              path; a frozen one loads nothing but w, below n_reg; a vector that straddles an end is done element by
//              element.  The rule's elem() sees the same values in the same order per lane in every form, so an
//              all-default table leaves the bits of no table, and the vector form those of the scalar form.
//   ticket   : lane 0 stores the workgroup's sq_sum slot (stored, not accumulated: no fill before the kernel, a fixed
//              order) and draws one ticket on the step block; the workgroup that draws the last one writes
//              steps_done + 1, with a schedule the rate used, the segments' counts and the average's count, and resets
//              the ticket.  The ticket orders one thing only: every workgroup's read of the step block and the tables
//              before the last workgroup's write of them.  No data passes between workgroups, so no release / acquire of
//              the parameter stores is needed (the kernel boundary publishes those); the wait makes sure this wave's
//              loads have returned before it draws.  One atomic per workgroup on ONE address serialises at about 12 ns
//              each: hence the 256 workgroups of 1024 threads of the rules that always draw.
template <typename Rule, typename S, bool VEC, bool MASTER, typename... G>
__global__ __launch_bounds__(Rule::THREADS) void flat_step_k(S* __restrict__ w, float* __restrict__ wm,
                                                            const S* __restrict__ g, float* __restrict__ s0,
                                                            float* __restrict__ s1, float* __restrict__ sq_sum,
                                                            StepStateBlock* __restrict__ state, long long n,
                                                            long long n_reg, typename Rule::Coef k, G... pack) {
  using Segment = typename Rule::Segment;
  constexpr bool GUARD = pack_has_v<const GradGuardBlock*, G...>, SCHED = pack_has_v<const LrScheduleBlock*, G...>;
  constexpr bool GROUPED = pack_has_v<ParamGroupBlock*, G...>, EMA = pack_has_v<WeightEma, G...>;
  constexpr bool HAS_STATE = Rule::STATE_ALWAYS || SCHED || GROUPED || EMA;
  constexpr int NSEG = GROUPED ? DCTN_PG_MAX_SEGMENTS : 1, WAVES = Rule::THREADS / 64;
  static_assert(!VEC || Rule::HAS_VEC, "this rule has no vector form");
  __shared__ float red[WAVES];
  __shared__ float published[3];   // halted, coef, the average's weight
  __shared__ long long seg_end[NSEG];
  __shared__ Segment seg[NSEG];
  __shared__ int seg_count;
  [[maybe_unused]] WeightEma ema{nullptr, nullptr};
  if constexpr (EMA) ema = pack_get<WeightEma>(pack...);
  [[maybe_unused]] ParamGroupBlock* groups = nullptr;
  if constexpr (GROUPED) groups = pack_get<ParamGroupBlock*>(pack...);
  const bool has1 = Rule::SECOND == SecondState::always || (Rule::SECOND == SecondState::if_given && s1 != nullptr);
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
  const long long n_vec = VEC ? (n & ~3LL) : 0;
  // EARLY (the vector form without a table): every lane issues the loads of its first trip HERE, in front of the prologue
  // and the barrier.  None of them depends on the rate, the guard's decision or the average's weight, so the prologue's
  // round trip and the barrier pass while they are in flight; a plain load survives __syncthreads().  A halted launch
  // has then read its gradients and stores nothing, as before.  (With a table a frozen segment's gradient must not be
  // read, and which segments are frozen is only known behind the barrier.)
  constexpr bool EARLY = VEC && !GROUPED;
  using RawS = decltype(raw4((const S*)nullptr));
  [[maybe_unused]] std::conditional_t<MASTER, float4, RawS> rw;
  [[maybe_unused]] RawS rg;
  [[maybe_unused]] float4 ra, rb, re;   // rb: loaded, and looked at, only with a second state array
  [[maybe_unused]] bool early = false;
  if constexpr (EARLY) {
    const long long i = tid * 4;
    if (i < n_vec) {
      early = true;
      if constexpr (MASTER) rw = raw4(wm + i); else rw = raw4(w + i);
      rg = raw4(g + i), ra = raw4(s0 + i);
      if (has1) rb = raw4(s1 + i);
      if constexpr (EMA) re = raw4(ema.values + i);
    }
  }
  int steps_done = 0;
  float rate = 0.f;
  [[maybe_unused]] int my_steps = 0;
  [[maybe_unused]] bool my_live = false;             // wave 0: this lane's segment is in use and not frozen
  [[maybe_unused]] WeightEmaLane ema_lane{0, 0.f};   // lane 0
  float coef = 1.f;
  [[maybe_unused]] float omd = 0.f;
  Segment sg;
  if constexpr (HAS_STATE || GUARD) {
    if (threadIdx.x < 64) {   // wave 0, every lane
      const int lane = threadIdx.x;
      [[maybe_unused]] ParamGroupLane tl{};
      if constexpr (GROUPED) tl = param_group_lane_load(groups, lane);
      if constexpr (EMA) {
        if (lane == 0) published[2] = (ema_lane = weight_ema_lane_load(ema.block)).omd;
      }
      if constexpr (SCHED) {
        const LrScheduleLane knot = lr_schedule_lane_load(pack_get<const LrScheduleBlock*>(pack...), lane);
        steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rate = lr_schedule_wave_value(knot, lane, steps_done);
      } else if constexpr (HAS_STATE) {
        steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rate = __hip_atomic_load(&state->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        steps_done = k.first_step ? 0 : 1, rate = k.lr;
      }
      if constexpr (GUARD) {
        if (lane == 0) {
          const GradGuardBlock* guard = pack_get<const GradGuardBlock*>(pack...);
          published[0] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
          published[1] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if constexpr (GROUPED) {
        my_steps = tl.steps;
        my_live = lane < tl.n_segments && (tl.flags & DCTN_PG_FROZEN) == 0u;
        seg_end[lane] = tl.end;
        seg[lane] = Rule::segment(k, __fmul_rn(rate, tl.lr_scale), tl.steps, tl.weight_decay,
                                  (tl.flags & DCTN_PG_FROZEN) != 0u);
        if (lane == 0) seg_count = tl.n_segments;
      } else {
        if (lane == 0) seg[0] = Rule::segment(k, rate, steps_done, Rule::launch_wd(k, pack...), false);
      }
    }
    __syncthreads();
    if constexpr (GUARD) {
      if (published[0] != 0.f) return;   // the whole workgroup, before any store and before the ticket
      coef = published[1];
    }
    if constexpr (EMA) omd = published[2];
    sg = seg[0];
  } else {   // no step block and no guard: the launch's arguments are all there is
    sg = Rule::segment(k, k.lr, k.first_step ? 0 : 1, Rule::launch_wd(k, pack...), false);
  }
  [[maybe_unused]] float* __restrict__ em = nullptr;
  if constexpr (EMA) em = ema.values;
  [[maybe_unused]] int n_seg = 1;
  [[maybe_unused]] ParamGroupCursor cur{0, 0x7fffffffffffffffLL};
  if constexpr (GROUPED) {
    n_seg = seg_count;
    cur.end = param_group_end(seg_end, 0, n_seg);
  }
  auto follow = [&](long long i) {
    if constexpr (GROUPED) {
      if (param_group_advance(cur, i, seg_end, n_seg)) sg = seg[cur.seg];
    }
  };
  float part = 0.f;
  // one element with its own loads and stores: the scalar form, the tail, and a vector that straddles a segment's end
  auto one = [&](long long i) {
    const bool reg = i < n_reg;
    if (GROUPED && sg.frozen) {   // only the regulariser's value: no gradient read, no store
      if (reg) {
        const float wi = MASTER ? wm[i] : (float)w[i];
        part = fmaf(wi, wi, part);
      }
      return;
    }
    float a = Rule::skips_state_read(sg) ? 0.f : s0[i], b = has1 ? s1[i] : 0.f;
    const float wi = Rule::template elem<G...>(MASTER ? wm[i] : (float)w[i], clipped<GUARD>((float)g[i], coef), a, b, has1,
                                               reg, k, sg, part);
    w[i] = (S)wi;
    if (MASTER) wm[i] = wi;
    s0[i] = a;
    if (has1) s1[i] = b;
    if constexpr (EMA) em[i] = weight_ema_elem(em[i], weight_ema_kept<S, MASTER>(wi), omd);
  };
  // four elements of one segment whose values are in registers: the clip, the step, the stores
  auto vec_step = [&](long long i, float (&wi)[4], float (&gi)[4], float (&ai)[4], float (&bi)[4], float (&ei)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) gi[e] = clipped<GUARD>(gi[e], coef);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      wi[e] = Rule::template elem<G...>(wi[e], gi[e], ai[e], bi[e], has1, i + e < n_reg, k, sg, part);
    store4(s0 + i, ai);
    if (has1) store4(s1 + i, bi);
    store4(w + i, wi);
    if (MASTER) store4(wm + i, wi);
    if constexpr (EMA) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ei[e] = weight_ema_elem(ei[e], weight_ema_kept<S, MASTER>(wi[e]), omd);
      store4(em + i, ei);
    }
  };
  if constexpr (VEC) {
    long long i = tid * 4;
    if constexpr (EARLY) {
      if (early) {   // the first trip, loaded above the barrier
        float wi[4], gi[4], ai[4], bi[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float ei[4];
        unpack4(rw, wi), unpack4(rg, gi), unpack4(ra, ai);
        if (has1) unpack4(rb, bi);
        if constexpr (EMA) unpack4(re, ei);
        vec_step(i, wi, gi, ai, bi, ei);
        i += nthr * 4;
      }
    }
    for (; i < n_vec; i += nthr * 4) {
      follow(i);
      if (!GROUPED || i + 3 < cur.end) {   // the four elements share a segment
        if (GROUPED && sg.frozen) {
          if (i < n_reg) {
            float wi[4];
            if (MASTER) load4(wm + i, wi); else load4(w + i, wi);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (i + e < n_reg) part = fmaf(wi[e], wi[e], part);
          }
          continue;
        }
        float wi[4], gi[4], ai[4], bi[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float ei[4];
        if (MASTER) load4(wm + i, wi); else load4(w + i, wi);
        load4(g + i, gi), load4(s0 + i, ai);
        if (has1) load4(s1 + i, bi);
        if constexpr (EMA) load4(em + i, ei);
        vec_step(i, wi, gi, ai, bi, ei);
      } else {   // an end inside the vector: element by element, each with its own segment's constants and stores
        for (int e = 0; e < 4; ++e) {
          follow(i + e);
          one(i + e);
        }
      }
    }
  }
  for (long long i = n_vec + tid; i < n; i += nthr) {
    follow(i);
    one(i);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if constexpr (!HAS_STATE) {   // the caller adds the slots when it wants the regulariser's value
    if (threadIdx.x == 0 && sq_sum) sq_sum[blockIdx.x] = flat_step_slot<WAVES>(red);
  } else if (threadIdx.x < 64) {   // wave 0: lane 0 draws the ticket, every lane hears the answer
    unsigned drawn = 0u;
    if (threadIdx.x == 0) {
      if (sq_sum) sq_sum[blockIdx.x] = flat_step_slot<WAVES>(red);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      drawn = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    drawn = __shfl(drawn, 0, 64);
    if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
      if constexpr (GROUPED) {
        if (my_live) groups->steps[threadIdx.x] = my_steps + 1;
      }
      if (threadIdx.x == 0) {
        state->steps_done = steps_done + 1;
        if constexpr (SCHED) state->lr = rate;   // the GLOBAL rate of this step, before any segment's scale
        if constexpr (EMA) weight_ema_advance(ema.block, ema_lane);
        state->ticket = 0u;
      }
    }
  }
}
#endif   // __HIPCC__

// One workgroup per access of every lane, up to the rule's cap
template <typename Rule> unsigned flat_step_blocks_for(long long n) {
  constexpr long long per = (long long)Rule::THREADS * (Rule::HAS_VEC ? 4 : 1);
  long long b = (n + per - 1) / per;
  if (b > Rule::MAX_BLOCKS) b = Rule::MAX_BLOCKS;
  return (unsigned)(b < 1 ? 1 : b);
}

// One step as the host sees it: the descriptor (include/dctn_amd.h), the rule's state arrays and coefficients
template <typename Rule> struct FlatStepLaunch {
  const dctn_flat_step_t& d;
  void *s0, *s1;                  // s1: null where the rule or the launch has no second array
  typename Rule::Coef k;
  hipStream_t st;
  const dctn_weight_ema_t* ema;   // null: no average
};

// What every entry point answers first: a null pointer (`required`: the rule's own, the step block where it is needed),
// then the shape.  The caller's own checks follow, and flat_step_run's dtype check is the last
inline int flat_step_check(const dctn_flat_step_t& d, const dctn_weight_ema_t* ema, std::initializer_list<const void*> required) {
  bool missing = !d.params || !d.grads || (ema && (!ema->ema || !ema->block));
  for (const void* p : required) missing = missing || !p;
  if (missing) return DCTN_ERR_NULL;
  if (d.n < 1 || d.n_reg < 0 || d.n_reg > d.n) return DCTN_ERR_BAD_SHAPE;
  return DCTN_OK;
}

#if defined(__HIPCC__)
// The one launcher, for every pack: the vector or the scalar kernel by alignment
template <typename Rule, typename S, bool MASTER, typename... G> void flat_step_launch(const FlatStepLaunch<Rule>& a, G... pack) {
  const dctn_flat_step_t& d = a.d;
  auto kernel = flat_step_k<Rule, S, false, MASTER, G...>;
  if constexpr (Rule::HAS_VEC) {
    const bool vec = ((uintptr_t)d.params | (uintptr_t)d.grads) % (4 * sizeof(S)) == 0 &&
                     ((uintptr_t)a.s0 | (uintptr_t)a.s1 | (uintptr_t)d.master | (uintptr_t)(a.ema ? a.ema->ema : nullptr)) % 16 == 0;
    if (vec) kernel = flat_step_k<Rule, S, true, MASTER, G...>;
  }
  hipLaunchKernelGGL(kernel, dim3(flat_step_blocks_for<Rule>(d.n)), dim3(Rule::THREADS), 0, a.st, (S*)d.params,
                     (float*)d.master, (const S*)d.grads, (float*)a.s0, (float*)a.s1, (float*)d.sq_sum,
                     (StepStateBlock*)d.state, (long long)d.n, (long long)d.n_reg, a.k, pack...);
}

// The pack is the optional blocks the step has, in the order flat_step_k names them: guard, schedule, group table, the
// average (a pair by value) behind them, and last what the rule adds (`own`, by value)
template <typename Rule, typename S, bool MASTER, typename... X> void flat_step_dispatch(const FlatStepLaunch<Rule>& a, X... own) {
  with_blocks([&](auto... pack) {
    if (a.ema) flat_step_launch<Rule, S, MASTER>(a, pack..., WeightEma{(float*)a.ema->ema, (WeightEmaBlock*)a.ema->block}, own...);
    else flat_step_launch<Rule, S, MASTER>(a, pack..., own...);
  }, (const GradGuardBlock*)a.d.guard, (const LrScheduleBlock*)a.d.schedule, (ParamGroupBlock*)a.d.groups);
}

// The last check, and the launch: a master copy goes with bf16 parameters
template <typename Rule, typename... X> int flat_step_run(const FlatStepLaunch<Rule>& a, X... own) {
  const dctn_flat_step_t& d = a.d;
  if ((d.dtype != DCTN_F32 && d.dtype != DCTN_BF16) || (d.master && d.dtype != DCTN_BF16)) return DCTN_ERR_BAD_DTYPE;
  if (d.master) flat_step_dispatch<Rule, bf16_t, true>(a, own...);
  else if (d.dtype == DCTN_F32) flat_step_dispatch<Rule, float, false>(a, own...);
  else flat_step_dispatch<Rule, bf16_t, false>(a, own...);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}
#endif
