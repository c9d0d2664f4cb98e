// The reference's ConvSBS classifier trains with RMSprop (mnist.py:466-476: RMSprop(lr, alpha, momentum, weight_decay)).
//   rmsprop_l2_k : torch.optim.RMSprop (coupled weight decay, optional momentum, not centered) + the L2 regulariser over
//                  ONE flat parameter buffer: adam_l2_k's geometry, access forms and step-block protocol (adam_score.hip)
//                  with RMSprop's arithmetic.  The step count and the learning rate are read from the 16-byte device
//                  block, and the launch itself advances the count.
#include "common.h"
#include "grad_guard.h"
#include "lr_schedule.h"
#include "param_groups.h"
#include "weight_ema.h"

#include <cmath>

namespace {

struct RmsCoef {
  float alpha, oma;   // alpha, 1 - alpha (formed in double on the host, then rounded once)
  float eps, wd, two_l2, momentum;
};

// What an element's segment decides: without a group table the launch's one rate and weight decay
struct RmsSegment {
  float rate, wd;
  bool frozen;
};

// The arithmetic of one element; every product-sum is an explicit fmaf, as adam_elem's and for its reason: the vector
// and the scalar form, and every instantiation, produce the same bits whatever the compiler would contract on its own.
// There is no first-step case: torch starts square_avg and the momentum buffer from zeros.  `b` is read and written
// only when the launch has a momentum buffer (has_buf is uniform over the launch).
__device__ __forceinline__ float rms_elem(float wi, float gi, float& sq, float& b, bool has_buf, bool reg,
                                          const RmsCoef& k, const RmsSegment& sg, float& part) {
  gi = fmaf(sg.wd, wi, gi);
  if (reg) {
    gi = fmaf(k.two_l2, wi, gi);
    part = fmaf(wi, wi, part);
  }
  sq = fmaf(k.alpha, sq, (k.oma * gi) * gi);
  const float avg = sqrtf(sq) + k.eps;
  if (has_buf) {
    b = fmaf(k.momentum, b, gi / avg);
    return fmaf(-sg.rate, b, wi);
  }
  return fmaf(-sg.rate, gi / avg, wi);
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
// Four elements as they come from memory, not yet looked at: a load whose result is unpacked at once makes the compiler
// wait for it there, and the early loads of rmsprop_l2_k must stay in flight across the prologue and the barrier
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

// One element with its own loads and stores: the scalar form, the tail, and a vector that straddles a segment's end
template <typename S, bool MASTER, bool GUARD, bool EMA>
__device__ __forceinline__ void rms_one(long long i, S* __restrict__ w, float* __restrict__ wm, const S* __restrict__ g,
                                        float* __restrict__ sq, float* __restrict__ buf, bool reg, const RmsCoef& k,
                                        const RmsSegment& sg, float coef, float& part, float* __restrict__ em, float omd) {
  if (sg.frozen) {   // only the regulariser's value: no gradient read, no store
    if (reg) {
      const float wi = MASTER ? wm[i] : (float)w[i];
      part = fmaf(wi, wi, part);
    }
    return;
  }
  const bool has_buf = buf != nullptr;
  float s = sq[i], b = has_buf ? buf[i] : 0.f;
  const float wi = rms_elem(MASTER ? wm[i] : (float)w[i], clipped<GUARD>((float)g[i], coef), s, b, has_buf, reg, k, sg, part);
  w[i] = (S)wi;
  if (MASTER) wm[i] = wi;
  sq[i] = s;
  if (has_buf) buf[i] = b;
  if constexpr (EMA) em[i] = weight_ema_elem(em[i], weight_ema_kept<S, MASTER>(wi), omd);
}

// Geometry and protocol are adam_l2_k's: workgroups of 1024 threads, at most 256 of them (rms_blocks_for), one ticket per
// workgroup on the step block, no workgroup waits for another.
// VEC: four elements per lane and access when every pointer is aligned for it; the tail of n and the unaligned case take
// one element per lane.  MASTER (S = bf16_t): the step runs on the float32 array `wm`; `w` gets its rounding and is not
// read.  `buf` == nullptr (momentum 0): there is no momentum buffer and the launch moves nothing for it - a branch that
// is uniform over the launch, not a template flag, so the file holds as many kernels as adam_score.hip's adam_l2_k.
// G, the trailing pack, holds a const GradGuardBlock* (GUARD), a const LrScheduleBlock* (SCHED), a ParamGroupBlock*
// (GROUPED) and a WeightEma by value (EMA), any of them in that order, found by type (step_pack.h); the headers of the
// four state the semantics.  One body serves every pack: everything of an option is behind `if constexpr`.
//   prologue : wave 0, every lane.  All loads - steps_done, the rate or the schedule's knot, the lane's segment of the
//              table, the guard's decision, the average's block - are independent of one another and go out together; the
//              only arithmetic in front of the barrier is the schedule's evaluation (a ballot and one float64 division)
//              and one rounded product rate * lr_scale per segment.  (Adam's prologue also forms two float64 expm1 per
//              workgroup or segment there; RMSprop has no bias correction and nothing of that kind.)
//   halted   : the whole workgroup returns after the barrier, before any store and before the ticket.
//   elements : without a table every element has the launch's rate and weight decay; with one every lane walks a cursor
//              over the segments' ends as its elements increase (param_groups.h).  A vector inside one segment takes the
//              vector path; a frozen one loads nothing but w, below n_reg; a vector that straddles an end is done element
//              by element.  rms_elem sees the same values in the same order per lane in every form, so an all-default
//              table leaves the bits of no table, and the vector form those of the scalar form.
//   ticket   : lane 0 stores the workgroup's sq_sum slot and draws; the workgroup that draws the last one writes
//              steps_done + 1, with a schedule the rate used, the segments' counts and the average's count.
template <typename S, bool VEC, bool MASTER, typename... G>
__global__ __launch_bounds__(1024) void rmsprop_l2_k(S* __restrict__ w, float* __restrict__ wm, const S* __restrict__ g,
                                                    float* __restrict__ sq, float* __restrict__ buf,
                                                    float* __restrict__ sq_sum, StepStateBlock* __restrict__ state,
                                                    long long n, long long n_reg, RmsCoef k, G... pack) {
  constexpr bool GUARD = pack_has_v<const GradGuardBlock*, G...>, SCHED = pack_has_v<const LrScheduleBlock*, G...>;
  constexpr bool GROUPED = pack_has_v<ParamGroupBlock*, G...>, EMA = pack_has_v<WeightEma, G...>;
  constexpr int NSEG = GROUPED ? DCTN_PG_MAX_SEGMENTS : 1;
  __shared__ float red[16];
  __shared__ float published[4];   // rate (no table), halted, coef, the average's weight
  __shared__ long long seg_end[NSEG];
  __shared__ float seg_rate[NSEG], seg_wd[NSEG];
  __shared__ int seg_frozen[NSEG];
  __shared__ int seg_count;
  [[maybe_unused]] WeightEma ema{nullptr, nullptr};
  if constexpr (EMA) ema = pack_get<WeightEma>(pack...);
  [[maybe_unused]] ParamGroupBlock* groups = nullptr;
  if constexpr (GROUPED) groups = pack_get<ParamGroupBlock*>(pack...);
  const bool has_buf = buf != nullptr;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
  const long long n_vec = VEC ? (n & ~3LL) : 0;
  // EARLY (the vector form without a table): every lane issues the loads of its first trip HERE, in front of the prologue
  // and the barrier.  None of them depends on the rate, the guard's decision or the average's weight, so the prologue's
  // round trip and the barrier pass while they are in flight; a plain load survives __syncthreads().  A halted launch
  // has then read its gradients and stores nothing, as before.  (With a table a frozen segment's gradient must not be
  // read, and which segments are frozen is only known behind the barrier.)
  constexpr bool EARLY = VEC && !GROUPED;
  using RawW = std::conditional_t<MASTER, float4, decltype(raw4((const S*)nullptr))>;
  [[maybe_unused]] RawW rw;
  [[maybe_unused]] decltype(raw4((const S*)nullptr)) rg;
  [[maybe_unused]] float4 rs, rb, re;   // rb: loaded, and looked at, only with a momentum buffer
  [[maybe_unused]] bool early = false;
  if constexpr (EARLY) {
    const long long i = tid * 4;
    if (i < n_vec) {
      early = true;
      if constexpr (MASTER) rw = raw4(wm + i); else rw = raw4(w + i);
      rg = raw4(g + i), rs = raw4(sq + i);
      if (has_buf) rb = raw4(buf + i);
      if constexpr (EMA) re = raw4(ema.values + i);
    }
  }
  int steps_done = 0;
  float rate = 0.f;
  [[maybe_unused]] int my_steps = 0;
  [[maybe_unused]] bool my_live = false;             // wave 0: this lane's segment is in use and not frozen
  [[maybe_unused]] WeightEmaLane ema_lane{0, 0.f};   // lane 0
  if (threadIdx.x < 64) {   // wave 0, every lane: the schedule's ballot needs them all
    const int lane = threadIdx.x;
    [[maybe_unused]] ParamGroupLane sg{};
    if constexpr (GROUPED) sg = param_group_lane_load(groups, lane);
    if constexpr (EMA) {
      if (lane == 0) published[3] = (ema_lane = weight_ema_lane_load(ema.block)).omd;
    }
    if constexpr (SCHED) {
      const LrScheduleLane knot = lr_schedule_lane_load(pack_get<const LrScheduleBlock*>(pack...), lane);
      steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      rate = lr_schedule_wave_value(knot, lane, steps_done);
    } else {
      steps_done = __hip_atomic_load(&state->steps_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      rate = __hip_atomic_load(&state->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (GUARD) {
      if (lane == 0) {
        const GradGuardBlock* guard = pack_get<const GradGuardBlock*>(pack...);
        published[1] = __hip_atomic_load(&guard->halted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1.f : 0.f;
        published[2] = __hip_atomic_load(&guard->coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if constexpr (GROUPED) {   // the segment's rate: one rounded product
      my_steps = sg.steps;
      my_live = lane < sg.n_segments && (sg.flags & DCTN_PG_FROZEN) == 0u;
      seg_end[lane] = sg.end;
      seg_rate[lane] = __fmul_rn(rate, sg.lr_scale);
      seg_wd[lane] = sg.weight_decay;
      seg_frozen[lane] = (sg.flags & DCTN_PG_FROZEN) != 0u ? 1 : 0;
      if (lane == 0) seg_count = sg.n_segments;
    } else {
      if (lane == 0) published[0] = rate;
    }
  }
  __syncthreads();
  float coef = 1.f;
  if constexpr (GUARD) {
    if (published[1] != 0.f) return;   // the whole workgroup, before any store and before the ticket
    coef = published[2];
  }
  [[maybe_unused]] float omd = 0.f;
  [[maybe_unused]] float* __restrict__ em = nullptr;
  if constexpr (EMA) omd = published[3], em = ema.values;
  [[maybe_unused]] int n_seg = 1;
  [[maybe_unused]] ParamGroupCursor cur{0, 0x7fffffffffffffffLL};
  RmsSegment sg{0.f, k.wd, false};
  if constexpr (GROUPED) {
    n_seg = seg_count;
    cur.end = param_group_end(seg_end, 0, n_seg);
    sg = RmsSegment{seg_rate[0], seg_wd[0], seg_frozen[0] != 0};
  } else {
    sg.rate = published[0];
  }
  auto follow = [&](long long i) {
    if constexpr (GROUPED) {
      if (param_group_advance(cur, i, seg_end, n_seg))
        sg = RmsSegment{seg_rate[cur.seg], seg_wd[cur.seg], seg_frozen[cur.seg] != 0};
    }
  };
  float part = 0.f;
  // four elements of one segment whose values are in registers: the clip, the step, the stores
  auto vec_step = [&](long long i, float (&wi)[4], float (&gi)[4], float (&si)[4], float (&bi)[4], float (&ei)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) gi[e] = clipped<GUARD>(gi[e], coef);
#pragma unroll
    for (int e = 0; e < 4; ++e) wi[e] = rms_elem(wi[e], gi[e], si[e], bi[e], has_buf, i + e < n_reg, k, sg, part);
    store4(sq + i, si), store4(w + i, wi);
    if (has_buf) store4(buf + i, bi);
    if (MASTER) store4(wm + i, wi);
    if constexpr (EMA) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ei[e] = weight_ema_elem(ei[e], weight_ema_kept<S, MASTER>(wi[e]), omd);
      store4(em + i, ei);
    }
  };
  if (VEC) {
    long long i = tid * 4;
    if constexpr (EARLY) {
      if (early) {   // the first trip, loaded above the barrier
        float wi[4], gi[4], si[4], bi[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float ei[4];
        unpack4(rw, wi), unpack4(rg, gi), unpack4(rs, si);
        if (has_buf) unpack4(rb, bi);
        if constexpr (EMA) unpack4(re, ei);
        vec_step(i, wi, gi, si, bi, ei);
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
        float wi[4], gi[4], si[4], bi[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float ei[4];
        if (MASTER) load4(wm + i, wi); else load4(w + i, wi);
        load4(g + i, gi), load4(sq + i, si);
        if (has_buf) load4(buf + i, bi);
        if constexpr (EMA) load4(em + i, ei);
        vec_step(i, wi, gi, si, bi, ei);
      } else {   // an end inside the vector: element by element, each with its own segment's constants and stores
        for (int e = 0; e < 4; ++e) {
          follow(i + e);
          rms_one<S, MASTER, GUARD, EMA>(i + e, w, wm, g, sq, buf, i + e < n_reg, k, sg, coef, part, em, omd);
        }
      }
    }
  }
  for (long long i = n_vec + tid; i < n; i += nthr) {
    follow(i);
    rms_one<S, MASTER, GUARD, EMA>(i, w, wm, g, sq, buf, i < n_reg, k, sg, coef, part, em, omd);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x < 64) {   // wave 0: lane 0 draws the ticket, every lane hears the answer
    unsigned drawn = 0u;
    if (threadIdx.x == 0) {
      // one slot per workgroup, stored (not accumulated), as adam_l2_k
      float total = 0.f;
      for (int j = 0; j < 16; ++j) total += red[j];
      if (sq_sum) sq_sum[blockIdx.x] = total;
      // The ticket of adam_l2_k.  It orders one thing only: every workgroup's read of the step block and the tables
      // before the last workgroup's write of them; the wait makes sure this wave's loads have returned before it draws.
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

unsigned rms_blocks_for(long long n) {   // adam_blocks_for: one vector access of every lane per workgroup, up to 256
  long long b = (n + 4095) / 4096;
  if (b > 256) b = 256;
  return (unsigned)(b < 1 ? 1 : b);
}

// One step as the host sees it: the descriptor (include/dctn_amd.h) and what only RMSprop has
struct RmsStep {
  const dctn_flat_step_t& d;
  void *square_avg, *momentum_buf;   // momentum_buf: null without momentum
  RmsCoef k;
  hipStream_t st;
  const dctn_weight_ema_t* ema;   // null: no average
};

// The one launcher, for every pack: the vector or the scalar kernel by alignment
template <typename S, bool MASTER, typename... G> void rms_launch(const RmsStep& a, G... pack) {
  const dctn_flat_step_t& d = a.d;
  const size_t esz = sizeof(S);
  const bool vec = ((uintptr_t)d.params | (uintptr_t)d.grads) % (4 * esz) == 0 &&
                   ((uintptr_t)a.square_avg | (uintptr_t)a.momentum_buf | (uintptr_t)d.master |
                    (uintptr_t)(a.ema ? a.ema->ema : nullptr)) % 16 == 0;
  const auto kernel = vec ? rmsprop_l2_k<S, true, MASTER, G...> : rmsprop_l2_k<S, false, MASTER, G...>;
  hipLaunchKernelGGL(kernel, dim3(rms_blocks_for(d.n)), dim3(1024), 0, a.st, (S*)d.params, (float*)d.master,
                     (const S*)d.grads, (float*)a.square_avg, (float*)a.momentum_buf, (float*)d.sq_sum,
                     (StepStateBlock*)d.state, (long long)d.n, (long long)d.n_reg, a.k, pack...);
}

// The pack is the optional blocks the step has, in the order rmsprop_l2_k names them: guard, schedule, group table, and
// the average (a pair by value) behind them
template <typename S, bool MASTER> void rms_dispatch(const RmsStep& a) {
  with_blocks([&](auto... pack) {
    if (a.ema) rms_launch<S, MASTER>(a, pack..., WeightEma{(float*)a.ema->ema, (WeightEmaBlock*)a.ema->block});
    else rms_launch<S, MASTER>(a, pack...);
  }, (const GradGuardBlock*)a.d.guard, (const LrScheduleBlock*)a.d.schedule, (ParamGroupBlock*)a.d.groups);
}

}  // namespace

extern "C" {

int dctn_rmsprop_num_partials(int64_t n) { return n < 1 ? 0 : (int)rms_blocks_for(n); }

int dctn_rmsprop_flat_step(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* square_avg,
                           void* momentum_buf_or_null, double alpha, float eps, float weight_decay, float momentum,
                           void* stream) {
  if (!step) return DCTN_ERR_NULL;
  const dctn_flat_step_t& d = *step;
  if (!d.params || !d.grads || !square_avg || !d.state) return DCTN_ERR_NULL;
  if (ema_or_null && (!ema_or_null->ema || !ema_or_null->block)) return DCTN_ERR_NULL;
  if (momentum > 0.f && !momentum_buf_or_null) return DCTN_ERR_NULL;
  if (d.n < 1 || d.n_reg < 0 || d.n_reg > d.n) return DCTN_ERR_BAD_SHAPE;
  if (!(alpha >= 0.0 && alpha < 1.0)) return DCTN_ERR_BAD_SHAPE;   // not finite included; torch raises ValueError
  if (!(momentum >= 0.f) || !(eps >= 0.f) || !(weight_decay >= 0.f)) return DCTN_ERR_BAD_SHAPE;
  if ((d.dtype != DCTN_F32 && d.dtype != DCTN_BF16) || (d.master && d.dtype != DCTN_BF16)) return DCTN_ERR_BAD_DTYPE;
  RmsCoef k;
  k.alpha = (float)alpha, k.oma = (float)(1.0 - alpha), k.eps = eps;
  k.wd = d.groups ? 0.f : weight_decay, k.two_l2 = 2.f * d.l2, k.momentum = momentum;   // a table carries every segment's decay
  // momentum 0: no buffer exists, whatever the pointer says
  const RmsStep a{d, square_avg, momentum > 0.f ? momentum_buf_or_null : nullptr, k, (hipStream_t)stream, ema_or_null};
  if (d.master) rms_dispatch<bf16_t, true>(a);
  else if (d.dtype == DCTN_F32) rms_dispatch<float, false>(a);
  else rms_dispatch<bf16_t, false>(a);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
