// The learning-rate schedule's device block and its arithmetic (include/dctn_amd.h documents the layout and the
// evaluation: both are part of the ABI).  The scheduled forms of flat_step_k (flat_step.h)
// evaluate it from the device step count inside the optimizer launch; dctn_lr_schedule_value runs the
// same function on the host.
#pragma once

#include <cstdint>

#include "step_pack.h"

constexpr int DCTN_LR_MAX_KNOTS = 64;   // one knot per lane of a wave

struct LrScheduleBlock {
  int n_knots;                      // 1..64
  float scale;                      // multiplies every value; 1.0f leaves the bits alone
  int reserved[2];
  int k[DCTN_LR_MAX_KNOTS];         // strictly increasing step indices, k[0] >= 0
  float lr[DCTN_LR_MAX_KNOTS];      // the rate at each knot
  int hold[DCTN_LR_MAX_KNOTS];      // 1: lr[i] holds on [k[i], k[i+1]); 0: linear to lr[i+1]
};
static_assert(sizeof(LrScheduleBlock) == 784, "the schedule block is 784 bytes (include/dctn_amd.h)");

// The 16-byte step block of flat_step_k (include/dctn_amd.h documents this layout: it is part of the ABI)
struct StepStateBlock {
  int steps_done;
  float lr;
  unsigned ticket;
  unsigned reserved;
};
static_assert(sizeof(StepStateBlock) == 16, "the step block is 16 bytes (include/dctn_amd.h)");

// The value at step s.  `reached` = how many knots have k <= s; (k_i, lr_i, hold_i) is knot max(reached, 1) - 1 and
// (k_j, lr_j) the knot after it (knot i again when i is the last).  The linear form is one float64 division, one
// multiplication and one addition, each rounded on its own (contraction is off for this function: an FMA would round
// once where the definition rounds twice), then one rounding to float32; the scale is one rounded float32 product.
__host__ __device__ inline float lr_schedule_eval(long long s, int reached, int n_knots, int k_i, int k_j, float lr_i,
                                                  float lr_j, int hold_i, float scale) {
#pragma clang fp contract(off)
  float value = lr_i;   // in front of the first knot, on a hold segment, at and past the last knot
  if (reached > 0 && reached < n_knots && hold_i == 0) {
    const double frac = (double)(s - k_i) / (double)(k_j - k_i);
    const double rise = ((double)lr_j - (double)lr_i) * frac;
    value = (float)((double)lr_i + rise);
  }
  return value * scale;
}

// The whole block on the host (the knots counted one by one; the kernels count them with a ballot)
inline float lr_schedule_value_host(const LrScheduleBlock& b, long long s) {
  int reached = 0;
  while (reached < b.n_knots && (long long)b.k[reached] <= s) ++reached;
  const int i = reached > 0 ? reached - 1 : 0, j = i + 1 < b.n_knots ? i + 1 : i;
  return lr_schedule_eval(s, reached, b.n_knots, b.k[i], b.k[j], b.lr[i], b.lr[j], b.hold[i], b.scale);
}

#if defined(__HIPCC__)
// What one lane of wave 0 holds of the block: its own knot and the two header words.  Every load is unconditional and
// independent of every other (the block is always 784 bytes), so they go out together with the caller's load of
// steps_done; a lane at or past n_knots never counts as reached, whatever its slot holds.
struct LrScheduleLane {
  int n_knots, k, hold;
  float scale, lr;
};
__device__ __forceinline__ LrScheduleLane lr_schedule_lane_load(const LrScheduleBlock* __restrict__ b, int lane) {
  LrScheduleLane v;
  v.n_knots = b->n_knots, v.scale = b->scale;
  v.k = b->k[lane], v.lr = b->lr[lane], v.hold = b->hold[lane];
  return v;
}
// All 64 lanes of the wave call it; every lane returns the rate of step s.  The segment is the population count of the
// ballot "my knot is reached" (k is strictly increasing, so the reached knots are a prefix): no loop over the table.
__device__ __forceinline__ float lr_schedule_wave_value(const LrScheduleLane& v, int lane, int s) {
  const int reached = __popcll(__ballot(lane < v.n_knots && v.k <= s));
  const int i = reached > 0 ? reached - 1 : 0, j = i + 1 < v.n_knots ? i + 1 : i;
  return lr_schedule_eval(s, reached, v.n_knots, __shfl(v.k, i, 64), __shfl(v.k, j, 64), __shfl(v.lr, i, 64),
                          __shfl(v.lr, j, 64), __shfl(v.hold, i, 64), v.scale);
}
#endif
