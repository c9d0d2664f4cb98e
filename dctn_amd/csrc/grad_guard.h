// The gradient guard's device block (include/dctn_amd.h documents this layout: it is part of the ABI).  grad_guard.hip
// writes it; the guarded forms of flat_step_k (flat_step.h) read `halted` and `coef`.
#pragma once

#include "step_pack.h"

struct GradGuardBlock {
  float max_norm;     // clip threshold, +inf = never clip; the host writes it
  float last_norm;    // norm seen by the last launch (may be inf / NaN)
  unsigned halted;    // latch: 1 once a non-finite launch was seen; only the host clears it
  int bad_step;       // `seen` at the launch that set the latch, -1 before
  unsigned seen;      // launches so far
  unsigned clipped;   // launches whose coefficient was below 1
  unsigned ticket;    // 0 between launches
  float coef;         // decision for the step that follows: the gradient multiplier (0 when the step is not applied)
};
static_assert(sizeof(GradGuardBlock) == 32, "the guard block is 32 bytes (include/dctn_amd.h)");

#if defined(__HIPCC__)
// the guarded step's gradient: one rounded float32 product, never contracted into the FMA that follows
template <bool GUARD> __device__ __forceinline__ float clipped(float g, float coef) {
  if constexpr (GUARD) return __fmul_rn(g, coef); else return g;
}
#endif
