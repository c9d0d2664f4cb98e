// The weight average's device block and its arithmetic (include/dctn_amd.h documents the layout and the update: both are
// part of the ABI).  The EMA forms of flat_step_k (flat_step.h) update the average inside
// the optimizer launch, from the value they are about to store; dctn_weight_ema_weight runs the per-launch weight on the
// host.
#pragma once

#include <cstdint>

#include "step_pack.h"

constexpr unsigned DCTN_EMA_WARMUP = 1u;

struct WeightEmaBlock {
  float decay;        // in [0, 1); the host writes it
  unsigned flags;     // bit 0: warm-up
  int updates;        // updates done so far; the launch advances it
  float last_omd;     // the weight the last update used; 0 before the first
  int reserved[4];
};
static_assert(sizeof(WeightEmaBlock) == 32, "the weight-average block is 32 bytes (include/dctn_amd.h)");

// The member of the step kernels' trailing pack: the n float32 averages and the block, passed by value
struct WeightEma {
  float* values;
  WeightEmaBlock* block;
};

// The weight of one launch, 1 - d_u, from the block's three cells: formed in float64 (the warm-up is one division), then
// rounded once.  Contraction is off: the definition has no product-sum, and none may appear.
__host__ __device__ inline float weight_ema_omd(float decay, unsigned flags, int updates) {
#pragma clang fp contract(off)
  double d = (double)decay;
  if ((flags & DCTN_EMA_WARMUP) != 0u) {
    const double u = (double)updates;
    const double ramp = (1.0 + u) / (10.0 + u);
    d = ramp < d ? ramp : d;
  }
  return (float)(1.0 - d);
}

#if defined(__HIPCC__)
// What lane 0 of a workgroup holds of the block.  The three loads depend on nothing, so they go out with the caller's
// load of steps_done.
struct WeightEmaLane {
  int updates;
  float omd;
};
__device__ __forceinline__ WeightEmaLane weight_ema_lane_load(const WeightEmaBlock* b) {
  const float decay = __hip_atomic_load(&b->decay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned flags = __hip_atomic_load(&b->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int updates = __hip_atomic_load(&b->updates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return WeightEmaLane{updates, weight_ema_omd(decay, flags, updates)};
}
// The workgroup that drew the step block's last ticket: plain vector stores, beside steps_done
__device__ __forceinline__ void weight_ema_advance(WeightEmaBlock* b, const WeightEmaLane& v) {
  b->updates = v.updates + 1;
  b->last_omd = v.omd;
}

// One element: three float32 operations, each rounded on its own (numpy float32 gives the same bits): what __fsub_rn,
// __fmul_rn and __fadd_rn say.  They are written as plain operators under `fp contract(off)` because the intrinsics are
// inline functions of the HIP headers: their operations carry the contraction flag of THAT text, and the compiler fused
// the product and the sum into one v_fmac_f32, which rounds once where the definition rounds twice.
__device__ __forceinline__ float weight_ema_elem(float ema, float w_new, float omd) {
#pragma clang fp contract(off)
  const float diff = w_new - ema;
  const float move = omd * diff;
  return ema + move;
}
// The value the optimizer keeps for an element whose float32 result is wi: wi itself with a master copy (or float32
// parameters), else the parameter as stored, rounded to S and widened again
template <typename S, bool MASTER> __device__ __forceinline__ float weight_ema_kept(float wi) {
  if constexpr (MASTER) return wi; else return (float)(S)wi;
}
#endif
