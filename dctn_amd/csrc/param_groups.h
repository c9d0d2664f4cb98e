// The parameter-group table's device block (include/dctn_amd.h documents the layout and the semantics: both are part of
// the ABI).  The grouped forms of flat_step_k (flat_step.h) obey it inside the one
// optimizer launch; dctn_param_groups_check validates a host copy.
//
// One SEGMENT is one parameter of the flat buffer, in flat order: elements [end[s-1], end[s]) (end[-1] = 0).
//   rate of a segment  : ONE rounded float32 product rate * lr_scale, where rate is state->lr, or the schedule's value at
//                        the GLOBAL steps_done.  lr_scale == 1.0f leaves the bits alone.
//   Adam's corrections : formed from the SEGMENT's count steps + 1 (torch.optim.Adam's per-parameter state["step"]), in
//                        float64, exactly as lane 0 of a launch without a table forms them from steps_done + 1.
//   SGD's first step   : steps == 0 of the segment (torch's `momentum_buffer is None`).
//   frozen (flags bit 0): no element of w, master, m, v or buf of the segment is stored to, its gradient is not read and
//                        its `steps` does not advance; w * w still goes into sq_sum below n_reg (the reference's
//                        regulariser sums every core whatever requires_grad says; only the gradient term is dropped).
//   the last ticket    : writes steps + 1 for every unfrozen segment, beside steps_done.
//   a halted guarded step writes nothing and advances nothing.
// With every lr_scale 1, every weight_decay the optimizer's, nothing frozen and every count equal to steps_done, a
// grouped launch leaves the ungrouped launch's bits in every buffer, the sq_sum slots included.
//
// The kernels never trust the table for an address: the segment index stays in [0, n_segments - 1] with n_segments
// clamped to 1..64, the last used segment reaches to n whatever its `end` says, and elements are only ever indexed by
// i < n.  A malformed table gives a wrong update, never an access outside the buffers.
#pragma once

#include <cstdint>

#include "step_pack.h"

constexpr int DCTN_PG_MAX_SEGMENTS = 64;   // one segment per lane of a wave, as the schedule's knots
constexpr unsigned DCTN_PG_FROZEN = 1u;

struct ParamGroupBlock {
  int n_segments;                               // 1..64
  int reserved[3];
  long long end[DCTN_PG_MAX_SEGMENTS];          // exclusive, strictly increasing; the last used one equals n
  float lr_scale[DCTN_PG_MAX_SEGMENTS];         // multiplies the rate; 1.0f leaves the bits alone
  float weight_decay[DCTN_PG_MAX_SEGMENTS];     // the segment's coupled weight decay (SGD without SgdDecay ignores it)
  unsigned flags[DCTN_PG_MAX_SEGMENTS];         // bit 0: frozen
  int steps[DCTN_PG_MAX_SEGMENTS];              // steps taken by the segment; the kernel advances it
};
static_assert(sizeof(ParamGroupBlock) == 1552, "the parameter-group block is 1552 bytes (include/dctn_amd.h)");

#if defined(__HIPCC__)
// What one lane of wave 0 holds of the block: its own segment and the count.  Every load is unconditional and independent
// of every other (the block is always 1552 bytes), so they go out together with the caller's load of steps_done; a lane
// at or past n_segments publishes values that no element ever looks up.
struct ParamGroupLane {
  int n_segments, steps;
  long long end;
  float lr_scale, weight_decay;
  unsigned flags;
};
__device__ __forceinline__ ParamGroupLane param_group_lane_load(const ParamGroupBlock* b, int lane) {
  ParamGroupLane v;
  const int n = b->n_segments;
  v.n_segments = n < 1 ? 1 : n > DCTN_PG_MAX_SEGMENTS ? DCTN_PG_MAX_SEGMENTS : n;
  v.end = b->end[lane], v.lr_scale = b->lr_scale[lane], v.weight_decay = b->weight_decay[lane];
  v.flags = b->flags[lane], v.steps = b->steps[lane];
  return v;
}

// A lane's elements only ever increase, so the segment of the next element is found by walking on from the segment of
// the last one: a cursor over the LDS copy of `end`, no search.  The last used segment has no end the cursor could pass.
struct ParamGroupCursor {
  int seg;
  long long end;   // of segment `seg`; LLONG_MAX for the last used segment
};
__device__ __forceinline__ long long param_group_end(const long long* lds_end, int seg, int n_segments) {
  return seg >= n_segments - 1 ? 0x7fffffffffffffffLL : lds_end[seg];
}
// true when the cursor moved: the caller reloads the segment's constants
__device__ __forceinline__ bool param_group_advance(ParamGroupCursor& c, long long i, const long long* lds_end,
                                                    int n_segments) {
  bool moved = false;
  while (i >= c.end) {   // ends at the last used segment at the latest: its end is LLONG_MAX
    ++c.seg;
    c.end = param_group_end(lds_end, c.seg, n_segments);
    moved = true;
  }
  return moved;
}
#endif
