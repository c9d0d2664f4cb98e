// The reference's ConvSBS classifier trains with RMSprop (mnist.py:466-476: RMSprop(lr, alpha, momentum, weight_decay)).
//   RmsRule : torch.optim.RMSprop (coupled weight decay, optional momentum, not centered) as a rule of flat_step_k
//             (flat_step.h): one update + the L2 regulariser over ONE flat parameter buffer, in Adam's geometry and with
//             its 16-byte step block - the launch reads the step count and the learning rate from it and advances the
//             count itself.
#include "flat_step.h"

#include <cmath>

namespace {

struct RmsCoef {
  float alpha, oma;   // alpha, 1 - alpha (formed in double on the host, then rounded once)
  float eps, wd, two_l2, momentum;
};

// State arrays: square_avg, and the momentum buffer when the launch gives one (momentum 0: there is none and the launch
// moves nothing for it).  There is no first-step case - torch starts both from zeros - and no bias correction: a segment
// of a group table steps with its rate and its own weight decay, and its count only advances.
struct RmsRule {
  using Coef = RmsCoef;
  static constexpr int THREADS = 1024, MAX_BLOCKS = 256;
  static constexpr bool HAS_VEC = true, STATE_ALWAYS = true;
  static constexpr SecondState SECOND = SecondState::if_given;
  struct Segment {
    float rate, wd;
    bool frozen;
  };
  static __device__ __forceinline__ Segment segment(const Coef&, float rate, int, float wd, bool frozen) {
    return Segment{rate, wd, frozen};
  }
  template <typename... G> static __device__ __forceinline__ float launch_wd(const Coef& k, G...) { return k.wd; }
  static __device__ __forceinline__ bool skips_state_read(const Segment&) { return false; }
  template <typename... G>
  static __device__ __forceinline__ float elem(float wi, float gi, float& sq, float& b, bool has_buf, bool reg,
                                               const Coef& k, const Segment& sg, float& part) {
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
};

}  // namespace

extern "C" {

int dctn_rmsprop_num_partials(int64_t n) { return n < 1 ? 0 : (int)flat_step_blocks_for<RmsRule>(n); }

int dctn_rmsprop_flat_step(const dctn_flat_step_t* step, const dctn_weight_ema_t* ema_or_null, void* square_avg,
                           void* momentum_buf_or_null, double alpha, float eps, float weight_decay, float momentum,
                           void* stream) {
  if (!step) return DCTN_ERR_NULL;
  const dctn_flat_step_t& d = *step;
  if (const int rc = flat_step_check(d, ema_or_null, {square_avg, d.state, momentum > 0.f ? momentum_buf_or_null : &d}))
    return rc;
  if (!(alpha >= 0.0 && alpha < 1.0)) return DCTN_ERR_BAD_SHAPE;   // not finite included; torch raises ValueError
  if (!(momentum >= 0.f) || !(eps >= 0.f) || !(weight_decay >= 0.f)) return DCTN_ERR_BAD_SHAPE;
  RmsCoef k;
  k.alpha = (float)alpha, k.oma = (float)(1.0 - alpha), k.eps = eps;
  k.wd = d.groups ? 0.f : weight_decay, k.two_l2 = 2.f * d.l2, k.momentum = momentum;   // a table carries every segment's decay
  // momentum 0: no buffer exists, whatever the pointer says
  return flat_step_run(FlatStepLaunch<RmsRule>{d, square_avg, momentum > 0.f ? momentum_buf_or_null : nullptr, k,
                                               (hipStream_t)stream, ema_or_null});
}

}  // extern "C"
