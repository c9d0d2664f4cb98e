// The gradient guard: one launch in front of the optimizer step that forms the squared norm of the flat gradient buffer
// and turns it into the decision the guarded step kernels act on (grad_guard.h: `halted`, `coef`).
//   - a non-finite gradient (or loss) anywhere: the step is not applied, and a latch keeps every later one from being
//     applied until the host clears it - the reference's stop-on-NaN-loss hook (new_runner.py:544) without the host
//     reading a value per iteration, and before the optimizer has written NaN into every parameter and moment;
//   - otherwise coef = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s coefficient.
// Every workgroup sums g^2 over its elements in FLOAT64: the square of a float32 (or bf16) value cannot overflow a
// double, and 2^20 of them cannot either, so the sum is non-finite exactly when some element is.  Each workgroup STORES
// its sum into its own slot of `partials` and draws a ticket; the workgroup that draws the last ticket adds the slots in
// one fixed order and writes the block.  NO workgroup waits for another: every one but the last simply ends.
#include "common.h"
#include "grad_guard.h"

#include <cmath>

namespace {

__device__ __forceinline__ void gg_load4(const float* p, float (&x)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
}
__device__ __forceinline__ void gg_load4(const bf16_t* p, float (&x)[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);   // bf16 -> f32 is the upper half of the word
  x[0] = __uint_as_float(t.x << 16), x[1] = __uint_as_float(t.x & 0xffff0000u);
  x[2] = __uint_as_float(t.y << 16), x[3] = __uint_as_float(t.y & 0xffff0000u);
}

// VEC: four elements per lane and access when the gradient pointer is aligned for it (the rule of flat_step_k's vector forms); the tail of n
// and the unaligned case take one element per lane.  Workgroups of 1024 threads, at most 256 of them, grid-stride:
// the grid of flat_step_k's 1024-thread rules, so that the ticket costs what that kernel's does.
template <typename S, bool VEC>
__global__ __launch_bounds__(1024) void grad_guard_k(const S* __restrict__ g, long long n, const float* __restrict__ loss,
                                                    double* __restrict__ partials, GradGuardBlock* __restrict__ guard) {
  __shared__ double red[17];   // 16 wave sums; red[16] != 0: this workgroup drew the last ticket
  double part = 0.0;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
  const long long n_vec = VEC ? (n & ~3LL) : 0;
  if (VEC) {
    for (long long i = tid * 4; i < n_vec; i += nthr * 4) {
      float gi[4];
      gg_load4(g + i, gi);
#pragma unroll
      for (int e = 0; e < 4; ++e) part = fma((double)gi[e], (double)gi[e], part);
    }
  }
  for (long long i = n_vec + tid; i < n; i += nthr) {
    const double gi = (double)(float)g[i];
    part = fma(gi, gi, part);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int j = 0; j < 16; ++j) total += red[j];
    // The hand-over of the slot to whichever workgroup turns out to be last: the slot leaves this CU's caches
    // (agent-scope store), an agent-scope release and an explicit wait come BEFORE the ticket is drawn, and the
    // workgroup that draws the last ticket makes an agent-scope acquire AFTER it - the acquire-release ticket written
    // as its two fences, so that the wait between release and ticket is in the code and not left to the compiler.
    __hip_atomic_store(&partials[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(&guard->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    red[16] = last ? 1.0 : 0.0;
  }
  __syncthreads();
  if (red[16] == 0.0 || threadIdx.x >= 64) return;   // every workgroup but the last ends here; nobody waits
  // the last workgroup's first wave: lane j adds slots j, j + 64, ... in that order, then one fixed butterfly
  double total = 0.0;
  for (unsigned j = threadIdx.x; j < gridDim.x; j += 64)
    total += __hip_atomic_load(&partials[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(total);
  const float max_norm = guard->max_norm;
  const bool finite = isfinite(total) && (loss == nullptr || isfinite(loss[0]));
  const bool apply = guard->halted == 0u && finite;
  const unsigned seen = guard->seen;
  float coef = 0.f;
  if (apply) {
    coef = fminf(1.f, (float)((double)max_norm / ((double)norm + 1e-6)));   // torch.nn.utils.clip_grad_norm_
    if (coef < 1.f) guard->clipped = guard->clipped + 1u;
  } else if (!finite && guard->halted == 0u) {   // the first non-finite launch sets the latch and names itself
    guard->halted = 1u;
    guard->bad_step = (int)seen;
  }
  guard->last_norm = norm;
  guard->coef = coef;
  guard->seen = seen + 1u;
  guard->ticket = 0u;   // plain vector stores; the next launch starts from ticket 0 again
}

unsigned guard_blocks_for(long long n) {   // flat_step_blocks_for's rule for 1024 threads with a vector form
  long long b = (n + 4095) / 4096;
  if (b > 256) b = 256;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

size_t dctn_grad_guard_state_bytes(void) { return sizeof(GradGuardBlock); }

int dctn_grad_guard_num_partials(int64_t n) { return n < 1 ? 0 : (int)guard_blocks_for(n); }

int dctn_grad_guard_check(const void* grads, int64_t n, int dtype, const void* loss_or_null, void* partials, void* guard,
                          void* stream) {
  if (!grads || !partials || !guard) return DCTN_ERR_NULL;
  if (n < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  hipStream_t st = (hipStream_t)stream;
  const size_t esz = dtype == DCTN_F32 ? 4 : 2;
  const bool vec = (uintptr_t)grads % (4 * esz) == 0;
  const dim3 g(guard_blocks_for(n)), b(1024);
#define DCTN_GUARD_LAUNCH(S, VEC)                                                                                \
  hipLaunchKernelGGL((grad_guard_k<S, VEC>), g, b, 0, st, (const S*)grads, (long long)n, (const float*)loss_or_null, \
                     (double*)partials, (GradGuardBlock*)guard)
  if (dtype == DCTN_F32) {
    if (vec) DCTN_GUARD_LAUNCH(float, true); else DCTN_GUARD_LAUNCH(float, false);
  } else {
    if (vec) DCTN_GUARD_LAUNCH(bf16_t, true); else DCTN_GUARD_LAUNCH(bf16_t, false);
  }
#undef DCTN_GUARD_LAUNCH
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
