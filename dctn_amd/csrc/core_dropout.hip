// Component dropout of the EPS cores (reference: dctn/eps_plus_linear.py:139-143, `mask * core / p` with
// mask ~ Bernoulli(p) per component) as ONE launch each way for all cores of a model, with a mask that is a pure
// function of (seed, draw, core number, element index): Philox4x32-10, nothing stored.  include/dctn_amd.h holds the
// normative definition.  Three kernels from one template:
//   fwd  : out = keep ? core / p : 0; reads the draw index from the 16-byte device block, leaves the draw record for
//          the backward, and the launch itself advances the block (flat_step_k's ticket): replays draw d, d + 1, ...
//   bwd  : d_core = keep ? d_out / p : 0 from the record (d_core may BE d_out: a lane reads its 4 values, then writes them)
//   mask : 1 / 0 from the record (diagnostic)
#include "common.h"

namespace {

constexpr int DROP_MAX_SEG = 8;
constexpr int DROP_THREADS = 1024;   // 16 waves per workgroup: with at most 256 workgroups, 4 waves per SIMD hide the round trips of a large core

struct DropState {   // include/dctn_amd.h documents this layout: it is part of the ABI
  unsigned seed_lo, seed_hi, draws_done, ticket;
};

struct DropSegs {   // passed by value in the kernel argument
  const void* in[DROP_MAX_SEG];
  void* out[DROP_MAX_SEG];
  unsigned long long n[DROP_MAX_SEG];         // elements
  unsigned long long blk_end[DROP_MAX_SEG];   // running total of Philox blocks (4 elements; the last one may be partial)
  int count;
};

enum { DROP_FWD = 0, DROP_BWD = 1, DROP_MASK = 2 };

// the arithmetic type of the one division: float32 (double for float64), rounded once to the tensor dtype
template <typename S> struct DropArith { typedef float type; };
template <> struct DropArith<double> { typedef double type; };

template <typename S> struct Drop4 {};   // 4 consecutive elements through the widest accesses: 16 bytes, bf16 8
template <> struct Drop4<float> {
  static constexpr unsigned ALIGN = 16;
  static __device__ __forceinline__ void load(const float* p, float (&x)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&x)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  }
};
template <> struct Drop4<double> {
  static constexpr unsigned ALIGN = 16;
  static __device__ __forceinline__ void load(const double* p, double (&x)[4]) {
    const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
    x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
  }
  static __device__ __forceinline__ void store(double* p, const double (&x)[4]) {
    reinterpret_cast<double2*>(p)[0] = make_double2(x[0], x[1]);
    reinterpret_cast<double2*>(p)[1] = make_double2(x[2], x[3]);
  }
};
template <> struct Drop4<bf16_t> {
  static constexpr unsigned ALIGN = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&x)[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);   // bf16 -> f32 is the upper half of the word
    x[0] = __uint_as_float(t.x << 16), x[1] = __uint_as_float(t.x & 0xffff0000u);
    x[2] = __uint_as_float(t.y << 16), x[3] = __uint_as_float(t.y & 0xffff0000u);
  }
  static __device__ __forceinline__ unsigned bits(float x) { return __builtin_bit_cast(unsigned short, (bf16_t)x); }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&x)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(bits(x[0]) | (bits(x[1]) << 16), bits(x[2]) | (bits(x[3]) << 16));
  }
};

// A lane owns whole Philox blocks: block b of segment s is elements 4 b .. 4 b + 3 of that core.  Full blocks of a
// segment whose base (both bases, for fwd / bwd) is aligned for Drop4 move as vectors; the partial last block, and
// every block of a segment aligned only to its element size (a core that is a view into FlatAdam's flat buffer), go
// element by element.  At most 256 workgroups: the forward's ticket is one atomic per workgroup on one address
// (adam_score.hip).
template <typename S, int OP>
__global__ __launch_bounds__(DROP_THREADS) void core_dropout_k(DropSegs segs, const S* __restrict__ p_ptr,
                                                               DropState* state, unsigned* record) {
  typedef typename DropArith<S>::type A;
  __shared__ unsigned draw[3];
  unsigned k0, k1, d;
  if (OP == DROP_FWD) {
    // lane 0 of every workgroup reads the seed and the draw count BEFORE it takes the workgroup's ticket at the end; the
    // one write of the launch to draws_done happens after the last ticket is drawn, so no workgroup can see the new value
    if (threadIdx.x == 0) {
      draw[0] = __hip_atomic_load(&state->seed_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      draw[1] = __hip_atomic_load(&state->seed_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      draw[2] = __hip_atomic_load(&state->draws_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (blockIdx.x == 0) record[0] = draw[0], record[1] = draw[1], record[2] = draw[2], record[3] = 0u;
    }
    __syncthreads();
    k0 = draw[0], k1 = draw[1], d = draw[2];
  } else {
    k0 = record[0], k1 = record[1], d = record[2];
  }
  const A p = (A)*p_ptr;
  // keep iff word < T, T = min(floor(p * 2^32), 2^32 - 1) in double from p as the tensor dtype stores it
  const double scaled = floor((double)p * 4294967296.0);
  const unsigned T = scaled >= 4294967295.0 ? 0xFFFFFFFFu : (scaled > 0.0 ? (unsigned)scaled : 0u);

  const unsigned long long total = segs.blk_end[segs.count - 1];
  const unsigned long long stride = (unsigned long long)gridDim.x * DROP_THREADS;
  for (unsigned long long g = (unsigned long long)blockIdx.x * DROP_THREADS + threadIdx.x; g < total; g += stride) {
    int s = 0;
    while (s < segs.count - 1 && g >= segs.blk_end[s]) ++s;
    const unsigned long long b = g - (s ? segs.blk_end[s - 1] : 0ull);   // < 2^32: cores stay below 2^34 elements
    const unsigned long long e0 = b * 4ull, n = segs.n[s];
    const S* in = static_cast<const S*>(segs.in[s]);
    S* out = static_cast<S*>(segs.out[s]);
    unsigned w[4];
    philox4x32_10((unsigned)b, 0u, d, (unsigned)s, k0, k1, w);
    const bool vec = e0 + 4ull <= n && (((uintptr_t)out | (uintptr_t)in) % Drop4<S>::ALIGN) == 0   /* mask: in is null */;
    if (vec) {
      A x[4];
      if (OP == DROP_MASK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = w[i] < T ? (A)1 : (A)0;
      } else {
        Drop4<S>::load(in + e0, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = w[i] < T ? x[i] / p : (A)0;
      }
      Drop4<S>::store(out + e0, x);
    } else {
      for (int i = 0; i < 4 && e0 + i < n; ++i) {
        const bool keep = w[i] < T;
        if (OP == DROP_MASK) out[e0 + i] = (S)(keep ? (A)1 : (A)0);
        else out[e0 + i] = (S)(keep ? (A)in[e0 + i] / p : (A)0);
      }
    }
  }

  if (OP == DROP_FWD && threadIdx.x == 0) {
    // The ticket, as flat_step_k's (flat_step.h).  It orders one thing only: every workgroup's read of the block before the last
    // workgroup's write of it.  No data passes between workgroups (the kernel boundary publishes the cores); the wait
    // makes sure this lane's state loads have returned before the ticket is drawn, and the writer acts on the value its
    // own ticket returned.
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
      state->draws_done = d + 1u;
      state->ticket = 0u;
    }
  }
}

// [op][dtype code]
const char* const DROP_NAMES[3][3] = {
    {"core_dropout_fwd_f32", "core_dropout_fwd_f64", "core_dropout_fwd_bf16"},
    {"core_dropout_bwd_f32", "core_dropout_bwd_f64", "core_dropout_bwd_bf16"},
    {"core_dropout_mask_f32", "core_dropout_mask_f64", "core_dropout_mask_bf16"},
};

template <int OP>
int drop_launch(const void* const* in, void* const* out, const int64_t* numel, int n_cores, const void* p, void* state,
                void* record, int dtype, void* stream) {
  if (!out || !numel || !p || !record || (OP != DROP_MASK && !in) || (OP == DROP_FWD && !state)) return DCTN_ERR_NULL;
  if (n_cores < 1) return DCTN_ERR_BAD_SHAPE;
  if (n_cores > DROP_MAX_SEG) return DCTN_ERR_UNSUPPORTED;
  if (dtype != DCTN_F32 && dtype != DCTN_F64 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  DropSegs segs = {};
  unsigned long long blocks = 0;
  for (int s = 0; s < n_cores; ++s) {
    if (OP == DROP_BWD && !out[s] && !in[s]) {   // a core without a gradient: skipped, and it keeps its number
      segs.blk_end[s] = blocks;
      continue;
    }
    if (!out[s] || (OP != DROP_MASK && !in[s])) return DCTN_ERR_NULL;
    if (numel[s] < 1 || numel[s] >= (int64_t)1 << 34) return DCTN_ERR_BAD_SHAPE;   // the block index is 32 bits of the counter
    segs.in[s] = OP == DROP_MASK ? nullptr : in[s];
    segs.out[s] = out[s];
    segs.n[s] = (unsigned long long)numel[s];
    blocks += ((unsigned long long)numel[s] + 3) / 4;
    segs.blk_end[s] = blocks;
  }
  segs.count = n_cores;
  if (blocks == 0) return DCTN_OK;
  unsigned long long wgs = (blocks + DROP_THREADS - 1) / DROP_THREADS;
  const unsigned long long cap = dctn_dev().cus < 256 ? (dctn_dev().cus < 1 ? 1 : dctn_dev().cus) : 256;
  if (wgs > cap) wgs = cap;
  const dim3 g((unsigned)wgs), b(DROP_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define DCTN_DROP_LAUNCH(S) \
  hipLaunchKernelGGL((core_dropout_k<S, OP>), g, b, 0, st, segs, (const S*)p, (DropState*)state, (unsigned*)record)
  if (dtype == DCTN_F32) DCTN_DROP_LAUNCH(float);
  else if (dtype == DCTN_F64) DCTN_DROP_LAUNCH(double);
  else DCTN_DROP_LAUNCH(bf16_t);
#undef DCTN_DROP_LAUNCH
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel(DROP_NAMES[OP][dtype]);
  return DCTN_OK;
}

}  // namespace

extern "C" {

size_t dctn_core_dropout_state_bytes(void) { return sizeof(DropState); }

int dctn_core_dropout_fwd(const void* const* cores, void* const* out, const int64_t* numel, int n_cores, const void* p,
                          void* state, void* record, int dtype, void* stream) {
  return drop_launch<DROP_FWD>(cores, out, numel, n_cores, p, state, record, dtype, stream);
}

int dctn_core_dropout_bwd(const void* const* d_out, void* const* d_core, const int64_t* numel, int n_cores, const void* p,
                          const void* record, int dtype, void* stream) {
  return drop_launch<DROP_BWD>(d_out, d_core, numel, n_cores, p, nullptr, const_cast<void*>(record), dtype, stream);
}

int dctn_core_dropout_mask(void* const* mask, const int64_t* numel, int n_cores, const void* p, const void* record,
                           int dtype, void* stream) {
  return drop_launch<DROP_MASK>(nullptr, mask, numel, n_cores, p, nullptr, const_cast<void*>(record), dtype, stream);
}

}  // extern "C"
