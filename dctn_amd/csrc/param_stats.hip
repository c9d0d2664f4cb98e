// Sum, sum of squares, largest magnitude and non-finite count of EVERY parameter and of its gradient, for up to 64
// parameters in ONE launch (dctn_param_stats) - what the reference's classifier script logs per parameter and iteration
// through add_weights_and_grads_logging (mnist.py:535: a norm of each parameter and of its gradient) and the
// EPSesPlusLinear recipe through log_parameters_stats (dctn/training.py:247: mean and std) - from the two flat buffers a
// flat optimizer already holds, in float64, with a period counted on the device and a ring of rows in a caller-owned block.
//
// The plan.  Segment s is the elements ends[s - 1] .. ends[s] - 1 of both buffers (ends[-1] = 0).  A segment of c elements
// owns W = min(64, ceil(c / 8192)) workgroups of 256 threads, so it has 256 W threads, numbered workgroup-major.  The
// segment is cut into GROUPS of four consecutive elements counted from the SEGMENT's first element (the last group has
// c mod 4 elements when that is not 0); thread j owns the groups j, j + 256 W, j + 512 W, ... and takes their elements in
// index order, the weight and the gradient of an element in the same turn: a finite value x (widened exactly) adds
// x to `sum`, x * x to `sum_sq` (one fma) and joins |x| into `max_abs`, any other value counts in `nonfinite`.  A whole
// group is loaded in one access per buffer when its address allows - 16 bytes of float32, 8 bytes of bfloat16, two
// 16-byte accesses of float64, each at its own alignment - and element by element otherwise; the values and their order
// are the same either way.  A workgroup then reduces in a fixed tree: lanes by shuffles at distances 32, 16, ..., 1, the
// four waves through LDS in index order.
//
// Reproducible bits.  W, the ownership of groups and every summation order are functions of the segment's length alone:
// a segment's 64 bytes depend on its own values and on nothing else - not on its offset in the flat buffer (and so the
// alignment of its first element, and whether a group went as one access), not on the other segments of the launch or
// its place among them, not on the device's CU count, not on what the workspace held.  Workgroup k STORES its eight
// partial values into its own 64-byte slot of the workspace and draws the block's ticket; the workgroup that draws the
// launch's last ticket adds every segment's slots in index order (one lane per segment), writes the row and advances the
// header.  This is tensor_stats_k's hand-over (sbs_tail.hip) as tt_stats_k has it: slots, ticket, no workgroup waits for
// another, the release and acquire fences in the same places.  A launch that is not recorded (calls % period != 0) reads
// no element: its workgroups draw the ticket and end, and the last one advances `calls`.
#include "common.h"

namespace {

constexpr int PS_MAX_SEGMENTS = 64;
constexpr int PS_THREADS = 256;
constexpr int PS_MAX_WGS = 64;              // workgroups one segment owns at most
constexpr long long PS_PER_WG = 8192;       // elements that earn a segment one workgroup
constexpr long long PS_MAX_SEGMENT = 0x7fffffffLL;

// The block (include/dctn_amd.h): the header, then `capacity` rows of one PSRowHead and n_segments cells
struct PSHeader {
  unsigned calls, recorded, ticket, reserved[5];
};
static_assert(sizeof(PSHeader) == 32, "the header is 32 bytes");
struct PSRowHead {
  unsigned call, seq;
  unsigned long long reserved;
};
static_assert(sizeof(PSRowHead) == 16, "a row starts with 16 bytes");
struct PSHalf {
  double sum, sum_sq, max_abs;
  unsigned long long nonfinite;
};
struct PSCell {
  PSHalf w, g;
};
static_assert(sizeof(PSCell) == 64, "a cell, and a workgroup's slot, is 64 bytes");

// Everything the kernel knows beside its pointers, in its argument: segment s ends in front of element end[s] and owns
// the workgroups wg_first[s] .. wg_first[s + 1] - 1
struct PSArgs {
  long long end[PS_MAX_SEGMENTS];
  unsigned short wg_first[PS_MAX_SEGMENTS + 1];
  int n_segments;
};
static_assert(PS_MAX_SEGMENTS * PS_MAX_WGS <= 0xffff, "a workgroup index fits wg_first");

typedef unsigned short bf16_bits;   // a bfloat16 element as the kernel reads it: the upper half of a float32

__device__ __forceinline__ double ps_widen(float x) { return (double)x; }
__device__ __forceinline__ double ps_widen(double x) { return x; }
__device__ __forceinline__ double ps_widen(bf16_bits x) { return (double)__uint_as_float((unsigned)x << 16); }

template <typename T> struct PSAccess;   // BYTES: the alignment at which a whole group goes in one access (float64: two)
template <> struct PSAccess<float> { static constexpr unsigned BYTES = 16; };
template <> struct PSAccess<double> { static constexpr unsigned BYTES = 16; };
template <> struct PSAccess<bf16_bits> { static constexpr unsigned BYTES = 8; };

__device__ __forceinline__ void ps_load4(const float* p, double (&x)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
}
__device__ __forceinline__ void ps_load4(const double* p, double (&x)[4]) {
  const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
  x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
}
__device__ __forceinline__ void ps_load4(const bf16_bits* p, double (&x)[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);
  x[0] = (double)__uint_as_float(t.x << 16), x[1] = (double)__uint_as_float(t.x & 0xffff0000u);
  x[2] = (double)__uint_as_float(t.y << 16), x[3] = (double)__uint_as_float(t.y & 0xffff0000u);
}

struct PSAcc {
  double sum = 0.0, sum_sq = 0.0, max_abs = 0.0;
  unsigned long long bad = 0ull;
  __device__ __forceinline__ PSAcc() {}
  __device__ __forceinline__ explicit PSAcc(const PSHalf& h) : sum(h.sum), sum_sq(h.sum_sq), max_abs(h.max_abs), bad(h.nonfinite) {}
  __device__ __forceinline__ PSHalf half() const { return PSHalf{sum, sum_sq, max_abs, bad}; }
  __device__ __forceinline__ void take(double v) {
    const double a = fabs(v);
    if (a < INFINITY) {   // false for NaN and for +-Inf
      sum += v;
      sum_sq = fma(v, v, sum_sq);
      max_abs = fmax(max_abs, a);
    } else {
      bad += 1ull;
    }
  }
  __device__ __forceinline__ void join(const PSAcc& o) {
    sum += o.sum, sum_sq += o.sum_sq, max_abs = fmax(max_abs, o.max_abs), bad += o.bad;
  }
  __device__ __forceinline__ PSAcc shuffled_down(int off) const {
    PSAcc o;
    o.sum = __shfl_down(sum, off, 64), o.sum_sq = __shfl_down(sum_sq, off, 64), o.max_abs = __shfl_down(max_abs, off, 64);
    o.bad = __shfl_down(bad, off, 64);
    return o;
  }
};

__device__ __forceinline__ void ps_store_half(PSHalf* h, const PSAcc& a) {
  __hip_atomic_store(&h->sum, a.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&h->sum_sq, a.sum_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&h->max_abs, a.max_abs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&h->nonfinite, a.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ PSAcc ps_load_half(const PSHalf* h) {
  PSAcc a;
  a.sum = __hip_atomic_load(&h->sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.sum_sq = __hip_atomic_load(&h->sum_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.max_abs = __hip_atomic_load(&h->max_abs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.bad = __hip_atomic_load(&h->nonfinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return a;
}

// TW: the element of `weights` (float with a master copy), TG: the element of `grads`
template <typename TW, typename TG>
__global__ __launch_bounds__(PS_THREADS) void param_stats_k(const PSArgs args, const TW* __restrict__ weights,
                                                           const TG* __restrict__ grads, unsigned char* __restrict__ block,
                                                           unsigned capacity, unsigned period, PSCell* __restrict__ workspace) {
  __shared__ PSHalf red[2][PS_THREADS / 64];   // [weights, gradients][wave]
  __shared__ unsigned wg_calls;
  __shared__ int is_last;
  const int t = threadIdx.x;
  PSHeader* hdr = reinterpret_cast<PSHeader*>(block);

  if (t == 0) wg_calls = __hip_atomic_load(&hdr->calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const unsigned calls = wg_calls;
  const bool counted = calls % period == 0;   // the same answer in every workgroup: `calls` moves after the last ticket

  if (counted) {
    int s = 0;
    while (s + 1 < args.n_segments && blockIdx.x >= args.wg_first[s + 1]) ++s;
    const long long begin = s == 0 ? 0 : args.end[s - 1], c = args.end[s] - begin;
    const long long nthr = (long long)(args.wg_first[s + 1] - args.wg_first[s]) * PS_THREADS;
    const long long j = (long long)((int)blockIdx.x - args.wg_first[s]) * PS_THREADS + t;
    const TW* __restrict__ w = weights + begin;
    const TG* __restrict__ g = grads + begin;
    // a group's address is the segment's plus a multiple of the group's bytes: one answer for the whole segment
    const bool w_vec = (uintptr_t)w % PSAccess<TW>::BYTES == 0, g_vec = (uintptr_t)g % PSAccess<TG>::BYTES == 0;

    PSAcc aw, ag;
    for (long long i = j * 4; i < c; i += nthr * 4) {
      double wv[4], gv[4];
      if (c - i >= 4) {
        if (w_vec) {
          ps_load4(w + i, wv);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) wv[e] = ps_widen(w[i + e]);
        }
        if (g_vec) {
          ps_load4(g + i, gv);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) gv[e] = ps_widen(g[i + e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) aw.take(wv[e]), ag.take(gv[e]);
      } else {   // the segment's last group, of one to three elements
        for (long long e = i; e < c; ++e) aw.take(ps_widen(w[e])), ag.take(ps_widen(g[e]));
      }
    }
    for (int off = 32; off > 0; off >>= 1) aw.join(aw.shuffled_down(off)), ag.join(ag.shuffled_down(off));
    if ((t & 63) == 0) red[0][t >> 6] = aw.half(), red[1][t >> 6] = ag.half();
  }
  __syncthreads();

  if (t == 0) {
    if (counted) {
      PSAcc aw(red[0][0]), ag(red[1][0]);
      for (int wv = 1; wv < PS_THREADS / 64; ++wv) aw.join(PSAcc(red[0][wv])), ag.join(PSAcc(red[1][wv]));
      // tensor_stats_k's hand-over of the slot to whichever workgroup turns out to be last: agent-scope stores of the
      // slot, an agent-scope release and an explicit wait BEFORE the ticket is drawn; the workgroup that draws the last
      // ticket makes an agent-scope acquire AFTER it and reads the slots with agent-scope loads.
      PSCell* slot = workspace + blockIdx.x;
      ps_store_half(&slot->w, aw);
      ps_store_half(&slot->g, ag);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    const unsigned drawn = __hip_atomic_fetch_add(&hdr->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == gridDim.x - 1;
    if (last && counted) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    is_last = last ? 1 : 0;
  }
  __syncthreads();
  if (is_last == 0 || t >= 64) return;   // every workgroup but the launch's last ends here; nobody waits

  // the last workgroup's first wave: lane s adds the slots of segment s in index order and writes its cell; then lane 0
  // writes the row's head and the header, `seq` after the cells
  const unsigned recorded = __hip_atomic_load(&hdr->recorded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (counted) {
    unsigned char* row = block + sizeof(PSHeader) + (size_t)(recorded % capacity) * (sizeof(PSRowHead) + sizeof(PSCell) * (size_t)args.n_segments);
    if (t < args.n_segments) {
      const unsigned first = args.wg_first[t], end = args.wg_first[t + 1];
      PSAcc aw = ps_load_half(&workspace[first].w), ag = ps_load_half(&workspace[first].g);
      for (unsigned k = first + 1; k < end; ++k) aw.join(ps_load_half(&workspace[k].w)), ag.join(ps_load_half(&workspace[k].g));
      PSCell* cell = reinterpret_cast<PSCell*>(row + sizeof(PSRowHead)) + t;
      cell->w = aw.half(), cell->g = ag.half();
    }
    if (t == 0) {
      PSRowHead* head = reinterpret_cast<PSRowHead*>(row);
      head->call = calls;
      head->reserved = 0ull;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the cells of this wave's lanes before `seq`
      head->seq = recorded;
      __hip_atomic_store(&hdr->recorded, recorded + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (t != 0) return;
  __hip_atomic_store(&hdr->calls, calls + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&hdr->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch draws from 0 again
}

unsigned segment_workgroups(long long c) {
  const long long w = (c + PS_PER_WG - 1) / PS_PER_WG;
  return (unsigned)(w > PS_MAX_WGS ? PS_MAX_WGS : w);
}

// strictly increasing from at least 1: every segment has an element
bool ends_are_valid(const int64_t* ends, int n_segments) {
  int64_t before = 0;
  for (int s = 0; s < n_segments; ++s) {
    if (ends[s] <= before) return false;
    before = ends[s];
  }
  return true;
}

bool ends_are_supported(const int64_t* ends, int n_segments) {
  if (n_segments > PS_MAX_SEGMENTS) return false;
  int64_t before = 0;
  for (int s = 0; s < n_segments; ++s) {
    if (ends[s] - before > PS_MAX_SEGMENT) return false;
    before = ends[s];
  }
  return true;
}

template <typename TW, typename TG>
void launch(const PSArgs& args, unsigned n_wg, const void* weights, const void* grads, void* block, int capacity, int period,
            void* workspace, hipStream_t st) {
  hipLaunchKernelGGL((param_stats_k<TW, TG>), dim3(n_wg), dim3(PS_THREADS), 0, st, args, (const TW*)weights, (const TG*)grads,
                     (unsigned char*)block, (unsigned)capacity, (unsigned)period, (PSCell*)workspace);
}

}  // namespace

extern "C" {

size_t dctn_param_stats_block_bytes(int n_segments, int capacity) {
  if (n_segments < 1 || n_segments > PS_MAX_SEGMENTS || capacity < 1) return 0;
  return sizeof(PSHeader) + (size_t)capacity * (sizeof(PSRowHead) + sizeof(PSCell) * (size_t)n_segments);
}

size_t dctn_param_stats_workspace_bytes(const int64_t* ends, int n_segments) {
  if (!ends || n_segments < 1 || n_segments > PS_MAX_SEGMENTS) return 0;
  if (!ends_are_valid(ends, n_segments) || !ends_are_supported(ends, n_segments)) return 0;
  size_t workgroups = 0;
  int64_t before = 0;
  for (int s = 0; s < n_segments; ++s) {
    workgroups += segment_workgroups(ends[s] - before);
    before = ends[s];
  }
  return workgroups * sizeof(PSCell);
}

int dctn_param_stats(const void* params, const void* master_or_null, const void* grads, const int64_t* ends, int n_segments,
                     void* block, int capacity, int period, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  if (!params || !grads || !ends || !block) return DCTN_ERR_NULL;
  if (n_segments < 1 || !ends_are_valid(ends, n_segments)) return DCTN_ERR_BAD_SHAPE;
  if (capacity < 1 || period < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  if (!ends_are_supported(ends, n_segments)) return DCTN_ERR_UNSUPPORTED;
  const uintptr_t elem = dtype_size(dtype);
  if ((uintptr_t)params % elem != 0 || (uintptr_t)grads % elem != 0 || (uintptr_t)master_or_null % 4 != 0) return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)block % 8 != 0 || (uintptr_t)workspace % 8 != 0) return DCTN_ERR_UNSUPPORTED;
  if (master_or_null && dtype != DCTN_BF16) return DCTN_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < dctn_param_stats_workspace_bytes(ends, n_segments)) return DCTN_ERR_WORKSPACE;

  PSArgs args = {};
  args.n_segments = n_segments;
  unsigned n_wg = 0;
  int64_t before = 0;
  for (int s = 0; s < n_segments; ++s) {
    args.end[s] = ends[s];
    args.wg_first[s] = (unsigned short)n_wg;
    n_wg += segment_workgroups(ends[s] - before);
    before = ends[s];
  }
  for (int s = n_segments; s <= PS_MAX_SEGMENTS; ++s) args.wg_first[s] = (unsigned short)n_wg;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DCTN_F32)
    launch<float, float>(args, n_wg, params, grads, block, capacity, period, workspace, st);
  else if (dtype == DCTN_F64)
    launch<double, double>(args, n_wg, params, grads, block, capacity, period, workspace, st);
  else if (master_or_null)
    launch<float, bf16_bits>(args, n_wg, master_or_null, grads, block, capacity, period, workspace, st);
  else
    launch<bf16_bits, bf16_bits>(args, n_wg, params, grads, block, capacity, period, workspace, st);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
