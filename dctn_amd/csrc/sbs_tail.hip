// The tail of the ConvSBS classifier (mnist.py:255-263) and the statistics of its strings' outputs.
//   - dctn_position_mean_fwd / _bwd: the mean over positions of the final string's (B, H', W', L) output - the
//     reference's einops.reduce(result, "b h w l -> b l", "mean") - and its adjoint.  One workgroup per sample; the sum
//     is formed in FLOAT64 in an order that depends on (P, L) alone, divided once and rounded once, so a sample's row
//     has the same bits whatever batch it sits in and on whatever device.
//   - dctn_tensor_stats: the moments, |y| range and non-finite count of up to 8 tensors in ONE launch - what the
//     reference's runner logs per string through forward hooks (mnist.py:537-553: mean, std, mean |y|, min |y|, max |y|)
//     and what scale_layers_using_batch reads per string (mnist.py:273: tensor.std().item()).  The structure is
//     grad_guard.hip's and nothing else: every workgroup STORES its partials into its own slots and draws its tensor's
//     ticket; the workgroup that draws the tensor's last ticket adds the slots in index order and writes the record.
//     NO workgroup waits for another: every one but the last of a tensor simply ends.
#include "common.h"

#include <cmath>

namespace {

constexpr int PM_THREADS = 256;     // position mean: R * L <= 256 threads, R = 256 / L position phases
constexpr int PM_MAX_L = 64;
constexpr int TS_MAX_TENSORS = 8;
constexpr int TS_MAX_BLOCKS = 256;  // workgroups per tensor: min(256, ceil(n / 4096)), grad_guard.hip's rule
constexpr int TS_THREADS = 1024;
constexpr int TS_SLOT = 6;          // doubles per slot: sum, sum of squares, sum |y|, min |y|, max |y|, non-finite count

// thread t owns label t % L and position phase t / L: consecutive threads read consecutive elements of a sample; the R
// partial sums of a label are joined through LDS in phase order
template <typename T>
__global__ __launch_bounds__(PM_THREADS) void position_mean_fwd_k(const T* __restrict__ y, T* __restrict__ out, long long P,
                                                                  int L, int R) {
  __shared__ double red[PM_THREADS];
  const int t = threadIdx.x;
  const T* row = y + (long long)blockIdx.x * P * L;
  double part = 0.0;
  for (long long i = t; i < P * L; i += (long long)R * L) part += (double)row[i];   // i % L == t % L: R * L is a multiple of L
  red[t] = part;
  __syncthreads();
  if (t >= L) return;
  double total = 0.0;
  for (int r = 0; r < R; ++r) total += red[r * L + t];
  out[(long long)blockIdx.x * L + t] = (T)(total / (double)P);
}

// dy[b, p, l] = dlogits[b, l] / P: V elements (16 bytes) per thread where dy is aligned for it, one element per thread
// otherwise and for the tail
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void position_mean_bwd_k(const T* __restrict__ dlogits, T* __restrict__ dy, long long total,
                                                           long long PL, int L, double P) {
  constexpr int V = 16 / (int)sizeof(T);
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long long)gridDim.x * blockDim.x;
  const long long n_vec = VEC ? total - total % V : 0;
  if (VEC) {
    for (long long i = tid * V; i < n_vec; i += nthr * V) {
      alignas(16) T v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const long long j = i + e;
        v[e] = (T)((double)dlogits[(j / PL) * L + j % L] / P);
      }
      *reinterpret_cast<uint4*>(dy + i) = *reinterpret_cast<const uint4*>(v);
    }
  }
  for (long long j = n_vec + tid; j < total; j += nthr) dy[j] = (T)((double)dlogits[(j / PL) * L + j % L] / P);
}

// One record per tensor (include/dctn_amd.h)
struct TensorStatsRecord {
  long long n;
  double sum, sum_sq, sum_abs;
  float min_abs, max_abs;
  unsigned nonfinite, seq, ticket, reserved[3];
};
static_assert(sizeof(TensorStatsRecord) == 64, "the record is 64 bytes");

// blockIdx -> (tensor, block of that tensor): tensor i owns the workgroups first[i] .. first[i + 1] - 1
struct TensorStatsArgs {
  const void* ptr[TS_MAX_TENSORS];
  long long n[TS_MAX_TENSORS];
  unsigned first[TS_MAX_TENSORS + 1];
  unsigned char vec[TS_MAX_TENSORS];   // 1: the pointer is 16-byte aligned, four elements per access
  int n_tensors;
};

struct Moments {
  double sum = 0.0, sum_sq = 0.0, sum_abs = 0.0, min_abs = INFINITY, max_abs = 0.0, bad = 0.0;
  __device__ __forceinline__ void take(double v) {
    const double a = fabs(v);
    if (a < INFINITY) {   // false for NaN and for +-Inf
      sum += v;
      sum_sq = fma(v, v, sum_sq);
      sum_abs += a;
      min_abs = fmin(min_abs, a);
      max_abs = fmax(max_abs, a);
    } else {
      bad += 1.0;
    }
  }
  __device__ __forceinline__ void join(const Moments& o) {
    sum += o.sum, sum_sq += o.sum_sq, sum_abs += o.sum_abs;
    min_abs = fmin(min_abs, o.min_abs), max_abs = fmax(max_abs, o.max_abs), bad += o.bad;
  }
  __device__ __forceinline__ Moments shuffled_down(int off) const {
    Moments o;
    o.sum = __shfl_down(sum, off, 64), o.sum_sq = __shfl_down(sum_sq, off, 64), o.sum_abs = __shfl_down(sum_abs, off, 64);
    o.min_abs = __shfl_down(min_abs, off, 64), o.max_abs = __shfl_down(max_abs, off, 64), o.bad = __shfl_down(bad, off, 64);
    return o;
  }
  __device__ __forceinline__ Moments shuffled_xor(int off) const {
    Moments o;
    o.sum = __shfl_xor(sum, off, 64), o.sum_sq = __shfl_xor(sum_sq, off, 64), o.sum_abs = __shfl_xor(sum_abs, off, 64);
    o.min_abs = __shfl_xor(min_abs, off, 64), o.max_abs = __shfl_xor(max_abs, off, 64), o.bad = __shfl_xor(bad, off, 64);
    return o;
  }
};

__device__ __forceinline__ void ts_load4(const float* p, double (&x)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
}
__device__ __forceinline__ void ts_load4(const double* p, double (&x)[4]) {
  const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
  x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
}

// A lane owns the same four consecutive elements in both forms, so the record does not depend on the pointer's
// alignment: the aligned form reads them in 16-byte accesses, the other one element at a time.  The tail of n (fewer than
// four elements) goes one element per lane.
template <typename T>
__global__ __launch_bounds__(TS_THREADS) void tensor_stats_k(const TensorStatsArgs args, TensorStatsRecord* __restrict__ records,
                                                            double* __restrict__ workspace) {
  __shared__ double red[16][TS_SLOT];
  __shared__ int is_last;
  int ti = 0;
  while (ti + 1 < args.n_tensors && blockIdx.x >= args.first[ti + 1]) ++ti;
  const unsigned blk = blockIdx.x - args.first[ti], nblk = args.first[ti + 1] - args.first[ti];
  const T* __restrict__ x = (const T*)args.ptr[ti];
  const long long n = args.n[ti];
  const bool vec = args.vec[ti] != 0;
  TensorStatsRecord* rec = records + ti;
  double* slots = workspace + (size_t)ti * TS_MAX_BLOCKS * TS_SLOT;

  Moments m;
  const long long tid = (long long)blk * TS_THREADS + threadIdx.x, nthr = (long long)nblk * TS_THREADS;
  const long long n4 = n & ~3LL;
  for (long long i = tid * 4; i < n4; i += nthr * 4) {
    double v[4];
    if (vec) {
      ts_load4(x + i, v);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (double)x[i + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) m.take(v[e]);
  }
  for (long long i = n4 + tid; i < n; i += nthr) m.take((double)x[i]);

  for (int off = 32; off > 0; off >>= 1) m.join(m.shuffled_down(off));
  if ((threadIdx.x & 63) == 0) {
    double* r = red[threadIdx.x >> 6];
    r[0] = m.sum, r[1] = m.sum_sq, r[2] = m.sum_abs, r[3] = m.min_abs, r[4] = m.max_abs, r[5] = m.bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Moments t;
    for (int w = 0; w < TS_THREADS / 64; ++w) {
      Moments o;
      o.sum = red[w][0], o.sum_sq = red[w][1], o.sum_abs = red[w][2], o.min_abs = red[w][3], o.max_abs = red[w][4], o.bad = red[w][5];
      t.join(o);
    }
    // grad_guard_k's hand-over of the slot to whichever workgroup of this tensor turns out to be last: agent-scope
    // stores of the slot, an agent-scope release and an explicit wait BEFORE the ticket is drawn; the workgroup that
    // draws the last ticket makes an agent-scope acquire AFTER it and reads the slots with agent-scope loads.
    double* s = slots + (size_t)blk * TS_SLOT;
    __hip_atomic_store(&s[0], t.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s[1], t.sum_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s[2], t.sum_abs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s[3], t.min_abs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s[4], t.max_abs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s[5], t.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(&rec->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == nblk - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    is_last = last ? 1 : 0;
  }
  __syncthreads();
  if (is_last == 0 || threadIdx.x >= 64) return;   // every workgroup but the tensor's last ends here; nobody waits
  // the last workgroup's first wave: lane j joins slots j, j + 64, ... in that order, then one fixed butterfly
  Moments t;
  for (unsigned j = threadIdx.x; j < nblk; j += 64) {
    const double* s = slots + (size_t)j * TS_SLOT;
    Moments o;
    o.sum = __hip_atomic_load(&s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    o.sum_sq = __hip_atomic_load(&s[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    o.sum_abs = __hip_atomic_load(&s[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    o.min_abs = __hip_atomic_load(&s[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    o.max_abs = __hip_atomic_load(&s[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    o.bad = __hip_atomic_load(&s[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t.join(o);
  }
  for (int off = 32; off > 0; off >>= 1) t.join(t.shuffled_xor(off));
  if (threadIdx.x != 0) return;
  const unsigned seq = rec->seq;
  rec->n = n;
  rec->sum = t.sum, rec->sum_sq = t.sum_sq, rec->sum_abs = t.sum_abs;
  rec->min_abs = (float)t.min_abs, rec->max_abs = (float)t.max_abs;
  rec->nonfinite = (unsigned)t.bad;
  rec->seq = seq + 1u;
  rec->ticket = 0u;   // plain vector stores; the next launch starts from ticket 0 again
}

unsigned stats_blocks_for(long long n) {
  long long b = (n + 4095) / 4096;
  if (b > TS_MAX_BLOCKS) b = TS_MAX_BLOCKS;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

int dctn_position_mean_fwd(const void* y, void* out, int64_t B, int64_t P, int L, int dtype, void* stream) {
  if (!y || !out) return DCTN_ERR_NULL;
  if (B < 1 || P < 1 || B > 0x7fffffffLL) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64) return DCTN_ERR_BAD_DTYPE;
  if (L < 1 || L > PM_MAX_L) return DCTN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int R = PM_THREADS / L;
  const dim3 g((unsigned)B), b((unsigned)(R * L));
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL((position_mean_fwd_k<float>), g, b, 0, st, (const float*)y, (float*)out, (long long)P, L, R);
  else
    hipLaunchKernelGGL((position_mean_fwd_k<double>), g, b, 0, st, (const double*)y, (double*)out, (long long)P, L, R);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

int dctn_position_mean_bwd(const void* dlogits, void* dy, int64_t B, int64_t P, int L, int dtype, void* stream) {
  if (!dlogits || !dy) return DCTN_ERR_NULL;
  if (B < 1 || P < 1 || B > 0x7fffffffLL) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64) return DCTN_ERR_BAD_DTYPE;
  if (L < 1 || L > PM_MAX_L) return DCTN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long long PL = (long long)P * L, total = (long long)B * PL;
  const bool vec = (uintptr_t)dy % 16 == 0;
  const int V = dtype == DCTN_F32 ? 4 : 2;
  long long blocks = ((total + V - 1) / V + 255) / 256;
  if (blocks > (1 << 16)) blocks = 1 << 16;   // grid-stride beyond
  const dim3 g((unsigned)blocks), b(256);
#define DCTN_PM_BWD(T, VEC)                                                                                       \
  hipLaunchKernelGGL((position_mean_bwd_k<T, VEC>), g, b, 0, st, (const T*)dlogits, (T*)dy, total, PL, L, (double)P)
  if (dtype == DCTN_F32) {
    if (vec) DCTN_PM_BWD(float, true); else DCTN_PM_BWD(float, false);
  } else {
    if (vec) DCTN_PM_BWD(double, true); else DCTN_PM_BWD(double, false);
  }
#undef DCTN_PM_BWD
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

size_t dctn_tensor_stats_record_bytes(void) { return sizeof(TensorStatsRecord); }

size_t dctn_tensor_stats_workspace_bytes(int n_tensors) {
  return n_tensors < 1 ? 0 : (size_t)n_tensors * TS_MAX_BLOCKS * TS_SLOT * sizeof(double);
}

int dctn_tensor_stats(const void* const* tensors, const int64_t* counts, int n_tensors, void* records, void* workspace,
                      size_t workspace_bytes, int dtype, void* stream) {
  if (!tensors || !counts || !records || !workspace) return DCTN_ERR_NULL;
  if (n_tensors < 1 || n_tensors > TS_MAX_TENSORS) return DCTN_ERR_BAD_SHAPE;
  for (int i = 0; i < n_tensors; ++i)
    if (!tensors[i]) return DCTN_ERR_NULL;
  for (int i = 0; i < n_tensors; ++i)
    if (counts[i] < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64) return DCTN_ERR_BAD_DTYPE;
  if (workspace_bytes < dctn_tensor_stats_workspace_bytes(n_tensors)) return DCTN_ERR_WORKSPACE;
  TensorStatsArgs args = {};
  args.n_tensors = n_tensors;
  unsigned total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    args.ptr[i] = tensors[i];
    args.n[i] = counts[i];
    args.vec[i] = (uintptr_t)tensors[i] % 16 == 0;
    args.first[i] = total;
    total += stats_blocks_for(counts[i]);
  }
  for (int i = n_tensors; i <= TS_MAX_TENSORS; ++i) args.first[i] = total;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(total), b(TS_THREADS);
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL((tensor_stats_k<float>), g, b, 0, st, args, (TensorStatsRecord*)records, (double*)workspace);
  else
    hipLaunchKernelGGL((tensor_stats_k<double>), g, b, 0, st, args, (TensorStatsRecord*)records, (double*)workspace);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
