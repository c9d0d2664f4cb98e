// Histograms of up to 8 tensors in ONE launch, over a caller-given table of bin edges (dctn_tensor_hist) - what the
// reference's runner logs per string through `writer.add_histogram` (mnist.py:537-553, log_dumb_histogram), over
// TensorBoard's own bucket set or any other strictly increasing float64 table of 2..2048 edges.
//
// The partition is dctn_tensor_stats' (sbs_tail.hip): tensor i is read by min(256, ceil(n / 4096)) workgroups of 1024
// threads, blockIdx -> (tensor, block) through a `first[]` table that travels in the kernel argument.
//
// Why this kernel may use atomics where tensor_stats_k may not.  Everything a block accumulates is an INTEGER SUM (the
// bin counts and the six counters) or a MAX (the order-preserving keys of the largest finite value and of the complement
// of the smallest).  Integer addition and max are associative and commutative without rounding, so the block's bits are a
// function of the values seen and of nothing else - not of the order in which lanes, waves or workgroups arrive.
// tensor_stats_k sums float64, which rounds, and therefore stores slots and adds them in one fixed order; here a
// fixed-order slab would buy nothing, and the workgroups add straight into the block with no-return 64-bit atomics.
//
// A workgroup
//   1. reads the block's `calls` (one lane, agent scope) and broadcasts it through LDS: the launch is RECORDED iff
//      calls % period == 0; a workgroup of a skipped launch reads no element and no edge and goes to 4;
//   2. copies the edge table into LDS, zeroes its LDS counts and finds every element's bin by a binary search over the
//      table in LDS: the number of edges <= v, found by comparisons of float64 values alone (a float32 element is widened
//      exactly), so the bin satisfies edges[i] <= v < edges[i + 1] by construction and no logarithm decides anything.
//      Bins are counted with 32-bit LDS atomics into TH_REPLICAS interleaved sub-histograms (lane % TH_REPLICAS picks
//      one), so that the lanes of a wave that share a bin - all of them, for a constant tensor - spread over four words;
//   3. adds its non-zero bins, its counters and its two keys to the block (no-return agent-scope atomics) and waits for
//      them;
//   4. draws the block's ticket.  The workgroup that draws the tensor's last ticket adds 1 to `calls`, adds 1 to
//      `recorded` if the launch counted and stores ticket = 0.  Every workgroup has consumed `calls` before it draws, and
//      the last ticket exists only after all have drawn: no workgroup can see the advanced value, and none waits for
//      another.
#include "common.h"

#include <cmath>

#ifndef TH_REPLICAS
#define TH_REPLICAS 4        // sub-histograms per workgroup, interleaved per bin (a power of two)
#endif
// 1: a wave whose lanes all hit one bin makes one LDS add of their number.  Built and measured: with four replicas it
// loses 0.4 - 0.8 us on every input, a constant tensor included
#ifndef TH_WAVE_UNIFORM
#define TH_WAVE_UNIFORM 0
#endif

namespace {

constexpr int TH_MAX_TENSORS = 8;
constexpr int TH_MAX_BLOCKS = 256;   // workgroups per tensor: min(256, ceil(n / 4096))
constexpr int TH_THREADS = 1024;
constexpr int TH_MAX_EDGES = 2048;
constexpr int TH_DEPTH = 4;          // 16-byte-per-lane turns in flight: a workgroup takes 4096 x 4 elements per round
constexpr long long TH_MAX_COUNT = 1LL << 39;   // a workgroup's 32-bit LDS counts then stay below 2^31
constexpr int TH_COUNTERS = 6;       // total, below, above, nan, pos_inf, neg_inf: the header's order

// The header of one block (include/dctn_amd.h); n_edges - 1 uint64 counts follow
struct TensorHistHeader {
  unsigned long long total, below, above, nan, pos_inf, neg_inf;
  unsigned long long max_key;     // key of the largest finite value; 0: none yet
  unsigned long long min_key_c;   // ~key of the smallest finite value; 0: none yet
  unsigned calls, recorded, ticket, reserved;
};
static_assert(sizeof(TensorHistHeader) == 80, "the header is 80 bytes");

struct TensorHistArgs {
  const void* ptr[TH_MAX_TENSORS];
  long long n[TH_MAX_TENSORS];
  unsigned first[TH_MAX_TENSORS + 1];
  unsigned char vec[TH_MAX_TENSORS];   // 1: the pointer is 16-byte aligned, four elements per access
  int n_tensors;
};

// float64 -> uint64 whose unsigned order is the values' order; no finite value maps to 0 or to ~0
__device__ __forceinline__ unsigned long long th_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

__device__ __forceinline__ void th_load4(const float* p, double (&x)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
}
__device__ __forceinline__ void th_load4(const double* p, double (&x)[4]) {
  const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
  x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
}

// What a lane keeps in registers between its elements
struct LaneTally {
  unsigned c[TH_COUNTERS] = {0, 0, 0, 0, 0, 0};
  double lo = INFINITY, hi = -INFINITY;
};

// One element: the counters and the range go to the lane's registers, the bin to LDS.  Returns the bin, or -1 for an
// element that has none (outside the table, or not finite).
__device__ __forceinline__ int th_classify(double v, const double* __restrict__ edges, int n_edges, LaneTally& t) {
  t.c[0] += 1u;
  if (v != v) { t.c[3] += 1u; return -1; }
  if (v == INFINITY) { t.c[4] += 1u; return -1; }
  if (v == -INFINITY) { t.c[5] += 1u; return -1; }
  v += 0.0;   // -0.0 is 0.0, in the range as well
  t.lo = fmin(t.lo, v), t.hi = fmax(t.hi, v);
  int lo = 0, hi = n_edges;   // the number of edges <= v lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= v) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) { t.c[1] += 1u; return -1; }                 // v < edges[0]
  if (lo == n_edges) {                                      // edges[n_edges - 1] <= v: the last bin is closed on the right
    if (v == edges[n_edges - 1]) return n_edges - 2;
    t.c[2] += 1u;
    return -1;
  }
  return lo - 1;                                            // edges[lo - 1] <= v < edges[lo]
}

// The LDS add of one element's bin; every lane of the wave that is active here calls it together
__device__ __forceinline__ void th_count(unsigned* __restrict__ counts, int bin, int lane) {
#if TH_WAVE_UNIFORM
  const unsigned long long have = __ballot(bin >= 0);
  if (have == 0) return;
  const int src = __ffsll((long long)have) - 1;
  const int b0 = __shfl(bin, src, 64);
  if (__ballot(bin == b0) == have) {   // every lane that has a bin has this one (lanes without one hold -1 != b0)
    if (lane == src) atomicAdd(&counts[b0 * TH_REPLICAS], (unsigned)__popcll(have));
    return;
  }
#endif
  if (bin >= 0) atomicAdd(&counts[bin * TH_REPLICAS + (lane & (TH_REPLICAS - 1))], 1u);
}

// A lane owns the same four consecutive elements in both forms of the load, so nothing depends on the pointer's alignment
template <typename T>
__global__ __launch_bounds__(TH_THREADS) void tensor_hist_k(const TensorHistArgs args, unsigned char* __restrict__ blocks,
                                                           const double* __restrict__ edges_g, int n_edges, unsigned period,
                                                           size_t block_bytes) {
  __shared__ double edges[TH_MAX_EDGES];
  __shared__ unsigned counts[(TH_MAX_EDGES - 1) * TH_REPLICAS];
  __shared__ unsigned long long wg_counter[TH_COUNTERS];
  __shared__ unsigned long long wg_key[2];
  __shared__ unsigned wg_calls;
  __shared__ int is_last;
  int ti = 0;
  while (ti + 1 < args.n_tensors && blockIdx.x >= args.first[ti + 1]) ++ti;
  const unsigned blk = blockIdx.x - args.first[ti], nblk = args.first[ti + 1] - args.first[ti];
  TensorHistHeader* hdr = reinterpret_cast<TensorHistHeader*>(blocks + (size_t)ti * block_bytes);
  unsigned long long* bins_g = reinterpret_cast<unsigned long long*>(hdr + 1);
  const int n_bins = n_edges - 1, lane = threadIdx.x & 63;

  if (threadIdx.x == 0) wg_calls = __hip_atomic_load(&hdr->calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const unsigned calls = wg_calls;
  const bool counted = calls % period == 0;   // the same answer in every workgroup of the tensor: see the header comment

  if (counted) {
    for (int i = threadIdx.x; i < n_edges; i += TH_THREADS) edges[i] = edges_g[i];
    for (int i = threadIdx.x; i < n_bins * TH_REPLICAS; i += TH_THREADS) counts[i] = 0u;
    if (threadIdx.x < TH_COUNTERS) wg_counter[threadIdx.x] = 0ull;
    if (threadIdx.x < 2) wg_key[threadIdx.x] = 0ull;
    __syncthreads();

    const T* __restrict__ x = (const T*)args.ptr[ti];
    const long long n = args.n[ti];
    const bool vec = args.vec[ti] != 0;
    const long long tid = (long long)blk * TH_THREADS + threadIdx.x, nthr = (long long)nblk * TH_THREADS;
    const long long n4 = n & ~3LL;
    LaneTally tally;
    for (long long base = tid * 4; base < n4; base += nthr * 4 * TH_DEPTH) {
      double v[TH_DEPTH][4];
#pragma unroll
      for (int u = 0; u < TH_DEPTH; ++u) {
        const long long i = base + (long long)u * nthr * 4;
        if (i < n4) {
          if (vec) {
            th_load4(x + i, v[u]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = (double)x[i + e];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < TH_DEPTH; ++u) {
        if (base + (long long)u * nthr * 4 < n4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) th_count(counts, th_classify(v[u][e], edges, n_edges, tally), lane);
        }
      }
    }
    for (long long i = n4 + tid; i < n; i += nthr) th_count(counts, th_classify((double)x[i], edges, n_edges, tally), lane);

    // the lanes' counters and range: a wave butterfly, then one LDS atomic per wave and field
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < TH_COUNTERS; ++k) tally.c[k] += __shfl_xor(tally.c[k], off, 64);
      tally.lo = fmin(tally.lo, __shfl_xor(tally.lo, off, 64));
      tally.hi = fmax(tally.hi, __shfl_xor(tally.hi, off, 64));
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < TH_COUNTERS; ++k)
        if (tally.c[k] != 0u) atomicAdd(&wg_counter[k], (unsigned long long)tally.c[k]);
      if (tally.lo <= tally.hi) {   // the wave saw a finite value
        atomicMax(&wg_key[0], th_key(tally.hi));
        atomicMax(&wg_key[1], ~th_key(tally.lo));
      }
    }
    __syncthreads();

    // the flush: non-zero bins, counters and keys, no-return atomics into the block
    for (int b = threadIdx.x; b < n_bins; b += TH_THREADS) {
      unsigned c = 0u;
#pragma unroll
      for (int r = 0; r < TH_REPLICAS; ++r) c += counts[b * TH_REPLICAS + r];
      if (c != 0u) __hip_atomic_fetch_add(&bins_g[b], (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x < TH_COUNTERS) {
      const unsigned long long c = wg_counter[threadIdx.x];
      if (c != 0ull) __hip_atomic_fetch_add(&hdr->total + threadIdx.x, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (threadIdx.x < TH_COUNTERS + 2) {
      const unsigned long long k = wg_key[threadIdx.x - TH_COUNTERS];
      if (k != 0ull) __hip_atomic_fetch_max(&hdr->max_key + (threadIdx.x - TH_COUNTERS), k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // every add of this workgroup has been performed before its ticket is drawn, so all adds of the launch have been
    // performed before the last workgroup writes the header's three words
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  if (threadIdx.x == 0) {
    const unsigned drawn = __hip_atomic_fetch_add(&hdr->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last = drawn == nblk - 1 ? 1 : 0;
  }
  __syncthreads();
  if (is_last == 0 || threadIdx.x != 0) return;   // every workgroup but the tensor's last ends here; nobody waits
  if (counted) {
    const unsigned recorded = __hip_atomic_load(&hdr->recorded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&hdr->recorded, recorded + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(&hdr->calls, calls + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&hdr->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch draws from 0 again
}

// Everything of a block but `calls` (the period's phase survives a read) and the ticket (0 between launches)
__global__ __launch_bounds__(256) void tensor_hist_reset_k(unsigned char* __restrict__ blocks, int n_edges, size_t block_bytes) {
  TensorHistHeader* hdr = reinterpret_cast<TensorHistHeader*>(blocks + (size_t)blockIdx.y * block_bytes);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(hdr);
  constexpr int head_words = (int)(offsetof(TensorHistHeader, calls) / 8);   // the counters and the two keys
  const int n_words = (int)(sizeof(TensorHistHeader) / 8) + n_edges - 1;
  for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += gridDim.x * blockDim.x) {
    if (w < head_words || w >= (int)(sizeof(TensorHistHeader) / 8)) words[w] = 0ull;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr->recorded = 0u;
}

unsigned hist_blocks_for(long long n) {
  long long b = (n + 4095) / 4096;
  if (b > TH_MAX_BLOCKS) b = TH_MAX_BLOCKS;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

size_t dctn_tensor_hist_block_bytes(int n_edges) {
  return n_edges < 2 ? 0 : sizeof(TensorHistHeader) + (size_t)(n_edges - 1) * sizeof(unsigned long long);
}

int dctn_tensor_hist(const void* const* tensors, const int64_t* counts, int n_tensors, const void* edges, int n_edges,
                     void* blocks, int period, int dtype, void* stream) {
  if (!tensors || !counts || !edges || !blocks) return DCTN_ERR_NULL;
  if (n_tensors < 1 || n_tensors > TH_MAX_TENSORS) return DCTN_ERR_BAD_SHAPE;
  for (int i = 0; i < n_tensors; ++i)
    if (!tensors[i]) return DCTN_ERR_NULL;
  for (int i = 0; i < n_tensors; ++i)
    if (counts[i] < 1) return DCTN_ERR_BAD_SHAPE;
  if (n_edges < 2 || n_edges > TH_MAX_EDGES || period < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64) return DCTN_ERR_BAD_DTYPE;
  for (int i = 0; i < n_tensors; ++i)
    if (counts[i] > TH_MAX_COUNT) return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)edges % 8 != 0 || (uintptr_t)blocks % 8 != 0) return DCTN_ERR_UNSUPPORTED;
  TensorHistArgs args = {};
  args.n_tensors = n_tensors;
  unsigned total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    args.ptr[i] = tensors[i];
    args.n[i] = counts[i];
    args.vec[i] = (uintptr_t)tensors[i] % 16 == 0;
    args.first[i] = total;
    total += hist_blocks_for(counts[i]);
  }
  for (int i = n_tensors; i <= TH_MAX_TENSORS; ++i) args.first[i] = total;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(total), b(TH_THREADS);
  const size_t block_bytes = dctn_tensor_hist_block_bytes(n_edges);
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL((tensor_hist_k<float>), g, b, 0, st, args, (unsigned char*)blocks, (const double*)edges, n_edges,
                       (unsigned)period, block_bytes);
  else
    hipLaunchKernelGGL((tensor_hist_k<double>), g, b, 0, st, args, (unsigned char*)blocks, (const double*)edges, n_edges,
                       (unsigned)period, block_bytes);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

int dctn_tensor_hist_reset(void* blocks, int n_tensors, int n_edges, void* stream) {
  if (!blocks) return DCTN_ERR_NULL;
  if (n_tensors < 1 || n_edges < 2 || n_edges > TH_MAX_EDGES) return DCTN_ERR_BAD_SHAPE;
  if (n_tensors > 65535 || (uintptr_t)blocks % 8 != 0) return DCTN_ERR_UNSUPPORTED;
  const dim3 g(8, (unsigned)n_tensors), b(256);
  hipLaunchKernelGGL(tensor_hist_reset_k, g, b, 0, (hipStream_t)stream, (unsigned char*)blocks, n_edges,
                     dctn_tensor_hist_block_bytes(n_edges));
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
