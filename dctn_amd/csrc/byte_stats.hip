// Statistics of a byte-resident data set, from the bytes: what the reference's colour loader computes from the EXPANDED
// training tensor before it builds a single batch (get_cifar10_colored_data_loaders, dctn/dataset_loading.py:349-375) -
// the per-channel mean and std (:351-352) and calc_scaling_factor's window statistics (:79-94) - for sources that keep the
// data set on the device as uint8 (batch_source.hip, colour_source.hip).  Nothing of the data set's size is expanded:
//   byte_histogram_k     (n_pixels, C) interleaved bytes -> int64 counts[C][256]; the moments are 256-term sums over them
//                        (dctn_amd/batches.py `moments_from_counts`).  Integer counters: exact, whatever the order.
//   byte_window_stats_k  the two sums of dctn_window_stats for the tensor a 256-row table per channel WOULD expand the bytes
//                        to.  One workgroup per image (phi_window_stats_k's structure); every workgroup STORES its pair of
//                        partial sums into its own slot, and the one that draws the last ticket (grad_guard.hip's hand-over)
//                        adds the slots in one fixed order.  No float atomic: the same input leaves the same bits on every
//                        launch, CU count and rank, so ranks that autoscale the same bytes build the same table.
#include "common.h"

#include <climits>

namespace {

constexpr int BYTE_THREADS = 256, BYTE_WAVES = BYTE_THREADS / DCTN_WAVE;
// What dctn_last_kernel reports for the two entry points.  Both write caller-owned buffers only through the C-ABI, like the
// batch sources; their guarded and poisoned runs are tests/test_gpu_colour_prepare.py's.
const char* const BYTE_KERNEL_NAMES[2] = {"byte_histogram", "byte_window_stats"};
// A workgroup's private counters are 32-bit.  It counts at most HIST_MAX_GROUPS groups of four pixels plus the six pixels
// in front of the first and behind the last group (workgroup 0), and a pixel adds one to ONE counter of a channel:
// no counter passes 4 * 2^29 + 6 < 2^32.
constexpr long long HIST_MAX_GROUPS = 1LL << 29;
// A fixed grid bound, no function of the device (as dctn_zero_async's): eight workgroups of 4 C KiB for each of a
// full card's 256 CUs; a smaller device runs them in turns, and the counts do not depend on who counts what.
constexpr long long HIST_MAX_WGS = 2048;

// src: `head` pixels (< 4), then `groups` groups of four pixels, then `tail` pixels (< 4).  VEC: the first group starts on
// a 4-byte boundary and a group's 4 C bytes are C 32-bit loads (colour_k's form); otherwise byte loads.  Workgroup b owns
// groups [b * per_wg, (b + 1) * per_wg); workgroup 0 also counts the head and the tail.  Every wave has counters of its
// own (4 C KiB of LDS a workgroup), so that pixels of one value - a saturated image - serialise within a wave only.
template <int C, bool VEC>
__global__ __launch_bounds__(BYTE_THREADS) void byte_histogram_k(const unsigned char* __restrict__ src, unsigned head,
                                                                long long groups, unsigned tail, long long per_wg,
                                                                unsigned long long* __restrict__ counts) {
  __shared__ unsigned cnt[BYTE_WAVES][C][256];
  for (int i = threadIdx.x; i < BYTE_WAVES * C * 256; i += BYTE_THREADS) (&cnt[0][0][0])[i] = 0u;
  __syncthreads();
  unsigned (*mine)[256] = cnt[threadIdx.x / DCTN_WAVE];
  const unsigned char* body = src + (size_t)head * C;
  const long long g0 = (long long)blockIdx.x * per_wg;
  const long long g1 = g0 + per_wg < groups ? g0 + per_wg : groups;
  for (long long g = g0 + threadIdx.x; g < g1; g += BYTE_THREADS) {
    if (VEC) {
      unsigned w[C];
#pragma unroll
      for (int c = 0; c < C; ++c) w[c] = reinterpret_cast<const unsigned*>(body)[(size_t)g * C + c];
#pragma unroll
      for (int k = 0; k < 4 * C; ++k) atomicAdd(&mine[k % C][(w[k / 4] >> (8 * (k % 4))) & 255u], 1u);
    } else {
#pragma unroll
      for (int k = 0; k < 4 * C; ++k) atomicAdd(&mine[k % C][body[(size_t)g * 4 * C + k]], 1u);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < head + tail) {   // at most six pixels, one per lane
    const size_t p = threadIdx.x < head ? (size_t)threadIdx.x : (size_t)head + 4 * (size_t)groups + (threadIdx.x - head);
#pragma unroll
    for (int c = 0; c < C; ++c) atomicAdd(&mine[c][src[p * C + c]], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * 256; i += BYTE_THREADS) {
    unsigned long long v = 0ull;
#pragma unroll
    for (int w = 0; w < BYTE_WAVES; ++w) v += (&cnt[w][0][0])[i];
    if (v) atomicAdd(&counts[i], v);   // 64-bit integer atomic: exact in any order
  }
}

struct HistPlan { unsigned head, tail; long long groups, per_wg; unsigned wgs; bool vec; };

// `head`: the pixels in front of the first pixel that starts on a 4-byte boundary (src + head * C = 0 mod 4 has a solution
// below 4 for every address when C is odd, for even addresses when C = 2, for aligned ones when C = 4); none, or fewer
// pixels than that: byte loads throughout
HistPlan hist_plan(const void* src, long long n_pixels, int C) {
  HistPlan p = {};
  int head = -1;
  for (int h = 0; h < 4 && head < 0; ++h)
    if (((uintptr_t)src + (uintptr_t)(h * C)) % 4u == 0u) head = h;
  p.vec = head >= 0 && head <= n_pixels;
  p.head = p.vec ? (unsigned)head : 0u;
  p.groups = (n_pixels - p.head) / 4;
  p.tail = (unsigned)(n_pixels - p.head - 4 * p.groups);
  long long wgs = (p.groups + 8 * BYTE_THREADS - 1) / (8 * BYTE_THREADS);   // eight groups a lane before a second workgroup
  if (wgs > HIST_MAX_WGS) wgs = HIST_MAX_WGS;
  if (wgs < 1) wgs = 1;
  p.per_wg = (p.groups + wgs - 1) / wgs;
  if (p.per_wg > HIST_MAX_GROUPS) {   // the 32-bit counters' bound decides, not the device
    p.per_wg = HIST_MAX_GROUPS;
    wgs = (p.groups + p.per_wg - 1) / p.per_wg;
  }
  p.wgs = (unsigned)wgs;
  return p;
}

template <int C>
void hist_launch(const void* src, const HistPlan& p, void* counts, hipStream_t st) {
  const dim3 g(p.wgs), b(BYTE_THREADS);
  if (p.vec)
    hipLaunchKernelGGL((byte_histogram_k<C, true>), g, b, 0, st, (const unsigned char*)src, p.head, p.groups, p.tail,
                       p.per_wg, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL((byte_histogram_k<C, false>), g, b, 0, st, (const unsigned char*)src, p.head, p.groups, p.tail,
                       p.per_wg, (unsigned long long*)counts);
}

// ------------------------------------------------------------------------------------------------ window statistics
struct __attribute__((aligned(16))) TU { double t, u; };   // 16 bytes: one LDS read of a lookup

// workspace: n slots {sum_w prod t, sum_w prod u} of the images, then the ticket block
constexpr size_t BWS_TICKET_BYTES = 16, BWS_TAIL_BYTES = 2 * BYTE_WAVES * sizeof(double) + 16;
size_t bws_workspace_bytes(long long n) { return (size_t)n * sizeof(TU) + BWS_TICKET_BYTES; }

// LDS, all of it dynamic so that its base stays 16-byte aligned: tab[C][256] as it lies in global memory, the image's
// pix[H * W], then the eight wave sums and the last-ticket flag (BWS_TAIL_BYTES).  A lookup reads the 16 bytes of one (channel,
// byte value) - four neighbouring banks starting at 4 * value mod 64 - so byte values that differ by a multiple of 16 meet;
// independent pixels conflict at random in any layout (colour_source.hip), and two planes of 8 bytes would pay them twice.
// A pixel's pair is t0 + tab[0][b_0].t + tab[1][b_1].t + ..., channels ascending; a window's terms are the products over
// its pixels, rows then columns; a lane adds its windows w = lane, lane + 256, ... in that order, a wave its lanes by one
// butterfly, the workgroup its four waves as ((0 + 1) + (2 + 3)): nothing of it depends on the launch.
template <int C>
__global__ __launch_bounds__(BYTE_THREADS) void byte_window_stats_k(const unsigned char* __restrict__ src,
                                                                   const double* __restrict__ tu, double t0, double u0,
                                                                   int H, int W, int K, double* __restrict__ partials,
                                                                   unsigned* __restrict__ ticket,
                                                                   double* __restrict__ sums) {
  extern __shared__ __attribute__((aligned(16))) unsigned char byte_lds[];
  TU* tab = reinterpret_cast<TU*>(byte_lds);
  TU* pix = tab + C * 256;
  double (*red)[BYTE_WAVES] = reinterpret_cast<double (*)[BYTE_WAVES]>(pix + H * W);
  unsigned& last_flag = *reinterpret_cast<unsigned*>(red + 2);
  for (int i = threadIdx.x; i < C * 256; i += BYTE_THREADS) tab[i] = TU{tu[2 * i], tu[2 * i + 1]};
  __syncthreads();
  const int P = H * W;
  const unsigned char* im = src + (size_t)blockIdx.x * P * C;   // any alignment: byte loads (3 KiB an image at 32 x 32 x 3)
  for (int i = threadIdx.x; i < P; i += BYTE_THREADS) {
    double t = t0, u = u0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const TU e = tab[c * 256 + im[(size_t)i * C + c]];
      t += e.t;
      u += e.u;
    }
    pix[i] = TU{t, u};
  }
  __syncthreads();
  const int Ho = H - K + 1, Wo = W - K + 1;
  double s_sum = 0.0, s_sq = 0.0;
  for (int w = threadIdx.x; w < Ho * Wo; w += BYTE_THREADS) {
    const int ho = w / Wo, wo = w - ho * Wo;
    double ps = 1.0, pq = 1.0;
    for (int dh = 0; dh < K; ++dh)
      for (int dw = 0; dw < K; ++dw) {
        const TU e = pix[(ho + dh) * W + wo + dw];
        ps *= e.t;
        pq *= e.u;
      }
    s_sum += ps;
    s_sq += pq;
  }
  s_sum = wave_reduce_sum(s_sum);
  s_sq = wave_reduce_sum(s_sq);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[0][wv] = s_sum; red[1][wv] = s_sq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    // grad_guard.hip's hand-over: the slot leaves this CU's caches (agent-scope stores), a release and an explicit wait
    // come BEFORE the ticket is drawn, the workgroup that draws the last ticket makes an acquire AFTER it
    __hip_atomic_store(&partials[2 * blockIdx.x], (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&partials[2 * blockIdx.x + 1], (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    last_flag = last ? 1u : 0u;
  }
  __syncthreads();
  if (last_flag == 0u) return;   // every workgroup but the last ends here; nobody waits
  // The last workgroup adds the n slots in image order within a lane - lane j takes images j, j + 256, ... - then by the
  // same butterfly and the same wave order as above: one order for a given n.
  double a = 0.0, b = 0.0;
  for (unsigned j = threadIdx.x; j < gridDim.x; j += BYTE_THREADS) {
    a += __hip_atomic_load(&partials[2 * j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b += __hip_atomic_load(&partials[2 * j + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  a = wave_reduce_sum(a);
  b = wave_reduce_sum(b);   // (thread 0 read `red` in front of the barrier that published the flag: free again)
  if (lane == 0) { red[0][wv] = a; red[1][wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    sums[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

template <int C>
int bws_launch(const void* src, const void* tu, double t0, double u0, long long n, int H, int W, int K, size_t lds,
                void* workspace, void* sums, hipStream_t st) {
  if (!dctn_lds_optin((const void*)byte_window_stats_k<C>, lds)) return DCTN_ERR_UNSUPPORTED;
  unsigned* ticket = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(workspace) + (size_t)n * sizeof(TU));
  if (dctn_zero_async(ticket, BWS_TICKET_BYTES, st) != DCTN_OK) return DCTN_ERR_LAUNCH;
  hipLaunchKernelGGL((byte_window_stats_k<C>), dim3((unsigned)n), dim3(BYTE_THREADS), lds, st, (const unsigned char*)src,
                     (const double*)tu, t0, u0, H, W, K, (double*)workspace, ticket, (double*)sums);
  return DCTN_OK;
}

}  // namespace

extern "C" {

int dctn_byte_histogram(const void* src, int64_t n_pixels, int channels, void* counts, void* stream) {
  if (!src || !counts) return DCTN_ERR_NULL;
  if (n_pixels < 1 || channels < 1 || channels > 4) return DCTN_ERR_BAD_SHAPE;
  if ((uintptr_t)counts % 8u) return DCTN_ERR_UNSUPPORTED;   // 64-bit atomics
  hipStream_t st = (hipStream_t)stream;
  const HistPlan p = hist_plan(src, n_pixels, channels);
  if (dctn_zero_async(counts, (size_t)channels * 256 * sizeof(int64_t), st) != DCTN_OK) return DCTN_ERR_LAUNCH;
  switch (channels) {
    case 1: hist_launch<1>(src, p, counts, st); break;
    case 2: hist_launch<2>(src, p, counts, st); break;
    case 3: hist_launch<3>(src, p, counts, st); break;
    default: hist_launch<4>(src, p, counts, st); break;
  }
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel(BYTE_KERNEL_NAMES[0]);
  return DCTN_OK;
}

size_t dctn_byte_window_stats_workspace_bytes(int64_t n) { return n < 1 ? 0 : bws_workspace_bytes(n); }

int dctn_byte_window_stats(const void* src, int64_t n, int H, int W, int channels, const void* tu, double t0, double u0,
                           int K, void* workspace, void* sums, void* stream) {
  if (!src || !tu || !workspace || !sums) return DCTN_ERR_NULL;
  if (n < 1 || n > INT_MAX || channels < 1 || channels > 4 || K < 1 || H < K || W < K) return DCTN_ERR_BAD_SHAPE;
  const size_t lds = ((size_t)channels * 256 + (size_t)H * W) * sizeof(TU) + BWS_TAIL_BYTES;
  if (lds > (size_t)dctn_lds_wg_max() || (uintptr_t)tu % 8u || (uintptr_t)workspace % 8u || (uintptr_t)sums % 8u)
    return DCTN_ERR_UNSUPPORTED;   // table + pairs beyond a workgroup's LDS (the device's: dctn_device_limits)
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (channels) {
    case 1: rc = bws_launch<1>(src, tu, t0, u0, n, H, W, K, lds, workspace, sums, st); break;
    case 2: rc = bws_launch<2>(src, tu, t0, u0, n, H, W, K, lds, workspace, sums, st); break;
    case 3: rc = bws_launch<3>(src, tu, t0, u0, n, H, W, K, lds, workspace, sums, st); break;
    default: rc = bws_launch<4>(src, tu, t0, u0, n, H, W, K, lds, workspace, sums, st); break;
  }
  if (rc != DCTN_OK) return rc;
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel(BYTE_KERNEL_NAMES[1]);
  return DCTN_OK;
}

}  // extern "C"
