// What the reference's TensorBoard hooks read off the BATCH, in ONE launch (dctn_batch_monitor): the input statistics
// (mnist.py:298-311 and :571-591: mean and std of the quantum batch, std_of_coordinates_of_windows of its K x K windows as
// rank-one tensors), the whole model's output (mnist.py:555-569: signed min, max, mean, std of the logits and the
// histogram of softmax(logits, dim=1)) and the per-sample confidence (new_runner.py:512-531, --tb-batches: the probability
// every sample gives its true class, beside the sample indices) - with a period counted on the device and a ring of rows
// in a caller-owned block, as dctn_param_stats has them.
//
// The plan.  B + 1 workgroups of 256 threads: a function of B alone.
//   Workgroup b < B is sample b's INPUT part.  Thread t owns the (channel, pixel) pairs i = t, t + 256, ... of the
//   sample's C H W (i = c H W + h W + w) and walks the Q values of each in index order: a finite value v adds v to x_sum
//   and v * v to x_sum_sq (one fma), any other counts in x_nonfinite; EVERY value, finite or not, enters the pair
//   (s, u) = (sum_q v, sum_q v^2), which is staged in LDS when K > 0.  Thread t then owns the windows w = t, t + 256, ...
//   (w = ho Wo + wo) and forms each one's two products over (dh, dw, c), c innermost, from the staged pairs.  The five
//   partial values go through one fixed tree - lanes by shuffles at distances 32 .. 1, the four waves in index order - into
//   the workgroup's 40-byte slot of the workspace.
//   Workgroup B is the LOGITS part, and writes its piece of the row directly (the row's index is known at entry: `recorded`
//   moves only after the launch's last ticket).  It takes the rows in chunks of 256, thread t the row chunk + t: one pass
//   for the finite sum, sum of squares, min, max, non-finite count and the argmax (the lowest index among equal maxima),
//   then, for a row without a non-finite logit, S = sum_j exp(z_j - m) in increasing j and p_j = exp(z_j - m) / S, all
//   in float64; every p_j is binned by comparisons against the table (numpy.histogram's rule) into 32-bit counters in
//   LDS.  The rows' partial values are then added IN ROW ORDER, one thread per quantity.
//   The workgroup that draws the launch's last ticket adds the B slots IN SAMPLE ORDER, one thread per quantity, writes
//   the input piece of the row, `seq` last, and advances the header.
//
// Reproducible bits.  Every float sum has an order fixed by the shapes alone, the counters are integers: the same values
// leave the same row bytes on every launch, device and CU count, whatever the workspace held.  The hand-over is
// param_stats_k's (slots, agent-scope release, ticket, agent-scope acquire); no workgroup waits for another.  A launch
// that is not recorded (calls % period != 0) reads no element: its workgroups draw the ticket and end.
#include "common.h"

#include <math.h>

namespace {

constexpr int BM_THREADS = 256, BM_WAVES = BM_THREADS / DCTN_WAVE;
constexpr int BM_MAX_LABELS = 1024, BM_MAX_EDGES = 2048;
constexpr long long BM_MAX_BATCH = 0x7ffffffeLL;   // B + 1 workgroups in one grid dimension

struct BMHeader {
  unsigned calls, recorded, ticket, reserved[5];
};
static_assert(sizeof(BMHeader) == 32, "the header is 32 bytes");
// a row's fixed part (include/dctn_amd.h); behind it counts[n_edges - 1] padded to 8 bytes, label[B], index[B], p_true[B],
// pred[B]
struct BMRowHead {
  unsigned call, seq, rows, correct, bad_rows, z_nonfinite;
  unsigned long long x_nonfinite;
  double x_sum, x_sum_sq, win_sum, win_sq;
  double z_sum, z_sum_sq, z_min, z_max;
  unsigned below, above, nan, reserved;
};
static_assert(sizeof(BMRowHead) == 112, "a row starts with 112 bytes");
struct BMSlot {
  double x_sum, x_sum_sq, win_sum, win_sq;
  unsigned long long nonfinite;
};
static_assert(sizeof(BMSlot) == 40, "a sample's slot is 40 bytes");
struct __attribute__((aligned(16))) BMPair { double s, u; };

// LDS, all of it dynamic (its base stays 16-byte aligned): the flags, the chunk table [5][256] of the two in-order sums,
// the four waves' partial values, then the role's own: the sample's pairs, or the histogram's counters
constexpr size_t BM_FLAG_BYTES = 16, BM_CHUNK_BYTES = 5 * BM_THREADS * sizeof(double), BM_RED_BYTES = 5 * BM_WAVES * sizeof(double);
constexpr size_t BM_FIXED_LDS = BM_FLAG_BYTES + BM_CHUNK_BYTES + BM_RED_BYTES;
static_assert(BM_FIXED_LDS % 16 == 0, "the role's part starts on 16 bytes");

size_t counts_bytes(int n_edges) { return ((size_t)(n_edges - 1) * 4 + 7) & ~(size_t)7; }
size_t row_bytes(long long B, int n_edges) { return sizeof(BMRowHead) + counts_bytes(n_edges) + 24 * (size_t)B; }
size_t lds_bytes(int C, int H, int W, int K, int n_edges) {
  const size_t pairs = K > 0 ? (size_t)C * H * W * sizeof(BMPair) : 0;
  const size_t counters = ((size_t)(n_edges + 2) * 4 + 15) & ~(size_t)15;   // the bins, then below, above, nan
  return BM_FIXED_LDS + (pairs > counters ? pairs : counters);
}

struct BMArgs {
  const void *x, *logits;
  const long long *y, *indices;
  const double* edges;
  unsigned char* block;
  BMSlot* slots;
  long long B;
  int C, H, W, Q, K, L, n_edges;
  unsigned period, capacity;
};

typedef unsigned short bf16_bits;   // a bfloat16 element as the kernel reads it: the upper half of a float32

__device__ __forceinline__ double bm_widen(float x) { return (double)x; }
__device__ __forceinline__ double bm_widen(double x) { return x; }
__device__ __forceinline__ double bm_widen(bf16_bits x) { return (double)__uint_as_float((unsigned)x << 16); }

__device__ __forceinline__ bool bm_finite(double v) { return fabs(v) < INFINITY; }   // false for NaN and for +-Inf

// lanes by shuffles at distances 32 .. 1: lane 0 holds the wave's value
__device__ __forceinline__ double bm_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// TX: the element of x, TZ: the element of logits
template <typename TX, typename TZ>
__global__ __launch_bounds__(BM_THREADS) void batch_monitor_k(const BMArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bm_lds[];
  unsigned* flags = reinterpret_cast<unsigned*>(bm_lds);   // calls, recorded, is_last
  double (*chunk)[BM_THREADS] = reinterpret_cast<double (*)[BM_THREADS]>(bm_lds + BM_FLAG_BYTES);
  unsigned long long* chunk_bits = reinterpret_cast<unsigned long long*>(chunk[4]);
  double (*red)[BM_WAVES] = reinterpret_cast<double (*)[BM_WAVES]>(bm_lds + BM_FLAG_BYTES + BM_CHUNK_BYTES);
  unsigned char* own = bm_lds + BM_FIXED_LDS;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  BMHeader* hdr = reinterpret_cast<BMHeader*>(a.block);

  if (t == 0) {
    flags[0] = __hip_atomic_load(&hdr->calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flags[1] = __hip_atomic_load(&hdr->recorded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const unsigned calls = flags[0], recorded = flags[1];
  const bool counted = calls % a.period == 0;   // the same answer in every workgroup: `calls` moves after the last ticket
  const long long B = a.B;
  const size_t cbytes = ((size_t)(a.n_edges - 1) * 4 + 7) & ~(size_t)7;
  unsigned char* row = a.block + sizeof(BMHeader) + (size_t)(recorded % a.capacity) * (sizeof(BMRowHead) + cbytes + 24 * (size_t)B);
  BMRowHead* head = reinterpret_cast<BMRowHead*>(row);

  if (counted && (long long)blockIdx.x < B) {
    // ------------------------------------------------------------------------------------------- a sample's input part
    const long long b = blockIdx.x, P = (long long)a.H * a.W, n = P * a.C;
    const TX* __restrict__ x = static_cast<const TX*>(a.x);
    BMPair* pix = reinterpret_cast<BMPair*>(own);
    double sum = 0.0, sum_sq = 0.0;
    unsigned long long bad = 0ull;
    for (long long i = t; i < n; i += BM_THREADS) {
      const long long c = i / P, p = i - c * P;
      const TX* e = x + ((size_t)(c * B + b) * (size_t)P + (size_t)p) * (size_t)a.Q;
      double s = 0.0, u = 0.0;
      for (int q = 0; q < a.Q; ++q) {
        const double v = bm_widen(e[q]);
        s += v;
        u = fma(v, v, u);
        if (bm_finite(v)) {
          sum += v;
          sum_sq = fma(v, v, sum_sq);
        } else {
          bad += 1ull;
        }
      }
      if (a.K > 0) pix[i] = BMPair{s, u};
    }
    double win = 0.0, win_sq = 0.0;
    if (a.K > 0) {
      __syncthreads();
      const int Ho = a.H - a.K + 1, Wo = a.W - a.K + 1;
      for (int w = t; w < Ho * Wo; w += BM_THREADS) {
        const int ho = w / Wo, wo = w - ho * Wo;
        double ps = 1.0, pq = 1.0;
        for (int dh = 0; dh < a.K; ++dh)
          for (int dw = 0; dw < a.K; ++dw)
            for (int c = 0; c < a.C; ++c) {
              const BMPair e = pix[(long long)c * P + (ho + dh) * a.W + wo + dw];
              ps *= e.s;
              pq *= e.u;
            }
        win += ps;
        win_sq += pq;
      }
    }
    sum = bm_wave_sum(sum), sum_sq = bm_wave_sum(sum_sq), win = bm_wave_sum(win), win_sq = bm_wave_sum(win_sq);
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if (lane == 0) {
      red[0][wv] = sum, red[1][wv] = sum_sq, red[2][wv] = win, red[3][wv] = win_sq;
      reinterpret_cast<unsigned long long*>(red[4])[wv] = bad;
    }
  } else if (counted) {
    // ------------------------------------------------------------------------------------------- the logits part
    const TZ* __restrict__ logits = static_cast<const TZ*>(a.logits);
    const int L = a.L, n_edges = a.n_edges, n_bins = n_edges - 1;
    unsigned* cnt = reinterpret_cast<unsigned*>(own);   // the bins, then below, above, nan
    unsigned char* after = row + sizeof(BMRowHead) + cbytes;
    long long* out_label = reinterpret_cast<long long*>(after);
    long long* out_index = out_label + B;
    float* out_p = reinterpret_cast<float*>(out_index + B);
    int* out_pred = reinterpret_cast<int*>(out_p + B);
    for (int i = t; i < n_edges + 2; i += BM_THREADS) cnt[i] = 0u;
    __syncthreads();
    // threads 0, 64, 128, 192 each own one in-order total
    double total = 0.0, z_min = INFINITY, z_max = -INFINITY;
    unsigned n_rows = 0u, n_correct = 0u, n_bad = 0u, n_nonfinite = 0u;
    for (long long base = 0; base < B; base += BM_THREADS) {
      const long long r = base + t;
      if (r < B) {
        const TZ* z = logits + (size_t)r * (size_t)L;
        double s = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
        unsigned nf = 0u;
        int arg = 0;
        for (int j = 0; j < L; ++j) {
          const double v = bm_widen(z[j]);
          if (bm_finite(v)) {
            s += v;
            sq = fma(v, v, sq);
            mn = fmin(mn, v);
            if (v > mx) mx = v, arg = j;   // strictly: the lowest index among equal maxima
          } else {
            nf += 1u;
          }
        }
        const long long label = a.y[r];
        const bool valid = label >= 0 && label < L;
        float p_true = __uint_as_float(0x7fc00000u);
        int pred = -1;
        if (nf == 0u) {
          pred = arg;
          double S = 0.0;
          for (int j = 0; j < L; ++j) S += exp(bm_widen(z[j]) - mx);
          for (int j = 0; j < L; ++j) {
            const double p = exp(bm_widen(z[j]) - mx) / S;
            int lo = 0, hi = n_edges;   // the number of edges <= p
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (a.edges[mid] <= p) lo = mid + 1; else hi = mid;
            }
            int slot;
            if (lo == 0) slot = n_bins;                                           // below
            else if (lo == n_edges) slot = p == a.edges[n_bins] ? n_bins - 1 : n_bins + 1;   // the last bin is closed; above
            else slot = lo - 1;
            atomicAdd(&cnt[slot], 1u);
            if (valid && j == (int)label) p_true = (float)p;
          }
        } else {
          atomicAdd(&cnt[n_bins + 2], (unsigned)L);
        }
        out_label[r] = label;
        out_index[r] = a.indices ? a.indices[r] : -1ll;
        out_p[r] = p_true;
        out_pred[r] = pred;
        chunk[0][t] = s, chunk[1][t] = sq, chunk[2][t] = mn, chunk[3][t] = mx;
        chunk_bits[t] = (unsigned long long)nf | (valid ? 1ull << 32 : 0ull) | (valid && pred == (int)label ? 1ull << 33 : 0ull) |
                        (nf ? 1ull << 34 : 0ull);
      }
      __syncthreads();
      const int m = B - base < BM_THREADS ? (int)(B - base) : BM_THREADS;
      if (t == 0 || t == 64) {
        const double* v = chunk[t >> 6];
        for (int k = 0; k < m; ++k) total += v[k];
      } else if (t == 128) {
        for (int k = 0; k < m; ++k) z_min = fmin(z_min, chunk[2][k]), z_max = fmax(z_max, chunk[3][k]);
      } else if (t == 192) {
        for (int k = 0; k < m; ++k) {
          const unsigned long long bits = chunk_bits[k];
          n_nonfinite += (unsigned)bits;
          n_rows += (unsigned)(bits >> 32) & 1u, n_correct += (unsigned)(bits >> 33) & 1u, n_bad += (unsigned)(bits >> 34) & 1u;
        }
      }
      __syncthreads();
    }
    if (t == 0) head->z_sum = total;
    if (t == 64) head->z_sum_sq = total;
    if (t == 128) head->z_min = z_min, head->z_max = z_max;
    if (t == 192) head->rows = n_rows, head->correct = n_correct, head->bad_rows = n_bad, head->z_nonfinite = n_nonfinite;
    unsigned* out_counts = reinterpret_cast<unsigned*>(row + sizeof(BMRowHead));
    for (int i = t; i < n_bins; i += BM_THREADS) out_counts[i] = cnt[i];
    if (t == 0 && (n_bins & 1)) out_counts[n_bins] = 0u;   // the padding word: a row is written completely
    if (t == 1) head->below = cnt[n_bins], head->above = cnt[n_bins + 1], head->nan = cnt[n_bins + 2], head->reserved = 0u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave, in front of the barrier and thread 0's release
  }
  __syncthreads();

  if (t == 0) {
    if (counted) {
      if ((long long)blockIdx.x < B) {
        BMSlot* slot = a.slots + blockIdx.x;
        const unsigned long long* rb = reinterpret_cast<const unsigned long long*>(red[4]);
        __hip_atomic_store(&slot->x_sum, ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot->x_sum_sq, ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot->win_sum, ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot->win_sq, ((red[3][0] + red[3][1]) + red[3][2]) + red[3][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot->nonfinite, rb[0] + rb[1] + rb[2] + rb[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // param_stats_k's hand-over: agent-scope stores of the slot, an agent-scope release and an explicit wait BEFORE the
      // ticket is drawn; the workgroup that draws the last ticket makes an agent-scope acquire AFTER it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    const unsigned drawn = __hip_atomic_fetch_add(&hdr->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == gridDim.x - 1;
    if (last && counted) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    flags[2] = last ? 1u : 0u;
  }
  __syncthreads();
  if (flags[2] == 0u) return;   // every workgroup but the launch's last ends here; nobody waits

  if (counted) {
    // the B slots in sample order: chunks of 256 through LDS, then threads 0, 64, 128, 192 each add one quantity
    double total = 0.0;
    unsigned long long bad = 0ull;
    for (long long base = 0; base < B; base += BM_THREADS) {
      const long long b = base + t;
      if (b < B) {
        const BMSlot* slot = a.slots + b;
        chunk[0][t] = __hip_atomic_load(&slot->x_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        chunk[1][t] = __hip_atomic_load(&slot->x_sum_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        chunk[2][t] = __hip_atomic_load(&slot->win_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        chunk[3][t] = __hip_atomic_load(&slot->win_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        chunk_bits[t] = __hip_atomic_load(&slot->nonfinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      const int m = B - base < BM_THREADS ? (int)(B - base) : BM_THREADS;
      if (lane == 0) {
        const double* v = chunk[wv];
        for (int k = 0; k < m; ++k) total += v[k];
      } else if (t == 1) {
        for (int k = 0; k < m; ++k) bad += chunk_bits[k];
      }
      __syncthreads();
    }
    if (t == 0) head->x_sum = total, head->call = calls;
    if (t == 64) head->x_sum_sq = total;
    if (t == 128) head->win_sum = total;
    if (t == 192) head->win_sq = total;
    if (t == 1) head->x_nonfinite = bad;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the row's fields before `seq`
      head->seq = recorded;
      __hip_atomic_store(&hdr->recorded, recorded + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (t != 0) return;
  __hip_atomic_store(&hdr->calls, calls + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&hdr->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch draws from 0 again
}

template <typename TX, typename TZ>
int launch(const BMArgs& args, size_t lds, hipStream_t st) {
  if (!dctn_lds_optin((const void*)batch_monitor_k<TX, TZ>, lds)) return DCTN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((batch_monitor_k<TX, TZ>), dim3((unsigned)(args.B + 1)), dim3(BM_THREADS), lds, st, args);
  return DCTN_OK;
}

template <typename TX>
int launch_z(const BMArgs& args, int logits_dtype, size_t lds, hipStream_t st) {
  if (logits_dtype == DCTN_F32) return launch<TX, float>(args, lds, st);
  if (logits_dtype == DCTN_F64) return launch<TX, double>(args, lds, st);
  return launch<TX, bf16_bits>(args, lds, st);
}

bool is_dtype(int d) { return d == DCTN_F32 || d == DCTN_F64 || d == DCTN_BF16; }

}  // namespace

extern "C" {

size_t dctn_batch_monitor_block_bytes(int64_t B, int n_edges, int capacity) {
  if (B < 1 || B > BM_MAX_BATCH || n_edges < 2 || n_edges > BM_MAX_EDGES || capacity < 1) return 0;
  return sizeof(BMHeader) + (size_t)capacity * row_bytes(B, n_edges);
}

size_t dctn_batch_monitor_workspace_bytes(int64_t B) {
  if (B < 1 || B > BM_MAX_BATCH) return 0;
  return (size_t)B * sizeof(BMSlot);
}

int dctn_batch_monitor(const dctn_batch_monitor_t* m, void* stream) {
  if (!m || !m->x || !m->logits || !m->y || !m->edges || !m->block || !m->workspace) return DCTN_ERR_NULL;
  if (m->B < 1 || m->C < 1 || m->H < 1 || m->W < 1 || m->Q < 1) return DCTN_ERR_BAD_SHAPE;
  if (m->K < 0 || m->K > m->H || m->K > m->W) return DCTN_ERR_BAD_SHAPE;
  if (m->L < 1 || m->L > BM_MAX_LABELS || m->n_edges < 2 || m->n_edges > BM_MAX_EDGES) return DCTN_ERR_BAD_SHAPE;
  if (m->period < 1 || m->capacity < 1) return DCTN_ERR_BAD_SHAPE;
  if (!is_dtype(m->x_dtype) || !is_dtype(m->logits_dtype)) return DCTN_ERR_BAD_DTYPE;
  if (m->B > BM_MAX_BATCH || (unsigned long long)m->B * (unsigned long long)m->L >= (1ull << 32)) return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)m->x % dtype_size(m->x_dtype) != 0 || (uintptr_t)m->logits % dtype_size(m->logits_dtype) != 0)
    return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)m->y % 8 != 0 || (uintptr_t)m->indices % 8 != 0 || (uintptr_t)m->edges % 8 != 0) return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)m->block % 8 != 0 || (uintptr_t)m->workspace % 8 != 0) return DCTN_ERR_UNSUPPORTED;
  if (m->workspace_bytes != dctn_batch_monitor_workspace_bytes(m->B)) return DCTN_ERR_UNSUPPORTED;
  // with K > 0 a sample's pairs are staged in LDS: the device's limit (dctn_device_limits), never a constant
  if (m->K > 0 && (unsigned long long)m->C * (unsigned long long)m->H * (unsigned long long)m->W > 0x7ffffffull)
    return DCTN_ERR_UNSUPPORTED;
  const size_t lds = lds_bytes(m->C, m->H, m->W, m->K, m->n_edges);
  if (lds > (size_t)dctn_lds_wg_max()) return DCTN_ERR_UNSUPPORTED;

  BMArgs args = {};
  args.x = m->x, args.logits = m->logits;
  args.y = static_cast<const long long*>(m->y), args.indices = static_cast<const long long*>(m->indices);
  args.edges = static_cast<const double*>(m->edges);
  args.block = static_cast<unsigned char*>(m->block), args.slots = static_cast<BMSlot*>(m->workspace);
  args.B = m->B, args.C = m->C, args.H = m->H, args.W = m->W, args.Q = m->Q, args.K = m->K, args.L = m->L;
  args.n_edges = m->n_edges, args.period = (unsigned)m->period, args.capacity = (unsigned)m->capacity;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (m->x_dtype == DCTN_F32)
    rc = launch_z<float>(args, m->logits_dtype, lds, st);
  else if (m->x_dtype == DCTN_F64)
    rc = launch_z<double>(args, m->logits_dtype, lds, st);
  else
    rc = launch_z<bf16_bits>(args, m->logits_dtype, lds, st);
  if (rc != DCTN_OK) return rc;
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
