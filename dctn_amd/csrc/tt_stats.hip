// Sum and squared Frobenius norm of the tensor every ConvSBS string REPRESENTS, for up to 16 strings in ONE launch
// (dctn_tt_stats) - what the reference's runner logs per string every 20 iterations as mean_of_tt_tensor/<name> and
// std_of_tt_tensor/<name> (dctn/conv_sbs_statistics_logging.py: ConvSBS.mean(), ConvSBS.var() ** 0.5), from the cores
// alone, in float64, with a period counted on the device and a ring of records in a caller-owned block.
//
// Core c of a string is (o_c, l_c, r_c, q, ..., q) contiguous, P = q^C, its slices A_c[o, p] are l_c x r_c with
// A_c[o, p][k, b] = core[((o l_c + k) r_c + b) P + p].  With l_0 = bond_sizes[0] (1: an open chain; more: a ring)
//   sum     = sum_i  (e_i^T S_0 S_1 ... S_{N-1})[i],                    S_c    = sum_{o,p} A_c[o, p]
//   sq_norm = sum_i sum_j (F_{N-1} o ... o F_0)(e_i e_j^T)[i, j],         F_c(V) = sum_{o,p} A_c[o, p]^T V A_c[o, p]
// A string owns l_0 workgroups of 256 threads: workgroup i forms the i-th term of `sum` (a row vector through the
// chain) and, for j = 0 .. l_0 - 1 in that order, the (i, j) terms of `sq_norm` (one propagation of an l_0 x l_0 V each);
// an open chain is one workgroup and one propagation of a 1 x 1 V.
//
// One step of a propagation (tt_step): V (l x l) and a round of slices live in LDS as float64 (a float32 element is
// widened exactly).  A round holds G = TT_ROUND / (l r) slices - every slice of a core up to bond 8 at the shapes the
// classifier has, 8 at bond 16, 2 at bond 32:
//   stage   A_s[g][k][b]                                      from global memory, one element per thread and turn
//   phase 1 T_s[g][a][b]  = sum_k V[a][k] A_s[g][k][b]        one entry per thread and turn, k ascending
//   phase 2 V'[a'][b]    += sum_(g,k) A_s[g][k][a'] T_s[g][k][b]   thread t owns the entries t, t + 256, ..., in registers
// In phase 1 the lanes of a wave read consecutive b (V[a][k] is a broadcast), in phase 2 likewise (A_s[g][k][a'] is the
// broadcast): no access has a bank conflict beyond what r < 32 leaves idle.
//
// Reproducible bits.  Grid, round size and every summation order are functions of the string's own shape: the two values
// of a string do not depend on how many strings the launch holds, on the string's place among them, on the device or on
// what the workspace held.  Workgroup i STORES its two partial values into its own slot of the workspace and draws the
// block's ticket; the workgroup that draws the launch's last ticket adds every string's slots in index order, writes the
// row and advances the header.  This is tensor_stats_k's hand-over (sbs_tail.hip): slots, ticket, no workgroup waits for
// another, the release and acquire fences in the same places.  A launch that is not recorded (calls % period != 0)
// reads no core: its workgroups draw the ticket and end, and the last one advances `calls`.
#include "common.h"

namespace {

constexpr int TT_MAX_STRINGS = 16;
constexpr int TT_MAX_CORES = 16;
constexpr int TT_MAX_BOND = 32;
constexpr int TT_MAX_P = 256;
constexpr int TT_THREADS = 256;
constexpr int TT_ROUND = 2048;       // doubles of staged slices per round: at least two slices at bond 32
constexpr int TT_V = TT_MAX_BOND * TT_MAX_BOND;
constexpr int TT_OWN = TT_V / TT_THREADS;   // entries of V' a thread owns at most
constexpr long long TT_MAX_CORE_ELEMS = 0x7fffffffLL;

// The block (include/dctn_amd.h): the header, then `capacity` rows of one TTRowHead and n_strings {sum, sq_norm} pairs
struct TTHeader {
  unsigned calls, recorded, ticket, reserved[5];
};
static_assert(sizeof(TTHeader) == 32, "the header is 32 bytes");
struct TTRowHead {
  unsigned call, seq;
  unsigned long long reserved;
};
static_assert(sizeof(TTRowHead) == 16, "a row starts with 16 bytes");

// Everything the kernel knows, in its argument: string s owns the cores core_first[s] .. core_first[s + 1] - 1 of the
// three compact tables and the workgroups wg_first[s] .. wg_first[s + 1] - 1
struct TTArgs {
  const void* core[TT_MAX_STRINGS * TT_MAX_CORES];
  int out[TT_MAX_STRINGS * TT_MAX_CORES];
  unsigned char bond[TT_MAX_STRINGS * TT_MAX_CORES];   // the LEFT bond of the core
  unsigned short core_first[TT_MAX_STRINGS + 1];
  unsigned short wg_first[TT_MAX_STRINGS + 1];
  unsigned short P[TT_MAX_STRINGS];
  int n_strings;
};
static_assert(sizeof(TTArgs) <= 3584, "the argument stays well inside the 4 KiB a kernel may take");

// V (l x l, in LDS) -> F_c(V) (r x r, in the same place).  Every thread of the workgroup calls it; it ends behind a barrier.
template <typename T>
__device__ __forceinline__ void tt_step(const T* core, int l, int r, int n_slices, int P, double* V, double* A_s, double* T_s) {
  const int t = threadIdx.x, lr = l * r, rr = r * r;
  const int G = TT_ROUND / lr;
  double acc[TT_OWN];
#pragma unroll
  for (int x = 0; x < TT_OWN; ++x) acc[x] = 0.0;
  for (int g0 = 0; g0 < n_slices; g0 += G) {
    const int gb = n_slices - g0 < G ? n_slices - g0 : G;
    for (int e = t; e < gb * lr; e += TT_THREADS) {
      const int g = e / lr, rem = e - g * lr;
      const int o = (g0 + g) / P, p = (g0 + g) - o * P;
      A_s[e] = (double)core[((size_t)o * lr + rem) * P + p];
    }
    __syncthreads();
    for (int e = t; e < gb * lr; e += TT_THREADS) {
      const int g = e / lr, rem = e - g * lr, a = rem / r, b = rem - a * r;
      const double* Ag = A_s + g * lr;
      double x = 0.0;
      for (int k = 0; k < l; ++k) x = fma(V[a * l + k], Ag[k * r + b], x);
      T_s[e] = x;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < TT_OWN; ++x) {
      const int e = t + x * TT_THREADS;
      if (e < rr) {
        const int a = e / r, b = e - a * r;
        double v = acc[x];
        for (int gk = 0; gk < gb * l; ++gk) v = fma(A_s[gk * r + a], T_s[gk * r + b], v);   // (g, k): g lr + k r = (g l + k) r
        acc[x] = v;
      }
    }
    __syncthreads();   // the next round stages over A_s
  }
#pragma unroll
  for (int x = 0; x < TT_OWN; ++x) {
    const int e = t + x * TT_THREADS;
    if (e < rr) V[e] = acc[x];
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(TT_THREADS) void tt_stats_k(const TTArgs args, unsigned char* __restrict__ block, unsigned capacity,
                                                        unsigned period, double* __restrict__ workspace) {
  __shared__ double V[TT_V];
  __shared__ double A_s[TT_ROUND];
  __shared__ double T_s[TT_ROUND];
  __shared__ double w[2][TT_MAX_BOND];
  __shared__ unsigned wg_calls;
  __shared__ int is_last;
  const int t = threadIdx.x;
  TTHeader* hdr = reinterpret_cast<TTHeader*>(block);

  if (t == 0) wg_calls = __hip_atomic_load(&hdr->calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const unsigned calls = wg_calls;
  const bool counted = calls % period == 0;   // the same answer in every workgroup: `calls` moves after the last ticket

  double part_sum = 0.0, part_sq = 0.0;   // thread 0's
  if (counted) {
    int s = 0;
    while (s + 1 < args.n_strings && blockIdx.x >= args.wg_first[s + 1]) ++s;
    const int i = (int)blockIdx.x - args.wg_first[s];
    const int c0 = args.core_first[s], N = args.core_first[s + 1] - c0, P = args.P[s];
    const int l0 = args.bond[c0];

    // the i-th term of `sum`: the row vector e_i^T through S_0 ... S_{N-1}
    if (t < l0) w[0][t] = t == i ? 1.0 : 0.0;
    __syncthreads();
    int cur = 0;
    for (int c = 0; c < N; ++c) {
      const int l = args.bond[c0 + c], r = args.bond[c0 + (c + 1 == N ? 0 : c + 1)], n_out = args.out[c0 + c];
      const T* core = (const T*)args.core[c0 + c];
      for (int e = t; e < l * r; e += TT_THREADS) {   // S_c[k][b], e = k r + b: o ascending, then p
        double x = 0.0;
        for (int o = 0; o < n_out; ++o) {
          const T* a = core + ((size_t)o * (l * r) + e) * P;
          for (int p = 0; p < P; ++p) x += (double)a[p];
        }
        A_s[e] = x;
      }
      __syncthreads();
      if (t < r) {
        double x = 0.0;
        for (int k = 0; k < l; ++k) x = fma(w[cur][k], A_s[k * r + t], x);
        w[cur ^ 1][t] = x;
      }
      __syncthreads();
      cur ^= 1;
    }
    if (t == 0) part_sum = w[cur][i];

    // the (i, j) terms of `sq_norm`, j ascending
    for (int j = 0; j < l0; ++j) {
      for (int e = t; e < l0 * l0; e += TT_THREADS) V[e] = e == i * l0 + j ? 1.0 : 0.0;
      __syncthreads();
      for (int c = 0; c < N; ++c) {
        const int l = args.bond[c0 + c], r = args.bond[c0 + (c + 1 == N ? 0 : c + 1)];
        tt_step<T>((const T*)args.core[c0 + c], l, r, args.out[c0 + c] * P, P, V, A_s, T_s);
      }
      if (t == 0) part_sq += V[i * l0 + j];
      __syncthreads();   // the next j writes V
    }
  }

  if (t == 0) {
    if (counted) {
      // tensor_stats_k's hand-over of the slot to whichever workgroup turns out to be last: agent-scope stores of the
      // slot, an agent-scope release and an explicit wait BEFORE the ticket is drawn; the workgroup that draws the last
      // ticket makes an agent-scope acquire AFTER it and reads the slots with agent-scope loads.
      double* slot = workspace + (size_t)blockIdx.x * 2;
      __hip_atomic_store(&slot[0], part_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&slot[1], part_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

  // the last workgroup's first wave: lane s adds the slots of string s in index order and writes its pair; then lane 0
  // writes the row's head and the header, `seq` after the pairs
  const unsigned recorded = __hip_atomic_load(&hdr->recorded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (counted) {
    unsigned char* row = block + sizeof(TTHeader) + (size_t)(recorded % capacity) * (sizeof(TTRowHead) + 16 * (size_t)args.n_strings);
    if (t < args.n_strings) {
      const unsigned first = args.wg_first[t], end = args.wg_first[t + 1];
      double sum = __hip_atomic_load(&workspace[(size_t)first * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      double sq = __hip_atomic_load(&workspace[(size_t)first * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (unsigned k = first + 1; k < end; ++k) {
        sum += __hip_atomic_load(&workspace[(size_t)k * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sq += __hip_atomic_load(&workspace[(size_t)k * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      double* pair = reinterpret_cast<double*>(row + sizeof(TTRowHead)) + 2 * t;
      pair[0] = sum, pair[1] = sq;
    }
    if (t == 0) {
      TTRowHead* head = reinterpret_cast<TTRowHead*>(row);
      head->call = calls;
      head->reserved = 0ull;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the pairs of this wave's lanes before `seq`
      head->seq = recorded;
      __hip_atomic_store(&hdr->recorded, recorded + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (t != 0) return;
  __hip_atomic_store(&hdr->calls, calls + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&hdr->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch draws from 0 again
}

// q^C, or TT_MAX_P + 1 if it is larger than TT_MAX_P (q, C >= 1)
int slice_count(int q, int C) {
  long long p = 1;
  for (int c = 0; c < C && p <= TT_MAX_P; ++c) p *= q;
  return p > TT_MAX_P ? TT_MAX_P + 1 : (int)p;
}

bool string_is_valid(const dctn_tt_string_t& s) {
  if (s.n_cores < 1 || s.n_cores > TT_MAX_CORES || s.C < 1 || s.q < 1) return false;
  for (int c = 0; c < s.n_cores; ++c)
    if (s.out_sizes[c] < 1 || s.bond_sizes[c] < 1) return false;
  return true;
}

bool string_is_supported(const dctn_tt_string_t& s) {
  const int P = slice_count(s.q, s.C);
  if (P > TT_MAX_P) return false;
  for (int c = 0; c < s.n_cores; ++c)
    if (s.bond_sizes[c] > TT_MAX_BOND) return false;
  for (int c = 0; c < s.n_cores; ++c) {   // a core's element count fits the kernel's 32-bit slice arithmetic
    const long long lr = (long long)s.bond_sizes[c] * s.bond_sizes[(c + 1) % s.n_cores];
    if ((long long)s.out_sizes[c] * P > TT_MAX_CORE_ELEMS / lr) return false;
  }
  return true;
}

}  // namespace

extern "C" {

size_t dctn_tt_stats_block_bytes(int n_strings, int capacity) {
  if (n_strings < 1 || n_strings > TT_MAX_STRINGS || capacity < 1) return 0;
  return sizeof(TTHeader) + (size_t)capacity * (sizeof(TTRowHead) + 16 * (size_t)n_strings);
}

size_t dctn_tt_stats_workspace_bytes(const dctn_tt_string_t* strings, int n_strings) {
  if (!strings || n_strings < 1 || n_strings > TT_MAX_STRINGS) return 0;
  size_t workgroups = 0;
  for (int s = 0; s < n_strings; ++s) {
    if (!string_is_valid(strings[s]) || !string_is_supported(strings[s])) return 0;
    workgroups += (size_t)strings[s].bond_sizes[0];
  }
  return workgroups * 2 * sizeof(double);
}

int dctn_tt_stats(const void* const* cores, const dctn_tt_string_t* strings, int n_strings, void* block, int capacity, int period,
                  void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  if (!cores || !strings || !block) return DCTN_ERR_NULL;
  if (n_strings < 1 || n_strings > TT_MAX_STRINGS) return DCTN_ERR_BAD_SHAPE;
  int total_cores = 0;
  for (int s = 0; s < n_strings; ++s) {   // the walk over `cores` needs every n_cores in range first
    if (strings[s].n_cores < 1 || strings[s].n_cores > TT_MAX_CORES) return DCTN_ERR_BAD_SHAPE;
    total_cores += strings[s].n_cores;
  }
  for (int k = 0; k < total_cores; ++k)
    if (!cores[k]) return DCTN_ERR_NULL;
  for (int s = 0; s < n_strings; ++s)
    if (!string_is_valid(strings[s])) return DCTN_ERR_BAD_SHAPE;
  if (capacity < 1 || period < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64) return DCTN_ERR_BAD_DTYPE;
  for (int s = 0; s < n_strings; ++s)
    if (!string_is_supported(strings[s])) return DCTN_ERR_UNSUPPORTED;
  const uintptr_t elem = dtype == DCTN_F32 ? 4 : 8;
  for (int k = 0; k < total_cores; ++k)
    if ((uintptr_t)cores[k] % elem != 0) return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)block % 8 != 0 || (uintptr_t)workspace % 8 != 0) return DCTN_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < dctn_tt_stats_workspace_bytes(strings, n_strings)) return DCTN_ERR_WORKSPACE;

  TTArgs args = {};
  args.n_strings = n_strings;
  unsigned n_core = 0, n_wg = 0;
  for (int s = 0; s < n_strings; ++s) {
    const dctn_tt_string_t& st = strings[s];
    args.core_first[s] = (unsigned short)n_core;
    args.wg_first[s] = (unsigned short)n_wg;
    args.P[s] = (unsigned short)slice_count(st.q, st.C);
    for (int c = 0; c < st.n_cores; ++c, ++n_core) {
      args.core[n_core] = cores[n_core];
      args.out[n_core] = st.out_sizes[c];
      args.bond[n_core] = (unsigned char)st.bond_sizes[c];
    }
    n_wg += (unsigned)st.bond_sizes[0];
  }
  for (int s = n_strings; s <= TT_MAX_STRINGS; ++s) args.core_first[s] = (unsigned short)n_core, args.wg_first[s] = (unsigned short)n_wg;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(n_wg), b(TT_THREADS);
  if (dtype == DCTN_F32)
    hipLaunchKernelGGL((tt_stats_k<float>), g, b, 0, st, args, (unsigned char*)block, (unsigned)capacity, (unsigned)period,
                       (double*)workspace);
  else
    hipLaunchKernelGGL((tt_stats_k<double>), g, b, 0, st, args, (unsigned char*)block, (unsigned)capacity, (unsigned)period,
                       (double*)workspace);
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
