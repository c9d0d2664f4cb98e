// Device-resident batch source (reference: the train DataLoader of dctn/dataset_loading.py:69-70, 282-286, 319-325 -
// __getitem__ per sample, collate_quantum, pinning, a copy): ONE launch that picks the samples of a batch, moves them into
// the model's input layout and dtype, and advances a device counter, so that a captured graph draws batch k, k + 1, ... on
// its replays.  The epoch order is a pure function of (seed, epoch, position): a 6-round Feistel network with cycle
// walking, keyed by Philox4x32-10.  include/dctn_amd.h holds the normative definition; dctn_amd/batches.py restates it.
//   draw   : sample numbers from the 16-byte device block {seed, batches_done}; the launch itself advances the block
//            (core_dropout_k's ticket)
//   gather : the same data movement, sample numbers from a device int64 array; no state
// Two source kinds: raw uint8 intensities through a (256, Q) table staged in LDS (phi, the scale and the cast folded into
// the table), and rows of an already-expanded feature tensor copied as they are.
//
// One WAVE moves one sample at a time: its sample number is wave-uniform (scalar arithmetic, once per sample), its lanes
// share the row.  The launch is latency-bound, not bandwidth-bound: at cfg2's batch (1024 x 784 pixels, bf16, Q = 2) it
// reads 0.8 MB and writes 3.2 MB, a few microseconds of dependent round trips (block -> order -> row -> table -> store).
#include "common.h"

namespace {

constexpr int BATCH_THREADS = 256;                       // 4 waves: one per SIMD
constexpr int BATCH_WAVES = BATCH_THREADS / DCTN_WAVE;
constexpr int BATCH_UNROLL = 4;                          // a lane's loads in flight: a wave reads a 28 x 28 uint8 row in one pass, not in four dependent ones
constexpr int BATCH_MAX_WGS = 256;                       // the ticket is one atomic per workgroup on one address (adam_score.hip)
constexpr unsigned BATCH_TAG = 0x53485546u;              // counter word c3 of the round keys; dropout's c3 stays below 8

struct BatchState {   // include/dctn_amd.h documents this layout: it is part of the ABI
  unsigned seed_lo, seed_hi, batches_done, ticket;
};

struct BatchArgs {   // passed by value in the kernel argument
  const void* src;
  const void* table;
  const long long* labels;
  const long long* sample_idx;   // gather only
  void* x;
  long long* y;
  long long* indices;
  BatchState* state;             // draw only
  unsigned n, G, S, Bl, offset;  // samples, global batch, batches per epoch, this launch's samples, first position of the shard
  unsigned bits;                 // max(2, bit length of n - 1): the Feistel network permutes [0, 2^bits)
  unsigned identity;             // DCTN_BATCH_IDENTITY_ORDER
  unsigned row_len, width;       // U8_TABLE: pixels P, table columns Q;  ROWS: elements R, channels C
};

template <typename S> struct BatchBits {};   // the values only move: an unsigned integer of the element's size
template <> struct BatchBits<float> { typedef unsigned type; };
template <> struct BatchBits<double> { typedef unsigned long long type; };
template <> struct BatchBits<bf16_t> { typedef unsigned short type; };

__device__ __forceinline__ unsigned mix32(unsigned h) {   // murmur3's finaliser
  h ^= h >> 16, h *= 0x85EBCA6Bu, h ^= h >> 13, h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// one pass of the network: a bijection on [0, 2^b), 2 <= b <= 31; the halves swap widths every round
__device__ __forceinline__ unsigned perm_once(unsigned v, unsigned b, const unsigned (&K)[6]) {
  unsigned wl = b >> 1, wr = b - wl;
  unsigned L = v >> wr, R = v & ((1u << wr) - 1u);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const unsigned t = L ^ (mix32(R ^ K[j]) & ((1u << wl) - 1u));
    L = R, R = t;
    const unsigned w = wl;
    wl = wr, wr = w;
  }
  return (L << wr) | R;
}

// What the launch draws with, left in LDS by lane 0: the six round keys, the first position of the shard, the batch number
struct BatchHead {
  unsigned K[6], pos0, k;
};

// lane 0 reads the block BEFORE it takes the workgroup's ticket at the end; the launch's one write of batches_done happens
// after the last ticket is drawn, so no workgroup can see the new value (core_dropout_k)
__device__ __forceinline__ void batch_read_head(const BatchArgs& a, BatchHead& head) {
  const unsigned k0 = __hip_atomic_load(&a.state->seed_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned k1 = __hip_atomic_load(&a.state->seed_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned k = __hip_atomic_load(&a.state->batches_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned epoch = k / a.S;   // (the identity order, padded or not, uses neither the epoch nor the keys)
  unsigned w0[4], w1[4];
  philox4x32_10(0u, 0u, epoch, BATCH_TAG, k0, k1, w0);
  philox4x32_10(1u, 0u, epoch, BATCH_TAG, k0, k1, w1);
  head.K[0] = w0[0], head.K[1] = w0[1], head.K[2] = w0[2], head.K[3] = w0[3], head.K[4] = w1[0], head.K[5] = w1[1];
  // < S * G: at most n < 2^31, and with DCTN_BATCH_PAD_TAIL below n + G <= 2 n < 2^32, so neither this nor pos0 + j wraps
  head.pos0 = (k % a.S) * a.G + a.offset;
  head.k = k;
}

__device__ __forceinline__ void batch_take_ticket(const BatchArgs& a, unsigned k) {
  // The ticket, as core_dropout_k's.  It orders one thing only: every workgroup's read of the block before the last
  // workgroup's write of it.  The wait makes sure this lane's state loads have returned before the ticket is drawn.
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  const unsigned drawn = __hip_atomic_fetch_add(&a.state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (drawn == gridDim.x - 1) {   // plain vector stores; the next launch starts from ticket 0 again
    a.state->batches_done = k + 1u;
    a.state->ticket = 0u;
  }
}

// the sample of slot j of this launch, wave-uniform; under DCTN_BATCH_PAD_TAIL (identity order only) it may be >= n
template <bool DRAW>
__device__ __forceinline__ unsigned batch_sample(const BatchArgs& a, const unsigned (&K)[6], unsigned pos0, unsigned j) {
  if (!DRAW) return (unsigned)a.sample_idx[j];
  unsigned v = pos0 + j;
  if (!a.identity) {
    do v = perm_once(v, a.bits, K);   // cycle walking: position < n lies on a cycle of the bijection, so the walk returns below n
    while (v >= a.n);
  }
  return v;
}

// DCTN_BATCH_PAD_TAIL (PAD, identity order only): a slot whose position s is >= n is padding.  It reads the row of sample
// n - 1, so that x is fully written with finite values, and reports the label -100 (the score kernel's "skip this row")
// and the index -1.  PAD is a template parameter and the unpadded statements are the ones the kernels had before it: the
// instantiations without it - every training draw, every gather - compile to the instructions they compiled to then.
template <bool PAD>
__device__ __forceinline__ void batch_report(const BatchArgs& a, unsigned j, unsigned s, bool padding) {
  if constexpr (PAD) a.y[j] = padding ? -100ll : a.labels[s], a.indices[j] = padding ? -1ll : (long long)s;
  else a.y[j] = a.labels[s], a.indices[j] = (long long)s;
}

template <typename Tb, int Q> struct alignas((Q & (Q - 1)) == 0 ? (Q * sizeof(Tb) > 16 ? 16 : Q * sizeof(Tb)) : sizeof(Tb)) BatchEntry {
  Tb e[Q];
};

// 4 pixels' worth of table entries, N = 4 Q elements, as 16-byte stores (8-byte ones for bf16 with odd Q)
template <typename Tb, int N> struct BatchGroup {
  static constexpr int WORDS = N * (int)sizeof(Tb) / 4;
  static constexpr unsigned ALIGN = WORDS % 4 == 0 ? 16 : 8;
  static __device__ __forceinline__ void store(Tb* dst, const Tb (&v)[N]) {
    unsigned w[WORDS];
    if constexpr (sizeof(Tb) == 2) {
#pragma unroll
      for (int i = 0; i < WORDS; ++i) w[i] = (unsigned)v[2 * i] | ((unsigned)v[2 * i + 1] << 16);
    } else if constexpr (sizeof(Tb) == 4) {
#pragma unroll
      for (int i = 0; i < WORDS; ++i) w[i] = (unsigned)v[i];
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) w[2 * i] = (unsigned)v[i], w[2 * i + 1] = (unsigned)(v[i] >> 32);
    }
    if constexpr (WORDS % 4 == 0) {
#pragma unroll
      for (int c = 0; c < WORDS / 4; ++c)
        reinterpret_cast<uint4*>(dst)[c] = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
    } else {
#pragma unroll
      for (int c = 0; c < WORDS / 2; ++c) reinterpret_cast<uint2*>(dst)[c] = make_uint2(w[2 * c], w[2 * c + 1]);
    }
  }
};

// DCTN_BATCH_SRC_U8_TABLE: x[0, j, p, :] = table[src[s_j, p], :]
template <typename S, int Q, bool DRAW, bool PAD>
__global__ __launch_bounds__(BATCH_THREADS) void batch_u8_k(BatchArgs a) {
  typedef typename BatchBits<S>::type Tb;
  __shared__ BatchEntry<Tb, Q> tab[256];
  __shared__ BatchHead head;
  {
    const Tb* g = static_cast<const Tb*>(a.table);   // aligned to its element size only: element by element
    Tb* t = &tab[0].e[0];
    for (int i = threadIdx.x; i < 256 * Q; i += BATCH_THREADS) t[i] = g[i];
  }
  if (DRAW && threadIdx.x == 0) batch_read_head(a, head);
  __syncthreads();
  unsigned K[6] = {0u, 0u, 0u, 0u, 0u, 0u}, pos0 = 0u;
  if (DRAW) {
#pragma unroll
    for (int i = 0; i < 6; ++i) K[i] = __builtin_amdgcn_readfirstlane(head.K[i]);
    pos0 = __builtin_amdgcn_readfirstlane(head.pos0);
  }
  const unsigned lane = threadIdx.x % DCTN_WAVE;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * BATCH_WAVES + threadIdx.x / DCTN_WAVE);
  const unsigned P = a.row_len;
  const unsigned char* src = static_cast<const unsigned char*>(a.src);
  Tb* x = static_cast<Tb*>(a.x);
  // four pixels per 32-bit load: every row starts on a 4-byte boundary, and 4 Q elements of x on a store boundary
  const bool vec = P % 4u == 0u && (uintptr_t)src % 4u == 0u && (uintptr_t)x % BatchGroup<Tb, 4 * Q>::ALIGN == 0u;
  for (unsigned j = wave; j < a.Bl; j += gridDim.x * BATCH_WAVES) {
    const unsigned drawn = batch_sample<DRAW>(a, K, pos0, j);
    const bool padding = PAD && drawn >= a.n;   // wave-uniform
    const unsigned s = padding ? a.n - 1u : drawn;
    if (lane == 0) batch_report<PAD>(a, j, s, padding);
    const unsigned char* row = src + (size_t)s * P;
    Tb* out = x + (size_t)j * P * Q;
    if (vec) {
      const unsigned* row4 = reinterpret_cast<const unsigned*>(row);
      for (unsigned g0 = lane; g0 < P / 4u; g0 += DCTN_WAVE * BATCH_UNROLL) {
        unsigned four[BATCH_UNROLL];
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
          four[u] = g < P / 4u ? row4[g] : 0u;
        }
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
          if (g >= P / 4u) break;
          Tb v[4 * Q];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const BatchEntry<Tb, Q> e = tab[(four[u] >> (8 * p)) & 255u];
#pragma unroll
            for (int q = 0; q < Q; ++q) v[p * Q + q] = e.e[q];
          }
          BatchGroup<Tb, 4 * Q>::store(out + (size_t)g * 4 * Q, v);
        }
      }
    } else {
      for (unsigned p = lane; p < P; p += DCTN_WAVE) {
        const BatchEntry<Tb, Q> e = tab[row[p]];
#pragma unroll
        for (int q = 0; q < Q; ++q) out[(size_t)p * Q + q] = e.e[q];
      }
    }
  }
  if (DRAW && threadIdx.x == 0) batch_take_ticket(a, head.k);
}

// DCTN_BATCH_SRC_ROWS: x[c, j, :] = src[c, s_j, :]
template <typename S, bool DRAW, bool PAD>
__global__ __launch_bounds__(BATCH_THREADS) void batch_rows_k(BatchArgs a) {
  typedef typename BatchBits<S>::type Tb;
  __shared__ BatchHead head;
  unsigned K[6] = {0u, 0u, 0u, 0u, 0u, 0u}, pos0 = 0u;
  if (DRAW) {
    if (threadIdx.x == 0) batch_read_head(a, head);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 6; ++i) K[i] = __builtin_amdgcn_readfirstlane(head.K[i]);
    pos0 = __builtin_amdgcn_readfirstlane(head.pos0);
  }
  const unsigned lane = threadIdx.x % DCTN_WAVE;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * BATCH_WAVES + threadIdx.x / DCTN_WAVE);
  const unsigned R = a.row_len, C = a.width;
  const Tb* src = static_cast<const Tb*>(a.src);
  Tb* x = static_cast<Tb*>(a.x);
  const size_t row_bytes = (size_t)R * sizeof(Tb);
  const bool vec = row_bytes % 16u == 0u && ((uintptr_t)src | (uintptr_t)x) % 16u == 0u;
  for (unsigned j = wave; j < a.Bl; j += gridDim.x * BATCH_WAVES) {
    const unsigned drawn = batch_sample<DRAW>(a, K, pos0, j);
    const bool padding = PAD && drawn >= a.n;   // wave-uniform
    const unsigned s = padding ? a.n - 1u : drawn;
    if (lane == 0) batch_report<PAD>(a, j, s, padding);
    for (unsigned c = 0; c < C; ++c) {
      const Tb* in = src + ((size_t)c * a.n + s) * R;
      Tb* out = x + ((size_t)c * a.Bl + j) * R;
      if (vec) {
        const uint4* in16 = reinterpret_cast<const uint4*>(in);
        uint4* out16 = reinterpret_cast<uint4*>(out);
        const unsigned pieces = (unsigned)(row_bytes / 16u);
        for (unsigned i0 = lane; i0 < pieces; i0 += DCTN_WAVE * BATCH_UNROLL) {
          // four named values, not an array (hipcc moved the array into LDS); every load is issued - past the row's end its
          // last piece again - so none waits behind a branch
          static_assert(BATCH_UNROLL == 4, "the row copy is written out for four loads in flight");
          const unsigned i1 = i0 + DCTN_WAVE, i2 = i0 + 2 * DCTN_WAVE, i3 = i0 + 3 * DCTN_WAVE, last = pieces - 1u;
          const uint4 t0 = in16[i0], t1 = in16[min(i1, last)], t2 = in16[min(i2, last)], t3 = in16[min(i3, last)];
          out16[i0] = t0;
          if (i1 < pieces) out16[i1] = t1;
          if (i2 < pieces) out16[i2] = t2;
          if (i3 < pieces) out16[i3] = t3;
        }
      } else {
        for (unsigned i = lane; i < R; i += DCTN_WAVE) out[i] = in[i];
      }
    }
  }
  if (DRAW && threadIdx.x == 0) batch_take_ticket(a, head.k);
}

// [draw / gather][source kind][dtype code]
const char* const BATCH_NAMES[2][2][3] = {
    {{"batch_draw_u8_f32", "batch_draw_u8_f64", "batch_draw_u8_bf16"},
     {"batch_draw_rows_f32", "batch_draw_rows_f64", "batch_draw_rows_bf16"}},
    {{"batch_gather_u8_f32", "batch_gather_u8_f64", "batch_gather_u8_bf16"},
     {"batch_gather_rows_f32", "batch_gather_rows_f64", "batch_gather_rows_bf16"}},
};

template <typename S, bool DRAW, bool PAD>
void batch_launch_padded(const BatchArgs& a, int kind, dim3 g, hipStream_t st) {
  const dim3 b(BATCH_THREADS);
  if (kind == DCTN_BATCH_SRC_ROWS) {
    hipLaunchKernelGGL((batch_rows_k<S, DRAW, PAD>), g, b, 0, st, a);
    return;
  }
  switch (a.width) {
    case 1: hipLaunchKernelGGL((batch_u8_k<S, 1, DRAW, PAD>), g, b, 0, st, a); break;
    case 2: hipLaunchKernelGGL((batch_u8_k<S, 2, DRAW, PAD>), g, b, 0, st, a); break;
    case 3: hipLaunchKernelGGL((batch_u8_k<S, 3, DRAW, PAD>), g, b, 0, st, a); break;
    default: hipLaunchKernelGGL((batch_u8_k<S, 4, DRAW, PAD>), g, b, 0, st, a); break;
  }
}

template <typename S, bool DRAW>
void batch_launch_typed(const BatchArgs& a, int kind, bool pad, dim3 g, hipStream_t st) {
  if constexpr (DRAW) {   // a gather has no positions to pad
    if (pad) return batch_launch_padded<S, true, true>(a, kind, g, st);
  }
  batch_launch_padded<S, DRAW, false>(a, kind, g, st);
}

// everything is decided here, on the host, before any launch
template <bool DRAW>
int batch_launch(BatchArgs a, int64_t n, int64_t G, int64_t count, int64_t offset, int64_t row_len, int width, int kind,
                 int flags, int dtype, void* stream) {
  if (!a.src || !a.labels || !a.x || !a.y || !a.indices || (DRAW ? !a.state : !a.sample_idx)) return DCTN_ERR_NULL;
  if (kind != DCTN_BATCH_SRC_U8_TABLE && kind != DCTN_BATCH_SRC_ROWS) return DCTN_ERR_BAD_SHAPE;
  if (kind == DCTN_BATCH_SRC_U8_TABLE && !a.table) return DCTN_ERR_NULL;
  if (n < 1 || n >= (int64_t)1 << 31 || count < 1 || count >= (int64_t)1 << 31) return DCTN_ERR_BAD_SHAPE;
  if (row_len < 1 || row_len >= (int64_t)1 << 31 || width < 1) return DCTN_ERR_BAD_SHAPE;
  if (DRAW && (G < 1 || G > n || offset < 0 || offset + count > G)) return DCTN_ERR_BAD_SHAPE;
  if (DRAW && (flags & ~(DCTN_BATCH_IDENTITY_ORDER | DCTN_BATCH_PAD_TAIL))) return DCTN_ERR_BAD_SHAPE;
  if (DRAW && (flags & DCTN_BATCH_PAD_TAIL) && !(flags & DCTN_BATCH_IDENTITY_ORDER)) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_F64 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  if (width > 4) return DCTN_ERR_UNSUPPORTED;
  const bool pad = DRAW && (flags & DCTN_BATCH_PAD_TAIL);
  a.n = (unsigned)n, a.Bl = (unsigned)count, a.row_len = (unsigned)row_len, a.width = (unsigned)width;
  if (DRAW) {
    a.identity = (flags & DCTN_BATCH_IDENTITY_ORDER) ? 1u : 0u;
    a.G = (unsigned)G, a.S = (unsigned)(pad ? (n + G - 1) / G : n / G), a.offset = (unsigned)offset;
    a.bits = 2;
    while (a.bits < 31 && ((int64_t)1 << a.bits) < n) ++a.bits;
  }
  long long wgs = (count + BATCH_WAVES - 1) / BATCH_WAVES;
  const long long cap = dctn_dev().cus < BATCH_MAX_WGS ? (dctn_dev().cus < 1 ? 1 : dctn_dev().cus) : BATCH_MAX_WGS;
  if (wgs > cap) wgs = cap;
  const dim3 g((unsigned)wgs);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DCTN_F32) batch_launch_typed<float, DRAW>(a, kind, pad, g, st);
  else if (dtype == DCTN_F64) batch_launch_typed<double, DRAW>(a, kind, pad, g, st);
  else batch_launch_typed<bf16_t, DRAW>(a, kind, pad, g, st);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel(BATCH_NAMES[DRAW ? 0 : 1][kind][dtype]);
  return DCTN_OK;
}

}  // namespace

extern "C" {

size_t dctn_batch_state_bytes(void) { return sizeof(BatchState); }

int dctn_batch_draw(const void* src, const void* table, const void* labels, void* x, void* y, void* indices, void* state,
                    int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset, int64_t row_len, int width,
                    int src_kind, int flags, int dtype, void* stream) {
  BatchArgs a = {};
  a.src = src, a.table = table, a.labels = static_cast<const long long*>(labels);
  a.x = x, a.y = static_cast<long long*>(y), a.indices = static_cast<long long*>(indices);
  a.state = static_cast<BatchState*>(state);
  return batch_launch<true>(a, n, global_batch, local_batch, rank_offset, row_len, width, src_kind, flags, dtype, stream);
}

int dctn_batch_gather(const void* src, const void* table, const void* labels, const void* sample_idx, void* x, void* y,
                      void* indices, int64_t n, int64_t count, int64_t row_len, int width, int src_kind, int dtype,
                      void* stream) {
  BatchArgs a = {};
  a.src = src, a.table = table, a.labels = static_cast<const long long*>(labels);
  a.sample_idx = static_cast<const long long*>(sample_idx);
  a.x = x, a.y = static_cast<long long*>(y), a.indices = static_cast<long long*>(indices);
  return batch_launch<false>(a, n, 1, count, 0, row_len, width, src_kind, 0, dtype, stream);
}

}  // extern "C"
