// What the batch kernels of batch_source.hip and colour_source.hip share: the 16-byte state block, the epoch order (a
// 6-round Feistel network with cycle walking, keyed by Philox4x32-10), the read of the block and the ticket that advances
// it, the sample of a slot, the label and index it reports, and the wide store of four pixels' worth of output.  ONE
// definition of the order: include/dctn_amd.h holds the normative text; dctn_amd/batches.py restates it in Python.
#pragma once
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
  unsigned row_len, width;       // U8_TABLE: pixels P, table columns Q;  ROWS: elements R, channels C;  colour: pixels P, columns W
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

// 4 pixels' worth of table entries, N elements (N = 4 x the columns of a pixel), as 16-byte stores (8-byte ones for bf16
// with an odd number of columns)
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

}  // namespace
