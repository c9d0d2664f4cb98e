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
#include "draw_order.h"
#include "batch_plan.h"

namespace {

template <typename Tb, int Q> struct alignas((Q & (Q - 1)) == 0 ? (Q * sizeof(Tb) > 16 ? 16 : Q * sizeof(Tb)) : sizeof(Tb)) BatchEntry {
  Tb e[Q];
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

template <bool DRAW>
void batch_launch_op(const BatchArgs& a, const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st) {
  const dim3 g(p.wgs);
  if (c.dtype == DCTN_F32) batch_launch_typed<float, DRAW>(a, c.src_kind, p.pad, g, st);
  else if (c.dtype == DCTN_F64) batch_launch_typed<double, DRAW>(a, c.src_kind, p.pad, g, st);
  else batch_launch_typed<bf16_t, DRAW>(a, c.src_kind, p.pad, g, st);
}

}  // namespace

// batch_call.hip has checked and planned the launch
void batch_source_launch(const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st) {
  const BatchArgs a = batch_args(c, p);
  if (p.draw) batch_launch_op<true>(a, c, p, st);
  else batch_launch_op<false>(a, c, p, st);
}
