// Device batch source for raw colour images (reference: get_cifar10_colored_data_loaders, dctn/dataset_loading.py:331-389 -
// to_tensor, the optional per-channel centring and scaling, the optional constant channel, the per-channel nu).  Every
// value that pipeline gives is a function of ONE byte and its channel, so a 256-row table per channel holds them all
// (dctn_amd/batches.py `colour_table` builds it with the reference's own ops) and the data set stays on the device as the
// interleaved bytes torchvision holds, a quarter to a fifth of the expanded float32 tensor.
//   src (n, P, C) uint8, table (W, 256), x (1, Bl, P, W):  x[0, j, p, c] = table[c][src[s_j, p, c]] for c < C and
//   table[c][0] for C <= c < W (the constant channel; W is C or C + 1).
// The order, the state block, the ticket, the flags and the padding are batch_source.hip's (draw_order.h); the kernel has
// batch_u8_k's shape: one WAVE per sample, the sample number wave-uniform.
//
// The table in LDS is planar, tab[c][value], as it is in global memory.  A lookup here reads ONE element (its channel's),
// never a pixel's whole row as batch_u8_k does, so the interleaved layout has no wide read to offer; and the bank of a
// lookup would be (W * value + c) mod 32 there, which for W = 4 (W = 2) uses 8 (16) of the 32 banks.  Planar, the bank is
// value mod 32 for 4-byte elements whatever W is (every channel's plane is a multiple of 128 bytes), value / 2 mod 32 for
// bf16 (two neighbouring values share a word), and a 64-bank pair for float64.  Byte-indexed lookups of independent
// pixels conflict at random in any layout; this one spreads them over every bank.
#include "draw_order.h"
#include "batch_plan.h"

namespace {

template <typename S, int C, int W, bool DRAW, bool PAD>
__global__ __launch_bounds__(BATCH_THREADS) void colour_k(BatchArgs a) {
  static_assert(1 <= C && C <= 4 && (W == C || W == C + 1) && W <= 4, "channels 1 .. 4, at most one constant column");
  typedef typename BatchBits<S>::type Tb;
  __shared__ Tb tab[W][256];
  __shared__ BatchHead head;
  {
    const Tb* g = static_cast<const Tb*>(a.table);   // aligned to its element size only: element by element
    Tb* t = &tab[0][0];
    for (int i = threadIdx.x; i < 256 * W; i += BATCH_THREADS) t[i] = g[i];
  }
  if (DRAW && threadIdx.x == 0) batch_read_head(a, head);
  __syncthreads();
  unsigned K[6] = {0u, 0u, 0u, 0u, 0u, 0u}, pos0 = 0u;
  if (DRAW) {
#pragma unroll
    for (int i = 0; i < 6; ++i) K[i] = __builtin_amdgcn_readfirstlane(head.K[i]);
    pos0 = __builtin_amdgcn_readfirstlane(head.pos0);
  }
  Tb constant = 0;   // the column no source byte feeds; instantiations with W == C hold no trace of it
  if constexpr (W > C) constant = tab[C][0];
  const unsigned lane = threadIdx.x % DCTN_WAVE;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * BATCH_WAVES + threadIdx.x / DCTN_WAVE);
  const unsigned P = a.row_len;
  const unsigned char* src = static_cast<const unsigned char*>(a.src);
  Tb* x = static_cast<Tb*>(a.x);
  // four pixels per step: 4 C bytes as C 32-bit loads (every row starts on a 4-byte boundary), 4 W elements of x on a
  // store boundary
  const bool vec = P % 4u == 0u && (uintptr_t)src % 4u == 0u && (uintptr_t)x % BatchGroup<Tb, 4 * W>::ALIGN == 0u;
  for (unsigned j = wave; j < a.Bl; j += gridDim.x * BATCH_WAVES) {
    const unsigned drawn = batch_sample<DRAW>(a, K, pos0, j);
    const bool padding = PAD && drawn >= a.n;   // wave-uniform
    const unsigned s = padding ? a.n - 1u : drawn;
    if (lane == 0) batch_report<PAD>(a, j, s, padding);
    const unsigned char* row = src + (size_t)s * P * C;   // 64-bit: n P C may pass 4 GiB
    Tb* out = x + (size_t)j * P * W;
    if (vec) {
      const unsigned* row4 = reinterpret_cast<const unsigned*>(row);
      const unsigned groups = P / 4u;
      for (unsigned g0 = lane; g0 < groups; g0 += DCTN_WAVE * BATCH_UNROLL) {
        unsigned bytes[BATCH_UNROLL][C];
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
#pragma unroll
          for (int c = 0; c < C; ++c) bytes[u][c] = g < groups ? row4[(size_t)g * C + c] : 0u;
        }
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
          if (g >= groups) break;
          Tb v[4 * W];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
              if (c < C) {
                const int k = p * C + c;   // byte k of the group: pixel p, channel c
                v[p * W + c] = tab[c][(bytes[u][k / 4] >> (8 * (k % 4))) & 255u];
              } else {
                v[p * W + c] = constant;
              }
            }
          }
          BatchGroup<Tb, 4 * W>::store(out + (size_t)g * 4 * W, v);
        }
      }
    } else {
      for (unsigned p = lane; p < P; p += DCTN_WAVE) {
#pragma unroll
        for (int c = 0; c < W; ++c) out[(size_t)p * W + c] = c < C ? tab[c][row[(size_t)p * C + c]] : constant;
      }
    }
  }
  if (DRAW && threadIdx.x == 0) batch_take_ticket(a, head.k);
}

template <typename S, int C, bool DRAW, bool PAD>
void colour_launch_width(const BatchArgs& a, int width, dim3 g, hipStream_t st) {
  const dim3 b(BATCH_THREADS);
  if (width == C) hipLaunchKernelGGL((colour_k<S, C, C, DRAW, PAD>), g, b, 0, st, a);
  else if constexpr (C < 4) hipLaunchKernelGGL((colour_k<S, C, C + 1, DRAW, PAD>), g, b, 0, st, a);
}

template <typename S, bool DRAW, bool PAD>
void colour_launch_padded(const BatchArgs& a, int channels, int width, dim3 g, hipStream_t st) {
  switch (channels) {
    case 1: colour_launch_width<S, 1, DRAW, PAD>(a, width, g, st); break;
    case 2: colour_launch_width<S, 2, DRAW, PAD>(a, width, g, st); break;
    case 3: colour_launch_width<S, 3, DRAW, PAD>(a, width, g, st); break;
    default: colour_launch_width<S, 4, DRAW, PAD>(a, width, g, st); break;
  }
}

template <typename S, bool DRAW>
void colour_launch_typed(const BatchArgs& a, int channels, int width, bool pad, dim3 g, hipStream_t st) {
  if constexpr (DRAW) {   // a gather has no positions to pad
    if (pad) return colour_launch_padded<S, true, true>(a, channels, width, g, st);
  }
  colour_launch_padded<S, DRAW, false>(a, channels, width, g, st);
}

template <bool DRAW>
void colour_launch_op(const BatchArgs& a, const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st) {
  const dim3 g(p.wgs);
  if (c.dtype == DCTN_F32) colour_launch_typed<float, DRAW>(a, p.channels, c.width, p.pad, g, st);
  else if (c.dtype == DCTN_F64) colour_launch_typed<double, DRAW>(a, p.channels, c.width, p.pad, g, st);
  else colour_launch_typed<bf16_t, DRAW>(a, p.channels, c.width, p.pad, g, st);
}

}  // namespace

// batch_call.hip has checked and planned the launch
void colour_source_launch(const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st) {
  const BatchArgs a = batch_args(c, p);
  if (p.draw) colour_launch_op<true>(a, c, p, st);
  else colour_launch_op<false>(a, c, p, st);
}
