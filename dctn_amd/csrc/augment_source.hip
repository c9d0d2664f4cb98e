// Augmented draws of the two byte-resident batch sources: a random shift (pad by max_shift with a fill byte, crop) and a
// horizontal flip, applied to the BYTES of a sample before the table lookup of batch_source.hip (grey, (256, Q) table) or
// colour_source.hip (interleaved channels, (W, 256) planar tables).  include/dctn_amd.h holds the normative definition;
// dctn_amd/batches.py `augment_params` / `augment_bytes` restate it.  The parameters of a slot are a pure function of
// (seed, epoch, global position) - one Philox4x32-10 call, counter (g, 0, e, DCTN_AUG_TAG) - so they need no state: the
// order, the 16-byte block, the ticket, y and indices are draw_order.h's, unchanged.
//
// The kernels keep the siblings' shape: one WAVE per sample, the sample number and (dy, dx, flip) wave-uniform, the table
// staged in LDS behind the one workgroup barrier, four pixels' worth of output per lane and step in 16-byte stores
// (BatchGroup).  What does not survive a byte shift is the aligned 32-bit load of four pixels: dx * C is no multiple of 4
// and a flip reverses the pixels.  So a wave first copies its sample's bytes as they are - aligned 32-bit loads, four in
// flight per lane, independent of the shift - into a wave-private LDS region, and its lanes then pick the shifted or
// flipped bytes out of that region one by one (or the fill byte outside the image) and pack them into the words the
// aligned load would have given; from there on the lookup and the store are the siblings'.  The region is private to the
// wave: LDS operations of one wave complete in order, so no barrier is needed, only a wavefront-scope fence that keeps
// the compiler from moving the reads above the writes (and the next sample's writes above this one's reads).
//
// LDS: the table (256 * W elements, at most 8 KiB) + BATCH_WAVES regions of round_up(H * Wd * C, 16) bytes, dynamic.  A
// region is at most AUG_WAVE_LDS = 13 KiB (64 x 64 x 3 is 12 KiB), which keeps the workgroup below the 64 KiB that need no
// opt-in; a larger sample is DCTN_ERR_UNSUPPORTED before any launch.
#include "draw_order.h"
#include "batch_plan.h"

namespace {

struct AugArgs {   // passed by value in the kernel argument
  BatchArgs b;     // row_len = H * Wd pixels
  unsigned H, Wd;
  unsigned m, hflip;   // max_shift; DCTN_AUG_HFLIP set
  unsigned fill;       // channel c's fill byte in bits 8 c .. 8 c + 7
  unsigned region;     // bytes of a wave's LDS region: a multiple of 16
};

struct AugSlot {   // wave-uniform
  int dy, dx;
  unsigned flip;
};

template <typename Tb, int Q> struct alignas((Q & (Q - 1)) == 0 ? (Q * sizeof(Tb) > 16 ? 16 : Q * sizeof(Tb)) : sizeof(Tb)) AugEntry {
  Tb e[Q];   // a row of the grey table, read in one LDS access where Q is a power of two
};

extern __shared__ __attribute__((aligned(16))) unsigned char aug_regions[];

// the seed words: thread 0, beside batch_read_head (which keeps the round keys, not the seed)
struct AugSeed {
  unsigned k0, k1;
};

__device__ __forceinline__ void aug_read_seed(const BatchArgs& a, AugSeed& seed) {
  seed.k0 = __hip_atomic_load(&a.state->seed_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  seed.k1 = __hip_atomic_load(&a.state->seed_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (dy, dx, flip) of global position g in epoch e: multiply-high maps a 32-bit word onto [0, 2 m + 1)
__device__ __forceinline__ AugSlot aug_slot(const AugArgs& a, unsigned k0, unsigned k1, unsigned epoch, unsigned g) {
  unsigned w[4];
  philox4x32_10(g, 0u, epoch, DCTN_AUG_TAG, k0, k1, w);
  const unsigned span = 2u * a.m + 1u;
  AugSlot s;
  s.dy = __builtin_amdgcn_readfirstlane((int)__umulhi(w[0], span) - (int)a.m);
  s.dx = __builtin_amdgcn_readfirstlane((int)__umulhi(w[1], span) - (int)a.m);
  s.flip = __builtin_amdgcn_readfirstlane(a.hflip ? w[2] >> 31 : 0u);
  return s;
}

// orders this wave's LDS accesses for the compiler; the hardware completes one wave's LDS operations in order
__device__ __forceinline__ void aug_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sample's bytes, as they are, into the wave's region
__device__ __forceinline__ void aug_stage(unsigned char* region, const unsigned char* row, unsigned bytes, bool words,
                                          unsigned lane) {
  if (words) {
    const unsigned* row4 = reinterpret_cast<const unsigned*>(row);
    unsigned* region4 = reinterpret_cast<unsigned*>(region);
    const unsigned n4 = bytes / 4u;
    for (unsigned i0 = lane; i0 < n4; i0 += DCTN_WAVE * BATCH_UNROLL) {
      unsigned t[BATCH_UNROLL];
#pragma unroll
      for (int u = 0; u < BATCH_UNROLL; ++u) {
        const unsigned i = i0 + u * DCTN_WAVE;
        t[u] = i < n4 ? row4[i] : 0u;
      }
#pragma unroll
      for (int u = 0; u < BATCH_UNROLL; ++u) {
        const unsigned i = i0 + u * DCTN_WAVE;
        if (i < n4) region4[i] = t[u];
      }
    }
  } else {
    for (unsigned i = lane; i < bytes; i += DCTN_WAVE) region[i] = row[i];
  }
}

// the C source bytes of output pixel (h, w): row h + dy, column wf + dx of the staged sample, the fill outside it.  The
// LDS read is unconditional (byte 0 of the region outside the image), so the lanes do not diverge.
template <int C>
__device__ __forceinline__ void aug_pixel(const unsigned char* region, const AugArgs& a, const AugSlot& s, unsigned h,
                                          unsigned w, unsigned (&b)[C]) {
  const unsigned wf = s.flip ? a.Wd - 1u - w : w;
  const unsigned hs = h + (unsigned)s.dy, ws = wf + (unsigned)s.dx;   // a negative sum wraps far above H, Wd < 2^31
  const bool inside = hs < a.H && ws < a.Wd;
  const unsigned at = inside ? (hs * a.Wd + ws) * C : 0u;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned v = region[at + c];
    b[c] = inside ? v : (a.fill >> (8 * c)) & 255u;
  }
}

// the 4 C bytes of output pixels 4 g .. 4 g + 3 (row-major over (H, Wd): a group may run over a row's end), packed as the
// siblings' C aligned 32-bit loads give them: byte k = p * C + c in word k / 4, bits 8 (k % 4) ..
template <int C>
__device__ __forceinline__ void aug_group(const unsigned char* region, const AugArgs& a, const AugSlot& s, unsigned g,
                                          unsigned (&out)[C]) {
  unsigned h = 4u * g / a.Wd, w = 4u * g - h * a.Wd;
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = 0u;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned b[C];
    aug_pixel<C>(region, a, s, h, w, b);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int k = p * C + c;
      out[k / 4] |= b[c] << (8 * (k % 4));
    }
    if (++w == a.Wd) w = 0u, ++h;
  }
}

// what both kernels do before their sample loop
struct AugWave {
  unsigned K[6], pos0, k0, k1, epoch, lane, wave;
  unsigned char* region;
};

__device__ __forceinline__ void aug_wave_setup(const AugArgs& a, const BatchHead& head, const AugSeed& seed, AugWave& v) {
#pragma unroll
  for (int i = 0; i < 6; ++i) v.K[i] = __builtin_amdgcn_readfirstlane(head.K[i]);
  v.pos0 = __builtin_amdgcn_readfirstlane(head.pos0);
  v.k0 = __builtin_amdgcn_readfirstlane(seed.k0), v.k1 = __builtin_amdgcn_readfirstlane(seed.k1);
  v.epoch = __builtin_amdgcn_readfirstlane(head.k) / a.b.S;
  v.lane = threadIdx.x % DCTN_WAVE;
  const unsigned in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x / DCTN_WAVE);
  v.wave = blockIdx.x * BATCH_WAVES + in_wg;
  v.region = aug_regions + in_wg * a.region;
}

// grey: x[0, j, h, w, :] = table[b, :]
template <typename S, int Q>
__global__ __launch_bounds__(BATCH_THREADS) void aug_u8_k(AugArgs a) {
  typedef typename BatchBits<S>::type Tb;
  __shared__ AugEntry<Tb, Q> tab[256];
  __shared__ BatchHead head;
  __shared__ AugSeed seed;
  {
    const Tb* g = static_cast<const Tb*>(a.b.table);   // aligned to its element size only: element by element
    Tb* t = &tab[0].e[0];
    for (int i = threadIdx.x; i < 256 * Q; i += BATCH_THREADS) t[i] = g[i];
  }
  if (threadIdx.x == 0) batch_read_head(a.b, head), aug_read_seed(a.b, seed);
  __syncthreads();
  AugWave v;
  aug_wave_setup(a, head, seed, v);
  const unsigned P = a.b.row_len, lane = v.lane;
  const unsigned char* src = static_cast<const unsigned char*>(a.b.src);
  Tb* x = static_cast<Tb*>(a.b.x);
  const bool words = P % 4u == 0u && (uintptr_t)src % 4u == 0u;   // every row starts on a 4-byte boundary
  const bool vec = P % 4u == 0u && (uintptr_t)x % BatchGroup<Tb, 4 * Q>::ALIGN == 0u;
  for (unsigned j = v.wave; j < a.b.Bl; j += gridDim.x * BATCH_WAVES) {
    const unsigned s = batch_sample<true>(a.b, v.K, v.pos0, j);
    if (lane == 0) batch_report<false>(a.b, j, s, false);
    const AugSlot slot = aug_slot(a, v.k0, v.k1, v.epoch, v.pos0 + j);
    aug_wave_sync();   // the previous sample's reads are done
    aug_stage(v.region, src + (size_t)s * P, P, words, lane);
    aug_wave_sync();
    Tb* out = x + (size_t)j * P * Q;
    if (vec) {
      const unsigned groups = P / 4u;
      for (unsigned g0 = lane; g0 < groups; g0 += DCTN_WAVE * BATCH_UNROLL) {
        unsigned four[BATCH_UNROLL][1];
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
          four[u][0] = 0u;
          if (g < groups) aug_group<1>(v.region, a, slot, g, four[u]);
        }
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
          if (g >= groups) break;
          Tb val[4 * Q];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const AugEntry<Tb, Q> e = tab[(four[u][0] >> (8 * p)) & 255u];
#pragma unroll
            for (int q = 0; q < Q; ++q) val[p * Q + q] = e.e[q];
          }
          BatchGroup<Tb, 4 * Q>::store(out + (size_t)g * 4 * Q, val);
        }
      }
    } else {
      for (unsigned p = lane; p < P; p += DCTN_WAVE) {
        const unsigned h = p / a.Wd;
        unsigned b[1];
        aug_pixel<1>(v.region, a, slot, h, p - h * a.Wd, b);
        const AugEntry<Tb, Q> e = tab[b[0]];
#pragma unroll
        for (int q = 0; q < Q; ++q) out[(size_t)p * Q + q] = e.e[q];
      }
    }
  }
  if (threadIdx.x == 0) batch_take_ticket(a.b, head.k);
}

// colour: x[0, j, h, w, c] = table[c][b_c] for c < C, table[C][0] for the constant column
template <typename S, int C, int W>
__global__ __launch_bounds__(BATCH_THREADS) void aug_cols_k(AugArgs a) {
  static_assert(1 <= C && C <= 4 && (W == C || W == C + 1) && W <= 4, "channels 1 .. 4, at most one constant column");
  typedef typename BatchBits<S>::type Tb;
  __shared__ Tb tab[W][256];   // planar, as colour_source.hip explains
  __shared__ BatchHead head;
  __shared__ AugSeed seed;
  {
    const Tb* g = static_cast<const Tb*>(a.b.table);   // aligned to its element size only: element by element
    Tb* t = &tab[0][0];
    for (int i = threadIdx.x; i < 256 * W; i += BATCH_THREADS) t[i] = g[i];
  }
  if (threadIdx.x == 0) batch_read_head(a.b, head), aug_read_seed(a.b, seed);
  __syncthreads();
  AugWave v;
  aug_wave_setup(a, head, seed, v);
  Tb constant = 0;   // the column no source byte feeds
  if constexpr (W > C) constant = tab[C][0];
  const unsigned P = a.b.row_len, lane = v.lane;
  const unsigned char* src = static_cast<const unsigned char*>(a.b.src);
  Tb* x = static_cast<Tb*>(a.b.x);
  const bool words = (P * C) % 4u == 0u && (uintptr_t)src % 4u == 0u;   // every row starts on a 4-byte boundary
  const bool vec = P % 4u == 0u && (uintptr_t)x % BatchGroup<Tb, 4 * W>::ALIGN == 0u;
  for (unsigned j = v.wave; j < a.b.Bl; j += gridDim.x * BATCH_WAVES) {
    const unsigned s = batch_sample<true>(a.b, v.K, v.pos0, j);
    if (lane == 0) batch_report<false>(a.b, j, s, false);
    const AugSlot slot = aug_slot(a, v.k0, v.k1, v.epoch, v.pos0 + j);
    aug_wave_sync();   // the previous sample's reads are done
    aug_stage(v.region, src + (size_t)s * P * C, P * C, words, lane);   // 64-bit: n P C may pass 4 GiB
    aug_wave_sync();
    Tb* out = x + (size_t)j * P * W;
    if (vec) {
      const unsigned groups = P / 4u;
      for (unsigned g0 = lane; g0 < groups; g0 += DCTN_WAVE * BATCH_UNROLL) {
        unsigned bytes[BATCH_UNROLL][C];
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
#pragma unroll
          for (int c = 0; c < C; ++c) bytes[u][c] = 0u;
          if (g < groups) aug_group<C>(v.region, a, slot, g, bytes[u]);
        }
#pragma unroll
        for (int u = 0; u < BATCH_UNROLL; ++u) {
          const unsigned g = g0 + u * DCTN_WAVE;
          if (g >= groups) break;
          Tb val[4 * W];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
              if (c < C) {
                const int k = p * C + c;   // byte k of the group: pixel p, channel c
                val[p * W + c] = tab[c][(bytes[u][k / 4] >> (8 * (k % 4))) & 255u];
              } else {
                val[p * W + c] = constant;
              }
            }
          }
          BatchGroup<Tb, 4 * W>::store(out + (size_t)g * 4 * W, val);
        }
      }
    } else {
      for (unsigned p = lane; p < P; p += DCTN_WAVE) {
        const unsigned h = p / a.Wd;
        unsigned b[C];
        aug_pixel<C>(v.region, a, slot, h, p - h * a.Wd, b);
#pragma unroll
        for (int c = 0; c < C; ++c) out[(size_t)p * W + c] = tab[c][b[c]];
        if constexpr (W > C) out[(size_t)p * W + C] = constant;
      }
    }
  }
  if (threadIdx.x == 0) batch_take_ticket(a.b, head.k);
}

template <typename S>
void aug_launch_u8(const AugArgs& a, dim3 g, size_t lds, hipStream_t st) {
  const dim3 b(BATCH_THREADS);
  switch (a.b.width) {
    case 1: hipLaunchKernelGGL((aug_u8_k<S, 1>), g, b, lds, st, a); break;
    case 2: hipLaunchKernelGGL((aug_u8_k<S, 2>), g, b, lds, st, a); break;
    case 3: hipLaunchKernelGGL((aug_u8_k<S, 3>), g, b, lds, st, a); break;
    default: hipLaunchKernelGGL((aug_u8_k<S, 4>), g, b, lds, st, a); break;
  }
}

template <typename S, int C>
void aug_launch_width(const AugArgs& a, dim3 g, size_t lds, hipStream_t st) {
  const dim3 b(BATCH_THREADS);
  if (a.b.width == C) hipLaunchKernelGGL((aug_cols_k<S, C, C>), g, b, lds, st, a);
  else if constexpr (C < 4) hipLaunchKernelGGL((aug_cols_k<S, C, C + 1>), g, b, lds, st, a);
}

template <typename S>
void aug_launch_typed(const AugArgs& a, bool grey, int channels, dim3 g, size_t lds, hipStream_t st) {
  if (grey) return aug_launch_u8<S>(a, g, lds, st);
  switch (channels) {
    case 1: aug_launch_width<S, 1>(a, g, lds, st); break;
    case 2: aug_launch_width<S, 2>(a, g, lds, st); break;
    case 3: aug_launch_width<S, 3>(a, g, lds, st); break;
    default: aug_launch_width<S, 4>(a, g, lds, st); break;
  }
}

}  // namespace

// batch_call.hip has checked and planned the launch: a draw of one of the two byte sources.  The grey form has one
// source channel, which goes through a (256, width) table.
void augment_source_launch(const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st) {
  AugArgs a = {};
  a.b = batch_args(c, p);
  a.H = (unsigned)c.height, a.Wd = (unsigned)c.width_px, a.m = (unsigned)c.max_shift;
  a.hflip = (c.aug_flags & DCTN_AUG_HFLIP) ? 1u : 0u, a.fill = c.fill, a.region = p.region;
  const bool grey = c.src_kind == DCTN_BATCH_SRC_U8_TABLE;
  const dim3 g(p.wgs);
  const size_t lds = (size_t)p.region * BATCH_WAVES;
  if (c.dtype == DCTN_F32) aug_launch_typed<float>(a, grey, p.channels, g, lds, st);
  else if (c.dtype == DCTN_F64) aug_launch_typed<double>(a, grey, p.channels, g, lds, st);
  else aug_launch_typed<bf16_t>(a, grey, p.channels, g, lds, st);
}
