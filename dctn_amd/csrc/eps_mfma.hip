// MFMA EPS kernels, family "q2-reg": Q == 2 and a core small enough to live in registers
// (N = K*K*C in {8, 9}: the 3x3 single-channel MNIST layer of BASELINE config 2 and the 2x2
// two-channel layer).  Operands are bf16, accumulation f32 (v_mfma_f32_32x32x16_bf16).
//
// Forward (replaces dctn/eps.py:19-40).  The reference's path is K-R half 0, K-R half 1, one GEMM
// core x half0, a per-window dot with half 1.  Here, with a = index over the first n0 factors
// (A = 2^n0), b over the last n1 (Bn = 2^n1):
//     T[(b,o), w] = sum_a core[a,b,o] * P0[w,a]      <- MFMA, M = (b,o) rows, N = 32 windows, K = a
//     out[w,o]    = sum_b P1[w,b] * T[(b,o), w]      <- lane-local epilogue
// A lane owns ONE window, 64 windows per wave step (the kernels are bounded by VALU issue, so no
// lane may repeat another lane's loads, address arithmetic or products): it builds the whole P0
// row of its window in registers; the MFMA tile has only 32 columns, so the step runs as two
// "sets" (windows of lanes 0-31, then of lanes 32-63) and v_permlane32_swap turns the two k-halves
// a lane built for its own window into its operand share for set 0 and for set 1.  Each lane gets
// 16 rows (b,o) of T per tile back, weights them with P1 of the set's window (also handed over by
// permlane swaps), and one more swap per output joins the two row halves so that every lane ends
// up with the outputs of its own window.  Nothing but x and out touches HBM; no LDS in the main
// loop, no barriers.
//
// Work decomposition: a wave owns 64 consecutive window POSITIONS of the image (lane = position) and
// loops over a chunk of samples.  All addressing then is "per-lane constant + per-sample scalar":
// x, dY and out are accessed through raw buffer descriptors (buffer_load / buffer_store with the lane
// part in the VGPR offset and the sample / row part in the scalar offset), so the main loop holds no
// address arithmetic at all, lanes without a position and the 16-byte row load that would run past
// the end of x are handled by the hardware range check (probe: tools/bufprobe.hip), and everything
// that depends only on the position (in the fused-head backward: the lane's slice of the classifier
// weight) is loaded once per wave.
//
// Backward dCore[a,b,o] = sum_w P0[w,a] P1[w,b] dY[w,o]  reduces over windows, so windows must
// become the MFMA K index while lanes own windows: both operands of
//     Z[w,(b,o)] = P1[w,b] dY[w,o];   dCoreT[(b,o), a] += Zt (A operand) x P0t (B operand)
// need a transpose.  For the 3x3 shape (A = 32, <= 64 rows (b,o)) every lane writes the bf16 row of
// its own window into a per-wave LDS tile and the operand fragments come back through the hardware
// transpose read ds_read_b64_tr_b16 (swizzled 64-byte rows: conflict-free both ways).  The wider
// shapes transpose ON the matrix core instead: multiplying the lane-owns-window fragment (as A
// operand) by an identity B operand returns the tile with the feature index on the lane and 16
// windows in the accumulator registers - the layout the next MFMA consumes as an operand summing over
// windows (more MFMAs, conversions and lane swaps, but no LDS tiles).
// Per-wave partial sums stay in registers over all of the wave's samples, are reduced over the
// workgroup's waves in LDS, written to a workspace and summed by a second small kernel
// (deterministic: no float atomics).  With the classifier head fused (HEADC > 0) the same pass forms
// dY from dLogits and the head weight and accumulates the head's own gradients.
#include "common.h"

#include <cstdlib>
#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(2))) int int2v;
typedef __attribute__((ext_vector_type(4))) int int4v;
typedef __attribute__((ext_vector_type(2))) float f32x2;

namespace {

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

template <typename S> __device__ __forceinline__ float to_f32(S v) { return (float)v; }

// sum over the two lane halves (lane l and l^32), result in every lane
__device__ __forceinline__ float half_sum(float v) {
  const int iv = __float_as_int(v);
  const int2v r = __builtin_amdgcn_permlane32_swap(iv, iv, false, false);
  return __int_as_float(r[0]) + __int_as_float(r[1]);
}

// a <- [a.lo, b.lo], b <- [a.hi, b.hi]  (lo / hi = lanes 0-31 / 32-63): with a, b = the values a lane
// computed for the first / second lane half's role, a becomes the operand of set 0 (windows of lanes
// 0-31) and b the operand of set 1 (windows of lanes 32-63).
__device__ __forceinline__ void swap_halves(float& a, float& b) {
  const int2v r = __builtin_amdgcn_permlane32_swap(__float_as_int(a), __float_as_int(b), false, false);
  a = __int_as_float(r[0]);
  b = __int_as_float(r[1]);
}
__device__ __forceinline__ void swap_halves(bf16x8& a, bf16x8& b) {
  int4v ia = __builtin_bit_cast(int4v, a), ib = __builtin_bit_cast(int4v, b);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int2v r = __builtin_amdgcn_permlane32_swap(ia[i], ib[i], false, false);
    ia[i] = r[0];
    ib[i] = r[1];
  }
  a = __builtin_bit_cast(bf16x8, ia);
  b = __builtin_bit_cast(bf16x8, ib);
}

// LDS hand-over inside one wave (writes of all lanes visible to the reads of all lanes)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Transposition tiles of the dCore kernel: [64 windows][32 features] bf16, 64-byte rows, the four
// 16-byte chunks of row w rotated by (w >> 1) & 3.  With that rotation both sides are conflict-free:
// the row writes (ds_write_b128, 32-bank rule: 8 consecutive lanes cover 8 distinct 4-bank sets) and
// the hardware transpose reads (ds_read_b64_tr_b16, 64-bank rule: the 4 rows of a block are 16 banks
// apart and the 8 eight-byte units of a row keep distinct chunks), and every address is a per-lane
// constant plus a compile-time offset.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
constexpr int LROW = 32;   // shorts per row
struct TrLane {
  int wr[4];      // short offset inside a tile of logical chunk c of the lane's own row
  int rd_lo, rd_hi;   // short offsets of the lane's two transpose-read addresses at k-step 0
};
__device__ __forceinline__ TrLane tr_lane(int lane) {
  TrLane t;
#pragma unroll
  for (int c = 0; c < 4; ++c) t.wr[c] = lane * LROW + (((c + (lane >> 1)) & 3) << 3);
  // reader: 16-lane group g, lane 4q + p of it supplies row q, columns 4p..4p+3 of the block whose
  // rows are windows 16 ks + 8 (g >> 1) + {0..3} (lo) / {4..7} (hi), columns features 16 (g & 1) + ..
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int lc = 2 * (g & 1) + (pp >> 1), half = pp & 1;
  const int row = 8 * (g >> 1) + q;
  t.rd_lo = row * LROW + (((lc + (row >> 1)) & 3) << 3) + 4 * half;
  t.rd_hi = (row + 4) * LROW + (((lc + ((row + 4) >> 1)) & 3) << 3) + 4 * half;
  return t;
}
// One 32x32x16 bf16 operand fragment with the hardware transpose read (cdna_hip_programming.md T10):
// lane (r, h) gets feature r of windows 16 ks + 8 h + j, j = 0..7 - the windows on the MFMA k index.
// Lane i of a 16-lane group receives column i of the group's 4 rows.  EXEC must be all ones.
__device__ __forceinline__ bf16x8 tr_frag(const short* tile, int ks, const TrLane& t) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + t.rd_lo + ks * 16 * LROW));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + t.rd_hi + ks * 16 * LROW));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// unsigned 32-bit division by an invariant (Granlund-Montgomery, round-up variant):
//   q = (t + ((n - t) >> s1)) >> s2,  t = umulhi(M, n)
struct FastDiv {
  unsigned M, s1, s2;
};
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv& d) {
  const unsigned t = __umulhi(d.M, n);
  return (t + ((n - t) >> d.s1)) >> d.s2;
}

#define MFMA_MAXN 16
struct MfmaP {
  int C, B, K, O, Ho, Wo;
  int P;                        // window positions per sample = Ho * Wo
  int npg;                      // position groups of 64
  int spc, nchunks;             // samples per wave, number of sample chunks
  unsigned foffb[MFMA_MAXN];    // BYTE offset of factor n relative to the window's top-left pixel
  unsigned rowoffb[MFMA_MAXN];  // row loads: BYTE offset of window row (dh, ch), index dh*C + ch
  unsigned s1b, s2b, s3b, s4b;  // byte strides of x (batch, row, column, feature)
  unsigned x_bytes;             // extent of x in bytes (< 2^31: buffer range check, 32-bit offsets)
  unsigned o_bytes, o_s1b;      // extent of out / dY in bytes (< 2^31), bytes per sample
  FastDiv div_wo;
  int rowvec_ok;                // one 16-byte load per window row usable (bf16, Q=2 contiguous, K <= 4)
  int vec_ok;                   // x: last stride 1, even strides, 4-byte aligned base (pair loads)
  int Cout;                     // fused-head backward: number of classes (rows of the head weight)
  unsigned hw_rowb, hw_bytes;   //   bytes per row (P * O * 2) and in total
  int ncb;                      //   chunk blocks (8 sample chunks each) of the grouped wave mapping
  int skew;                     //   grouped mapping: the first half of a block's waves takes spc + skew samples each, the second spc - skew
  int opts;                     // DCTN_OPT_* flags of the call
  unsigned npg_rcp;             // ceil(2^16 / npg): ticket / npg = (ticket * npg_rcp) >> 16 (exact below 2^16 / npg)
#ifdef DCTN_STAMPS
  unsigned long long* stamps;   // diagnostic build only (tools/stamp_cfg2.hip): per-workgroup phase time stamps
#endif
};

#ifdef DCTN_STAMPS
// 100 MHz wall clock, comparable across workgroups; written by wave 0 / lane 0 to memory nothing else reads
#define DCTN_STAMP(P, SLOT)                                                                      \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    unsigned long long t_;                                                                       \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
    if ((P).stamps && threadIdx.x == 0) (P).stamps[(long long)blockIdx.x * 8 + (SLOT)] = t_;     \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
static unsigned long long* g_stamps = nullptr;
void dctn_stamps_set(unsigned long long* p) { g_stamps = p; }
// the finishing kernel has no parameter block: its stamps go through a device global
__device__ unsigned long long* g_dev_stamps = nullptr;
void dctn_reduce_stamps_set(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dev_stamps), &p, sizeof(p)); }
#define DCTN_STAMP_T(P, SLOT, TID)                                                              \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    unsigned long long t_;                                                                       \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
    if ((P).stamps && threadIdx.x == (TID)) (P).stamps[(long long)blockIdx.x * 8 + (SLOT)] = t_;  \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
// the dW role waves of the dCore kernel: the first role wave's lane 0, in the rows behind DCTN_STAMP_ROLE_ROW
#define DCTN_STAMP_ROLE_ROW 1024
#define DCTN_STAMP_R(P, SLOT)                                                                    \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    unsigned long long t_;                                                                       \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
    if ((P).stamps && threadIdx.x == 64 * 8)                                                     \
      (P).stamps[(long long)(DCTN_STAMP_ROLE_ROW + blockIdx.x) * 8 + (SLOT)] = t_;               \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
// every dCore wave's lane 0, slot = wave index, in the rows behind DCTN_STAMP_WAVE_ROW
#define DCTN_STAMP_WAVE_ROW 1536
#define DCTN_STAMP_W(P, WV)                                                                      \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    unsigned long long t_;                                                                       \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
    if ((P).stamps && (threadIdx.x & 63) == 0 && (WV) < 8)                                        \
      (P).stamps[(long long)(DCTN_STAMP_WAVE_ROW + blockIdx.x) * 8 + (WV)] = t_;                 \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
#define DCTN_STAMP_G(SLOT)                                                                       \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    unsigned long long t_;                                                                       \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
    if (g_dev_stamps && threadIdx.x == 0) g_dev_stamps[(long long)blockIdx.x * 8 + (SLOT)] = t_;  \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
#else
#define DCTN_STAMP(P, SLOT) do { } while (0)
#define DCTN_STAMP_T(P, SLOT, TID) do { } while (0)
#define DCTN_STAMP_G(SLOT) do { } while (0)
#define DCTN_STAMP_R(P, SLOT) do { } while (0)
#define DCTN_STAMP_W(P, WV) do { } while (0)
#endif

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* ptr, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, (int)bytes, 0x00020000);
}

// Raw features of one window, as loaded: the loads are issued back to back with no control flow
// between them and no use of the data, so a whole step's loads are in flight together and the next
// step's can be issued before this one is consumed.  Lanes without a window position carry an
// out-of-range offset and read zeros.
template <typename S, int N, bool VEC, int ROWS>
struct RawWindow {
  u32x4 row[ROWS > 0 ? ROWS : 1];  // row-vector mode (bf16): K pixels of one window row per 16-byte load
  unsigned v[(ROWS == 0 && VEC) ? N * (int)(sizeof(S) / 2) : 1];  // pair mode: both features of a factor
  unsigned e[(ROWS == 0 && !VEC) ? 2 * N : 1];                    // scalar mode: raw bits per feature
};

// ROWS > 0: row-vector mode with ROWS = K*C rows (one buffer_load_dwordx4 per row instead of K
// dword loads: 3x fewer memory requests per window for the 3x3 kernel)
template <typename S, int N, bool VEC, int ROWS>
__device__ __forceinline__ void issue_window(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff,
                                             const MfmaP& p, RawWindow<S, N, VEC, ROWS>& raw) {
  if constexpr (ROWS > 0) {
#pragma unroll
    for (int rw = 0; rw < ROWS; ++rw)
      raw.row[rw] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff + p.rowoffb[rw], 0);
  } else if constexpr (VEC) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      if constexpr (sizeof(S) == 2) {
        raw.v[n] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff + p.foffb[n], 0);
      } else {
        const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff + p.foffb[n], 0);
        raw.v[2 * n] = t.x;
        raw.v[2 * n + 1] = t.y;
      }
    }
  } else {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if constexpr (sizeof(S) == 2)
          raw.e[2 * n + q] = (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(
              rs, voff, soff + p.foffb[n] + q * p.s4b, 0);
        else
          raw.e[2 * n + q] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff + p.foffb[n] + q * p.s4b, 0);
      }
  }
}

template <typename S, int N, bool VEC, int ROWS>
__device__ __forceinline__ void unpack_window(const RawWindow<S, N, VEC, ROWS>& raw, float (&xv)[N][2]) {
  if constexpr (ROWS > 0) {
    constexpr int KK = N / ROWS;          // pixels per row = K
    constexpr int CC = ROWS * ROWS / N;   // channels: ROWS = K*C and N = K*K*C
#pragma unroll
    for (int rw = 0; rw < ROWS; ++rw) {
      const unsigned d[4] = {raw.row[rw].x, raw.row[rw].y, raw.row[rw].z, raw.row[rw].w};
#pragma unroll
      for (int dw = 0; dw < KK; ++dw) {
        // factor n = (dh*K + dw)*C + ch for row rw = dh*C + ch
        const int n = ((rw / CC) * KK + dw) * CC + (rw % CC);
        xv[n][0] = __uint_as_float(d[dw] << 16);
        xv[n][1] = __uint_as_float(d[dw] & 0xffff0000u);
      }
    }
  } else if constexpr (VEC) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      if constexpr (sizeof(S) == 2) {
        xv[n][0] = __uint_as_float(raw.v[n] << 16);
        xv[n][1] = __uint_as_float(raw.v[n] & 0xffff0000u);
      } else {
        xv[n][0] = __uint_as_float(raw.v[2 * n]);
        xv[n][1] = __uint_as_float(raw.v[2 * n + 1]);
      }
    }
  } else {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int q = 0; q < 2; ++q)
        xv[n][q] = sizeof(S) == 2 ? __uint_as_float(raw.e[2 * n + q] << 16) : __uint_as_float(raw.e[2 * n + q]);
  }
}

// OP consecutive values of one window (dY row / out row): DW dwords when VEC, element accesses else
template <typename S, int OP>
struct RawRow {
  static constexpr int DW = OP * (int)sizeof(S) / 4;
  unsigned d[DW];     // VEC
  unsigned e[OP];     // !VEC: raw bits per element (unused elements zero)
};
template <typename S, int OP, bool VEC>
__device__ __forceinline__ void issue_row(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, int O,
                                          RawRow<S, OP>& r) {
  constexpr int DW = RawRow<S, OP>::DW;
  if constexpr (VEC) {
    if constexpr (DW == 1) {
      r.d[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0);
    } else if constexpr (DW == 2) {
      const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
      r.d[0] = t.x; r.d[1] = t.y;
    } else {
#pragma unroll
      for (int i = 0; i < DW / 4; ++i) {
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff + 16u * i, 0);
        r.d[4 * i] = t.x; r.d[4 * i + 1] = t.y; r.d[4 * i + 2] = t.z; r.d[4 * i + 3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int o = 0; o < OP; ++o) {
      r.e[o] = 0u;
      if (o < O) {
        if constexpr (sizeof(S) == 2)
          r.e[o] = (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs, voff, soff + 2u * o, 0);
        else
          r.e[o] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff + 4u * o, 0);
      }
    }
  }
}
template <typename S, int OP, bool VEC>
__device__ __forceinline__ void unpack_row(const RawRow<S, OP>& r, float (&v)[OP]) {
#pragma unroll
  for (int o = 0; o < OP; ++o) {
    if constexpr (!VEC) {
      v[o] = sizeof(S) == 2 ? __uint_as_float(r.e[o] << 16) : __uint_as_float(r.e[o]);
    } else if constexpr (sizeof(S) == 2) {
      v[o] = (o & 1) ? __uint_as_float(r.d[o >> 1] & 0xffff0000u) : __uint_as_float(r.d[o >> 1] << 16);
    } else {
      v[o] = __uint_as_float(r.d[o]);
    }
  }
}
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
// one value against a pair: a single v_pk_mul_f32 (the broadcast is an operand selector, not an instruction)
__device__ __forceinline__ f32x2 bmul2(float s, f32x2 v) { return f32x2{s, s} * v; }
// (measured per site on one box, 20-step graph: P0 on packed multiplies -0.6 us per step, P1 / Z -0.2, the forward's
//  P1 halves 0; the forward's epilogue on v_pk_fma_f32 +1.4 us - packed FMAs beside MFMAs cost more than they save)
// acc + s * v on a pair as two scalar fused multiply-adds (v_pk_fma_f32 here cost 1.4 us per step: 33.4 against 32.0)
__device__ __forceinline__ f32x2 bfma2(float s, f32x2 v, f32x2 acc) { return f32x2{__builtin_fmaf(s, v[0], acc[0]), __builtin_fmaf(s, v[1], acc[1])}; }
// 8 floats -> one MFMA operand fragment: exactly four v_cvt_pk_bf16_f32 (element-wise casts into a
// bf16x8 make the compiler convert singly and re-pack with shifts and ors)
__device__ __forceinline__ bf16x8 pack8(float f0, float f1, float f2, float f3, float f4, float f5, float f6,
                                        float f7) {
  int4v r;
  r[0] = (int)pack_bf16(f0, f1);
  r[1] = (int)pack_bf16(f2, f3);
  r[2] = (int)pack_bf16(f4, f5);
  r[3] = (int)pack_bf16(f6, f7);
  return __builtin_bit_cast(bf16x8, r);
}
template <typename S, int OP, bool VEC>
__device__ __forceinline__ void store_row(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, int O,
                                          const float (&v)[OP]) {
  constexpr int DW = RawRow<S, OP>::DW;
  if constexpr (VEC) {
    unsigned d[DW];
#pragma unroll
    for (int i = 0; i < DW; ++i)
      d[i] = sizeof(S) == 2 ? pack_bf16(v[2 * i], v[2 * i + 1]) : __float_as_uint(v[i * (OP / DW)]);
    if constexpr (DW == 1) {
      __builtin_amdgcn_raw_buffer_store_b32(d[0], rs, voff, soff, 0);
    } else if constexpr (DW == 2) {
      __builtin_amdgcn_raw_buffer_store_b64(u32x2{d[0], d[1]}, rs, voff, soff, 0);
    } else {
#pragma unroll
      for (int i = 0; i < DW / 4; ++i)
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]}, rs, voff,
                                               soff + 16u * i, 0);
    }
  } else {
#pragma unroll
    for (int o = 0; o < OP; ++o)
      if (o < O) {
        if constexpr (sizeof(S) == 2)
          __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(pack_bf16(v[o], 0.f) & 0xffffu), rs, voff,
                                                soff + 2u * o, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[o]), rs, voff, soff + 4u * o, 0);
      }
  }
}

// Which samples and which window positions a wave works on (see the header comment).
struct WaveJob {
  int b0, b1;          // samples [b0, b1)
  unsigned voff_x;     // byte offset of the lane's window inside a sample of x (x_bytes: no window)
  unsigned voff_o;     // byte offset of the lane's row inside a sample of out / dY (o_bytes: no window)
  int pos;
  bool valid;
};
// grouped = true (fused-head backward): a workgroup is (chunk block cb, position group pg) and its
// waves are the 8 sample chunks of cb at the SAME positions, so that their per-position sums can
// meet in LDS; consecutive workgroups walk pg first, keeping the samples of a chunk block on one XCD.
__device__ __forceinline__ WaveJob wave_job(const MfmaP& p, int waves_per_block, int esz, bool grouped = false) {
  // XCD-contiguous mapping: workgroups b, b+8, ... share an XCD (round-robin dispatch), so give each
  // XCD one contiguous eighth of the waves: the position groups of a sample chunk then meet in one L2.
  const int nb = gridDim.x;
  const int vb = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(vb * waves_per_block + (int)(threadIdx.x >> 6));
  int chunk = wave / p.npg, pg = wave - chunk * p.npg;
  if (grouped) {
    const int cb = vb / p.npg;
    pg = vb - cb * p.npg;
    chunk = __builtin_amdgcn_readfirstlane(cb * waves_per_block + (int)(threadIdx.x >> 6));
    if (cb >= p.ncb) chunk = p.nchunks;   // padding workgroups: no samples
  }
  WaveJob j;
  j.b0 = chunk < p.nchunks ? chunk * p.spc : 0;
  j.b1 = chunk < p.nchunks ? (j.b0 + p.spc < p.B ? j.b0 + p.spc : p.B) : 0;
  if (grouped && p.skew > 0) {
    // uneven split (plan_grouped): the block's waves_per_block * spc consecutive samples go to its first half of waves
    // - the older wave of every SIMD - in runs of spc + skew and to the second half in runs of spc - skew
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), half = waves_per_block / 2;
    const int n_old = p.spc + p.skew, n_young = p.spc - p.skew;
    const int s0 = (vb / p.npg) * waves_per_block * p.spc + (w < half ? w * n_old : half * n_old + (w - half) * n_young);
    const int s1 = s0 + (w < half ? n_old : n_young);
    const bool live = vb / p.npg < p.ncb && s0 < p.B;
    j.b0 = live ? s0 : 0;
    j.b1 = live ? (s1 < p.B ? s1 : p.B) : 0;
  }
  j.pos = pg * 64 + (int)(threadIdx.x & 63);
  j.valid = j.pos < p.P;
  const unsigned pu = j.valid ? (unsigned)j.pos : 0u;
  const unsigned ho = fdiv(pu, p.div_wo), wo = pu - ho * (unsigned)p.Wo;
  j.voff_x = j.valid ? ho * p.s2b + wo * p.s3b : p.x_bytes;
  j.voff_o = j.valid ? pu * (unsigned)(p.O * esz) : p.o_bytes;
  return j;
}

// The whole P0 row of this lane's window, as the two k-halves of every 16-wide k-step:
// X[s][j] = P0[w][a = 16 s + j], Y[s][j] = P0[w][a = 16 s + 8 + j]; a's MSB = factor 0.
template <int N0>
__device__ __forceinline__ void build_p0(const float (*xv)[2], bf16x8 (&X)[(1 << N0) / 16],
                                         bf16x8 (&Y)[(1 << N0) / 16]) {
  // (packed f32 multiplies - v_pk_mul_f32, one scalar broadcast against a pair - in the same order of factors as the
  //  scalar form: 24 instead of 54 multiplies for the 32 products, and every result pair is one v_cvt_pk_bf16_f32)
  constexpr int KS = (1 << N0) / 16;
  const f32x2 x1 = {xv[N0 - 1][0], xv[N0 - 1][1]}, x2 = {xv[N0 - 2][0], xv[N0 - 2][1]};
  const f32x2 m01 = bmul2(xv[N0 - 3][0], x2), m23 = bmul2(xv[N0 - 3][1], x2);
  const f32x2 lo[4] = {bmul2(m01[0], x1), bmul2(m01[1], x1), bmul2(m23[0], x1), bmul2(m23[1], x1)};   // a = .. 2 i, 2 i + 1
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    float hi = 1.f;
#pragma unroll
    for (int t = 0; t < N0 - 4; ++t) hi = t == 0 ? xv[N0 - 5][s & 1] : hi * xv[N0 - 5 - t][(s >> t) & 1];
    const f32x2 x4 = {xv[N0 - 4][0], xv[N0 - 4][1]};
    const f32x2 h = N0 > 4 ? bmul2(hi, x4) : x4;
    int4v rx, ry;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2 a = bmul2(h[0], lo[i]), b = bmul2(h[1], lo[i]);
      rx[i] = (int)pack_bf16(a[0], a[1]);
      ry[i] = (int)pack_bf16(b[0], b[1]);
    }
    X[s] = __builtin_bit_cast(bf16x8, rx);
    Y[s] = __builtin_bit_cast(bf16x8, ry);
  }
}

// ------------------------------------------------------------------------------------ forward
// Row code of accumulator register v of M-tile t (lane-half bit h excluded):
//   code = (t << 4) | ((v >> 2) << 2) | (v & 3);   o = code & (OP-1);   b = ((code >> LOGO) << 1) | h
template <typename S, int N0, int N1, int OP, bool XVEC, bool OVEC, int ROWS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OP <= 4 ? 4 : 2))) void eps_fwd_q2reg_k(const S* __restrict__ x,
                                                       const S* __restrict__ core,
                                                       S* __restrict__ out, double* __restrict__ stats, MfmaP p) {
  // stats (optional): {sum y, sum y^2} over every output value, ACCUMULATED in float64 (the statistic behind the
  // empirical-output-std initialisation, dctn/eps.py:163-181); with out == nullptr nothing is stored at all
  constexpr int N = N0 + N1, A = 1 << N0, BN = 1 << N1, KS = A / 16, MT = BN * OP / 32;
  constexpr int LOGO = ilog2(OP);
  static_assert(MT >= 1 && KS >= 1, "tile too small");
  // A-operand fragments of the core, staged through LDS in fragment order
  // cs[((t*KS + s)*64 + lane)*8 + j] = core[a = 16s + 8h + j][b][o], where lane = 32h + row and
  // row = (g << 3) | (h' << 2) | i, code = (t << 4) | (g << 2) | i = (b >> 1 << LOGO) | o, h' = b & 1
  constexpr int TOT = A * BN * OP, PER = TOT / 256;
  static_assert(TOT % 256 == 0, "core staging assumes a multiple of 256 elements");
  __shared__ __attribute__((aligned(16))) bf16_t cs[TOT];
  const int tid = threadIdx.x, lane = tid & 63;
  DCTN_STAMP(p, 0);
  // the first sample's window loads go out before the core is staged: both memory round trips overlap
  const WaveJob job = wave_job(p, 4, (int)sizeof(S));
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, p.x_bytes), rs_o = make_rsrc(out, p.o_bytes);
  RawWindow<S, N, XVEC, ROWS> raw;
  if (job.b0 < job.b1) issue_window<S, N, XVEC, ROWS>(rs_x, job.voff_x, (unsigned)job.b0 * p.s1b, p, raw);
  {
    S tmp[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {  // all loads in flight together: one memory round trip
      const int e = tid + 256 * i, o = e % OP, ab = e / OP;
      tmp[i] = core[(long long)ab * p.O + (o < p.O ? o : 0)];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = tid + 256 * i, o = e % OP, ab = e / OP, bb = ab % BN, aa = ab / BN;
      const int code = ((bb >> 1) << LOGO) | o;
      const int row = (((code >> 2) & 3) << 3) | ((bb & 1) << 2) | (code & 3);
      const int dst = ((((code >> 4) * KS + (aa >> 4)) * 64 + ((aa >> 3) & 1) * 32 + row) << 3) | (aa & 7);
      cs[dst] = o < p.O ? (bf16_t)to_f32(tmp[i]) : (bf16_t)0.f;
    }
  }
  __syncthreads();
  bf16x8 cf[MT][KS];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s)
      cf[t][s] = *reinterpret_cast<const bf16x8*>(&cs[((t * KS + s) * 64 + lane) * 8]);
  DCTN_STAMP(p, 1);

  float st1 = 0.f, st2 = 0.f;   // this lane's part of the statistics (a wave covers only a few samples)
  for (int b = job.b0; b < job.b1; ++b) {
    float xv[N][2];
    unpack_window<S, N, XVEC, ROWS>(raw, xv);
    {  // prefetch the next sample of this wave (the last iteration re-reads its own)
      const int bn = b + 1 < job.b1 ? b + 1 : b;
      issue_window<S, N, XVEC, ROWS>(rs_x, job.voff_x, (unsigned)bn * p.s1b, p, raw);
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this step's arithmetic
    }
    bf16x8 pf0[KS], pf1[KS];   // after the swaps: B operands of set 0 / set 1
    build_p0<N0>(xv, pf0, pf1);
#pragma unroll
    for (int s = 0; s < KS; ++s) swap_halves(pf0[s], pf1[s]);
    // P1 over the last n1 factors: b bit u <-> factor N-1-u; bit 0 (factor N-1) is the lane half of
    // the accumulator row.  m0 / m1: multipliers this lane applies in set 0 / set 1.
    float m0[BN / 2], m1[BN / 2];
    {
      float ph[BN / 2];   // P1 without its last factor, built by doubling
      ph[0] = xv[N - 2][0];
      ph[1] = xv[N - 2][1];
#pragma unroll
      for (int u = 2; u < N1; ++u)
#pragma unroll
        for (int bh = (1 << (u - 1)) - 1; bh >= 0; --bh) {
          const float lo = ph[bh];
          ph[bh | (1 << (u - 1))] = lo * xv[N - 1 - u][1];
          ph[bh] = lo * xv[N - 1 - u][0];
        }
#pragma unroll
      for (int bh = 0; bh < BN / 2; ++bh) {
        m0[bh] = ph[bh] * xv[N - 1][0];
        m1[bh] = ph[bh] * xv[N - 1][1];
        swap_halves(m0[bh], m1[bh]);
      }
    }
    // (scalar FMAs on purpose: packed f32 VALU issues slower than two scalar ones on gfx950 — see
    // MI355X_MICROARCH.md, 'price of one filler beside MFMAs' — the build also disables SLP packing)
    float res0[OP], res1[OP];
#pragma unroll
    for (int o = 0; o < OP; ++o) { res0[o] = 0.f; res1[o] = 0.f; }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int set = 0; set < 2; ++set) {
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf[t][s], set ? pf1[s] : pf0[s], acc, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int code = (t << 4) | ((v >> 2) << 2) | (v & 3);
          const float mm = set ? m1[code >> LOGO] : m0[code >> LOGO];
          float& dst = set ? res1[code & (OP - 1)] : res0[code & (OP - 1)];
          dst = __builtin_fmaf(acc[v], mm, dst);
        }
      }
    }
    // join the two row halves: lanes 0-31 end up with set 0 (their own windows), lanes 32-63 with set 1
    float res[OP];
#pragma unroll
    for (int o = 0; o < OP; ++o) {
      float a0 = res0[o], a1 = res1[o];
      swap_halves(a0, a1);
      res[o] = a0 + a1;
    }
    if (stats) {   // wave-uniform; the values as the output tensor holds them (rounded to the storage type)
#pragma unroll
      for (int o = 0; o < OP; ++o) {
        const float r = to_f32((S)res[o]);
        const float keep = (o < p.O && job.valid) ? r : 0.f;
        st1 += keep;
        st2 = __builtin_fmaf(keep, keep, st2);
      }
    }
    if (out) store_row<S, OP, OVEC>(rs_o, job.voff_o, (unsigned)b * p.o_s1b, p.O, res);  // no position: out of range
    if (b == job.b0) DCTN_STAMP(p, 2);
  }
  DCTN_STAMP(p, 3);
  if (stats) {
    double d1 = wave_reduce_sum((double)st1), d2 = wave_reduce_sum((double)st2);
    if (lane == 0) {
      atomicAdd(&stats[0], d1);
      atomicAdd(&stats[1], d2);
    }
  }
}

// --------------------------------------------------------------------- forward with the linear head fused
// EPSesPlusLinear's tail (dctn/eps_plus_linear.py:144-147): features = eps(core, x), logits = Linear(flatten(features)).
// As separate kernels the head costs a launch, a kernel boundary and a re-read of the features (14.6 of the 38 us of a
// BASELINE cfg2 step).  Here a workgroup is ALL position groups (one wave each) of a few samples, so a sample's logits
//   logits[b, c] = bias[c] + sum_(pos, o) W[c, pos, o] * features[b, pos, o]
// meet inside the workgroup.  Per wave the sum over its 64 positions x OP outputs is a small GEMM on the matrix core
// (v_mfma_f32_16x16x32_bf16: rows = classes, columns = the samples of a group, k = (position, output)), which also IS
// the cross-lane reduction: the lane stores the bf16 pairs it writes to memory into a per-wave LDS tile
// [sample][position][output] (one ds_write_b64), the B fragments come back as ds_read_b128 (k-contiguous), the A
// fragments - the wave's slice of the head weight, W[c, 64 pg .. 64 pg + 63, :] - are loaded once per wave straight
// from memory in fragment layout.  A first version did the products on the vector ALU (v_dot2c) and summed the lanes
// with a swap/DPP butterfly: 460 cycles per sample and wave, which ate the launch it saved; this costs ~60.
constexpr int HEAD_FWD_MAXPG = 12;   // waves per workgroup (launch bound 768 threads: 3-4 waves per SIMD)
constexpr int HEAD_FWD_HS = 4;       // samples per group (columns of the head GEMM in use; one LDS flush per group)

template <int N0, int N1, int OP, int ROWS>
__global__ __launch_bounds__(64 * HEAD_FWD_MAXPG) void eps_fwd_head_q2reg_k(const bf16_t* __restrict__ x,
                                                                           const bf16_t* __restrict__ core,
                                                                           const bf16_t* __restrict__ hw,
                                                                           const bf16_t* __restrict__ bias,
                                                                           bf16_t* __restrict__ out,
                                                                           bf16_t* __restrict__ logits, MfmaP p) {
  typedef bf16_t S;
  typedef __attribute__((ext_vector_type(4))) float f32x4v;
  constexpr int N = N0 + N1, A = 1 << N0, BN = 1 << N1, KS = A / 16, MT = BN * OP / 32;
  constexpr int LOGO = ilog2(OP);
  constexpr int TOT = A * BN * OP;
  constexpr int HK = 64 * OP / 32;              // k-steps of the head GEMM of one wave (k = (position, output))
  constexpr int SROW = 64 * OP + 8;             // shorts per sample row of the tile (+16 bytes: the samples' banks differ)
  static_assert(OP % 2 == 0 && (64 * OP) % 32 == 0, "outputs are handled as bf16 pairs, 32 k per matrix step");
  __shared__ __attribute__((aligned(16))) bf16_t cs[TOT];
  __shared__ __attribute__((aligned(16))) short ftile[HEAD_FWD_MAXPG][HEAD_FWD_HS * SROW];
  __shared__ float hsum[2][HEAD_FWD_HS][16][HEAD_FWD_MAXPG];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nwv = (int)(blockDim.x >> 6);
  DCTN_STAMP(p, 0);
  const int b0 = (int)blockIdx.x * p.spc, b1 = b0 + p.spc < p.B ? b0 + p.spc : p.B;
  const int pos = wv * 64 + lane;
  const bool valid = pos < p.P;
  const unsigned pu = valid ? (unsigned)pos : 0u;
  const unsigned ho = fdiv(pu, p.div_wo), wo = pu - ho * (unsigned)p.Wo;
  const unsigned voff_x = valid ? ho * p.s2b + wo * p.s3b : p.x_bytes;
  const unsigned voff_o = valid ? pu * (unsigned)(OP * 2) : p.o_bytes;
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, p.x_bytes), rs_o = make_rsrc(out, p.o_bytes);
  // Order of the prologue's loads (a wave's loads return in order, and the workgroup's 11 waves share one 64 B/clk
  // vector-memory path): the core's first batch and the FIRST sample's rows go out before the barrier that publishes the
  // core; the other samples of the group and the head weight (17 sixteen-byte loads per lane, 190 KB per CU) only after
  // it - issued in front, every wave sat in their queue before it could reach the barrier.
  S core_first[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ec = tid + i * (int)blockDim.x, e = ec < TOT ? ec : TOT - 1, o = e % OP, ab = e / OP;   // clamped: no branch
    core_first[i] = core[(long long)ab * p.O + (o < p.O ? o : 0)];                                    // around the load
  }
  __builtin_amdgcn_sched_barrier(0);
  // a group's samples are all in flight before the first is used (a sample's rows are fresh lines: ~1.5 us from
  // HBM / MALL, two to three steps of arithmetic; a one-deep prefetch left the SIMDs waiting), and a slot is re-issued
  // for the next group as soon as it has been unpacked
  RawWindow<S, N, true, ROWS> raw[HEAD_FWD_HS];
  auto first_of_group = [&](int u) { return b0 + u < b1 ? b0 + u : (b1 > b0 ? b1 - 1 : b0); };
  issue_window<S, N, true, ROWS>(rs_x, voff_x, (unsigned)first_of_group(0) * p.s1b, p, raw[0]);   // (a workgroup without
                                                                                                 // samples reads zeros past the end)
  // core -> LDS in fragment order (as eps_fwd_q2reg_k), by however many threads the workgroup has: batches of 4
  // elements per thread, the 4 loads of a batch in flight together
  auto core_commit = [&](int e0, const S (&tmp)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = e0 + tid + i * (int)blockDim.x, o = e % OP, ab = e / OP, bb = ab % BN, aa = ab / BN;
      const int code = ((bb >> 1) << LOGO) | o;
      const int row = (((code >> 2) & 3) << 3) | ((bb & 1) << 2) | (code & 3);
      const int dst = ((((code >> 4) * KS + (aa >> 4)) * 64 + ((aa >> 3) & 1) * 32 + row) << 3) | (aa & 7);
      if (e < TOT) cs[dst] = o < p.O ? tmp[i] : (bf16_t)0.f;
    }
  };
  core_commit(0, core_first);
  for (int e0 = 4 * (int)blockDim.x; e0 < TOT; e0 += 4 * (int)blockDim.x) {   // small workgroups: the rest of the core
    S tmp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = e0 + tid + i * (int)blockDim.x, o = e % OP, ab = e / OP;
      tmp[i] = e < TOT ? core[(long long)ab * p.O + (o < p.O ? o : 0)] : (S)0.f;
    }
    core_commit(e0, tmp);
  }
  __syncthreads();
  bf16x8 cf[MT][KS];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s)
      cf[t][s] = *reinterpret_cast<const bf16x8*>(&cs[((t * KS + s) * 64 + lane) * 8]);
#pragma unroll
  for (int u = 1; u < HEAD_FWD_HS; ++u)
    issue_window<S, N, true, ROWS>(rs_x, voff_x, (unsigned)first_of_group(u) * p.s1b, p, raw[u]);
  // A fragments of the head GEMM: lane (c = lane % 16, g = lane / 16) holds W[c, k = 32 ks + 8 g .. + 7] of this wave's
  // positions; rows c >= Cout and bytes past the end of the weight read zeros (range check).  A position past P
  // inside a row meets a zero feature (lanes without a position produce zeros), so it needs no mask.
  bf16x8 wf[HK];
  {
    const __amdgpu_buffer_rsrc_t rs_hw = make_rsrc(hw, p.hw_bytes);
    const int c = lane & 15, g = lane >> 4;
    const unsigned base = c < p.Cout ? (unsigned)c * p.hw_rowb + (unsigned)(wv * 64 * OP + 8 * g) * 2u : p.hw_bytes;
#pragma unroll
    for (int ks = 0; ks < HK; ++ks)
      wf[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_hw, base, (unsigned)(ks * 64), 0));
  }
  __builtin_amdgcn_sched_barrier(0);

  short* tile = &ftile[wv][0];
  // B fragment reads: lane (column = sample lane % 16, clamped to the group; k group lane / 16)
  const int bcol = (lane & 15) < HEAD_FWD_HS ? (lane & 15) : HEAD_FWD_HS - 1;
  const short* brd = tile + bcol * SROW + 8 * (lane >> 4);
  DCTN_STAMP(p, 1);
  for (int g0 = b0, grp = 0; g0 < b1; g0 += HEAD_FWD_HS, ++grp) {
    const int g1 = g0 + HEAD_FWD_HS < b1 ? g0 + HEAD_FWD_HS : b1;
#pragma unroll
    for (int u = 0; u < HEAD_FWD_HS; ++u) {
      const int b = g0 + u;
      if (b >= g1) break;   // wave-uniform
      float xv[N][2];
      unpack_window<S, N, true, ROWS>(raw[u], xv);
      {  // the same slot of the next group (past the end: a harmless re-read of the last sample)
        const int bn = b + HEAD_FWD_HS < b1 ? b + HEAD_FWD_HS : b1 - 1;
        issue_window<S, N, true, ROWS>(rs_x, voff_x, (unsigned)bn * p.s1b, p, raw[u]);
        __builtin_amdgcn_sched_barrier(0);
      }
      bf16x8 pf0[KS], pf1[KS];
      build_p0<N0>(xv, pf0, pf1);
#pragma unroll
      for (int s = 0; s < KS; ++s) swap_halves(pf0[s], pf1[s]);
      float m0[BN / 2], m1[BN / 2];
      {
        float ph[BN / 2];
        ph[0] = xv[N - 2][0];
        ph[1] = xv[N - 2][1];
#pragma unroll
        for (int u = 2; u < N1; ++u)
#pragma unroll
          for (int bh = (1 << (u - 1)) - 1; bh >= 0; --bh) {
            const f32x2 pr = bmul2(ph[bh], f32x2{xv[N - 1 - u][0], xv[N - 1 - u][1]});
            ph[bh] = pr[0];
            ph[bh | (1 << (u - 1))] = pr[1];
          }
#pragma unroll
        for (int bh = 0; bh < BN / 2; ++bh) {
          const f32x2 mm = bmul2(ph[bh], f32x2{xv[N - 1][0], xv[N - 1][1]});
          m0[bh] = mm[0];
          m1[bh] = mm[1];
          swap_halves(m0[bh], m1[bh]);
        }
      }
      float res0[OP], res1[OP];
#pragma unroll
      for (int o = 0; o < OP; ++o) { res0[o] = 0.f; res1[o] = 0.f; }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int set = 0; set < 2; ++set) {
          f32x16 acc;
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
          for (int s = 0; s < KS; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf[t][s], set ? pf1[s] : pf0[s], acc, 0, 0, 0);
          // registers v, v + 1 (v even) are the outputs o, o + 1 of one b: a packed fused multiply-add per pair
#pragma unroll
          for (int v = 0; v < 16; v += 2) {
            const int code = (t << 4) | ((v >> 2) << 2) | (v & 3);
            const float mm = set ? m1[code >> LOGO] : m0[code >> LOGO];
            float* dst = set ? res1 : res0;
            const int o = code & (OP - 1);
            const f32x2 r = bfma2(mm, f32x2{acc[v], acc[v + 1]}, f32x2{dst[o], dst[o + 1]});
            dst[o] = r[0];
            dst[o + 1] = r[1];
          }
        }
      }
      // the lane's OP outputs as the bf16 pairs that go to memory (lanes without a position: zeros) ...
      unsigned pk[OP / 2];
#pragma unroll
      for (int i = 0; i < OP / 2; ++i) {
        float a0 = res0[2 * i], a1 = res1[2 * i], c0 = res0[2 * i + 1], c1 = res1[2 * i + 1];
        swap_halves(a0, a1);
        swap_halves(c0, c1);
        pk[i] = pack_bf16(a0 + a1, c0 + c1);
      }
      if constexpr (OP == 2) {
        __builtin_amdgcn_raw_buffer_store_b32(pk[0], rs_o, voff_o, (unsigned)b * p.o_s1b, 0);
        *reinterpret_cast<unsigned*>(tile + (b - g0) * SROW + lane * OP) = pk[0];
      } else if constexpr (OP == 4) {
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{pk[0], pk[1]}, rs_o, voff_o, (unsigned)b * p.o_s1b, 0);
        *reinterpret_cast<u32x2*>(tile + (b - g0) * SROW + lane * OP) = u32x2{pk[0], pk[1]};
      } else {
#pragma unroll
        for (int i = 0; i < OP / 8; ++i) {
          const u32x4 q = u32x4{pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]};
          __builtin_amdgcn_raw_buffer_store_b128(q, rs_o, voff_o, (unsigned)b * p.o_s1b + 16u * i, 0);
          *reinterpret_cast<u32x4*>(tile + (b - g0) * SROW + lane * OP + 8 * i) = q;
        }
      }
      if (b == b0) DCTN_STAMP(p, 2);
    }
    // ... and the group's head GEMM of this wave: D[c, s] = sum_k W[c, k] * features[s, k]
    wave_lds_sync();
    f32x4v hd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HK; ++ks) {
      const bf16x8 fb = *reinterpret_cast<const bf16x8*>(brd + 32 * ks);
      hd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks], fb, hd, 0, 0, 0);
    }
    wave_lds_sync();   // the tile is free for the next group's rows
    {  // D: column = lane % 16 (sample of the group), rows 4 (lane / 16) + v (classes)
      const int sl = lane & 15, cb = 4 * (lane >> 4);
      if (sl < g1 - g0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) hsum[grp & 1][sl][cb + v][wv] = hd[v];
      }
    }
    DCTN_STAMP(p, 3);
    __syncthreads();   // one barrier per group: the buffers alternate, a buffer is rewritten two groups later
    for (int e = tid; e < (g1 - g0) * p.Cout; e += (int)blockDim.x) {
      const int sl = e / p.Cout, c = e - sl * p.Cout;
      float t = (float)bias[c];
      for (int w = 0; w < nwv; ++w) t += hsum[grp & 1][sl][c][w];
      logits[(long long)(g0 + sl) * p.Cout + c] = (bf16_t)t;
    }
  }
  DCTN_STAMP(p, 4);
}

// ---- the same forward, second structure (round 5): steps PULLED from a counter, head as a tail phase.
// The structure above ties a wave to one position group (its head-weight fragments live in registers), so a workgroup is
// 11 waves on 4 SIMDs (3 + 3 + 3 + 2) and, the kernel being bound by vector-instruction issue, the SIMDs with three
// waves set its length: wave 0 of a workgroup was done at 5.1 us, the kernel at 9.4.  Here a workgroup is 16 waves
// (4 per SIMD, <= 128 registers) that draw (sample, position group) steps from an LDS counter, two steps ahead of the
// one they compute - whichever wave is done takes the next step, the SIMDs end together.  Every step leaves its
// bf16 features in an LDS tile [sample][feature]; when the group's steps are done the workgroup forms
// logits[s][c] = bias[c] + sum_k W[c][k] * feat[s][k] on v_mfma_f32_16x16x32_bf16 (rows = classes, columns = the 4
// samples, k-steps of 32 features dealt over the waves; the weight fragments - 16-byte loads straight from memory in
// operand order - are requested BEFORE the barrier that closes the group, they depend on nothing), the waves' partial
// tiles meet in LDS and are summed in wave order.  Same arithmetic as above: bf16 products, float32 sums.
// BLK4 (DCTN_OPT_HEAD_FEATURES_BLOCKED4): the steps leave their features in the tile only; once the group is complete
// the workgroup writes it as ONE contiguous [F][4] block of `out` ("blocked4": out[((g0 / 4) * F + f) * 4 + i] =
// feature f of sample g0 + i, the samples past the batch as zeros; the launcher aligns the groups to 4 samples), the
// layout whose k-contiguous fragments the backward's dW product loads directly (head_dw_gemm_role).
constexpr int HEADT_WAVES = 16;
constexpr int HEADT_GS = 4;          // samples per group = columns of the head product in use
constexpr int HEADT_MAXKS = 6;       // 32-feature steps per wave of the head product: at most 16 * 6 * 32 = 3072 features
constexpr int headt_pitch(int F) { return (F + 31) / 32 * 32 + 8; }   // shorts per sample row of the tile (+16 bytes: the samples' banks differ)

template <int N0, int N1, int OP, int ROWS, bool BLK4>
__global__ __launch_bounds__(64 * HEADT_WAVES) void eps_fwd_head_q2reg_t_k(const bf16_t* __restrict__ x,
                                                                           const bf16_t* __restrict__ core,
                                                                           const bf16_t* __restrict__ hw,
                                                                           const bf16_t* __restrict__ bias,
                                                                           bf16_t* __restrict__ out,
                                                                           bf16_t* __restrict__ logits, MfmaP p_in) {
  typedef bf16_t S;
  typedef __attribute__((ext_vector_type(4))) float f32x4v;
  constexpr int N = N0 + N1, A = 1 << N0, BN = 1 << N1, KS = A / 16, MT = BN * OP / 32;
  constexpr int LOGO = ilog2(OP);
  constexpr int TOT = A * BN * OP;
  static_assert(OP % 2 == 0 && TOT % 4 == 0, "outputs are handled as bf16 pairs");
#if DCTN_FWD_ARGS_ONCE
  // Every argument the kernel uses, read in the scalar round at entry: the empty statement needs them all in registers
  // here, so no load of the argument block is left behind a barrier, on the way to the first window (they came in four
  // dependent rounds, the last one behind the barrier that publishes the core)
  MfmaP p = p_in;
  asm volatile("" ::"s"(x), "s"(core), "s"(hw), "s"(bias), "s"(out), "s"(logits), "s"(p.B), "s"(p.O), "s"(p.Wo), "s"(p.P),
               "s"(p.npg), "s"(p.spc), "s"(p.rowoffb[0]), "s"(p.rowoffb[1]), "s"(p.rowoffb[2]), "s"(p.rowoffb[ROWS - 1]),
               "s"(p.s1b), "s"(p.s2b), "s"(p.s3b), "s"(p.x_bytes), "s"(p.o_bytes), "s"(p.o_s1b), "s"(p.div_wo.M),
               "s"(p.div_wo.s1), "s"(p.div_wo.s2), "s"(p.Cout), "s"(p.hw_rowb), "s"(p.hw_bytes), "s"(p.npg_rcp));
#else
  const MfmaP& p = p_in;
#endif
  __shared__ __attribute__((aligned(16))) bf16_t cs[TOT];
  __shared__ float hsum[HEADT_WAVES][HEADT_GS][16];
  __shared__ unsigned step_ctr;
#if DCTN_FWD_POS_TABLE
  // per (position group, lane): {byte offset of the window in a sample of x, byte offset of the position's features in a
  // sample's row of the tile and of `out`}; lanes without a position and the whole row npg (the row of a dead ticket):
  // {past x, POS_NONE}
  static_assert((HEAD_FWD_MAXPG + 1) * 64 <= 64 * HEADT_WAVES, "one table entry per thread");
  __shared__ u32x2 pos_tab[(HEAD_FWD_MAXPG + 1) * 64];
#endif
  constexpr unsigned POS_NONE = 0x80000000u;   // as an offset into `out` it is past every extent (o_bytes < 2^31)
  extern __shared__ __attribute__((aligned(16))) short ftile[];   // [HEADT_GS][LP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b0 = (int)blockIdx.x * p.spc, b1 = b0 + p.spc < p.B ? b0 + p.spc : p.B;
  const int F = p.P * OP, LP = headt_pitch(F);
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, p.x_bytes), rs_o = make_rsrc(out, p.o_bytes);
  __shared__ float bias_s[16];
  DCTN_STAMP(p, 0);
  // The bias of the final sums is staged in LDS by wave 0 and published by the barrier below, so no load follows a
  // group's last barrier.  Its load goes out BEHIND the core's first loads and in front of their LDS stores: a wave's
  // loads return in order, so it neither holds the core back nor waits for a round trip of its own.
  float bias_v = 0.f;
  // offsets of window position `pos`: into a sample of x (past x without a position), and into a sample's feature row
  auto lane_at = [&](int pos, unsigned& voff_x, unsigned& toff) {
    const bool valid = pos < p.P;
    const unsigned pu = (unsigned)(valid ? pos : p.P - 1);
    const unsigned ho = fdiv(pu, p.div_wo), wo = pu - ho * (unsigned)p.Wo;
    voff_x = valid ? ho * p.s2b + wo * p.s3b : p.x_bytes;
    toff = valid ? pu * (unsigned)(OP * 2) : POS_NONE;
  };
  // a wave's first step of a group is the static ticket wv: its sample and its lane's offsets, without the table (the
  // first group's goes out before the table is published)
  auto first_ticket = [&](int nsteps, int& s, unsigned& voff_x, unsigned& toff) {
    const int sq = (int)(((unsigned)wv * p.npg_rcp) >> 16), pg = wv - sq * p.npg;
    const bool live = wv < nsteps;
    s = live ? sq : 0;
    lane_at(live ? pg * 64 + lane : p.P, voff_x, toff);
  };
  const int ng0 = b0 + HEADT_GS < b1 ? HEADT_GS : b1 - b0, nsteps0 = ng0 * p.npg;
  int s;
  unsigned voff_x, toff;
  RawWindow<S, N, true, ROWS> raw;
#if DCTN_FWD_EARLY_WINDOW
  if (tid == 0) step_ctr = 2 * HEADT_WAVES;   // the first group's: published by the barrier below
#endif
  // core -> LDS in fragment order (as eps_fwd_q2reg_k): 4 elements per thread and batch, the loads of a batch in flight together
  for (int e0 = 0; e0 < TOT; e0 += 4 * 64 * HEADT_WAVES) {
    S tmp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ec = e0 + tid + i * 64 * HEADT_WAVES, e = ec < TOT ? ec : TOT - 1, o = e % OP, ab = e / OP;
      tmp[i] = core[(long long)ab * p.O + (o < p.O ? o : 0)];
    }
    if (e0 == 0 && wv == 0) bias_v = (float)bias[(lane & 15) < p.Cout ? (lane & 15) : 0];
#if DCTN_FWD_EARLY_WINDOW
    // the wave's first window of the first group (a static ticket) goes out behind the core's loads as well
    if (e0 == 0) {
      first_ticket(nsteps0, s, voff_x, toff);
      issue_window<S, N, true, ROWS>(rs_x, voff_x, (unsigned)(b0 + s) * p.s1b, p, raw);
    }
#endif
#if DCTN_FWD_POS_TABLE
    if (e0 == 0 && tid < (p.npg + 1) * 64) {   // the table: arithmetic while the loads above are in flight
      unsigned vx, t;
      lane_at(tid, vx, t);
      pos_tab[tid] = u32x2{vx, t};
    }
#endif
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = e0 + tid + i * 64 * HEADT_WAVES, o = e % OP, ab = e / OP, bb = ab % BN, aa = ab / BN;
      const int code = ((bb >> 1) << LOGO) | o;
      const int row = (((code >> 2) & 3) << 3) | ((bb & 1) << 2) | (code & 3);
      const int dst = ((((code >> 4) * KS + (aa >> 4)) * 64 + ((aa >> 3) & 1) * 32 + row) << 3) | (aa & 7);
      if (e < TOT) cs[dst] = o < p.O ? tmp[i] : (bf16_t)0.f;
    }
  }
  if (wv == 0) bias_s[lane & 15] = bias_v;
  // the tile's features past F meet zero weights: they must be finite
  for (int e = tid; e < HEADT_GS * (LP - F); e += 64 * HEADT_WAVES) ftile[(e / (LP - F)) * LP + F + e % (LP - F)] = 0;
  __syncthreads();
  bf16x8 cf[MT][KS];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s)
      cf[t][s] = *reinterpret_cast<const bf16x8*>(&cs[((t * KS + s) * 64 + lane) * 8]);
  DCTN_STAMP(p, 1);

  auto draw = [&]() {
    unsigned v = 0;
    if (lane == 0) v = __hip_atomic_fetch_add(&step_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return (int)__builtin_amdgcn_readfirstlane(v);
  };

  for (int g0 = b0; g0 < b1; g0 += HEADT_GS) {
    const int ng = g0 + HEADT_GS < b1 ? HEADT_GS : b1 - g0;
    const int nsteps = ng * p.npg;
    // ticket -> sample of the group and the lane's offsets; a dead ticket (past the group's steps): sample 0, no position
    auto locate = [&](int ticket, int& s, unsigned& voff_x, unsigned& toff) {
      const bool live = ticket < nsteps;
#if DCTN_FWD_POS_TABLE
      const int sq = (int)(((unsigned)ticket * p.npg_rcp) >> 16), pg = ticket - sq * p.npg;
      s = live ? sq : 0;
      const u32x2 e = pos_tab[(live ? pg : p.npg) * 64 + lane];
      voff_x = e.x;
      toff = e.y;
#else
      const int sq = ticket / p.npg, pg = ticket - sq * p.npg;
      s = live ? sq : 0;
      lane_at(live ? pg * 64 + lane : p.P, voff_x, toff);
#endif
    };
    // (built and dropped in round 11: the first window sent in FRONT of the core staging, and at the end of the group
    //  before for later groups: the core fragments came 0.17 us later, the step was 0.16 us slower - NOTEBOOK, "critical
    //  path of cfg2".  DCTN_FWD_EARLY_WINDOW sends the first group's BEHIND the core's loads, in the prologue above.)
    if (!DCTN_FWD_EARLY_WINDOW || g0 != b0) {
      if (tid == 0) step_ctr = 2 * HEADT_WAVES;   // steps 0 .. 31 are dealt: wave w starts with w and w + 16
      __syncthreads();
      first_ticket(nsteps, s, voff_x, toff);
      issue_window<S, N, true, ROWS>(rs_x, voff_x, (unsigned)(g0 + s) * p.s1b, p, raw);
    }
    int cur = wv, nxt = wv + HEADT_WAVES;
#ifdef DCTN_STAMPS
    bool first_step = true;
#endif
    while (cur < nsteps) {
      float xv[N][2];
      unpack_window<S, N, true, ROWS>(raw, xv);
      const unsigned vo = toff, so = (unsigned)(g0 + s) * p.o_s1b;
      const bool tvalid = toff != POS_NONE;
      short* trow = reinterpret_cast<short*>(reinterpret_cast<char*>(ftile + s * LP) + toff);   // used under tvalid only
      {  // the wave's next step: its window goes out before this step's arithmetic (past the last step every lane is out
         // of range: zeros, no control flow around the loads); and the ticket of the step after it
        cur = nxt;
        locate(cur, s, voff_x, toff);
        issue_window<S, N, true, ROWS>(rs_x, voff_x, (unsigned)(g0 + s) * p.s1b, p, raw);
        nxt = draw();
        __builtin_amdgcn_sched_barrier(0);
      }
      bf16x8 pf0[KS], pf1[KS];
      build_p0<N0>(xv, pf0, pf1);
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) swap_halves(pf0[s2], pf1[s2]);
      float m0[BN / 2], m1[BN / 2];
      {
        float ph[BN / 2];
        ph[0] = xv[N - 2][0];
        ph[1] = xv[N - 2][1];
#pragma unroll
        for (int u = 2; u < N1; ++u)
#pragma unroll
          for (int bh = (1 << (u - 1)) - 1; bh >= 0; --bh) {
            const f32x2 pr = bmul2(ph[bh], f32x2{xv[N - 1 - u][0], xv[N - 1 - u][1]});
            ph[bh] = pr[0];
            ph[bh | (1 << (u - 1))] = pr[1];
          }
#pragma unroll
        for (int bh = 0; bh < BN / 2; ++bh) {
          const f32x2 mm = bmul2(ph[bh], f32x2{xv[N - 1][0], xv[N - 1][1]});
          m0[bh] = mm[0];
          m1[bh] = mm[1];
          swap_halves(m0[bh], m1[bh]);
        }
      }
      float res0[OP], res1[OP];
#pragma unroll
      for (int o = 0; o < OP; ++o) { res0[o] = 0.f; res1[o] = 0.f; }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int set = 0; set < 2; ++set) {
          f32x16 acc;
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
          for (int s2 = 0; s2 < KS; ++s2)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf[t][s2], set ? pf1[s2] : pf0[s2], acc, 0, 0, 0);
#pragma unroll
          for (int v = 0; v < 16; v += 2) {
            const int code = (t << 4) | ((v >> 2) << 2) | (v & 3);
            const float mm = set ? m1[code >> LOGO] : m0[code >> LOGO];
            float* dst = set ? res1 : res0;
            const int o = code & (OP - 1);
            const f32x2 r = __builtin_elementwise_fma(f32x2{mm, mm}, f32x2{acc[v], acc[v + 1]}, f32x2{dst[o], dst[o + 1]});
            dst[o] = r[0];
            dst[o + 1] = r[1];
          }
        }
      }
      unsigned pk[OP / 2];
#pragma unroll
      for (int i = 0; i < OP / 2; ++i) {
        float a0 = res0[2 * i], a1 = res1[2 * i], c0 = res0[2 * i + 1], c1 = res1[2 * i + 1];
        swap_halves(a0, a1);
        swap_halves(c0, c1);
        pk[i] = pack_bf16(a0 + a1, c0 + c1);
      }
      if constexpr (OP == 2) {
        if constexpr (!BLK4) __builtin_amdgcn_raw_buffer_store_b32(pk[0], rs_o, vo, so, 0);
        if (tvalid) *reinterpret_cast<unsigned*>(trow) = pk[0];
      } else if constexpr (OP == 4) {
        if constexpr (!BLK4) __builtin_amdgcn_raw_buffer_store_b64(u32x2{pk[0], pk[1]}, rs_o, vo, so, 0);
        if (tvalid) *reinterpret_cast<u32x2*>(trow) = u32x2{pk[0], pk[1]};
      } else {
#pragma unroll
        for (int i = 0; i < OP / 8; ++i) {
          const u32x4 q = u32x4{pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]};
          if constexpr (!BLK4) __builtin_amdgcn_raw_buffer_store_b128(q, rs_o, vo, so + 16u * i, 0);
          if (tvalid) *reinterpret_cast<u32x4*>(trow + 8 * i) = q;
        }
      }
#ifdef DCTN_STAMPS
      if (first_step) DCTN_STAMP(p, 2);
      first_step = false;
#endif
    }
    DCTN_STAMP(p, 3);
    DCTN_STAMP_T(p, 4, 64 * (HEADT_WAVES - 1));
    // ---- the group's head product: weight fragments first (they depend on nothing of the group)
    const int nks = (F + 31) / 32;
    const int c = lane & 15, kg = lane >> 4;
    const __amdgpu_buffer_rsrc_t rs_hw = make_rsrc(hw, p.hw_bytes);
    u32x4 wf[HEADT_MAXKS];
#pragma unroll
    for (int i = 0; i < HEADT_MAXKS; ++i) {
      const int ks = wv + HEADT_WAVES * i, k = 32 * ks + 8 * kg;
      const unsigned vo2 = (ks < nks && c < p.Cout && k + 7 < F) ? (unsigned)c * p.hw_rowb + (unsigned)k * 2u : p.hw_bytes;
      wf[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_hw, vo2, 0, 0);
    }
    __syncthreads();   // every wave's feature rows of the group are in the tile
    DCTN_STAMP(p, 5);
    // (in front of the head product: the stores are on their way while the logits are formed; behind the partial tiles
    //  they were the last thing before the group's second barrier: +0.1 us per step)
    if constexpr (BLK4) {   // the group's [F][4] block: thread t stores features 2 t, 2 t + 1 of the 4 samples, 16 bytes
      static_assert(HEADT_GS == 4, "a group is one block of the blocked4 layout");
      const unsigned sob = (unsigned)(g0 >> 2) * (unsigned)F * 8u;   // g0 is a multiple of 4 (fwd_head_launch_t)
      for (int f = 2 * tid; f < F; f += 2 * 64 * HEADT_WAVES) {
        unsigned r[HEADT_GS];   // r[i] = features f, f + 1 of sample i (a sample past the batch: zeros)
#pragma unroll
        for (int i = 0; i < HEADT_GS; ++i) r[i] = i < ng ? *reinterpret_cast<const unsigned*>(ftile + i * LP + f) : 0u;
        const u32x4 q = u32x4{__builtin_amdgcn_perm(r[1], r[0], 0x05040100u), __builtin_amdgcn_perm(r[3], r[2], 0x05040100u),
                              __builtin_amdgcn_perm(r[1], r[0], 0x07060302u), __builtin_amdgcn_perm(r[3], r[2], 0x07060302u)};
        __builtin_amdgcn_raw_buffer_store_b128(q, rs_o, (unsigned)f * 8u, sob, DCTN_WT_FEATURES);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4v hd = {0.f, 0.f, 0.f, 0.f};
    const short* brd = ftile + (c < HEADT_GS ? c : HEADT_GS - 1) * LP + 8 * kg;
#pragma unroll
    for (int i = 0; i < HEADT_MAXKS; ++i) {
      const int ks = wv + HEADT_WAVES * i;
      if (ks < nks) {   // wave-uniform
        const bf16x8 fb = *reinterpret_cast<const bf16x8*>(brd + 32 * ks);
        hd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[i]), fb, hd, 0, 0, 0);
      }
    }
    // D: column = lane % 16 (sample of the group), rows 4 (lane / 16) + v (classes)
    if (c < HEADT_GS) {
#pragma unroll
      for (int v = 0; v < 4; ++v) hsum[wv][c][4 * kg + v] = hd[v];
    }
    __syncthreads();
    if (tid < HEADT_GS * 16) {
      const int sl = tid >> 4, cc = tid & 15;
      if (sl < ng && cc < p.Cout) {
        float t = bias_s[cc];
#pragma unroll
        for (int w = 0; w < HEADT_WAVES; ++w) t += hsum[w][sl][cc];
        logits[(long long)(g0 + sl) * p.Cout + cc] = (bf16_t)t;
      }
    }
    // (the next group's steps write the tile only behind the barrier at its start; its partial tiles behind its own
    //  first barrier after that: the sums just read are safe)
  }
  DCTN_STAMP(p, 6);
}

// ------------------------------------------------------------------------------ backward: dCore
// feature index m of Z: code = m = (mt << 5) | (s << 4) | (h << 3) | j;  o = m & (OP-1), b = m >> LOGO
constexpr int BWD_WAVES = 8;  // waves per workgroup of the dCore kernel (one LDS reduction per block)
// dynamic LDS of the dCore kernel's LDST path: per wave one P0 tile and MT Z tiles of [64 windows][32 features] bf16
constexpr size_t dcore_dyn_lds_bytes(int mt) { return (size_t)BWD_WAVES * (1 + mt) * 64 * 32 * sizeof(short); }

// HEADC > 0: fused classifier-head backward.  dY is not read; instead `dY` points at dLogits
// (B, Cout) and `hw` at the head weight (Cout, P*O), both bf16, and the wave forms
// dY[w, o] = sum_c dLogits[b, c] * hw[c, pos*O + o] itself: the lane's weight slice is loaded once
// (HEADC = Cout padded to the instantiated bound), dLogits of the sample is wave-uniform.  The same
// loop accumulates the head-weight gradient of the lane's position,
// dW[c, pos*O + o] += dLogits[b, c] * feat[b, pos, o]  (`feat` = the layer's forward output), reduced
// over the workgroup's 8 sample chunks in LDS and written as one partial tile per chunk block to
// `dwpart` [ncb][Cout][P*O]; eps_head_reduce_k sums the tiles (and dLogits into dBias).
// Exception (round 4): the HEADMM shapes (cfg2) leave dW to eps_head_reduce_k altogether - dW = dLogits^T x feat
// is a plain (Cout x B) x (B x P*O) product that needs nothing of this kernel; formed here it cost 4 of the 12 matrix
// instructions of a group, 64 accumulator registers, the loads of `feat`, a 1.7 us LDS epilogue and 2.5 MB of partial
// tiles written and read back (the "1.6x traffic" of rounds 2-3).
// DWROLE (0 or 4; the HEADMM shapes with blocked4 features): the workgroup has DWROLE more waves, which form dW on the
// wave slots the dCore waves leave free (162 VGPRs: a third wave per SIMD fits) - head_dw_role_waves, below the
// finishing kernel's gemm role whose arithmetic it shares.  Waves 0 .. BWD_WAVES - 1 are what they are without it.
__device__ __forceinline__ void head_dw_role_waves(const bf16_t* __restrict__ feat, const bf16_t* __restrict__ dL,
                                                   bf16_t* __restrict__ dW, int B, int Cout, long long F, int n_dw,
                                                   int rw, float* __restrict__ lds, const MfmaP& p);
template <typename S, int N0, int N1, int OP, bool XVEC, bool OVEC, int ROWS, int HEADC, int DWROLE = 0>
__global__ __launch_bounds__(64 * (BWD_WAVES + DWROLE)) void eps_bwd_dcore_q2reg_k(const S* __restrict__ x,
                                                             const S* __restrict__ dY,
                                                             const S* __restrict__ hw,
                                                             const S* __restrict__ feat,
                                                             float* __restrict__ partial,
                                                             float* __restrict__ dwpart, MfmaP p,
                                                             S* __restrict__ dW, int n_dw) {
  constexpr int N = N0 + N1, A = 1 << N0, BN = 1 << N1, KS = A / 16, MT = BN * OP / 32;
  constexpr int AT = A >= 32 ? A / 32 : 1;
  constexpr int LOGO = ilog2(OP);
  // LDST: windows reach the MFMA k index through LDS with the hardware transpose read instead of
  // through identity MFMAs (3 tiles of [64 windows][32 features] per wave; the cfg2 shape).  It
  // removes, per 64 windows, 12 of the 20 MFMAs, the 48 bf16 conversions behind them and all 24
  // lane swaps from a kernel that is bound by VALU + MFMA issue.
  constexpr bool LDST = A == 32 && MT <= 2;
  // (Round 4, built and dropped: Z through identity products on the matrix core and only P0 through LDS - 12 instead
  //  of 36 LDS instructions per step, 8 more matrix instructions, 48 more vector ones: 11.4 against 11.2 us.)
  __shared__ float red[BWD_WAVES][32 * 32];
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5, wv = tid >> 6;
  DCTN_STAMP(p, 0);
  if constexpr (DWROLE > 0) {
    static_assert(HEADC > 0 && HEADC <= 16 && LDST && OVEC && XVEC && sizeof(S) == 2 && OP == 4, "the dW role rides the HEADMM path");
    const int rw = __builtin_amdgcn_readfirstlane(wv) - BWD_WAVES;
    if (rw >= 0) {   // (wave-uniform: the role waves meet the dCore waves at the three barriers only)
      head_dw_role_waves(feat, dY, dW, p.B, p.Cout, (long long)p.P * OP, n_dw, rw,
                         reinterpret_cast<float*>(dsm + dcore_dyn_lds_bytes(MT) + 8192), p);
      return;
    }
#ifdef DCTN_DWROLE_PRIO
    __builtin_amdgcn_s_setprio(DCTN_DWROLE_PRIO);
#endif
  }
  short* tiles = reinterpret_cast<short*>(dsm) + wv * ((1 + MT) * 64 * LROW);
  const TrLane trl = tr_lane(lane);

  // identity B operands of the transposing MFMA: element j of k-step parity sp is
  // [16*sp + 8*h + j == r]
  bf16x8 ident[2];
#pragma unroll
  for (int sp = 0; sp < 2; ++sp)
#pragma unroll
    for (int j = 0; j < 8; ++j) ident[sp][j] = (bf16_t)((16 * sp + 8 * h + j == r) ? 1.f : 0.f);

  f32x16 acc[MT][AT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int a = 0; a < AT; ++a)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][a][v] = 0.f;

  const WaveJob job = wave_job(p, BWD_WAVES, (int)sizeof(S), HEADC > 0);
  const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, p.x_bytes);
  // non-head: rows of dY; head: rows of the forward output (same layout)
  const __amdgpu_buffer_rsrc_t rs_dy = make_rsrc(HEADC > 0 ? feat : dY, p.o_bytes);
  // HEADMM (the head fused, cfg2's shape): dY and dW of a group of 8 samples come from small matrix-core products instead
  // of 2 * Cout * OP multiply-adds per window on the vector ALU (84 of the loop's 290 vector instructions).
  constexpr bool HEADMM = HEADC > 0 && HEADC <= 16 && LDST && OVEC && XVEC && sizeof(S) == 2 && OP == 4;
  float hwf[HEADC > 0 && !HEADMM ? HEADC : 1][OP];
  float dwacc[HEADC > 0 && !HEADMM ? HEADC : 1][OP];
#pragma unroll
  for (int c = 0; c < (HEADC > 0 && !HEADMM ? HEADC : 1); ++c)
#pragma unroll
    for (int o = 0; o < OP; ++o) dwacc[c][o] = 0.f;
  constexpr int DLW = HEADC > 0 ? HEADC / 2 : 1;   // dwords of one row of dLogits (bf16 pairs)
  const unsigned* dl32 = reinterpret_cast<const unsigned*>(dY);
  unsigned dlraw[DLW];
  RawRow<S, OP> rr[HEADC > 0 && !HEADMM ? HEADC : 1];
  // LATE (the cfg2 shape with the head fused): the first sample's window goes out BEFORE the head-weight slice (a wave's
  // loads return in order) and dY / dW are formed after the window's own products, so the 150 instructions that need only
  // x run while the weight slice is still on its way
  constexpr bool LATE = HEADC > 0 && LDST && !HEADMM;
  auto issue_head_weight = [&]() {
    if constexpr (HEADC > 0 && !HEADMM) {
      const __amdgpu_buffer_rsrc_t rs_hw = make_rsrc(hw, p.hw_bytes);
      const unsigned voff_hw = job.valid ? (unsigned)job.pos * (unsigned)(OP * 2) : p.hw_bytes;
#pragma unroll
      for (int c = 0; c < HEADC; ++c)   // rows >= Cout: out of range -> zeros
        issue_row<S, OP, true>(rs_hw, c < p.Cout ? voff_hw : p.hw_bytes, (unsigned)c * p.hw_rowb, OP, rr[c]);
    }
  };
  // One 64-window step of the LDST shapes: the lane's rows of P0 and Z = P1 (x) dY go to the wave's transposition tiles,
  // come back with the windows on the k index and meet on the matrix core.  `make_dy` supplies dY of the lane's window
  // after the P0 / P1 products have been formed and P0 written (whatever it waits for has had that long to arrive).
  auto ldst_step = [&](const float (&xv)[N][2], auto&& make_dy) {
    if constexpr (LDST) {
      bf16x8 X[KS], Y[KS];
      build_p0<N0>(xv, X, Y);
      // P1 by doubling, a pair per multiply: (p1[bb], p1[bb | 1 << u]) = p1[bb] * (x[0], x[1]) (b bit u <-> factor N-1-u)
      float p1[BN];
      p1[0] = xv[N - 1][0];
      p1[1] = xv[N - 1][1];
#pragma unroll
      for (int u = 1; u < N1; ++u)
#pragma unroll
        for (int bb = (1 << u) - 1; bb >= 0; --bb) {
          const f32x2 pr = bmul2(p1[bb], f32x2{xv[N - 1 - u][0], xv[N - 1 - u][1]});
          p1[bb] = pr[0];
          p1[bb | (1 << u)] = pr[1];
        }
      wave_lds_sync();   // the previous step's transposed reads are done
      // the lane's window = its row of every tile; features in natural a order: 16 s + j, 16 s + 8 + j
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        *reinterpret_cast<bf16x8*>(tiles + trl.wr[2 * s2]) = X[s2];
        *reinterpret_cast<bf16x8*>(tiles + trl.wr[2 * s2 + 1]) = Y[s2];
      }
      float dyl[OP];
      make_dy(dyl);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
          int4v zr;   // z[j] = p1[m >> LOGO] * dy[m & (OP - 1)], m = (t << 5) | (c4 << 3) | j: pairs share the p1 factor
#pragma unroll
          for (int jp = 0; jp < 4; ++jp) {
            const int m = (t << 5) | (c4 << 3) | (2 * jp);
            static_assert(OP >= 2, "a pair of consecutive m shares b = m >> LOGO");
            const f32x2 zz = bmul2(p1[m >> LOGO], f32x2{dyl[m & (OP - 1)], dyl[(m + 1) & (OP - 1)]});
            zr[jp] = (int)pack_bf16(zz[0], zz[1]);
          }
          *reinterpret_cast<bf16x8*>(tiles + (1 + t) * 64 * LROW + trl.wr[c4]) = __builtin_bit_cast(bf16x8, zr);
        }
      wave_lds_sync();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 p0t = tr_frag(tiles, ks, trl);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const bf16x8 zt = tr_frag(tiles + (1 + t) * 64 * LROW, ks, trl);
          acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(zt, p0t, acc[t][0], 0, 0, 0);
        }
      }
    }
  };
  if constexpr (HEADMM) {
    // Role of the lane in the small product of a group of 8 samples (32x32x16 tiles, lane = (r, h)):
    //   dY[sample][pos] = sum_class dLogits[sample][class] W[class][pos][o]:   A row r <-> sample slot 4 (r >> 3) + (r & 3) of
    //     the lane half (r >> 2) & 1 whose positions the tile holds (rows of the other half are zero), so the two tiles
    //     of an output (positions 0-31 / 32-63 of the wave) add into ONE accumulator and register v of lane (r, h) is
    //     sample v at the lane's own position;
    //   (dW = dLogits^T x feat is NOT formed here: eps_head_reduce_k's `gemm` role.)
    // The head-weight operand is the same for the workgroup's 8 waves (same positions): 16 classes x 64 positions x 8 bytes
    // are staged ONCE through LDS (one 16-byte load per thread, behind the tiles) - loaded per wave it was 64 KB per CU
    // through the vector-memory path in front of the first sample.
    static_assert(BWD_WAVES * 64 * 16 == 16 * 64 * OP * 2, "one 16-byte load per thread stages the weight slice");
    RawWindow<S, N, XVEC, ROWS> rawm;
    if (job.b0 < job.b1) issue_window<S, N, XVEC, ROWS>(rs_x, job.voff_x, (unsigned)job.b0 * p.s1b, p, rawm);
    const unsigned dl_bytes = (unsigned)p.B * (unsigned)p.Cout * 2u, dlrow = (unsigned)p.Cout * 2u;
    const __amdgpu_buffer_rsrc_t rs_dl = make_rsrc(dY, dl_bytes);
    const int slot = 4 * (r >> 3) + (r & 3);
    const bool rlow = ((r >> 2) & 1) == 0;
    // a group's operand: 16 bytes of dLogits per lane
    u32x4 fa;
    auto issue_group = [&](int g0) {
      const unsigned voff_a = (r < 16 && g0 + slot < job.b1 && 8 * h < p.Cout) ? (unsigned)slot * dlrow + 16u * h : dl_bytes;
      fa = __builtin_amdgcn_raw_buffer_load_b128(rs_dl, voff_a, (unsigned)g0 * dlrow, 0);
    };
    u32x4 wv4;
    {
      const __amdgpu_buffer_rsrc_t rs_hw = make_rsrc(hw, p.hw_bytes);
      const int e = 2 * tid, c = e >> 6, posl = e & 63, pos = job.pos - lane + posl;   // two positions of one class
      const unsigned voff = pos < p.P ? (unsigned)pos * (unsigned)(OP * 2) : p.hw_bytes;   // (a class >= Cout lies past the end: zeros)
      wv4 = __builtin_amdgcn_raw_buffer_load_b128(rs_hw, voff, (unsigned)c * p.hw_rowb, 0);
      if (pos + 1 >= p.P) { wv4.z = 0u; wv4.w = 0u; }   // the second position lies in the next class's row (or past the end)
    }
    // the first group's dLogits go out behind the weight slice and in front of the barrier that publishes it: one
    // 16-byte load of 16 lanes per wave whose round trip the slice's hides (an empty wave: out of range, zeros)
    issue_group(job.b0);
    *reinterpret_cast<u32x4*>(dsm + dcore_dyn_lds_bytes(MT) + (size_t)tid * 16) = wv4;
    __syncthreads();
    const unsigned* wlds = reinterpret_cast<const unsigned*>(dsm + dcore_dyn_lds_bytes(MT));   // [class][position][2 dwords]
    DCTN_STAMP(p, 1);
    for (int g0 = job.b0; g0 < job.b1; g0 += 8) {
      // (round 3, the kernel at 254 registers with dW inside: the first group's loads in front of the barrier made it
      //  slower, 250 VGPRs, 32.3 against 32.1 us per step)
      if (g0 != job.b0) issue_group(g0);
      f32x8 dyg[OP];   // registers 0..7 = the 8 samples of the group at the lane's position
      // dY of the group's samples and the group's share of dW (formed in front of the group's first sample: inside its
      // step, behind the window's own products, the operands' registers met P0 / P1's and the kernel spilled: 15.3 us)
      auto group_products = [&]() {
        int4v a0, a1;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const bool dv = 8 * h + 2 * d < p.Cout;   // classes past Cout: the next sample's row, not zeros
          const int v = (int)(d == 0 ? fa.x : d == 1 ? fa.y : d == 2 ? fa.z : fa.w);
          a0[d] = (dv && rlow) ? v : 0;
          a1[d] = (dv && !rlow) ? v : 0;
        }
        // Every B operand is built before the first product and none is overwritten until 16 wait states after the last
        // one.  Interleaved, the compiler let a v_perm_b32 overwrite the B operand of the 32x32x16 product issued just
        // before it, with no wait state between them, and gave two products a destination overlapping their own B
        // operand; a few dY entries then changed from run to run (found by the exact-input tests, tests/test_gpu_exact.py).
        int4v bw[OP][2];   // B[k = class 8 h + 2 d, 2 d + 1][column = position 32 hh + r]
#pragma unroll
        for (int o = 0; o < OP; ++o) {
          const unsigned sel = (o & 1) ? 0x07060302u : 0x05040100u;   // the odd / even halves of two dwords
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const unsigned lo = wlds[((8 * h + 2 * d) * 64 + 32 * hh + r) * 2 + (o >> 1)];
              const unsigned hi = wlds[((8 * h + 2 * d + 1) * 64 + 32 * hh + r) * 2 + (o >> 1)];
              bw[o][hh][d] = (int)__builtin_amdgcn_perm(hi, lo, sel);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 0; o < OP; ++o) {
          f32x16 dya;
#pragma unroll
          for (int v = 0; v < 16; ++v) dya[v] = 0.f;
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
            dya = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, hh == 0 ? a0 : a1),
                                                           __builtin_bit_cast(bf16x8, bw[o][hh]), dya, 0, 0, 0);
          dyg[o] = __builtin_shufflevector(dya, dya, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        // the operands stay live through the wait, so no product's destination and no later write can take their registers
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7\n\ts_nop 7" ::"v"(a0), "v"(a1), "v"(bw[0][0]), "v"(bw[0][1]), "v"(bw[1][0]), "v"(bw[1][1]),
                     "v"(bw[2 % OP][0]), "v"(bw[2 % OP][1]), "v"(bw[3 % OP][0]), "v"(bw[3 % OP][1]) : "memory");
        __builtin_amdgcn_sched_barrier(0);
      };
      group_products();
      // the 8 samples unrolled: dY of sample s is a fixed register (a run-time index costs a 7-deep select chain each)
#pragma unroll
      for (int sidx = 0; sidx < 8; ++sidx) {
        const int b = g0 + sidx;
        if (b < job.b1) {
          float xv[N][2];
          unpack_window<S, N, XVEC, ROWS>(rawm, xv);
          {
            const int bn = b + 1 < job.b1 ? b + 1 : b;
            issue_window<S, N, XVEC, ROWS>(rs_x, job.voff_x, (unsigned)bn * p.s1b, p, rawm);
            __builtin_amdgcn_sched_barrier(0);
          }
          ldst_step(xv, [&](float (&dyo)[OP]) {
#pragma unroll
            for (int o = 0; o < OP; ++o) dyo[o] = dyg[o][sidx];
          });
          __builtin_amdgcn_sched_barrier(0);
          if (sidx == 0 && g0 == job.b0) DCTN_STAMP(p, 2);
        }
      }
    }
  } else {
  if constexpr (!LATE) issue_head_weight();
  RawWindow<S, N, XVEC, ROWS> raw;
  RawRow<S, OP> rawdy;
  if (job.b0 < job.b1) {
    issue_window<S, N, XVEC, ROWS>(rs_x, job.voff_x, (unsigned)job.b0 * p.s1b, p, raw);
    if constexpr (HEADC > 0) {
#pragma unroll
      for (int i = 0; i < DLW; ++i) {   // clamped index + select: no control flow around the scalar loads
        const unsigned v = dl32[(long long)job.b0 * (p.Cout / 2) + (2 * i < p.Cout ? i : 0)];
        dlraw[i] = 2 * i < p.Cout ? v : 0u;
      }
    }
    issue_row<S, OP, OVEC>(rs_dy, job.voff_o, (unsigned)job.b0 * p.o_s1b, p.O, rawdy);
  }
  if constexpr (LATE) issue_head_weight();
  if constexpr (HEADC > 0 && !LATE) {   // the weight slice arrives together with the first sample's loads
#pragma unroll
    for (int c = 0; c < HEADC; ++c) unpack_row<S, OP, true>(rr[c], hwf[c]);
  }
  DCTN_STAMP(p, 1);
  for (int b = job.b0; b < job.b1; ++b) {
    float xv[N][2];
    unpack_window<S, N, XVEC, ROWS>(raw, xv);
    if (b == job.b0) DCTN_STAMP(p, 2);
    float dy[OP];
    float ft[OP];                 // head: forward output of the window (zeros for lanes without a position)
    unsigned dlnow[DLW];          // head: dLogits of this sample (the prefetch below overwrites dlraw)
    auto head_dy_dw = [&]() {
#pragma unroll
      for (int o = 0; o < OP; ++o) dy[o] = 0.f;
#pragma unroll
      for (int c = 0; c < HEADC; ++c) {
        const float dl = (c & 1) ? __uint_as_float(dlnow[c >> 1] & 0xffff0000u) : __uint_as_float(dlnow[c >> 1] << 16);
#pragma unroll
        for (int o = 0; o < OP; ++o) {
          dy[o] = __builtin_fmaf(dl, hwf[c][o], dy[o]);
          dwacc[c][o] = __builtin_fmaf(dl, ft[o], dwacc[c][o]);
        }
      }
    };
    if constexpr (HEADC > 0) {
      unpack_row<S, OP, OVEC>(rawdy, ft);
#pragma unroll
      for (int i = 0; i < DLW; ++i) dlnow[i] = dlraw[i];
      if constexpr (!LATE) head_dy_dw();
    } else {
      unpack_row<S, OP, OVEC>(rawdy, dy);
    }
    {  // prefetch the next sample of this wave
      const int bn = b + 1 < job.b1 ? b + 1 : b;
      issue_window<S, N, XVEC, ROWS>(rs_x, job.voff_x, (unsigned)bn * p.s1b, p, raw);
      if constexpr (HEADC > 0) {
#pragma unroll
        for (int i = 0; i < DLW; ++i) {
          const unsigned v = dl32[(long long)bn * (p.Cout / 2) + (2 * i < p.Cout ? i : 0)];
          dlraw[i] = 2 * i < p.Cout ? v : 0u;
        }
      }
      issue_row<S, OP, OVEC>(rs_dy, job.voff_o, (unsigned)bn * p.o_s1b, p.O, rawdy);
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this step's arithmetic
    }
    // lanes without a window position read zeros for x: their P0 is 0 and they contribute nothing

    if constexpr (LDST) {
      ldst_step(xv, [&](float (&dyo)[OP]) {
        if constexpr (LATE) {
          if (b == job.b0) {   // the weight slice has had the whole P0 / P1 build to arrive
#pragma unroll
            for (int c = 0; c < HEADC; ++c) unpack_row<S, OP, true>(rr[c], hwf[c]);
          }
          head_dy_dw();
        }
#pragma unroll
        for (int o = 0; o < OP; ++o) dyo[o] = dy[o];
      });
      continue;
    }

    // P0 of the lane's own window -> A operands of set 0 / set 1 -> transposed on the matrix core:
    // features on lanes, windows in registers = B operand fragments summing over windows
    bf16x8 pf[2][KS];
    build_p0<N0>(xv, pf[0], pf[1]);
#pragma unroll
    for (int s = 0; s < KS; ++s) swap_halves(pf[0][s], pf[1][s]);
    bf16x8 p0t[2][AT][2];
#pragma unroll
    for (int set = 0; set < 2; ++set)
#pragma unroll
      for (int a = 0; a < AT; ++a) {
        f32x16 d;
#pragma unroll
        for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
        for (int sp = 0; sp < 2; ++sp)
          if (2 * a + sp < KS)
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[set][2 * a + sp], ident[sp], d, 0, 0, 0);
        p0t[set][a][0] = pack8(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
        p0t[set][a][1] = pack8(d[8], d[9], d[10], d[11], d[12], d[13], d[14], d[15]);
      }
    // full P1 table of this window (b bit u <-> factor N-1-u)
    float p1[BN];   // built by doubling: 2 + 4 + ... + BN multiplies instead of (N1 - 1) * BN
    p1[0] = xv[N - 1][0];
    p1[1] = xv[N - 1][1];
#pragma unroll
    for (int u = 1; u < N1; ++u)
#pragma unroll
      for (int b = (1 << u) - 1; b >= 0; --b) {
        const float lo = p1[b];
        p1[b | (1 << u)] = lo * xv[N - 1 - u][1];
        p1[b] = lo * xv[N - 1 - u][0];
      }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      // Z of the own window for both k-halves, then the same hand-over as for P0
      bf16x8 zf[2][2];   // [set after the swap][sp]
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        float za[8], zb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ma = (t << 5) | (sp << 4) | j;        // first k-half
          const int mb = ma | 8;                           // second k-half
          za[j] = p1[ma >> LOGO] * dy[ma & (OP - 1)];
          zb[j] = p1[mb >> LOGO] * dy[mb & (OP - 1)];
        }
        zf[0][sp] = pack8(za[0], za[1], za[2], za[3], za[4], za[5], za[6], za[7]);
        zf[1][sp] = pack8(zb[0], zb[1], zb[2], zb[3], zb[4], zb[5], zb[6], zb[7]);
        swap_halves(zf[0][sp], zf[1][sp]);
      }
#pragma unroll
      for (int set = 0; set < 2; ++set) {
        f32x16 d;
#pragma unroll
        for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
        for (int sp = 0; sp < 2; ++sp)
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(zf[set][sp], ident[sp], d, 0, 0, 0);
        bf16x8 zt[2];
        zt[0] = pack8(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
        zt[1] = pack8(d[8], d[9], d[10], d[11], d[12], d[13], d[14], d[15]);
#pragma unroll
        for (int a = 0; a < AT; ++a)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
            acc[t][a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(zt[s2], p0t[set][a][s2], acc[t][a], 0, 0, 0);
      }
    }
  }
  }   // !HEADMM

  DCTN_STAMP(p, 3);
  DCTN_STAMP_W(p, wv);
  // workgroup reduction of the per-wave partial dCoreT tiles, then one coalesced store per block
  float* dst = partial + (long long)blockIdx.x * (MT * 32) * (AT * 32);
  if constexpr (LDST) {
    // the transposition tiles (96 KiB) are free once every wave has left the loop: all MT tiles of all waves meet
    // there in ONE round (two barriers) instead of one round per tile through the 32 KiB static buffer
    static_assert(AT == 1 && (size_t)BWD_WAVES * MT * 1024 * 4 <= dcore_dyn_lds_bytes(MT), "dCore tiles must fit");
    float* big = reinterpret_cast<float*>(dsm);
    DCTN_STAMP_T(p, 6, 64 * (BWD_WAVES - 1));
    __syncthreads();
    DCTN_STAMP(p, 7);
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = (v & 3) + 8 * (v >> 2) + 4 * h;
        big[(wv * MT + t) * 1024 + row * 32 + r] = acc[t][0][v];
      }
    __syncthreads();
    // thread t sums elements 4 t .. 4 t + 3 (each in wave order k = 0 .. 7) and stores them as one 16-byte store whose
    // policy is DCTN_WT_TILES; MT = 2: every dCore thread once, MT = 1: the first half of them
    typedef __attribute__((ext_vector_type(4))) float f32x4v;
    const __amdgpu_buffer_rsrc_t rs_t = make_rsrc(dst, (unsigned)(MT * 1024 * sizeof(float)));
    for (int e = 4 * tid; e < MT * 1024; e += 4 * 64 * BWD_WAVES) {
      f32x4v sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < BWD_WAVES; ++k) sum += *reinterpret_cast<const f32x4v*>(big + k * MT * 1024 + e);
      // [t][row][col] = row-major (MT * 32) x 32
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sum), rs_t, (unsigned)e * 4u, 0, DCTN_WT_TILES);
    }
  } else {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int a = 0; a < AT; ++a) {
        __syncthreads();
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = (v & 3) + 8 * (v >> 2) + 4 * h;
          red[wv][row * 32 + r] = acc[t][a][v];
        }
        __syncthreads();
        for (int e = tid; e < 1024; e += 64 * BWD_WAVES) {
          float sum = 0.f;
#pragma unroll
          for (int k = 0; k < BWD_WAVES; ++k) sum += red[k][e];
          const int row = e >> 5, col = e & 31;
          dst[(long long)(t * 32 + row) * (AT * 32) + a * 32 + col] = sum;
        }
      }
  }

  DCTN_STAMP(p, 4);
  if constexpr (HEADC > 0 && !HEADMM) {
    // head-weight gradient: sum the 8 waves (same positions, different sample chunks) in LDS and store the
    // workgroup's partial tile; LDS index (cc*64 + lane)*OP + o makes the stores run along the feature index.
    // LDST shapes: as many classes per round as the 96 KiB of tiles hold (all 10 of cfg2: one round); others: the
    // 32 KiB static buffer, a few classes per round.
    constexpr int SLOT = LDST ? (int)(dcore_dyn_lds_bytes(MT) / (BWD_WAVES * 4)) : 1024;   // floats per wave
    constexpr int CPR_RAW = SLOT / (64 * OP);
    constexpr int CPR = CPR_RAW > HEADC ? HEADC : CPR_RAW;   // classes per round
    float* red1 = LDST ? reinterpret_cast<float*>(dsm) : &red[0][0];
    const int nbk = gridDim.x;
    const int vbk = (nbk % 8 == 0) ? (int)(blockIdx.x % 8) * (nbk / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    const int cb = vbk / p.npg, pg = vbk - cb * p.npg;
    const int F = p.P * OP;
#pragma unroll
    for (int c0 = 0; c0 < HEADC; c0 += CPR) {
      __syncthreads();
#pragma unroll
      for (int cc = 0; cc < CPR; ++cc)
#pragma unroll
        for (int o = 0; o < OP; ++o) {
          // static register index: unrolled over every (c0, cc) pair that can occur
          float v = 0.f;
#pragma unroll
          for (int c = 0; c < HEADC; ++c) v = (c == c0 + cc) ? dwacc[c][o] : v;
          red1[wv * SLOT + (cc * 64 + lane) * OP + o] = v;
        }
      __syncthreads();
      for (int e = tid; e < CPR * 64 * OP; e += 64 * BWD_WAVES) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < BWD_WAVES; ++k) sum += red1[k * SLOT + e];
        const int cc = e / (64 * OP), rem = e - cc * (64 * OP);   // rem = lane*OP + o
        const int c = c0 + cc, f = pg * 64 * OP + rem;
        if (cb < p.ncb && c < p.Cout && f < F) dwpart[((long long)cb * p.Cout + c) * F + f] = sum;
      }
    }
  }
  DCTN_STAMP(p, 5);
}

// dCore[a][b][o] = sum_blocks partial[blk][m = b*OP + o][a].  One workgroup per 32 consecutive
// (m, a) entries: lane (k8 = tid / 32, c = tid % 32) streams every 8th block's 128-byte segment
// (coalesced), the 8 partial sums meet in LDS.
template <typename S>
__global__ __launch_bounds__(256) void eps_bwd_dcore_reduce_k(const float* __restrict__ partial,
                                                              S* __restrict__ dCore, int nblk, int A,
                                                              int BN, int O, int OP, int ACOLS) {
  __shared__ float red[8][32];
  const int tid = threadIdx.x, c = tid & 31, k8 = tid >> 5;
  const long long stride = (long long)BN * OP * ACOLS;
  const long long e = (long long)blockIdx.x * 32 + c;  // flat (m, a) index
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  int k = k8;
  for (; k + 56 < nblk; k += 64) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += partial[(k + 8 * i) * stride + e];
  }
  for (; k < nblk; k += 8) acc[0] += partial[k * stride + e];
  red[k8][c] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (k8 == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][c];
    const int m = (int)(e / ACOLS), a = (int)(e % ACOLS);
    const int b = m / OP, o = m % OP;
    if (a < A && o < O) dCore[((long long)a * BN + b) * O + o] = (S)t;
  }
}

// Second (and last) kernel of the fused head backward: workgroups [0, n_core) finish dCore exactly
// as eps_bwd_dcore_reduce_k does, the next n_dw sum the ncb partial tiles of the head-weight gradient
// (256 consecutive features each), the last one sums dLogits over the batch into dBias.
// The `gemm` role of eps_head_reduce_k (HEADMM shapes, cfg2): dW[c][f] = sum_b dLogits[b][c] * feat[b][f] for the
// DWG_FW features of one workgroup's slice, on v_mfma_f32_16x16x32_bf16 (rows = classes, columns = features,
// k = samples).  Wave w takes the samples [w spw, (w + 1) spw) in blocks of 32; lane (n, kg) = (lane % 16, lane / 16)
// loads, for the 8 samples 8 kg .. 8 kg + 7 of a block, its FL = DWG_FW / 16 features of the row and one value of
// dLogits - the k-contiguous fragments come from 8 loads, never from a transpose; tile j of the wave is the features
// FL n + j.  The next block's loads are issued before the current block's products (B = 1024: both blocks of a wave in
// flight at once).  The 16 waves' tiles meet in LDS (dynamic), thread (slot, lane) sums one element in wave order
// (deterministic) and stores it.
// What bounds the role (tools/stamp_cfg2.hip) is the volume ONE CU pulls through its memory path: with 64-feature
// slices (128-byte pieces of 1024 rows, 43 workgroups) the first loads are back 2.3 us after the kernel's start, the
// last wave's after 5.5, the role ends at 6.1 us (the dCore roles next to it at 2.0).  32-feature slices (64-byte
// pieces - the memory path fetches 64-byte sectors, so the volume per CU halves; 85 workgroups) end at 4.8 us;
// 16-feature slices (32-byte pieces, 169 workgroups) at 5.3: a sector is the least a piece costs.  Tried and dropped:
//  * the product as its own kernel on a forked side stream next to the dCore kernel - the two cross-stream
//    dependencies cost more than the kernel: 45.9 us per step in the graph, 30.7 us per eager call;
//  * the samples split 4 ways over 172 workgroups, the 4 KiB partial tiles combined by the last workgroup of a slice
//    to arrive (write-through stores, an agent-scope counter zeroed by the dCore kernel, agent-scope loads; parity
//    green): products done after 2.5 us instead of 5.5, but the store-and-count costs 1.3 us and the last arriver's
//    re-read 1.2 (release / acquire on the counter: 2.5 + 2.5) - the role ends at 6.0 us, no gain for the machinery.
// BLK4: the features in the blocked4 layout (eps_fwd_head_q2reg_t_k under DCTN_OPT_HEAD_FEATURES_BLOCKED4): the 8
// samples of lane kg are the 4-sample blocks 2 kg, 2 kg + 1 of the 32-sample block, and a block's FL features of the
// lane are FL * 8 contiguous bytes in exactly the fragment's k order - TWO loads (FL * 8 bytes each) instead of eight,
// no byte permutes, and a slice of the features is one contiguous (DWG_BFW * 8)-byte piece per 4 samples instead of
// four row pieces.  Same products, same sample split over the waves, same LDS join: the same bits as the row-major role.
constexpr int DWG_WAVES = 16;
constexpr int DWG_FW = 32;   // features of one workgroup's slice (4 bytes of a row per lane: 64-byte pieces of 4 rows per load)
constexpr int DWG_BFW = 16;  // ... with blocked4 features (8 bytes of a block per lane: 128-byte pieces, 169 workgroups at cfg2)
typedef __attribute__((ext_vector_type(4))) float f32x4v;
// The loaded operands of one 32-sample block of the product, as the lane holds them.  row-major: f[j] = the lane's piece
// of sample 8 kg + j; blocked4: f[h][.] = its 2 FL dwords of block 2 kg + h; a[j] = dLogits of sample 8 kg + j, the dword
// that holds class n (a 16-bit load's widening is an instruction that waits for the load where it was issued).
template <int FW, bool BLK4>
struct DwBlock {
  static constexpr int FL = FW / 16;               // features per lane = tiles per wave
  static constexpr int FD = FL >= 2 ? FL / 2 : 1;   // dwords of a row piece per lane
  static constexpr int NF = BLK4 ? 2 : 8, ND = BLK4 ? 2 * FL : FD;
  static_assert(!BLK4 || FL == 1 || FL == 2, "blocked4 pieces of 8 or 16 bytes");
  unsigned f[NF][ND];
  unsigned a[8];
};
// The lane's share of a slice: lane (n, kg) = (lane % 16, lane / 16), features fcol .. fcol + FL - 1.  Every address of
// a block is "per-lane offset inside the block + the block's scalar offset": fo[j] / ao[j] are the lane's byte offsets of
// its j-th feature piece / dLogits dword in block 0 (out of range for a lane without a feature or a class), the block
// adds kb * F * 2 / kb * Cout * 2 as the loads' scalar offset - a whole block inside the batch costs no address
// arithmetic at all (what the role waves of the dCore kernel issue next to its prologue).
template <int NF>
struct DwLane {
  unsigned f_bytes, dl_bytes;
  unsigned frow2, arow;   // bytes of a sample's features / dLogits
  unsigned fo[NF], ao[8];
  int n, kg;
  unsigned asel;   // v_perm selector of class n's half of two dLogits dwords
};
template <int FW, bool BLK4>
__device__ __forceinline__ DwLane<DwBlock<FW, BLK4>::NF> dw_lane(int B, int Cout, long long F, int blk) {
  constexpr int FL = FW / 16, NF = DwBlock<FW, BLK4>::NF;
  const int lane = threadIdx.x & 63;
  DwLane<NF> l;
  const long long fb = BLK4 ? (long long)(B + 3) / 4 * 4 * F * 2 : (long long)B * F * 2;
  l.f_bytes = (unsigned)fb;
  l.dl_bytes = (unsigned)B * (unsigned)Cout * 2u;
  l.frow2 = (unsigned)F * 2u;
  l.arow = (unsigned)Cout * 2u;
  l.n = lane & 15;
  l.kg = lane >> 4;
  l.asel = (l.n & 1) ? 0x07060302u : 0x05040100u;
  const long long fcol = (long long)blk * FW + FL * l.n;
  const bool fok = fcol + FL - 1 < F;   // (F is a multiple of 4: OP == 4)
#pragma unroll
  for (int j = 0; j < NF; ++j)   // blocked4: the 4-sample block 2 kg + j; row-major: sample 8 kg + j
    l.fo[j] = !fok ? l.f_bytes : BLK4 ? (unsigned)(((long long)(2 * l.kg + j) * F + fcol) * 8) : (unsigned)((8 * l.kg + j) * F * 2 + fcol * 2);
#pragma unroll
  for (int j = 0; j < 8; ++j)   // (Cout is even and dLogits 4-byte aligned: the dword of the classes n & ~1, n | 1)
    l.ao[j] = l.n < Cout ? (unsigned)(8 * l.kg + j) * l.arow + 2u * (unsigned)(l.n & ~1) : l.dl_bytes;
  return l;
}
// samples per (virtual) wave of the product: the batch split DWG_WAVES ways in whole 32-sample blocks
__device__ __forceinline__ int dw_spw(int B) { return (((B + DWG_WAVES - 1) / DWG_WAVES) + 31) / 32 * 32; }
// issue the loads of the block of samples kb .. kb + 31 (samples >= b1: zeros)
template <int FW, bool BLK4>
__device__ __forceinline__ void dw_block_issue(const __amdgpu_buffer_rsrc_t rs_f, const __amdgpu_buffer_rsrc_t rs_dl,
                                               const DwLane<DwBlock<FW, BLK4>::NF>& l, int kb, int b1, DwBlock<FW, BLK4>& q) {
  constexpr int FL = DwBlock<FW, BLK4>::FL, NF = DwBlock<FW, BLK4>::NF, ND = DwBlock<FW, BLK4>::ND;
  const unsigned so_f = (unsigned)kb * l.frow2, so_a = (unsigned)kb * l.arow;
  auto loads = [&](auto whole) {   // whole: every sample of the block is one of the wave's (wave-uniform)
#pragma unroll
    for (int j = 0; j < NF; ++j) {   // a piece is loaded if it holds a sample of the wave (past the batch: zeros)
      const unsigned vo = (decltype(whole)::value || kb + 8 * l.kg + (BLK4 ? 4 : 1) * j < b1) ? l.fo[j] : l.f_bytes;
      if constexpr (ND == 1 && !BLK4 && FL == 1) {
        q.f[j][0] = (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs_f, vo, so_f, 0);
      } else if constexpr (ND == 1) {
        q.f[j][0] = __builtin_amdgcn_raw_buffer_load_b32(rs_f, vo, so_f, 0);
      } else if constexpr (ND == 2) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_f, vo, so_f, 0);
        q.f[j][0] = v.x;
        q.f[j][1] = v.y;
      } else {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_f, vo, so_f, 0);
#pragma unroll
        for (int d = 0; d < 4; ++d) q.f[j][d] = v[d];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      q.a[j] = __builtin_amdgcn_raw_buffer_load_b32(
          rs_dl, (decltype(whole)::value || kb + 8 * l.kg + j < b1) ? l.ao[j] : l.dl_bytes, so_a, 0);
  };
  if (kb + 32 <= b1) loads(std::true_type{}); else loads(std::false_type{});
}
// acc[j] += dLogits^T x features of the block, tile j = the features FL n + j
template <int FW, bool BLK4>
__device__ __forceinline__ void dw_block_mfma(const DwBlock<FW, BLK4>& q, unsigned asel, f32x4v (&acc)[FW / 16]) {
  constexpr int FL = DwBlock<FW, BLK4>::FL;
  int4v at;
#pragma unroll
  for (int d = 0; d < 4; ++d) at[d] = (int)__builtin_amdgcn_perm(q.a[2 * d + 1], q.a[2 * d], asel);
#pragma unroll
  for (int j = 0; j < FL; ++j) {
    int4v bf;
    if constexpr (BLK4) {   // feature fcol + j of samples 0-3 and 4-7: dwords 2 j, 2 j + 1 of the two blocks
#pragma unroll
      for (int d = 0; d < 4; ++d) bf[d] = (int)q.f[d >> 1][2 * j + (d & 1)];
    } else {
      const unsigned sel = (j & 1) ? 0x07060302u : 0x05040100u;   // the odd / even halves of two dwords
#pragma unroll
      for (int d = 0; d < 4; ++d)
        bf[d] = FL == 1 ? (int)(q.f[2 * d][0] | (q.f[2 * d + 1][0] << 16))
                        : (int)__builtin_amdgcn_perm(q.f[2 * d + 1][j >> 1], q.f[2 * d][j >> 1], sel);
    }
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, at), __builtin_bit_cast(bf16x8, bf), acc[j], 0, 0, 0);
  }
}

template <int FW, bool BLK4>
__device__ __forceinline__ void head_dw_gemm_role(const bf16_t* __restrict__ feat, const bf16_t* __restrict__ dL,
                                                  bf16_t* __restrict__ dW, int B, int Cout, long long F, int blk,
                                                  float* __restrict__ lds) {
  constexpr int FL = FW / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const auto l = dw_lane<FW, BLK4>(B, Cout, F, blk);
  const int n = l.n, kg = l.kg;
  const __amdgpu_buffer_rsrc_t rs_f = make_rsrc(feat, l.f_bytes), rs_dl = make_rsrc(dL, l.dl_bytes);
  const int spw = dw_spw(B);
  const int b0 = wv * spw, b1 = b0 + spw < B ? b0 + spw : B;
  f32x4v acc[FL];
#pragma unroll
  for (int j = 0; j < FL; ++j) acc[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
  DwBlock<FW, BLK4> cur, nxt;
  DCTN_STAMP_G(0);
  if (b0 < b1) dw_block_issue<FW, BLK4>(rs_f, rs_dl, l, b0, b1, cur);
  for (int kb = b0; kb < b1; kb += 32) {
    if (kb + 32 < b1) dw_block_issue<FW, BLK4>(rs_f, rs_dl, l, kb + 32, b1, nxt);
    __builtin_amdgcn_sched_barrier(0);
    dw_block_mfma<FW, BLK4>(cur, l.asel, acc);
    cur = nxt;
  }
  // acc[j][i] = dW[class 4 kg + i][feature DWG_FW blk + FL n + j] of this wave's samples
#pragma unroll
  for (int j = 0; j < FL; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) lds[(wv * (4 * FL) + j * 4 + i) * 64 + lane] = acc[j][i];
  DCTN_STAMP_G(1);
  __syncthreads();
  DCTN_STAMP_G(2);
  if (tid < 4 * FL * 64) {
    const int slot = tid >> 6, j = slot >> 2, i = slot & 3;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < DWG_WAVES; ++w) t += lds[(w * (4 * FL) + slot) * 64 + lane];
    const int c = 4 * kg + i;
    const long long f = (long long)blk * FW + FL * n + j;
    if (c < Cout && f < F) dW[(long long)c * F + f] = (bf16_t)t;
  }
  DCTN_STAMP_G(4);
}

// The same product on the spare wave slots of eps_bwd_dcore_q2reg_k<.., DWROLE> (blocked4 features): the dCore
// workgroup's waves BWD_WAVES .. BWD_WAVES + DWR_WAVES - 1 form the slice `blockIdx.x` together, each as DWR_VPW of the
// finishing kernel's DWG_WAVES waves ("virtual waves": same sample range, one accumulator from zero per virtual wave,
// its 64 x 4 tile in LDS, the same ordered join - the bits of head_dw_gemm_role<DWG_BFW, true>).  Up to DWR_DEPTH blocks
// of a wave are in flight at once (B = 1024: all 8 of a wave); larger batches go round by round.
// Grids smaller than the number of slices (small batches): the slices past the first round are dealt to single role
// waves, which run all DWG_WAVES virtual waves of a slice one after the other - the join is lane-local (tile element
// (i, lane) of every virtual wave sits in register i of the same lane), so the wave sums in registers in the same order
// and needs no hand-over between waves: the kernel keeps its three workgroup barriers.
// All DWR_WAVES waves execute the three barriers of the HEADMM path: (1) the weight slice is published - the role takes
// no part in it, a bare s_barrier that lets its loads stay in flight; (2) every dCore wave has left its loop - the
// role's tiles are in LDS by then; (3) the dCore tiles are in LDS.  The join and the dW stores come after (3), next to
// the dCore tile sums of waves 0 .. BWD_WAVES - 1: nothing of the role lies between the dCore loop and its epilogue.
constexpr int DWR_WAVES = 4, DWR_VPW = DWG_WAVES / DWR_WAVES, DWR_DEPTH = 8;
constexpr size_t DWR_LDS_BYTES = (size_t)DWG_WAVES * 4 * 64 * sizeof(float);   // the 16 virtual waves' tiles
static_assert(DWG_BFW == 16, "one tile per virtual wave");
#ifndef DCTN_DWROLE_EARLY_LOADS
// 1: the role's first loads go out in front of barrier (1).  Off: stamped, the role's 320 loads per CU were in the memory
// path's queue ahead of the weight slice and held barrier (1) back from 1.3 to 3.3 us
#define DCTN_DWROLE_EARLY_LOADS 0
#endif
__device__ __forceinline__ void head_dw_role_waves(const bf16_t* __restrict__ feat, const bf16_t* __restrict__ dL,
                                                   bf16_t* __restrict__ dW, int B, int Cout, long long F, int n_dw,
                                                   int rw, float* __restrict__ lds, const MfmaP& p) {
  typedef DwBlock<DWG_BFW, true> Blk;
  const int lane = threadIdx.x & 63;
  const int nb = dw_spw(B) / 32;   // 32-sample blocks of a virtual wave
  const int slice0 = (int)blockIdx.x;
  const bool coop = slice0 < n_dw;
  auto l = dw_lane<DWG_BFW, true>(B, Cout, F, slice0);
  const __amdgpu_buffer_rsrc_t rs_f = make_rsrc(feat, l.f_bytes), rs_dl = make_rsrc(dL, l.dl_bytes);
  Blk q[DWR_DEPTH];
  // A virtual wave's samples are whole 32-sample blocks, so the blocks of consecutive virtual waves are consecutive
  // blocks of the batch: the wave walks the blocks [gi, ge) of its slice, DWR_DEPTH at a time, and a tile is complete
  // after every nb-th one.  gi = the next block to issue, gc = the next to consume (block kc of virtual wave vc).
  int s = slice0, gi = rw * DWR_VPW * nb, ge = gi + DWR_VPW * nb, gc = gi, kc = 0, vc = rw * DWR_VPW;
  bool solo = false;
  auto issue_round = [&]() {
    const int b1 = 32 * ge < B ? 32 * ge : B;   // (blocks past the wave's share or the batch: no address in range, zeros)
#pragma unroll
    for (int j = 0; j < DWR_DEPTH; ++j) dw_block_issue<DWG_BFW, true>(rs_f, rs_dl, l, 32 * (gi + j), b1, q[j]);
    gi += DWR_DEPTH;
  };
  f32x4v acc[1] = {f32x4v{0.f, 0.f, 0.f, 0.f}};
  f32x4v t4 = f32x4v{0.f, 0.f, 0.f, 0.f};   // a solo slice's join, in registers
  auto consume_round = [&]() {
#pragma unroll
    for (int j = 0; j < DWR_DEPTH; ++j)
      if (gc < ge) {
        if (32 * gc < B) dw_block_mfma<DWG_BFW, true>(q[j], l.asel, acc);   // (as the finishing kernel: no product past the batch)
        ++gc;
        if (++kc == nb) {   // virtual wave vc is complete
          if (solo) {
            t4 += acc[0];
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) lds[(vc * 4 + i) * 64 + lane] = acc[0][i];
          }
          acc[0] = f32x4v{0.f, 0.f, 0.f, 0.f};
          kc = 0;
          ++vc;
        }
      }
  };
  if (DCTN_DWROLE_EARLY_LOADS && coop) issue_round();
  __builtin_amdgcn_s_barrier();   // (1)
  if (coop) {
    if (!DCTN_DWROLE_EARLY_LOADS) issue_round();
    DCTN_STAMP_R(p, 0);
    for (;;) {
      __builtin_amdgcn_sched_barrier(0);
      consume_round();
      if (gc >= ge) {   // the slice is done: on to the next one no workgroup takes in the first round, this wave alone
        if (solo) {
          const long long f = (long long)s * DWG_BFW + l.n;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = 4 * l.kg + i;
            if (c < Cout && f < F) dW[(long long)c * F + f] = (bf16_t)t4[i];
          }
        } else {
          DCTN_STAMP_R(p, 1);
        }
        s += (int)gridDim.x * (solo ? DWR_WAVES : 1 + rw);
        if (s >= n_dw) break;
        solo = true;
        l = dw_lane<DWG_BFW, true>(B, Cout, F, s);
        gi = gc = kc = vc = 0;
        ge = DWG_WAVES * nb;
        t4 = f32x4v{0.f, 0.f, 0.f, 0.f};
      }
      issue_round();
    }
  }
  __syncthreads();                // (2)
  __builtin_amdgcn_s_barrier();   // (3)
  if (coop) {   // thread (slot = rw, lane) sums element (rw, lane) of the 16 tiles in wave order, as head_dw_gemm_role does
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < DWG_WAVES; ++w) t += lds[(w * 4 + rw) * 64 + lane];
    const int c = 4 * (lane >> 4) + rw;
    const long long f = (long long)slice0 * DWG_BFW + (lane & 15);
    if (c < Cout && f < F) dW[(long long)c * F + f] = (bf16_t)t;
  }
  DCTN_STAMP_R(p, 2);
}

__global__ __launch_bounds__(1024) void eps_head_reduce_k(const float* __restrict__ partial,
                                                          bf16_t* __restrict__ dCore, int nblk, int A, int BN,
                                                          int O, int OP, int ACOLS, int n_core,
                                                          const float* __restrict__ dwpart,
                                                          bf16_t* __restrict__ dW, int ncb, long long nW, int n_dw,
                                                          const bf16_t* __restrict__ dL,
                                                          bf16_t* __restrict__ dBias, int B, int Cout,
                                                          const bf16_t* __restrict__ feat, int gemm) {
  // The kernel is a latency chain, not a bandwidth problem: 1024 threads per workgroup so that every
  // partial tile of an element is fetched in ONE round of independent loads.
  __shared__ float red[32][33];
  const int tid = threadIdx.x;
  // gemm == 2 (blocked4 features): the n_dw product workgroups take the lowest block ids, they are dispatched first
  const int bid = gemm == 2 && (int)blockIdx.x < n_core + n_dw
                      ? ((int)blockIdx.x < n_dw ? n_core + (int)blockIdx.x : (int)blockIdx.x - n_dw)
                      : (int)blockIdx.x;
  if (bid < n_core) {
    DCTN_STAMP_G(0);
    const int c = tid & 31, k32 = tid >> 5;
    const long long stride = (long long)BN * OP * ACOLS;
    const long long e = (long long)bid * 32 + c;  // flat (m, a) index
    float acc = 0.f;
    for (int k0 = 0; k0 < nblk; k0 += 256) {   // nblk <= 256: one trip
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {   // clamped index + select: a predicated load is a branch and a wait on the spot (four round trips for eight loads)
        const int k = k0 + k32 + 32 * i;
        const float ld = partial[(k < nblk ? k : nblk - 1) * stride + e];
        v[i] = k < nblk ? ld : 0.f;
      }
      acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    red[k32][c] = acc;
    __syncthreads();
    if (k32 == 0) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) t += red[i][c];
      const int m = (int)(e / ACOLS), a = (int)(e % ACOLS);
      const int b = m / OP, o = m % OP;
      if (a < A && o < O) dCore[((long long)a * BN + b) * O + o] = (bf16_t)t;
    }
    DCTN_STAMP_G(4);
    return;
  }
  if (bid < n_core + n_dw) {
    if (!dW) return;
    if (gemm) {   // no partial tiles: the product itself (n_dw = ceil(F / slice) workgroups, nW = Cout * F)
      extern __shared__ __attribute__((aligned(16))) float gemm_lds[];
      if (gemm == 2) head_dw_gemm_role<DWG_BFW, true>(feat, dL, dW, B, Cout, nW / Cout, bid - n_core, gemm_lds);
      else head_dw_gemm_role<DWG_FW, false>(feat, dL, dW, B, Cout, nW / Cout, bid - n_core, gemm_lds);
      return;
    }
    // 4 threads per element, each up to 8 independent loads (ncb <= 32), joined by two lane shuffles
    const long long e = (long long)(bid - n_core) * 256 + (tid >> 2);
    const int sub = tid & 3;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = sub + 4 * i;
      const float ld = dwpart[(long long)(k < ncb ? k : ncb - 1) * nW + (e < nW ? e : nW - 1)];   // (no branch between the loads)
      v[i] = (k < ncb && e < nW) ? ld : 0.f;
    }
    float t = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    for (int k = 32 + sub; k < ncb; k += 4) t += e < nW ? dwpart[(long long)k * nW + e] : 0.f;
    t += __shfl_xor(t, 1, 64);
    t += __shfl_xor(t, 2, 64);
    if (sub == 0 && e < nW) dW[e] = (bf16_t)t;
    return;
  }
  if (!dBias) return;
  {  // dBias[c] = sum_b dLogits[b, c]: thread (c = tid % 16, j = tid / 16) takes every 64th sample
    const int c = tid & 15, j = tid >> 4;
    float t = 0.f;
    if (c < Cout) {
      int b = j;
      for (; b + 64 * 7 < B; b += 64 * 8) {   // 8 independent loads in flight
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)dL[(long long)(b + 64 * i) * Cout + c];
        t += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
      }
      for (; b < B; b += 64) t += (float)dL[(long long)b * Cout + c];
    }
    __shared__ float rb[64][17];
    rb[j][c] = t;
    __syncthreads();
    if (tid < 16 && tid < Cout) {
      float u = 0.f;
#pragma unroll 8
      for (int i = 0; i < 64; ++i) u += rb[i][tid];
      dBias[tid] = (bf16_t)u;
    }
  }
}

int next_pow2(int v) {
  int r = 1;
  while (r < v) r <<= 1;
  return r;
}

bool family_ok(const EpsP& p, int dtype, int precision) {
  if (p.Q != 2) return false;
  if (dtype == DCTN_F64) return false;
  if (dtype == DCTN_F32 && precision != DCTN_PREC_BF16) return false;
  if (p.N != 8 && p.N != 9) return false;
  const long long esz = dtype == DCTN_BF16 ? 2 : 4;
  {  // 32-bit byte offsets with the hardware range check: non-negative strides, extents below 2 GiB
    long long ext = 0;
    const long long dims[5] = {p.C, p.B, p.H, p.W, p.Q};
    for (int i = 0; i < 5; ++i) {
      if (p.s[i] < 0) return false;
      ext += (dims[i] - 1) * p.s[i];
    }
    if ((ext + 1) * esz >= (1LL << 31)) return false;
    if (p.Wn * p.O * esz >= (1LL << 31)) return false;
  }
  const int op = next_pow2(p.O);
  return op >= 2 ? op <= 16 : true;
}

FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  if (d <= 1) {
    f.M = 0; f.s1 = 0; f.s2 = 0;
    return f;
  }
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  f.M = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  f.s1 = 1;
  f.s2 = l - 1;
  return f;
}

void fill_mp(MfmaP& m, const EpsP& p, const void* x, int dtype) {
  const long long esz = dtype == DCTN_BF16 ? 2 : 4;
  for (int n = 0; n < p.N && n < MFMA_MAXN; ++n) {
    const int pos = n / p.C, ch = n - pos * p.C;
    const int dh = pos / p.K, dw = pos - dh * p.K;
    m.foffb[n] = (unsigned)((ch * p.s[0] + dh * p.s[2] + dw * p.s[3]) * esz);
  }
  m.s1b = (unsigned)(p.s[1] * esz); m.s2b = (unsigned)(p.s[2] * esz);
  m.s3b = (unsigned)(p.s[3] * esz); m.s4b = (unsigned)(p.s[4] * esz);
  long long ext = 0;
  const long long dims[5] = {p.C, p.B, p.H, p.W, p.Q};
  for (int i = 0; i < 5; ++i) ext += (dims[i] - 1) * p.s[i];
  m.x_bytes = (unsigned)((ext + 1) * esz);
  const int rows = p.K * p.C;
  for (int rw = 0; rw < MFMA_MAXN; ++rw) m.rowoffb[rw] = 0;
  for (int rw = 0; rw < rows && rw < MFMA_MAXN; ++rw) {
    const int dh = rw / p.C, ch = rw - dh * p.C;
    m.rowoffb[rw] = (unsigned)((ch * p.s[0] + dh * p.s[2]) * esz);
  }
  // K pixels of a row in one 16-byte load: bf16 pairs (4 bytes per pixel), pixels contiguous
  m.rowvec_ok = dtype == DCTN_BF16 && p.s[4] == 1 && p.s[3] == 2 && p.K <= 4 && rows <= MFMA_MAXN / 2 &&
                ((p.N == 9 && rows == 3) || (p.N == 8 && rows == 4));
  m.div_wo = make_fastdiv((unsigned)p.Wo);
  m.C = p.C; m.B = p.B; m.K = p.K; m.O = p.O; m.Ho = p.Ho; m.Wo = p.Wo;
  m.P = p.Ho * p.Wo;
  m.npg = (m.P + 63) / 64;
  m.npg_rcp = (65536u + (unsigned)m.npg - 1u) / (unsigned)m.npg;   // exact for tickets below 2^16 / npg
  m.spc = 1; m.nchunks = p.B;
  m.o_s1b = (unsigned)((long long)m.P * p.O * esz);
  m.o_bytes = (unsigned)(p.Wn * p.O * esz);
  m.vec_ok = p.s[4] == 1 && p.s[0] % 2 == 0 && p.s[1] % 2 == 0 && p.s[2] % 2 == 0 &&
             p.s[3] % 2 == 0 && ((uintptr_t)x % 4) == 0;
  m.Cout = 0; m.hw_rowb = 0; m.hw_bytes = 0; m.ncb = 0; m.skew = 0;
  m.opts = p.opts;
#ifdef DCTN_STAMPS
  m.stamps = g_stamps;
#endif
}

constexpr int FWD_BLOCKS_PER_CU = 4;

// dynamic LDS of the dCore kernel: the per-wave transposition tiles of its LDST path, else nothing
template <int N0, int N1, int OP>
constexpr size_t dcore_dyn_lds() {
  constexpr int A = 1 << N0, MT = (1 << N1) * OP / 32;
  return (A == 32 && MT <= 2) ? (size_t)BWD_WAVES * (1 + MT) * 64 * LROW * sizeof(short) : 0;
}
#define DCTN_DCORE_LAUNCH(KERNEL, G, B, DYN, ST, ...)                                                  \
  do {                                                                                                 \
    if ((DYN) > 0 && !dctn_lds_optin((const void*)KERNEL, DYN)) return DCTN_ERR_UNSUPPORTED;       \
    hipLaunchKernelGGL(KERNEL, G, B, DYN, ST, __VA_ARGS__);                                            \
  } while (0)

// Split the batch into sample chunks so that (chunks x position groups) is about `target` waves;
// returns the number of workgroups of `wpb` waves (a multiple of 8 for the XCD-contiguous mapping).
int plan_waves(MfmaP& m, int wpb, long long target) {
  long long chunks = target / m.npg;
  if (chunks < 1) chunks = 1;
  if (chunks > m.B) chunks = m.B;
  m.spc = (int)((m.B + chunks - 1) / chunks);
  m.nchunks = (m.B + m.spc - 1) / m.spc;
  const long long waves = (long long)m.nchunks * m.npg;
  long long blocks = (waves + wpb - 1) / wpb;
  if (blocks >= 8) blocks = (blocks + 7) / 8 * 8;
  return (int)blocks;
}

// vector row accesses of out / dY: O already a power of two and a dword-aligned base
template <typename S>
bool row_vec_ok(const MfmaP& m, int OP, const void* ptr) {
  return m.O == OP && ((uintptr_t)ptr % 4) == 0 && (OP * sizeof(S)) % 4 == 0;
}

template <typename S, int N0, int N1, int OP>
int fwd_launch_t(const void* x, const void* core, void* out, double* stats, const MfmaP& m_in, hipStream_t st) {
  MfmaP m = m_in;
  const int blocks = plan_waves(m, 4, (long long)FWD_BLOCKS_PER_CU * dctn_dev().cus * 4);
  const bool ovec = out == nullptr || row_vec_ok<S>(m, OP, out);
  const dim3 g((unsigned)blocks), b(256);
  constexpr int NN = N0 + N1;
  constexpr int RW = NN == 9 ? 3 : 4;   // K*C window rows: 3x3 single channel, 2x2 two channels
  if (m.rowvec_ok && m.vec_ok && ovec && sizeof(S) == 2)
    hipLaunchKernelGGL((eps_fwd_q2reg_k<S, N0, N1, OP, true, true, RW>), g, b, 0, st, (const S*)x,
                       (const S*)core, (S*)out, stats, m);
  else if (m.vec_ok && ovec)
    hipLaunchKernelGGL((eps_fwd_q2reg_k<S, N0, N1, OP, true, true, 0>), g, b, 0, st, (const S*)x,
                       (const S*)core, (S*)out, stats, m);
  else if (m.vec_ok)
    hipLaunchKernelGGL((eps_fwd_q2reg_k<S, N0, N1, OP, true, false, 0>), g, b, 0, st, (const S*)x,
                       (const S*)core, (S*)out, stats, m);
  else
    hipLaunchKernelGGL((eps_fwd_q2reg_k<S, N0, N1, OP, false, false, 0>), g, b, 0, st, (const S*)x,
                       (const S*)core, (S*)out, stats, m);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel("eps_fwd_mfma_q2reg");
  return DCTN_OK;
}

template <typename S, int N0, int N1, int OP>
int bwd_launch_t(const void* x, const void* dY, void* dCore, void* ws, const MfmaP& m_in,
                 hipStream_t st) {
  constexpr int A = 1 << N0, BN = 1 << N1, AT = A >= 32 ? A / 32 : 1;
  constexpr size_t DYN = dcore_dyn_lds<N0, N1, OP>();
  MfmaP m = m_in;
  const int grid = plan_waves(m, BWD_WAVES, (long long)dctn_dev().cus * BWD_WAVES);   // <= one partial tile per CU
  const bool ovec = row_vec_ok<S>(m, OP, dY);
  const dim3 g(grid), b(64 * BWD_WAVES);
  constexpr int NN = N0 + N1;
  constexpr int RW = NN == 9 ? 3 : 4;
  if (m.rowvec_ok && m.vec_ok && ovec && sizeof(S) == 2)
    DCTN_DCORE_LAUNCH((eps_bwd_dcore_q2reg_k<S, N0, N1, OP, true, true, RW, 0>), g, b, DYN, st,
                       (const S*)x, (const S*)dY, (const S*)nullptr, (const S*)nullptr, (float*)ws, (float*)nullptr, m, (S*)nullptr, 0);
  else if (m.vec_ok && ovec)
    DCTN_DCORE_LAUNCH((eps_bwd_dcore_q2reg_k<S, N0, N1, OP, true, true, 0, 0>), g, b, DYN, st,
                       (const S*)x, (const S*)dY, (const S*)nullptr, (const S*)nullptr, (float*)ws, (float*)nullptr, m, (S*)nullptr, 0);
  else if (m.vec_ok)
    DCTN_DCORE_LAUNCH((eps_bwd_dcore_q2reg_k<S, N0, N1, OP, true, false, 0, 0>), g, b, DYN, st,
                       (const S*)x, (const S*)dY, (const S*)nullptr, (const S*)nullptr, (float*)ws, (float*)nullptr, m, (S*)nullptr, 0);
  else
    DCTN_DCORE_LAUNCH((eps_bwd_dcore_q2reg_k<S, N0, N1, OP, false, false, 0, 0>), g, b, DYN, st,
                       (const S*)x, (const S*)dY, (const S*)nullptr, (const S*)nullptr, (float*)ws, (float*)nullptr, m, (S*)nullptr, 0);
  DCTN_CHECK_LAUNCH();
  if (m.opts & DCTN_OPT_MAIN_KERNEL_ONLY) return DCTN_PARTIAL;   // measurement option: partial sums only, gradients NOT written
  hipLaunchKernelGGL((eps_bwd_dcore_reduce_k<S>), dim3(BN * OP * AT), dim3(256), 0, st,
                     (const float*)ws, (S*)dCore, grid, A, BN, m.O, OP, AT * 32);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel("eps_bwd_mfma_q2reg");
  return DCTN_OK;
}

// Uneven split of a chunk block's samples over its waves (wave_job): n_old = spc + k for waves 0-3, n_young = spc - k
// for waves 4-7.  The two dCore waves of a SIMD do not share it evenly: the older one (waves 0-3) wins the arbitration
// and ran its spc samples in 8.4 us where the younger one needed 10.7 (per-wave stamps, B = 1024), so the older takes
// more.  k = spc / 3 is the measured choice (spc = 6: k = 2 of 0 .. 5; spc = 23: k = 7 of 0, 4, 7, 11);
// the macro is the build-time switch of that comparison.
#ifndef DCTN_DCORE_SKEW
#define DCTN_DCORE_SKEW(spc) ((spc) / 3)
#endif

// grouped wave mapping of the fused head backward: ncb chunk blocks x npg position groups workgroups
// (<= the CU count: one dCore partial tile per workgroup), 8 sample chunks per chunk block
int plan_grouped(MfmaP& m) {
  if (m.npg > dctn_dev().cus) return 0;
  long long ncb = dctn_dev().cus / m.npg;
  const long long need = (m.B + BWD_WAVES - 1) / BWD_WAVES;
  if (ncb > need) ncb = need;
  m.spc = (int)((m.B + ncb * BWD_WAVES - 1) / (ncb * BWD_WAVES));
  m.nchunks = (m.B + m.spc - 1) / m.spc;
  m.ncb = (m.nchunks + BWD_WAVES - 1) / BWD_WAVES;
  long long blocks = (long long)m.ncb * m.npg;
  if (blocks >= 8) blocks = (blocks + 7) / 8 * 8;
  return blocks <= dctn_dev().cus ? (int)blocks : 0;
}

size_t head_dw_partial_bytes(const EpsP& p, int Cout) {
  const long long P = (long long)p.Ho * p.Wo, npg = (P + 63) / 64;
  if (npg > dctn_dev().cus) return 0;
  return (size_t)(dctn_dev().cus / npg) * ((size_t)Cout * (size_t)(P * p.O) + 16) * sizeof(float);
}

// DCTN_OPT_HEAD_FEATURES_BLOCKED4 is honoured exactly where the fused backward takes its HEADMM path (`headmm` in
// bwd_head_launch_t: the dCore kernel reads no features, eps_head_reduce_k's gemm role reads them all), the forward
// runs eps_fwd_head_q2reg_t_k (the only writer of the layout; not under DCTN_OPT_SMALL_CHUNKS) and the padded buffer
// stays inside a 32-bit buffer descriptor.  Both directions decline the same requests.
// bytes of the blocked4 feature buffer: ceil(B / 4) blocks of [F][4] bf16
long long blocked4_bytes(const MfmaP& m) { return (long long)(m.B + 3) / 4 * 4 * m.P * m.O * 2; }
template <int N0, int N1, int OP>
bool head_blocked4_ok(const MfmaP& m) {
  constexpr int A = 1 << N0, MT = (1 << N1) * OP / 32;
  const long long F = (long long)m.P * OP;
  return A == 32 && MT <= 2 && OP == 4 && m.vec_ok && blocked4_bytes(m) < (1LL << 31) && !(m.opts & DCTN_OPT_SMALL_CHUNKS) &&
         F % 8 == 0 && F <= (long long)HEADT_WAVES * HEADT_MAXKS * 32;
}

// fused classifier-head backward (bf16 only): dLogits (B, Cout), head weight (Cout, P*O), feat (B, P*O)
template <int N0, int N1, int OP>
int bwd_head_launch_t(const void* x, const void* dL, const void* hw, const void* feat, void* dCore, void* dW,
                      void* dBias, void* ws, size_t core_ws_bytes, const MfmaP& m_in, hipStream_t st) {
  typedef bf16_t S;
  constexpr int A = 1 << N0, BN = 1 << N1, AT = A >= 32 ? A / 32 : 1;
  constexpr size_t DYN = dcore_dyn_lds<N0, N1, OP>();
  MfmaP m = m_in;
  const bool blk = (m.opts & DCTN_OPT_HEAD_FEATURES_BLOCKED4) != 0;
  if (m.O != OP || m.Cout < 2 || m.Cout > 16 || m.Cout % 2 != 0) return DCTN_ERR_UNSUPPORTED;
  if (((uintptr_t)dL % 4) != 0 || ((uintptr_t)hw % 4) != 0 || ((uintptr_t)feat % (blk ? 16 : 4)) != 0) return DCTN_ERR_UNSUPPORTED;
  if (blk && !head_blocked4_ok<N0, N1, OP>(m)) return DCTN_ERR_UNSUPPORTED;   // (before any launch)
  const int grid = plan_grouped(m);
  if (grid == 0) return DCTN_ERR_UNSUPPORTED;
  float* dwpart = reinterpret_cast<float*>(static_cast<unsigned char*>(ws) + core_ws_bytes);
  const long long nW = (long long)m.Cout * m.P * OP;   // dwpart: [ncb][Cout][P*O]
  // the condition under which the kernel below takes its HEADMM path and leaves dW to eps_head_reduce_k's gemm role
  constexpr int MT = BN * OP / 32;
  // `headmm` is exactly the kernel's compile-time HEADMM condition for the instantiations launched below (XVEC = m.vec_ok,
  // OVEC = true, bf16); such a kernel forms no dW, so the finishing kernel MUST take its gemm role, which addresses the
  // features through a 32-bit buffer descriptor: a batch beyond that range is declined here (family_ok already bounds
  // B * P * O * 2 below 2^31, so the two conditions cannot disagree - stated once, for both)
  const bool headmm = A == 32 && MT <= 2 && OP == 4 && m.vec_ok;
  if (headmm && (long long)m.B * m.P * OP * 2 >= (1LL << 31)) return DCTN_ERR_UNSUPPORTED;
  const bool gemm = headmm;
  // the HEADMM kernels index nothing by sample chunk: their waves may take uneven runs of a block's samples
  m.skew = headmm ? DCTN_DCORE_SKEW(m.spc) : 0;
  if (m.skew >= m.spc) m.skew = m.spc - 1;

  const dim3 g(grid), b(64 * BWD_WAVES);
  constexpr int NN = N0 + N1;
  constexpr int RW = NN == 9 ? 3 : 4;
  // blocked4 features: dW is formed by DWR_WAVES more waves of the dCore workgroups (head_dw_role_waves), whose tiles
  // take DWR_LDS_BYTES more of dynamic LDS; where that opt-in is refused the finishing kernel's gemm role forms dW
  const int n_slices = (int)(((long long)m.P * OP + DWG_BFW - 1) / DWG_BFW);
  bool dwrole = false;
  if constexpr (A == 32 && MT <= 2 && OP == 4) {
    constexpr size_t RDYN = DYN + 8192 + DWR_LDS_BYTES;
#define DCTN_HEAD_ROLE_LAUNCH(ROWSV, HC)                                                                          \
  do {                                                                                                            \
    const void* kfn = (const void*)eps_bwd_dcore_q2reg_k<S, N0, N1, OP, true, true, ROWSV, HC, DWR_WAVES>;        \
    if (dctn_lds_optin(kfn, RDYN)) {                                                                              \
      hipLaunchKernelGGL((eps_bwd_dcore_q2reg_k<S, N0, N1, OP, true, true, ROWSV, HC, DWR_WAVES>), g,             \
                         dim3(64 * (BWD_WAVES + DWR_WAVES)), RDYN, st, (const S*)x, (const S*)dL, (const S*)hw,   \
                         (const S*)feat, (float*)ws, dwpart, m, (S*)dW, dW ? n_slices : 0);                       \
      dwrole = true;                                                                                              \
    }                                                                                                             \
  } while (0)
    if (blk && headmm) {
      if (m.rowvec_ok) {
        if (m.Cout <= 10) DCTN_HEAD_ROLE_LAUNCH(RW, 10); else DCTN_HEAD_ROLE_LAUNCH(RW, 16);
      } else {
        if (m.Cout <= 10) DCTN_HEAD_ROLE_LAUNCH(0, 10); else DCTN_HEAD_ROLE_LAUNCH(0, 16);
      }
    }
#undef DCTN_HEAD_ROLE_LAUNCH
  }
#define DCTN_HEAD_LAUNCH(XV, ROWSV, HC)                                                                        \
  DCTN_DCORE_LAUNCH((eps_bwd_dcore_q2reg_k<S, N0, N1, OP, XV, true, ROWSV, HC>), g, b, (DYN > 0 ? DYN + 8192 : 0), st, (const S*)x, \
                     (const S*)dL, (const S*)hw, (const S*)feat, (float*)ws, dwpart, m, (S*)nullptr, 0)
  if (dwrole) {   // (launched above)
  } else if (m.rowvec_ok && m.vec_ok) {
    if (m.Cout <= 10) DCTN_HEAD_LAUNCH(true, RW, 10); else DCTN_HEAD_LAUNCH(true, RW, 16);
  } else if (m.vec_ok) {
    if (m.Cout <= 10) DCTN_HEAD_LAUNCH(true, 0, 10); else DCTN_HEAD_LAUNCH(true, 0, 16);
  } else {
    if (m.Cout <= 10) DCTN_HEAD_LAUNCH(false, 0, 10); else DCTN_HEAD_LAUNCH(false, 0, 16);
  }
#undef DCTN_HEAD_LAUNCH
  DCTN_CHECK_LAUNCH();
  if (m.opts & DCTN_OPT_MAIN_KERNEL_ONLY) return DCTN_PARTIAL;   // measurement option: partial sums only, gradients NOT written
  const int fw = blk ? DWG_BFW : DWG_FW;   // features of a gemm workgroup's slice
  const int n_core = BN * OP * AT;
  if (dwrole) {   // dW is written: the finishing kernel keeps its dCore and dBias roles (no LDS opt-in)
    hipLaunchKernelGGL(eps_head_reduce_k, dim3(n_core + 1), dim3(1024), 0, st, (const float*)ws, (S*)dCore, grid, A, BN, m.O, OP,
                       AT * 32, n_core, (const float*)dwpart, (S*)nullptr, m.ncb, nW, 0, (const S*)dL, (S*)dBias, m.B, m.Cout,
                       (const S*)feat, 0);
    DCTN_CHECK_LAUNCH();
    dctn_set_last_kernel("eps_head_bwd_mfma_q2reg");
    return DCTN_OK;
  }
  const int n_dw = gemm ? (int)(((long long)m.P * OP + fw - 1) / fw) : (int)((nW + 255) / 256);
  const size_t gemm_lds = (size_t)DWG_WAVES * (fw / 4) * 64 * sizeof(float);
  static_assert(DWG_WAVES * 64 == 1024, "the gemm role is the whole workgroup of eps_head_reduce_k");
  if (gemm && !dctn_lds_optin((const void*)eps_head_reduce_k, gemm_lds)) return DCTN_ERR_LAUNCH;   // (after the main kernel)
  hipLaunchKernelGGL(eps_head_reduce_k, dim3(n_core + n_dw + 1), dim3(1024), gemm ? gemm_lds : 0, st, (const float*)ws, (S*)dCore,
                     grid, A, BN, m.O, OP, AT * 32, n_core, (const float*)dwpart, (S*)dW, m.ncb, nW, n_dw,
                     (const S*)dL, (S*)dBias, m.B, m.Cout, (const S*)feat, gemm ? (blk ? 2 : 1) : 0);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel("eps_head_bwd_mfma_q2reg");
  return DCTN_OK;
}

// forward of (EPS layer -> flatten -> linear head) as one kernel (bf16, fast input layout only)
template <int N0, int N1, int OP>
int fwd_head_launch_t(const void* x, const void* core, const void* hw, const void* bias, void* out, void* logits,
                      const MfmaP& m_in, hipStream_t st) {
  typedef bf16_t S;
  MfmaP m = m_in;
  const bool blk = (m.opts & DCTN_OPT_HEAD_FEATURES_BLOCKED4) != 0;
  if (m.O != OP || !(m.rowvec_ok && m.vec_ok) || m.npg > HEAD_FWD_MAXPG) return DCTN_ERR_UNSUPPORTED;
  // 16-byte weight fragments, (OP * 2)-byte feature rows (blocked4: 16-byte stores)
  if (((uintptr_t)hw % 16) != 0 || m.hw_rowb % 16 != 0 || ((uintptr_t)out % (blk ? 16 : OP * 2)) != 0) return DCTN_ERR_UNSUPPORTED;
  int nwg = m.B < dctn_dev().cus ? m.B : dctn_dev().cus;
  m.spc = (m.B + nwg - 1) / nwg;
  if (blk) m.spc = (m.spc + HEADT_GS - 1) / HEADT_GS * HEADT_GS;   // groups = absolute 4-sample blocks
  nwg = (m.B + m.spc - 1) / m.spc;
  constexpr int RW = (N0 + N1) == 9 ? 3 : 4;
  const long long F = (long long)m.P * OP;
  const bool tk = !(m.opts & DCTN_OPT_SMALL_CHUNKS) && F % 8 == 0 && F <= (long long)HEADT_WAVES * HEADT_MAXKS * 32;
  if (blk) {   // only the kernel below writes blocked4, only for the shapes whose backward reads it (head_blocked4_ok)
    if (!tk || !head_blocked4_ok<N0, N1, OP>(m)) return DCTN_ERR_UNSUPPORTED;
    m.o_bytes = blocked4_bytes(m);
  }
  if (tk) {
    // steps pulled from a counter by 16 waves, head as a tail phase (DCTN_OPT_SMALL_CHUNKS keeps the round-4 structure:
    // a wave per position group, for same-box comparisons)
    const size_t dyn = (size_t)HEADT_GS * headt_pitch((int)F) * sizeof(short);
#define DCTN_HEADT_LAUNCH(BLK)                                                                                          \
    if (!dctn_lds_optin((const void*)eps_fwd_head_q2reg_t_k<N0, N1, OP, RW, BLK>, dyn)) return DCTN_ERR_UNSUPPORTED;    \
    hipLaunchKernelGGL((eps_fwd_head_q2reg_t_k<N0, N1, OP, RW, BLK>), dim3((unsigned)nwg), dim3(64 * HEADT_WAVES), dyn, st, \
                       (const S*)x, (const S*)core, (const S*)hw, (const S*)bias, (S*)out, (S*)logits, m)
    if (blk) { DCTN_HEADT_LAUNCH(true); } else { DCTN_HEADT_LAUNCH(false); }
#undef DCTN_HEADT_LAUNCH
    DCTN_CHECK_LAUNCH();
    dctn_set_last_kernel("eps_head_fwd_mfma_q2reg");
    return DCTN_OK;
  }
  const dim3 g((unsigned)nwg), b((unsigned)(64 * m.npg));
  hipLaunchKernelGGL((eps_fwd_head_q2reg_k<N0, N1, OP, RW>), g, b, 0, st, (const S*)x, (const S*)core, (const S*)hw,
                     (const S*)bias, (S*)out, (S*)logits, m);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel("eps_head_fwd_mfma_q2reg");
  return DCTN_OK;
}

#define DISPATCH_OP(FN, S, N0, N1, OPV, ...)                         \
  switch (OPV) {                                                     \
    case 2: return FN<S, N0, N1, 2>(__VA_ARGS__);                    \
    case 4: return FN<S, N0, N1, 4>(__VA_ARGS__);                    \
    case 8: return FN<S, N0, N1, 8>(__VA_ARGS__);                    \
    case 16: return FN<S, N0, N1, 16>(__VA_ARGS__);                  \
  }                                                                  \
  return DCTN_ERR_UNSUPPORTED;

template <typename S>
int fwd_dispatch(const void* x, const void* core, void* out, double* stats, const MfmaP& m, int N, int op,
                 hipStream_t st) {
  if (N == 9) { DISPATCH_OP(fwd_launch_t, S, 5, 4, op, x, core, out, stats, m, st) }
  DISPATCH_OP(fwd_launch_t, S, 4, 4, op, x, core, out, stats, m, st)
}

template <typename S>
int bwd_dispatch(const void* x, const void* dY, void* dCore, void* ws, const MfmaP& m, int N,
                 int op, hipStream_t st) {
  if (N == 9) { DISPATCH_OP(bwd_launch_t, S, 5, 4, op, x, dY, dCore, ws, m, st) }
  DISPATCH_OP(bwd_launch_t, S, 4, 4, op, x, dY, dCore, ws, m, st)
}

}  // namespace

int eps_fwd_mfma(const void* x, const void* core, void* out, const EpsP& p, int dtype,
                 int precision, hipStream_t st, double* stats) {
  if (!family_ok(p, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  if (!out && !stats) return DCTN_ERR_NULL;
  MfmaP m;
  fill_mp(m, p, x, dtype);
  const int op = next_pow2(p.O) < 2 ? 2 : next_pow2(p.O);
  if (dtype == DCTN_BF16) return fwd_dispatch<bf16_t>(x, core, out, stats, m, p.N, op, st);
  return fwd_dispatch<float>(x, core, out, stats, m, p.N, op, st);
}

size_t eps_bwd_mfma_workspace(const EpsP& p, int dtype, int precision, int need_dx,
                              int need_dcore) {
  (void)need_dx;
  if (!need_dcore || !family_ok(p, dtype, precision)) return 0;
  const int op = next_pow2(p.O) < 2 ? 2 : next_pow2(p.O);
  const int n0 = (p.N + 1) / 2, n1 = p.N - n0;
  const long long A = 1LL << n0, BN = 1LL << n1, acols = A >= 32 ? A : 32;
  return (size_t)dctn_dev().cus * (size_t)(BN * op) * (size_t)acols * sizeof(float);
}

// dCore only; the caller (capi) sends dX to the generic kernels.
int eps_bwd_mfma(const void* x, const void* core, const void* dY, void* dX, void* dCore, void* ws,
                 size_t ws_bytes, const EpsP& p, int dtype, int precision, hipStream_t st) {
  (void)core;
  if (dX || !dCore) return DCTN_ERR_UNSUPPORTED;
  if (!family_ok(p, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < eps_bwd_mfma_workspace(p, dtype, precision, 0, 1)) return DCTN_ERR_WORKSPACE;
  MfmaP m;
  fill_mp(m, p, x, dtype);
  const int op = next_pow2(p.O) < 2 ? 2 : next_pow2(p.O);
  if (dtype == DCTN_BF16) return bwd_dispatch<bf16_t>(x, dY, dCore, ws, m, p.N, op, st);
  return bwd_dispatch<float>(x, dY, dCore, ws, m, p.N, op, st);
}

// Backward of (EPS layer -> flatten -> linear head) in one pass over x: dCore, dW and dBias from
// dLogits, the head weight and the layer's forward output; dY is never materialised (see
// eps_bwd_dcore_q2reg_k).
static bool head_family_ok(const EpsP& p, int Cout, int dtype, int precision) {
  if (dtype != DCTN_BF16 || !family_ok(p, dtype, precision)) return false;
  const int op = next_pow2(p.O) < 2 ? 2 : next_pow2(p.O);
  if (op != p.O || op > 4) return false;   // the weight slice and its gradient live in registers
  if (Cout < 2 || Cout > 16 || Cout % 2 != 0) return false;
  const long long P = (long long)p.Ho * p.Wo;
  if ((P + 63) / 64 > dctn_dev().cus) return false;
  return P * p.O * 2 * Cout < (1LL << 31);
}

size_t eps_head_bwd_mfma_workspace(const EpsP& p, int Cout, int dtype, int precision) {
  if (!head_family_ok(p, Cout, dtype, precision)) return 0;
  const size_t a = (eps_bwd_mfma_workspace(p, dtype, precision, 0, 1) + 255) / 256 * 256;
  return a + head_dw_partial_bytes(p, Cout);
}

int eps_head_bwd_mfma(const void* x, const void* feat, const void* dLogits, const void* head_w, void* dCore,
                      void* dW, void* dBias, void* ws, size_t ws_bytes, const EpsP& p, int Cout, int dtype,
                      int precision, hipStream_t st) {
  if (!dCore) return DCTN_ERR_UNSUPPORTED;
  if (!head_family_ok(p, Cout, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < eps_head_bwd_mfma_workspace(p, Cout, dtype, precision)) return DCTN_ERR_WORKSPACE;
  const size_t core_ws = (eps_bwd_mfma_workspace(p, dtype, precision, 0, 1) + 255) / 256 * 256;
  MfmaP m;
  fill_mp(m, p, x, dtype);
  m.Cout = Cout;
  const long long rowb = (long long)m.P * p.O * 2;
  m.hw_rowb = (unsigned)rowb;
  m.hw_bytes = (unsigned)(rowb * Cout);
  if (p.N == 9) {
    if (p.O == 2) return bwd_head_launch_t<5, 4, 2>(x, dLogits, head_w, feat, dCore, dW, dBias, ws, core_ws, m, st);
    return bwd_head_launch_t<5, 4, 4>(x, dLogits, head_w, feat, dCore, dW, dBias, ws, core_ws, m, st);
  }
  if (p.O == 2) return bwd_head_launch_t<4, 4, 2>(x, dLogits, head_w, feat, dCore, dW, dBias, ws, core_ws, m, st);
  return bwd_head_launch_t<4, 4, 4>(x, dLogits, head_w, feat, dCore, dW, dBias, ws, core_ws, m, st);
}

// Forward of the same tail: features (stored, the backward needs them) and logits from one kernel.
int eps_head_fwd_mfma(const void* x, const void* core, const void* head_w, const void* bias, void* feat, void* logits,
                      const EpsP& p, int Cout, int dtype, int precision, hipStream_t st) {
  if (!head_family_ok(p, Cout, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  MfmaP m;
  fill_mp(m, p, x, dtype);
  m.Cout = Cout;
  const long long rowb = (long long)m.P * p.O * 2;
  m.hw_rowb = (unsigned)rowb;
  m.hw_bytes = (unsigned)(rowb * Cout);
  if (p.N == 9) {
    if (p.O == 2) return fwd_head_launch_t<5, 4, 2>(x, core, head_w, bias, feat, logits, m, st);
    return fwd_head_launch_t<5, 4, 4>(x, core, head_w, bias, feat, logits, m, st);
  }
  if (p.O == 2) return fwd_head_launch_t<4, 4, 2>(x, core, head_w, bias, feat, logits, m, st);
  return fwd_head_launch_t<4, 4, 4>(x, core, head_w, bias, feat, logits, m, st);
}

bool eps_mfma_covers(const EpsP& p, int dtype, int precision) { return family_ok(p, dtype, precision); }
