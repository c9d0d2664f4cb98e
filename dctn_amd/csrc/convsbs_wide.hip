// Wide ConvSBS backward: strings whose core gradients do not fit one workgroup's LDS (the generic sweep keeps the dCore
// accumulators of the whole string there and declines above dctn_lds_wg_max() / 2).  float32, float64, bf16 storage
// (float32 arithmetic), open chains and rings, any core order, outputs on any cores, q^C <= 4096.
//
// Nothing of a core's gradient lives in LDS: every step is a GEMM or a per-window contraction over HBM buffers of one
// chunk of windows (the chunk bounds the workspace), and the dCore GEMM leaves per-split partial records that one
// reduction kernel sums in a fixed order.  No float atomics: two identical calls give bit-identical dX and dCores.
//
// Per pass s of the traced bond (one pass for an open chain) and per chunk of windows w:
//   F_c(w)[k]              pixel features of core c                                 (wide_feat_k)
//   T_c(w)[o,l,r]        = sum_k F_c(w)[k] core_c[o,l,r,k]                          (GEMM  M = windows, N = o l r, K = q^C)
//   V_{c+1}(w)[(a,o),r]  = sum_l V_c(w)[a,l] T_c(w)[o,l,r]       forward sweep      (wide_fwd_step_k)
//   adjoint, right to left, G_c = d/d(output state of core c), G_{n-1} = dY (x) e_s:
//   G_{c-1}(w)[a,l]      = sum_{o,r} G_c(w)[(a,o),r] T_c(w)[o,l,r]                   (wide_bwd_state_k)
//   dT_c(w)[o,l,r]       = sum_a V_c(w)[a,l] G_c(w)[(a,o),r]                         (wide_dt_k)
//   dCore_c[o,l,r,k]    += sum_w dT_c(w)[o,l,r] F_c(w)[k]                            (GEMM  M = o l r, N = q^C, K = windows)
//   df_c(w)[k]           = sum_{o,l,r} dT_c(w)[o,l,r] core_c[o,l,r,k]                (GEMM  M = windows, N = q^C, K = o l r)
//   df_c -> the per-window input gradients gxw of the generic sweep's layout         (wide_gxw_k; dX by its gather kernel)
// The GEMMs run on v_mfma_f32_16x16x4_f32 (exact float32) and as FMA on the vector ALU for float64.
#include <type_traits>

#include "common.h"

namespace {

constexpr int WIDE_MAXC = 32;
constexpr size_t WIDE_CHUNK_BYTES = (size_t)512 << 20;   // per-chunk buffers (states, T / dT, gradients of the states)
constexpr int WIDE_MAX_SPLITS = 64;                      // partial records of one core's dCore GEMM

typedef __attribute__((ext_vector_type(4))) float wd_f4;

struct WideP {
  int n, C, B, H, W, q, qc, Ho, Wo, l0, Otot;
  long long Wn;
  long long s[5];
  int o[WIDE_MAXC], bl[WIDE_MAXC], br[WIDE_MAXC], ph[WIDE_MAXC], pw[WIDE_MAXC];
  int oacc[WIDE_MAXC + 1];
  long long st_off[WIDE_MAXC + 1];   // per-window element offsets of the states V_c in a chunk's state buffer
  long long emax;                    // largest o l r
  long long gmax;                    // largest gradient of a state: max over c of oacc[c+1] * br[c] and oacc[c] * bl[c]
  long long cemax, cetot;            // largest core, all cores (elements)
};

// the chunk plan and the workspace layout (bytes from the start of the workspace)
struct WideLayout {
  long long wc;   // windows per chunk
  int splits;     // partial records per dCore GEMM
  size_t gxw, acc, part, v, f, t, g0, g1, df, total;
};

int wide_fill(WideP& p, const SbsShape& sh) {
  if (sh.n < 1 || sh.n > WIDE_MAXC || sh.C < 1 || sh.B < 1 || sh.q < 1) return DCTN_ERR_UNSUPPORTED;
  int max_h = 0, max_w = 0;
  for (int c = 0; c < sh.n; ++c) {
    if (sh.out_sizes[c] < 1 || sh.bond_sizes[c] < 1 || sh.pos_h[c] < 0 || sh.pos_w[c] < 0) return DCTN_ERR_BAD_SHAPE;
    max_h = sh.pos_h[c] > max_h ? sh.pos_h[c] : max_h;
    max_w = sh.pos_w[c] > max_w ? sh.pos_w[c] : max_w;
  }
  if (sh.H <= max_h || sh.W <= max_w) return DCTN_ERR_BAD_SHAPE;
  p.n = sh.n; p.C = sh.C; p.B = sh.B; p.H = sh.H; p.W = sh.W; p.q = sh.q;
  long long qc = 1;
  for (int c = 0; c < sh.C; ++c) { qc *= sh.q; if (qc > 4096) return DCTN_ERR_UNSUPPORTED; }
  p.qc = (int)qc;
  p.Ho = sh.H - max_h; p.Wo = sh.W - max_w;
  p.Wn = (long long)sh.B * p.Ho * p.Wo;
  p.l0 = sh.bond_sizes[0];
  long long oacc = 1, off = 0;
  p.emax = p.gmax = p.cemax = p.cetot = 0;
  for (int c = 0; c < sh.n; ++c) {
    p.o[c] = sh.out_sizes[c];
    p.bl[c] = sh.bond_sizes[c];
    p.br[c] = sh.bond_sizes[(c + 1) % sh.n];
    p.ph[c] = sh.pos_h[c];
    p.pw[c] = sh.pos_w[c];
    p.oacc[c] = (int)oacc;
    p.st_off[c] = off;
    const long long gin = oacc * p.bl[c];
    off += gin;
    oacc *= sh.out_sizes[c];
    const long long gout = oacc * p.br[c];
    if (gout > (1 << 20)) return DCTN_ERR_UNSUPPORTED;   // (fill()'s limits)
    const long long e = (long long)p.o[c] * p.bl[c] * p.br[c];
    if (e * p.qc > (1 << 20)) return DCTN_ERR_UNSUPPORTED;
    p.emax = e > p.emax ? e : p.emax;
    p.gmax = gin > p.gmax ? gin : p.gmax;
    p.gmax = gout > p.gmax ? gout : p.gmax;
    p.cemax = e * p.qc > p.cemax ? e * p.qc : p.cemax;
    p.cetot += e * p.qc;
  }
  p.oacc[sh.n] = (int)oacc;
  p.st_off[sh.n] = off;
  p.Otot = (int)oacc;
  return DCTN_OK;
}

WideLayout wide_layout(const WideP& p, int dtype) {
  const size_t asz = acc_size(dtype);
  WideLayout L;
  // per window of a chunk: the states of every core, features, T / dT, two state gradients, feature gradients
  const size_t per_win = ((size_t)p.st_off[p.n] + 2 * (size_t)p.qc + (size_t)p.emax + 2 * (size_t)p.gmax) * asz;
  long long wc = (long long)(WIDE_CHUNK_BYTES / per_win) & ~63LL;
  if (wc < 256) wc = 256;
  if (wc > (1 << 20)) wc = 1 << 20;   // (GEMM grids: at most 16384 row tiles)
  const long long wall = (p.Wn + 63) & ~63LL;
  L.wc = wc < wall ? wc : wall;
  // the dCore GEMM's K (windows of a chunk) is split in pieces of at least 512 windows
  long long sp = (L.wc + 511) / 512;
  L.splits = (int)(sp < WIDE_MAX_SPLITS ? sp : WIDE_MAX_SPLITS);
  size_t off = 0;
  L.gxw = off; off += align256((size_t)p.n * p.C * p.q * p.Wn * asz);
  L.acc = off; if (dtype == DCTN_BF16) off += align256((size_t)p.cetot * sizeof(float));
  L.part = off; off += align256((size_t)L.splits * p.cemax * asz);
  L.v = off; off += align256((size_t)p.st_off[p.n] * L.wc * asz);
  L.f = off; off += align256((size_t)p.qc * L.wc * asz);
  L.t = off; off += align256((size_t)p.emax * L.wc * asz);
  L.g0 = off; off += align256((size_t)p.gmax * L.wc * asz);
  L.g1 = off; off += align256((size_t)p.gmax * L.wc * asz);
  L.df = off; off += align256((size_t)p.qc * L.wc * asz);
  L.total = off;
  return L;
}

unsigned wd_grid(long long total) {
  const long long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

// ---------------------------------------------------------------------------------------------------- per-window kernels
// F[wl][k] = prod_ch x[ch][pixel of core c in window w0 + wl][digit_ch(k)], channel 0 most significant
template <typename S, typename A>
__global__ __launch_bounds__(256) void wide_feat_k(const S* __restrict__ x, WideP p, int c, long long w0, int wcur,
                                                   A* __restrict__ F) {
  const long long total = (long long)wcur * p.qc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % p.qc);
    const long long w = w0 + i / p.qc;
    const int hw = p.Ho * p.Wo;
    const long long b = w / hw;
    const int rem = (int)(w - b * hw);
    const int ho = rem / p.Wo, wo = rem - (rem / p.Wo) * p.Wo;
    const long long base = b * p.s[1] + (long long)(ho + p.ph[c]) * p.s[2] + (long long)(wo + p.pw[c]) * p.s[3];
    A pr = A(1);
    int t = k;
    for (int ch = p.C - 1; ch >= 0; --ch) {
      const int dg = t % p.q;
      t /= p.q;
      pr *= (A)x[ch * p.s[0] + base + dg * p.s[4]];
    }
    F[i] = pr;
  }
}

// the state in front of core 0 in pass s: e_s (one row: no outputs before core 0)
template <typename A>
__global__ __launch_bounds__(256) void wide_state0_k(A* __restrict__ v, int wcur, int l0, int s) {
  const long long total = (long long)wcur * l0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    v[i] = (i % l0) == s ? A(1) : A(0);
}

// vn[wl][(a oc + o) R + r] = sum_l v[wl][a L + l] T[wl][(o L + l) R + r]
template <typename A>
__global__ __launch_bounds__(256) void wide_fwd_step_k(const A* __restrict__ v, const A* __restrict__ T, A* __restrict__ vn,
                                                       int wcur, int Oacc, int oc, int L, int R) {
  const long long per = (long long)Oacc * oc * R, total = (long long)wcur * per;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long wl = i / per;
    const int e = (int)(i - wl * per);
    const int r = e % R, ao = e / R, o = ao % oc, a = ao / oc;
    const A* vp = v + wl * ((long long)Oacc * L) + (long long)a * L;
    const A* tp = T + wl * ((long long)oc * L * R) + (long long)o * L * R + r;
    A acc = A(0);
    for (int l = 0; l < L; ++l) acc += vp[l] * tp[(long long)l * R];
    vn[i] = acc;
  }
}

// gradient of the last output state in pass s: g[wl][a l0 + r] = (r == s) dY[w][a]
template <typename S, typename A>
__global__ __launch_bounds__(256) void wide_grad0_k(const S* __restrict__ dY, A* __restrict__ g, long long w0, int wcur,
                                                    int Otot, int l0, int s) {
  const long long per = (long long)Otot * l0, total = (long long)wcur * per;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long wl = i / per;
    const int e = (int)(i - wl * per);
    const int r = e % l0, a = e / l0;
    g[i] = r == s ? (A)dY[(w0 + wl) * Otot + a] : A(0);
  }
}

// gn[wl][a L + l] = sum_{o,r} g[wl][(a oc + o) R + r] T[wl][(o L + l) R + r]
template <typename A>
__global__ __launch_bounds__(256) void wide_bwd_state_k(const A* __restrict__ g, const A* __restrict__ T, A* __restrict__ gn,
                                                        int wcur, int Oacc, int oc, int L, int R) {
  const long long per = (long long)Oacc * L, total = (long long)wcur * per;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long wl = i / per;
    const int e = (int)(i - wl * per);
    const int l = e % L, a = e / L;
    const A* gp = g + wl * ((long long)Oacc * oc * R) + (long long)a * oc * R;
    const A* tp = T + wl * ((long long)oc * L * R) + (long long)l * R;
    A acc = A(0);
    for (int o = 0; o < oc; ++o)
      for (int r = 0; r < R; ++r) acc += gp[o * R + r] * tp[(long long)o * L * R + r];
    gn[i] = acc;
  }
}

// dT[wl][(o L + l) R + r] = sum_a v[wl][a L + l] g[wl][(a oc + o) R + r]
template <typename A>
__global__ __launch_bounds__(256) void wide_dt_k(const A* __restrict__ v, const A* __restrict__ g, A* __restrict__ dT, int wcur,
                                                 int Oacc, int oc, int L, int R) {
  const long long per = (long long)oc * L * R, total = (long long)wcur * per;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long wl = i / per;
    const int e = (int)(i - wl * per);
    const int r = e % R, ol = e / R, l = ol % L, o = ol / L;
    const A* vp = v + wl * ((long long)Oacc * L) + l;
    const A* gp = g + wl * ((long long)Oacc * oc * R) + (long long)o * R + r;
    A acc = A(0);
    for (int a = 0; a < Oacc; ++a) acc += vp[(long long)a * L] * gp[(long long)a * oc * R];
    dT[i] = acc;
  }
}

// gxw[((c C + ch) q + qv)][w] (= or +=) sum_{k: digit_ch(k) = qv} df[wl][k] prod_{ch' != ch} x[ch'][pixel][digit_ch'(k)]
template <typename S, typename A>
__global__ __launch_bounds__(256) void wide_gxw_k(const S* __restrict__ x, WideP p, int c, long long w0, int wcur,
                                                  const A* __restrict__ df, A* __restrict__ gxw, int accumulate) {
  const int cq = p.C * p.q;
  const long long total = (long long)wcur * cq;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long wl = i % wcur;   // windows fastest: coalesced stores into gxw
    const int chq = (int)(i / wcur), ch = chq / p.q, qv = chq - (chq / p.q) * p.q;
    const long long w = w0 + wl;
    const int hw = p.Ho * p.Wo;
    const long long b = w / hw;
    const int rem = (int)(w - b * hw);
    const int ho = rem / p.Wo, wo = rem - (rem / p.Wo) * p.Wo;
    const long long base = b * p.s[1] + (long long)(ho + p.ph[c]) * p.s[2] + (long long)(wo + p.pw[c]) * p.s[3];
    A acc = A(0);
    for (int k = 0; k < p.qc; ++k) {
      int t = k;
      A pr = A(1);
      bool hit = false;
      for (int c2 = p.C - 1; c2 >= 0; --c2) {
        const int dg = t % p.q;
        t /= p.q;
        if (c2 == ch) hit = dg == qv;
        else pr *= (A)x[c2 * p.s[0] + base + dg * p.s[4]];
      }
      if (hit) acc += df[wl * p.qc + k] * pr;
    }
    A* dst = gxw + (long long)((c * p.C + ch) * p.q + qv) * p.Wn + w;
    *dst = accumulate ? *dst + acc : acc;
  }
}

// dst[e] = (accumulate ? dst[e] : 0) + sum_{z = 0 .. splits-1} part[z][e], in that order
template <typename A>
__global__ __launch_bounds__(256) void wide_reduce_k(const A* __restrict__ part, int splits, long long E, A* __restrict__ dst,
                                                     int accumulate) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
    A acc = accumulate ? dst[e] : A(0);
    for (int z = 0; z < splits; ++z) acc += part[(long long)z * E + e];
    dst[e] = acc;
  }
}

template <typename S>
__global__ __launch_bounds__(256) void wide_convert_k(const float* __restrict__ src, S* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = (S)src[i];
}

// ---------------------------------------------------------------------------------------------------- strided GEMM
// C[m][n] = sum_{k in split z} A[m][k] B[k][n]; operands at a + m sam + k sak, b + k sbk + n sbn, C at c + z csplit + m scm + n scn.
// 256 threads; WM x WN waves, each wave FM x FN fragments of 16 x 16; K in steps of 16 through LDS, zero-padded at the
// edges (only real entries are written back).  float: v_mfma_f32_16x16x4_f32; double: 4 x 4 outputs per thread on FMA.
template <typename TA, typename TB, typename A, int WM, int WN, int FM, int FN>
__global__ __launch_bounds__(256) void wide_gemm_k(const TA* __restrict__ a, long long sam, long long sak, const TB* __restrict__ b,
                                                   long long sbk, long long sbn, A* __restrict__ c, long long scm, long long scn,
                                                   long long csplit, int M, int N, int K, int kchunk) {
  constexpr int TM = WM * FM * 16, TN = WN * FN * 16, BK = 16;
  static_assert(WM * WN == 4 && TM * TN == 4096, "tile");
  __shared__ A as[BK][TM + 4];
  __shared__ A bs[BK][TN + 4];
  const int tid = threadIdx.x;
  const long long m0 = (long long)blockIdx.y * TM, n0 = (long long)blockIdx.x * TN;
  const int kb0 = (int)blockIdx.z * kchunk;
  const int kb1 = kb0 + kchunk < K ? kb0 + kchunk : K;
  c += (long long)blockIdx.z * csplit;
  const int lane = tid & 63, wave = tid >> 6, wm = wave % WM, wn = wave / WM;
  wd_f4 acc[FM][FN];
  double dacc[4][4];
  if constexpr (std::is_same<A, float>::value) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = wd_f4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dacc[i][j] = 0.0;
  }
  const int ty = tid / (TN / 4), tx = tid % (TN / 4);
  for (int k0 = kb0; k0 < kb1; k0 += BK) {
    // stage the tiles; the index order follows whichever stride is unit (coalesced loads)
    for (int i = tid; i < TM * BK; i += 256) {
      int mm, kk;
      if (sak == 1) { kk = i % BK; mm = i / BK; } else { mm = i % TM; kk = i / TM; }
      const long long m = m0 + mm;
      const int k = k0 + kk;
      as[kk][mm] = (m < M && k < kb1) ? (A)a[m * sam + (long long)k * sak] : A(0);
    }
    for (int i = tid; i < TN * BK; i += 256) {
      int nn, kk;
      if (sbn == 1) { nn = i % TN; kk = i / TN; } else { kk = i % BK; nn = i / BK; }
      const long long nx = n0 + nn;
      const int k = k0 + kk;
      bs[kk][nn] = (nx < N && k < kb1) ? (A)b[(long long)k * sbk + nx * sbn] : A(0);
    }
    __syncthreads();
    if constexpr (std::is_same<A, float>::value) {
#pragma unroll
      for (int kk = 0; kk < BK; kk += 4) {
        float av[FM], bv[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) av[i] = as[kk + (lane >> 4)][(wm * FM + i) * 16 + (lane & 15)];
#pragma unroll
        for (int j = 0; j < FN; ++j) bv[j] = bs[kk + (lane >> 4)][(wn * FN + j) * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll 4
      for (int kk = 0; kk < BK; ++kk) {
        A av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = as[kk][ty * 4 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = bs[kk][tx * 4 + j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) dacc[i][j] = fma((double)av[i], (double)bv[j], dacc[i][j]);
      }
    }
    __syncthreads();
  }
  if constexpr (std::is_same<A, float>::value) {
    // C/D of the 16x16x4 form: col = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const long long nx = n0 + (wn * FN + j) * 16 + (lane & 15);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const long long m = m0 + (wm * FM + i) * 16 + 4 * (lane >> 4) + v;
          if (m < M && nx < N) c[m * scm + nx * scn] = acc[i][j][v];
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long m = m0 + ty * 4 + i, nx = n0 + tx * 4 + j;
        if (m < M && nx < N) c[m * scm + nx * scn] = (A)dacc[i][j];
      }
  }
}

template <typename TA, typename TB, typename A>
int wide_gemm(const TA* a, long long sam, long long sak, const TB* b, long long sbk, long long sbn, A* c, long long scm,
              long long scn, long long M, long long N, long long K, int splits, long long csplit, hipStream_t st) {
  const long long kchunk = ((K + splits - 1) / splits + 15) & ~15LL;
  if (N <= 16) {   // narrow N (q^C small): 256 x 16 tiles, four waves stacked along M
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)((M + 255) / 256), (unsigned)splits);
    hipLaunchKernelGGL((wide_gemm_k<TA, TB, A, 4, 1, 4, 1>), grid, dim3(256), 0, st, a, sam, sak, b, sbk, sbn, c, scm, scn, csplit,
                       (int)M, (int)N, (int)K, (int)kchunk);
  } else {
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64), (unsigned)splits);
    hipLaunchKernelGGL((wide_gemm_k<TA, TB, A, 2, 2, 2, 2>), grid, dim3(256), 0, st, a, sam, sak, b, sbk, sbn, c, scm, scn, csplit,
                       (int)M, (int)N, (int)K, (int)kchunk);
  }
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

#define WD_TRY(expr)                   \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != DCTN_OK) return rc_;    \
  } while (0)

template <typename S, typename A>
int wide_run(const void* xv, const void* const* cores, const void* dYv, int need_dx, void* const* dcores_out, unsigned char* ws,
             const WideP& p, const WideLayout& L, hipStream_t st) {
  const S* x = (const S*)xv;
  const S* dY = (const S*)dYv;
  const int need_dcore = dcores_out != nullptr;
  A* gxw = (A*)(ws + L.gxw);
  A* part = (A*)(ws + L.part);
  A* V = (A*)(ws + L.v);
  A* F = (A*)(ws + L.f);
  A* T = (A*)(ws + L.t);
  A* G = (A*)(ws + L.g0);
  A* Gn = (A*)(ws + L.g1);
  A* df = (A*)(ws + L.df);
  A* dst[WIDE_MAXC];
  {
    size_t off = 0;
    for (int c = 0; c < p.n; ++c) {
      const long long ce = (long long)p.o[c] * p.bl[c] * p.br[c] * p.qc;
      dst[c] = std::is_same<S, A>::value ? (A*)(need_dcore ? dcores_out[c] : nullptr) : (A*)(ws + L.acc) + off;
      off += (size_t)ce;
    }
  }
  const long long nchunks = (p.Wn + L.wc - 1) / L.wc;
  for (int s = 0; s < p.l0; ++s)
    for (long long ch = 0; ch < nchunks; ++ch) {
      const long long w0 = ch * L.wc;
      const int wcur = (int)(p.Wn - w0 < L.wc ? p.Wn - w0 : L.wc);
      // ---- forward sweep: the input state of every core into V
      hipLaunchKernelGGL((wide_state0_k<A>), dim3(wd_grid((long long)wcur * p.l0)), dim3(256), 0, st, V, wcur, p.l0, s);
      DCTN_CHECK_LAUNCH();
      for (int c = 0; c + 1 < p.n; ++c) {
        const int oc = p.o[c], Lb = p.bl[c], R = p.br[c], Oacc = p.oacc[c];
        const long long E = (long long)oc * Lb * R;
        hipLaunchKernelGGL((wide_feat_k<S, A>), dim3(wd_grid((long long)wcur * p.qc)), dim3(256), 0, st, x, p, c, w0, wcur, F);
        DCTN_CHECK_LAUNCH();
        WD_TRY((wide_gemm<A, S, A>(F, p.qc, 1, (const S*)cores[c], 1, p.qc, T, E, 1, wcur, E, p.qc, 1, 0, st)));
        hipLaunchKernelGGL((wide_fwd_step_k<A>), dim3(wd_grid((long long)wcur * Oacc * oc * R)), dim3(256), 0, st,
                           V + p.st_off[c] * wcur, T, V + p.st_off[c + 1] * wcur, wcur, Oacc, oc, Lb, R);
        DCTN_CHECK_LAUNCH();
      }
      // ---- adjoint sweep, right to left
      hipLaunchKernelGGL((wide_grad0_k<S, A>), dim3(wd_grid((long long)wcur * p.Otot * p.l0)), dim3(256), 0, st, dY, G, w0, wcur,
                         p.Otot, p.l0, s);
      DCTN_CHECK_LAUNCH();
      for (int c = p.n - 1; c >= 0; --c) {
        const int oc = p.o[c], Lb = p.bl[c], R = p.br[c], Oacc = p.oacc[c];
        const long long E = (long long)oc * Lb * R;
        const A* Vc = V + p.st_off[c] * wcur;
        hipLaunchKernelGGL((wide_feat_k<S, A>), dim3(wd_grid((long long)wcur * p.qc)), dim3(256), 0, st, x, p, c, w0, wcur, F);
        DCTN_CHECK_LAUNCH();
        if (c > 0) {
          WD_TRY((wide_gemm<A, S, A>(F, p.qc, 1, (const S*)cores[c], 1, p.qc, T, E, 1, wcur, E, p.qc, 1, 0, st)));
          hipLaunchKernelGGL((wide_bwd_state_k<A>), dim3(wd_grid((long long)wcur * Oacc * Lb)), dim3(256), 0, st, G, T, Gn, wcur,
                             Oacc, oc, Lb, R);
          DCTN_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL((wide_dt_k<A>), dim3(wd_grid((long long)wcur * E)), dim3(256), 0, st, Vc, G, T, wcur, Oacc, oc, Lb, R);
        DCTN_CHECK_LAUNCH();
        if (need_dcore) {
          // partial records over window splits, then their fixed-order sum into the gradient (first pass, first chunk: =)
          WD_TRY((wide_gemm<A, A, A>(T, 1, E, F, p.qc, 1, part, p.qc, 1, E, p.qc, wcur, L.splits, E * p.qc, st)));
          hipLaunchKernelGGL((wide_reduce_k<A>), dim3(wd_grid(E * p.qc)), dim3(256), 0, st, part, L.splits, E * p.qc, dst[c],
                             (s > 0 || ch > 0) ? 1 : 0);
          DCTN_CHECK_LAUNCH();
        }
        if (need_dx) {
          WD_TRY((wide_gemm<A, S, A>(T, E, 1, (const S*)cores[c], p.qc, 1, df, p.qc, 1, wcur, p.qc, E, 1, 0, st)));
          hipLaunchKernelGGL((wide_gxw_k<S, A>), dim3(wd_grid((long long)wcur * p.C * p.q)), dim3(256), 0, st, x, p, c, w0, wcur,
                             df, gxw, s > 0 ? 1 : 0);
          DCTN_CHECK_LAUNCH();
        }
        A* tmp = G; G = Gn; Gn = tmp;
      }
    }
  if constexpr (!std::is_same<S, A>::value) {
    if (need_dcore)
      for (int c = 0; c < p.n; ++c) {
        const long long ce = (long long)p.o[c] * p.bl[c] * p.br[c] * p.qc;
        hipLaunchKernelGGL((wide_convert_k<S>), dim3(wd_grid(ce)), dim3(256), 0, st, (const float*)dst[c], (S*)dcores_out[c], ce);
        DCTN_CHECK_LAUNCH();
      }
  }
  return DCTN_OK;
}

}  // namespace

size_t convsbs_wide_bwd_workspace(const SbsShape& sh) {
  if (sh.dtype != DCTN_F32 && sh.dtype != DCTN_F64 && sh.dtype != DCTN_BF16) return 0;
  WideP p;
  if (wide_fill(p, sh) != DCTN_OK) return 0;
  return wide_layout(p, sh.dtype).total;
}

int convsbs_bwd_wide(const void* x, const int64_t xs[5], const void* const* cores, const void* dY, void* dX,
                     void* const* dcores, const SbsShape& sh, hipStream_t st, void* ws, size_t ws_bytes) {
  const int dtype = sh.dtype;
  if (dtype != DCTN_F32 && dtype != DCTN_F64 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  WideP p;
  int rc = wide_fill(p, sh);
  if (rc != DCTN_OK) return rc;
  for (int i = 0; i < 5; ++i) p.s[i] = xs[i];
  // the family's only LDS is the GEMM tiles (static): a device whose workgroups get less declines before any write
  const size_t tile_lds = (size_t)16 * (64 + 4 + 64 + 4) * acc_size(dtype);
  const size_t tile_lds_narrow = (size_t)16 * (256 + 4 + 16 + 4) * acc_size(dtype);
  if ((tile_lds > tile_lds_narrow ? tile_lds : tile_lds_narrow) > (size_t)dctn_lds_wg_max()) return DCTN_ERR_UNSUPPORTED;
  const WideLayout L = wide_layout(p, dtype);
  if (!ws || ws_bytes < L.total) return DCTN_ERR_WORKSPACE;
  for (int c = 0; c < sh.n; ++c)
    if (!cores[c] || (dcores && !dcores[c])) return DCTN_ERR_NULL;
  unsigned char* w = (unsigned char*)ws;
  switch (dtype) {
    case DCTN_F32: rc = wide_run<float, float>(x, cores, dY, dX != nullptr, dcores, w, p, L, st); break;
    case DCTN_F64: rc = wide_run<double, double>(x, cores, dY, dX != nullptr, dcores, w, p, L, st); break;
    case DCTN_BF16: rc = wide_run<bf16_t, float>(x, cores, dY, dX != nullptr, dcores, w, p, L, st); break;
  }
  // dX: gathered from the per-window input gradients at the start of the workspace, as the generic sweep's is
  if (rc == DCTN_OK && dX) rc = convsbs_gather_dx(sh, ws, dX, st);
  if (rc != DCTN_OK) return rc;
  dctn_set_last_kernel(dtype == DCTN_F64 ? "convsbs_bwd_wide_f64" : dtype == DCTN_BF16 ? "convsbs_bwd_wide_bf16"
                                                                                    : "convsbs_bwd_wide_f32");
  return DCTN_OK;
}
