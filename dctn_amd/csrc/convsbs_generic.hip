// Generic ConvSBS kernels: any string (arbitrary core order, ring or open chain, per-bond sizes,
// outputs on several cores, C channels), float32 / float64 / bf16 storage.
//
// Replaces dctn/conv_sbs.py:258-304 (ConvSBS.forward) and torch autograd through it.
// The reference materialises, per core, a (B,H',W',o,l,r) tensor in HBM and then multiplies the
// chain.  Here one lane owns one window and sweeps the string left to right carrying only the
// state v[o_acc][bond] in its LDS column; the per-window matrices T_c are never written out.
// A ring (bond_sizes[0] > 1) is closed by running the sweep once per value of the traced bond.
//
// Backward: the forward states are kept in a caller-supplied workspace ([element][window],
// coalesced), then an adjoint sweep right to left produces dT_c, from which
//   dCore_c += dT_c (x) f_c   (wave reduction, one float atomic per element per wave)
//   df_c -> d/d(pixel features), written per window and summed per pixel by a gather kernel.
#include "common.h"

#define SBS_MAXC 32

struct SbsP {
  int n, C, B, H, W, q, qc, Ho, Wo, l0, Otot, vmax;
  int cs;   // window columns per workgroup (power of two <= 64); lanes t and t+cs mirror one window
  int cst;  // LDS column stride (cs forward; cs + 1 backward: conflict-free for both lane roles)
  int cmax;                          // largest core (elements): size of the LDS core tile
  long long core_off[SBS_MAXC + 1];  // offsets of the cores in the workgroup's LDS dCore accumulator
  long long Wn;
  long long s[5];
  int o[SBS_MAXC], bl[SBS_MAXC], br[SBS_MAXC], ph[SBS_MAXC], pw[SBS_MAXC];
  int oacc[SBS_MAXC + 1];        // product of out sizes of cores < c
  long long st_off[SBS_MAXC + 1];  // element offsets of the stored forward states
  const void* core[SBS_MAXC];
  void* dcore[SBS_MAXC];  // A-typed accumulators (== dCores for f32/f64)
};

namespace {

struct WinCoord {
  long long b;
  int ho, wo;
};
__device__ __forceinline__ WinCoord win_coord(const SbsP& p, long long w) {
  WinCoord c;
  const int hw = p.Ho * p.Wo;
  c.b = w / hw;
  const int rem = (int)(w - c.b * hw);
  c.ho = rem / p.Wo;
  c.wo = rem - c.ho * p.Wo;
  return c;
}

// f[qq] = prod_ch x[ch][pixel of core c][digit_ch(qq)], channel 0 most significant
template <typename S, typename A>
__device__ __forceinline__ void pixel_features(const S* __restrict__ x, const SbsP& p, int c,
                                               bool valid, const WinCoord& wc, A* f, int col) {
  for (int qq = 0; qq < p.qc; ++qq) {
    A pr = A(1);
    int t = qq;
    for (int ch = p.C - 1; ch >= 0; --ch) {
      const int dg = t % p.q;
      t /= p.q;
      const S* px = x + ch * p.s[0] + wc.b * p.s[1] + (long long)(wc.ho + p.ph[c]) * p.s[2] +
                    (long long)(wc.wo + p.pw[c]) * p.s[3] + dg * p.s[4];
      pr *= valid ? (A)(*px) : A(0);
    }
    f[qq * p.cst + col] = pr;
  }
}

// one sweep step: vb[(a*oc+o)*R + r] = sum_l va[a*L + l] * sum_qq core[o,l,r,qq] f[qq]
template <typename S, typename A>
__device__ __forceinline__ void sweep_step(const SbsP& p, int c, const A* va, A* vb, const A* f,
                                           int col) {
  const int L = p.bl[c], R = p.br[c], oc = p.o[c], Oacc = p.oacc[c];
  const S* core = (const S*)p.core[c];
  for (int e = 0; e < Oacc * oc * R; ++e) vb[e * p.cst + col] = A(0);
  for (int o = 0; o < oc; ++o)
    for (int l = 0; l < L; ++l)
      for (int r = 0; r < R; ++r) {
        const S* cp = core + (long long)((o * L + l) * R + r) * p.qc;
        A t = A(0);
        for (int qq = 0; qq < p.qc; ++qq) t += (A)cp[qq] * f[qq * p.cst + col];
        for (int a = 0; a < Oacc; ++a)
          vb[((a * oc + o) * R + r) * p.cst + col] += va[(a * L + l) * p.cst + col] * t;
      }
}

template <typename S, typename A>
__global__ __launch_bounds__(DCTN_WAVE) void convsbs_fwd_generic_k(const S* __restrict__ x,
                                                                   S* __restrict__ out, SbsP p) {
  extern __shared__ __align__(16) unsigned char smem[];
  A* va = reinterpret_cast<A*>(smem);
  A* vb = va + (size_t)p.vmax * p.cs;
  A* f = vb + (size_t)p.vmax * p.cs;
  A* oa = f + (size_t)p.qc * p.cs;
  const int tid = threadIdx.x;
  const int col = tid & (p.cs - 1);
  const bool primary = tid < p.cs;  // lanes tid >= cs mirror the window of lane tid % cs
  const long long w = (long long)blockIdx.x * p.cst + col;
  const bool valid = w < p.Wn;
  WinCoord wc = {0, 0, 0};
  if (valid) wc = win_coord(p, w);
  for (int a = 0; a < p.Otot; ++a) oa[a * p.cst + col] = A(0);
  for (int s = 0; s < p.l0; ++s) {
    for (int l = 0; l < p.l0; ++l) va[l * p.cst + col] = (l == s) ? A(1) : A(0);
    A* cur = va;
    A* nxt = vb;
    for (int c = 0; c < p.n; ++c) {
      pixel_features<S, A>(x, p, c, valid, wc, f, col);
      sweep_step<S, A>(p, c, cur, nxt, f, col);
      A* tmp = cur; cur = nxt; nxt = tmp;
    }
    for (int a = 0; a < p.Otot; ++a)
      oa[a * p.cst + col] += cur[(a * p.l0 + s) * p.cst + col];
  }
  if (valid && primary)
    for (int a = 0; a < p.Otot; ++a) out[w * p.Otot + a] = (S)oa[a * p.cst + col];
}

// Backward.  Lanes play two roles per core:
//   role "window"  (lane = window column): forward sweep (states to the workspace), adjoint sweep:
//       dT, d(state), d(pixel features); v_c, dv_{c+1} and f_c stay in the lane's LDS column;
//   role "element" (lane = core element (o,l,r,qq)): dCore_c[e] += sum over the block's windows of
//       f[qq] * sum_a v[a,l] * dv[(a,o),r], read from the same LDS image (column stride cs + 1 keeps
//       both access patterns conflict-free).  No shuffles, no atomics inside the loop.
// Workgroups are persistent: dCore is accumulated in LDS over all their window groups and
// flushed with one atomic per element per workgroup at the end.
template <typename S, typename A>
__global__ __launch_bounds__(256) void convsbs_bwd_generic_k(
    const S* __restrict__ x, const S* __restrict__ dY, A* __restrict__ states,
    A* __restrict__ gxw, SbsP p, int need_dx, int need_dcore, long long ngroups) {
  extern __shared__ __align__(16) unsigned char smem[];
  A* va = reinterpret_cast<A*>(smem);
  A* vb = va + (size_t)p.vmax * p.cst;
  A* vc = vb + (size_t)p.vmax * p.cst;
  A* f = vc + (size_t)p.vmax * p.cst;
  A* df = f + (size_t)p.qc * p.cst;
  A* dys = df + (size_t)p.qc * p.cst;
  A* dacc = dys + (size_t)p.Otot * p.cst;   // [core_off[n]] dCore accumulator of this workgroup
  // a workgroup has blockDim.x / 64 waves; with several waves every wave carries 64 columns
  // (cs == 64), with one wave the mirror-lane scheme applies (cs <= 64)
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int csb = p.cst - 1;                       // window columns of the workgroup
  const int col = nthr > DCTN_WAVE ? tid : (tid & (p.cs - 1));
  const bool primary = nthr > DCTN_WAVE ? true : tid < p.cs;
  if (need_dcore)
    for (long long e = tid; e < p.core_off[p.n]; e += nthr) dacc[e] = A(0);

  for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const long long w = grp * csb + col;
    const bool valid = w < p.Wn;
    const long long wcol = valid ? w : 0;
    WinCoord wc = {0, 0, 0};
    if (valid) wc = win_coord(p, w);
    __syncthreads();
    for (int a = 0; a < p.Otot; ++a) dys[a * p.cst + col] = valid ? (A)dY[w * p.Otot + a] : A(0);

    for (int s = 0; s < p.l0; ++s) {
      // ---- forward sweep, storing the input state of every core
      for (int l = 0; l < p.l0; ++l) va[l * p.cst + col] = (l == s) ? A(1) : A(0);
      A* cur = va;
      A* nxt = vb;
      for (int c = 0; c < p.n; ++c) {
        const int ne = p.oacc[c] * p.bl[c];
        if (valid)  // mirror lanes store the same values: every lane later reads what it wrote itself
          for (int e = 0; e < ne; ++e)
            states[(p.st_off[c] + e) * p.Wn + wcol] = cur[e * p.cst + col];
        if (c + 1 < p.n) {
          pixel_features<S, A>(x, p, c, valid, wc, f, col);
          sweep_step<S, A>(p, c, cur, nxt, f, col);
          A* tmp = cur; cur = nxt; nxt = tmp;
        }
      }
      // ---- adjoint sweep.  dv: gradient wrt the OUTPUT state of core c, shape [Oacc*oc][R]
      A* dv = vb;
      A* dvn = vc;
      for (int a = 0; a < p.Otot; ++a)
        for (int r = 0; r < p.l0; ++r)
          dv[(a * p.l0 + r) * p.cst + col] = (r == s) ? dys[a * p.cst + col] : A(0);
      for (int c = p.n - 1; c >= 0; --c) {
        const int L = p.bl[c], R = p.br[c], oc = p.o[c], Oacc = p.oacc[c];
        const S* core = (const S*)p.core[c];
        for (int e = 0; e < Oacc * L; ++e)
          va[e * p.cst + col] = valid ? states[(p.st_off[c] + e) * p.Wn + wcol] : A(0);
        pixel_features<S, A>(x, p, c, valid, wc, f, col);
        for (int e = 0; e < Oacc * L; ++e) dvn[e * p.cst + col] = A(0);
        for (int qq = 0; qq < p.qc; ++qq) df[qq * p.cst + col] = A(0);
        for (int o = 0; o < oc; ++o)
          for (int l = 0; l < L; ++l)
            for (int r = 0; r < R; ++r) {
              const int cbase = ((o * L + l) * R + r) * p.qc;
              A t = A(0);
              for (int qq = 0; qq < p.qc; ++qq) t += (A)core[cbase + qq] * f[qq * p.cst + col];
              A dT = A(0);
              for (int a = 0; a < Oacc; ++a) {
                const A g = dv[((a * oc + o) * R + r) * p.cst + col];
                dT += va[(a * L + l) * p.cst + col] * g;
                dvn[(a * L + l) * p.cst + col] += t * g;
              }
              if (need_dx)
                for (int qq = 0; qq < p.qc; ++qq) df[qq * p.cst + col] += dT * (A)core[cbase + qq];
            }
        if (need_dcore) {
          // role "element": this lane owns elements e = tid, tid + 64, ... of core c
          __syncthreads();
          const int E = oc * L * R * p.qc;
          for (int e = tid; e < E; e += nthr) {
            const int qq = e % p.qc;
            int t2 = e / p.qc;
            const int r = t2 % R; t2 /= R;
            const int l = t2 % L;
            const int o = t2 / L;
            A acc = A(0);
            for (int wl = 0; wl < csb; ++wl) {
              A dT = A(0);
              for (int a = 0; a < Oacc; ++a)
                dT += va[(a * L + l) * p.cst + wl] * dv[((a * oc + o) * R + r) * p.cst + wl];
              acc += dT * f[qq * p.cst + wl];
            }
            dacc[p.core_off[c] + e] += acc;
          }
          __syncthreads();
        }
        if (need_dx && valid && primary) {
          // d/d x[ch][pixel_c][qv] = sum_{qq: digit_ch(qq) = qv} df[qq] * prod_{ch' != ch} x[ch'][digit]
          for (int ch = 0; ch < p.C; ++ch)
            for (int qv = 0; qv < p.q; ++qv) {
              A g = A(0);
              for (int qq = 0; qq < p.qc; ++qq) {
                int t = qq;
                A pr = A(1);
                bool hit = false;
                for (int c2 = p.C - 1; c2 >= 0; --c2) {
                  const int dg = t % p.q;
                  t /= p.q;
                  if (c2 == ch) {
                    hit = (dg == qv);
                  } else {
                    pr *= (A)x[c2 * p.s[0] + wc.b * p.s[1] + (long long)(wc.ho + p.ph[c]) * p.s[2] +
                               (long long)(wc.wo + p.pw[c]) * p.s[3] + dg * p.s[4]];
                  }
                }
                if (hit) g += df[qq * p.cst + col] * pr;
              }
              A* dst = &gxw[(long long)((c * p.C + ch) * p.q + qv) * p.Wn + w];
              if (s == 0) *dst = g; else *dst += g;
            }
        }
        A* tmp = dv; dv = dvn; dvn = tmp;
      }
    }
  }
  if (need_dcore) {
    __syncthreads();
    for (int c = 0; c < p.n; ++c) {
      A* dcore = (A*)p.dcore[c];
      const long long E = p.core_off[c + 1] - p.core_off[c];
      for (long long e = tid; e < E; e += nthr) atomicAdd(&dcore[e], dacc[p.core_off[c] + e]);
    }
  }
}

// dX[ch,b,h,w,qv] = sum_c gxw[((c*C+ch)*q+qv)][window (h-ph_c, w-pw_c)]
template <typename S, typename A>
__global__ void convsbs_gather_dx_k(const A* __restrict__ gxw, S* __restrict__ dX, SbsP p) {
  const long long total = (long long)p.C * p.B * p.H * p.W * p.q;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    long long t = idx;
    const int qv = (int)(t % p.q); t /= p.q;
    const int wi = (int)(t % p.W); t /= p.W;
    const int hi = (int)(t % p.H); t /= p.H;
    const int b = (int)(t % p.B);
    const int ch = (int)(t / p.B);
    A acc = A(0);
    for (int c = 0; c < p.n; ++c) {
      const int ho = hi - p.ph[c], wo = wi - p.pw[c];
      if (ho < 0 || ho >= p.Ho || wo < 0 || wo >= p.Wo) continue;
      const long long win = ((long long)b * p.Ho + ho) * p.Wo + wo;
      acc += gxw[(long long)((c * p.C + ch) * p.q + qv) * p.Wn + win];
    }
    dX[idx] = (S)acc;
  }
}

template <typename S, typename A>
__global__ void convert_sbs_k(const A* __restrict__ src, S* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    dst[i] = (S)src[i];
}

// cores (optional): the calls' core pointers, every one non-NULL
int fill(SbsP& p, const int64_t xs[5], const SbsShape& sh, const void* const* cores = nullptr) {
  if (sh.n < 1 || sh.n > SBS_MAXC) return sh.n < 1 ? DCTN_ERR_BAD_SHAPE : DCTN_ERR_UNSUPPORTED;
  if (sh.C < 1 || sh.B < 1 || sh.q < 1) return DCTN_ERR_BAD_SHAPE;
  int max_h = 0, max_w = 0, min_h = 1 << 30, min_w = 1 << 30;
  for (int c = 0; c < sh.n; ++c) {
    if (sh.out_sizes[c] < 1 || sh.bond_sizes[c] < 1 || sh.pos_h[c] < 0 || sh.pos_w[c] < 0)
      return DCTN_ERR_BAD_SHAPE;
    max_h = sh.pos_h[c] > max_h ? sh.pos_h[c] : max_h;
    max_w = sh.pos_w[c] > max_w ? sh.pos_w[c] : max_w;
    min_h = sh.pos_h[c] < min_h ? sh.pos_h[c] : min_h;
    min_w = sh.pos_w[c] < min_w ? sh.pos_w[c] : min_w;
  }
  if (min_h != 0 || min_w != 0) return DCTN_ERR_BAD_SHAPE;  // dctn/align.py:18-19
  if (sh.H <= max_h || sh.W <= max_w) return DCTN_ERR_BAD_SHAPE;
  p.n = sh.n; p.C = sh.C; p.B = sh.B; p.H = sh.H; p.W = sh.W; p.q = sh.q;
  long long qc = 1;
  for (int c = 0; c < sh.C; ++c) { qc *= sh.q; if (qc > 4096) return DCTN_ERR_UNSUPPORTED; }
  p.qc = (int)qc;
  p.Ho = sh.H - max_h; p.Wo = sh.W - max_w;
  p.Wn = (long long)sh.B * p.Ho * p.Wo;
  for (int i = 0; i < 5; ++i) p.s[i] = xs ? xs[i] : 0;
  p.l0 = sh.bond_sizes[0];
  long long oacc = 1, off = 0;
  int vmax = p.l0;
  for (int c = 0; c < sh.n; ++c) {
    p.o[c] = sh.out_sizes[c];
    p.bl[c] = sh.bond_sizes[c];
    p.br[c] = sh.bond_sizes[(c + 1) % sh.n];
    p.ph[c] = sh.pos_h[c];
    p.pw[c] = sh.pos_w[c];
    p.oacc[c] = (int)oacc;
    p.st_off[c] = off;
    off += oacc * p.bl[c];
    oacc *= sh.out_sizes[c];
    if (oacc * p.br[c] > (1 << 20)) return DCTN_ERR_UNSUPPORTED;
    if ((int)(oacc * p.br[c]) > vmax) vmax = (int)(oacc * p.br[c]);
  }
  p.oacc[sh.n] = (int)oacc;
  p.st_off[sh.n] = off;
  p.cmax = 0;
  p.core_off[0] = 0;
  for (int c = 0; c < sh.n; ++c) {
    const long long e = (long long)p.o[c] * p.bl[c] * p.br[c] * p.qc;
    if (e > (1 << 20)) return DCTN_ERR_UNSUPPORTED;
    if ((int)e > p.cmax) p.cmax = (int)e;
    p.core_off[c + 1] = p.core_off[c] + e;
  }
  p.Otot = (int)oacc;
  p.vmax = vmax;
  for (int c = 0; cores && c < sh.n; ++c) {
    if (!cores[c]) return DCTN_ERR_NULL;
    p.core[c] = cores[c];
    p.dcore[c] = nullptr;
  }
  return DCTN_OK;
}

long long core_elems(const SbsP& p, int c) { return p.core_off[c + 1] - p.core_off[c]; }

// f(S(), A()) with the storage and accumulator types of a dtype code
template <typename F>
int with_types(int dtype, F f) {
  switch (dtype) {
    case DCTN_F32: return f(float(), float());
    case DCTN_F64: return f(double(), double());
    case DCTN_BF16: return f(bf16_t(), float());
  }
  return DCTN_ERR_BAD_DTYPE;
}

// The backward workspace, region by region in this order (bytes, each a multiple of 256): forward states
// [element][window] | per-window d/d(pixel features) | bf16 storage: the float32 accumulators of the cores, one aligned row
// each | float32: the matrix-core backward's per-workgroup records (fixed-order reduce instead of atomics)
struct BwdLayout { size_t states, gxw, acc, partials, total; };
BwdLayout bwd_layout(const SbsP& p, const SbsShape& sh) {
  const size_t asz = acc_size(sh.dtype);
  // State elements per window: the generic sweep's own need, or the matrix-core sweep's when that is more - a padded bond
  // (6 -> 8) or a ring (whose generic states are counted differently) would otherwise let its states run into the
  // feature-gradient region behind them, which ring / many-output slices accumulate across launches.
  const long long own = p.st_off[p.n], mfma = convsbs_mfma_state_elems(sh);
  BwdLayout L;
  L.states = align256((size_t)(mfma > own ? mfma : own) * p.Wn * asz);
  L.gxw = align256((size_t)p.n * p.C * p.q * p.Wn * asz);
  L.acc = 0;
  if (sh.dtype == DCTN_BF16)
    for (int c = 0; c < p.n; ++c) L.acc += align256((size_t)core_elems(p, c) * asz);
  L.partials = align256(convsbs_mfma_partial_bytes(sh));
  L.total = L.states + L.gxw + L.acc + L.partials;
  return L;
}

// The backward's LDS plan: sets p.cs, p.cst; lds == 0: no fit; several waves share one dCore accumulator when each has its 64 columns
struct BwdLds { size_t lds; int waves; };
BwdLds bwd_lds_plan(SbsP& p, size_t asz, bool need_dcore) {
  const size_t acc_bytes = need_dcore ? (size_t)p.core_off[p.n] * asz : 0;
  if (acc_bytes > dctn_lds_wg_max() / 2) return {0, 0};
  const size_t per_col = ((size_t)3 * p.vmax + 2 * p.qc + p.Otot) * asz;
  p.cs = DCTN_WAVE;
  while (p.cs > 1 && per_col * (p.cs + 1) + acc_bytes > dctn_lds_wg_max()) p.cs >>= 1;
  int waves = 1;
  if (p.cs == DCTN_WAVE && acc_bytes >= 4096)  // small strings: more, smaller workgroups win
    while (waves < 4 && per_col * (2 * waves * DCTN_WAVE + 1) + acc_bytes <= dctn_lds_wg_max()) waves *= 2;
  p.cst = waves * p.cs + 1;
  const size_t lds = per_col * p.cst + acc_bytes;
  return {lds > dctn_lds_wg_max() ? 0 : lds, waves};
}

// the A-typed accumulators of the cores: the gradients themselves, or (bf16 storage) their rows in the workspace
template <typename S, typename A>
void set_accumulators(SbsP& p, void* const* dCores, unsigned char* acc) {
  for (int c = 0; c < p.n; ++c) {
    p.dcore[c] = sizeof(S) == sizeof(A) ? dCores[c] : acc;
    acc += align256((size_t)core_elems(p, c) * sizeof(A));
  }
}

}  // namespace

// (the launchers below stand in the order in which they first use their kernels: the device code keeps it)
int convsbs_check_shape(const SbsShape& sh, const void* const* cores) {
  SbsP p;
  return fill(p, nullptr, sh, cores);
}

int convsbs_fwd_generic(const void* x, const int64_t xs[5], const void* const* cores, void* out, const SbsShape& sh, hipStream_t st) {
  return with_types(sh.dtype, [&](auto s, auto a) -> int {
    using S = decltype(s); using A = decltype(a);
    SbsP p;
    const int rc = fill(p, xs, sh, cores);
    if (rc != DCTN_OK) return rc;
    const size_t per_col = ((size_t)2 * p.vmax + p.qc + p.Otot) * sizeof(A);
    p.cs = DCTN_WAVE;
    while (p.cs > 1 && per_col * p.cs > dctn_lds_wg_max()) p.cs >>= 1;
    const size_t lds = per_col * p.cs;
    if (lds > dctn_lds_wg_max() || !dctn_lds_optin((const void*)convsbs_fwd_generic_k<S, A>, lds)) return DCTN_ERR_UNSUPPORTED;
    p.cst = p.cs;
    const unsigned grid = (unsigned)((p.Wn + p.cs - 1) / p.cs);
    hipLaunchKernelGGL((convsbs_fwd_generic_k<S, A>), dim3(grid), dim3(DCTN_WAVE), lds, st, (const S*)x, (S*)out, p);
    DCTN_CHECK_LAUNCH();
    dctn_set_last_kernel("convsbs_fwd_generic");
    return DCTN_OK;
  });
}

int convsbs_gather_dx(const SbsShape& sh, const void* gxw, void* dX, hipStream_t st) {
  return with_types(sh.dtype, [&](auto s, auto a) -> int {
    using S = decltype(s); using A = decltype(a);
    SbsP p;
    const int rc = fill(p, nullptr, sh);
    if (rc != DCTN_OK) return rc;
    const long long total = (long long)p.C * p.B * p.H * p.W * p.q;
    const unsigned g2 = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL((convsbs_gather_dx_k<S, A>), dim3(g2), dim3(256), 0, st, (const A*)gxw, (S*)dX, p);
    DCTN_CHECK_LAUNCH();
    return DCTN_OK;
  });
}

size_t convsbs_bwd_generic_workspace(const SbsShape& sh, bool* lds_fits) {
  SbsP p;
  if (fill(p, nullptr, sh) != DCTN_OK) return 0;
  if (lds_fits) *lds_fits = bwd_lds_plan(p, acc_size(sh.dtype), true).lds != 0;
  return bwd_layout(p, sh).total;
}

// (declines - DCTN_ERR_UNSUPPORTED - only in its LDS plan, before anything is written)
int convsbs_bwd_generic_plan(SbsBwdPlan& pl, const SbsShape& sh, void* const* dCores, void* ws, size_t ws_bytes, hipStream_t st) {
  return with_types(sh.dtype, [&](auto s, auto a) -> int {
    using S = decltype(s); using A = decltype(a);
    SbsP p;
    const int rc = fill(p, nullptr, sh);
    if (rc != DCTN_OK) return rc;
    const BwdLayout L = bwd_layout(p, sh);
    if (!ws || L.total > ws_bytes) return DCTN_ERR_WORKSPACE;
    const size_t lds = bwd_lds_plan(p, sizeof(A), dCores != nullptr).lds;
    if (!lds || !dctn_lds_optin((const void*)convsbs_bwd_generic_k<S, A>, lds)) return DCTN_ERR_UNSUPPORTED;
    pl.states = ws;
    pl.gxw = (unsigned char*)ws + L.states;
    pl.acc = (unsigned char*)pl.gxw + L.gxw;
    // the matrix-core backward's records; a tail too short for them is no error: that sweep then uses its other reduction
    unsigned char* tail = pl.acc + L.acc;
    pl.partial_bytes = convsbs_mfma_partial_bytes(sh);
    pl.partials = (size_t)((unsigned char*)ws + ws_bytes - tail) >= pl.partial_bytes ? (float*)tail : nullptr;
    if (!dCores) return DCTN_OK;
    for (int c = 0; c < p.n; ++c)
      if (!dCores[c]) return DCTN_ERR_NULL;
    set_accumulators<S, A>(p, dCores, pl.acc);
    // the accumulators start from zero: ONE fill when they sit back to back (the Python wrapper allocates the
    // gradients of a string as one flat buffer; nine separate fills were 30 us of a 200 us backward), else one each
    bool flat = true;
    size_t total = 0;
    for (int c = 0; c < p.n; ++c) {
      if (c > 0 && (unsigned char*)p.dcore[c] != (unsigned char*)p.dcore[0] + total) flat = false;
      total += (size_t)core_elems(p, c) * sizeof(A);
    }
    if (flat) return dctn_zero_async(p.dcore[0], total, st) != DCTN_OK ? DCTN_ERR_LAUNCH : DCTN_OK;
    for (int c = 0; c < p.n; ++c)
      if (dctn_zero_async(p.dcore[c], (size_t)core_elems(p, c) * sizeof(A), st) != DCTN_OK) return DCTN_ERR_LAUNCH;
    return DCTN_OK;
  });
}

int convsbs_bwd_generic_run(const SbsBwdPlan& pl, const void* x, const int64_t xs[5], const void* const* cores,
                            const void* dY, void* dX, void* const* dCores, const SbsShape& sh, hipStream_t st) {
  return with_types(sh.dtype, [&](auto s, auto a) -> int {
    using S = decltype(s); using A = decltype(a);
    SbsP p;
    int rc = fill(p, xs, sh, cores);
    if (rc != DCTN_OK) return rc;
    const int need_dcore = dCores != nullptr;
    const BwdLds lp = bwd_lds_plan(p, sizeof(A), need_dcore);
    if (need_dcore) set_accumulators<S, A>(p, dCores, pl.acc);
    const int csb = p.cst - 1;
    const long long ngroups = (p.Wn + csb - 1) / csb;
    // persistent workgroups: as many as can be resident (LDS-limited), at most one per window group
    long long grid = dctn_resident_wgs(lp.lds, 1, 8);
    if (grid > ngroups) grid = ngroups;
    hipLaunchKernelGGL((convsbs_bwd_generic_k<S, A>), dim3((unsigned)grid), dim3(DCTN_WAVE * lp.waves), lp.lds, st,
                       (const S*)x, (const S*)dY, (A*)pl.states, (A*)pl.gxw, p, dX != nullptr, need_dcore, ngroups);
    DCTN_CHECK_LAUNCH();
    if (dX && (rc = convsbs_gather_dx(sh, pl.gxw, dX, st)) != DCTN_OK) return rc;
    if constexpr (sizeof(S) != sizeof(A)) {
      for (int c = 0; need_dcore && c < p.n; ++c) {
        const long long ne = core_elems(p, c);
        hipLaunchKernelGGL((convert_sbs_k<S, A>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                           st, (const A*)p.dcore[c], (S*)dCores[c], ne);
        DCTN_CHECK_LAUNCH();
      }
    }
    dctn_set_last_kernel("convsbs_bwd_generic");
    return DCTN_OK;
  });
}

