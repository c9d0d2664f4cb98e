// MFMA EPS kernels, family "bigcore": power-of-two Q, cores that do not fit in registers
// (BASELINE cfg3: K=4/Q=2 cores of 1-2 MiB, K=3/Q=4 of 6 MiB, K=2/Q=8).  Exact float32:
// v_mfma_f32_32x32x2_f32 is bit-for-bit an fmaf chain, so this path keeps the reference's
// float32 numerics (no bf16 rounding) while running on the matrix cores.
//
// One template covers the three GEMMs of the path (reference: dctn/eps.py:25-30 and its autograd):
//     FWD  T[(b,o), w] = sum_a     core[a,b,o] * P0[w,a]            rows (b,o), k = a
//     G0   G0[a, w]    = sum_(b,o) core[a,b,o] * P1[w,b] dY[w,o]    rows a,     k = (b,o)
//     G1   G1[b, w]    = sum_(a,o) core[a,b,o] * P0[w,a] dY[w,o]    rows b,     k = (a,o)
// In every mode the matrix operand is a 32-row tile of the core streamed through LDS (double
// buffered, gathered from the core's natural layout - no packed copy in HBM), and the other
// operand is GENERATED: a lane owns one window (column of the MFMA tile) and produces
// P[w][k] = hi(k) * table[k_lo] from a small per-lane register table and the window's features in
// LDS.  Epilogues are lane-local: FWD weights the 16 accumulator rows with P1[w,b] and reduces
// over b; G0/G1 turn dL/dP0 (dL/dP1) into per-factor gradients by leave-one-out products.
// A wave carries NT column tiles (NT*32 windows) per streamed core tile.
#include "eps_bigcore_k.h"

#if BC_PART == 1
#ifdef DCTN_STAMPS
extern "C" int dctn_debug_read_bc_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bc_stamps), (size_t)n * sizeof(unsigned long long));
}
#endif
int dctn_bc::launch_fwd_hi(const void* x, const void* core, void* out, const BigP& b, size_t lds, hipStream_t st) {
  switch (b.LOGO) {
    case 3: return launch_fwd<3>(x, core, out, b, lds, st);
    case 4: return launch_fwd<4>(x, core, out, b, lds, st);
    case 5: return launch_fwd<5>(x, core, out, b, lds, st);
  }
  return DCTN_ERR_UNSUPPORTED;
}
#elif BC_PART == 2
#ifdef DCTN_STAMPS
extern "C" int dctn_debug_read_bc_stamps_g(unsigned long long* host, int n) {   // the transposed (dX) launches' stamps
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bc_stamps), (size_t)n * sizeof(unsigned long long));
}
#endif
int dctn_bc::launch_g(int mode, const void* x, const void* core, const void* dY, void* out, const BigP& b,
                      size_t lds, hipStream_t st) {
  if (mode == MODE_G0) return launch_tbl<MODE_G0, BC_NT_G, 0>(x, core, dY, out, b, lds, st);
  return launch_tbl<MODE_G1, BC_NT_G, 0>(x, core, dY, out, b, lds, st);
}
#else


bool eps_bigcore_covers(const EpsP& p, int dtype, int precision) {
  if (dtype != DCTN_F32 || precision != DCTN_PREC_EXACT || !bigcore_wanted(p)) return false;
  BigP b;
  return fill_big(b, p, MODE_FWD) && big_lds(b) <= (size_t)dctn_lds_wg_max();
}

size_t eps_fwd_bigcore_workspace(const EpsP& p, int dtype, int precision) {
  if (dtype != DCTN_F32 || precision != DCTN_PREC_EXACT || !bigcore_wanted(p)) return 0;
  BigP b;
  if (!fill_big(b, p, MODE_FWD)) return 0;
  choose_row_groups(b, BC_NT_FWD, BC_MAX_RG, big_lds(b));
  return b.rg_count > 1 ? (size_t)b.rg_count * p.Wn * p.O * sizeof(float) : 0;
}


size_t eps_bigcore_saved_bytes(const EpsP& p, int dtype, int precision) {
  if (dtype != DCTN_F32 || precision != DCTN_PREC_EXACT || !bigcore_wanted(p)) return 0;
  BigP b;
  if (!fill_big(b, p, MODE_FWD) || big_lds(b) > dctn_lds_wg_max()) return 0;
  BigP b0;
  if (!fill_big(b0, p, MODE_G0) || big_lds(b0) > dctn_lds_wg_max()) return 0;
  Dp1P d;
  size_t lds, zbytes;
  if (!dp1_plan(p, b, d, lds, zbytes)) return 0;
  return zbytes;
}

int eps_fwd_bigcore(const void* x, const void* core, void* out, void* ws, size_t ws_bytes,
                    const EpsP& p, int dtype, int precision, hipStream_t st, void* zsave) {
  if (dtype != DCTN_F32 || precision != DCTN_PREC_EXACT || !bigcore_wanted(p)) return DCTN_ERR_UNSUPPORTED;
  BigP b;
  if (!fill_big(b, p, MODE_FWD)) return DCTN_ERR_UNSUPPORTED;
  const size_t lds = big_lds(b);
  if (lds > dctn_lds_wg_max()) return DCTN_ERR_UNSUPPORTED;
  b.zsave = (float*)zsave;
  choose_row_groups(b, BC_NT_FWD, BC_MAX_RG, lds);
  const size_t need = b.rg_count > 1 ? (size_t)b.rg_count * p.Wn * p.O * sizeof(float) : 0;
  if (need > 0 && (!ws || ws_bytes < need)) {  // no scratch: keep every row tile in one workgroup
    b.rg_count = 1;
    b.mt_per_rg = (b.rows + 31) / 32;
  }
  void* dst = b.rg_count > 1 ? ws : out;
  int rc = DCTN_ERR_UNSUPPORTED;
  switch (b.LOGO) {
    case 1: rc = launch_fwd<1>(x, core, dst, b, lds, st); break;
    case 2: rc = launch_fwd<2>(x, core, dst, b, lds, st); break;
    case 3: case 4: case 5: rc = dctn_bc::launch_fwd_hi(x, core, dst, b, lds, st); break;
  }
  if (rc != DCTN_OK) return rc;
  if (b.rg_count > 1) {
    const long long n = p.Wn * p.O;
    const long long nt = (n + 3) / 4;   // (a thread takes four values where the sizes allow)
    const unsigned g = (unsigned)((nt + 255) / 256 < 2048 ? (nt + 255) / 256 : 2048);
    hipLaunchKernelGGL(bigcore_sum_slices_k, dim3(g), dim3(256), 0, st, (const float*)ws, (float*)out, n,
                       b.rg_count);
    DCTN_CHECK_LAUNCH();
  }
  dctn_set_last_kernel(zsave ? "eps_fwd_mfma_bigcore_f32_saving" : "eps_fwd_mfma_bigcore_f32");
  return DCTN_OK;
}



size_t eps_bwd_dfactor_bigcore_workspace(const EpsP& p, int dtype, int precision) {
  if (dtype != DCTN_F32 || precision != DCTN_PREC_EXACT || !bigcore_wanted(p)) return 0;
  BigP b0, b1;
  if (!dfactor_plan(p, b0, b1)) return 0;
  int rg = b0.rg_count;
  BigP g0;
  if (g0_plan(p, g0) && g0.rg_count > rg) rg = g0.rg_count;
  return (size_t)rg * p.N * p.Q * p.Wn * sizeof(float);
}

int eps_bwd_dx_bigcore(const void* x, const void* core, const void* dY, void* dX, void* ws,
                       size_t ws_bytes, const EpsP& p, int dtype, int precision, hipStream_t st,
                       const void* zsaved, size_t zsaved_bytes) {
  if (dtype != DCTN_F32 || precision != DCTN_PREC_EXACT || !bigcore_wanted(p)) return DCTN_ERR_UNSUPPORTED;
  const long long total = (long long)p.C * p.B * p.H * p.W * p.Q;
  const unsigned g2 = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (zsaved) {
    // the forward kept Z: half 0 by the GEMM G0, half 1 by one pass over Z
    BigP bf, b0;
    Dp1P d;
    size_t lds1, zbytes;
    if (fill_big(bf, p, MODE_FWD) && dp1_plan(p, bf, d, lds1, zbytes) && zsaved_bytes >= zbytes && g0_plan(p, b0)) {
      const size_t need = (size_t)b0.rg_count * p.N * p.Q * p.Wn * sizeof(float);
      if (!ws || ws_bytes < need) return DCTN_ERR_WORKSPACE;
      float* gxw = (float*)ws;
      int rc = dctn_bc::launch_g(MODE_G0, x, core, dY, gxw, b0, big_lds(b0), st);
      if (rc != DCTN_OK) return rc;
      rc = launch_dp1(x, zsaved, dY, gxw, d, lds1, st);
      if (rc != DCTN_OK) return rc == DCTN_ERR_UNSUPPORTED ? DCTN_ERR_LAUNCH : rc;   // (after a launch: no fall-through)
      hipLaunchKernelGGL(bigcore_gather_dx_k, dim3(g2), dim3(256), 0, st, (const float*)gxw, (float*)dX, p, b0.n0,
                         b0.rg_count, 1);
      DCTN_CHECK_LAUNCH();
      dctn_set_last_kernel("eps_bwd_mfma_bigcore_f32_savedz");
      return DCTN_OK;
    }
  }
  BigP b0, b1;
  if (!dfactor_plan(p, b0, b1)) return DCTN_ERR_UNSUPPORTED;
  const size_t need = (size_t)b0.rg_count * p.N * p.Q * p.Wn * sizeof(float);
  if (!ws || ws_bytes < need) return DCTN_ERR_WORKSPACE;
  float* gxw = (float*)ws;
  int rc = dctn_bc::launch_g(MODE_G0, x, core, dY, gxw, b0, big_lds(b0), st);
  if (rc != DCTN_OK) return rc;
  rc = dctn_bc::launch_g(MODE_G1, x, core, dY, gxw, b1, big_lds(b1), st);
  if (rc != DCTN_OK) return rc == DCTN_ERR_UNSUPPORTED ? DCTN_ERR_LAUNCH : rc;   // (after a launch: no fall-through)
  hipLaunchKernelGGL(bigcore_gather_dx_k, dim3(g2), dim3(256), 0, st, (const float*)gxw, (float*)dX, p, b0.n0,
                     b0.rg_count, b0.rg_count);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel("eps_bwd_mfma_bigcore_f32");
  return DCTN_OK;
}


// room for one dCore slice per window chunk: the chunks are then summed in a fixed order (bit-reproducible dCore)
size_t eps_bwd_dcore_bigcore_workspace(const EpsP& p, int dtype, int precision) {
  DcoreP d;
  long long tiles, chunks;
  size_t lds;
  if (!dcore_plan(p, dtype, precision, d, tiles, chunks, lds) || chunks < 2) return 0;
  return (size_t)chunks * p.R * p.O * sizeof(float);
}

int eps_bwd_dcore_bigcore(const void* x, const void* dY, void* dCore, const EpsP& p, int dtype,
                          int precision, hipStream_t st, void* ws, size_t ws_bytes) {
  DcoreP d;
  long long tiles, chunks;
  size_t lds;
  if (!dcore_plan(p, dtype, precision, d, tiles, chunks, lds)) return DCTN_ERR_UNSUPPORTED;
  const size_t slices = (size_t)chunks * p.R * p.O * sizeof(float);
  float* target = (float*)dCore;
  const bool small = p.N * p.Q <= 40 && d.OP <= 8;
  if (!dctn_lds_optin(small ? (const void*)BC_DCORE_KERNEL<10, 2> : (const void*)BC_DCORE_KERNEL<20, 8>, lds))
    return DCTN_ERR_UNSUPPORTED;
  if (chunks < 2) {
    // one chunk: every element has one writer; (the kernel adds) start from zero
    if (dctn_zero_async(dCore, (size_t)p.R * p.O * sizeof(float), st) != DCTN_OK) return DCTN_ERR_LAUNCH;
  } else if (ws && ws_bytes >= slices) {
    d.part = (float*)ws;
  } else {
    // no room for the slices: float atomics in arrival order (the low bits of dCore then differ from run to run)
    if (dctn_zero_async(dCore, (size_t)p.R * p.O * sizeof(float), st) != DCTN_OK) return DCTN_ERR_LAUNCH;
  }
#define DC_LAUNCH(PX, PY)                                                                                  \
  hipLaunchKernelGGL((BC_DCORE_KERNEL<PX, PY>), dim3((unsigned)tiles, (unsigned)chunks), dim3(DC_THREADS), lds, st, \
                     (const float*)x, (const float*)dY, target, d)
  if (small) DC_LAUNCH(10, 2);
  else DC_LAUNCH(20, 8);
#undef DC_LAUNCH
  DCTN_CHECK_LAUNCH();
  if (d.part) {
    const long long n = (long long)p.R * p.O;
    const long long nt = (n + 3) / 4;
    const unsigned g = (unsigned)((nt + 255) / 256 < 4096 ? (nt + 255) / 256 : 4096);
    hipLaunchKernelGGL(bigcore_sum_slices_k, dim3(g), dim3(256), 0, st, (const float*)d.part, target, n, (int)chunks);
    DCTN_CHECK_LAUNCH();
  }
  dctn_set_last_kernel("eps_bwd_mfma_bigcore_f32");
  return DCTN_OK;
}
#endif  // BC_PART
