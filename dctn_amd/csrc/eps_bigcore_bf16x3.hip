// MFMA EPS kernels, family "bigcore bf16x3" (DCTN_PREC_SPLIT, "high"): the large-core family's GEMMs on
// v_mfma_f32_32x32x16_bf16.  Every float32 operand value v is carried as two bf16 values, hi = bf16_rn(v) and
// lo = bf16_rn(v - hi), and every product as hi*hi + hi*lo + lo*hi accumulated in float32: a relative error of about
// 3 * 2^-18 per product, where "bf16" (one plane) has 2^-8.  The kernels are eps_bigcore_k.h compiled with BC_X3 = 1:
// the same staging, tables, epilogues, Z layout and fixed-order slice sums as the exact family (eps_bigcore.hip); only
// the matrix products differ:
//   - the core tile is loaded as float32 (the same HBM bytes as the exact path, no pre-split copy, no extra workspace)
//     and split into hi / lo bf16 planes [row][k] while it is written to LDS;
//   - the generated operand is formed in float32 from the same digit tables and split in registers;
//   - the dCore product splits both generated operands.
// A shape the plans below decline stays on the exact family (capi.hip routes it there with the policy read as exact).
#ifdef DCTN_STAMPS
#undef DCTN_STAMPS   // the phase stamps are a diagnostic of the exact kernels only
#endif
#define BC_X3 1
#include "eps_bigcore_k.h"

namespace {

bool x3_ok(const EpsP& p, int dtype, int precision) {
  return dtype == DCTN_F32 && precision == DCTN_PREC_SPLIT && bigcore_wanted(p);
}

bool x3_fwd_plan(const EpsP& p, BigP& b) {
  return fill_big(b, p, MODE_FWD) && big_lds(b) <= (size_t)dctn_lds_wg_max();
}

bool x3_dcore_plan(const EpsP& p, DcoreP& d, long long& tiles, long long& chunks, size_t& lds) {
  // the dCore kernel's plan (tiles, window chunks, tables) is the exact kernel's: ask it as for an exact call
  return dcore_plan(p, DCTN_F32, DCTN_PREC_EXACT, d, tiles, chunks, lds);
}

// a shape is the family's when every product of its forward and backward plans here: it never runs half bf16x3
bool x3_covers(const EpsP& p) {
  BigP bf, b0, b1;
  DcoreP d;
  long long tiles, chunks;
  size_t lds;
  return x3_fwd_plan(p, bf) && dfactor_plan(p, b0, b1) && x3_dcore_plan(p, d, tiles, chunks, lds);
}

void sum_slices(const float* part, float* out, long long n, int groups, unsigned max_grid, hipStream_t st) {
  const long long nt = (n + 3) / 4;
  const unsigned g = (unsigned)((nt + 255) / 256 < max_grid ? (nt + 255) / 256 : max_grid);
  hipLaunchKernelGGL(bigcore_sum_slices_k, dim3(g), dim3(256), 0, st, part, out, n, groups);
}

}  // namespace

bool eps_bf16x3_covers(const EpsP& p, int dtype, int precision) {
  return x3_ok(p, dtype, precision) && x3_covers(p);
}

size_t eps_fwd_bf16x3_workspace(const EpsP& p, int dtype, int precision) {
  BigP b;
  if (!eps_bf16x3_covers(p, dtype, precision) || !x3_fwd_plan(p, b)) return 0;
  choose_row_groups(b, BC_NT_FWD, BC_MAX_RG, big_lds(b));
  return b.rg_count > 1 ? (size_t)b.rg_count * p.Wn * p.O * sizeof(float) : 0;
}

size_t eps_bf16x3_saved_bytes(const EpsP& p, int dtype, int precision) {
  BigP b, b0;
  Dp1P d;
  size_t lds, zbytes;
  if (!eps_bf16x3_covers(p, dtype, precision) || !x3_fwd_plan(p, b) || !g0_plan(p, b0)) return 0;
  return dp1_plan(p, b, d, lds, zbytes) ? zbytes : 0;
}

int eps_fwd_bf16x3(const void* x, const void* core, void* out, void* ws, size_t ws_bytes, const EpsP& p, int dtype,
                   int precision, hipStream_t st, void* zsave) {
  if (!eps_bf16x3_covers(p, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  BigP b;
  if (!x3_fwd_plan(p, b)) return DCTN_ERR_UNSUPPORTED;
  const size_t lds = big_lds(b);
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
    case 3: rc = launch_fwd<3>(x, core, dst, b, lds, st); break;
    case 4: rc = launch_fwd<4>(x, core, dst, b, lds, st); break;
    case 5: rc = launch_fwd<5>(x, core, dst, b, lds, st); break;
  }
  if (rc != DCTN_OK) return rc;
  if (b.rg_count > 1) {
    sum_slices((const float*)ws, (float*)out, p.Wn * p.O, b.rg_count, 2048, st);
    DCTN_CHECK_LAUNCH();
  }
  dctn_set_last_kernel(zsave ? "bf16x3_eps_fwd_bigcore_saving" : "bf16x3_eps_fwd_bigcore");
  return DCTN_OK;
}

size_t eps_bwd_dfactor_bf16x3_workspace(const EpsP& p, int dtype, int precision) {
  BigP b0, b1, g0;
  if (!eps_bf16x3_covers(p, dtype, precision) || !dfactor_plan(p, b0, b1)) return 0;
  int rg = b0.rg_count;
  if (g0_plan(p, g0) && g0.rg_count > rg) rg = g0.rg_count;
  return (size_t)rg * p.N * p.Q * p.Wn * sizeof(float);
}

// dX: G0 and G1 (or G0 and the dP1 pass over the saved Z) into per-window factor gradients, then the exact family's gather
int eps_bwd_dx_bf16x3(const void* x, const void* core, const void* dY, void* dX, void* ws, size_t ws_bytes, const EpsP& p,
                      int dtype, int precision, hipStream_t st, const void* zsaved, size_t zsaved_bytes) {
  if (!eps_bf16x3_covers(p, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  const long long total = (long long)p.C * p.B * p.H * p.W * p.Q;
  const unsigned g2 = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  float* gxw = (float*)ws;
  if (zsaved) {
    BigP bf, b0;
    Dp1P d;
    size_t lds1, zbytes;
    if (x3_fwd_plan(p, bf) && dp1_plan(p, bf, d, lds1, zbytes) && zsaved_bytes >= zbytes && g0_plan(p, b0)) {
      const size_t need = (size_t)b0.rg_count * p.N * p.Q * p.Wn * sizeof(float);
      if (!ws || ws_bytes < need) return DCTN_ERR_WORKSPACE;
      int rc = launch_tbl<MODE_G0, BC_NT_G, 0>(x, core, dY, gxw, b0, big_lds(b0), st);
      if (rc != DCTN_OK) return rc;
      rc = launch_dp1(x, zsaved, dY, gxw, d, lds1, st);
      if (rc != DCTN_OK) return rc == DCTN_ERR_UNSUPPORTED ? DCTN_ERR_LAUNCH : rc;   // (after a launch: no fall-through)
      hipLaunchKernelGGL(bigcore_gather_dx_k, dim3(g2), dim3(256), 0, st, (const float*)gxw, (float*)dX, p, b0.n0,
                         b0.rg_count, 1);
      DCTN_CHECK_LAUNCH();
      dctn_set_last_kernel("bf16x3_eps_bwd_bigcore_savedz");
      return DCTN_OK;
    }
  }
  BigP b0, b1;
  if (!dfactor_plan(p, b0, b1)) return DCTN_ERR_UNSUPPORTED;
  const size_t need = (size_t)b0.rg_count * p.N * p.Q * p.Wn * sizeof(float);
  if (!ws || ws_bytes < need) return DCTN_ERR_WORKSPACE;
  int rc = launch_tbl<MODE_G0, BC_NT_G, 0>(x, core, dY, gxw, b0, big_lds(b0), st);
  if (rc != DCTN_OK) return rc;
  rc = launch_tbl<MODE_G1, BC_NT_G, 0>(x, core, dY, gxw, b1, big_lds(b1), st);
  if (rc != DCTN_OK) return rc == DCTN_ERR_UNSUPPORTED ? DCTN_ERR_LAUNCH : rc;
  hipLaunchKernelGGL(bigcore_gather_dx_k, dim3(g2), dim3(256), 0, st, (const float*)gxw, (float*)dX, p, b0.n0,
                     b0.rg_count, b0.rg_count);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel("bf16x3_eps_bwd_bigcore");
  return DCTN_OK;
}

size_t eps_bwd_dcore_bf16x3_workspace(const EpsP& p, int dtype, int precision) {
  DcoreP d;
  long long tiles, chunks;
  size_t lds;
  if (!eps_bf16x3_covers(p, dtype, precision) || !x3_dcore_plan(p, d, tiles, chunks, lds) || chunks < 2) return 0;
  return (size_t)chunks * p.R * p.O * sizeof(float);
}

// dCore: one slice per window chunk, summed in a fixed order (no float atomics: without room for the slices the call
// returns DCTN_ERR_WORKSPACE)
int eps_bwd_dcore_bf16x3(const void* x, const void* dY, void* dCore, const EpsP& p, int dtype, int precision,
                         hipStream_t st, void* ws, size_t ws_bytes) {
  if (!eps_bf16x3_covers(p, dtype, precision)) return DCTN_ERR_UNSUPPORTED;
  DcoreP d;
  long long tiles, chunks;
  size_t lds;
  if (!x3_dcore_plan(p, d, tiles, chunks, lds)) return DCTN_ERR_UNSUPPORTED;
  const size_t slices = (size_t)chunks * p.R * p.O * sizeof(float);
  const bool small = p.N * p.Q <= 40 && d.OP <= 8;
  if (!dctn_lds_optin(small ? (const void*)BC_DCORE_KERNEL<10, 2> : (const void*)BC_DCORE_KERNEL<20, 8>, lds))
    return DCTN_ERR_UNSUPPORTED;
  if (chunks < 2) {
    // one chunk: every element has one writer; (the kernel adds) start from zero
    if (dctn_zero_async(dCore, (size_t)p.R * p.O * sizeof(float), st) != DCTN_OK) return DCTN_ERR_LAUNCH;
  } else {
    if (!ws || ws_bytes < slices) return DCTN_ERR_WORKSPACE;
    d.part = (float*)ws;
  }
  if (small)
    hipLaunchKernelGGL((BC_DCORE_KERNEL<10, 2>), dim3((unsigned)tiles, (unsigned)chunks), dim3(DC_THREADS), lds, st,
                       (const float*)x, (const float*)dY, (float*)dCore, d);
  else
    hipLaunchKernelGGL((BC_DCORE_KERNEL<20, 8>), dim3((unsigned)tiles, (unsigned)chunks), dim3(DC_THREADS), lds, st,
                       (const float*)x, (const float*)dY, (float*)dCore, d);
  DCTN_CHECK_LAUNCH();
  if (d.part) {
    sum_slices(d.part, (float*)dCore, (long long)p.R * p.O, (int)chunks, 4096, st);
    DCTN_CHECK_LAUNCH();
  }
  dctn_set_last_kernel("bf16x3_eps_bwd_bigcore");
  return DCTN_OK;
}
