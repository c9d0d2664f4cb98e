"""Every launch plan on a device of 2 and of 5 CUs (DCTN_DEVICE_LIMITS, capi.hip:25): many turns per workgroup, exact.

Almost every family sizes its grid from the CU count (`dctn_dev().cus`, `dctn_resident_wgs`, `resident_blocks`).  On the
256-CU card the small shapes of the exact-input tests fit one round: a persistent wave takes one unit of work, a
workgroup sums one sample chunk, a planner takes its "plenty of CUs" branch.  With 2 CUs the same small shapes put every
plan into its many-turns or scarce-CU regime; with 5 the divisions leave remainders (`cus / npg`, a grid that is no
multiple of 8).  The comparisons are those of tests/test_gpu_exact.py - bit for bit, whatever the summation order - so a
dropped, duplicated or misplaced sample, chunk, tile or band is a mismatch.

`PLANS` is the table: one row per (family, shape) with the planner it is for (`site`), the comparison (`run`) and the
regime the shape reaches, restated from the planner in Python.  A regime statement is one of
  * turns(units, cap): the planner deals `units` (samples, chunks, tiles, windows groups) over at most `cap(cus)` workers.
    Held to: units >= 2 * cap(2) + 1 (three turns for the fullest worker), units % cap(2) != 0 (a ragged last turn) and
    units <= cap(256) (the card as it is never gets there at this shape).  Where the cap depends on an occupancy the host
    cannot restate (registers), `cap` is the largest the planner may pick and `cap_min` the smallest; the raggedness is
    then held for every `caps(2)` candidate.
  * alternative(holds): a branch of the planner, true at 2 CUs and false at 256.
tests/test_host_small_device.py asserts every statement on any machine and holds the sources to this table: a file
with a CU-dependent call site and no row fails there.

The halves families (eps_halves.hip, float64 / float32 / bf16) read neither the CU count nor the resident-workgroup
count: their grids are functions of the shape alone, so they have no row (their boundary cases run below all the same).

The library reads the limits once per process, so each limit is one child process (the protocol of
tests/test_gpu_boundary.py); the two children run one after the other and are memoised.  In a child, any exception other
than AssertionError / NotImplementedError - a launch failure, a HIP error, anything unforeseen - ends the loop at once;
the remaining cases are reported as not run and fail here.  Nothing is retried."""
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

LDS = 160 * 1024                       # the card's own LDS per CU: only the CU count moves
LIMITS = ("2,%d" % LDS, "5,%d" % LDS)
CARD = 256                             # the CU count every shape below must NOT be a many-turns shape for

# One clean run of a child on an MI355X - interpreter start, imports, all of PLANS and the 16 boundary cases: 4.4 s of wall
# time inside the whole suite (8.7 s for the two), 4.7 s as the first thing a fresh machine runs (9.3 s for the two); the
# cases themselves 2.7 s at 2 CUs and 2.2 s at 5 CUs, the float64 oracles on the CPU included.  Five times the 4.7 s.
CHILD_TIMEOUT = 24

# (case name, CUs) -> the line that declines: rows whose family hands the shape to another one under the limit
HANDED = {}


def ceil_div(a, b):
    return -(-a // b)


def resident_wgs(cus, lds_bytes, lo, hi):
    """capi.hip:40 dctn_resident_wgs"""
    per_cu = LDS // lds_bytes if lds_bytes else hi
    return cus * min(max(per_cu, lo), hi)


def turns(what, units, cap, cap_min=None, caps=None):
    return {"kind": "turns", "what": what, "units": units, "cap": cap, "cap_min": cap_min or cap,
            "caps": caps or (lambda cus: [cap(cus)])}


def alternative(what, holds):
    return {"kind": "alternative", "what": what, "holds": holds}


def check_regime(r):
    """The conditions of the module docstring, for one statement; tests/test_host_small_device.py calls it per row."""
    if r["kind"] == "turns":
        units = r["units"]
        assert units >= 2 * r["cap"](2) + 1, (r["what"], units, r["cap"](2))
        for c in r["caps"](2):
            assert units % c != 0, (r["what"], units, c)
        assert units <= r["cap_min"](CARD), (r["what"], units, r["cap_min"](CARD))
    else:
        assert r["kind"] == "alternative"
        assert r["holds"](2) is True and r["holds"](CARD) is False, r["what"]


def _exact():
    from tests import test_gpu_exact as E
    return E


BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ EPS, bf16 registers
def q2reg_row(C, K, H, W, B, O):
    P = (H - K + 1) * (W - K + 1)
    npg = ceil_div(P, 64)                                          # eps_mfma.hip:2184

    def run(cus):
        E = _exact()
        core, x, dy = E.eps_operands(C, K, 2, O, B, H, W, BF16, seed=C + B + H + W + K + O)
        E.run_eps(core, x, dy, BF16, need_dx=False, fwd="eps_fwd_mfma_q2reg", bwd="eps_bwd_mfma_q2reg", rounding="q2reg",
                  tag=f"q2reg at {cus} CUs")

    # plan_waves (eps_mfma.hip:2214): chunks = target / npg sample chunks, spc = ceil(B / chunks) samples per chunk;
    # target = FWD_BLOCKS_PER_CU * cus * 4 waves forward (:2235), cus * BWD_WAVES backward (:2263)
    return {"name": f"q2reg_bf16_C{C}K{K}_{H}x{W}_B{B}_O{O}", "site": "eps_mfma.hip: plan_waves (fwd_launch_t, bwd_launch_t)",
            "run": run,
            "regime": [turns("forward: samples over sample chunks", B, lambda cus: max(4 * cus * 4 // npg, 1)),
                       turns("dCore: samples over sample chunks", B, lambda cus: max(cus * 8 // npg, 1))]}


# ------------------------------------------------------------------------------------------------ fused head, bf16
def plan_grouped(B, npg, cus):
    """eps_mfma.hip:2300 plan_grouped -> (spc, nchunks, ncb, blocks); blocks == 0: declined"""
    if npg > cus:
        return 0, 0, 0, 0
    ncb = min(cus // npg, ceil_div(B, 8))
    spc = ceil_div(B, ncb * 8)
    nchunks = ceil_div(B, spc)
    ncb = ceil_div(nchunks, 8)
    blocks = ncb * npg
    if blocks >= 8:
        blocks = ceil_div(blocks, 8) * 8
    return spc, nchunks, ncb, (blocks if blocks <= cus else 0)


def head_bf16_row(B, mode, size=12, C=1, K=3, O=4, Cout=10):
    P = (size - K + 1) ** 2
    npg = ceil_div(P, 64)

    def run(cus):
        E = _exact()
        core, x, w, bias, g = E.head_operands(C, K, size, size, B, O, Cout, BF16, seed=C + K + size + B + O + Cout)
        fused, ffwd, blocked = E.HEAD_MODES[mode]
        E.run_head(core, x, w, bias, g, BF16, fused=fused, fused_fwd=ffwd, blocked=blocked, fwd="eps_head_fwd_mfma_q2reg",
                   bwd="eps_head_bwd_mfma_q2reg", tag=f"{mode} B={B} at {cus} CUs")

    regime = [turns("backward: samples over the wave slots of the chunk blocks", B, lambda cus: max(cus // npg, 1) * 8)]
    if B % 2:   # eps_mfma.hip:2436 nwg = min(B, cus): the forward's workgroups take several samples each
        regime.append(turns("forward: samples over workgroups", B, lambda cus: cus))
    return {"name": f"head_bf16_{mode}_B{B}", "site": "eps_mfma.hip: plan_grouped, fwd_head_launch_t (nwg = min(B, cus))",
            "run": run, "regime": regime, "grouped": (B, npg)}


# ------------------------------------------------------------------------------------------------ EPS and head, float32 registers
def q2f32_row(B, head, C=1, K=3, H=12, W=12, O=4, Cout=10):
    npg = ceil_div((H - K + 1) * (W - K + 1), 64)

    def run(cus):
        E = _exact()
        if head:
            core, x, w, bias, g = E.head_operands(C, K, H, W, B, O, Cout, F32, seed=C + K + H + W + B + O + Cout)
            E.run_head(core, x, w, bias, g, F32, fused=True, fused_fwd=True, blocked=False, fwd="eps_head_fwd_q2f32",
                       bwd="eps_head_bwd_q2f32", tag=f"q2f32 head B={B} at {cus} CUs")
        else:
            core, x, dy = E.eps_operands(C, K, 2, O, B, H, W, F32, seed=C + K + H + W + B + O)
            E.run_eps(core, x, dy, F32, need_dx=False, fwd="eps_fwd_q2f32", bwd="eps_bwd_q2f32", tag=f"q2f32 B={B} at {cus} CUs")

    # plan_bwd (eps_q2f32.hip:880): ncb = min(cus / npg, ceil(B / QF_WAVES)) chunk blocks; with few CUs the first term binds
    # (2 CUs: ncb = 1; 5 CUs: ncb = 2 and one CU idle) and every wave of a chunk block takes several samples
    bwd = alternative("backward: the chunk blocks are bounded by the CU count, not by the batch",
                      lambda cus: cus // npg < ceil_div(B, 8))
    if head:   # fwd_head_launch_t (eps_q2f32.hip:862): nwg = min(B, cus), spc = ceil(B / nwg)
        fwd = turns("fused forward: samples over workgroups", B, lambda cus: cus)
    else:      # fwd_launch_t (eps_q2f32.hip:828): nwg = min(B, 2 * cus)
        fwd = turns("forward: samples over workgroups", B, lambda cus: 2 * cus)
    return {"name": f"q2f32_{'head' if head else 'eps'}_B{B}", "run": run, "regime": [fwd, bwd],
            "site": "eps_q2f32.hip: " + ("fwd_head_launch_t, plan_bwd" if head else "fwd_launch_t, plan_bwd")}


# ------------------------------------------------------------------------------------------------ EPS, large cores
def bigcore_row(high, C=1, B=3, H=9, W=9, Q=4, K=3, O=6):
    N = K * K * C
    n0 = (N + 1) // 2
    n1 = N - n0
    A, BN = Q ** n0, Q ** n1
    Wn = B * (H - K + 1) * (W - K + 1)
    # dcore_plan (eps_bigcore_k.h:1659-1672): tiles of 128 rows x 512 columns, chunks = cus / tiles window chunks of whole
    # 128-window pieces
    tiles = ceil_div(A, 2 * 2 * 32) * ceil_div(BN * O, 4 * 4 * 32)

    def chunks(cus):
        c = min(max(cus // tiles, 1), ceil_div(Wn, 128))
        wpb = ceil_div(ceil_div(Wn, c), 128) * 128
        return ceil_div(Wn, wpb)

    # choose_row_groups (eps_bigcore_k.h:1249-1273), forward: Wn / 256 window blocks x up to min(row tiles, 32) row groups
    # against the resident workgroups; where they do not fit one round the planner keeps several row tiles per group
    fwd_lds = ((N * Q + 1) * 256 + 2 * 64 * 2 * 33) * 4           # big_lds (:1497), forward, float32 staging
    mtiles = ceil_div(BN * O, 32)                                  # fill_big (:1192): rows = BN * O

    def run(cus):
        import dctn_amd
        E = _exact()
        core, x, dy = E.eps_operands(C, K, Q, O, B, H, W, F32, seed=C + B + H + W + Q + K + O)
        names = ("bf16x3_eps_fwd_bigcore_saving", "bf16x3_eps_bwd_bigcore_savedz") if high else (
            "eps_fwd_mfma_bigcore_f32_saving", "eps_bwd_mfma_bigcore_f32_savedz")
        dctn_amd.set_float32_matmul_precision("high" if high else "exact")
        try:
            with E.keep_gemm_result(True):
                E.run_eps(core, x, dy, F32, fwd=names[0], bwd=names[1], tag=f"bigcore {'high ' if high else ''}at {cus} CUs")
        finally:
            dctn_amd.set_float32_matmul_precision("exact")

    regime = [alternative("dCore: one window chunk (more output tiles than CUs)", lambda cus: chunks(cus) == 1)]
    if not high:   # (the bf16x3 build stages other planes: its LDS figure is not restated)
        regime.append(alternative("forward: window blocks x row tiles exceed the resident workgroups",
                                  lambda cus: ceil_div(Wn, 256) * min(mtiles, 32) > resident_wgs(cus, fwd_lds, 1, 8)))
    return {"name": "bigcore_" + ("bf16x3_high" if high else "f32"), "run": run, "regime": regime,
            "site": "eps_bigcore_k.h: choose_row_groups, dcore_plan (eps_bigcore.hip, eps_bigcore_bf16x3.hip)"}


# ------------------------------------------------------------------------------------------------ ConvSBS
SNAKE9 = ((0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2))
MID2 = (1, 1, 1, 1, 2, 1, 1, 1, 1)


def reg_band_search(H, W, max_h, max_w, B, cus):
    """convsbs_reg.hip:1364-1379 (and :1432-1447, the many-valued string): (bands, which break ended the search).  The LDS
    test of :1375 is left out: the shapes here are far below it."""
    Ho, Wo = H - max_h, W - max_w
    for nb in range(1, H + 1):
        br = ceil_div(H, nb)
        bands = ceil_div(H, br)
        maxwin = 0
        for b2 in range(bands):
            r0 = b2 * br
            r1 = min(r0 + br, H)
            wr0, wr1 = max(r0 - max_h, 0), min(r1, Ho)
            maxwin = max(maxwin, (wr1 - wr0) * Wo if wr1 > wr0 else 0)
        if maxwin <= 512 and B * bands >= cus:
            return bands, "enough workgroups"
        if maxwin <= 256:
            return bands, "finest useful"
    return 0, "none"


def sbs_reg_row(outs, C, q, B=3, H=20, W=20):
    def run(cus):
        E = _exact()
        E.run_sbs(E.sbs_spec(SNAKE9, (1,) + (4,) * 8, outs, C, q), B, H, W, F32, B + H + W, fwd="convsbs_fwd_reg_f32",
                  bwd="convsbs_bwd_reg_f32", tag=f"reg at {cus} CUs")

    return {"name": f"sbs_reg_o{max(outs)}_C{C}q{q}_B{B}_{H}x{W}", "run": run,
            "site": "convsbs_reg.hip: sr_fill / sm_fill band search (B * bands >= cus)",
            "regime": [alternative("the band search stops at the first plan with a workgroup per CU: coarser bands",
                                   lambda cus: reg_band_search(H, W, 2, 2, B, cus)[1] == "enough workgroups")]}


def band_fwd_lds(qc):
    return (8 * qc * 256 + 128 + 8 * 2 * 9 * 16 * 4) * 4           # convsbs_band.hip:1248


def sbs_band_row(r, B, H, W, C=1, q=3):
    Ho, Wo = H - 2, W - 2
    units = ceil_div(ceil_div(B * Ho * Wo, 16), 8)                 # convsbs_band.hip:1247-1249: 8 tiles of 16 windows per workgroup

    def run(cus):
        E = _exact()
        E.run_sbs(E.sbs_spec(SNAKE9, (1,) + (r,) * 8, MID2, C, q), B, H, W, F32, B + H + W + r, fwd="convsbs_fwd_band_f32",
                  bwd="convsbs_bwd_band_f32", tag=f"band r={r} at {cus} CUs")

    if units == 1:
        # bd_plan (convsbs_band.hip:1134-1137): nb = ceil(cus / B) bands per image, at most Ho / max_h; one band has no shared
        # pixel rows (side_bytes == 0).  (The rows of such small bands fit the LDS test of :1141 at once.)  5 CUs: three bands.
        regime = [alternative("backward: one band per image", lambda cus: min(max(ceil_div(cus, B), 1), Ho // 2) == 1)]
    else:
        regime = [turns("forward: groups of 8 window tiles over persistent workgroups", units,
                        lambda cus: resident_wgs(cus, band_fwd_lds(q ** C), 1, 2))]   # :1250
    return {"name": f"sbs_band_r{r}_B{B}_{H}x{W}", "run": run, "regime": regime,
            "site": "convsbs_band.hip: bd_plan (nb = ceil(cus / B)), convsbs_fwd_band (resident workgroups)"}


def sbs_band_many_row(B, H, W, bond=16, C=1, q=3):
    units = ceil_div(ceil_div(B * (H - 2) * (W - 2), 16), 8)

    def run(cus):
        _exact().run_many_convsbs(bond, C, q, MID2, MID2, B, H, W)

    return {"name": f"sbs_band_many_r{bond}_B{B}_{H}x{W}", "run": run,
            "site": "convsbs_band.hip: convsbs_many_fwd_band (resident workgroups / strings), bd_plan_many",
            "regime": [turns("forward: groups of 8 window tiles over the persistent workgroups of each string", units,
                             lambda cus: resident_wgs(cus, band_fwd_lds(q ** C), 1, 2) // 2)]}   # convsbs_band.hip:1325


RING = (((0, 0), (0, 1), (1, 1), (1, 0)), (3, 4, 5, 6), (1, 3, 2, 4), 2, 2)   # tests/test_gpu_boundary.py sbs_ring, as an exact case


def sbs_mfma_row(B=3, H=38, W=41):
    pos, bonds, outs, C, q = RING
    units = ceil_div(ceil_div(B * (H - 1) * (W - 1), 32), 4)      # convsbs_mfma.hip:1362/1412, :1608/1615: 4 groups of 32 windows per workgroup

    def run(cus):
        E = _exact()
        E.run_sbs(E.sbs_spec(pos, bonds, outs, C, q), B, H, W, F32, B + H + W, fwd="convsbs_fwd_mfma_f32",
                  bwd="convsbs_bwd_mfma_f32", tag=f"mfma ring at {cus} CUs")

    # dctn_resident_wgs(lds, 2, 8) forward (:1413), (lds2, 1, 8) backward (:1618): the LDS plans are not restated, the
    # statement holds for every count of workgroups per CU the clamps allow
    return {"name": f"sbs_mfma_ring_B{B}_{H}x{W}", "run": run,
            "site": "convsbs_mfma.hip: convsbs_fwd_mfma_one, convsbs_bwd_mfma_one (resident workgroups)",
            "regime": [turns("window groups over persistent workgroups, forward and backward", units, lambda cus: 8 * cus,
                             cap_min=lambda cus: cus, caps=lambda cus: [cus * k for k in range(1, 9)])]}


def sbs_generic_row(B=3, H=29, W=29):
    bonds, outs, C, q = (1,) + (3,) * 8, MID2, 2, 2                # tests/test_gpu_exact.py GENERIC_SBS[0]
    # bwd_lds_plan (convsbs_generic.hip:384-395): 64 window columns per wave, one wave while the accumulators of all cores
    # stay below 4096 bytes (float64 here)
    acc_bytes = 8 * sum(o * (1 if i == 0 else bonds[i]) * (1 if i == 8 else bonds[i + 1]) * q ** C for i, o in enumerate(outs))
    assert acc_bytes < 4096
    units = ceil_div(B * (H - 2) * (W - 2), 64)                    # :504 ngroups = ceil(Wn / (cst - 1))

    def run(cus):
        E = _exact()
        E.run_sbs(E.sbs_spec(SNAKE9, bonds, outs, C, q), B, H, W, F64, B + H + W + 9, fwd="convsbs_fwd_generic",
                  bwd="convsbs_bwd_generic", tag=f"generic at {cus} CUs")

    return {"name": f"sbs_generic_bond3_B{B}_{H}x{W}", "run": run,
            "site": "convsbs_generic.hip: convsbs_bwd_generic_run (resident workgroups)",
            "regime": [turns("backward: groups of 64 windows over persistent workgroups", units, lambda cus: 8 * cus,
                             cap_min=lambda cus: cus, caps=lambda cus: [cus * k for k in range(1, 9)])]}   # :506 (lds, 1, 8)


# ------------------------------------------------------------------------------------------------ linear head, fold
def linear_head_row(B, F, Cout):
    def run(cus):
        _exact().run_linear_head(B, F, Cout, BF16)

    return {"name": f"linear_head_bf16_B{B}_F{F}_C{Cout}", "run": run, "site": "linear_head.hip: dctn_linear_head_fwd (head_fwd_k<16>)",
            "regime": [alternative("16 samples per workgroup (a last workgroup with fewer)",   # linear_head.hip:456
                                   lambda cus: B % 16 != 0 and ceil_div(B, 16) >= cus)]}


def fold_row(Wn, L):
    def run(cus):
        from tests.test_gpu_fuzz import test_logmatmulexp_fold16_all_chain_lengths
        test_logmatmulexp_fold16_all_chain_lengths(Wn, L)   # its own tolerances; windows 2 and Wn - 1 take the exact path

    # logmatmulexp.hip:1013/1021 (forward, 4 windows per workgroup of 256 lanes) and :842/843 (backward, LME_BWD_WAVES = 4):
    # blocks = min(ceil(Wn / 4), resident_blocks); the occupancy query gives 1 .. 8 workgroups of 256 lanes per CU
    regime = [turns("windows over persistent waves, four per workgroup", ceil_div(Wn, 4), lambda cus: 8 * cus,
                    cap_min=lambda cus: cus, caps=lambda cus: [cus * k for k in range(1, 9)])] if Wn > 4 * 33 else [
        # the short shape: a second turn only where a CU holds at most 4 workgroups; (257, 9) is the many-turns case
        alternative("more workgroups asked for than there are CUs", lambda cus: ceil_div(Wn, 4) > cus)]
    return {"name": f"fold16_Wn{Wn}_L{L}", "run": run, "site": "logmatmulexp.hip: resident_blocks (fold16 forward and backward)",
            "regime": regime}


# ------------------------------------------------------------------------------------------------ helper kernels
def _capped_by_cus(units, const):
    """min(cus, const) workgroups (batch_call.hip: batch_plan, for the three batch-source kernel files;
    core_dropout.hip:177): the CU count is the bound, and it binds"""
    return lambda cus: cus < const and units > cus


def helper_rows():
    def batches(cus):
        from tests import test_gpu_batches as T
        T.test_more_samples_than_waves_and_single_column_tables()
        T.test_raw_abi_u8_table(28, 1, 3, F32, "draw")
        T.test_raw_abi_rows(2104, BF16, "gather")

    def colour(cus):
        from tests import test_gpu_colour_source as T
        T.test_more_samples_than_the_launch_has_waves()
        T.test_raw_abi(36, 0, 3, 4, F32, "draw")

    def augment(cus):
        from tests import test_gpu_augment as T
        T.test_more_samples_than_the_launch_has_waves()
        T.test_raw_abi((36, 36, 3, 4), BF16)

    def dropout(cus):
        from tests.test_gpu_core_dropout import test_raw_abi_against_the_restatement_and_torch_on_the_cpu as t
        t(F32, 0.5, "several_workgroups")

    def run_state(cus):
        from tests.test_gpu_run_state import test_gather_of_16_regions_under_the_guarded_arena as t
        t(0xFF)

    def window_stats(cus):
        from tests.test_gpu_boundary import _limits_cases
        from tests.test_gpu_parity import test_window_statistics_kernel_against_reference_fixture_and_oracle as t
        t()
        torch.manual_seed(12)
        ok, _ = _limits_cases()["window_stats"]()   # 40 images of 28 x 28, K = 3: 27 040 windows
        assert ok

    from tests.test_gpu_run_state import REGIONS
    state_tiles = sum(ceil_div(nbytes, 4096) for nbytes, _, _ in REGIONS)                 # run_state.hip:192
    return [
        {"name": "batch_source", "site": "batch_call.hip: batch_plan (the grey and row kernels)", "run": batches,     # 2100 samples, 4 waves a workgroup
         "regime": [alternative("the grid cap is the CU count", _capped_by_cus(ceil_div(2100, 4), 256))]},
        {"name": "colour_source", "site": "batch_call.hip: batch_plan (the colour kernels)", "run": colour,   # 1100 samples
         "regime": [alternative("the grid cap is the CU count", _capped_by_cus(ceil_div(1100, 4), 256))]},
        {"name": "augment_source", "site": "batch_call.hip: batch_plan (the augmented kernels)", "run": augment,   # 1030 samples
         "regime": [alternative("the grid cap is the CU count", _capped_by_cus(ceil_div(1030, 4), 256))]},
        {"name": "core_dropout", "site": "core_dropout.hip: drop_launch", "run": dropout,       # 2051 blocks of 4 elements, 1024 lanes
         "regime": [alternative("the grid cap is the CU count", _capped_by_cus(ceil_div(1025 + 1026, 1024), 256))]},
        {"name": "run_state_gather", "site": "run_state.hip: state_launch", "run": run_state,   # :216-217: 4 tiles a pass, 2 * cus workgroups
         "regime": [turns("passes of 4 tiles over persistent workgroups", ceil_div(state_tiles, 4), lambda cus: 2 * cus)]},
        {"name": "window_stats", "site": "window_stats.hip: dctn_window_stats", "run": window_stats,   # :167-168
         "regime": [turns("blocks of 256 windows over 8 workgroups per CU", ceil_div(40 * 26 * 26, 256), lambda cus: 8 * cus)]},
    ]


PLANS = (
    # C1 K3 (N = 9 cores) and C2 K2 (N = 8), O = 4 and 2; 12 x 12 / 10 x 10: two position groups, so the family plans at 2 CUs
    [q2reg_row(1, 3, 12, 12, 37, 4), q2reg_row(1, 3, 12, 12, 37, 2), q2reg_row(2, 2, 10, 10, 37, 4), q2reg_row(2, 2, 10, 10, 37, 2)]
    # spc = 3, 4, 5, 7 at 2 CUs: skew 1, 1, 1, 2; both feature layouts
    + [head_bf16_row(B, mode) for B in (20, 29, 37, 50) for mode in ("fused_blocked4", "fused_rowmajor")]
    + [q2f32_row(B, head) for B in (9, 21) for head in (False, True)]
    + [bigcore_row(False), bigcore_row(True)]
    + [sbs_reg_row(MID2, 1, 3), sbs_reg_row((1, 1, 1, 1, 10, 1, 1, 1, 1), 2, 2)]
    + [sbs_band_row(8, 2, 10, 10), sbs_band_row(16, 2, 10, 10), sbs_band_row(8, 2, 26, 26), sbs_band_row(16, 2, 26, 26),
       sbs_band_many_row(2, 26, 26)]
    + [sbs_mfma_row(), sbs_generic_row()]
    + [linear_head_row(37, 3176, 10), linear_head_row(130, 200, 16)]
    + [fold_row(257, 9), fold_row(33, 5)]
    + helper_rows()
)
PLAN_NAMES = [row["name"] for row in PLANS]
assert len(set(PLAN_NAMES)) == len(PLAN_NAMES)
BOUNDARY_NAMES = ["eps_q2reg_bf16", "eps_q2f32", "eps_bigcore_f32", "eps_halves_f64", "eps_generic", "head_f32", "head_bf16",
                  "sbs_reg_r4", "sbs_band_r8", "sbs_band_r16", "sbs_band_many", "sbs_mfma", "sbs_generic", "fold",
                  "window_stats", "tn_inner"]   # the keys of tests/test_gpu_boundary._limits_cases(), in its order


# ------------------------------------------------------------------------------------------------ the child and the parent
def _child():
    """Child process: every row and every boundary case once; one JSON line.  Per case {"ok": true}, {"failed": message} (an
    assertion: a mismatch, another kernel than expected), {"declined": message} (NotImplementedError), {"error": message}
    (anything else: the loop ends there) or {"not_run": true}."""
    import ctypes
    import time

    import dctn_amd
    from dctn_amd import _lib
    from tests.test_gpu_boundary import _limits_cases

    cus, lds = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().dctn_device_limits(ctypes.byref(cus), ctypes.byref(lds)) == 0
    boundary = _limits_cases()
    assert list(boundary) == BOUNDARY_NAMES

    def boundary_run(name):
        def run(_cus):
            torch.manual_seed(sum(map(ord, name)))
            ok, names = boundary[name]()
            assert ok, f"outside the tolerance of tests/test_gpu_boundary.py on {names}"
            return names
        return run

    cases = [(row["name"], row["run"]) for row in PLANS] + [("boundary_" + n, boundary_run(n)) for n in BOUNDARY_NAMES]
    out, stopped = {}, False
    t0 = time.time()
    for name, run in cases:
        if stopped:
            out[name] = {"not_run": True}
            continue
        try:
            names = run(cus.value)
            torch.cuda.synchronize()
            out[name] = {"ok": True, "kernels": names or [dctn_amd.last_kernel()]}
        except AssertionError as e:
            out[name] = {"failed": str(e)[:600]}
        except NotImplementedError as e:
            out[name] = {"declined": str(e)[:300]}
        except BaseException as e:   # a launch failure, a HIP error, anything unforeseen: nothing more runs on this device
            out[name] = {"error": f"{type(e).__name__}: {str(e)[:600]}"}
            stopped = True
    print(json.dumps({"limits": [cus.value, lds.value], "seconds": round(time.time() - t0, 1), "cases": out}))


def _run_child(limits):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["DCTN_DEVICE_LIMITS"] = limits
    code = f"import sys; sys.path.insert(0, {root!r}); from tests.test_gpu_small_device import _child; _child()"
    try:
        res = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        return {"broken": f"the child did not end within {CHILD_TIMEOUT} s"}
    if res.returncode != 0:
        return {"broken": f"the child ended with status {res.returncode}: {res.stderr[-3000:]}"}
    return json.loads(res.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def _small_runs():
    """Both children, one after the other, once.  After a child that broke or reported an error nothing more is started."""
    runs, stop = {}, False
    for lim in LIMITS:
        if stop:
            runs[lim] = {"broken": "not started: the child before it broke or reported an error"}
            continue
        runs[lim] = _run_child(lim)
        stop = "broken" in runs[lim] or any("error" in r for r in runs[lim]["cases"].values())
    return runs


def _result(limits, name):
    run = _small_runs()[limits]
    assert "broken" not in run, run["broken"]
    assert run["limits"] == [int(limits.split(",")[0]), LDS], run["limits"]
    return run["cases"][name]


def _judge(limits, name, r):
    cus = int(limits.split(",")[0])
    assert "not_run" not in r, f"{name} at {cus} CUs was not run: an earlier case ended the child"
    assert "error" not in r, (name, cus, r["error"])
    assert "failed" not in r, (name, cus, r["failed"])
    if "declined" in r:
        assert (name, cus) in HANDED, f"{name} declined at {cus} CUs without an entry in HANDED: {r['declined']}"
        return
    assert r.get("ok") is True, (name, cus, r)


@pytest.mark.parametrize("name", PLAN_NAMES)
@pytest.mark.parametrize("limits", LIMITS, ids=["2cus", "5cus"])
def test_plan_on_a_small_device(limits, name):
    _judge(limits, name, _result(limits, name))


@pytest.mark.parametrize("name", BOUNDARY_NAMES)
@pytest.mark.parametrize("limits", LIMITS, ids=["2cus", "5cus"])
def test_boundary_case_on_a_small_device(limits, name):
    """The rounding-level oracle comparisons of tests/test_gpu_boundary.py on random inputs: the exact cases cannot see a
    rounding placed in the wrong spot of a multi-turn sum.  Same kernels as on the whole card, or an entry in HANDED."""
    from tests.test_gpu_boundary import _limits_run

    r = _result(limits, "boundary_" + name)
    _judge(limits, "boundary_" + name, r)
    cus = int(limits.split(",")[0])
    if "declined" not in r and ("boundary_" + name, cus) not in HANDED:
        assert not any("error" in c for run in _small_runs().values() for c in run["cases"].values()), "a child reported an error"
        full = _limits_run(None)["cases"][name]
        assert r["kernels"] == full["kernels"], (name, cus, r["kernels"], full["kernels"])
