"""Host checks of tests/test_gpu_small_device.py: every row of its `PLANS` table reaches the regime it claims - asserted
from the planners' rules restated there, at 2, 5 and 256 CUs, on any machine -, every source file with a CU-dependent call
site has a row (the idiom of tests/test_host_buffer_contract.py: a new planner cannot arrive without its few-CU case), and
the tile rule of logmatmulexp_gemm.hip, which no CU count selects, for the parameter sets of the factored-GEMM test."""
import glob
import os
import re

import pytest

from tests import test_gpu_small_device as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dctn_amd", "csrc")
CALL_SITE = re.compile(r"dctn_dev\(\)\.cus|dctn_resident_wgs\(|resident_blocks\(")

# files with such a call site that need no row, and why
EXEMPT = {
    "capi.hip": "defines dctn_dev() and dctn_resident_wgs(); its own kernels have fixed grids",
    "common.h": "the declaration of dctn_resident_wgs() only",
}


@pytest.mark.parametrize("row", S.PLANS, ids=S.PLAN_NAMES)
def test_every_row_reaches_its_regime(row):
    assert row["regime"], row["name"]
    for r in row["regime"]:
        S.check_regime(r)
        # 5 CUs is the uneven case: the statement must at least be computable there
        if r["kind"] == "turns":
            assert r["cap"](5) >= 1 and all(c >= 1 for c in r["caps"](5)) and r["cap_min"](5) >= 1
        else:
            assert r["holds"](5) in (True, False)
    assert callable(row["run"]) and re.match(r"[a-z0-9_]+\.(hip|h): ", row["site"]), row["site"]


# the rows, by name: one that leaves the table has to leave here too, in sight of a reviewer
ROWS = """q2reg_bf16_C1K3_12x12_B37_O4 q2reg_bf16_C1K3_12x12_B37_O2 q2reg_bf16_C2K2_10x10_B37_O4 q2reg_bf16_C2K2_10x10_B37_O2
head_bf16_fused_blocked4_B20 head_bf16_fused_rowmajor_B20 head_bf16_fused_blocked4_B29 head_bf16_fused_rowmajor_B29
head_bf16_fused_blocked4_B37 head_bf16_fused_rowmajor_B37 head_bf16_fused_blocked4_B50 head_bf16_fused_rowmajor_B50
q2f32_eps_B9 q2f32_head_B9 q2f32_eps_B21 q2f32_head_B21 bigcore_f32 bigcore_bf16x3_high
sbs_reg_o2_C1q3_B3_20x20 sbs_reg_o10_C2q2_B3_20x20 sbs_band_r8_B2_10x10 sbs_band_r16_B2_10x10 sbs_band_r8_B2_26x26
sbs_band_r16_B2_26x26 sbs_band_many_r16_B2_26x26 sbs_mfma_ring_B3_38x41 sbs_generic_bond3_B3_29x29
linear_head_bf16_B37_F3176_C10 linear_head_bf16_B130_F200_C16 fold16_Wn257_L9 fold16_Wn33_L5
batch_source colour_source augment_source core_dropout run_state_gather window_stats""".split()


def test_limits_and_protocol():
    assert S.LIMITS == ("2,163840", "5,163840") and S.CARD == 256 and S.CHILD_TIMEOUT <= 600
    assert S.PLAN_NAMES == ROWS and len(S.BOUNDARY_NAMES) == 16
    src = open(os.path.join(ROOT, "tests", "test_gpu_boundary.py")).read()
    body = src[src.index("    return {\n        \"eps_q2reg_bf16\""):]
    assert re.findall(r'^        "([a-z0-9_]+)": ', body, re.M) == S.BOUNDARY_NAMES
    for (name, cus), line in S.HANDED.items():
        assert cus in (2, 5) and (name in S.PLAN_NAMES or name[len("boundary_"):] in S.BOUNDARY_NAMES) and line


def test_the_regimes_of_the_issue():
    """The figures the rows were chosen for, from the restated planners."""
    # plan_grouped at 2 CUs, two position groups: spc 3, 4, 5, 7 -> skew (spc / 3, eps_mfma.hip:2295) 1, 1, 1, 2, so the old
    # and the young waves of a SIMD take different counts; fewer sample chunks than the 8 wave slots at B = 20 and 50
    got = {B: S.plan_grouped(B, 2, 2) for B in (20, 29, 37, 50)}
    assert [got[B][0] for B in (20, 29, 37, 50)] == [3, 4, 5, 7]
    assert [got[B][0] // 3 for B in (20, 29, 37, 50)] == [1, 1, 1, 2]
    assert got[20][1] == 7 and got[50][1] == 8 and got[37][1] == 8 and all(v[2] == 1 and v[3] == 2 for v in got.values())
    # 5 CUs: cus / npg = 2 chunk blocks, 4 workgroups on 5 CUs; 256: one sample per wave; npg > cus: declined
    assert S.plan_grouped(37, 2, 5) == (3, 13, 2, 4) and S.plan_grouped(37, 2, 256)[0] == 1 and S.plan_grouped(37, 3, 2)[3] == 0
    # the register family's band search: one band of 324 windows at 2 CUs, two bands of 180 on the card
    assert S.reg_band_search(20, 20, 2, 2, 3, 2) == (1, "enough workgroups")
    assert S.reg_band_search(20, 20, 2, 2, 3, 5) == (2, "enough workgroups")
    assert S.reg_band_search(20, 20, 2, 2, 3, 256) == (2, "finest useful")
    assert S.resident_wgs(2, S.band_fwd_lds(3), 1, 2) == 4 and S.resident_wgs(5, 0, 1, 8) == 40


def _files_with_call_sites():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        n = len(CALL_SITE.findall(open(path).read()))
        if n:
            found[os.path.basename(path)] = n
    return found


def test_every_cu_dependent_file_has_a_row():
    found = _files_with_call_sites()
    assert len(found) >= 15, found   # (17 until the three batch-source files got one planner, batch_call.hip)
    sites = " ".join(row["site"] for row in S.PLANS)
    named = set(re.findall(r"[a-z0-9_]+\.(?:hip|h)", sites))
    missing = sorted(set(found) - named - set(EXEMPT))
    assert not missing, f"files that read the CU count without a row in PLANS of tests/test_gpu_small_device.py: {missing}"
    gone = sorted((named | set(EXEMPT)) - set(found) - {"eps_bigcore.hip", "eps_bigcore_bf16x3.hip"})   # (they include eps_bigcore_k.h)
    assert not gone, f"rows or exemptions for files without a call site: {gone}"
    assert all(reason for reason in EXEMPT.values())


# ------------------------------------------------------------------ the GEMM tile rule no CU count selects
def gemm_tile(batch, M, N):
    """logmatmulexp_gemm.hip:298-301 gemm_plan: 64 x 64 tiles (lme_gemm_k<MODE, 2, 1>) when they fill the chip, else 32 x 32"""
    return 64 if S.ceil_div(M, 64) * S.ceil_div(N, 64) * batch >= 256 else 32


def gemm_tiles(nb, T, R, I):
    """forward C = T x I over R (:352), dA = T x R over I (:381), dB = R x I over T (:387)"""
    return gemm_tile(nb, T, I), gemm_tile(nb, T, R), gemm_tile(nb, R, I)


def test_gemm_plan_tiles_of_the_factored_gemm_cases():
    import ast

    src = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    m = re.search(r'@pytest\.mark\.parametrize\("nb,T,Rr,I", (\[.*?\])\)\ndef test_logmatmulexp_factored_gemm_and_exact_fallback', src, re.S)
    cases = ast.literal_eval(m.group(1))
    assert cases == [(1, 256, 256, 256), (3, 100, 70, 130), (2, 64, 16, 64), (5, 33, 40, 65), (64, 100, 100, 100)]
    assert [gemm_tiles(*c) for c in cases[:4]] == [(32, 32, 32)] * 4
    assert gemm_tiles(*cases[4]) == (64, 64, 64)
    # 2 x 2 ragged tiles (a 36-wide edge) x 64 batch elements = 256 exactly, a 4-element last k chunk of 32
    assert S.ceil_div(100, 64) ** 2 * 64 == 256 and 100 - 64 == 36 and 100 % 32 == 4
