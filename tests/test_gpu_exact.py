"""Bit-exact parity on exact inputs (tests/exact_inputs.py, DESIGN.md "Exact-input tests"): every operand on a
power-of-two grid inside the family's budget, so every kernel result equals the float64 oracle after the one final
rounding to the storage dtype - whatever the summation order, tiling, split count or atomics.  A dropped, duplicated or
misplaced window, sample, tile or column is a mismatch at any batch size; the tolerance tests elsewhere test rounding.

Every case asserts the kernel it ran (`dctn_amd.last_kernel()`), and `KERNELS` lists every EPS / head / ConvSBS kernel
name the library can report: tests/test_host_exact_inputs.py fails when a new one is missing here."""
import contextlib
import math

import pytest
import torch

import dctn_amd
import dctn_amd.eps_plus_linear as EPL
from dctn_amd import _lib as L
from dctn_amd import conv_sbs as CS
from dctn_amd.conv_sbs import ConvSBS, ManyConvSBS, matrix_core_sweep, wide_sweep
from dctn_amd.conv_sbs_spec import SBSSpecCore, SBSSpecString
from dctn_amd.eps import eps, eps_one_by_one, keep_gemm_result, output_sums_in_slices
from dctn_amd.pos2d import Pos2D
from oracle import ref_cpu as R
from tests import exact_inputs as X
from tests import guarded_buffers as G
from tests.test_gpu_convsbs_wide import FAILS_TODAY, FORCED, WIDE
from tests.test_gpu_fuzz import (BAND_CASES, BIGCORE_XO_CASES, F32_HALVES_CASES, F64_CASES, HEAD_CASES, MANY_CASES, MV_CASES,
                                 Q2F32_CASES, REG_CASES, SNAKE9, SNAKE9B, eps_cases, sbs_band_family_takes, sbs_mfma_cases,
                                 sbs_reg_family_takes)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# every EPS / fused-head / linear-head / ConvSBS kernel name of dctn_set_last_kernel, and where it is held exact
KERNELS = {
    "eps_fwd_generic": "test_eps_generic", "eps_bwd_generic": "test_eps_generic",
    "eps_fwd_mfma_q2reg": "test_eps_q2reg_bf16", "eps_bwd_mfma_q2reg": "test_eps_q2reg_bf16",
    "eps_fwd_q2f32": "test_eps_q2f32", "eps_bwd_q2f32": "test_eps_q2f32",
    "eps_fwd_mfma_bigcore_f32": "test_eps_bigcore_f32", "eps_fwd_mfma_bigcore_f32_saving": "test_eps_bigcore_f32",
    "eps_bwd_mfma_bigcore_f32": "test_eps_bigcore_f32", "eps_bwd_mfma_bigcore_f32_savedz": "test_eps_bigcore_f32",
    "eps_fwd_mfma_f64_halves": "test_eps_halves_f64", "eps_fwd_mfma_f64_halves_saving": "test_eps_halves_f64",
    "eps_bwd_mfma_f64_halves": "test_eps_halves_f64", "eps_bwd_mfma_f64_halves_savedz": "test_eps_halves_f64",
    "eps_fwd_mfma_f32_halves": "test_eps_halves_f32", "eps_fwd_mfma_f32_halves_saving": "test_eps_halves_f32",
    "eps_bwd_mfma_f32_halves": "test_eps_halves_f32", "eps_bwd_mfma_f32_halves_savedz": "test_eps_halves_f32",
    "eps_fwd_mfma_bf16_halves": "test_eps_halves_bf16", "eps_fwd_mfma_bf16_halves_saving": "test_eps_halves_bf16",
    "eps_bwd_mfma_bf16_halves": "test_eps_halves_bf16", "eps_bwd_mfma_bf16_halves_savedz": "test_eps_halves_bf16",
    "eps_head_fwd_mfma_q2reg": "test_head_bf16", "eps_head_bwd_mfma_q2reg": "test_head_bf16",
    "eps_head_fwd_q2f32": "test_head_f32", "eps_head_bwd_q2f32": "test_head_f32",
    "linear_head_fwd_mfma": "test_linear_head", "linear_head_fwd_generic": "test_linear_head",
    "linear_head_bwd": "test_linear_head", "linear_head_bwd_generic": "test_linear_head",
    "convsbs_fwd_reg_f32": "test_convsbs_reg", "convsbs_bwd_reg_f32": "test_convsbs_reg",
    "convsbs_fwd_band_f32": "test_convsbs_band", "convsbs_bwd_band_f32": "test_convsbs_band",
    "convsbs_fwd_mfma_f32": "test_convsbs_mfma", "convsbs_bwd_mfma_f32": "test_convsbs_mfma",
    "convsbs_fwd_generic": "test_convsbs_generic", "convsbs_bwd_generic": "test_convsbs_generic",
    "convsbs_bwd_wide_f32": "test_convsbs_wide", "convsbs_bwd_wide_f64": "test_convsbs_wide",
    "convsbs_bwd_wide_bf16": "test_convsbs_wide",
    "convsbs_many_fwd_reg_f32": "test_many_convsbs", "convsbs_many_bwd_reg_f32": "test_many_convsbs",
    "convsbs_many_fwd_band_f32": "test_many_convsbs", "convsbs_many_bwd_band_f32": "test_many_convsbs",
}

ACC = {torch.float64: torch.float64, torch.float32: torch.float32, torch.bfloat16: torch.float32}


def on_dev(t, arena=None):
    """Input placement: on the device - and, under a guarded arena (tests/guarded_buffers.py: the one given, else the active
    one), inside a guarded allocation with the same values and strides.  Without an arena: `t.to(DEV)`, as ever."""
    t = t.to(DEV)
    arena = arena if arena is not None else G.current()
    return t if arena is None else arena.place(t)


def strided_copy(t):
    """The same values behind a non-contiguous view (pixel rows no longer contiguous)."""
    return t.permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4)


def core_view(t):
    return t.reshape(X.decode_core_layout(t.shape))


# ------------------------------------------------------------------------------------------------ EPS
def run_eps(core64, x64, dy64, dtype, *, strided=False, need_dx=True, fn=eps, fwd=None, bwd=None, rounding=None, tag="",
            arena=None):
    """forward, dCore with dX (need_dx) or dCore alone, all exact against the oracle; returns the budget report."""
    N = core64.ndim - 1
    C = x64.shape[0]
    K = math.isqrt(N // C)
    mags = X.eps_mags(core64, x64, dy64)
    if not need_dx:
        mags.pop("dx")
    bf16 = X.eps_bf16_intermediates(core64, x64, dy64, rounding) if rounding else None
    report = X.check_budget(mags, ACC[dtype], bf16)
    X.assert_every_window_counts(X.eps_window_weights(x64, K, dy64), tag)
    want = R.eps_4step(core64, x64)
    dcore, dx = R.grads(R.eps_4step, [core64, x64], dy64)
    X.assert_nonzero(forward=want, dcore=dcore, **({"dx": dx} if need_dx else {}))
    xd = x64.to(dtype).to(DEV)
    if strided:
        xd = strided_copy(xd)
    xd = on_dev(xd, arena).requires_grad_(need_dx)
    cd = on_dev(core64.to(dtype), arena).requires_grad_(True)
    y = fn(cd, xd)
    kf = dctn_amd.last_kernel()
    if fwd is not None:
        assert kf == fwd, f"{tag}: forward ran {kf}, expected {fwd}"
    X.assert_exact(y, want, dtype, X.EPS_LAYOUT, f"{tag} forward [{kf}]")
    y.backward(on_dev(dy64.to(dtype), arena))
    kb = dctn_amd.last_kernel()
    if bwd is not None:
        assert kb == bwd, f"{tag}: backward ran {kb}, expected {bwd}"
    X.assert_exact(core_view(cd.grad), core_view(dcore), dtype, X.CORE_LAYOUT, f"{tag} dCore [{kb}]")
    if need_dx:
        X.assert_exact(xd.grad, dx, dtype, ("channel", "sample", "row", "col", "q"), f"{tag} dX [{kb}]")
    return report


def eps_operands(C, K, Q, O, B, H, W, dtype, seed, two_hot=True):
    N = K * K * C
    halves = dtype != torch.bfloat16 and N <= 9   # a 2^-1 pixel puts the grid at 2^-N: more factors, no halves
    x = X.pixels(C, B, H, W, Q, seed, two_hot=two_hot, halves=halves)
    core = X.eps_core(Q, N, O, seed + 1, vmax=8)
    dy = X.small_ints((B, H - K + 1, W - K + 1, O), seed + 2, 3, nonzero=True)
    return core, x, dy


GENERIC_CASES = [c for c in eps_cases() if c[2] ** (c[1] * c[1] * c[0]) <= 2 ** 12][:14]


@pytest.mark.parametrize("case", GENERIC_CASES, ids=lambda c: "C%dK%dQ%dO%dB%d_%dx%d_%s%s" % (
    c[0], c[1], c[2], c[3], c[4], c[5], c[6], str(c[7]).split(".")[1], "_strided" if c[8] else ""))
def test_eps_generic(case):
    """eps_one_by_one: the generic kernels (DCTN_OPT_GENERIC_KERNELS), one lane per window, split launches joined by fixed-order slice sums."""
    C, K, Q, O, B, H, W, dtype, strided = case
    core, x, dy = eps_operands(C, K, Q, O, B, H, W, dtype, seed=sum(case[:7]))
    run_eps(core, x, dy, dtype, strided=strided, fn=eps_one_by_one, fwd="eps_fwd_generic", bwd="eps_bwd_generic",
            tag="generic")


Q2REG_CASES = [(1, 7, 28, 28, 3, 4), (1, 70, 8, 8, 3, 4), (2, 5, 9, 7, 2, 4), (1, 3, 10, 10, 3, 1), (1, 3, 10, 10, 3, 2),
               (1, 3, 10, 10, 3, 3), (1, 3, 10, 10, 3, 6), (1, 3, 10, 10, 3, 8), (1, 2, 9, 9, 3, 10), (2, 3, 6, 6, 2, 16),
               (1, 1100, 7, 9, 3, 4)]


Q2REG_RUNS = [c + (False, dx) for c in Q2REG_CASES for dx in (False, True)] + [Q2REG_CASES[0] + (True, False),
                                                                                     Q2REG_CASES[2] + (True, False)]


@pytest.mark.parametrize("C,B,H,W,K,O,strided,need_dx", Q2REG_RUNS)
def test_eps_q2reg_bf16(C, B, H, W, K, O, strided, need_dx):
    """The bf16 register family (eps_mfma.hip).  With dX, dCore runs here (the dcore runs of the same shape pin it) and the
    input gradient on the generic kernels after it: that is the kernel reported last."""
    core, x, dy = eps_operands(C, K, 2, O, B, H, W, torch.bfloat16, seed=C + B + H + W + K + O)
    run_eps(core, x, dy, torch.bfloat16, strided=strided, need_dx=need_dx, fwd="eps_fwd_mfma_q2reg",
            bwd="eps_bwd_generic" if need_dx else "eps_bwd_mfma_q2reg",   # with dX: dCore here, then dX (the last) generic
            rounding="q2reg", tag="q2reg")


@pytest.mark.parametrize("C,K,H,W,B,O,Cout,strided", Q2F32_CASES)
def test_eps_q2f32(C, K, H, W, B, O, Cout, strided):
    """The exact-f32 register family (eps_q2f32.hip): forward and dCore (the input needs no gradient)."""
    core, x, dy = eps_operands(C, K, 2, O, B, H, W, torch.float32, seed=C + K + H + W + B + O)
    run_eps(core, x, dy, torch.float32, strided=strided, need_dx=False, fwd="eps_fwd_q2f32", bwd="eps_bwd_q2f32", tag="q2f32")


@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
@pytest.mark.parametrize("C,B,H,W,Q,K,O", BIGCORE_XO_CASES)
def test_eps_bigcore_f32(C, B, H, W, Q, K, O, keep):
    core, x, dy = eps_operands(C, K, Q, O, B, H, W, torch.float32, seed=C + B + H + W + Q + K + O)
    with keep_gemm_result(keep):
        run_eps(core, x, dy, torch.float32, fwd="eps_fwd_mfma_bigcore_f32" + ("_saving" if keep else ""),
                bwd="eps_bwd_mfma_bigcore_f32" + ("_savedz" if keep else ""), tag="bigcore")


def _halves(case, dtype, keep, name, opts=0, rounding=None):
    C, K, Q, O, B, H, W, strided = case
    core, x, dy = eps_operands(C, K, Q, O, B, H, W, dtype, seed=sum(case[:7]))
    with keep_gemm_result(keep), L.options(opts):
        run_eps(core, x, dy, dtype, strided=strided, fwd=f"eps_fwd_mfma_{name}_halves" + ("_saving" if keep else ""),
                bwd=f"eps_bwd_mfma_{name}_halves" + ("_savedz" if keep else ""), rounding=rounding, tag=f"{name} halves")
        # dCore alone (the input needs no gradient: nothing is kept)
        run_eps(core, x, dy, dtype, strided=strided, need_dx=False, fwd=f"eps_fwd_mfma_{name}_halves",
                bwd=f"eps_bwd_mfma_{name}_halves", rounding=rounding, tag=f"{name} halves, dCore alone")


@pytest.mark.parametrize("chunks", [0, L.OPT_SMALL_CHUNKS], ids=["whole", "small_chunks"])
@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
@pytest.mark.parametrize("case", F64_CASES, ids=lambda c: "C%dK%dQ%dO%dB%d_%dx%d%s" % (c[:7] + ("_strided" if c[7] else "",)))
def test_eps_halves_f64(case, keep, chunks):
    _halves(case, torch.float64, keep, "f64", chunks)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
@pytest.mark.parametrize("case", F32_HALVES_CASES, ids=lambda c: "C%dK%dQ%dO%dB%d_%dx%d%s" % (c[:7] + ("_strided" if c[7] else "",)))
def test_eps_halves_f32(case, keep, dtype):
    """float32 arithmetic; bf16 tensors outside the bf16 register family take it too (bf16 storage only)."""
    _halves(case, dtype, keep, "f32")


@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
def test_eps_halves_f32_small_chunks(keep):
    """OPT_SMALL_CHUNKS: 1 000 windows in chunks of 64, dCore summed over the chunks."""
    _halves((1, 3, 3, 2, 10, 12, 12, False), torch.float32, keep, "f32", L.OPT_SMALL_CHUNKS)


@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
def test_eps_halves_f32_preferred(keep):
    """OPT_F32_PREFER_HALVES: a shape of the large-core family (BIGCORE_XO_CASES, cfg3a's layer-2 core) that the two-halves
    path covers too runs there instead."""
    C, B, H, W, Q, K, O = 1, 2, 9, 9, 4, 3, 6
    assert (C, B, H, W, Q, K, O) in BIGCORE_XO_CASES
    _halves((C, K, Q, O, B, H, W, False), torch.float32, keep, "f32", L.OPT_F32_PREFER_HALVES)


@pytest.mark.parametrize("chunks", [0, L.OPT_SMALL_CHUNKS], ids=["whole", "small_chunks"])
@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
@pytest.mark.parametrize("C,B,H,W,Q,K,O", [(1, 5, 9, 8, 2, 4, 4), (1, 3, 7, 7, 4, 3, 6), (1, 7, 9, 10, 8, 2, 5),
                                           (1, 3, 10, 11, 4, 3, 3)])
def test_eps_halves_bf16(C, B, H, W, Q, K, O, keep, chunks):
    """bf16 two-halves GEMMs: rounded intermediates are the scaled operands (half-row x dY) and the kept Z'."""
    core, x, dy = eps_operands(C, K, Q, O, B, H, W, torch.bfloat16, seed=B + H + W + Q + K + O)
    with keep_gemm_result(keep), L.options(chunks):
        run_eps(core, x, dy, torch.bfloat16, fwd="eps_fwd_mfma_bf16_halves" + ("_saving" if keep else ""),
                bwd="eps_bwd_mfma_bf16_halves" + ("_savedz" if keep else ""), rounding="halves", tag="bf16 halves")


@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
def test_eps_f32_under_the_bf16_policy(keep):
    """float32 tensors under set_float32_matmul_precision("bf16"): a large core on the bf16 two-halves GEMMs, a
    register-family core on the bf16 register family; exact operands are bf16-exact, so the policy changes no bit."""
    core, x, dy = eps_operands(1, 4, 2, 4, 4, 9, 8, torch.bfloat16, seed=32)
    core2, x2, dy2 = eps_operands(1, 3, 2, 4, 6, 12, 12, torch.bfloat16, seed=33)
    dctn_amd.set_float32_matmul_precision("bf16")
    try:
        with keep_gemm_result(keep):
            run_eps(core, x, dy, torch.float32, fwd="eps_fwd_mfma_bf16_halves" + ("_saving" if keep else ""),
                    bwd="eps_bwd_mfma_bf16_halves" + ("_savedz" if keep else ""), rounding="halves", tag="bf16 policy, halves")
        run_eps(core2, x2, dy2, torch.float32, need_dx=False, fwd="eps_fwd_mfma_q2reg", bwd="eps_bwd_mfma_q2reg",
                rounding="q2reg", tag="bf16 policy, q2reg")
    finally:
        dctn_amd.set_float32_matmul_precision("exact")


@pytest.mark.parametrize("dtype,C,K,Q,O,B,H,W", [(torch.bfloat16, 1, 3, 2, 4, 37, 28, 28), (torch.float32, 1, 3, 2, 4, 9, 12, 12),
                                                 (torch.float32, 1, 2, 4, 5, 6, 7, 7), (torch.float64, 1, 3, 3, 2, 5, 9, 9)])
def test_eps_fwd_stats(dtype, C, K, Q, O, B, H, W):
    """dctn_eps_fwd_stats: [sum y, sum y^2] over the storage-rounded y, exact in float64."""
    run_eps_fwd_stats(dtype, C, K, Q, O, B, H, W)


def run_eps_fwd_stats(dtype, C, K, Q, O, B, H, W, arena=None):
    x = X.one_hot_pixels(C, B, H, W, Q, B + H)
    core = X.eps_core(Q, K * K * C, O, B + H + 1)
    y = X.expected(R.eps_4step(core, x), dtype).double()
    # integer y of at most 8: the per-lane float32 sums of y and y^2 are bounded by the totals
    X.check_budget({"sum |y|": y.abs().sum().reshape(1), "sum y^2": (y * y).sum().reshape(1)}, torch.float32)
    count, sums = output_sums_in_slices(on_dev(core.to(dtype), arena), on_dev(x.to(dtype), arena), 16)
    assert count == y.numel()
    want = torch.stack([y.sum(), (y * y).sum()])
    assert torch.equal(sums.cpu(), want), (sums.cpu().tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------ fused head
def head_operands(C, K, H, W, B, O, Cout, dtype, seed, two_hot=True):
    N = K * K * C
    x = X.pixels(C, B, H, W, 2, seed, two_hot=two_hot)
    core = X.eps_core(2, N, O, seed + 1, vmax=8)
    F = (H - K + 1) * (W - K + 1) * O
    w, bias, g = X.head_operands(Cout, F, B, seed + 3)
    return core, x, w, bias, g


def head_oracle(core, x, w, bias, g, closed_form=False):
    """(logits, dCore, dW, dBias, report) in float64, with the budget of the head: features and dY = dLogits . W are
    rounded to the storage dtype inside the families (bf16: <= 2^8 units), every sum fits float32."""
    C, B = x.shape[:2]
    K = math.isqrt((core.ndim - 1) // C)
    if closed_form:
        feat = X.eps_onehot_forward(core, x)
        feat_mag = X.eps_onehot_forward(core.abs(), x)
    else:
        feat = R.eps_4step(core, x)
        feat_mag = R.eps_4step(core.abs(), x.abs())
    f2 = feat.reshape(B, -1)
    logits = f2 @ w.T + bias
    dfeat = (g @ w).reshape(feat.shape)
    dcore = X.eps_onehot_dcore(core.shape, x, dfeat) if closed_form else R.grads(R.eps_4step, [core, x], dfeat)[0]
    dw, db = g.T @ f2, g.sum(0)
    dfeat_mag = (g.abs() @ w.abs()).reshape(feat.shape)
    mags = {"logits": feat_mag.reshape(B, -1) @ w.abs().T + bias.abs(), "dW": g.abs().T @ feat_mag.reshape(B, -1),
            "dBias": g.abs().sum(0),
            "dcore": X.eps_onehot_dcore(core.shape, x, dfeat_mag) if closed_form else R.grads(R.eps_4step, [core.abs(), x.abs()], dfeat_mag)[0]}
    # the q2reg family's bf16 roundings with the head fused: the stored features, dY = dLogits . W and Z = P1 . dY
    p1 = 1.0 if closed_form else float(X.khatri_rao_halves(x.abs(), K)[1].max())
    report = X.check_budget(mags, torch.float32, {"features": float(feat_mag.max()), "dY = dLogits W": float(dfeat_mag.max()),
                                                  "Z = P1 dY": p1 * float(dfeat_mag.max())})
    X.assert_every_window_counts(X.eps_window_weights(x, K, dfeat), "head")
    X.assert_nonzero(logits=logits, dcore=dcore, dW=dw, dBias=db)
    return logits, dcore, dw, db, report


def run_head(core, x, w, bias, g, dtype, *, fused=True, fused_fwd=True, blocked=True, strided=False, oracle=None,
             fwd=None, bwd=None, tag="", arena=None):
    from dctn_amd.eps_plus_linear import _EpsLinearHeadFunction, _LinearHeadFunction

    logits, dcore, dw, db, _ = oracle or head_oracle(core, x, w, bias, g)
    cd, wd, bd = (on_dev(t.to(dtype), arena).requires_grad_(True) for t in (core, w, bias))
    xd = x.to(dtype).to(DEV)
    if strided:
        xd = strided_copy(xd)
    xd = on_dev(xd, arena)
    saved = EPL.FUSED_HEAD_FWD, EPL.BLOCKED_FEATURES
    EPL.FUSED_HEAD_FWD, EPL.BLOCKED_FEATURES = fused_fwd, blocked
    try:
        if fused:
            assert _EpsLinearHeadFunction.supported(cd, xd, wd, bd)
            out = _EpsLinearHeadFunction.apply(cd, xd, wd, bd)
        else:
            out = _LinearHeadFunction.apply(eps(cd, xd).reshape(x.shape[1], -1), wd, bd)
        kf = dctn_amd.last_kernel()
        out.backward(on_dev(g.to(dtype), arena))
        kb = dctn_amd.last_kernel()
    finally:
        EPL.FUSED_HEAD_FWD, EPL.BLOCKED_FEATURES = saved
    assert fwd is None or kf == fwd, f"{tag}: forward ran {kf}, expected {fwd}"
    assert bwd is None or kb == bwd, f"{tag}: backward ran {kb}, expected {bwd}"
    X.assert_exact(out, logits, dtype, ("sample", "class"), f"{tag} logits [{kf}]")
    X.assert_exact(core_view(cd.grad), core_view(dcore), dtype, X.CORE_LAYOUT, f"{tag} dCore [{kb}]")
    X.assert_exact(wd.grad, dw, dtype, ("class", "feature"), f"{tag} dW [{kb}]")
    X.assert_exact(bd.grad, db, dtype, ("class",), f"{tag} dBias [{kb}]")
    return out.detach(), cd.grad, wd.grad, bd.grad


HEAD_MODES = {   # (fused node, fused forward kernel, blocked4 features)
    "fused_blocked4": (True, True, True), "fused_rowmajor": (True, True, False), "fused_bwd_only": (True, False, False),
    "unfused": (False, False, False)}


# shapes the one-kernel forwards decline (bf16: more position groups than HEAD_FWD_MAXPG): layer and head run as two kernels
TWO_KERNEL_FWD_BF16 = {(1, 3, 70, 2, 4, 10), (1, 3, 30, 19, 4, 6), (1, 3, 70, 250, 4, 10)}
TWO_KERNEL_FWD_F32 = {(1, 3, 5, 17, 7, 2, 4, False), (1, 3, 40, 40, 3, 4, 10, False)}


def _bf16_kernels(mode, case=None):
    fused, ffwd, _ = HEAD_MODES[mode]
    if not fused:
        return "linear_head_fwd_mfma", "eps_bwd_mfma_q2reg"
    one = ffwd and case not in TWO_KERNEL_FWD_BF16
    return ("eps_head_fwd_mfma_q2reg" if one else "linear_head_fwd_mfma"), "eps_head_bwd_mfma_q2reg"


@pytest.mark.parametrize("mode", sorted(HEAD_MODES))
@pytest.mark.parametrize("C,K,size,B,O,Cout", HEAD_CASES)
def test_head_bf16(C, K, size, B, O, Cout, mode):
    """bf16 layer + head (eps_mfma.hip): logits, dCore, dW and dBias exact in every layout and split of the path."""
    core, x, w, bias, g = head_operands(C, K, size, size, B, O, Cout, torch.bfloat16, seed=C + K + size + B + O + Cout)
    fused, ffwd, blocked = HEAD_MODES[mode]
    fwd, bwd = _bf16_kernels(mode, (C, K, size, B, O, Cout))
    run_head(core, x, w, bias, g, torch.bfloat16, fused=fused, fused_fwd=ffwd, blocked=blocked, fwd=fwd, bwd=bwd, tag=mode)


@pytest.mark.parametrize("mode", ["fused", "fused_bwd_only", "unfused"])
@pytest.mark.parametrize("C,K,H,W,B,O,Cout,strided", [c for c in Q2F32_CASES if c[5] in (2, 4)])
def test_head_f32(C, K, H, W, B, O, Cout, strided, mode):
    """float32 layer + head (eps_q2f32.hip), fused and as two nodes."""
    core, x, w, bias, g = head_operands(C, K, H, W, B, O, Cout, torch.float32, seed=C + K + H + W + B + O + Cout)
    fused = mode != "unfused"
    one = (C, K, H, W, B, O, Cout, strided) not in TWO_KERNEL_FWD_F32
    fwd = {"fused": "eps_head_fwd_q2f32" if one else "linear_head_fwd_generic", "fused_bwd_only": "linear_head_fwd_generic", "unfused": "linear_head_fwd_generic"}[mode]
    bwd = "eps_head_bwd_q2f32" if fused else "eps_bwd_q2f32"
    run_head(core, x, w, bias, g, torch.float32, fused=fused, fused_fwd=mode == "fused", blocked=False, strided=strided,
             fwd=fwd, bwd=bwd, tag=mode)


@pytest.mark.parametrize("mode", sorted(HEAD_MODES))
@pytest.mark.parametrize("B", [1, 5, 37, 1024, 1280])
def test_head_bf16_cfg2_batches(B, mode):
    """The headline model's layer (C = 1, K = 3, 28 x 28, O = 4, 10 classes) at the batch sizes around its tiles."""
    core, x, w, bias, g = head_operands(1, 3, 28, 28, B, 4, 10, torch.bfloat16, seed=B, two_hot=False)
    fused, ffwd, blocked = HEAD_MODES[mode]
    fwd, bwd = _bf16_kernels(mode)
    run_head(core, x, w, bias, g, torch.bfloat16, fused=fused, fused_fwd=ffwd, blocked=blocked,
             oracle=head_oracle(core, x, w, bias, g, closed_form=True), fwd=fwd, bwd=bwd, tag=f"cfg2 B={B} {mode}")


# ------------------------------------------------------------------------------------------------ linear head
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("B,F,Cout", [(1024, 2704, 10), (37, 3176, 10), (5, 64, 3), (130, 200, 16), (128, 3174, 10),
                                      (37, 201, 10), (5, 7, 3), (70, 1000, 1)])
def test_linear_head(B, F, Cout, dtype):
    run_linear_head(B, F, Cout, dtype)


def run_linear_head(B, F, Cout, dtype, arena=None):
    from dctn_amd.eps_plus_linear import _LinearHeadFunction

    feat = X.small_ints((B, F), B + F, 8) * (0.5 if dtype != torch.bfloat16 else 1.0)
    w, bias, g = X.head_operands(Cout, F, B, B * F)
    fa, wa, ga = X.to_grid(feat).abs(), w.abs(), g.abs()
    X.check_budget({"out": fa @ wa.T + bias.abs(), "dFeat": ga @ wa, "dW": ga.T @ fa, "dBias": ga.sum(0)}, ACC[dtype])
    fd, wd, bd = (on_dev(t.to(dtype), arena).requires_grad_(True) for t in (feat, w, bias))
    out = _LinearHeadFunction.apply(fd, wd, bd)
    kf = dctn_amd.last_kernel()
    assert kf == ("linear_head_fwd_mfma" if dtype == torch.bfloat16 and F % 8 == 0 else "linear_head_fwd_generic")
    out.backward(on_dev(g.to(dtype), arena))
    kb = dctn_amd.last_kernel()
    assert kb == ("linear_head_bwd" if kf == "linear_head_fwd_mfma" else "linear_head_bwd_generic"), kb
    X.assert_exact(out, feat @ w.T + bias, dtype, ("sample", "class"), f"out [{kf}]")
    X.assert_exact(fd.grad, g @ w, dtype, ("sample", "feature"), f"dFeat [{kb}]")
    X.assert_exact(wd.grad, g.T @ feat, dtype, ("class", "feature"), f"dW [{kb}]")
    X.assert_exact(bd.grad, g.sum(0), dtype, ("class",), f"dBias [{kb}]")


# ------------------------------------------------------------------------------------------------ ConvSBS
def sbs_spec(pos, bonds, outs, C, q):
    return SBSSpecString(tuple(SBSSpecCore(Pos2D(h, w), o) for (h, w), o in zip(pos, outs)), tuple(bonds), C, q)


def sbs_operands(spec, B, H, W, dtype, seed, p2=0.125, two_hot=True):
    C, q = spec.in_num_channels, spec.in_quantum_dim_size
    shapes = R.sbs_core_shapes([c.out_quantum_dim_size for c in spec.cores], spec.bond_sizes, C, q)
    cores = X.sbs_cores(shapes, seed, p2=p2)
    x = X.pixels(C, B, H, W, q, seed + 1, two_hot=two_hot)   # 0 / 1 pixels: a 2^-1 one costs 2^(cores * C) units
    pos = [(p.h, p.w) for p in spec.positions]
    Ho, Wo = H - max(p[0] for p in pos), W - max(p[1] for p in pos)
    dy = X.small_ints((B, Ho, Wo, spec.out_total_quantum_dim_size), seed + 2, 2, nonzero=True)
    return cores, x, dy, pos


def sbs_oracle(cores, x, dy, pos, dtype):
    report = X.check_budget(X.sbs_mags(cores, pos, x, dy), ACC[dtype])
    X.assert_every_window_counts(X.sbs_window_weights(cores, pos, x, dy), "ConvSBS")
    want = R.convsbs_forward(cores, pos, x)
    gr = R.grads(lambda xx, *cc: R.convsbs_forward(cc, pos, xx), [x] + list(cores), dy)
    X.assert_nonzero(forward=want, dx=gr[0], **{f"dcore{i}": g for i, g in enumerate(gr[1:])})
    return want, gr, report


def check_sbs(y, dx, dcores, want, gr, dtype, tag):
    X.assert_exact(y, want, dtype, X.EPS_LAYOUT, f"{tag} forward")
    if dx is not None:
        X.assert_exact(dx, gr[0], dtype, ("channel", "sample", "row", "col", "q"), f"{tag} dX")
    for i, (gc, wc) in enumerate(zip(dcores, gr[1:])):
        if gc is not None:
            X.assert_exact(gc, wc, dtype, ("o", "l", "r") + ("q",) * (wc.ndim - 3), f"{tag} dCore{i}")


def sbs_bwd_recompute(m, xd, dy, arena=None):
    """The backward without the forward's saved states (`dctn_convsbs_bwd`: the states are recomputed)."""
    plan = CS._plan(m.spec)
    C, B, H, W, q = xd.shape
    code = L.dtype_code(xd) | CS._sbs_flags
    cores = [c.detach().contiguous() for c in m.cores]
    arena = arena if arena is not None else G.current()
    if arena is None:
        dx = torch.empty((C, B, H, W, q), dtype=xd.dtype, device=DEV)
        dcores = [torch.empty_like(c) for c in cores]
    else:   # the outputs of this direct library call guarded and poisoned like the host modules' own
        dx = arena.empty((C, B, H, W, q), xd.dtype, DEV)
        dcores = [arena.empty_like(c) for c in cores]
    ws = L.workspace(CS._workspace_bytes(plan, B, H, W, code, 1), DEV)
    L.check(L.lib().dctn_convsbs_bwd(xd.data_ptr(), L.strides5(xd), L.ptr_array(cores), dy.contiguous().data_ptr(), dx.data_ptr(),
                                     L.ptr_array(dcores), plan.n, plan.outs, plan.bonds, plan.ph, plan.pw, C, B, H, W, q,
                                     ws.data_ptr(), ws.numel(), code, L.stream_ptr(DEV)), "ConvSBS backward (recompute)")
    return dx, dcores


def run_sbs(spec, B, H, W, dtype, seed, *, fwd=None, bwd=None, strided=False, x_grad=True, core_grad=True, ctx=None,
            recompute=True, p2=0.125, two_hot=True, tag="", arena=None):
    cores, x, dy, pos = sbs_operands(spec, B, H, W, dtype, seed, p2, two_hot)
    want, gr, report = sbs_oracle(cores, x, dy, pos, dtype)
    m = ConvSBS(spec).to(DEV).to(dtype)
    with torch.no_grad():
        for c, v in zip(m.cores, cores):
            c.copy_(v)
            c.requires_grad_(core_grad)
    xd = x.to(dtype).to(DEV)
    if strided:
        xd = strided_copy(xd)
    xd = on_dev(xd, arena).requires_grad_(x_grad)
    with (ctx() if ctx else contextlib.nullcontext()):
        y = m(xd)
        kf = dctn_amd.last_kernel()
        y.backward(on_dev(dy.to(dtype), arena))
        kb = dctn_amd.last_kernel()
        assert fwd is None or kf == fwd, f"{tag}: forward ran {kf}, expected {fwd}"
        assert bwd is None or kb == bwd, f"{tag}: backward ran {kb}, expected {bwd}"
        check_sbs(y, xd.grad if x_grad else None, [c.grad for c in m.cores] if core_grad else [], want, gr, dtype,
                  f"{tag} [{kf} / {kb}]")
        if recompute and x_grad and core_grad:
            dx2, dc2 = sbs_bwd_recompute(m, xd.detach(), on_dev(dy.to(dtype), arena), arena)
            kr = dctn_amd.last_kernel()
            assert bwd is None or kr == bwd, f"{tag}: recomputing backward ran {kr}, expected {bwd}"
            check_sbs(y, dx2, dc2, want, gr, dtype, f"{tag} recomputed states [{kr}]")
    return report


def _case_id(c):
    return "n%d_b%s_o%s_C%dq%d_B%d_%dx%d%s%s%s" % (
        len(c[0]), max(c[1]), "x".join(map(str, c[2])), c[3], c[4], c[5], c[6], c[7], "" if c[8] else "_nodx",
        "" if c[9] else "_nodcore", "_strided" if c[10] else "")


@pytest.mark.parametrize("case", REG_CASES + MV_CASES, ids=_case_id)
def test_convsbs_reg(case):
    """Register-resident small-bond sweep (convsbs_reg.hip), the many-valued core included."""
    pos, bonds, outs, C, q, B, H, W, x_grad, core_grad, strided = case
    run_sbs(sbs_spec(pos, bonds, outs, C, q), B, H, W, torch.float32, B + H + W, fwd="convsbs_fwd_reg_f32",
            bwd="convsbs_bwd_reg_f32", strided=strided, x_grad=x_grad, core_grad=core_grad, tag="reg")


@pytest.mark.parametrize("case", BAND_CASES, ids=_case_id)
def test_convsbs_band(case):
    pos, bonds, outs, C, q, B, H, W, x_grad, core_grad, strided = case
    run_sbs(sbs_spec(pos, bonds, outs, C, q), B, H, W, torch.float32, B + H + W, fwd="convsbs_fwd_band_f32",
            bwd="convsbs_bwd_band_f32", strided=strided, x_grad=x_grad, core_grad=core_grad, tag="band")


MFMA_SBS_CASES = [c for c in sbs_mfma_cases() if not (sbs_band_family_takes(*c) and max(c[1]) > 8)]   # bonds 9..16: band


@pytest.mark.parametrize("case", MFMA_SBS_CASES, ids=lambda c: "n%d_r%s_o%s_C%dq%d" % (
    len(c[0]), c[1][1] if len(set(c[1][1:])) == 1 else "".join("%x" % b for b in c[1]), "".join(map(str, c[2])), c[3], c[4]))
def test_convsbs_mfma(case):
    """The matrix-core sweep (convsbs_mfma.hip), forced with matrix_core_sweep() where another family is the default;
    strings longer than 9 cores accumulate in LDS with float atomics - exact all the same."""
    pos, bonds, outs, C, q = case
    spec = sbs_spec(pos, bonds, outs, C, q)
    reg, band = sbs_reg_family_takes(*case), sbs_band_family_takes(*case)
    run_sbs(spec, 3, spec.max_height_pos + 6, spec.max_width_pos + 7, torch.float32, len(pos) * 10 + bonds[1],
            fwd="convsbs_fwd_mfma_f32", bwd="convsbs_bwd_mfma_f32", ctx=matrix_core_sweep if (reg or band) else None,
            tag="mfma")


GENERIC_SBS = [  # (positions, bonds, outs, C, q, B, H, W): float64 strings and rings on the generic sweep
    (SNAKE9, (1,) + (3,) * 8, (1, 1, 1, 1, 2, 1, 1, 1, 1), 2, 2, 3, 7, 8),
    (SNAKE9, (4,) * 9, (1, 1, 1, 1, 5, 1, 1, 1, 1), 2, 2, 3, 7, 8),
    (((0, 0), (0, 1), (1, 1), (1, 0)), (3, 4, 5, 6), (1, 3, 2, 4), 2, 2, 2, 6, 7),
    (((0, 1), (0, 0), (1, 0)), (1, 5, 2), (2, 1, 3), 1, 3, 4, 5, 6),
    (((0, 0), (0, 1), (0, 2)), (2, 2, 2), (1, 1, 1), 1, 4, 1, 3, 3),
]


@pytest.mark.parametrize("case", GENERIC_SBS, ids=lambda c: "n%d_b%s_o%s_C%dq%d" % (
    len(c[0]), "".join(map(str, c[1])), "".join(map(str, c[2])), c[3], c[4]))
def test_convsbs_generic(case):
    """The generic sweep (convsbs_generic.hip): float64 open chains and rings, unequal bonds, outputs on several cores."""
    pos, bonds, outs, C, q, B, H, W = case
    run_sbs(sbs_spec(pos, bonds, outs, C, q), B, H, W, torch.float64, B + H + W + len(pos), fwd="convsbs_fwd_generic",
            bwd="convsbs_bwd_generic", tag="generic")


@pytest.mark.parametrize("name", sorted(FAILS_TODAY) + ["forced_" + n for n in sorted(FORCED)])
def test_convsbs_wide(name):
    """The wide backward (convsbs_wide.hip): strings the generic sweep declines, and strings it takes forced with
    wide_sweep()."""
    if name.startswith("forced_"):
        spec, dtype = FORCED[name[len("forced_"):]]
        ctx = wide_sweep
    else:
        make, dtype = FAILS_TODAY[name]
        spec, ctx = make(), None
    run_sbs(spec, 2, 7, 7, dtype, len(name), bwd=WIDE[dtype], ctx=ctx, p2=0.0, tag=name)


@pytest.mark.parametrize("bond,C,q,outs_a,outs_b,B,H,W", MANY_CASES)
def test_many_convsbs(bond, C, q, outs_a, outs_b, B, H, W):
    """ManyConvSBS: two nine-core strings in one launch each way, dX summed over the strings by the kernel."""
    run_many_convsbs(bond, C, q, outs_a, outs_b, B, H, W)


def run_many_convsbs(bond, C, q, outs_a, outs_b, B, H, W, arena=None):
    specs = (tuple(SBSSpecCore(Pos2D(h, w), o) for (h, w), o in zip(SNAKE9, outs_a)),
             tuple(SBSSpecCore(Pos2D(h, w), o) for (h, w), o in zip(SNAKE9B, outs_b)))
    many = ManyConvSBS(C, q, bond, False, specs).to(DEV)
    seed = bond * 100 + B
    x = X.pixels(C, B, H, W, q, seed)
    wants, dx_sum, dys = [], torch.zeros_like(x), []
    mags_dx = torch.zeros_like(x)
    for k, (string, pos) in enumerate(zip(many.strings, (SNAKE9, SNAKE9B))):
        shapes = [tuple(c.shape) for c in string.cores]
        cores = X.sbs_cores(shapes, seed + 10 * k)
        with torch.no_grad():
            for c, v in zip(string.cores, cores):
                c.copy_(v)
        dy = X.small_ints((B, H - 2, W - 2, math.prod(s[0] for s in shapes)), seed + 10 * k + 5, 2, nonzero=True)
        want, gr, _ = sbs_oracle(cores, x, dy, list(pos), torch.float32)
        mags_dx += X.sbs_mags(cores, list(pos), x, dy)["dx"]
        wants.append((cores, want, gr))
        dx_sum += gr[0]
        dys.append(dy)
    X.check_budget({"dx summed over the strings": mags_dx}, torch.float32)
    xd = on_dev(x.float(), arena).requires_grad_(True)
    fam = "band" if bond > 4 else "reg"
    ya, yb = many(xd)
    assert dctn_amd.last_kernel() == f"convsbs_many_fwd_{fam}_f32"
    ((ya * on_dev(dys[0].float(), arena)).sum() + (yb * on_dev(dys[1].float(), arena)).sum()).backward()
    assert dctn_amd.last_kernel() == f"convsbs_many_bwd_{fam}_f32"
    for string, y, (cores, want, gr) in zip(many.strings, (ya, yb), wants):
        check_sbs(y, None, [c.grad for c in string.cores], want, gr, torch.float32, f"many {fam}")
    X.assert_exact(xd.grad, dx_sum, torch.float32, ("channel", "sample", "row", "col", "q"), f"many {fam} dX")


# ------------------------------------------------------------------------------------------------ determinism and replay
def _replay_case(which, arena=None):
    """(run: () -> list of results, want: list of float64 expected values, dtype) for a captured forward + backward."""
    if which.startswith("eps"):
        dtype, C, K, Q, O, B, H, W = {"eps_generic_q3": (torch.float32, 1, 2, 3, 3, 5, 6, 6),
                                      "eps_bigcore_f32": (torch.float32, 1, 3, 4, 6, 3, 6, 7),
                                      "eps_q2reg_bf16": (torch.bfloat16, 1, 3, 2, 4, 37, 12, 12)}[which]
        core, x, dy = eps_operands(C, K, Q, O, B, H, W, dtype, seed=7)
        want = [R.eps_4step(core, x)] + R.grads(R.eps_4step, [core, x], dy)[::-1]
        xd = on_dev(x.to(dtype), arena).requires_grad_(True)
        cd = on_dev(core.to(dtype), arena).requires_grad_(True)
        g = on_dev(dy.to(dtype), arena)
        fn = eps_one_by_one if which == "eps_generic_q3" else eps

        def run():
            xd.grad, cd.grad = None, None
            y = fn(cd, xd)
            y.backward(g)
            return [y, xd.grad, cd.grad]
        return run, want, dtype
    if which == "head_bf16_cfg2":
        core, x, w, bias, g = head_operands(1, 3, 28, 28, 64, 4, 10, torch.bfloat16, seed=64, two_hot=False)
        logits, dcore, dw, db, _ = head_oracle(core, x, w, bias, g, closed_form=True)
        from dctn_amd.eps_plus_linear import _EpsLinearHeadFunction
        cd, wd, bd = (on_dev(t.to(torch.bfloat16), arena).requires_grad_(True) for t in (core, w, bias))
        xd, gd = on_dev(x.to(torch.bfloat16), arena), on_dev(g.to(torch.bfloat16), arena)

        def run():
            cd.grad = wd.grad = bd.grad = None
            out = _EpsLinearHeadFunction.apply(cd, xd, wd, bd)
            out.backward(gd)
            return [out, cd.grad, wd.grad, bd.grad]
        return run, [logits, dcore, dw, db], torch.bfloat16
    bonds, outs, dtype, ctx = {"convsbs_generic_f64": ((4,) * 9, (1, 1, 1, 1, 5, 1, 1, 1, 1), torch.float64, None),
                               "convsbs_mfma_lds_12": ((1,) + (8,) * 11, (1,) * 12, torch.float32, None),
                               "convsbs_band_16": ((1,) + (16,) * 8, (1, 1, 1, 1, 2, 1, 1, 1, 1), torch.float32, None)}[which]
    pos = list(SNAKE9) if len(bonds) == 9 else [(h, w) for h in range(3) for w in range(4)]
    spec = sbs_spec(pos, bonds, outs, 2 if len(bonds) == 9 else 1, 2)
    cores, x, dy, pos = sbs_operands(spec, 3, 7, 8, dtype, seed=11)
    want, gr, _ = sbs_oracle(cores, x, dy, pos, dtype)
    m = ConvSBS(spec).to(DEV).to(dtype)
    with torch.no_grad():
        for c, v in zip(m.cores, cores):
            c.copy_(v)
    xd = on_dev(x.to(dtype), arena).requires_grad_(True)
    g = on_dev(dy.to(dtype), arena)

    def run():
        xd.grad = None
        for c in m.cores:
            c.grad = None
        y = m(xd)
        y.backward(g)
        return [y, xd.grad] + [c.grad for c in m.cores]
    return run, [want] + list(gr), dtype


def two_eager_calls(which, arena=None):
    """The eager half of the test below: two calls in a row, each equal to the oracle; returns (run, check) for the replays."""
    run, want, dtype = _replay_case(which, arena)

    def check(got, label):
        for i, (gt, wt) in enumerate(zip(got, want)):
            X.assert_exact(gt.reshape(wt.shape), wt, dtype, (), f"{which} {label} result {i}")

    for call in range(2):
        check(run(), f"eager call {call}")
    return run, check


REPLAY_CASES = ["eps_generic_q3", "eps_bigcore_f32", "eps_q2reg_bf16", "head_bf16_cfg2", "convsbs_generic_f64",
                "convsbs_mfma_lds_12", "convsbs_band_16"]


@pytest.mark.parametrize("which", REPLAY_CASES)
def test_two_calls_and_graph_replays_equal_the_oracle(which):
    """Atomics, LDS counters and split joins give the same bits every time: two eager calls and two replays of a
    captured graph (result buffers dirtied in between) all equal the oracle."""
    run, check = two_eager_calls(which)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for rep in range(2):
        for t in got:
            t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        check(got, f"replay {rep}")


# ------------------------------------------------------------------------------------------------ full size
@pytest.mark.parametrize("mode", ["bf16_blocked4", "bf16_rowmajor", "f32"])
def test_cfg2_full_batch_1024_exact(mode):
    """The bench workload (cfg2: C = 1, K = 3, 28 x 28, O = 4, 10 classes, B = 1024): logits, dCore, dW and dBias
    against float64 (closed form for one-hot pixels), bit for bit."""
    dtype = torch.float32 if mode == "f32" else torch.bfloat16
    core, x, w, bias, g = head_operands(1, 3, 28, 28, 1024, 4, 10, dtype, seed=1024, two_hot=False)
    oracle = head_oracle(core, x, w, bias, g, closed_form=True)
    if dtype == torch.float32:
        fwd, bwd = "eps_head_fwd_q2f32", "eps_head_bwd_q2f32"
    else:
        fwd, bwd = "eps_head_fwd_mfma_q2reg", "eps_head_bwd_mfma_q2reg"
    run_head(core, x, w, bias, g, dtype, fused=True, fused_fwd=True, blocked=mode == "bf16_blocked4", oracle=oracle,
             fwd=fwd, bwd=bwd, tag=f"cfg2 {mode}")


@pytest.mark.parametrize("r", [4, 8, 16])
def test_cfg4_convsbs_batch_128_exact(r):
    """cfg4: the 9-core snake, open chain of bond r, x (1, 128, 32, 32, 3).  Values +-1 only (p2 = 0): with 115 200
    windows a +-2 entry would push dCore past 2^24 grid units; the budget check says so before any launch."""
    spec = sbs_spec(SNAKE9, (1,) + (r,) * 8, (1, 1, 1, 1, 2, 1, 1, 1, 1), 1, 3)
    fam = "reg" if r <= 4 else "band"
    run_sbs(spec, 128, 32, 32, torch.float32, r, fwd=f"convsbs_fwd_{fam}_f32", bwd=f"convsbs_bwd_{fam}_f32", p2=0.0,
            two_hot=False, recompute=False, tag=f"cfg4 r={r}")
