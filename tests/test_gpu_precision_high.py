"""set_float32_matmul_precision("high"): the bf16x3 large-core family (eps_bigcore_bf16x3.hip).

Float32 shapes the family plans run bf16x3 (hi*hi + hi*lo + lo*hi on the bf16 matrix instructions), forward and backward;
every other shape runs exactly as under "exact".  Every test restores "exact", also when it fails."""
import math

import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd.eps import _f32_through_bf16, eps, keep_gemm_result
from oracle import ref_cpu as R
from tests import exact_inputs as X
from tests import guarded_buffers as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# every name the family reports through dctn_set_last_kernel -> the test here that pins it on exact inputs
# (tests/test_host_precision_policy.py holds the sources to this table)
KERNELS = {
    "bf16x3_eps_fwd_bigcore": "test_bf16x3_exact_inputs", "bf16x3_eps_fwd_bigcore_saving": "test_bf16x3_exact_inputs",
    "bf16x3_eps_bwd_bigcore": "test_bf16x3_exact_inputs", "bf16x3_eps_bwd_bigcore_savedz": "test_bf16x3_exact_inputs",
}

# the shapes of tests/test_gpu_parity.py::test_eps_f32_bigcore_vs_oracle with Q < 16
ORACLE_SHAPES = [
    (1, 3, 9, 10, 2, 4, 4),
    (1, 2, 8, 8, 2, 4, 8),
    (1, 2, 7, 7, 2, 4, 2),
    (1, 2, 6, 7, 4, 3, 6),
    (1, 3, 9, 9, 8, 2, 8),
    (1, 40, 6, 6, 4, 2, 5),
    (2, 3, 6, 5, 4, 2, 3),
    (1, 2, 6, 6, 2, 3, 16),
]


@pytest.fixture(autouse=True)
def high():
    dctn_amd.set_float32_matmul_precision("high")
    try:
        yield
    finally:
        dctn_amd.set_float32_matmul_precision("exact")


def close(got, want, rtol=2e-4, atol=2e-5):
    """the float32 tolerance of the parity tests: rtol 2e-4, atol 2e-5 * max |want|"""
    want = torch.as_tensor(want).double()
    got = got.detach().cpu().double()
    scale = float(want.abs().max()) or 1.0
    return torch.allclose(got, want, rtol=rtol, atol=atol * scale)


def normwise(got, want):
    want = want.double()
    return float((got.detach().cpu().double() - want).norm() / want.norm())


def _place(t, arena=None):
    """On the device; inside a guarded allocation under an arena of tests/guarded_buffers.py (given, or the active one)."""
    t = t.to(DEV)
    arena = arena if arena is not None else G.current()
    return t if arena is None else arena.place(t)


def _run(core, x, dy, need_dx=True, arena=None):
    xd = _place(x, arena).requires_grad_(need_dx)
    cd = _place(core, arena).requires_grad_(True)
    y = eps(cd, xd)
    kf = dctn_amd.last_kernel()
    y.backward(_place(dy, arena))
    kb = dctn_amd.last_kernel()
    return y.detach(), (xd.grad.clone() if need_dx else None), cd.grad.clone(), kf, kb


@pytest.mark.parametrize("C,B,H,W,Q,K,O", ORACLE_SHAPES)
def test_high_vs_oracle(C, B, H, W, Q, K, O):
    torch.manual_seed(7 * Q + K + O)
    N = K * K * C
    x = torch.randn(C, B, H, W, Q)
    core = torch.randn(*(Q,) * N, O) * Q ** (-N / 4)
    want = R.eps_4step(core.double(), x.double())
    dy = torch.randn(*want.shape)
    dcore, dx = R.grads(R.eps_4step, [core.double(), x.double()], dy.double())
    y, gx, gc, kf, kb = _run(core, x, dy)
    assert kf == "bf16x3_eps_fwd_bigcore_saving" and kb == "bf16x3_eps_bwd_bigcore_savedz"
    errs = {}
    for name, got, ref in (("out", y, want), ("dx", gx, dx), ("dcore", gc, dcore)):
        assert close(got, ref), f"{name} outside the float32 tolerance"
        errs[name] = normwise(got, ref)
        assert errs[name] <= 3e-5, f"{name}: normwise relative error {errs[name]:.3e}"
    # bit-reproducible from call to call (fixed-order slice sums, no float atomics)
    y2, gx2, gc2, _, _ = _run(core, x, dy)
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(gc, gc2)
    # against one bf16 plane ("bf16" policy) on the same inputs - where that policy rounds at all: the small-batch shapes
    # it does not send to the bf16 matrix cores run float32 arithmetic under it, and there is no bf16 error to compare to
    dctn_amd.set_float32_matmul_precision("bf16")
    if not _f32_through_bf16(core.to(DEV), x.to(DEV)):
        return
    yb, gxb, gcb, _, _ = _run(core, x, dy)
    dctn_amd.set_float32_matmul_precision("high")
    for name, got, ref in (("out", yb, want), ("dx", gxb, dx), ("dcore", gcb, dcore)):
        eb = normwise(got, ref)
        assert errs[name] <= eb / 30, f"{name}: high {errs[name]:.3e} vs bf16 {eb:.3e}"


@pytest.mark.parametrize("C,B,H,W,Q,K,O", [ORACLE_SHAPES[0], ORACLE_SHAPES[3], ORACLE_SHAPES[4]])
def test_high_routes(C, B, H, W, Q, K, O):
    """x without a gradient (dCore alone), and x with one but nothing kept (dX from the G0 and G1 products)."""
    torch.manual_seed(C + B + Q)
    N = K * K * C
    x = torch.randn(C, B, H, W, Q)
    core = torch.randn(*(Q,) * N, O) * Q ** (-N / 4)
    want = R.eps_4step(core.double(), x.double())
    dy = torch.randn(*want.shape)
    dcore, dx = R.grads(R.eps_4step, [core.double(), x.double()], dy.double())
    y, _, gc, kf, kb = _run(core, x, dy, need_dx=False)
    assert kf == "bf16x3_eps_fwd_bigcore" and kb == "bf16x3_eps_bwd_bigcore"
    assert close(y, want) and close(gc, dcore)
    with keep_gemm_result(False):
        y, gx, gc, kf, kb = _run(core, x, dy)
    assert kf == "bf16x3_eps_fwd_bigcore" and kb == "bf16x3_eps_bwd_bigcore"
    assert close(y, want) and close(gx, dx) and close(gc, dcore)


EXACT_CASES = [  # C, K, Q, O, B, H, W
    (1, 4, 2, 4, 3, 9, 10),
    (1, 3, 4, 6, 2, 7, 7),
    (1, 4, 2, 8, 2, 8, 8),
    (1, 2, 8, 8, 3, 9, 9),
    (2, 2, 4, 3, 3, 6, 5),
]


@pytest.mark.parametrize("keep", [True, False], ids=["savedz", "recompute"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "C%dK%dQ%dO%dB%d_%dx%d" % c)
def test_bf16x3_exact_inputs(case, keep):
    """Exact inputs (tests/exact_inputs.py): the core entries are small integers (<= 8 bits, lo = 0), the pixels powers
    of two and the incoming gradient integers of up to 9 bits, so that the generated operands of G0, G1 and dCore carry
    a nonzero lo plane.  Every product is then exact in bf16x3 and every sum stays on the float32 grid: the output, dX
    and dCore equal the float64 oracle bit for bit."""
    C, K, Q, O, B, H, W = case
    seed = sum(case)
    N = K * K * C
    x = X.pixels(C, B, H, W, Q, seed, two_hot=True, halves=N <= 9)
    core = X.eps_core(Q, N, O, seed + 1, vmax=8)
    dy = X.small_ints((B, H - K + 1, W - K + 1, O), seed + 2, 511, nonzero=True)
    X.check_budget(X.eps_mags(core, x, dy), torch.float32)
    assert float(((dy.abs() > 256) & (dy % 2 == 1)).double().mean()) > 0.2   # 9 significant bits: a nonzero lo plane
    want = R.eps_4step(core, x)
    dcore, dx = R.grads(R.eps_4step, [core, x], dy)
    X.assert_nonzero(forward=want, dcore=dcore, dx=dx)
    for need_dx in (True, False):
        with keep_gemm_result(keep):
            y, gx, gc, kf, kb = _run(core.float(), x.float(), dy.float(), need_dx=need_dx)
        saving = keep and need_dx
        assert kf == "bf16x3_eps_fwd_bigcore" + ("_saving" if saving else "")
        assert kb == "bf16x3_eps_bwd_bigcore" + ("_savedz" if saving else "")
        X.assert_exact(y, want, torch.float32, X.EPS_LAYOUT, f"forward [{kf}]")
        X.assert_exact(gc.reshape(-1, O), dcore.reshape(-1, O), torch.float32, X.CORE_LAYOUT, f"dCore [{kb}]")
        if need_dx:
            X.assert_exact(gx, dx, torch.float32, ("channel", "sample", "row", "col", "q"), f"dX [{kb}]")


def _both_policies(core, x, dy, need_dx=True):
    out = {}
    for mode in ("exact", "high"):
        dctn_amd.set_float32_matmul_precision(mode)
        out[mode] = _run(core, x, dy, need_dx)
    dctn_amd.set_float32_matmul_precision("high")
    return out["exact"], out["high"]


@pytest.mark.parametrize("which", ["cfg2_f32", "f64", "q16"])
def test_high_unchanged_outside_family(which):
    """Shapes the bf16x3 family does not plan run the same kernels and give the same bits as under "exact"."""
    C, B, H, W, Q, K, O, dtype = {"cfg2_f32": (1, 16, 28, 28, 2, 3, 4, torch.float32),
                                  "f64": (1, 3, 9, 10, 2, 4, 4, torch.float64),
                                  "q16": (1, 2, 7, 7, 16, 2, 4, torch.float32)}[which]
    torch.manual_seed(11)
    N = K * K * C
    x = torch.rand(C, B, H, W, Q, dtype=dtype)
    core = torch.randn(*(Q,) * N, O, dtype=dtype) * Q ** (-N / 4)
    dy = torch.randn(B, H - K + 1, W - K + 1, O, dtype=dtype)
    assert L.lib().dctn_eps_family(C, B, H, W, Q, K, O, L.dtype_code(x), L.PREC_SPLIT) != 5
    for need_dx in (True, False):
        ex, hi = _both_policies(core, x, dy, need_dx)
        ex2, _ = _both_policies(core, x, dy, need_dx)
        assert ex[3:] == hi[3:], (ex[3:], hi[3:])
        for a, a2, b in zip(ex[:3], ex2[:3], hi[:3]):
            if a is None:
                assert b is None
            elif torch.equal(a, a2):
                assert torch.equal(a, b)
            else:   # the generic kernels' float atomics (Q = 16 gradients): "exact" differs from itself in the last bits
                assert close(b, a.cpu(), rtol=1e-5, atol=1e-6)


def test_fused_head_under_high():
    from dctn_amd import eps_plus_linear as EPL
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(0)
    model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, DEV, torch.float32, image_size=28)
    u = torch.rand(1, 8, 28, 28, device=DEV)
    x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1)
    assert EPL._EpsLinearHeadFunction.supported(model.epses[0], x, model.linear.weight, model.linear.bias)
    out = model(x)
    assert dctn_amd.last_kernel() == "eps_head_fwd_q2f32"
    out.sum().backward()
    assert dctn_amd.last_kernel() == "eps_head_bwd_q2f32"


def _mnist_like(batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(1, batch, size, size, generator=g)
    return torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(DEV)


def test_cfg3a_full_batch_128_high():
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(3)
    model = EPSesPlusLinear(((4, 4), (3, 6)), UnitTheoreticalOutputStd(), 1.0, DEV, torch.float32)
    x = _mnist_like(128, 28, 4)
    g = torch.randn(128, 10, generator=torch.Generator().manual_seed(5)).to(DEV)
    res = {}
    for mode in ("exact", "high"):
        dctn_amd.set_float32_matmul_precision(mode)
        for prm in model.parameters():
            prm.grad = None
        logits = model(x)
        logits.backward(g)
        res[mode] = [logits.detach()] + [prm.grad.detach().clone() for prm in model.parameters()]
    dctn_amd.set_float32_matmul_precision("high")
    for i, (a, b) in enumerate(zip(res["exact"], res["high"])):
        assert close(b, a.cpu()), f"tensor {i}: high vs exact"
    # oracle spot check on two samples, both layers
    e1, e2 = model.epses[0].detach(), model.epses[1].detach()
    idx = [0, 127]
    y1 = eps(e1, x)
    assert dctn_amd.last_kernel() == "bf16x3_eps_fwd_bigcore"
    y2 = eps(e2, y1.unsqueeze(0))
    assert dctn_amd.last_kernel() == "bf16x3_eps_fwd_bigcore"
    w1 = R.eps_4step(e1.cpu().double(), x[:, idx].cpu().double())
    w2 = R.eps_4step(e2.cpu().double(), w1.unsqueeze(0))
    # the exact path's bound (1e-5) is float32 rounding alone; bf16x3 adds ~3 * 2^-18 = 1.1e-5 per product, twice
    # over for layer 2, whose input carries layer 1's error (measured 1.6e-5 on layer 2)
    for got, want in ((y1[idx], w1), (y2[idx], w2)):
        err = float((got.cpu().double() - want).abs().max() / want.abs().max())
        assert err < 4e-5, err


def test_graphed_training_high_tracks_exact():
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd
    from dctn_amd.training import FlatSGD, GraphedTrainStep, fused_cross_entropy

    x = _mnist_like(32, 28, 9)
    y = torch.randint(0, 10, (32,), generator=torch.Generator().manual_seed(2)).to(DEV)
    losses = {}
    for mode in ("exact", "high"):
        dctn_amd.set_float32_matmul_precision(mode)
        torch.manual_seed(21)
        model = EPSesPlusLinear(((4, 4), (3, 6)), UnitTheoreticalOutputStd(), 1.0, DEV, torch.float32)
        opt = FlatSGD(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=0.05, momentum=0.9, l2=1e-3)
        step = GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=1)
        got = []
        for _ in range(5):
            out = step(x, y)
            got.append(float(out["loss"].detach()))
        torch.cuda.synchronize(DEV)
        assert all(math.isfinite(v) for v in got)
        losses[mode] = got
    dctn_amd.set_float32_matmul_precision("high")
    for a, b in zip(losses["exact"], losses["high"]):
        assert abs(a - b) <= 1e-4 * abs(a), (losses["exact"], losses["high"])
