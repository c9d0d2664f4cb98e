"""The sample-blocked feature layout of the fused head ("blocked4", DCTN_OPT_HEAD_FEATURES_BLOCKED4): the forward
writes features[((j * F) + f) * 4 + i] = feature f of sample 4 j + i, and the backward's dW product reads it.  Both must
give the bits of the row-major path; shapes, dtypes and options outside the HEADMM shapes decline before any launch, and
the autograd node then falls back to the row-major layout with the same numbers."""
import pytest
import torch

import dctn_amd
import dctn_amd.eps_plus_linear as EPL
from dctn_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BLK = L.OPT_HEAD_FEATURES_BLOCKED4
SENTINEL = -12345.0   # exactly representable in bf16: marks what a call must not (or must) overwrite


def problem(B, cout, C=1, K=3, O=4, size=28, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(seed + 7 * B + cout)
    N = K * K * C
    u = torch.rand(C, B, size, size)
    x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype).to(DEV)
    core = (torch.randn(*(2,) * N, O) * 2 ** (-N / 4)).to(dtype).to(DEV)
    Ho = size - K + 1
    F = Ho * Ho * O
    w = (torch.randn(cout, F) * F ** -0.5).to(dtype).to(DEV)
    bias = torch.randn(cout).to(dtype).to(DEV)
    return dict(x=x, core=core, w=w, bias=bias, C=C, B=B, K=K, O=O, size=size, F=F, cout=cout)


def head_fwd(p, policy, feat, logits):
    x = p["x"]
    return L.lib().dctn_eps_head_fwd(x.data_ptr(), L.strides5(x), p["core"].data_ptr(), p["w"].data_ptr(),
                                     p["bias"].data_ptr(), feat.data_ptr(), logits.data_ptr(), p["C"], p["B"], p["size"],
                                     p["size"], 2, p["K"], p["O"], p["cout"], L.dtype_code(x), policy, L.stream_ptr(DEV))


def head_bwd(p, policy, feat, g, d_core, d_w, d_b):
    x, lib, code = p["x"], L.lib(), L.dtype_code(p["x"])
    args = (p["C"], p["B"], p["size"], p["size"], 2, p["K"], p["O"])
    ws = L.workspace(lib.dctn_eps_head_bwd_workspace_bytes(*args, p["cout"], code, policy), DEV)
    return lib.dctn_eps_head_bwd(x.data_ptr(), L.strides5(x), feat.data_ptr(), g.data_ptr(), p["w"].data_ptr(),
                                 d_core.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), ws.data_ptr(), ws.numel(), *args,
                                 p["cout"], code, policy, L.stream_ptr(DEV))


def dcore_close(a, b):
    """dCore of two calls of the same dCore kernel (it reads no features on these shapes): at B = 1024 two row-major
    steps already differ in a few elements by up to 2^-7.2 of the largest one, so two bf16 units of it are allowed."""
    a, b = a.float(), b.float()
    return float((a - b).abs().max()) <= 2 ** -6 * float(a.abs().max())


def blocked_buffer(B, F, dtype=torch.bfloat16):
    return torch.full(((B + 3) // 4, F, 4), SENTINEL, dtype=dtype, device=DEV)


def unblock(feat, B):
    return feat.permute(0, 2, 1).reshape(-1, feat.shape[1])[:B]


def forward_both(p):
    B, F, cout = p["B"], p["F"], p["cout"]
    feat_r = torch.full((B, F), SENTINEL, dtype=torch.bfloat16, device=DEV)
    log_r = torch.full((B, cout), SENTINEL, dtype=torch.bfloat16, device=DEV)
    L.check(head_fwd(p, 0, feat_r, log_r), "row-major forward")
    feat_b, log_b = blocked_buffer(B, F), torch.full((B, cout), SENTINEL, dtype=torch.bfloat16, device=DEV)
    L.check(head_fwd(p, BLK, feat_b, log_b), "blocked4 forward")
    assert dctn_amd.last_kernel() == "eps_head_fwd_mfma_q2reg"
    torch.cuda.synchronize()
    return feat_r, log_r, feat_b, log_b


@pytest.mark.parametrize("cout", [2, 10, 16])
@pytest.mark.parametrize("B", [1, 5, 37, 1024, 1280, 2048])
def test_blocked_forward_is_the_row_major_forward_reordered(B, cout):
    p = problem(B, cout)
    feat_r, log_r, feat_b, log_b = forward_both(p)
    assert torch.equal(unblock(feat_b, B), feat_r)
    assert torch.equal(log_b, log_r)
    pad = feat_b.permute(0, 2, 1).reshape(-1, p["F"])[B:]   # the samples past the batch: written, as zeros
    assert pad.shape[0] == (-B) % 4 and bool((pad == 0).all())


@pytest.mark.parametrize("cout", [2, 10, 16])
@pytest.mark.parametrize("B", [5, 37, 1024, 1280])
def test_blocked_backward_is_bit_identical_and_reproducible(B, cout):
    """dW and dBias from blocked4 features are the row-major call's bits, and a second call gives them again."""
    p = problem(B, cout, seed=1)
    feat_r, _, feat_b, _ = forward_both(p)
    g = torch.randn(B, cout, device=DEV).bfloat16()

    def run(policy, feat):
        d_core = torch.full_like(p["core"], SENTINEL)
        d_w, d_b = torch.full_like(p["w"], SENTINEL), torch.full_like(p["bias"], SENTINEL)
        L.check(head_bwd(p, policy, feat, g, d_core, d_w, d_b), "head backward")
        assert dctn_amd.last_kernel() == "eps_head_bwd_mfma_q2reg"
        torch.cuda.synchronize()
        return d_core, d_w, d_b

    want = run(0, feat_r)
    got = run(BLK, feat_b)
    again = run(BLK, feat_b)
    for name, a, b, c in zip(("dW", "dBias"), want[1:], got[1:], again[1:]):
        assert torch.equal(b, a), name
        assert torch.equal(c, b), name + " (second call)"
    # dCore: the same kernel with either bit, held to its own run-to-run spread (dcore_close)
    for d_core in (got[0], again[0]):
        assert dcore_close(want[0], d_core), "dCore"


@pytest.mark.parametrize("case", ["out2", "n8", "small_chunks", "float32"])
def test_blocked_layout_declines_outside_the_headmm_shapes(case):
    """Out size 2, 8 factors (2x2 windows of 2 channels), DCTN_OPT_SMALL_CHUNKS and float32: both calls return
    DCTN_ERR_UNSUPPORTED and write nothing; the model then runs row-major with the same numbers."""
    kw = {"out2": dict(O=2), "n8": dict(C=2, K=2, size=13), "small_chunks": {}, "float32": dict(dtype=torch.float32)}[case]
    dtype = kw.get("dtype", torch.bfloat16)
    p = problem(37, 10, **kw)
    policy = BLK | (L.OPT_SMALL_CHUNKS if case == "small_chunks" else 0)
    feat = blocked_buffer(37, p["F"], dtype)
    logits = torch.full((37, 10), SENTINEL, dtype=dtype, device=DEV)
    assert head_fwd(p, policy, feat, logits) == L.ERR_UNSUPPORTED
    g = torch.randn(37, 10, device=DEV).to(dtype)
    d_core, d_w, d_b = torch.full_like(p["core"], SENTINEL), torch.full_like(p["w"], SENTINEL), torch.full_like(p["bias"], SENTINEL)
    assert head_bwd(p, policy, feat, g, d_core, d_w, d_b) == L.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (feat, logits, d_core, d_w, d_b):
        assert bool((t == SENTINEL).all())
    # the other entry points keep rejecting the bit
    x = p["x"]
    out = torch.full((37, p["F"]), SENTINEL, dtype=dtype, device=DEV)
    assert L.lib().dctn_eps_fwd(x.data_ptr(), L.strides5(x), p["core"].data_ptr(), out.data_ptr(), None, 0, p["C"], 37,
                                p["size"], p["size"], 2, p["K"], p["O"], L.dtype_code(x), BLK, L.stream_ptr(DEV)) == L.ERR_UNSUPPORTED

    core = p["core"].clone().requires_grad_(True)
    w, bias = p["w"].clone().requires_grad_(True), p["bias"].clone().requires_grad_(True)

    def run(blocked):
        EPL.BLOCKED_FEATURES = blocked
        try:
            for t in (core, w, bias):
                t.grad = None
            if case == "small_chunks":
                with L.options(L.OPT_SMALL_CHUNKS):
                    out = EPL._EpsLinearHeadFunction.apply(core, x, w, bias)
            else:
                out = EPL._EpsLinearHeadFunction.apply(core, x, w, bias)
            out.backward(g)
            torch.cuda.synchronize()
            return [out.detach()] + [t.grad.detach().clone() for t in (core, w, bias)]
        finally:
            EPL.BLOCKED_FEATURES = True

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def cfg2_model(B, seed=5):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    m = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, DEV, torch.bfloat16, image_size=28)
    u = torch.rand(1, B, 28, 28)
    x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).bfloat16().to(DEV)
    g = torch.randn(B, 10, device=DEV).bfloat16()
    return m, x, g


@pytest.mark.parametrize("B", [1024, 37])
def test_model_gradients_do_not_depend_on_the_layout(B):
    """EPSesPlusLinear, bf16 cfg2: logits and gradients with BLOCKED_FEATURES on equal those with it off - eager,
    replayed from a captured HIP graph, and with the core frozen (dWeight / dBias from the row-major view)."""
    m, x, g = cfg2_model(B)
    params = list(m.parameters())

    def eager(blocked):
        EPL.BLOCKED_FEATURES = blocked
        try:
            for prm in params:
                prm.grad = None
            out = m(x)
            out.backward(g)
            torch.cuda.synchronize()
            return [out.detach()] + [prm.grad.detach().clone() for prm in params if prm.requires_grad]
        finally:
            EPL.BLOCKED_FEATURES = True

    def check(got):   # [logits, dCore, dW, dBias]: dCore to one bf16 unit (see the test above), the rest bit for bit
        for i, (a, b) in enumerate(zip(want, got)):
            if i == 1:
                assert dcore_close(a, b), "dCore"
            else:
                assert torch.equal(a, b), i

    want = eager(False)
    assert dctn_amd.last_kernel() == "eps_head_bwd_mfma_q2reg"
    check(eager(True))

    # replayed from a HIP graph, the outputs dirtied between replays
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            out = m(x)
            grads = torch.autograd.grad(out, params, g)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(x)
        grads = torch.autograd.grad(out, params, g)
    for _ in range(2):
        out.fill_(float("nan"))
        for t in grads:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        check([out] + list(grads))

    # the core frozen: the node's backward takes the stand-alone head backward on the features
    m.epses[0].requires_grad_(False)
    try:
        frozen_want, frozen_got = eager(False), eager(True)
    finally:
        m.epses[0].requires_grad_(True)
    assert len(frozen_got) == 3
    for a, b in zip(frozen_want, frozen_got):
        assert torch.equal(a, b)
