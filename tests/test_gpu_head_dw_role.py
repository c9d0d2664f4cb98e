"""The head weight gradient of the fused backward with blocked4 features is formed by four extra waves of the dCore
workgroups (head_dw_role_waves in eps_mfma.hip), as 16 virtual waves with the finishing kernel's sample split,
accumulation order and ordered join.  The row-major call still forms it in the finishing kernel's product role, so
the two must agree bit for bit: at batches of one block, of part blocks, of several rounds of loads per wave, with
more slices than workgroups (28 x 28 images, small batches: the slices past the first round go to single waves) and
with fewer (12 x 12 images)."""
import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BLK = L.OPT_HEAD_FEATURES_BLOCKED4
SENTINEL = -12345.0   # exactly representable in bf16


def problem(B, cout, size, seed=0):
    torch.manual_seed(seed + 7 * B + cout + 1000 * size)
    K, O = 3, 4
    u = torch.rand(1, B, size, size)
    x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).bfloat16().to(DEV)
    core = (torch.randn(*(2,) * (K * K), O) * 2 ** (-K * K / 4)).bfloat16().to(DEV)
    F = (size - K + 1) ** 2 * O
    w = (torch.randn(cout, F) * F ** -0.5).bfloat16().to(DEV)
    bias = torch.randn(cout).bfloat16().to(DEV)
    g = torch.randn(B, cout, device=DEV).bfloat16()
    return dict(x=x, core=core, w=w, bias=bias, g=g, B=B, K=K, O=O, size=size, F=F, cout=cout)


def _args(p):
    return (1, p["B"], p["size"], p["size"], 2, p["K"], p["O"])


def forward(p, policy):
    B, F, cout, x = p["B"], p["F"], p["cout"], p["x"]
    shape = ((B + 3) // 4, F, 4) if policy & BLK else (B, F)
    feat = torch.full(shape, SENTINEL, dtype=torch.bfloat16, device=DEV)
    logits = torch.full((B, cout), SENTINEL, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().dctn_eps_head_fwd(x.data_ptr(), L.strides5(x), p["core"].data_ptr(), p["w"].data_ptr(),
                                      p["bias"].data_ptr(), feat.data_ptr(), logits.data_ptr(), *_args(p), p["cout"],
                                      L.dtype_code(x), policy, L.stream_ptr(DEV)), "head forward")
    return feat


def backward(p, policy, feat, d_w=None):
    """-> (status, dCore, dW, dBias); d_w: the (cout, F) view to write, else a sentinel-filled tensor of its own."""
    x, lib, code = p["x"], L.lib(), L.dtype_code(p["x"])
    ws = L.workspace(lib.dctn_eps_head_bwd_workspace_bytes(*_args(p), p["cout"], code, policy), DEV)
    d_core = torch.full_like(p["core"], SENTINEL)
    d_w = torch.full_like(p["w"], SENTINEL) if d_w is None else d_w
    d_b = torch.full_like(p["bias"], SENTINEL)
    status = lib.dctn_eps_head_bwd(x.data_ptr(), L.strides5(x), feat.data_ptr(), p["g"].data_ptr(), p["w"].data_ptr(),
                                   d_core.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), ws.data_ptr(), ws.numel(), *_args(p),
                                   p["cout"], code, policy, L.stream_ptr(DEV))
    torch.cuda.synchronize()
    return L.check(status, "head backward"), d_core, d_w, d_b


@pytest.mark.parametrize("size", [28, 12])
@pytest.mark.parametrize("cout", [2, 10, 16])
@pytest.mark.parametrize("B", [1, 4, 8, 33, 64, 1000, 1024, 2048, 4096])
def test_role_waves_give_the_finishing_kernels_bits(B, cout, size):
    p = problem(B, cout, size)
    _, _, want_w, want_b = backward(p, 0, forward(p, 0))
    assert dctn_amd.last_kernel() == "eps_head_bwd_mfma_q2reg"
    _, _, got_w, got_b = backward(p, BLK, forward(p, BLK))
    assert dctn_amd.last_kernel() == "eps_head_bwd_mfma_q2reg"
    assert not bool((got_w == SENTINEL).any()), "every element of dW is written"
    assert torch.equal(got_w, want_w), "dW"
    assert torch.equal(got_b, want_b), "dBias"


@pytest.mark.parametrize("size", [28, 12])
@pytest.mark.parametrize("cout", [2, 10])
@pytest.mark.parametrize("B", [5, 1024])
def test_role_waves_write_nothing_outside_dw(B, cout, size):
    """dW sits inside a larger sentinel-filled buffer: the 16 - cout classes a tile has beyond the head's and the
    features a last slice has beyond F must not be stored."""
    p = problem(B, cout, size, seed=2)
    F = p["F"]
    pad = 16 * F   # room for every row a 16-class tile could name
    buf = torch.full((pad + cout * F + pad,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    d_w = buf[pad:pad + cout * F].view(cout, F)
    backward(p, BLK, forward(p, BLK), d_w=d_w)
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + cout * F:] == SENTINEL).all())
    _, _, want_w, _ = backward(p, 0, forward(p, 0))
    assert torch.equal(d_w, want_w)


@pytest.mark.parametrize("B", [5, 1024])
def test_main_kernel_only_then_full_call(B):
    """DCTN_OPT_MAIN_KERNEL_ONLY launches the dCore kernel alone, which with blocked4 features also writes dW; a full
    call after it gives the full call's bits, and the main kernel's dW is already that."""
    p = problem(B, 10, 28, seed=3)
    feat = forward(p, BLK)
    _, want_core, want_w, want_b = backward(p, BLK, feat)
    status, _, part_w, part_b = backward(p, BLK | L.OPT_MAIN_KERNEL_ONLY, feat)
    assert status == L.PARTIAL
    assert torch.equal(part_w, want_w)
    assert bool((part_b == SENTINEL).all())   # the finishing kernel did not run
    status, got_core, got_w, got_b = backward(p, BLK, feat)
    assert status == 0
    assert torch.equal(got_w, want_w) and torch.equal(got_b, want_b)
    a, b = want_core.float(), got_core.float()   # dCore: the kernel's own run-to-run spread (dcore_close of test_gpu_head_blocked_features)
    assert float((a - b).abs().max()) <= 2 ** -6 * float(a.abs().max())
