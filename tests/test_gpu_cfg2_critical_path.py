"""The wrappers around the steady-state loops of the cfg2 step's two main kernels (eps_mfma.hip):

* eps_fwd_head_q2reg_t_k sums the logits from a bias staged in LDS and sends a group's blocked4 feature block in front of
  the head product (a first window sent in front of the core staging was built and dropped; its cases stay: they are
  the shapes on which most waves' first ticket is dead, a workgroup has one or two groups, a group 1-4 steps);
* eps_bwd_dcore_q2reg_k (HEADMM path) sends the first group's dLogits in front of the barrier that publishes the weight
  slice, and its waves take uneven runs of a chunk block's samples (wave_job, MfmaP::skew = spc / 3).

Exact inputs (tests/exact_inputs.py): every sum is exact in any order, so a dropped, duplicated or mis-addressed sample,
window or class shows as a bit difference in logits, dCore, dW or dBias (run_head asserts all four and the kernel names).
The oracle of a shape is computed once and shared by the two feature layouts."""
import functools

import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L
from oracle import ref_cpu as R
from tests.test_gpu_exact import HEAD_MODES, head_operands, head_oracle, run_head
from tests.test_gpu_head_blocked_features import BLK, dcore_close, forward_both, head_bwd, problem

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["fused_blocked4", "fused_rowmajor"]
FWD, BWD = "eps_head_fwd_mfma_q2reg", "eps_head_bwd_mfma_q2reg"


@functools.lru_cache(maxsize=None)
def case(size, B, cout):
    """Operands and closed-form float64 oracle of the layer C = 1, K = 3, O = 4 on size x size one-hot images."""
    ops = head_operands(1, 3, size, size, B, 4, cout, torch.bfloat16, seed=size + B + cout, two_hot=False)
    return ops, head_oracle(*ops, closed_form=True)


def check(size, B, cout, mode):
    (core, x, w, bias, g), oracle = case(size, B, cout)
    fused, ffwd, blocked = HEAD_MODES[mode]
    run_head(core, x, w, bias, g, torch.bfloat16, fused=fused, fused_fwd=ffwd, blocked=blocked, oracle=oracle, fwd=FWD, bwd=BWD,
             tag=f"{size}x{size} B={B} classes={cout} {mode}")


# ---- forward: first windows, bias from LDS, the feature block in front of the head product
# 6 x 6: one position group, F = 64 (two head k-steps for 16 waves), a group has 1-4 steps: most waves' first ticket is
# dead and must read zeros in range.  28 x 28: 11 steps < 16 waves at B = 1; B = 5: a second workgroup with one sample;
# B = 1028: workgroups with two groups, the last with one.  2 and 16 classes: the bias staging is indexed by class.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,B,cout", [(6, 1, 10), (6, 3, 10), (6, 4, 10), (6, 5, 10), (28, 1, 10), (28, 5, 10), (28, 1028, 10),
                                         (6, 5, 2), (28, 5, 16)])
def test_forward_first_window_and_bias(size, B, cout, mode):
    check(size, B, cout, mode)


# ---- dCore: dLogits in front of the barrier, uneven split of a chunk block's samples
@pytest.mark.parametrize("mode", MODES)
def test_dcore_every_clipping_of_the_ranges(mode):
    """12 x 12 (two position groups), B = 1 ... 64: young waves empty, a single live wave, ranges that end inside a group
    of 8, blocks that end inside a wave's run."""
    for B in range(1, 65):
        check(12, B, 10, mode)


# 28 x 28: 47, 48, 49 (one sample per wave, the last blocks partly empty), the headline batch (spc = 6: runs of 8 and 4),
# a batch that fills its 22 blocks exactly (1056) and spc = 23 (runs of 30 and 16: four and two groups of 8, several rounds)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [47, 48, 49, 1024, 1056, 4096])
def test_dcore_cfg2_batches(B, mode):
    check(28, B, 10, mode)


# ---- two calls on the same buffers
def dcore_f64(core_shape, x, dfeat, K=3):
    """Float64 dCore of the layer: sum over windows of (outer product of the window's K * K pixel vectors) x dFeat."""
    _, B, H, W, _ = x.shape
    Ho, Wo, O = H - K + 1, W - K + 1, dfeat.shape[-1]
    acc = torch.zeros(2 ** (K * K), O, dtype=torch.float64, device=x.device)
    for lo in range(0, B, 64):
        xs, p = x[0, lo:lo + 64], None
        for dh in range(K):
            for dw in range(K):
                f = xs[:, dh:dh + Ho, dw:dw + Wo, :].reshape(-1, 2)
                p = f if p is None else (p[:, :, None] * f[:, None, :]).reshape(f.shape[0], -1)
        acc += p.T @ dfeat[lo:lo + 64].reshape(-1, O)
    return acc.reshape(core_shape)


def test_two_calls_give_the_same_gradients():
    """B = 1024, 28 x 28, seeded inputs: dW and dBias of two calls are equal bit for bit (they do not depend on the split
    of the samples over the dCore waves), dCore within the bound of dcore_close for two runs of this kernel (2^-6 of the
    largest element) and within the cfg2 bf16 tolerance of
    tests/test_gpu_fullsize.py (2e-2 of the largest element) of the float64 gradient."""
    p = problem(1024, 10)
    feat_r, log_r, feat_b, log_b = forward_both(p)
    g = (torch.randn(1024, 10, generator=torch.Generator().manual_seed(3)) * 0.1).to(torch.bfloat16).to(DEV)
    runs = []
    for _ in range(2):
        d_core, d_w, d_b = torch.zeros_like(p["core"]), torch.zeros_like(p["w"]), torch.zeros_like(p["bias"])
        L.check(head_bwd(p, BLK, feat_b, g, d_core, d_w, d_b), "blocked4 backward")
        assert dctn_amd.last_kernel() == BWD
        runs.append((d_core, d_w, d_b))
    torch.cuda.synchronize()
    (c0, w0, b0), (c1, w1, b1) = runs
    assert torch.equal(w0, w1) and torch.equal(b0, b1)
    assert dcore_close(c0, c1)
    x64, dfeat = p["x"].double(), (g.double() @ p["w"].double()).reshape(1024, 26, 26, 4)
    want = dcore_f64(p["core"].shape, x64, dfeat)
    # the formula above against the project's oracle on three samples
    ref = R.grads(R.eps_4step, [p["core"].double().cpu(), x64[:, :3].cpu()], dfeat[:3].cpu())[0]
    got = dcore_f64(p["core"].shape, x64[:, :3], dfeat[:3]).cpu()
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    for c in (c0, c1):
        err = float((c.double() - want).abs().max())
        print(f"dCore against float64: max error {err:.3e}, largest element {float(want.abs().max()):.3e}")
        assert err < 2e-2 * float(want.abs().max())
