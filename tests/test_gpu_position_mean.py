"""`dctn_position_mean_fwd` / `_bwd` (csrc/sbs_tail.hip) and `mnist_model.position_mean` on the GPU (`-m gpu`).

The kernel sums in float64 and rounds once, so on inputs whose float64 sum is exact (integers) it must equal the float64
expression bit for bit in both dtypes; on random float32 inputs the float64 sum's own rounding can only move the result
across a float32 rounding boundary (one ulp); for float64 the error is that of P additions.  Every buffer sits in a guarded
arena: outputs start as NaN, and nothing outside them may change."""
import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd.mnist_model import position_mean
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 1), (3, 16, 10), (2, 25, 10), (2, 484, 10), (2, 7, 33), (4, 300, 1), (1, 1000, 64)]
DTYPES = [torch.float32, torch.float64]


def _fwd(y):
    """The kernel on a guarded copy of y (B, P, L); the output starts as NaN."""
    B, P, Lb = y.shape
    with guarded(fill=0xFF) as arena:
        yg = arena.place(y)
        out = arena.empty((B, Lb), y.dtype, DEV)
        assert torch.isnan(out).all()
        L.check(L.lib().dctn_position_mean_fwd(yg.data_ptr(), out.data_ptr(), B, P, Lb, L.dtype_code(y), L.stream_ptr(DEV)), "fwd")
    arena.check()
    assert torch.equal(yg, y)
    return out


def _bwd(g, P):
    B, Lb = g.shape
    with guarded(fill=0xFF) as arena:
        gg = arena.place(g)
        dy = arena.empty((B, P, Lb), g.dtype, DEV)
        L.check(L.lib().dctn_position_mean_bwd(gg.data_ptr(), dy.data_ptr(), B, P, Lb, L.dtype_code(g), L.stream_ptr(DEV)), "bwd")
    arena.check()
    assert torch.equal(gg, g)
    return dy


def _mean(y, P):
    """``y.double().sum(1).div(P).to(dtype)`` with the division done on the host: torch's device kernel divides by a Python
    number by multiplying with its rounded reciprocal, which is not the correctly rounded quotient (1 ulp off for P = 484)."""
    return torch.from_numpy(y.double().sum(1).cpu().numpy() / np.float64(P)).to(y.dtype).to(y.device)


def _spread(g, P, shape):
    """``(g.double() / P).to(dtype)`` over the positions, divided on the host likewise."""
    q = torch.from_numpy(g.double().cpu().numpy() / np.float64(P)).to(g.dtype).to(g.device)
    return q.reshape((shape[0],) + (1,) * (len(shape) - 2) + (shape[-1],)).expand(shape)


def _integers(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_inputs_equal_the_float64_expression_bit_for_bit(shape, dtype):
    B, P, Lb = shape
    y = _integers(shape, dtype, 1)
    out = _fwd(y)
    assert out.dtype == dtype and torch.equal(out, _mean(y, P))
    g = _integers((B, Lb), dtype, 2)
    dy = _bwd(g, P)
    assert dy.dtype == dtype and torch.equal(dy, _spread(g, P, (B, P, Lb)))


@pytest.mark.parametrize("shape", SHAPES)
def test_random_float32_forward_is_within_one_ulp(shape):
    B, P, Lb = shape
    y = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    out = _fwd(y).cpu().numpy()
    want = _mean(y, P).cpu().numpy()
    ulps = np.abs(out.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"\n{shape}: max error {ulps.max():.3f} ulp")
    assert ulps.max() <= 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_random_float64_forward_error_is_that_of_P_additions(shape):
    B, P, Lb = shape
    y = torch.randn(shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    import math

    want = torch.tensor([[math.fsum(y[b, :, l].tolist()) / P for l in range(Lb)] for b in range(B)], dtype=torch.float64)
    out = _fwd(y.to(DEV)).cpu()
    bound = P * 2.0 ** -53 * y.abs().mean(1)
    err = (out - want).abs()
    print(f"\n{shape}: max error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,Lb", [(25, 10), (484, 10), (7, 33), (1000, 64)])
def test_a_sample_has_the_same_bits_whatever_batch_it_sits_in(P, Lb, dtype):
    y = torch.randn((4, P, Lb), generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    whole = _fwd(y)
    for b in range(4):
        assert torch.equal(_fwd(y[b : b + 1].clone()), whole[b : b + 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_from_an_unaligned_gradient_buffer(dtype):
    """dy one element into its storage: the one-element-per-thread form, nothing written in front of it."""
    B, P, Lb = 2, 25, 10
    g = _integers((B, Lb), dtype, 6)
    with guarded(fill=0xFF) as arena:
        store = arena.empty((B * P * Lb + 1,), dtype, DEV)
        dy = store[1:]
        L.check(L.lib().dctn_position_mean_bwd(g.data_ptr(), dy.data_ptr(), B, P, Lb, L.dtype_code(g), L.stream_ptr(DEV)), "bwd")
    arena.check()
    assert torch.isnan(store[0])
    assert torch.equal(dy.view(B, P, Lb), _spread(g, P, (B, P, Lb)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_through_position_mean(dtype):
    y = _integers((3, 4, 5, 10), dtype, 7).requires_grad_(True)
    w = _integers((3, 10), dtype, 8)
    out = position_mean(y)
    (out * w).sum().backward()
    assert out.shape == (3, 10)
    assert torch.equal(out, _mean(y.detach().reshape(3, 20, 10), 20))
    assert torch.equal(y.grad, _spread(w, 20, (3, 4, 5, 10)))
    # a CPU tensor is staged to the device and the result comes back (the project's boundary rule)
    yc = y.detach().cpu().requires_grad_(True)
    oc = position_mean(yc)
    oc.sum().backward()
    assert oc.device.type == "cpu" and torch.equal(oc, out.detach().cpu()) and yc.grad.device.type == "cpu"
