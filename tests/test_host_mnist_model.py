"""What the ConvSBS classifier promises without a GPU: the exports of library version 518 and their pinned return codes
(all decided on the host before any launch), the reference's module tree, the feature map's byte table, the float64
moment arithmetic of the calibration, and the golden fixture's own consistency."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

from dctn_amd import _lib
from dctn_amd.batches import feature_table
from dctn_amd.conv_sbs import DumbNormalInitialization
from dctn_amd.mnist_model import DCTNMnistModel, batch_to_quantum, position_mean, quantum_phi, string_scales
from dctn_amd.tensor_stats import OutputStats, combine_moments, std_from_moments

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mnist_model_*.npz")))
F32_TOL = dict(rtol=2e-4, atol=2e-5)   # the project's float32 TOL (tests/test_gpu_parity.py)
PTR = 4096   # any non-null, 16-byte aligned number: the calls below return before they would use it


def test_exports_and_version():
    lib = _lib.lib()
    assert lib.dctn_version() >= 518
    for name in ("dctn_position_mean_fwd", "dctn_position_mean_bwd", "dctn_tensor_stats", "dctn_tensor_stats_record_bytes",
                 "dctn_tensor_stats_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dctn_tensor_stats_record_bytes() == 64
    assert lib.dctn_tensor_stats_workspace_bytes(0) == 0
    assert lib.dctn_tensor_stats_workspace_bytes(8) == 8 * lib.dctn_tensor_stats_workspace_bytes(1) > 0


@pytest.mark.parametrize("entry", ["dctn_position_mean_fwd", "dctn_position_mean_bwd"])
def test_position_mean_return_codes(entry):
    fn = getattr(_lib.lib(), entry)
    assert fn(None, PTR, 2, 3, 10, _lib.F32, None) == _lib.ERR_NULL
    assert fn(PTR, None, 2, 3, 10, _lib.F32, None) == _lib.ERR_NULL
    assert fn(PTR, PTR, 0, 3, 10, _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert fn(PTR, PTR, 2, 0, 10, _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert fn(PTR, PTR, 2, 3, 10, _lib.BF16, None) == _lib.ERR_BAD_DTYPE
    assert fn(PTR, PTR, 2, 3, 65, _lib.F32, None) == _lib.ERR_UNSUPPORTED
    assert fn(PTR, PTR, 2, 3, 0, _lib.F64, None) == _lib.ERR_UNSUPPORTED
    # the project's order: NULL, shape, dtype, unsupported
    assert fn(None, PTR, 0, 3, 65, _lib.BF16, None) == _lib.ERR_NULL
    assert fn(PTR, PTR, 0, 3, 65, _lib.BF16, None) == _lib.ERR_BAD_SHAPE
    assert fn(PTR, PTR, 2, 3, 65, _lib.BF16, None) == _lib.ERR_BAD_DTYPE


def test_tensor_stats_return_codes():
    lib = _lib.lib()
    ptrs, counts = (ctypes.c_void_p * 9)(*[PTR] * 9), (ctypes.c_int64 * 9)(*[5] * 9)
    big = lib.dctn_tensor_stats_workspace_bytes(8)
    call = lambda p, c, n, rec=PTR, ws=PTR, nbytes=big, dtype=_lib.F32: lib.dctn_tensor_stats(p, c, n, rec, ws, nbytes, dtype, None)
    assert call(None, counts, 8) == call(ptrs, None, 8) == call(ptrs, counts, 8, rec=None) == call(ptrs, counts, 8, ws=None) \
        == _lib.ERR_NULL
    assert call(ptrs, counts, 9) == call(ptrs, counts, 0) == _lib.ERR_BAD_SHAPE
    counts[3] = 0
    assert call(ptrs, counts, 8) == _lib.ERR_BAD_SHAPE
    assert call(ptrs, counts, 8, dtype=_lib.BF16) == _lib.ERR_BAD_SHAPE   # shape before dtype
    counts[3] = 5
    assert call(ptrs, counts, 8, dtype=_lib.BF16) == _lib.ERR_BAD_DTYPE
    assert call(ptrs, counts, 8, nbytes=big - 1) == _lib.ERR_WORKSPACE
    ptrs[7] = None
    assert call(ptrs, counts, 8) == _lib.ERR_NULL


def test_the_module_tree_is_the_references():
    model = DCTNMnistModel(3, 2, False, DumbNormalInitialization(0.5), False, 1.0)
    want = [f"conv_sbses.{layer}.strings.{string}.cores.{core}" for layer, strings in enumerate((2, 2, 1))
            for string in range(strings) for core in range(9)]
    assert list(model.state_dict()) == want and len(want) == 45
    assert model.string_names() == ["conv_sbses.0.strings.0", "conv_sbses.0.strings.1", "conv_sbses.1.strings.0",
                                    "conv_sbses.1.strings.1", "conv_sbses.2.strings.0"]
    assert tuple(model.conv_sbses[2].strings[0].cores[4].shape) == (10, 2, 2, 2, 2)
    assert tuple(model.conv_sbses[0].strings[1].cores[0].shape) == (1, 1, 2, 2)
    ring = DCTNMnistModel(2, 3, True, DumbNormalInitialization(0.5), True, 1.3)
    assert len(ring.state_dict()) == 27 and tuple(ring.conv_sbses[1].strings[0].cores[0].shape) == (1, 3, 3, 2, 2)
    with pytest.raises(AssertionError):
        DCTNMnistModel(1, 2, False, DumbNormalInitialization(0.5), False, 1.0)


@pytest.mark.parametrize("name", [os.path.basename(f) for f in FIXTURES])
def test_a_reference_checkpoint_loads(name):
    g = dict(np.load(os.path.join(GOLDEN, name)))
    model = DCTNMnistModel(int(g["layers"]), int(g["bond"]), bool(g["trace_edge"]), DumbNormalInitialization(0.5),
                           bool(g["cos_sin_squared"]), float(g["multiplier"]))
    names = [str(n) for n in g["names"]]
    model.load_state_dict({n: torch.from_numpy(g[f"cal32_{k}"]) for k, n in enumerate(names)}, strict=True)
    assert list(model.state_dict()) == names


@pytest.mark.parametrize("multiplier", [1.0, 0.7])
@pytest.mark.parametrize("cos_sin_squared", [False, True])
def test_the_byte_table_is_batch_to_quantum_bit_for_bit(cos_sin_squared, multiplier):
    table = feature_table(quantum_phi(cos_sin_squared), multiplier, torch.float32)
    u = (torch.arange(256, dtype=torch.uint8).float() / 255.0).reshape(256, 1, 1, 1)
    want = batch_to_quantum(u, cos_sin_squared, multiplier).reshape(256, 2)
    assert table.shape == (256, 2) and torch.equal(table, want)
    # the reference's expression, written out
    s, c = torch.sin(u[:, 0]), torch.cos(u[:, 0])
    ref = torch.stack((s ** 2, c ** 2) if cos_sin_squared else (s, c), dim=3) * multiplier
    assert torch.equal(want, ref.reshape(256, 2))


@pytest.mark.parametrize("n,offset", [(2, 0), (100, 0), (4097, 1000), (200000, 30000)])
def test_std_from_moments_against_the_two_pass_std(n, offset):
    """Integer data: n, sum and sum of squares are exact, so the only error is the cancellation in ss - s^2 / n, whose
    relative size is kappa * 2^-52 per operation with kappa = sum y^2 / (n var)."""
    y = np.random.default_rng(n).integers(-50, 51, n).astype(np.float64) + offset
    s, ss = float(y.sum()), float((y * y).sum())
    want = float(np.std(y, ddof=1))
    kappa = ss / (n * np.var(y))
    got = std_from_moments(n, s, ss)
    print(f"\nn={n} offset={offset}: kappa={kappa:.3e}, relative error {abs(got - want) / want:.3e}, bound {kappa * n * 2.0 ** -52:.3e}")
    assert abs(got - want) <= kappa * n * 2.0 ** -52 * want
    assert math.isnan(std_from_moments(1, 3.0, 9.0)) and std_from_moments(5, 10.0, 20.0) == 0.0


def test_combine_moments_of_two_shards_is_the_whole_exactly():
    y = np.random.default_rng(7).integers(-1000, 1001, 5001).astype(np.float64)
    triple = lambda v: (float(v.size), float(v.sum()), float((v * v).sum()))
    assert combine_moments([triple(y[:1234]), triple(y[1234:])]) == triple(y)
    assert combine_moments([triple(y)]) == triple(y)


def test_calibration_scales_with_an_injected_reduce_that_doubles_the_shard():
    """Two ranks holding the same shard: the union has 2n elements, and its unbiased std is not the shard's."""
    rng = np.random.default_rng(3)
    shards = [rng.integers(-9, 10, 640).astype(np.float64), rng.integers(0, 5, 640).astype(np.float64)]
    rows = [(v.size, v.sum(), (v * v).sum(), 0.0) for v in shards]
    seen = []

    def doubled(r):
        seen.append(r)
        return [tuple(2 * x for x in row) for row in r]

    got = string_scales(rows, doubled)
    assert len(seen) == 1 and seen[0] == [tuple(float(x) for x in row) for row in rows]
    for std, v in zip(got, shards):
        assert std == pytest.approx(np.std(np.concatenate([v, v]), ddof=1), rel=1e-13)
        assert std != pytest.approx(np.std(v, ddof=1), rel=1e-6)
    alone = string_scales(rows, lambda r: r)
    assert alone == [std_from_moments(*row[:3]) for row in rows]
    # a string is skipped (None) when its std is 0, when an output was non-finite on ANY rank, or with a single element
    assert string_scales([(4, 8.0, 16.0, 0.0), (640, 1.0, 9.0, 0.0), (1, 2.0, 4.0, 0.0)], lambda r: r)[::2] == [None, None]
    assert string_scales([rows[0][:3] + (0.0,)], lambda r: [r[0][:3] + (1.0,)]) == [None]


@pytest.mark.parametrize("name", [os.path.basename(f) for f in FIXTURES])
def test_the_fixtures_float32_values_agree_with_its_float64_ones(name):
    g = dict(np.load(os.path.join(GOLDEN, name)))
    n = len(g["names"])
    assert n == {3: 45, 2: 27}[int(g["layers"])]

    def close(a32, a64):
        a64 = np.asarray(a64, dtype=np.float64)
        scale = float(np.abs(a64).max()) or 1.0
        return np.allclose(np.asarray(a32, dtype=np.float64), a64, rtol=F32_TOL["rtol"], atol=F32_TOL["atol"] * scale)

    assert g["logits32"].dtype == np.float32 and g["logits64"].dtype == np.float64
    assert close(g["logits32"], g["logits64"]) and close(g["loss32"], g["loss64"])
    for k in range(n):
        assert g[f"cal32_{k}"].dtype == np.float32 and g[f"grad64_{k}"].dtype == np.float64
        assert close(g[f"cal32_{k}"], g[f"cal64_{k}"]), k
        assert close(g[f"grad32_{k}"], g[f"grad64_{k}"]), k
        assert np.array_equal(g[f"init_{k}"].astype(np.float32).astype(np.float64), g[f"init_{k}"])
    assert np.isfinite(g["logits64"]).all() and g["images"].shape[1] == 1 and g["labels"].dtype == np.int64


@pytest.mark.skipif(torch.cuda.is_available(), reason="what the calls do where there is no GPU")
def test_without_a_gpu_the_calls_raise():
    with pytest.raises(RuntimeError):
        OutputStats(torch.device("cpu"), ["a"])
    with pytest.raises(RuntimeError):
        position_mean(torch.zeros(2, 3, 10))
    model = DCTNMnistModel(2, 2, False, DumbNormalInitialization(0.5), False, 1.0)
    with pytest.raises(RuntimeError):
        model(torch.zeros(2, 1, 8, 8))
