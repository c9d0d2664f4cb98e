"""What preparing a colour (or grey) source from its bytes promises without a GPU: the exports of version 517, the return
codes of `dctn_byte_histogram` / `dctn_byte_window_stats` before any launch, `moments_from_counts` against
`channel_moments`, `colour_table(nu_constant=...)`, the float64 tables of the statistics kernel and the argument errors of
the new `from_colour` / `DeviceBatches` arguments."""
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd import batches as B
from dctn_amd import window_stats as WS

PTR = 4096   # any non-NULL, 8-byte aligned address: the checks below return before anything is read


def test_exports_and_version():
    lib = L.lib()
    assert lib.dctn_version() >= 517
    for name in ("dctn_byte_histogram", "dctn_byte_window_stats", "dctn_byte_window_stats_workspace_bytes"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.dctn_byte_window_stats_workspace_bytes(0) == 0
    assert lib.dctn_byte_window_stats_workspace_bytes(1) == 32 and lib.dctn_byte_window_stats_workspace_bytes(10880) == 10880 * 16 + 16


def test_histogram_return_codes_before_any_launch():
    h = L.lib().dctn_byte_histogram
    assert h(None, 10, 3, PTR, None) == L.ERR_NULL and h(PTR, 10, 3, None, None) == L.ERR_NULL
    assert h(None, 0, 3, PTR, None) == L.ERR_NULL          # NULL comes first
    assert h(PTR, 0, 3, PTR, None) == L.ERR_BAD_SHAPE
    assert h(PTR, 10, 0, PTR, None) == L.ERR_BAD_SHAPE and h(PTR, 10, 5, PTR, None) == L.ERR_BAD_SHAPE
    assert h(PTR, 0, 3, PTR + 4, None) == L.ERR_BAD_SHAPE   # shape before unsupported
    assert h(PTR, 10, 3, PTR + 4, None) == L.ERR_UNSUPPORTED   # int64 counts off their alignment


def test_window_stats_return_codes_before_any_launch():
    w = L.lib().dctn_byte_window_stats

    def call(src=PTR, n=2, H=5, W=5, C=3, tu=PTR, K=3, ws=PTR, sums=PTR):
        return w(src, n, H, W, C, tu, 0.0, 0.0, K, ws, sums, None)

    for missing in ("src", "tu", "ws", "sums"):
        assert call(**{missing: None}) == L.ERR_NULL
    assert call(src=None, n=0) == L.ERR_NULL
    assert call(n=0) == L.ERR_BAD_SHAPE and call(n=1 << 31) == L.ERR_BAD_SHAPE
    assert call(C=0) == L.ERR_BAD_SHAPE and call(C=5) == L.ERR_BAD_SHAPE
    assert call(H=2) == L.ERR_BAD_SHAPE and call(W=2) == L.ERR_BAD_SHAPE and call(K=0) == L.ERR_BAD_SHAPE
    assert call(H=2, ws=PTR + 4) == L.ERR_BAD_SHAPE
    # 16 * (3 * 256 + 100 * 100) + 80 = 172 368 bytes: more than 15/16 of a CU's 160 KiB
    assert call(H=100, W=100) == L.ERR_UNSUPPORTED
    assert call(ws=PTR + 4) == L.ERR_UNSUPPORTED


def test_python_dtype_and_shape_errors_need_no_device():
    table = B.colour_table(3, nu=1.0, dtype=torch.float32)
    with pytest.raises(TypeError):
        B.byte_histogram(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError):
        B.byte_histogram(torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        B.byte_histogram(torch.zeros(0, 3, dtype=torch.uint8))
    images = torch.zeros(2, 5, 5, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        WS.calc_scaling_factor_from_bytes(images.float(), table, 3)
    with pytest.raises(TypeError):
        WS.calc_scaling_factor_from_bytes(images, table.double(), 3)
    with pytest.raises(ValueError):
        WS.calc_scaling_factor_from_bytes(images, table, 6)
    with pytest.raises(ValueError):
        WS.calc_scaling_factor_from_bytes(images, table[:2], 3)
    with pytest.raises(ValueError):
        WS.calc_scaling_factor_from_bytes(images, table, 3, samples=0)
    with pytest.raises(TypeError):
        B.moments_from_counts(torch.zeros(3, 256))


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_moments_from_counts_are_channel_moments_bit_for_bit(C):
    g = torch.Generator().manual_seed(100 + C)
    images = torch.randint(0, 256, (13, 7, 9, C), dtype=torch.uint8, generator=g)
    flat = images.reshape(-1, C)
    counts = torch.stack([torch.bincount(flat[:, c].long(), minlength=256) for c in range(C)])
    mean, std = B.moments_from_counts(counts)
    want_mean, want_std = B.channel_moments(images)
    assert mean.dtype == std.dtype == torch.float64 and mean.shape == std.shape == (C,)
    assert torch.equal(mean, want_mean) and torch.equal(std, want_std)


def test_nu_constant_defaults_to_one_and_scales_the_constant_column_only():
    kw = dict(nu=(0.5, 2.0, 3.0), mean=torch.tensor([0.1, 0.2, 0.3]), std=torch.tensor([0.5, 0.6, 0.7]),
              constant_channel=0.25, dtype=torch.float32)
    base = B.colour_table(3, **kw)
    assert torch.equal(B.colour_table(3, nu_constant=1.0, **kw), base)
    scaled = B.colour_table(3, nu_constant=3.0, **kw)
    assert torch.equal(scaled[:3], base[:3])
    assert torch.equal(scaled[3], torch.full((256,), 0.25) * torch.tensor(3.0))
    # the reference's autoscale, one factor on all four columns (dataset_loading.py:372), is nu = nu_constant
    nu = 0.7312345678901234
    t = torch.arange(256, dtype=torch.uint8).float().div(255).unsqueeze(1).repeat(1, 3)
    t = torch.cat((t, 0.25 * torch.ones_like(t[:, :1])), dim=1)
    t *= torch.tensor((nu, nu, nu, nu))
    assert torch.equal(B.colour_table(3, nu=nu, constant_channel=0.25, dtype=torch.float32, nu_constant=nu), t.t())


def test_the_statistics_tables_hold_the_float32_values_in_float64():
    table = B.colour_table(3, nu=1.0, mean=torch.tensor([0.4, 0.5, 0.6]), std=torch.tensor([0.2, 0.25, 0.3]),
                           constant_channel=0.5, dtype=torch.float32)
    tu, t0, u0 = WS._byte_tables(table, 3, False)
    assert tu.shape == (3, 256, 2) and tu.dtype == torch.float64 and tu.is_contiguous()
    assert torch.equal(tu[..., 0], table[:3].double()) and torch.equal(tu[..., 1], table[:3].double() ** 2)
    assert (t0, u0) == (0.5, 0.25)
    plain = B.colour_table(4, nu=1.0, dtype=torch.float32)
    assert WS._byte_tables(plain, 4, False)[1:] == (0.0, 0.0)
    grey = B.feature_table(WS.φ_cos_sin_squared_1, 1.0, torch.float32).t().contiguous()
    tu, t0, u0 = WS._byte_tables(grey, 1, True)
    assert tu.shape == (1, 256, 2) and (t0, u0) == (0.0, 0.0)
    assert torch.equal(tu[0, :, 0], grey[0].double() + grey[1].double())
    assert torch.equal(tu[0, :, 1], grey[0].double() ** 2 + grey[1].double() ** 2)


def _colour(**kw):
    images = torch.zeros(6, 8, 8, 3, dtype=torch.uint8)
    args = dict(dtype=torch.float32, seed=1)
    args.update(kw)
    return B.DeviceBatches.from_colour(images, torch.zeros(6, dtype=torch.long), 2, **args)


def test_from_colour_argument_errors_come_before_the_device():
    with pytest.raises(ValueError, match="exactly one of nu and autoscale_kernel_size"):
        _colour()
    with pytest.raises(ValueError, match="exactly one of nu and autoscale_kernel_size"):
        _colour(nu=1.0, autoscale_kernel_size=3)
    with pytest.raises(ValueError, match="excludes mean and std"):
        _colour(nu=1.0, center_and_normalize=True, mean=torch.zeros(3), std=torch.ones(3))
    with pytest.raises(ValueError, match="excludes mean and std"):
        _colour(autoscale_kernel_size=3, center_and_normalize=True, mean=torch.zeros(3))
    with pytest.raises(ValueError, match="autoscale_kernel_size is an integer"):
        _colour(autoscale_kernel_size=9)
    with pytest.raises(ValueError, match="autoscale_kernel_size is an integer"):
        _colour(autoscale_kernel_size=0)
    with pytest.raises(ValueError, match="autoscale_samples"):
        _colour(autoscale_kernel_size=3, autoscale_samples=0)
    with pytest.raises(ValueError, match="excludes nu_constant"):
        _colour(autoscale_kernel_size=3, nu_constant=2.0)
    with pytest.raises(NotImplementedError):   # the table's own errors still come first
        B.DeviceBatches.from_colour(torch.zeros(6, 8, 8, 4, dtype=torch.uint8), torch.zeros(6, dtype=torch.long), 2,
                                    dtype=torch.float32, seed=1, autoscale_kernel_size=3, constant_channel=1.0)
    with pytest.raises(ValueError, match="global batch"):   # and `_plan`'s after them, as before
        B.DeviceBatches.from_colour(torch.zeros(6, 8, 8, 3, dtype=torch.uint8), torch.zeros(6, dtype=torch.long), 7,
                                    dtype=torch.float32, seed=1, autoscale_kernel_size=3, center_and_normalize=True)


def test_grey_autoscale_argument_errors_come_before_the_device():
    images, labels = torch.zeros(6, 8, 8, dtype=torch.uint8), torch.zeros(6, dtype=torch.long)
    with pytest.raises(ValueError, match="computes the scale"):
        B.DeviceBatches(images, labels, 2, dtype=torch.float32, seed=1, scale=0.5, autoscale_kernel_size=3)
    with pytest.raises(ValueError, match="autoscale_kernel_size is an integer"):
        B.DeviceBatches(images, labels, 2, dtype=torch.float32, seed=1, autoscale_kernel_size=9)
    with pytest.raises(ValueError, match="autoscale_samples"):
        B.DeviceBatches(images, labels, 2, dtype=torch.float32, seed=1, autoscale_kernel_size=3, autoscale_samples=-1)
