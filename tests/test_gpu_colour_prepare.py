"""Preparing a source from its bytes on the GPU (`-m gpu`): the per-channel histogram bit for bit against torch.bincount
on the CPU (every load path, guarded and poisoned outputs), the window statistics through a table against the oracle on the
CPU-expanded tensor (a bound from the oracle's own per-window terms, identical bits on every launch, exact and stale
workspaces), and the reference's colour pipeline - centre, normalise, constant channel, autoscale - end to end through
`DeviceBatches.from_colour`, with the grey source's autoscale beside it."""
import functools

import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd import batches as B
from dctn_amd import window_stats as WS
from oracle import ref_cpu as R
from tests.guarded_buffers import StalePool, guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, GUARD_BYTE, STALE_BYTE = 256, 0xA5, 0xFF


class Framed:
    """A tensor inside a guarded byte allocation (the pattern of tests/test_gpu_colour_source.py): guards of 0xA5 on both
    sides, an output (``values`` None) poisoned with 0xFF; ``shift`` moves the payload off the allocation's alignment."""

    def __init__(self, shape, dtype, values=None, shift=0):
        numel = 1
        for s in shape:
            numel *= s
        self.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + self.nbytes + 16,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + shift
        body = self.raw[self.lo : self.lo + self.nbytes]
        body.fill_(STALE_BYTE)
        self.view = body.view(dtype).view(shape)
        if values is not None:
            self.view.copy_(values)
        self.before = self.raw.clone()

    def guards_intact(self):
        a, b = self.raw, self.before
        return torch.equal(a[: self.lo], b[: self.lo]) and torch.equal(a[self.lo + self.nbytes :], b[self.lo + self.nbytes :])

    def untouched(self):
        return torch.equal(self.raw, self.before)


def _bytes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    images.view(-1)[0], images.view(-1)[-1] = 0, 255
    return images


def _bincount(images):
    C = images.shape[-1]
    flat = images.reshape(-1, C)
    return torch.stack([torch.bincount(flat[:, c].long(), minlength=256) for c in range(C)])


# ------------------------------------------------------------------ 1. the histogram
def _raw_histogram(images, first=0, shift=0):
    """dctn_byte_histogram over ``images[first:]``, the whole tensor placed ``shift`` bytes off its alignment."""
    C = images.shape[-1]
    src = Framed(tuple(images.shape), torch.uint8, images, shift=shift)
    counts = Framed((C, 256), torch.int64)
    part = src.view[first:]
    rc = L.lib().dctn_byte_histogram(part.data_ptr(), part.numel() // C, C, counts.view.data_ptr(), L.stream_ptr(DEV))
    assert rc == 0 and dctn_amd.last_kernel() == "byte_histogram"
    torch.cuda.synchronize()
    assert counts.guards_intact() and src.untouched()
    return counts.view.cpu(), part.data_ptr()


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "base_off_by_one"])
@pytest.mark.parametrize("first", [0, 1], ids=["whole", "from_sample_1"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_histogram_equals_bincount_on_every_load_path(C, first, shift):
    """(5, 7, 9, C): 63 pixels a sample, no multiple of four.  From sample 1 the bytes start 63 C bytes in (odd for odd C), and
    one byte further with the shifted base: head pixels in front of the 32-bit loads for odd C, byte loads throughout for
    C = 2 and 4 at an odd address, a tail behind the last group of four in every case."""
    images = _bytes((5, 7, 9, C), 40 + C)
    got, address = _raw_histogram(images, first, shift)
    assert address % 2 == (63 * C * first + shift) % 2
    assert torch.equal(got, _bincount(images[first:]))


@pytest.mark.parametrize("C", [1, 3, 4])
def test_histogram_of_a_single_pixel(C):
    images = _bytes((1, 1, 1, C), 50 + C)
    got, _ = _raw_histogram(images)
    assert torch.equal(got, _bincount(images)) and int(got.sum()) == C


def test_histogram_when_every_increment_hits_one_counter():
    images = torch.full((64, 32, 32, 3), 255, dtype=torch.uint8)
    got, _ = _raw_histogram(images)
    want = torch.zeros(3, 256, dtype=torch.int64)
    want[:, 255] = 64 * 32 * 32
    assert torch.equal(got, want)


def test_histogram_of_random_images_and_the_moments_from_it():
    images = _bytes((64, 32, 32, 3), 60)
    got, _ = _raw_histogram(images)
    assert torch.equal(got, _bincount(images))
    counts = B.byte_histogram(images)          # CPU bytes are staged
    assert counts.device == DEV and counts.dtype == torch.int64 and torch.equal(counts.cpu(), got)
    assert torch.equal(B.byte_histogram(images.to(DEV)[3:]).cpu(), _bincount(images[3:]))
    want_mean, want_std = B.channel_moments(images)
    for source in (images, images.to(DEV)):
        mean, std = B.colour_moments(source)
        assert mean.device.type == "cpu" and mean.dtype == torch.float64
        assert torch.equal(mean, want_mean) and torch.equal(std, want_std)


# ------------------------------------------------------------------ 2. window statistics through a table
def _expand(table, images):
    """The (1, n, H, W, columns) tensor the table stands for, on the CPU, in the table's float32: column c reads channel c,
    a column behind the channels its entry 0; for grey (n, H, W) images every column reads the one byte."""
    if images.ndim == 3:
        return torch.stack([table[q][images.long()] for q in range(table.shape[0])], dim=-1).unsqueeze(0)
    C = images.shape[-1]
    cols = [table[c][images[..., c].long()] for c in range(C)]
    cols += [table[c][torch.zeros_like(images[..., 0]).long()] for c in range(C, table.shape[0])]
    return torch.stack(cols, dim=-1).unsqueeze(0)


def _abs_first_terms(x, K):
    """sum_w |prod t| with the oracle's own per-window terms (`oracle.ref_cpu.window_sums`'s loop, C = 1)."""
    _, B_, H, W, _ = x.shape
    ps = torch.ones(B_, H - K + 1, W - K + 1, dtype=torch.float64)
    for dh in range(K):
        for dw in range(K):
            ps = ps * x[0, :, dh : dh + H - K + 1, dw : dw + W - K + 1, :].double().sum(-1)
    return float(ps.abs().sum())


@functools.lru_cache(maxsize=None)
def _case(name):
    """(images, float32 table): computed once, shared, never modified."""
    if name == "centred_plus_constant":
        images = _bytes((13, 7, 9, 3), 71)
        mean, std = B.channel_moments(images)
        return images, B.colour_table(3, nu=1.0, mean=mean, std=std, constant_channel=1.0, dtype=torch.float32)
    if name == "one_window":
        images = _bytes((3, 5, 5, 1), 72)
        mean, std = B.channel_moments(images)
        return images, B.colour_table(1, nu=1.0, mean=mean, std=std, dtype=torch.float32)
    if name == "32x32":
        return _bytes((2, 32, 32, 3), 73), B.colour_table(3, nu=1.0, constant_channel=0.5, dtype=torch.float32)
    if name == "four_channels":
        images = _bytes((5, 7, 9, 4), 74)
        mean, std = B.channel_moments(images)
        return images, B.colour_table(4, nu=1.0, mean=mean, std=std, dtype=torch.float32)
    assert name == "grey"
    return _bytes((7, 12, 12), 75), B.feature_table(WS.φ_cos_sin_squared_1, 1.0, torch.float32).t().contiguous()


@functools.lru_cache(maxsize=None)
def _want(name, K):
    images, table = _case(name)
    x = _expand(table, images)
    total, sq = R.window_sums(x, K)
    return float(total), float(sq), _abs_first_terms(x, K), float(R.window_mean_var_factor(x, K)[2])


def _sums(images, table, K, **arena):
    """`window_sums_from_bytes` with its output and its workspace inside a guarded, poisoned (NaN) arena: the workspace is
    exactly the queried size."""
    with guarded(fill=0xFF, **arena) as a:
        got = WS.window_sums_from_bytes(images, table, K, DEV)
    assert dctn_amd.last_kernel() == "byte_window_stats"
    a.check()
    assert a.count["workspace"] == 1 and a.count["empty"] == 1
    return got.cpu()


CASES = [("centred_plus_constant", 2), ("centred_plus_constant", 3), ("centred_plus_constant", 4), ("one_window", 5),
         ("32x32", 3), ("four_channels", 3), ("grey", 3)]


@pytest.mark.parametrize("name,K", CASES, ids=[f"{n}_K{k}" for n, k in CASES])
def test_window_sums_meet_the_oracle_and_repeat_their_bits(name, K):
    """Centred data gives window terms of both signs, so the first sum is held to an ABSOLUTE bound from the oracle's
    per-window terms, 1e-12 * sum_w |prod t|; the second sum is all positive: rtol 1e-12 (test_gpu_parity.py's tolerance
    for `window_sums`); the factor rtol 1e-10."""
    images, table = _case(name)
    want_total, want_sq, abs_terms, want_factor = _want(name, K)
    got = _sums(images, table, K)
    print(f"{name} K={K}: first sum {float(got[0])!r} want {want_total!r} (|diff| {abs(float(got[0]) - want_total):.3e}, "
          f"bound {1e-12 * abs_terms:.3e}); second {float(got[1])!r} want {want_sq!r} "
          f"(rel {abs(float(got[1]) / want_sq - 1):.3e})")
    assert abs(float(got[0]) - want_total) <= 1e-12 * abs_terms
    assert abs(float(got[1]) - want_sq) <= 1e-12 * want_sq
    again = _sums(images.to(DEV), table, K)          # bytes already on the device; a second launch
    assert torch.equal(got.view(torch.uint8), again.view(torch.uint8))
    factor = WS.calc_scaling_factor_from_bytes(images, table, K, device=DEV)
    assert abs(factor / want_factor - 1.0) <= 1e-10, (factor, want_factor)


def test_window_sums_from_a_stale_workspace_of_another_size():
    """One never-refilled workspace buffer under two calls with different n: the second finds the first's slots and its
    used ticket where its own lie, and must neither read nor keep them."""
    images, table = _case("centred_plus_constant")
    pool = StalePool(fill=0xFF)
    first = _sums(images, table, 3, stale=pool)
    fewer = _sums(images[:5], table, 3, stale=pool)
    more = _sums(images, table, 3, stale=pool)
    assert torch.equal(first.view(torch.uint8), more.view(torch.uint8))
    x = _expand(table, images[:5])
    total, sq = R.window_sums(x, 3)
    assert abs(float(fewer[0]) - float(total)) <= 1e-12 * _abs_first_terms(x, 3)
    assert abs(float(fewer[1]) - float(sq)) <= 1e-12 * float(sq)
    assert torch.equal(fewer.view(torch.uint8), _sums(images[:5], table, 3).view(torch.uint8))


def test_samples_limits_the_images_that_count():
    images, table = _case("centred_plus_constant")
    x = _expand(table, images[:4])
    want = float(R.window_mean_var_factor(x, 3)[2])
    assert abs(WS.calc_scaling_factor_from_bytes(images, table, 3, samples=4, device=DEV) / want - 1.0) <= 1e-10


def test_an_image_beyond_the_lds_is_refused_by_name():
    images = torch.zeros(1, 100, 100, 3, dtype=torch.uint8)
    table = B.colour_table(3, nu=1.0, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="LDS"):
        WS.calc_scaling_factor_from_bytes(images, table, 3, device=DEV)


# ------------------------------------------------------------------ 3. end to end
def test_from_colour_centres_normalises_and_autoscales_from_the_bytes():
    images = _bytes((40, 8, 8, 3), 81)
    labels = torch.arange(40) % 10
    make = functools.partial(B.DeviceBatches.from_colour, labels=labels, batch_size=10, dtype=torch.float32, seed=5,
                             shuffle=False, device=DEV)
    src = make(images, center_and_normalize=True, constant_channel=1.0, autoscale_kernel_size=3, autoscale_samples=10)
    want_mean, want_std = B.channel_moments(images)
    assert torch.equal(src.mean, want_mean) and torch.equal(src.std, want_std)

    # the reference's pipeline (dataset_loading.py:349-375) restated in torch on the expanded tensor
    x = (images.float() / 255).unsqueeze(0)       # to_tensor: (1, 40, 8, 8, 3) float32
    x -= src.mean
    x /= src.std
    x = torch.cat((x, 1.0 * torch.ones_like(x[..., :1])), dim=4)
    want_nu = float(R.window_mean_var_factor(x[:, :10], 3)[2])
    assert isinstance(src.nu, float) and abs(src.nu / want_nu - 1.0) <= 1e-10, (src.nu, want_nu)
    x *= torch.tensor((src.nu,) * 4)

    idx = torch.arange(10, dtype=torch.int64, device=DEV)
    got, y, _ = src.gather(idx)
    assert got.shape == (1, 10, 8, 8, 4) and torch.equal(got.cpu(), x[:, :10]) and torch.equal(y.cpu(), labels[:10])
    m, v = WS.window_mean_var(got.double(), 3)
    assert abs(float(m**2 + v) - 1.0) < 1e-5, float(m**2 + v)

    assert set(src.colour_pipeline) == {"nu", "mean", "std", "constant_channel", "nu_constant"}
    twin = make(images, **src.colour_pipeline)    # how the validation and test sources are built
    assert torch.equal(twin.table.cpu(), src.table.cpu()) and twin.nu == src.nu
    again = make(images, center_and_normalize=True, constant_channel=1.0, autoscale_kernel_size=3, autoscale_samples=10)
    assert again.nu == src.nu and torch.equal(again.table.cpu(), src.table.cpu())


def test_grey_source_autoscales_from_the_bytes():
    images = _bytes((40, 12, 12), 82)
    labels = torch.arange(40) % 10
    src = B.DeviceBatches(images, labels, 10, dtype=torch.float32, seed=5, shuffle=False, device=DEV,
                          autoscale_kernel_size=3, autoscale_samples=10)
    want = WS.calc_scaling_factor(WS.apply_feature_map(images[:10].float() / 255), 3, DEV)
    assert abs(src.scale / want - 1.0) <= 1e-6, (src.scale, want)
    x, _, _ = src.gather(torch.arange(10, dtype=torch.int64, device=DEV))
    assert torch.equal(x.cpu(), B.feature_table(WS.φ_cos_sin_squared_1, src.scale, torch.float32)[images[:10].long()].unsqueeze(0))
    plain = B.DeviceBatches(images, labels, 10, dtype=torch.float32, seed=5, shuffle=False, device=DEV)
    assert plain.scale == 1.0
