"""Batches drawn on the device (dctn_amd/csrc/batch_source.hip, colour_source.hip): the input side of the reference's
``train(dl, ...)``.

The reference makes a batch with ``__getitem__`` per sample, ``collate_quantum``, pinning and a copy
(dctn/dataset_loading.py:69-70, 282-286, 319-325).  Here the whole data set lives on the device - the raw uint8
intensities, the raw interleaved colour bytes (`DeviceBatches.from_colour`), or an already-expanded feature tensor - and
ONE launch picks the samples of a batch, applies the feature map
and the scale (a 256-row table), casts to the model dtype and advances a device counter.  The epoch order is a pure
function of (seed, epoch, position) - a 6-round Feistel network with cycle walking, keyed by the Philox4x32-10 of
`dropout` - so nothing of the size of the data set is shuffled or stored, every rank that holds the same 16-byte block
draws its shard of the same global batch, a resumed run repeats its batches from ``{"seed", "batches_done"}``, and a
captured graph that holds the launch draws batch k, k + 1, ... on its replays.  include/dctn_amd.h holds the normative
definition; `round_keys`, `order_at` and `expected_indices` restate it in plain Python.

`Augment` adds a random shift (pad and crop) and a horizontal flip to the two byte-resident sources
(dctn_amd/csrc/augment_source.hip).  Both act on the bytes, inside the same one launch, and their parameters are a pure
function of (seed, epoch, global position) as the order is: no new state, the same batch on every sharding, the same
augmentations after a resume, other ones on every replay of a captured graph.  `augment_params`, `augment_bytes` and
`DeviceBatches.expected_augment` restate the definition of include/dctn_amd.h.

What the reference's loaders compute from the expanded training tensor before the first batch comes from the bytes too
(dctn_amd/csrc/byte_stats.hip): `byte_histogram` / `colour_moments` give the per-channel mean and std, and
``from_colour(center_and_normalize=, autoscale_kernel_size=)`` / ``DeviceBatches(autoscale_kernel_size=)`` put them and
`window_stats.calc_scaling_factor_from_bytes` together in the reference's order - exact or fixed-order sums, the same
table bits on every rank.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist
from torch import Tensor

from . import _lib as L
from .dropout import _MASK32, philox4x32_10
from .window_stats import calc_scaling_factor_from_bytes, φ_cos_sin_squared_1

TAG = 0x53485546   # counter word c3 of the round keys; dropout's c3 is a core number below 8
MAX_WIDTH = 4      # table columns / channels of one launch (include/dctn_amd.h)
AUG_TAG = 0x41554731            # counter word c3 of a slot's augmentation parameters (DCTN_AUG_TAG)
AUG_MAX_SHIFT = (1 << 15) - 1   # the largest max_shift
AUG_MAX_SAMPLE_BYTES = 13 * 1024   # an augmented launch keeps a sample's bytes (rounded up to 16) in a wave's LDS region


def round_keys(seed: int, epoch: int) -> Tuple[int, ...]:
    """The six 32-bit round keys of epoch ``epoch`` under the 64-bit ``seed``."""
    key = (seed & _MASK32, (seed >> 32) & _MASK32)
    return (philox4x32_10((0, 0, epoch, TAG), key) + philox4x32_10((1, 0, epoch, TAG), key))[:6]


def mix32(h: int) -> int:
    """murmur3's finaliser in 32-bit arithmetic."""
    h ^= h >> 16
    h = h * 0x85EBCA6B & _MASK32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & _MASK32
    return h ^ (h >> 16)


def perm_once(v: int, b: int, K: Sequence[int]) -> int:
    """One pass of the unbalanced Feistel network: a bijection on [0, 2**b)."""
    wl, wr = b // 2, b - b // 2
    left, right = v >> wr, v & ((1 << wr) - 1)
    for j in range(6):
        left, right = right, left ^ (mix32(right ^ K[j]) & ((1 << wl) - 1))
        wl, wr = wr, wl
    return (left << wr) | right


def _walk(v: int, n: int, b: int, K: Sequence[int]) -> int:
    while True:   # cycle walking: v < n lies on a cycle of the bijection, so the walk comes back below n
        v = perm_once(v, b, K)
        if v < n:
            return v


def order_at(seed: int, epoch: int, n: int, i: int) -> int:
    """The sample at position ``i`` of epoch ``epoch`` over ``n`` samples (1 <= n < 2**31)."""
    return _walk(i, n, max(2, (n - 1).bit_length()), round_keys(seed, epoch))


def order(seed: int, epoch: int, n: int) -> List[int]:
    """The whole epoch: a permutation of ``range(n)``."""
    b, K = max(2, (n - 1).bit_length()), round_keys(seed, epoch)
    return [_walk(i, n, b, K) for i in range(n)]


def steps_per_epoch(n: int, batch_size: int, drop_last: bool = True) -> int:
    """S: the batches of one pass.  ``batch_size`` is the GLOBAL batch."""
    if batch_size < 1 or n // batch_size < 1:
        raise ValueError(f"a global batch of {batch_size} needs 1 <= batch_size <= number of samples ({n})")
    return n // batch_size if drop_last else -(-n // batch_size)


def local_batch(batch_size: int, rank: int, world: int) -> int:
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of world {world}")
    if batch_size % world:
        raise ValueError(f"the global batch ({batch_size}) must be a multiple of the number of ranks ({world})")
    return batch_size // world


def expected_indices(seed: int, k: int, n: int, batch_size: int, rank: int = 0, world: int = 1,
                     shuffle: bool = True) -> List[int]:
    """The sample numbers of draw ``k`` (the device counter) for ``rank`` of ``world``: epoch ``k // S``, positions
    ``(k % S) * batch_size + rank * Bl + j`` for ``j < Bl = batch_size // world``."""
    S, Bl = steps_per_epoch(n, batch_size), local_batch(batch_size, rank, world)
    first = (k % S) * batch_size + rank * Bl
    if not shuffle:
        return list(range(first, first + Bl))
    b, K = max(2, (n - 1).bit_length()), round_keys(seed, k // S)
    return [_walk(first + j, n, b, K) for j in range(Bl)]


def expected_padded_indices(k: int, n: int, batch_size: int, rank: int = 0, world: int = 1) -> List[int]:
    """The sample numbers of draw ``k`` of the padded sequential form (`DeviceBatches.draw_padded_into`,
    DCTN_BATCH_PAD_TAIL) for ``rank`` of ``world``: S = ceil(n / batch_size) batches a pass, positions
    ``(k % S) * batch_size + rank * Bl + j`` for ``j < Bl = batch_size // world``, and -1 where the position is >= n
    (padding: the slot's label is -100)."""
    S, Bl = steps_per_epoch(n, batch_size, drop_last=False), local_batch(batch_size, rank, world)
    first = (k % S) * batch_size + rank * Bl
    return [pos if pos < n else -1 for pos in range(first, first + Bl)]


class Augment:
    """What an augmented source does to the bytes of every drawn sample, before the table lookup: a shift by
    (dy, dx), each uniform in [-max_shift, max_shift] (pad the image by ``max_shift`` with ``fill`` on every side and crop
    a window of the image's size: ``RandomCrop(padding=max_shift, fill)`` in distribution), then with ``hflip`` a
    horizontal flip with probability 1/2.  ``fill`` is a BYTE value, 0 .. 255, one for all source channels or one per
    channel: after per-channel centring, ``round(255 * mean_c)`` is about 0 in the model's units.  Validated here, without
    a device.  One ``max_shift`` serves both axes."""

    def __init__(self, max_shift: int = 0, hflip: bool = False, fill: Union[int, Sequence[int]] = 0):
        if isinstance(max_shift, bool) or not isinstance(max_shift, int) or not 0 <= max_shift <= AUG_MAX_SHIFT:
            raise ValueError(f"max_shift is an integer in [0, {AUG_MAX_SHIFT}], got {max_shift!r}")
        if not isinstance(hflip, bool):
            raise ValueError(f"hflip is a bool, got {hflip!r}")
        values = tuple(fill) if isinstance(fill, (tuple, list)) else (fill,)
        if not 1 <= len(values) <= MAX_WIDTH or any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255
                                                    for v in values):
            raise ValueError(f"fill is one byte value (0 .. 255) or one per source channel (at most {MAX_WIDTH}), got {fill!r}")
        self.max_shift, self.hflip = max_shift, hflip
        self.fill = values if isinstance(fill, (tuple, list)) else values[0]

    @property
    def flags(self) -> int:
        return L.AUG_HFLIP if self.hflip else 0

    def fill_bytes(self, channels: int) -> Tuple[int, ...]:
        """One fill byte per source channel."""
        if isinstance(self.fill, int):
            return (self.fill,) * channels
        if len(self.fill) != channels:
            raise ValueError(f"fill needs one byte per source channel ({channels}), got {len(self.fill)}")
        return self.fill

    def packed_fill(self, channels: int) -> int:
        """The 32-bit `fill` argument: channel c in bits 8 c .. 8 c + 7."""
        return sum(v << (8 * c) for c, v in enumerate(self.fill_bytes(channels)))

    def __repr__(self) -> str:
        return f"Augment(max_shift={self.max_shift}, hflip={self.hflip}, fill={self.fill})"


def augment_params(seed: int, epoch: int, position: int, max_shift: int, hflip: bool) -> Tuple[int, int, int]:
    """``(dy, dx, flip)`` of the slot at GLOBAL position ``position`` of epoch ``epoch``: the words of
    Philox4x32-10(counter (position, 0, epoch, AUG_TAG), key (seed_lo, seed_hi)), the first two mapped onto
    [-max_shift, max_shift] by multiply-high, the top bit of the third the flip."""
    w = philox4x32_10((position, 0, epoch, AUG_TAG), (seed & _MASK32, (seed >> 32) & _MASK32))
    span = 2 * max_shift + 1
    return ((w[0] * span >> 32) - max_shift, (w[1] * span >> 32) - max_shift, w[2] >> 31 if hflip else 0)


def augment_bytes(images_u8: Tensor, params: Sequence[Tuple[int, int, int]], fill=0) -> Tensor:
    """The augmentation on CPU bytes: ``images_u8`` (count, H, Wd) or (count, H, Wd, C) uint8, one ``(dy, dx, flip)`` per
    image, ``fill`` one byte value or one per channel.  ``out[i, h, w] = images_u8[i, h + dy, wf + dx]`` with
    ``wf = Wd - 1 - w`` when flipped, else ``w``, where that lies inside the image, and the fill elsewhere."""
    if images_u8.dtype != torch.uint8 or images_u8.ndim not in (3, 4) or len(params) != images_u8.shape[0]:
        raise ValueError("augment_bytes takes (count, H, Wd[, C]) uint8 images and one (dy, dx, flip) per image")
    H, Wd = images_u8.shape[1], images_u8.shape[2]
    channels = 1 if images_u8.ndim == 3 else images_u8.shape[3]
    fills = torch.tensor(Augment(fill=fill).fill_bytes(channels), dtype=torch.uint8)
    out = (fills[0] if images_u8.ndim == 3 else fills).expand(images_u8.shape).clone()
    for i, (dy, dx, flip) in enumerate(params):
        h0, h1, w0, w1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(Wd, Wd - dx)   # where the source covers the window
        if h0 < h1 and w0 < w1:
            out[i, h0:h1, w0:w1] = images_u8[i, h0 + dy : h1 + dy, w0 + dx : w1 + dx]
        if flip:
            out[i] = out[i].flip(1)
    return out


def _new_state(seed: int, device: torch.device, batches_done: int = 0) -> Tensor:
    """The 16-byte device block {uint32 seed_lo, seed_hi, batches_done, ticket} as four int32 (same bits)."""
    assert L.lib().dctn_batch_state_bytes() == 16
    return torch.tensor(_state_words(seed, batches_done), dtype=torch.int32).to(device)


def _state_words(seed: int, batches_done: int) -> List[int]:
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"the batch seed is a 64-bit unsigned integer, got {seed}")
    if not 0 <= int(batches_done) < 1 << 32:
        raise ValueError(f"batches_done is a 32-bit unsigned integer, got {batches_done}")
    words = [int(seed) & _MASK32, int(seed) >> 32, int(batches_done), 0]
    return [w - (1 << 32) if w >= 1 << 31 else w for w in words]


def feature_table(phi: Sequence[Callable[[Tensor], Tensor]], scale: float, dtype: torch.dtype) -> Tensor:
    """(256, len(phi)): what the reference's float32 ops (dataset_loading.py:60-63 and the runner's ``x *= scale``) give for
    each of the 256 intensities, cast to ``dtype``.  Built on the CPU."""
    u = torch.arange(256, dtype=torch.uint8).float() / 255.0
    return (scale * torch.stack(tuple(f(u) for f in phi), dim=1)).to(dtype).contiguous()


def _per_channel(value, channels: int, what: str) -> Tuple[float, ...]:
    out = (float(value),) * channels if isinstance(value, (int, float)) else tuple(float(v) for v in value)
    if len(out) != channels:
        raise ValueError(f"{what} needs one value per channel ({channels}), got {len(out)}")
    return out


def colour_table(channels: int, *, nu, mean: Optional[Tensor] = None, std: Optional[Tensor] = None,
                 constant_channel: Optional[float] = None, dtype: torch.dtype, nu_constant: float = 1.0) -> Tensor:
    """(W, 256), W = ``channels`` (+ 1 with a constant channel): row c holds what the reference's colour pipeline
    (dataset_loading.py:349-375) gives for each of the 256 byte values in channel c, cast to ``dtype``.  Every value of
    that pipeline is a function of one byte and its channel, so the table IS the pipeline: it is built on the CPU with
    the reference's own ops in the reference's order on a (256, channels) float32 tensor -
    ``arange(256, uint8).float().div(255)`` (``to_tensor``), in-place ``-= mean`` and ``/= std`` with float64 (channels,)
    tensors when given (both or neither), the concatenated column ``constant_channel * ones``, in-place
    ``*= torch.tensor(nu)`` where ``nu`` gets ``(nu_constant,)`` appended when a constant channel is added - and indexing it
    with the bytes gives the bits of the expanded tensor.  ``nu``: one value per channel, or one number for all of them.
    ``nu_constant``: the factor of the constant column, 1.0 for a given ``nu`` (dataset_loading.py:369) and the one factor of
    all columns under autoscale (:372).  Row ``channels`` (the constant channel) holds one value 256 times."""
    channels = int(channels)
    width = channels + (constant_channel is not None)
    if not 1 <= channels <= MAX_WIDTH or width > MAX_WIDTH:
        raise NotImplementedError(f"one launch writes 1 .. {MAX_WIDTH} columns, got {channels} channels"
                                  + (" and a constant one" if constant_channel is not None else ""))
    if (mean is None) != (std is None):
        raise ValueError("centring and scaling go together: give both mean and std, or neither")
    L.dtype_code(torch.empty(0, dtype=dtype))
    nu = _per_channel(nu, channels, "nu")
    t = torch.arange(256, dtype=torch.uint8).float().div(255).unsqueeze(1).repeat(1, channels)
    if mean is not None:
        mean, std = (torch.as_tensor(v, dtype=torch.float64).cpu().reshape(-1) for v in (mean, std))
        if mean.shape != (channels,) or std.shape != (channels,):
            raise ValueError(f"mean and std need one value per channel ({channels})")
        t -= mean
        t /= std
    if constant_channel is not None:
        t = torch.cat((t, constant_channel * torch.ones_like(t[:, :1])), dim=1)
        nu = nu + (float(nu_constant),)
    t *= torch.tensor(nu)
    return t.to(dtype).t().contiguous()


def channel_moments(images_u8: Tensor) -> Tuple[Tensor, Tensor]:
    """``(mean, std)`` of ``images_u8 / 255`` per channel (the last dimension), float64 (channels,) on the input's device,
    population std: what dataset_loading.py:351-352 computes from the expanded training tensor, here from a 256-bin
    histogram of each channel, so nothing of the data set's size is expanded.  It agrees with
    ``x.double().mean(...)`` / ``x.double().std(..., unbiased=False)`` to rounding (a few float64 ulps), NOT bit for bit: for
    bit parity with a given reference run pass that run's own logged mean and std to `colour_table` / ``from_colour``."""
    if images_u8.dtype != torch.uint8 or images_u8.ndim < 2:
        raise TypeError(f"channel_moments takes (..., channels) uint8 bytes, got {images_u8.dtype}, {tuple(images_u8.shape)}")
    C = images_u8.shape[-1]
    flat = images_u8.reshape(-1, C)
    if flat.shape[0] < 1:
        raise ValueError("channel_moments needs at least one pixel")
    return moments_from_counts(torch.stack([torch.bincount(flat[:, c].int(), minlength=256) for c in range(C)]))


def moments_from_counts(counts: Tensor) -> Tuple[Tensor, Tensor]:
    """``(mean, std)`` float64 (channels,) from the (channels, 256) histogram of the bytes: `channel_moments` from its
    counts onward.  The sums run where ``counts`` lives; `colour_moments` hands it counts on the CPU, so its numbers are
    those of ``channel_moments(bytes.cpu())`` on every device and rank."""
    if counts.ndim != 2 or counts.shape[1] != 256 or counts.dtype.is_floating_point:
        raise TypeError(f"moments_from_counts takes (channels, 256) integer counts, got {counts.dtype}, {tuple(counts.shape)}")
    total = float(counts[0].sum())   # every channel counts every pixel once
    if total < 1:
        raise ValueError("moments_from_counts needs at least one pixel")
    counts = counts.double()   # (C, 256)
    values = torch.arange(256, dtype=torch.uint8).float().div(255).double().to(counts.device)   # to_tensor's float32 values
    mean = (counts * values).sum(dim=1) / total
    var = (counts * (values.unsqueeze(0) - mean.unsqueeze(1)) ** 2).sum(dim=1) / total
    return mean, var.sqrt()


def _source_device(device, tensor: Tensor) -> torch.device:
    """Where a byte-resident source lives: ``device``, else the tensor's GPU, else the current one.  No GPU: RuntimeError."""
    if not torch.cuda.is_available():
        raise RuntimeError("dctn_amd: a DeviceBatches source lives on an MI355X device, but no GPU is visible. "
                           "There is deliberately no CPU implementation of this path.")
    if device is not None:
        return torch.device(device)
    return tensor.device if tensor.is_cuda else torch.device("cuda", torch.cuda.current_device())


def byte_histogram(images_u8: Tensor, device=None) -> Tensor:
    """(channels, 256) int64 on the device: how often each byte value occurs in each channel (the last dimension, at most
    4) of ``images_u8`` (..., channels) uint8 - one launch over the bytes (`dctn_byte_histogram`), exact.  CPU bytes are
    moved to the device first; bytes already there are read in place."""
    if images_u8.dtype != torch.uint8 or images_u8.ndim < 2:
        raise TypeError(f"byte_histogram takes (..., channels) uint8 bytes, got {images_u8.dtype}, {tuple(images_u8.shape)}")
    C = images_u8.shape[-1]
    if not 1 <= C <= MAX_WIDTH:
        raise NotImplementedError(f"one launch counts 1 .. {MAX_WIDTH} channels, got {C}")
    if images_u8.numel() < 1:
        raise ValueError("byte_histogram needs at least one pixel")
    dev = _source_device(device, images_u8)
    src = images_u8.to(dev).contiguous()
    counts = torch.empty((C, 256), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().dctn_byte_histogram(src.data_ptr(), src.numel() // C, C, counts.data_ptr(), L.stream_ptr(dev)),
                "byte histogram")
    return counts


def colour_moments(images_u8: Tensor, device=None) -> Tuple[Tensor, Tensor]:
    """`channel_moments` of bytes that live on the device, without the 4-byte copy of every channel that ``bincount`` needs:
    the histogram kernel, a copy of channels x 256 integers to the host, `moments_from_counts` there.  Returns CPU float64
    tensors that equal ``channel_moments(images_u8.cpu())`` bit for bit - integer counts have no summation order - and so
    are the same on every rank."""
    return moments_from_counts(byte_histogram(images_u8, device).cpu())


def _check_autoscale(kernel_size, samples, H: int, Wd: int) -> None:
    """The errors of ``autoscale_kernel_size`` / ``autoscale_samples``, without a device."""
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise ValueError(f"autoscale_samples is a positive integer, got {samples!r}")
    if kernel_size is None:
        return
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, int) or not 1 <= kernel_size <= min(H, Wd):
        raise ValueError(f"autoscale_kernel_size is an integer in [1, {min(H, Wd)}] for {H} x {Wd} images, got {kernel_size!r}")


class DeviceBatches:
    """``(x, y, indices)`` batches of a data set that lives on the device, in place of the reference's train ``DataLoader``.

    ``images_u8``: (n, height, width) uint8 intensities (what ``torchvision_dataset.data`` holds); ``labels``: n integers.
    ``batch_size`` is the GLOBAL batch; ``rank`` of ``world`` takes its ``batch_size // world`` samples of it (they default
    to ``torch.distributed``'s when a process group is up, else 0 / 1; when they default, rank 0's 16-byte block is
    broadcast, so every rank draws the same global batch whatever seed it was given).  ``x`` comes out as
    (1, Bl, height, width, len(phi)) in ``dtype``: ``scale * phi(intensity / 255)`` evaluated with the reference's own
    float32 ops once per intensity (`feature_table`), then cast.  `from_colour` takes raw (n, height, width, channels)
    colour bytes and one 256-row table per channel (`colour_table`); `from_features` takes a tensor that is already expanded.
    CPU inputs are moved to the device once, here; without a GPU the constructor raises.
    ``autoscale_kernel_size=K`` (instead of a ``scale``) is the reference's ``get_data_loaders(..., autoscale_kernel_size)``:
    the scale is `calc_scaling_factor_from_bytes` of the first ``autoscale_samples`` images, computed from the bytes on the
    device, the same float on every rank; ``src.scale`` holds it.

    ``draw_into(x, y, indices)`` enqueues one launch into caller-owned buffers and never reads the device: it can be
    captured, and the replays draw the following batches (``GraphedTrainStep(batch_source=...)`` does so).  ``draw()``
    returns fresh tensors.  Iterating yields ``len(self)`` batches, so ``training.train(dl=src, ...)``,
    ``batches_forever`` and ``evaluation.score_fused`` work unchanged.  One difference from a ``DataLoader``: a pass that
    is abandoned early does not reshuffle - the next pass continues from the device counter.

    ``shuffle=False`` gives the identity order.  ``drop_last=False`` (with ``shuffle=False`` only: the form of the
    reference's validation and test loaders) makes every pass a sequential walk over ALL samples through
    `dctn_batch_gather`, the last batch short; such a pass is eager and does not touch the counter.

    ``draw_padded_into(x, y, indices)`` (``shuffle=False`` sources) is the capturable form of that walk: every batch has
    the full shape, ``padded_steps`` = ceil(n / batch_size) draws cover all samples once, and the slots past the last sample
    are padding (label -100, index -1; `expected_padded_indices`).  It reads the SAME counter word as ``draw_into`` with a
    different number of batches per pass, so a source used for padded passes is used for nothing else.  Its sharding differs
    from the eager ``drop_last=False`` iteration: rank r takes slots ``r * Bl .. r * Bl + Bl - 1`` of every batch (of the
    last one too, where a rank may get nothing but padding), whereas the eager iteration splits the short tail evenly; the
    sums over all ranks are the same.

    ``augment=Augment(...)`` (the uint8 and the colour sources; not `from_features`, whose rows have no height or width)
    makes ``draw_into`` / ``draw`` - and with them ``GraphedTrainStep(batch_source=...)``, ``train(dl=...)`` and
    ``batches_forever`` - shift and flip every sample's bytes inside the same launch (`augment_params`,
    `expected_augment`, `augment_bytes`).  ``gather`` stays unaugmented, ``draw_padded_into`` raises and
    ``drop_last=False`` is refused: evaluation is not augmented.  It takes a second source over the same bytes with
    ``augment=None``: a constructor does not copy a tensor that is already on the device, so building both from one
    device tensor (``train_src.src``, ``train_src.labels``) shares the data set.  ``state_dict`` is unchanged, and a loaded
    state repeats the augmentations with the batches.
    """

    def __init__(self, images_u8: Tensor, labels: Tensor, batch_size: int, *, dtype: torch.dtype, seed: int,
                 scale: float = 1.0, phi: Sequence[Callable[[Tensor], Tensor]] = φ_cos_sin_squared_1,
                 shuffle: bool = True, drop_last: bool = True, rank: Optional[int] = None,
                 world: Optional[int] = None, device=None, augment: Optional[Augment] = None,
                 autoscale_kernel_size: Optional[int] = None, autoscale_samples: int = 10880):
        if images_u8.dtype != torch.uint8 or images_u8.ndim != 3:
            raise TypeError("DeviceBatches takes (samples, height, width) uint8 intensities; float-valued sources go "
                            f"through DeviceBatches.from_features (got {images_u8.dtype}, {tuple(images_u8.shape)})")
        if not 1 <= len(phi) <= MAX_WIDTH:
            raise NotImplementedError(f"the table of one launch has 1 .. {MAX_WIDTH} columns, phi has {len(phi)}")
        L.dtype_code(torch.empty(0, dtype=dtype))
        n, H, W = images_u8.shape
        if autoscale_kernel_size is not None and scale != 1.0:
            raise ValueError("autoscale_kernel_size computes the scale: give one of the two, not both")
        _check_autoscale(autoscale_kernel_size, autoscale_samples, H, W)
        self._plan(n, labels, batch_size, seed, shuffle, drop_last, rank, world)
        self._plan_augment(augment, H, W, 1)
        dev = self._device(device, images_u8)
        self.kind, self.dtype = L.BATCH_SRC_U8_TABLE, dtype
        self.src = images_u8.to(dev).contiguous()
        if autoscale_kernel_size is not None:   # get_data_loaders(..., autoscale_kernel_size): the factor of phi's float32 values
            scale = calc_scaling_factor_from_bytes(self.src, feature_table(phi, 1.0, torch.float32).t().contiguous(),
                                                   autoscale_kernel_size, samples=autoscale_samples, device=dev)
        self.scale = float(scale)
        self.table = feature_table(phi, scale, dtype).to(dev)
        self.row_len, self.width = H * W, len(phi)
        self.x_shape = lambda count: (1, count, H, W, len(phi))
        self._finish(labels, dev)

    @classmethod
    def from_features(cls, x_full: Tensor, labels: Tensor, batch_size: int, *, seed: int, shuffle: bool = True,
                      drop_last: bool = True, rank: Optional[int] = None,
                      world: Optional[int] = None) -> "DeviceBatches":
        """A source over features that are already expanded: ``x_full`` (channels, samples, ...) in the model dtype,
        channels <= 4 (whatever no 256-row table per channel holds: augmented or otherwise pre-computed features; raw
        colour bytes go through `from_colour`).  ``x`` comes out as (channels, Bl, ...): a row copy."""
        self = cls.__new__(cls)
        if x_full.ndim < 2:
            raise TypeError(f"from_features takes (channels, samples, ...) features, got {tuple(x_full.shape)}")
        if not 1 <= x_full.shape[0] <= MAX_WIDTH:
            raise NotImplementedError(f"one launch moves 1 .. {MAX_WIDTH} channels, got {x_full.shape[0]}")
        L.dtype_code(x_full)
        C, n, rest = x_full.shape[0], x_full.shape[1], tuple(x_full.shape[2:])
        self._plan(n, labels, batch_size, seed, shuffle, drop_last, rank, world)
        self._plan_augment(None, 0, 0, 1)   # rows have no height, width or source channels
        dev = self._device(None, x_full)
        self.kind, self.dtype = L.BATCH_SRC_ROWS, x_full.dtype
        self.src = x_full.to(dev).contiguous()
        self.table = None
        self.row_len, self.width = max(1, x_full[0, 0].numel()), C
        self.x_shape = lambda count: (C, count) + rest
        self._finish(labels, dev)
        return self

    @classmethod
    def from_colour(cls, images_u8: Tensor, labels: Tensor, batch_size: int, *, dtype: torch.dtype, seed: int, nu=None,
                    mean: Optional[Tensor] = None, std: Optional[Tensor] = None,
                    constant_channel: Optional[float] = None, shuffle: bool = True, drop_last: bool = True,
                    rank: Optional[int] = None, world: Optional[int] = None, device=None,
                    augment: Optional[Augment] = None, center_and_normalize: bool = False,
                    autoscale_kernel_size: Optional[int] = None, autoscale_samples: int = 10880,
                    nu_constant: float = 1.0) -> "DeviceBatches":
        """A source over raw colour images: ``images_u8`` (n, height, width, channels) uint8 with the channels interleaved
        (what ``torchvision.datasets.CIFAR10.data`` holds; for YCbCr the caller converts the bytes on the host first),
        channels <= 4.  ``x`` comes out as (1, Bl, height, width, Wout), Wout = channels (+ 1 with ``constant_channel``):
        the reference's colour pipeline (dataset_loading.py:331-389 - ``to_tensor``, the per-channel ``mean`` / ``std``,
        the constant channel, the per-channel ``nu``) evaluated once per byte value and channel (`colour_table`), then
        cast.  `channel_moments` gives ``mean`` and ``std`` of a training split from its bytes.  The data set stays on the
        device as its bytes: 45 000 x 32 x 32 x 3 is 138 MB, against 737 MB expanded to float32 with a constant channel.

        The loader's two remaining arguments work from the bytes as well, in the reference's order (:349-375).
        ``center_and_normalize=True`` (instead of ``mean`` / ``std``) takes the moments of THESE bytes (`colour_moments`: the
        histogram kernel).  ``autoscale_kernel_size=K`` (instead of ``nu``: exactly one of the two) then builds the nu = 1
        table with the constant channel, takes `calc_scaling_factor_from_bytes` of the first ``autoscale_samples`` images
        and puts that factor on EVERY column, the constant one included (:372).  Both are exact or fixed-order sums, so
        every rank that holds the same bytes builds the same table bits.  The source carries ``mean``, ``std`` (CPU float64,
        or None), ``nu`` and ``colour_pipeline`` - a dict of ``nu``, ``mean``, ``std``, ``constant_channel`` and
        ``nu_constant`` - so that the validation and test sources are ``from_colour(val_bytes, ..., **train.colour_pipeline)``:
        the reference applies the training split's numbers to all three splits."""
        self = cls.__new__(cls)
        if images_u8.dtype != torch.uint8 or images_u8.ndim != 4:
            raise TypeError("from_colour takes (samples, height, width, channels) uint8 bytes; float-valued sources go "
                            f"through DeviceBatches.from_features (got {images_u8.dtype}, {tuple(images_u8.shape)})")
        n, H, W, C = images_u8.shape
        if (nu is None) == (autoscale_kernel_size is None):
            raise ValueError("give exactly one of nu and autoscale_kernel_size")
        if center_and_normalize and (mean is not None or std is not None):
            raise ValueError("center_and_normalize=True takes the moments of these bytes: it excludes mean and std")
        if autoscale_kernel_size is not None and nu_constant != 1.0:
            raise ValueError("autoscale_kernel_size puts its factor on every column: it excludes nu_constant")
        _check_autoscale(autoscale_kernel_size, autoscale_samples, H, W)
        pipeline = dict(mean=mean, std=std, constant_channel=constant_channel)
        # the table's own errors (channels, width, dtype, the lengths of nu, mean and std) before a device is needed
        table = colour_table(C, nu=1.0 if nu is None else nu, dtype=dtype, nu_constant=nu_constant, **pipeline)
        Wout = table.shape[0]
        self._plan(n, labels, batch_size, seed, shuffle, drop_last, rank, world)
        self._plan_augment(augment, H, W, C)
        dev = self._device(device, images_u8)
        self.kind, self.dtype = L.BATCH_SRC_COLOUR, dtype
        self.src = images_u8.to(dev).contiguous()
        if center_and_normalize:
            pipeline["mean"], pipeline["std"] = colour_moments(self.src, dev)
        if autoscale_kernel_size is not None:
            unit = colour_table(C, nu=1.0, dtype=torch.float32, **pipeline)
            nu = nu_constant = calc_scaling_factor_from_bytes(self.src, unit, autoscale_kernel_size,
                                                              samples=autoscale_samples, device=dev)
        if center_and_normalize or autoscale_kernel_size is not None:
            table = colour_table(C, nu=nu, dtype=dtype, nu_constant=nu_constant, **pipeline)
        self.mean, self.std, self.nu = pipeline["mean"], pipeline["std"], nu
        self.colour_pipeline = dict(pipeline, nu=nu, nu_constant=nu_constant)
        self.table = table.to(dev)
        self.row_len, self.width = H * W, Wout
        self.x_shape = lambda count: (1, count, H, W, Wout)
        self._finish(labels, dev)
        return self

    # ---------------------------------------------------------------------------------------------- construction
    def _plan(self, n, labels, batch_size, seed, shuffle, drop_last, rank, world) -> None:
        """Everything that needs no device, first: the arithmetic errors are ValueErrors with or without a GPU."""
        if not 1 <= n < 1 << 31:
            raise ValueError(f"1 <= number of samples < 2^31, got {n}")
        if labels.shape != (n,):
            raise ValueError(f"{n} samples need labels of shape ({n},), got {tuple(labels.shape)}")
        self.defaulted = rank is None and world is None
        if self.defaulted and dist.is_available() and dist.is_initialized():
            rank, world = dist.get_rank(), dist.get_world_size()
        self.rank, self.world = (0 if rank is None else int(rank)), (1 if world is None else int(world))
        self.n, self.batch_size, self.seed = int(n), int(batch_size), int(seed)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        if shuffle and not drop_last:
            raise ValueError("drop_last=False is the sequential form: it needs shuffle=False")
        self.steps = steps_per_epoch(self.n, self.batch_size)             # S of the device counter: whole batches
        self.padded_steps = steps_per_epoch(self.n, self.batch_size, drop_last=False)   # S of `draw_padded_into`
        self.local_batch = local_batch(self.batch_size, self.rank, self.world)
        _state_words(self.seed, 0)

    def _plan_augment(self, augment: Optional[Augment], H: int, Wd: int, channels: int) -> None:
        """The augmentation's own errors, before the device as well; `_plan` has run."""
        self.augment, self.height, self.width_px, self.channels, self._fill = augment, int(H), int(Wd), int(channels), 0
        if augment is None:
            return
        if not isinstance(augment, Augment):
            raise TypeError(f"augment takes an Augment, got {type(augment).__name__}")
        if not self.drop_last:
            raise ValueError("drop_last=False is the evaluation form, which is not augmented: build that source with augment=None")
        self._fill = augment.packed_fill(channels)
        if -(-H * Wd * channels // 16) * 16 > AUG_MAX_SAMPLE_BYTES:
            raise NotImplementedError(f"an augmented draw keeps a sample's bytes in LDS: at most {AUG_MAX_SAMPLE_BYTES} "
                                      f"bytes, got {H} x {Wd} x {channels}")

    @staticmethod
    def _device(device, tensor: Tensor) -> torch.device:
        return _source_device(device, tensor)

    def _finish(self, labels: Tensor, dev: torch.device) -> None:
        self.device = dev
        self.labels = labels.to(dev, torch.int64).contiguous()
        self._state = _new_state(self.seed, dev)
        if self.defaulted and self.world > 1:   # every rank draws from rank 0's block
            dist.broadcast(self._state, src=0)
            self.seed = self.state_dict()["seed"]
        self._all = None   # arange(n) for the sequential passes, made on first use
        # The one description of this source's launches (dctn_batch_call_t): everything that is stable for the source's
        # life, written once.  `_draw` and `gather` write the outputs and what the two operations do not share.
        assert L.lib().dctn_batch_call_bytes() == ctypes.sizeof(L.BatchCall)
        aug = self.augment
        self._call = L.BatchCall(
            src=self.src.data_ptr(), table=None if self.table is None else self.table.data_ptr(),
            labels=self.labels.data_ptr(), state=self._state.data_ptr(), n=self.n, global_batch=self.batch_size,
            count=self.local_batch, rank_offset=self.rank * self.local_batch, row_len=self.row_len, height=self.height,
            width_px=self.width_px, src_kind=self.kind, src_channels=self.channels, width=self.width,
            dtype=L.dtype_code(torch.empty(0, dtype=self.dtype)), augment=aug is not None,
            max_shift=0 if aug is None else aug.max_shift, aug_flags=0 if aug is None else aug.flags, fill=self._fill)
        self._call_ref = ctypes.byref(self._call)
        colour = "colour " if self.kind == L.BATCH_SRC_COLOUR else ""
        self._what = {"draw": ("augmented " if aug is not None else "") + colour + "batch draw",
                      "gather": colour + "batch gather"}

    # ---------------------------------------------------------------------------------------------- batches
    def __len__(self) -> int:
        return steps_per_epoch(self.n, self.batch_size, self.drop_last)

    def empty_batch(self, count: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """Uninitialised ``(x, y, indices)`` of this rank's batch shape (static buffers for a capture)."""
        count = self.local_batch if count is None else count
        return (torch.empty(self.x_shape(count), dtype=self.dtype, device=self.device),
                torch.empty(count, dtype=torch.int64, device=self.device),
                torch.empty(count, dtype=torch.int64, device=self.device))

    def _check_out(self, x: Tensor, y: Tensor, indices: Tensor, count: int) -> None:
        L.require_device(x, y, indices, self.src)
        if (tuple(x.shape) != self.x_shape(count) or x.dtype != self.dtype or y.shape != (count,)
                or indices.shape != (count,) or y.dtype != torch.int64 or indices.dtype != torch.int64
                or not (x.is_contiguous() and y.is_contiguous() and indices.is_contiguous())):
            raise ValueError(f"a batch of {count} samples needs contiguous x {self.x_shape(count)} in {self.dtype} and "
                             f"int64 y, indices of shape ({count},)")

    def _draw(self, x: Tensor, y: Tensor, indices: Tensor, flags: int) -> None:
        self._check_out(x, y, indices, self.local_batch)
        c = self._call
        c.x, c.y, c.indices, c.flags = x.data_ptr(), y.data_ptr(), indices.data_ptr(), flags
        c.count, c.augment = self.local_batch, self.augment is not None   # (a gather leaves its own there)
        with torch.cuda.device(self.device):
            L.check(L.lib().dctn_batch_draw_call(self._call_ref, L.stream_ptr(self.device)), self._what["draw"])

    def draw_into(self, x: Tensor, y: Tensor, indices: Tensor) -> None:
        """The next batch (this rank's shard of it) into caller-owned buffers: one launch, capturable.  With ``augment``
        the launch shifts and flips the samples' bytes (`expected_augment`)."""
        self._draw(x, y, indices, 0 if self.shuffle else L.BATCH_IDENTITY_ORDER)

    def draw_padded_into(self, x: Tensor, y: Tensor, indices: Tensor) -> None:
        """The next batch of the padded sequential walk (this rank's shard of it): one launch, capturable, never reads the
        device.  ``padded_steps`` draws from a counter at 0 (mod ``padded_steps``) cover every sample once and leave the
        counter there again; padding slots carry the label -100 and the index -1 (see the class docstring: the source is
        then used for nothing else)."""
        if self.shuffle:
            raise ValueError("the padded pass is sequential: it needs a source built with shuffle=False")
        if self.augment is not None:
            raise ValueError("the padded pass is an evaluation pass, which is not augmented: use a source with augment=None")
        self._draw(x, y, indices, L.BATCH_IDENTITY_ORDER | L.BATCH_PAD_TAIL)

    def draw(self) -> Tuple[Tensor, Tensor, Tensor]:
        out = self.empty_batch()
        self.draw_into(*out)
        return out

    def gather(self, sample_idx: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        """The batch made of the given samples (a device int64 vector, every entry in [0, n): not checked).  Reads no
        state.  Never augmented."""
        L.require_device(sample_idx, self.src)
        if sample_idx.dtype != torch.int64 or sample_idx.ndim != 1 or sample_idx.numel() < 1:
            raise ValueError("gather takes a non-empty int64 vector of sample numbers")
        idx = sample_idx.contiguous()
        x, y, indices = self.empty_batch(idx.numel())
        c = self._call
        c.x, c.y, c.indices = x.data_ptr(), y.data_ptr(), indices.data_ptr()
        c.sample_idx, c.count, c.augment = idx.data_ptr(), idx.numel(), 0
        with torch.cuda.device(self.device):
            L.check(L.lib().dctn_batch_gather_call(self._call_ref, L.stream_ptr(self.device)), self._what["gather"])
        return x, y, indices

    def __iter__(self) -> Iterator[Tuple[Tensor, Tensor, Tensor]]:
        if self.drop_last:
            for _ in range(len(self)):
                yield self.draw()
            return
        if self._all is None:
            self._all = torch.arange(self.n, dtype=torch.int64, device=self.device)
        for step in range(len(self)):   # sequential: this rank's slice of every batch, the last one short
            first, count = step * self.batch_size, min(self.batch_size, self.n - step * self.batch_size)
            lo, hi = first + count * self.rank // self.world, first + count * (self.rank + 1) // self.world
            if hi > lo:
                yield self.gather(self._all[lo:hi])

    def expected_padded_indices(self, k: int) -> List[int]:
        """Host restatement: what draw ``k`` of the padded walk gives this rank (-1: padding)."""
        return expected_padded_indices(k, self.n, self.batch_size, self.rank, self.world)

    def expected_indices(self, k: int) -> List[int]:
        """Host restatement: the sample numbers draw ``k`` gives this rank."""
        return expected_indices(self.seed, k, self.n, self.batch_size, self.rank, self.world, self.shuffle)

    def expected_augment(self, k: int) -> List[Tuple[int, int, int]]:
        """Host restatement: ``(dy, dx, flip)`` of this rank's slots of draw ``k`` (all (0, 0, 0) without ``augment``)."""
        if self.augment is None:
            return [(0, 0, 0)] * self.local_batch
        first = (k % self.steps) * self.batch_size + self.rank * self.local_batch
        return [augment_params(self.seed, k // self.steps, first + j, self.augment.max_shift, self.augment.hflip)
                for j in range(self.local_batch)]

    # ---------------------------------------------------------------------------------------------- resume
    def state_dict(self) -> Dict[str, int]:
        """``{"seed", "batches_done"}`` (reads the device: it synchronises).  Save it beside the optimizer's and the
        dropout's; a source built from the same data and arguments that loads it repeats the batches from there."""
        w = [int(v) & _MASK32 for v in self._state.cpu().tolist()]
        return {"seed": w[0] | (w[1] << 32), "batches_done": w[2]}

    def load_state_dict(self, state: Dict[str, int]) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceBatches.load_state_dict writes the device block from the host: not during a capture")
        words = _state_words(state["seed"], state["batches_done"])
        self._state.copy_(torch.tensor(words, dtype=torch.int32))   # in place: a captured graph keeps its pointer
        self.seed = int(state["seed"])

    # A part of a run (`checkpoint.RunState`): the device tensors that travel, the host scalars
    # beside them, what of those a run refuses before anything is written, and how the host mirrors follow.
    def run_regions(self):
        return [("state", self._state)]

    def run_host(self) -> Dict[str, int]:
        return dict(n=self.n, batch_size=self.batch_size, seed=self.seed)

    def run_check(self, host: Dict[str, int]) -> None:
        for key in ("n", "batch_size"):
            if host[key] != getattr(self, key):
                raise ValueError(f"snapshot: entry 'batch_source.{key}' is {host[key]} in the file, "
                                 f"{getattr(self, key)} in the run")

    def run_restored(self, host: Dict[str, int], blocks) -> None:
        self.seed = int(host["seed"])
