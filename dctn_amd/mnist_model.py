"""The ConvSBS classifier: the reference's ``DCTNMnistModel`` (mnist.py:169-284) - two or more `ManyConvSBS` layers of two
9-core snake strings, a final string with ten labels on its middle core, the mean over positions.

Same constructor, same module tree (``conv_sbses.{layer}.strings.{string}.cores.{core}``: a reference checkpoint loads),
same ``forward`` and ``scale_layers_using_batch``.  What differs is how the tail runs:
  - a layer hands ONE stacked tensor to the next (`ManyConvSBS.forward_stacked`), not a tuple that is stacked again;
  - the mean over positions is `position_mean` (csrc/sbs_tail.hip): float64 sum in a fixed order, rounded once;
  - ``model.output_stats = OutputStats(dev, model.string_names())`` makes every training forward end with one launch that
    leaves mean / std / |y| range / non-finite count of every string's output on the device - the reference's forward
    hooks (mnist.py:537-553), which no captured step can run.  Eval forwards record nothing;
  - ``model.output_histograms = OutputHistograms(dev, model.string_names(), period=20)`` adds one more launch over the
    same outputs: the reference's `log_dumb_histogram` over TensorBoard's buckets, accumulated on the device;
  - ``model.tt_stats = TTStats.for_model(model, period=20)`` makes every training forward BEGIN with one launch that
    leaves the sum and squared norm of the tensor every string represents on the device, from the cores as the iteration
    finds them: the reference's ``mean_of_tt_tensor`` / ``std_of_tt_tensor`` (conv_sbs_statistics_logging.py);
  - `scale_layers_using_batch` reads the std of a layer's strings from one such launch and one host read per layer, and
    with a process group scales by the std of the UNION of the ranks' shards, so that replicas stay replicas.
`forward` also takes the quantum batch (1, B, H, W, 2) that a ``DeviceBatches(phi=quantum_phi(...), scale=multiplier)``
draws, which is how the model sits under `GraphedTrainStep` and `GraphedScore`.
"""
from __future__ import annotations

import logging
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib as L
from . import ddp
from .conv_sbs import Initialization, ManyConvSBS
from .conv_sbs_spec import SBSSpecCore
from .pos2d import Pos2D
from .tensor_hist import OutputHistograms
from .tensor_stats import OutputStats, std_from_moments
from .tt_stats import TTStats

logger = logging.getLogger(__name__)

NUM_LABELS = 10


def batch_to_quantum(x: Tensor, cos_sin_squared: bool, multiplier: float) -> Tensor:
    """(B, 1, H, W) -> (B, H, W, 2): (sin x, cos x), or their squares, times ``multiplier`` (mnist.py:132-141)."""
    assert x.ndim == 4 and x.shape[1] == 1
    batch = x[:, 0]
    if not cos_sin_squared:
        batch_quantum = torch.stack((torch.sin(batch), torch.cos(batch)), dim=3)
    else:
        batch_quantum = torch.stack((torch.sin(batch) ** 2, torch.cos(batch) ** 2), dim=3)
    assert batch_quantum.shape == (*batch.shape, 2)  # b h w 2
    return batch_quantum * multiplier


def quantum_phi(cos_sin_squared: bool) -> Tuple[Callable[[Tensor], Tensor], Callable[[Tensor], Tensor]]:
    """The feature map of `batch_to_quantum` as the callables of ``DeviceBatches(phi=..., scale=multiplier)``: the source's
    table then holds, for every byte value u, exactly ``batch_to_quantum(u / 255)``."""
    if not cos_sin_squared:
        return (torch.sin, torch.cos)
    return (lambda X: torch.sin(X) ** 2, lambda X: torch.cos(X) ** 2)


class _PositionMean(torch.autograd.Function):
    """y: (B, ..., L) -> (B, L), `dctn_position_mean_fwd` / `_bwd`."""

    @staticmethod
    def forward(ctx, y: Tensor) -> Tensor:
        dev = L.require_device(y)
        if y.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"position_mean takes float32 or float64, got {y.dtype}")
        assert y.ndim >= 2
        B, Lb = y.shape[0], y.shape[-1]
        P = y.numel() // max(B * Lb, 1)
        yc = y.contiguous()
        out = torch.empty((B, Lb), dtype=y.dtype, device=dev)
        L.check(L.lib().dctn_position_mean_fwd(yc.data_ptr(), out.data_ptr(), B, P, Lb, L.dtype_code(y), L.stream_ptr(dev)),
                "position mean forward")
        ctx.shape = tuple(y.shape)
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        shape = ctx.shape
        B, Lb = shape[0], shape[-1]
        P = 1
        for s in shape[1:-1]:
            P *= s
        g = d_out.contiguous()
        d_y = torch.empty(shape, dtype=g.dtype, device=g.device)
        L.check(L.lib().dctn_position_mean_bwd(g.data_ptr(), d_y.data_ptr(), B, P, Lb, L.dtype_code(g), L.stream_ptr(g.device)),
                "position mean backward")
        return d_y


def position_mean(y: Tensor) -> Tensor:
    """The mean over every dimension between the first and the last, ``einops.reduce(y, "b h w l -> b l", "mean")``: summed in
    float64 in a fixed order and rounded once; a sample's row does not depend on the batch it sits in.  L <= 64."""
    return L.on_device(_PositionMean.apply, y)


def _snake(positions: Sequence[Tuple[int, int]], middle_out: int) -> Tuple[SBSSpecCore, ...]:
    return tuple(SBSSpecCore(Pos2D(h, w), middle_out if i == 4 else 1) for i, (h, w) in enumerate(positions))


_SNAKE_ROWS = ((0, 0), (0, 1), (0, 2), (1, 2), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2))      # mnist.py:190-199
_SNAKE_COLUMNS = ((0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1), (0, 2), (1, 2), (2, 2))   # mnist.py:201-210


def string_scales(rows: Sequence[Sequence[float]], reduce: Optional[Callable] = None) -> List[Optional[float]]:
    """What `scale_layers_using_batch` divides each string of a layer by.  ``rows``: per string ``(n, sum, sum of squares,
    non-finite count)`` of its output on this rank's batch; ``reduce`` maps the rows of a shard to the rows of the union
    of all shards (default `ddp.all_reduce_moment_rows`: the identity without a process group).  Returns the unbiased std
    per string, or None for a string that is not to be scaled: std 0 or not finite, or non-finite outputs."""
    rows = (reduce or ddp.all_reduce_moment_rows)([tuple(float(v) for v in row) for row in rows])
    scales: List[Optional[float]] = []
    for n, s, ss, bad in rows:
        std = std_from_moments(n, s, ss)
        scales.append(std if bad == 0 and std > 0.0 and std != float("inf") else None)
    return scales


class DCTNMnistModel(nn.Module):
    def __init__(
        self,
        num_sbs_layers: int,
        bond_dim_size: int,
        trace_edge: bool,
        initialization: Initialization,
        cos_sin_squared: bool,
        input_multiplier: float,
        after_batch_to_quantum_callback: Optional[Callable[[Tensor], None]] = None,
    ):
        super().__init__()
        assert num_sbs_layers >= 2
        self.cos_sin_squared = cos_sin_squared
        self.input_multiplier = input_multiplier
        cores_specs = (_snake(_SNAKE_ROWS, 2), _snake(_SNAKE_COLUMNS, 2))
        final_string_cores_spec = _snake(_SNAKE_ROWS, NUM_LABELS)
        self.conv_sbses = nn.Sequential(
            ManyConvSBS(
                in_num_channels=1,
                in_quantum_dim_size=2,
                bond_dim_size=bond_dim_size,
                trace_edge=trace_edge,
                cores_specs=cores_specs,
                initializations=(initialization,) * len(cores_specs),
            ),
            *(
                ManyConvSBS(
                    in_num_channels=2,
                    in_quantum_dim_size=2,
                    bond_dim_size=bond_dim_size,
                    trace_edge=trace_edge,
                    cores_specs=cores_specs,
                    initializations=(initialization,) * len(cores_specs),
                )
                for i in range(num_sbs_layers - 2)
            ),
            ManyConvSBS(
                in_num_channels=2,
                in_quantum_dim_size=2,
                bond_dim_size=bond_dim_size,
                trace_edge=trace_edge,
                cores_specs=(final_string_cores_spec,),
                initializations=(initialization,),
            ),
        )
        self.after_batch_to_quantum_callback = after_batch_to_quantum_callback
        self.output_stats: Optional[OutputStats] = None   # opt-in: OutputStats(device, model.string_names())
        self.output_histograms: Optional[OutputHistograms] = None   # opt-in: OutputHistograms(device, model.string_names())
        self.tt_stats: Optional[TTStats] = None   # opt-in: TTStats.for_model(model, period), built after the optimizer

    def string_names(self) -> List[str]:
        """One name per string, in the order a forward records them: ``conv_sbses.{layer}.strings.{string}``."""
        return [f"conv_sbses.{li}.strings.{si}" for li, layer in enumerate(self.conv_sbses) for si in range(len(layer.strings))]

    def _quantum(self, x: Tensor) -> Tensor:
        """(1, B, H, W, 2) from the reference's (B, 1, H, W) images, or from a quantum batch as it is."""
        if x.ndim == 5:
            assert x.shape[0] == 1 and x.shape[-1] == 2, f"a quantum batch is (1, B, H, W, 2), got {tuple(x.shape)}"
            quantumized = x[0]
        else:
            quantumized = batch_to_quantum(x, self.cos_sin_squared, self.input_multiplier)
        if self.after_batch_to_quantum_callback is not None:
            self.after_batch_to_quantum_callback(quantumized)
        return quantumized.unsqueeze(0)

    @staticmethod
    def _layer(conv_sbs: ManyConvSBS, stacked: Tensor) -> Tensor:
        """(n_strings, B, H', W', out) of one layer; a single string's output is its own buffer already."""
        if len(conv_sbs.strings) == 1:
            return conv_sbs(stacked)[0].unsqueeze(0)
        return conv_sbs.forward_stacked(stacked)

    def forward(self, x: Tensor) -> Tensor:
        intermediate = self._quantum(x)
        stats = self.output_stats if self.training else None
        hists = self.output_histograms if self.training else None
        record = stats is not None or hists is not None
        outputs: List[Tensor] = []
        if self.training and self.tt_stats is not None:
            self.tt_stats.record()   # ONE launch over every string's cores, as the iteration finds them
        for conv_sbs in self.conv_sbses:
            intermediate = self._layer(conv_sbs, intermediate)
            if record:
                outputs.extend(intermediate.unbind(0))
        assert intermediate.shape[0] == 1
        if stats is not None:
            stats.record(outputs)   # ONE launch over every string's output (two beyond eight strings)
        if hists is not None:
            hists.record(outputs)   # and one more over the same list
        return position_mean(intermediate[0])

    def scale_layers_using_batch(self, x: Tensor, reduce: Optional[Callable] = None) -> Tensor:
        """The reference's calibration (mnist.py:265-284), layer by layer: every string is divided by the unbiased std of
        its output on the batch, the layer is recomputed and fed on.  The std comes from `dctn_tensor_stats` - one launch
        and one host read per layer - and, with a process group, from the moments summed over the ranks (``reduce``:
        see `string_scales`), so every rank divides by the same number.  Returns the pooled result."""
        with torch.no_grad():
            intermediate = self._quantum(x)
            for li, conv_sbs in enumerate(self.conv_sbses):
                before = self._layer(conv_sbs, intermediate)
                stats = OutputStats(before.device, [f"conv_sbses.{li}.strings.{si}" for si in range(len(conv_sbs.strings))])
                stats.record(before.unbind(0))
                raw = stats.raw()
                rows = [(float(int(r["n"]) - int(r["nonfinite"])), float(r["sum"]), float(r["sum_sq"]), float(r["nonfinite"]))
                        for r in raw]
                if reduce is None:
                    rows = ddp.all_reduce_moment_rows(rows, stats.device)
                    scales = string_scales(rows, reduce=lambda r: r)
                else:
                    scales = string_scales(rows, reduce)
                for string, std in zip(conv_sbs.strings, scales):
                    if std is not None:
                        string.multiply_by_scalar(std ** -1)
                        logger.info(f"Divided a ConvSBS by {std}")
                    else:
                        logger.warning("std == 0.0, not scaling")
                intermediate = self._layer(conv_sbs, intermediate)
            assert intermediate.shape[0] == 1
            return position_mean(intermediate[0])
