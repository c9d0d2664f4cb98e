"""Histograms of several tensors in one launch, over TensorBoard's bucket set (`dctn_tensor_hist`, csrc/tensor_hist.hip).

The reference's runner logs a histogram of every ConvSBS string's output every 20 iterations through a forward hook and
``writer.add_histogram`` (mnist.py:537-553, ``log_dumb_histogram``).  No hook runs inside a captured training step, and
nothing capturable in torch produces that histogram: ``torch.histogram`` has no GPU kernel, ``histc`` has uniform bins
only, ``bincount`` synchronises.  `OutputHistograms` keeps one block per named tensor on the device - a header of
counters and ``n_edges - 1`` uint64 counts (`block_dtype`, include/dctn_amd.h): ``record`` only enqueues a launch (it is
capturable), every recorded launch ADDS to the block, and a device-side ``period`` makes only every period-th launch
count, so a K-iteration graph launch gives the reference's "every 20 iterations" without a host decision.  ``read`` is
the one place that synchronises.  The counts are those of ``numpy.histogram(values.astype(float64), bins=edges)``,
exactly: integer sums, found by comparisons against the table (`reference_counts` is the numpy mirror).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

MAX_TENSORS_PER_LAUNCH = 8
MAX_EDGES = 2048
HEADER_BYTES = 80
COUNTERS = ("total", "below", "above", "nan", "pos_inf", "neg_inf")
_HEADER_FIELDS = [(name, "<u8") for name in COUNTERS] + [("max_key", "<u8"), ("min_key_c", "<u8"), ("calls", "<u4"),
                                                         ("recorded", "<u4"), ("ticket", "<u4"), ("reserved", "<u4")]
_SIGN = 1 << 63
_MASK = (1 << 64) - 1


def block_dtype(n_edges: int) -> np.dtype:
    """The block of include/dctn_amd.h for a table of ``n_edges`` edges: the header, then ``counts``."""
    dt = np.dtype(_HEADER_FIELDS + [("counts", "<u8", (int(n_edges) - 1,))])
    assert dt.itemsize == HEADER_BYTES + 8 * (int(n_edges) - 1)
    return dt


def tensorboard_edges() -> np.ndarray:
    """The 1549 float64 edges of TensorBoard's default bucket set (what ``add_histogram(bins="tensorflow")`` uses).  The
    rule, in Python floats::

        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1

    and the table is the negated list reversed, then 0.0, then the list: 774 positive edges, strictly increasing, the
    last one 9.920775621859783e+19."""
    pos: List[float] = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-p for p in reversed(pos)] + [0.0] + pos, dtype=np.float64)


def check_edges(edges) -> np.ndarray:
    """``edges`` as a float64 array the kernel accepts: 2..2048 finite, strictly increasing values."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    if not 2 <= e.size <= MAX_EDGES:
        raise ValueError(f"an edge table has 2..{MAX_EDGES} edges, got {e.size}")
    if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError("an edge table is finite and strictly increasing")
    return e


def key_to_float(key: int) -> float:
    """The float64 value of an order-preserving key (include/dctn_amd.h)."""
    key = int(key)
    bits = key ^ _SIGN if key & _SIGN else ~key & _MASK
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def float_to_key(value: float) -> int:
    bits = int(np.array([value], dtype=np.float64).view(np.uint64)[0])
    return ~bits & _MASK if bits & _SIGN else bits | _SIGN


def reference_counts(values, edges) -> dict:
    """What one recorded launch of the kernel adds for ``values``, in numpy: ``counts`` (int64, one per bin), the six
    counters, and ``min`` / ``max`` of the finite values (+inf / -inf if there is none).  A finite v counts in bin i when
    ``edges[i] <= v < edges[i + 1]``, the last bin closed on the right; values are widened to float64 exactly and
    compared there; -0.0 is 0.0; finite values outside the table count in ``below`` / ``above``, the others in ``nan``,
    ``pos_inf``, ``neg_inf``."""
    e = check_edges(edges)
    v = np.asarray(values).reshape(-1).astype(np.float64)
    finite = v[np.isfinite(v)] + 0.0
    at = np.searchsorted(e, finite, side="right")   # the number of edges <= v
    inside = (at > 0) & (at < e.size)
    counts = np.bincount(at[inside] - 1, minlength=e.size - 1).astype(np.int64)
    counts[-1] += int(np.count_nonzero(finite == e[-1]))
    return {
        "counts": counts, "total": int(v.size), "below": int(np.count_nonzero(finite < e[0])),
        "above": int(np.count_nonzero(finite > e[-1])), "nan": int(np.count_nonzero(np.isnan(v))),
        "pos_inf": int(np.count_nonzero(v == np.inf)), "neg_inf": int(np.count_nonzero(v == -np.inf)),
        "min": float(finite.min()) if finite.size else float("inf"),
        "max": float(finite.max()) if finite.size else float("-inf"),
    }


def trim_buckets(counts, edges) -> Tuple[List[float], List[int]]:
    """``(bucket_limits, bucket_counts)`` as TensorBoard's ``make_histogram`` cuts them: the buckets from the first to
    the last non-empty one, each with its RIGHT limit, and one empty bucket in front whose limit is the first bucket's
    left edge.  A histogram without a count, which ``make_histogram`` refuses, keeps the table's first bucket."""
    counts = np.asarray(counts).astype(np.int64)
    limits = np.asarray(edges, dtype=np.float64)
    if not counts.any():
        return limits[:2].tolist(), [0, 0]
    cum = np.cumsum(counts > 0)
    start, end = (int(i) for i in np.searchsorted(cum, [0, cum[-1] - 1], side="right"))
    end += 1
    kept = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    return limits[start:end + 1].tolist(), [int(c) for c in kept]


def histogram_summary(entry: dict, edges) -> dict:
    """The arguments of ``SummaryWriter.add_histogram_raw`` from one entry of `OutputHistograms.read`.  ``min``, ``max``,
    ``num`` (every element seen), ``bucket_limits`` and ``bucket_counts`` are exact.  ``sum`` and ``sum_squares`` are
    APPROXIMATIONS formed here in float64 from each bucket's geometric centre (0 for a bucket that touches or straddles
    0), over the elements inside the table only: the kernel deliberately holds no float sums."""
    e = np.asarray(edges, dtype=np.float64)
    counts = np.asarray(entry["counts"]).astype(np.float64)
    lo, hi = e[:-1], e[1:]
    same_sign = lo * hi > 0.0
    centre = np.where(same_sign, np.sign(lo) * np.sqrt(np.where(same_sign, lo * hi, 1.0)), 0.0)
    limits, kept = trim_buckets(entry["counts"], e)
    return {"min": float(entry["min"]), "max": float(entry["max"]), "num": int(entry["total"]),
            "sum": float((counts * centre).sum()), "sum_squares": float((counts * centre * centre).sum()),
            "bucket_limits": limits, "bucket_counts": kept}


class OutputHistograms:
    """``names``: one name per tensor that every ``record`` call will be given, in that order.  ``edges``: one table for
    all of them (default `tensorboard_edges`).  ``period``: launch number c (counted on the device from 0, and kept by
    ``reset``) is recorded iff ``c % period == 0``."""

    def __init__(self, device, names: Sequence[str], edges=None, period: int = 1):
        names = tuple(str(n) for n in names)
        if not names or len(set(names)) != len(names):
            raise ValueError(f"OutputHistograms takes at least one name, each once; got {names!r}")
        if int(period) < 1:
            raise ValueError(f"OutputHistograms: period >= 1, got {period}")
        table = check_edges(tensorboard_edges() if edges is None else edges)
        dev = torch.device(device)
        if dev.type != "cuda":   # the project's boundary rule: a CPU caller is served by the current GPU, or not at all
            dev, _ = L.placement(torch.empty(0, device=dev))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.names, self.device, self.period = names, dev, int(period)
        self.edges, self.n_edges = table, int(table.size)
        self.dtype = block_dtype(self.n_edges)
        self.block_bytes = int(L.lib().dctn_tensor_hist_block_bytes(self.n_edges))
        assert self.block_bytes == self.dtype.itemsize
        self.edges_device = torch.from_numpy(table.copy()).to(dev)
        self.blocks = torch.zeros(len(names) * self.block_bytes, dtype=torch.uint8, device=dev)
        # (first tensor, number of tensors, pointer to the chunk's blocks) of every launch, built once
        self._chunks = [(k, min(MAX_TENSORS_PER_LAUNCH, len(names) - k), self.blocks.data_ptr() + k * self.block_bytes)
                        for k in range(0, len(names), MAX_TENSORS_PER_LAUNCH)]

    def record(self, tensors: Sequence[Tensor]) -> None:
        """Enqueues ceil(len / 8) launches on the current stream of the blocks' device; reads nothing back."""
        tensors = list(tensors)
        if len(tensors) != len(self.names):
            raise ValueError(f"OutputHistograms.record: {len(self.names)} tensors ({', '.join(self.names)}), got {len(tensors)}")
        dtype = tensors[0].dtype
        if any(t.dtype != dtype for t in tensors):
            raise TypeError("OutputHistograms.record: the tensors of one call have one dtype")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"OutputHistograms.record takes float32 or float64 tensors, got {dtype}")
        _, staged = L.placement(*tensors)
        held = [t.detach().to(self.device) if staged else t.detach() for t in tensors]
        L.require_device(self.blocks, *held)
        held = [t if t.is_contiguous() else t.contiguous() for t in held]
        lib, code = L.lib(), L.dtype_code(held[0])
        with torch.cuda.device(self.device):
            stream = L.stream_ptr(self.device)
            for first, count, block_ptr in self._chunks:
                part = held[first : first + count]
                L.check(lib.dctn_tensor_hist(L.ptr_array(part), L.i64_array([t.numel() for t in part]), count,
                                             self.edges_device.data_ptr(), self.n_edges, block_ptr, self.period, code, stream),
                        "tensor histograms")

    def reset(self) -> None:
        """Empties every block and keeps ``calls``: the period's phase survives.  One launch on the current stream."""
        with torch.cuda.device(self.device):
            L.check(L.lib().dctn_tensor_hist_reset(self.blocks.data_ptr(), len(self.names), self.n_edges,
                                                   L.stream_ptr(self.device)), "tensor histograms reset")

    def raw(self) -> np.ndarray:
        """The blocks as they are on the device (structured array, `block_dtype`); synchronises."""
        return self.blocks.cpu().numpy().view(self.dtype).copy()

    def read(self, reset: bool = False) -> Dict[str, dict]:
        """Per name: counts (int64 array), below, above, nan, pos_inf, neg_inf, total, min, max (of the finite values;
        +inf / -inf while there is none), calls, recorded.  Synchronises; ``reset=True`` empties the blocks afterwards."""
        out = {}
        for name, r in zip(self.names, self.raw()):
            entry = {"counts": r["counts"].astype(np.int64)}
            entry.update({key: int(r[key]) for key in COUNTERS[1:]})
            entry["total"] = int(r["total"])
            entry["min"] = key_to_float(~int(r["min_key_c"]) & _MASK) if int(r["min_key_c"]) else float("inf")
            entry["max"] = key_to_float(r["max_key"]) if int(r["max_key"]) else float("-inf")
            entry["calls"], entry["recorded"] = int(r["calls"]), int(r["recorded"])
            out[name] = entry
        if reset:
            self.reset()
        return out

    def trimmed(self, name: str) -> Tuple[List[float], List[int]]:
        """``(bucket_limits, bucket_counts)`` of one name, cut as TensorBoard's ``make_histogram`` cuts them
        (`trim_buckets`).  Synchronises."""
        return trim_buckets(self.read()[name]["counts"], self.edges)


Sink = Callable[[str, dict, int], None]


class HistogramLogger:
    """Hook for `training.train_graphed`: every ``every`` calls (launches) it reads the histograms - the one
    synchronisation it makes -, calls ``sink(name, summary, num_iters_done)`` per name with `histogram_summary`'s dict,
    and resets the blocks."""

    def __init__(self, hists: "OutputHistograms", every: int, sink: Sink):
        assert every >= 1
        self.hists, self.every, self.sink = hists, int(every), sink
        self._calls = 0

    def __call__(self, st_x, st_it) -> None:
        self._calls += 1
        if self._calls % self.every == 0:
            self.flush(int(st_it["num_iters_done"]))

    def flush(self, num_iters_done: int) -> None:
        """Reads, reports and resets now (call it when the loop ends, for the launches after the last multiple)."""
        for name, entry in self.hists.read(reset=True).items():
            self.sink(name, histogram_summary(entry, self.hists.edges), num_iters_done)
