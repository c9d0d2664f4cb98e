"""What the reference's TensorBoard hooks read off the BATCH, kept on the device in one launch per iteration
(`dctn_batch_monitor`, csrc/batch_monitor.hip).

Three hooks of the reference look at the batch itself, not at the model's insides:

* the input statistics (mnist.py:298-311 and :571-591): ``train_input/dumb_mean`` and ``dumb_std`` of the quantum batch and
  ``std_of_coordinates_of_windows`` of its 3 x 3 windows as rank-one tensors (``RankOneTensorsBatch.std_over_batch``), every
  20 iterations;
* the whole model's output (mnist.py:555-569): signed min, max, mean and std of the logits and the histogram of
  ``softmax(logits, dim=1)`` (``log_logits_as_probabilities``);
* the per-sample confidence (new_runner.py:512-531, ``--tb-batches``): the probability every sample gives its true class,
  beside the sample indices.

None of them can run inside a captured step, and under ``iters_per_launch=K`` the K - 1 inner batches are never visible
to the host at all.  `BatchMonitor` keeps one block on the device (`block_dtype`, include/dctn_amd.h): ``record`` only
enqueues the launch (it is capturable), a device-side ``period`` makes only every period-th launch read anything, and every
recorded launch writes one row of a ring of ``capacity`` rows.  ``read`` is the one place that synchronises.  `mirror` is
the same definition in numpy float64, `decode` the pure ring logic (`param_stats.decode`).

Pass it to the step - ``GraphedTrainStep(..., monitor=mon)`` or ``train_step(..., monitor=mon, indices=...)`` - and every
iteration ends with the record of the batch it trained on, the logits it produced and the labels.  In a data-parallel run
every rank records its own shard.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import tensor_hist
from .param_stats import decode  # noqa: F401  (the ring logic is the parameter monitor's)

HEADER_BYTES = 32
ROW_HEAD_BYTES = 112
SLOT_BYTES = 40
MAX_LABELS = 1024
MAX_EDGES = tensor_hist.MAX_EDGES
MAX_BATCH = (1 << 31) - 2

_HEAD = [("call", "<u4"), ("seq", "<u4"), ("rows", "<u4"), ("correct", "<u4"), ("bad_rows", "<u4"), ("z_nonfinite", "<u4"),
         ("x_nonfinite", "<u8"), ("x_sum", "<f8"), ("x_sum_sq", "<f8"), ("win_sum", "<f8"), ("win_sq", "<f8"),
         ("z_sum", "<f8"), ("z_sum_sq", "<f8"), ("z_min", "<f8"), ("z_max", "<f8"),
         ("below", "<u4"), ("above", "<u4"), ("nan", "<u4"), ("reserved", "<u4")]

TAGS = {
    "input_mean": "train_input/dumb_mean",
    "input_std": "train_input/dumb_std",
    "window_std": "train_input_intermediate_output_std_of_coordinates_of_windows/",
    "logits_min": "train_outputs_of_the_whole_model_intermediate_output_dumb_min/",
    "logits_max": "train_outputs_of_the_whole_model_intermediate_output_dumb_max/",
    "logits_mean": "train_outputs_of_the_whole_model_intermediate_output_dumb_mean/",
    "logits_std": "train_outputs_of_the_whole_model_intermediate_output_dumb_std/",
    "probabilities": "train_outputs_of_the_whole_model_intermediate_output_logits_as_probabilities/",
}


def row_dtype(batch: int, n_edges: int) -> np.dtype:
    """One row of the block: the 112-byte head, ``counts[n_edges - 1]`` (padded to 8 bytes), then the four per-sample
    arrays."""
    bins = int(n_edges) - 1
    fields = list(_HEAD) + [("counts", "<u4", (bins,))]
    if bins % 2:
        fields.append(("counts_pad", "<u4"))
    fields += [("label", "<i8", (int(batch),)), ("index", "<i8", (int(batch),)), ("p_true", "<f4", (int(batch),)),
               ("pred", "<i4", (int(batch),))]
    dt = np.dtype(fields)
    assert dt.itemsize == ROW_HEAD_BYTES + 8 * ((bins + 1) // 2) + 24 * int(batch)
    return dt


def block_dtype(batch: int, n_edges: int, capacity: int) -> np.dtype:
    """The block of include/dctn_amd.h as ONE structured element: the header, then ``rows`` (``capacity`` of `row_dtype`)."""
    dt = np.dtype([("calls", "<u4"), ("recorded", "<u4"), ("ticket", "<u4"), ("reserved", "<u4", (5,)),
                   ("rows", row_dtype(batch, n_edges), (int(capacity),))])
    assert dt.itemsize == HEADER_BYTES + int(capacity) * row_dtype(batch, n_edges).itemsize
    return dt


def probability_edges() -> np.ndarray:
    """Entries 774..1065 of `tensor_hist.tensorboard_edges`: 292 edges from 0.0 to 1.0089710279437536 - TensorBoard's own
    buckets restricted to where a probability can fall.  The default table."""
    return tensor_hist.tensorboard_edges()[774:1066].copy()


def mirror(x, logits, y, indices=None, kernel_size: int = 3, edges=None) -> dict:
    """What one recorded launch writes for these inputs, by the header's definitions in numpy float64: every field of a row
    but ``call`` / ``seq``, under the row's names; ``p_true`` is left in float64 (the device rounds it to float32).
    ``x``: (C, B, H, W, Q), ``logits``: (B, L), ``y``: (B,), tensors or arrays of any float dtype."""
    table = tensor_hist.check_edges(probability_edges() if edges is None else edges)

    def f64(a):
        return (a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)

    xs, z = f64(x), f64(logits)
    labels = (y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)).astype(np.int64)
    C, B, H, W, Q = xs.shape
    L_ = z.shape[1]
    K = int(kernel_size)
    out = {}
    finite = np.isfinite(xs)
    kept = np.where(finite, xs, 0.0)
    out["x_nonfinite"] = int(xs.size - np.count_nonzero(finite))
    out["x_sum"], out["x_sum_sq"] = float(kept.sum()), float((kept * kept).sum())
    if K > 0:
        with np.errstate(invalid="ignore", over="ignore"):
            s, u = xs.sum(axis=4), (xs * xs).sum(axis=4)   # (C, B, H, W): the pairs, nothing filtered
            Ho, Wo = H - K + 1, W - K + 1
            ps, pq = np.ones((B, Ho, Wo)), np.ones((B, Ho, Wo))
            for dh in range(K):
                for dw in range(K):
                    for c in range(C):
                        ps = ps * s[c, :, dh:dh + Ho, dw:dw + Wo]
                        pq = pq * u[c, :, dh:dh + Ho, dw:dw + Wo]
            out["win_sum"], out["win_sq"] = float(ps.sum()), float(pq.sum())
    else:
        out["win_sum"], out["win_sq"] = 0.0, 0.0

    zf = np.isfinite(z)
    zk = np.where(zf, z, 0.0)
    out["z_nonfinite"] = int(z.size - np.count_nonzero(zf))
    out["z_sum"], out["z_sum_sq"] = float(zk.sum()), float((zk * zk).sum())
    out["z_min"] = float(z[zf].min()) if zf.any() else float("inf")
    out["z_max"] = float(z[zf].max()) if zf.any() else float("-inf")
    good = zf.all(axis=1)
    valid = (labels >= 0) & (labels < L_)
    p = np.full((B, L_), np.nan)
    if good.any():
        zg = z[good]
        e = np.exp(zg - zg.max(axis=1, keepdims=True))
        S = np.zeros(e.shape[0])
        for j in range(L_):   # in increasing j
            S = S + e[:, j]
        p[good] = e / S[:, None]
    pred = np.where(good, np.where(zf, z, -np.inf).argmax(axis=1), -1).astype(np.int32)
    ref = tensor_hist.reference_counts(p[good], table)
    out["counts"] = ref["counts"]
    out["below"], out["above"] = ref["below"], ref["above"]
    out["nan"] = int(np.count_nonzero(~good)) * L_
    out["bad_rows"] = int(np.count_nonzero(~good))
    out["rows"] = int(np.count_nonzero(valid))
    out["correct"] = int(np.count_nonzero(valid & (pred == labels)))
    p_true = np.full(B, np.nan)
    sel = valid & good
    p_true[sel] = p[sel, labels[sel]]
    out["p_true"], out["pred"], out["label"] = p_true, pred, labels
    out["index"] = (np.full(B, -1, dtype=np.int64) if indices is None else
                    (indices.detach().cpu().numpy() if isinstance(indices, torch.Tensor) else np.asarray(indices)).astype(np.int64))
    return out


def _unbiased_std(total: float, sq: float, n: float) -> float:
    """``torch.std`` of n values from their sum and sum of squares; NaN for n < 2."""
    if n < 2:
        return float("nan")
    return math.sqrt(max((sq - total * total / n) / (n - 1), 0.0))


def summarise(row, x_shape: Tuple[int, int, int, int], batch: int, labels: int, kernel_size: int) -> dict:
    """One entry of `BatchMonitor.read` from a row (a `row_dtype` element, or `mirror`'s dict): Python floats and ints,
    and the four per-sample arrays.  ``mean`` and ``std`` divide by EVERY element's count; the sums run over the finite
    ones.  The window values are `window_stats.window_mean_var`'s formula in float64
    (``RankOneTensorsBatch.std_over_batch``); None when ``kernel_size`` is 0."""
    C, H, W, Q = (int(v) for v in x_shape)
    K = int(kernel_size)
    n_x, n_z = float(C * batch * H * W * Q), float(batch * labels)
    x_sum, x_sq = float(row["x_sum"]), float(row["x_sum_sq"])
    z_sum, z_sq = float(row["z_sum"]), float(row["z_sum_sq"])
    window_mean = window_std = None
    if K > 0:
        n = batch * (H - K + 1) * (W - K + 1) * float(Q) ** (K * K * C)
        total, sq = float(row["win_sum"]), float(row["win_sq"])
        window_mean = total / n
        var = sq / (n - 1) - 2 * total / (n - 1) * window_mean + n / (n - 1) * window_mean**2
        window_std = math.sqrt(var) if var >= 0 else float("nan")
    return {
        "rows": int(row["rows"]), "correct": int(row["correct"]), "bad_rows": int(row["bad_rows"]),
        "input": {"mean": x_sum / n_x, "std": _unbiased_std(x_sum, x_sq, n_x), "nonfinite": int(row["x_nonfinite"]),
                  "window_mean": window_mean, "window_std": window_std, "sum": x_sum, "sum_sq": x_sq,
                  "win_sum": float(row["win_sum"]), "win_sq": float(row["win_sq"])},
        "logits": {"min": float(row["z_min"]), "max": float(row["z_max"]), "mean": z_sum / n_z,
                   "std": _unbiased_std(z_sum, z_sq, n_z), "nonfinite": int(row["z_nonfinite"]), "sum": z_sum, "sum_sq": z_sq},
        "hist": {"counts": np.asarray(row["counts"]).astype(np.int64), "below": int(row["below"]), "above": int(row["above"]),
                 "nan": int(row["nan"])},
        "p_true": np.array(row["p_true"]), "pred": np.array(row["pred"]), "label": np.array(row["label"]),
        "index": np.array(row["index"]),
    }


def histogram_summary(hist: dict, edges) -> dict:
    """The arguments of ``SummaryWriter.add_histogram_raw`` from the ``hist`` of one entry of `BatchMonitor.read`.
    ``num`` (the probabilities inside the table), ``bucket_limits`` and ``bucket_counts`` (`tensor_hist.trim_buckets`) are
    exact; ``min`` / ``max`` are the outer limits of the first and last non-empty bucket, and ``sum`` / ``sum_squares`` come
    from the buckets' geometric centres (`tensor_hist.histogram_summary`): the kernel keeps no float sums of the
    probabilities."""
    e = np.asarray(edges, dtype=np.float64)
    counts = np.asarray(hist["counts"]).astype(np.int64)
    filled = np.flatnonzero(counts)
    lo, hi = (float(e[filled[0]]), float(e[filled[-1] + 1])) if filled.size else (float("inf"), float("-inf"))
    return tensor_hist.histogram_summary({"counts": counts, "min": lo, "max": hi, "total": int(counts.sum())}, e)


_TORCH_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


class BatchMonitor:
    """``batch`` samples of ``x_shape = (C, H, W, Q)`` and ``labels`` logits each.  Launch number c (counted on the device
    from 0) is recorded iff ``c % period == 0``; the block keeps the last ``capacity`` recorded rows.  ``kernel_size`` 0
    turns the window sums off.  ``edges``: the probabilities' table (default `probability_edges`)."""

    def __init__(self, device, batch: int, labels: int, x_shape: Sequence[int], kernel_size: int = 3, period: int = 20,
                 capacity: int = 16, edges=None):
        x_shape = tuple(int(v) for v in x_shape)
        batch, labels, K = int(batch), int(labels), int(kernel_size)
        if len(x_shape) != 4 or min(x_shape) < 1 or batch < 1:
            raise ValueError(f"BatchMonitor: x_shape = (C, H, W, Q) and batch are positive, got {x_shape} and {batch}")
        if not 1 <= labels <= MAX_LABELS:
            raise ValueError(f"BatchMonitor: 1..{MAX_LABELS} labels, got {labels}")
        if K < 0 or K > x_shape[1] or K > x_shape[2]:
            raise ValueError(f"BatchMonitor: windows of {K} x {K} on {x_shape[1]} x {x_shape[2]} pixels")
        if int(period) < 1 or int(capacity) < 1:
            raise ValueError(f"BatchMonitor: period >= 1 and capacity >= 1, got {period} and {capacity}")
        if batch > MAX_BATCH or batch * labels >= 1 << 32:
            raise NotImplementedError(f"BatchMonitor: batch * labels < 2^32 and batch <= {MAX_BATCH}, got {batch} x {labels}")
        table = tensor_hist.check_edges(probability_edges() if edges is None else edges)
        dev = torch.device(device)   # (a block on the CPU can be built and decoded, as `ParamStats`'; not recorded into)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device, self.batch, self.labels, self.x_shape, self.kernel_size = dev, batch, labels, x_shape, K
        self.period, self.capacity = int(period), int(capacity)
        self.edges, self.n_edges = table, int(table.size)
        self.dtype = block_dtype(batch, self.n_edges, self.capacity)
        lib = L.lib()
        self.block_bytes = int(lib.dctn_batch_monitor_block_bytes(batch, self.n_edges, self.capacity))
        assert self.block_bytes == self.dtype.itemsize
        self.workspace_bytes = int(lib.dctn_batch_monitor_workspace_bytes(batch))
        assert self.workspace_bytes == SLOT_BYTES * batch
        self.block = torch.zeros(self.block_bytes, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.edges_device = torch.from_numpy(table.copy()).to(dev)
        C, H, W, Q = x_shape
        self._call = L.BatchMonitorCall(edges=self.edges_device.data_ptr(), block=self.block.data_ptr(),
                                        workspace=self.workspace.data_ptr(), workspace_bytes=self.workspace_bytes, B=batch,
                                        C=C, H=H, W=W, Q=Q, K=K, L=labels, n_edges=self.n_edges, period=self.period,
                                        capacity=self.capacity)
        self._call_ref = ctypes.byref(self._call)
        self._seen = 0     # rows read so far, counted as the device counts `recorded`
        self.lost = 0      # rows overwritten before they were read

    def record(self, x: torch.Tensor, logits: torch.Tensor, y: torch.Tensor, indices: Optional[torch.Tensor] = None) -> None:
        """Enqueues the one launch on the current stream of the block's device; reads nothing back.  ``x``: contiguous
        (C, batch, H, W, Q); ``logits``: contiguous (batch, labels); float32, float64 or bfloat16 each; ``y`` and
        ``indices`` (optional): int64 (batch,)."""
        C, H, W, Q = self.x_shape
        if x.ndim == 4:
            raise ValueError(f"BatchMonitor.record reads the QUANTUM form of the batch, (C, B, H, W, Q) = "
                             f"{(C, self.batch, H, W, Q)} as a DeviceBatches draws it, not a {tuple(x.shape)} image batch")
        for what, t, shape in (("x", x, (C, self.batch, H, W, Q)), ("logits", logits, (self.batch, self.labels)),
                               ("y", y, (self.batch,)), ("indices", indices, (self.batch,))):
            if t is None:
                continue
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"BatchMonitor.record: {what} must be contiguous {shape}, got {tuple(t.shape)}")
            if t.device != self.device:
                raise ValueError(f"BatchMonitor reads the buffers where they are: {what} on {t.device}, the block on {self.device}")
        if x.dtype not in _TORCH_DTYPES or logits.dtype not in _TORCH_DTYPES:
            raise TypeError(f"BatchMonitor.record takes float32, float64 or bfloat16, got x {x.dtype}, logits {logits.dtype}")
        if y.dtype != torch.int64 or (indices is not None and indices.dtype != torch.int64):
            raise TypeError(f"BatchMonitor.record: y and indices are int64, got {y.dtype} and "
                            f"{None if indices is None else indices.dtype}")
        L.require_device(self.block, x, logits, y)   # the project's boundary rule: a library call has no CPU form
        c = self._call
        c.x, c.logits, c.y = x.data_ptr(), logits.data_ptr(), y.data_ptr()
        c.indices = None if indices is None else indices.data_ptr()
        c.x_dtype, c.logits_dtype = L.dtype_code(x), L.dtype_code(logits)
        with torch.cuda.device(self.device):
            L.check(L.lib().dctn_batch_monitor(self._call_ref, L.stream_ptr(self.device)), "batch monitor")

    def reset(self, calls: int = 0) -> None:
        """Zeroes header and rows on the current stream, between launches, and starts the count again at ``calls``; what
        was not read is dropped (``lost`` returns to 0).  `GraphedTrainStep`'s warm-up steps count as calls: reset after
        building it."""
        if not 0 <= int(calls) < 1 << 32:
            raise ValueError(f"BatchMonitor.reset: calls is a uint32, got {calls}")
        self.block.zero_()
        if int(calls):
            word = torch.from_numpy(np.array([int(calls)], dtype="<u4").view(np.uint8).copy())
            self.block[:4].copy_(word.to(self.device))
        self._seen, self.lost = 0, 0

    def raw(self) -> np.ndarray:
        """The block as it is on the device (one structured element, `block_dtype`); synchronises."""
        return self.block.cpu().numpy().view(self.dtype)[0].copy()

    def read(self) -> List[dict]:
        """The rows not yet read, oldest first: ``call``, ``seq`` and `summarise`'s entries.  Rows overwritten before this
        read are counted in ``lost``.  Synchronises."""
        raw = self.raw()
        rows, lost = decode(raw, self._seen, self.capacity)
        self.lost += lost
        self._seen = int(raw["recorded"])
        out = []
        for row in rows:
            entry = {"call": int(row["call"]), "seq": int(row["seq"])}
            entry.update(summarise(row, self.x_shape, self.batch, self.labels, self.kernel_size))
            out.append(entry)
        return out


ScalarSink = Callable[[str, float, int], None]


class BatchMonitorLogger:
    """Hook for `training.train_graphed`: every ``every`` calls (launches) it reads the unread rows - the one
    synchronisation it makes - and reports each with ``iteration = first_iter + call``:
    ``scalar_sink(tag, value, iteration)`` for the seven scalars (``add_scalar``'s argument order; the window std is left
    out when the monitor has no windows), ``histogram_sink(tag, summary, iteration)`` with `histogram_summary`'s dict, and
    ``sample_sink(iteration, index, label, pred, p_true)`` with the four arrays.  ``tags``: `TAGS`, the reference's."""

    def __init__(self, mon, every: int, scalar_sink: ScalarSink, histogram_sink=None, sample_sink=None, first_iter: int = 0,
                 tags: Optional[Dict[str, str]] = None):
        assert every >= 1
        self.mon, self.every, self.first_iter = mon, int(every), int(first_iter)
        self.scalar_sink, self.histogram_sink, self.sample_sink = scalar_sink, histogram_sink, sample_sink
        self.tags = dict(TAGS, **(tags or {}))
        self._calls = 0

    def __call__(self, st_x, st_it) -> None:
        self._calls += 1
        if self._calls % self.every == 0:
            self.flush()

    def flush(self) -> None:
        """Reads and reports now (call it when the loop ends, for the launches after the last multiple)."""
        tags = self.tags
        for entry in self.mon.read():
            it = self.first_iter + int(entry["call"])
            if self.scalar_sink is not None:
                self.scalar_sink(tags["input_mean"], entry["input"]["mean"], it)
                self.scalar_sink(tags["input_std"], entry["input"]["std"], it)
                if entry["input"]["window_std"] is not None:
                    self.scalar_sink(tags["window_std"], entry["input"]["window_std"], it)
                for key in ("min", "max", "mean", "std"):
                    self.scalar_sink(tags["logits_" + key], entry["logits"][key], it)
            if self.histogram_sink is not None:
                self.histogram_sink(tags["probabilities"], histogram_summary(entry["hist"], self.mon.edges), it)
            if self.sample_sink is not None:
                self.sample_sink(it, entry["index"], entry["label"], entry["pred"], entry["p_true"])
