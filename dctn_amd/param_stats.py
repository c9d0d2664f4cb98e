"""Norm, mean, std, largest magnitude and non-finite count of every parameter and of its gradient, every iteration, in one
launch over a flat optimizer's two buffers (`dctn_param_stats`, csrc/param_stats.hip).

The reference's classifier script attaches ``add_weights_and_grads_logging(trainer, tb_logger, model)`` (mnist.py:535): a
norm of each parameter and of its gradient, every iteration.  The `EPSesPlusLinear` recipe has ``log_parameters_stats``
(dctn/training.py:247; here `training.log_parameters_stats`): mean, std and shape of every parameter.  Both read the host
once or twice per parameter, which no captured step can do, and in a bfloat16 run they see the rounded parameters, not
the float32 master copy the optimizer keeps.  `ParamStats` keeps one block on the device (`block_dtype`,
include/dctn_amd.h): ``record`` only enqueues the launch (it is capturable), a device-side ``period`` makes only every
period-th launch read anything, and every recorded launch writes one row of a ring of ``capacity`` rows - one 64-byte
cell per parameter, sums in float64 over the finite elements - so a launch of K iterations keeps every recorded
iteration.  ``read`` is the one place that synchronises.

Pass it to a flat optimizer - ``FlatAdam(..., param_stats=ps)``, `FlatSGD`, `FlatRMSprop` - and every ``step()`` ends with
the record, behind the step launch: the weights are the ones the step just wrote (the master copy where there is one),
the gradients the buffer the step read, before the guard's coefficient.  `cell_moments` and `decode` are the pure
functions behind ``read``.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

MAX_SEGMENTS = 64
MAX_SEGMENT_ELEMENTS = (1 << 31) - 1
HEADER_BYTES = 32
ROW_HEAD_BYTES = 16
CELL_BYTES = 64
PER_WORKGROUP = 8192    # elements that earn a segment one workgroup of the kernel's plan
MAX_WORKGROUPS = 64     # per segment

CELL = np.dtype([("w_sum", "<f8"), ("w_sum_sq", "<f8"), ("w_max_abs", "<f8"), ("w_nonfinite", "<u8"),
                 ("g_sum", "<f8"), ("g_sum_sq", "<f8"), ("g_max_abs", "<f8"), ("g_nonfinite", "<u8")])
assert CELL.itemsize == CELL_BYTES


def block_dtype(n_segments: int, capacity: int) -> np.dtype:
    """The block of include/dctn_amd.h as ONE structured element: the header, then ``rows`` (``capacity`` of them), each
    with ``cells[n_segments]`` of `CELL`."""
    row = np.dtype([("call", "<u4"), ("seq", "<u4"), ("reserved", "<u8"), ("cells", CELL, (int(n_segments),))])
    dt = np.dtype([("calls", "<u4"), ("recorded", "<u4"), ("ticket", "<u4"), ("reserved", "<u4", (5,)),
                   ("rows", row, (int(capacity),))])
    assert dt.itemsize == HEADER_BYTES + int(capacity) * (ROW_HEAD_BYTES + CELL_BYTES * int(n_segments))
    return dt


def workspace_bytes(ends: Sequence[int]) -> int:
    """The header's rule, on the host: 64 bytes per workgroup, ``min(64, ceil(c / 8192))`` workgroups per segment of c
    elements."""
    sizes = np.diff(np.concatenate(([0], np.asarray(ends, dtype=np.int64))))
    return int(sum(min(MAX_WORKGROUPS, -(-int(c) // PER_WORKGROUP)) for c in sizes)) * CELL_BYTES


def cell_moments(n: int, cell) -> Dict[str, Dict[str, float]]:
    """``{"weights": {...}, "grads": {...}}`` of one cell of a segment of ``n`` elements: ``n``, ``sum``, ``sum_sq``,
    ``max_abs``, ``nonfinite`` as the device left them, and ``norm = sqrt(sum_sq)``, ``mean = sum / n``,
    ``std = sqrt(max(sum_sq / n - mean ** 2, 0))`` - the POPULATION std, as `training.log_parameters_stats` reports it.
    All Python floats.  The sums run over the finite elements only; ``n`` counts every element."""
    out = {}
    for key, prefix in (("weights", "w_"), ("grads", "g_")):
        total, sq = float(cell[prefix + "sum"]), float(cell[prefix + "sum_sq"])
        mean = total / n
        out[key] = {"n": float(n), "sum": total, "sum_sq": sq, "max_abs": float(cell[prefix + "max_abs"]),
                    "nonfinite": float(cell[prefix + "nonfinite"]), "norm": math.sqrt(sq), "mean": mean,
                    "std": math.sqrt(max(sq / n - mean * mean, 0.0))}
    return out


def decode(raw, seen: int, capacity: int) -> Tuple[list, int]:
    """The ring logic of ``read``: ``(rows, lost)`` for a block ``raw`` (one `block_dtype` element) of which ``seen``
    rows were read before.  ``rows``: the unread rows still in the ring, oldest first; ``lost``: how many were
    overwritten before this read.  The next ``seen`` is ``int(raw["recorded"])``."""
    recorded = int(raw["recorded"])
    first = max(int(seen), recorded - int(capacity))
    rows = []
    for seq in range(first, recorded):
        row = raw["rows"][seq % int(capacity)]
        assert int(row["seq"]) == seq, (int(row["seq"]), seq)
        rows.append(row)
    return rows, first - int(seen)


class ParamStats:
    """``names``: one per parameter of the optimizer that will hold the object, in its flat order (regularised + others),
    at most 64 (NotImplementedError).  Launch number c (counted on the device from 0) is recorded iff ``c % period == 0``;
    the block keeps the last ``capacity`` recorded rows.  The optimizer binds the segments' sizes (`bind`) when it is
    built; ``record`` refuses buffers of another size."""

    def __init__(self, device, names: Sequence[str], period: int = 1, capacity: int = 64):
        names = tuple(str(n) for n in names)
        if not names:
            raise ValueError("ParamStats takes at least one name")
        if len(set(names)) != len(names):
            raise ValueError(f"ParamStats takes every name once; got {names!r}")
        if int(period) < 1 or int(capacity) < 1:
            raise ValueError(f"ParamStats: period >= 1 and capacity >= 1, got {period} and {capacity}")
        if len(names) > MAX_SEGMENTS:
            raise NotImplementedError(f"ParamStats: at most {MAX_SEGMENTS} parameters (one segment per lane of a wave), "
                                      f"got {len(names)}")
        dev = torch.device(device)   # (a block on the CPU can be built, bound and decoded, as `ParamGroups`'; not recorded into)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.names, self.device, self.period, self.capacity = names, dev, int(period), int(capacity)
        self.dtype = block_dtype(len(names), self.capacity)
        self.block_bytes = int(L.lib().dctn_param_stats_block_bytes(len(names), self.capacity))
        assert self.block_bytes == self.dtype.itemsize
        self.block = torch.zeros(self.block_bytes, dtype=torch.uint8, device=dev)
        self.ends: Optional[List[int]] = None
        self.sizes: Optional[List[int]] = None
        self.workspace: Optional[torch.Tensor] = None
        self._seen = 0     # rows read so far, counted as the device counts `recorded`
        self.lost = 0      # rows overwritten before they were read

    @classmethod
    def for_parameters(cls, model: torch.nn.Module, params, period: int = 1, capacity: int = 64) -> "ParamStats":
        """The names ``model.named_parameters()`` gives the tensors of ``params`` (matched by identity), in the order of
        ``params`` - pass the optimizer's: regularised + others."""
        params = list(params)
        if not params:
            raise ValueError("ParamStats.for_parameters: no parameters")
        known = {id(p): name for name, p in model.named_parameters()}
        missing = [i for i, p in enumerate(params) if id(p) not in known]
        if missing:
            raise ValueError(f"ParamStats.for_parameters: parameters {missing} are not among model.named_parameters()")
        return cls(params[0].device, [known[id(p)] for p in params], period, capacity)

    def bind(self, sizes: Sequence[int]) -> None:
        """The element count of every name's segment, in order; a flat optimizer calls it with its parameters' sizes."""
        sizes = [int(s) for s in sizes]
        if len(sizes) != len(self.names):
            raise ValueError(f"ParamStats holds {len(self.names)} names, the optimizer {len(sizes)} parameters")
        if any(s < 1 for s in sizes):
            raise ValueError("ParamStats: a parameter without elements has no segment")
        if any(s > MAX_SEGMENT_ELEMENTS for s in sizes):
            raise NotImplementedError("ParamStats: a parameter of 2^31 elements or more")
        self.sizes, self.ends = sizes, [int(e) for e in np.cumsum(sizes)]
        self._ends = L.i64_array(self.ends)
        self.workspace_bytes = int(L.lib().dctn_param_stats_workspace_bytes(self._ends, len(sizes)))
        assert self.workspace_bytes == workspace_bytes(self.ends)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=self.device)

    def record(self, params: torch.Tensor, master: Optional[torch.Tensor], grads: torch.Tensor) -> None:
        """Enqueues the one launch on the current stream of the block's device; reads nothing back.  ``params`` and
        ``grads``: the flat buffers, one dtype; ``master``: the float32 copy of bfloat16 parameters, or None."""
        if self.ends is None:
            raise RuntimeError("ParamStats.record: no segments yet; pass the object to a flat optimizer (or call bind)")
        n = self.ends[-1]
        L.require_device(self.block, params, grads)   # the project's boundary rule: a library call has no CPU form
        for what, t in (("params", params), ("master", master), ("grads", grads)):
            if t is None:
                continue
            if t.device != self.device:
                raise RuntimeError(f"ParamStats reads the buffers where they are: {what} on {t.device}, the block on {self.device}")
            if t.numel() != n or not t.is_contiguous():
                raise ValueError(f"ParamStats.record: {what} must be contiguous with {n} elements, got {t.numel()}")
        if grads.dtype != params.dtype or (master is not None and master.dtype != torch.float32):
            raise TypeError(f"ParamStats.record: params {params.dtype}, grads {grads.dtype}, master "
                            f"{None if master is None else master.dtype}")
        with torch.cuda.device(self.device):
            L.check(L.lib().dctn_param_stats(params.data_ptr(), None if master is None else master.data_ptr(),
                                             grads.data_ptr(), self._ends, len(self.names), self.block.data_ptr(),
                                             self.capacity, self.period, self.workspace.data_ptr(), self.workspace_bytes,
                                             L.dtype_code(params), L.stream_ptr(self.device)), "parameter statistics")

    def reset(self, calls: int = 0) -> None:
        """Zeroes header and rows on the current stream, between launches, and starts the count again at ``calls``; what
        was not read is dropped (``lost`` returns to 0).  `GraphedTrainStep`'s warm-up steps count as calls: reset after
        building it."""
        if not 0 <= int(calls) < 1 << 32:
            raise ValueError(f"ParamStats.reset: calls is a uint32, got {calls}")
        self.block.zero_()
        if int(calls):
            word = torch.from_numpy(np.array([int(calls)], dtype="<u4").view(np.uint8).copy())
            self.block[:4].copy_(word.to(self.device))
        self._seen, self.lost = 0, 0

    def raw(self) -> np.ndarray:
        """The block as it is on the device (one structured element, `block_dtype`); synchronises."""
        return self.block.cpu().numpy().view(self.dtype)[0].copy()

    def read(self) -> List[dict]:
        """The rows not yet read, oldest first: ``{"call", "seq", "stats"}`` with ``stats[name] = {"weights": {...},
        "grads": {...}}`` (`cell_moments` of the parameter's element count).  Rows overwritten before this read are counted
        in ``lost``.  Synchronises."""
        if self.sizes is None:
            raise RuntimeError("ParamStats.read: no segments yet; pass the object to a flat optimizer (or call bind)")
        raw = self.raw()
        rows, lost = decode(raw, self._seen, self.capacity)
        self.lost += lost
        self._seen = int(raw["recorded"])
        return [{"call": int(row["call"]), "seq": int(row["seq"]),
                 "stats": {name: cell_moments(n, cell) for name, n, cell in zip(self.names, self.sizes, row["cells"])}}
                for row in rows]

    # a part of a run, as `GradGuard`; the optimizer that holds the monitor lists the block among its own regions
    def run_regions(self):
        return [("param_stats", self.block)]

    def run_host(self) -> Dict[str, object]:
        return dict(names=list(self.names), period=self.period, capacity=self.capacity, seen=self._seen, lost=self.lost)

    def run_restored(self, host, blocks) -> None:
        """The block came back (`checkpoint.RunState.load` put it in place): ``calls``, ``recorded`` and the ring go on
        from the file's, and so does what was read of it."""
        if host is not None:
            if list(host["names"]) != list(self.names):
                raise ValueError(f"ParamStats: the file's monitor names {list(host['names'])}, the run's {list(self.names)}")
            self._seen, self.lost = int(host["seen"]), int(host["lost"])


Sink = Callable[[str, float, int], None]


class ParamStatsLogger:
    """Hook for `training.train_graphed`: every ``every`` calls (launches) it reads the unread rows - the one
    synchronisation it makes - and reports each parameter of each row as
    ``sink(f"{weight_tag}/{name.replace('.', '/')}", weights norm, iteration)`` and
    ``sink(f"{grad_tag}/{name.replace('.', '/')}", gradient norm, iteration)`` with ``iteration = first_iter + call``
    (``add_scalar``'s argument order)."""

    def __init__(self, ps, every: int, sink: Sink, first_iter: int = 0, weight_tag: str = "weights_norm",
                 grad_tag: str = "grads_norm"):
        assert every >= 1
        self.ps, self.every, self.sink, self.first_iter = ps, int(every), sink, int(first_iter)
        self.weight_tag, self.grad_tag = str(weight_tag), str(grad_tag)
        self._calls = 0

    def __call__(self, st_x, st_it) -> None:
        self._calls += 1
        if self._calls % self.every == 0:
            self.flush()

    def flush(self) -> None:
        """Reads and reports now (call it when the loop ends, for the launches after the last multiple)."""
        for entry in self.ps.read():
            iteration = self.first_iter + int(entry["call"])
            for name, st in entry["stats"].items():
                path = name.replace(".", "/")
                self.sink(f"{self.weight_tag}/{path}", st["weights"]["norm"], iteration)
                self.sink(f"{self.grad_tag}/{path}", st["grads"]["norm"], iteration)
