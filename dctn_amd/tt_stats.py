"""Mean and std of the tensor every ConvSBS string REPRESENTS, from the cores, in one launch (`dctn_tt_stats`,
csrc/tt_stats.hip).

The reference's runner attaches ``add_conv_sbs_tt_tensor_statistics_logging(model, writer, trainer, 20)``
(dctn/conv_sbs_statistics_logging.py, mnist.py:554) to every string: every 20 iterations it logs
``mean_of_tt_tensor/<name>`` and ``std_of_tt_tensor/<name>`` from ``ConvSBS.mean()`` and ``ConvSBS.var() ** 0.5`` - two
path-cache contractions of 9 and 18 operands and two host reads per string, which no captured step can run.  `TTStats`
keeps one block on the device (`block_dtype`, include/dctn_amd.h): ``record`` only enqueues the launch (it is capturable),
a device-side ``period`` makes only every period-th launch compute anything, and every recorded launch writes one row of
a ring of ``capacity`` rows - ``{sum, sq_norm}`` in float64 per string - so a launch of K iterations keeps every recorded
iteration.  ``read`` is the one place that synchronises.  `ConvSBS.sum` / `.var` themselves stay the differentiable,
CPU-capable torch contractions they are; `reference_moments` is a numpy mirror of the two formulas for tests and for
anyone without a GPU.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .conv_sbs import ConvSBS

MAX_STRINGS = 16
MAX_CORES = 16
MAX_BOND = 32
MAX_SLICES = 256   # q ** C
HEADER_BYTES = 32
ROW_HEAD_BYTES = 16


def block_dtype(n_strings: int, capacity: int) -> np.dtype:
    """The block of include/dctn_amd.h as ONE structured element: the header, then ``rows`` (``capacity`` of them), each
    with ``stats[n_strings, 2]`` = (sum, sq_norm) per string."""
    row = np.dtype([("call", "<u4"), ("seq", "<u4"), ("reserved", "<u8"), ("stats", "<f8", (int(n_strings), 2))])
    dt = np.dtype([("calls", "<u4"), ("recorded", "<u4"), ("ticket", "<u4"), ("reserved", "<u4", (5,)),
                   ("rows", row, (int(capacity),))])
    assert dt.itemsize == HEADER_BYTES + int(capacity) * (ROW_HEAD_BYTES + 16 * int(n_strings))
    return dt


def moments(n: int, total: float, sq: float, unbiased: bool = True) -> Dict[str, float]:
    """``mean``, ``var`` and ``std`` of a tensor of ``n`` elements with sum ``total`` and squared Frobenius norm ``sq``:
    the reference's formula (conv_sbs.py:197-207) in Python floats, in its operation order.  A negative ``var`` (the
    formula cancels) gives ``std = nan``, as ``tensor ** 0.5`` does there; so does n = 1 with ``unbiased``."""
    total, sq = float(total), float(sq)
    mean = total / n
    d = n - 1 if unbiased else n
    var = sq / d - 2 * total / d * mean + n / d * mean**2 if d != 0 else float("nan")
    std = var**0.5 if var >= 0.0 else float("nan")
    return {"mean": mean, "var": var, "std": std}


def reference_moments(cores: Sequence, bond_sizes: Optional[Sequence[int]] = None) -> Dict[str, float]:
    """``{"sum", "sq_norm"}`` of the tensor a string represents, in numpy float64: a mirror of the MATHEMATICS of
    csrc/tt_stats.hip (the products of the S_c and of the transfer matrices sum_{o,p} A (x) A, and their traces), not of
    its summation order.  ``cores``: arrays (or tensors) shaped (o, l, r, q, ..., q); ``bond_sizes``, if given, are checked
    against them (cyclically: core c sits between bond c and bond c + 1)."""
    mats = []
    for core in cores:
        a = core.detach().cpu().numpy() if isinstance(core, torch.Tensor) else np.asarray(core)
        mats.append(a.astype(np.float64).reshape(a.shape[0], a.shape[1], a.shape[2], -1))
    n = len(mats)
    for c, a in enumerate(mats):
        if a.shape[2] != mats[(c + 1) % n].shape[1]:
            raise ValueError(f"core {c} ends on bond {a.shape[2]}, core {(c + 1) % n} starts on {mats[(c + 1) % n].shape[1]}")
        if bond_sizes is not None and int(bond_sizes[c]) != a.shape[1]:
            raise ValueError(f"core {c} starts on bond {a.shape[1]}, bond_sizes says {int(bond_sizes[c])}")
    row = None    # S_0 ... S_c
    chain = None  # E_0 ... E_c, E_c[(a, a'), (b, b')] = sum_{o,p} A[a, b] A[a', b']
    for a in mats:
        o, l, r, p = a.shape
        s = a.sum(axis=(0, 3))
        flat = a.transpose(1, 2, 0, 3).reshape(l * r, o * p)
        e = (flat @ flat.T).reshape(l, r, l, r).transpose(0, 2, 1, 3).reshape(l * l, r * r)
        row = s if row is None else row @ s
        chain = e if chain is None else chain @ e
    return {"sum": float(np.trace(row)), "sq_norm": float(np.trace(chain))}


def _descriptor(string: ConvSBS) -> L.TTString:
    spec = string.spec
    n = len(spec)
    q, C = int(spec.in_quantum_dim_size), int(spec.in_num_channels)
    if n > MAX_CORES:
        raise NotImplementedError(f"TTStats: a string of {n} cores (at most {MAX_CORES})")
    if max(spec.bond_sizes) > MAX_BOND:
        raise NotImplementedError(f"TTStats: bond {max(spec.bond_sizes)} (at most {MAX_BOND})")
    if q**C > MAX_SLICES:
        raise NotImplementedError(f"TTStats: q ** C = {q ** C} input slices per core (at most {MAX_SLICES})")
    d = L.TTString()
    d.n_cores, d.C, d.q = n, C, q
    for c, shape in enumerate(spec.shapes):
        d.out_sizes[c], d.bond_sizes[c] = int(shape.out_quantum_dim_size), int(shape.bond_left_size)
    return d


class TTStats:
    """``strings``: `ConvSBS` modules (at most 16), ``names``: one per string (default "0", "1", ...).  Launch number c
    (counted on the device from 0) is recorded iff ``c % period == 0``; the block keeps the last ``capacity`` recorded
    rows.  The descriptors and the cores' addresses are taken ONCE, here: the cores' storage must stay where it is
    afterwards (the flat optimizers move the parameters into their flat buffer when they are built - build them first -
    and keep them there); ``record`` refuses cores that have moved."""

    def __init__(self, device, strings: Sequence[ConvSBS], names: Optional[Sequence[str]] = None, period: int = 1,
                 capacity: int = 64):
        strings = list(strings)
        names = tuple(str(i) for i in range(len(strings))) if names is None else tuple(str(n) for n in names)
        if not strings:
            raise ValueError("TTStats takes at least one string")
        if len(names) != len(strings) or len(set(names)) != len(names):
            raise ValueError(f"TTStats takes one name per string, each once; got {names!r} for {len(strings)} strings")
        if int(period) < 1 or int(capacity) < 1:
            raise ValueError(f"TTStats: period >= 1 and capacity >= 1, got {period} and {capacity}")
        if len(strings) > MAX_STRINGS:
            raise ValueError(f"TTStats takes at most {MAX_STRINGS} strings, got {len(strings)}")
        cores = [core for s in strings for core in s.cores]
        dtype = cores[0].dtype
        if any(c.dtype != dtype for c in cores):
            raise TypeError("TTStats: the cores of one object have one dtype")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"TTStats takes float32 or float64 cores, got {dtype}")
        descriptors = [_descriptor(s) for s in strings]
        dev = torch.device(device)
        if dev.type != "cuda":   # the project's boundary rule: there is no CPU implementation of a library call
            dev, _ = L.placement(torch.empty(0, device=dev))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        for c in cores:
            if c.device != dev:
                raise RuntimeError(f"TTStats reads the cores where they are: a core on {c.device}, the block on {dev}")
            if not c.is_contiguous():
                raise ValueError("TTStats reads contiguous cores")
        self.names, self.device, self.period, self.capacity = names, dev, int(period), int(capacity)
        self.strings, self.nelements = strings, [int(s.spec.nelement) for s in strings]
        self._cores = cores
        self._addresses = [c.data_ptr() for c in cores]
        self._descriptors = (L.TTString * len(strings))(*descriptors)
        self._pointers = L.ptr_array(cores)
        self._code = L.dtype_code(cores[0])
        lib = L.lib()
        self.dtype = block_dtype(len(strings), self.capacity)
        self.block_bytes = int(lib.dctn_tt_stats_block_bytes(len(strings), self.capacity))
        assert self.block_bytes == self.dtype.itemsize
        self.workspace_bytes = int(lib.dctn_tt_stats_workspace_bytes(self._descriptors, len(strings)))
        assert self.workspace_bytes >= 16
        self.block = torch.zeros(self.block_bytes, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self._seen = 0     # rows read so far, counted as the device counts `recorded`
        self.lost = 0      # rows overwritten before they were read

    @classmethod
    def for_model(cls, model: torch.nn.Module, period: int = 1, capacity: int = 64) -> "TTStats":
        """Every `ConvSBS` of ``model`` in ``named_modules()`` order, under those names - for `DCTNMnistModel` they are
        ``model.string_names()``."""
        found = [(name, m) for name, m in model.named_modules() if isinstance(m, ConvSBS)]
        if not found:
            raise ValueError("TTStats.for_model: the module holds no ConvSBS")
        return cls(found[0][1].cores[0].device, [m for _, m in found], [name for name, _ in found], period, capacity)

    def record(self) -> None:
        """Enqueues the one launch on the current stream of the block's device; reads nothing back."""
        if any(c.data_ptr() != a for c, a in zip(self._cores, self._addresses)):
            raise RuntimeError("TTStats.record: a core's storage has moved since the object was built; build it again")
        with torch.cuda.device(self.device):
            L.check(L.lib().dctn_tt_stats(self._pointers, self._descriptors, len(self.names), self.block.data_ptr(),
                                          self.capacity, self.period, self.workspace.data_ptr(), self.workspace_bytes,
                                          self._code, L.stream_ptr(self.device)), "TT statistics")

    def reset(self, calls: int = 0) -> None:
        """Zeroes header and rows on the current stream, between launches, and starts the count again at ``calls``; what
        was not read is dropped (``lost`` returns to 0).  `GraphedTrainStep`'s warm-up forwards count as calls: reset
        after building it."""
        if not 0 <= int(calls) < 1 << 32:
            raise ValueError(f"TTStats.reset: calls is a uint32, got {calls}")
        self.block.zero_()
        if int(calls):
            word = torch.from_numpy(np.array([int(calls)], dtype="<u4").view(np.uint8).copy())
            self.block[:4].copy_(word.to(self.device))
        self._seen, self.lost = 0, 0

    def raw(self) -> np.ndarray:
        """The block as it is on the device (one structured element, `block_dtype`); synchronises."""
        return self.block.cpu().numpy().view(self.dtype)[0].copy()

    def read(self) -> List[dict]:
        """The rows not yet read, oldest first: ``{"call", "seq", "stats"}`` with ``stats[name] = {sum, sq_norm, mean, var,
        std}`` (`moments` of the string's element count).  Rows overwritten before this read are counted in ``lost``.
        Synchronises."""
        raw = self.raw()
        recorded = int(raw["recorded"])
        first = max(self._seen, recorded - self.capacity)
        self.lost += first - self._seen
        out = []
        for seq in range(first, recorded):
            row = raw["rows"][seq % self.capacity]
            assert int(row["seq"]) == seq, (int(row["seq"]), seq)
            stats = {}
            for name, n, (total, sq) in zip(self.names, self.nelements, row["stats"]):
                stats[name] = dict(moments(n, float(total), float(sq)), sum=float(total), sq_norm=float(sq))
            out.append({"call": int(row["call"]), "seq": seq, "stats": stats})
        self._seen = recorded
        return out


Sink = Callable[[str, float, int], None]


class TTStatsLogger:
    """Hook for `training.train_graphed`: every ``every`` calls (launches) it reads the unread rows - the one
    synchronisation it makes - and reports each as the reference does: ``sink("mean_of_tt_tensor/" + name, mean, iteration)``
    and ``sink("std_of_tt_tensor/" + name, std, iteration)`` with ``iteration = first_iter + call`` (``add_scalar``'s
    argument order)."""

    def __init__(self, tt, every: int, sink: Sink, first_iter: int = 0):
        assert every >= 1
        self.tt, self.every, self.sink, self.first_iter = tt, int(every), sink, int(first_iter)
        self._calls = 0

    def __call__(self, st_x, st_it) -> None:
        self._calls += 1
        if self._calls % self.every == 0:
            self.flush()

    def flush(self) -> None:
        """Reads and reports now (call it when the loop ends, for the launches after the last multiple)."""
        for entry in self.tt.read():
            iteration = self.first_iter + int(entry["call"])
            for name, st in entry["stats"].items():
                self.sink("mean_of_tt_tensor/" + name, st["mean"], iteration)
                self.sink("std_of_tt_tensor/" + name, st["std"], iteration)

