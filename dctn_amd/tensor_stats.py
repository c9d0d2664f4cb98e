"""Output statistics of several tensors in one launch, in one fixed order (`dctn_tensor_stats`, csrc/sbs_tail.hip).

The reference's runner logs mean, std, mean |y|, min |y| and max |y| of every ConvSBS string's output every 20
iterations through forward hooks (mnist.py:537-553), and its calibration reads ``tensor.std().item()`` once per string
(mnist.py:273).  No hook runs inside a captured training step, and a host read per string is a synchronisation per
string.  `OutputStats` keeps one 64-byte record per named tensor on the device: ``record`` only enqueues a launch (it is
capturable, and a replay advances the records' ``seq``), ``read`` is the one place that synchronises.  The sums are
float64 and are added in an order that depends on the element counts alone, so the same values give the same record on
every launch, device and rank - which is what lets ranks sum their ``(n, sum, sum of squares)`` triples and scale by the
standard deviation of the union of their shards (`combine_moments`, `std_from_moments`).
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

MAX_TENSORS_PER_LAUNCH = 8
RECORD_BYTES = 64
# the record of include/dctn_amd.h
RECORD_DTYPE = np.dtype([("n", "<i8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("sum_abs", "<f8"), ("min_abs", "<f4"),
                         ("max_abs", "<f4"), ("nonfinite", "<u4"), ("seq", "<u4"), ("ticket", "<u4"), ("reserved", "<u4", (3,))])
assert RECORD_DTYPE.itemsize == RECORD_BYTES

Moments = Tuple[float, float, float]   # (n, sum, sum of squares) in float64


def std_from_moments(n: float, s: float, ss: float, unbiased: bool = True) -> float:
    """Standard deviation from ``(n, sum, sum of squares)`` in float64: sqrt((ss - s^2 / n) / (n - 1)).  NaN where torch's
    ``std`` is (fewer than two elements); a variance that rounding made negative counts as 0."""
    n, s, ss = float(n), float(s), float(ss)
    divisor = n - 1.0 if unbiased else n
    if n < 1.0 or divisor <= 0.0:
        return float("nan")
    var = (ss - s * s / n) / divisor
    return math.sqrt(var) if var > 0.0 else (0.0 if var == var else float("nan"))


def combine_moments(parts: Sequence[Moments]) -> Moments:
    """The triple of the union of several disjoint shards: the three sums, added in the order given."""
    n = s = ss = 0.0
    for pn, ps, pss in parts:
        n, s, ss = n + float(pn), s + float(ps), ss + float(pss)
    return n, s, ss


class OutputStats:
    """``names``: one name per tensor that every ``record`` call will be given, in that order."""

    def __init__(self, device, names: Sequence[str]):
        names = tuple(str(n) for n in names)
        if not names or len(set(names)) != len(names):
            raise ValueError(f"OutputStats takes at least one name, each once; got {names!r}")
        dev = torch.device(device)
        if dev.type != "cuda":   # the project's boundary rule: a CPU caller is served by the current GPU, or not at all
            dev, _ = L.placement(torch.empty(0, device=dev))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        lib = L.lib()
        assert lib.dctn_tensor_stats_record_bytes() == RECORD_BYTES
        self.names, self.device = names, dev
        self.records = torch.zeros(len(names) * RECORD_BYTES, dtype=torch.uint8, device=dev)
        self._ws_bytes = lib.dctn_tensor_stats_workspace_bytes(min(len(names), MAX_TENSORS_PER_LAUNCH))
        self.workspace = torch.empty(self._ws_bytes, dtype=torch.uint8, device=dev)   # launches on one stream share it
        # (first tensor, number of tensors, pointer to the chunk's records) of every launch, built once
        self._chunks = [(k, min(MAX_TENSORS_PER_LAUNCH, len(names) - k), self.records.data_ptr() + k * RECORD_BYTES)
                        for k in range(0, len(names), MAX_TENSORS_PER_LAUNCH)]
        self._ws_ptr = self.workspace.data_ptr()

    def record(self, tensors: Sequence[Tensor]) -> None:
        """Enqueues ceil(len / 8) launches on the current stream of the records' device; reads nothing back."""
        tensors = list(tensors)
        if len(tensors) != len(self.names):
            raise ValueError(f"OutputStats.record: {len(self.names)} tensors ({', '.join(self.names)}), got {len(tensors)}")
        dtype = tensors[0].dtype
        if any(t.dtype != dtype for t in tensors):
            raise TypeError("OutputStats.record: the tensors of one call have one dtype")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"OutputStats.record takes float32 or float64 tensors, got {dtype}")
        _, staged = L.placement(*tensors)
        held = [t.detach().to(self.device) if staged else t.detach() for t in tensors]
        L.require_device(self.records, *held)
        held = [t if t.is_contiguous() else t.contiguous() for t in held]
        lib, code = L.lib(), L.dtype_code(held[0])
        with torch.cuda.device(self.device):
            stream = L.stream_ptr(self.device)
            for first, count, rec_ptr in self._chunks:
                part = held[first : first + count]
                L.check(lib.dctn_tensor_stats(L.ptr_array(part), L.i64_array([t.numel() for t in part]), count, rec_ptr,
                                              self._ws_ptr, self._ws_bytes, code, stream), "tensor statistics")

    def raw(self) -> np.ndarray:
        """The records as they are on the device (structured array, `RECORD_DTYPE`); synchronises."""
        return self.records.cpu().numpy().view(RECORD_DTYPE).copy()

    def read(self) -> Dict[str, dict]:
        """Per name: n, mean, std (unbiased), mean_abs, min_abs, max_abs, nonfinite, seq.  The moments run over the finite
        elements; ``n`` counts all of them.  Synchronises."""
        out = {}
        for name, r in zip(self.names, self.raw()):
            n, bad = int(r["n"]), int(r["nonfinite"])
            finite = n - bad
            s, ss = float(r["sum"]), float(r["sum_sq"])
            out[name] = {
                "n": n, "mean": s / finite if finite > 0 else float("nan"), "std": std_from_moments(finite, s, ss),
                "mean_abs": float(r["sum_abs"]) / finite if finite > 0 else float("nan"), "min_abs": float(r["min_abs"]),
                "max_abs": float(r["max_abs"]), "nonfinite": bad, "seq": int(r["seq"]),
            }
        return out

    def moments(self) -> List[Moments]:
        """``(n, sum, sum of squares)`` per name in float64, over the finite elements.  Synchronises."""
        return [(float(int(r["n"]) - int(r["nonfinite"])), float(r["sum"]), float(r["sum_sq"])) for r in self.raw()]
