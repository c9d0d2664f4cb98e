"""Host side of the step trace (no GPU): the exports and sizes of `dctn_step_trace_*`, the slot arithmetic of
`training.StepTrace.decode` on hand-built bytes, and the argument errors of `GraphedTrainStep(iters_per_launch=...)` that
are decided before any GPU call."""
import ctypes
import os
import re

import numpy as np
import pytest

from dctn_amd import _lib
from dctn_amd.training import GraphedTrainStep, StepTrace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dctn_step_trace_head_bytes", "dctn_step_trace_record_bytes", "dctn_step_trace_record")


def test_the_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    declared = set(re.findall(r"\b(dctn_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/dctn_amd.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        assert hasattr(handle, name), f"{name} not exported by {_lib.LIB_PATH}"
    c_void, c_int, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib.SIGNATURES["dctn_step_trace_record"] == (c_int, [c_void] * 9 + [c_int, c_i64, c_int, c_int, c_void])
    lib = _lib.lib()
    assert lib.dctn_step_trace_head_bytes() == 16 and lib.dctn_step_trace_record_bytes() == 64
    assert lib.dctn_version() >= 509
    assert StepTrace.RECORD.itemsize == 64
    assert [StepTrace.RECORD.fields[n][1] for n in StepTrace.RECORD.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52]
    flags = {name: int(value) for name, value in re.findall(r"#define\s+DCTN_TRACE_HAS_([A-Z]+)\s+(\d+)", header)}
    assert flags == {k.upper(): v for k, v in StepTrace.PRESENT.items()} == {"REG": 1, "GUARD": 2, "ADAM": 4, "SOURCE": 8}


def test_bad_arguments_return_their_codes_before_any_launch():
    """Validation happens on the host, so it is checkable here (the pointers are never followed)."""
    rec = _lib.lib().dctn_step_trace_record
    ok = dict(logits=64, labels=64, loss=64, reg=None, guard=None, adam=None, batch=None, head=64, ring=64, capacity=3,
              B=4, C=2, dtype=_lib.F32)

    def call(**change):
        a = dict(ok, **change)
        return rec(a["logits"], a["labels"], a["loss"], a["reg"], a["guard"], a["adam"], a["batch"], a["head"], a["ring"],
                   a["capacity"], a["B"], a["C"], a["dtype"], None)

    for name in ("logits", "labels", "loss", "head", "ring"):
        assert call(**{name: None}) == _lib.ERR_NULL, name
    for change in (dict(B=0), dict(C=0), dict(capacity=0), dict(B=-1), dict(capacity=-5)):
        assert call(**change) == _lib.ERR_BAD_SHAPE, change
    assert call(dtype=_lib.F64) == _lib.ERR_BAD_DTYPE and call(dtype=9) == _lib.ERR_BAD_DTYPE
    assert call(logits=None, B=0, dtype=9) == _lib.ERR_NULL   # in this order, as the neighbouring entry points


# ------------------------------------------------------------------ decode
def _bytes(capacity, done, stale=0xEE):
    """Head and ring as `done` launches leave them: record s in slot s % capacity, later ones over earlier ones; slots never
    written hold `stale` bytes.  Every record carries fields that name its seq."""
    ring = np.frombuffer(bytes([stale]) * (64 * capacity), dtype=StepTrace.RECORD).copy()
    for s in range(done):
        r = np.zeros((), dtype=StepTrace.RECORD)
        r["seq"], r["present"], r["loss"], r["rows"], r["correct"] = s, 15, 0.5 * s, 8, s % 9
        r["opt_steps_done"], r["batches_done"], r["bad_step"] = s + 1, s + 1, -1
        ring[s % capacity] = r
    head = np.array([done, 0, 0, 0], dtype="<u4")
    return head.tobytes(), ring.tobytes()


@pytest.mark.parametrize("capacity", [1, 3, 4])
@pytest.mark.parametrize("done", [0, 2, 4, 11])
def test_decode_returns_the_unread_window_and_counts_the_lost(capacity, done):
    head, ring = _bytes(capacity, done)
    start = max(0, done - capacity)                      # the ring holds seq in [start, done)
    # last_read before the window, at its start, inside it, at its end, and past it
    for last_read in sorted({0, max(0, start - 1), start, start + 1, max(start, done - 1), done, done + 1, done + 7}):
        records, lost, new_done = StepTrace.decode(head, ring, capacity, last_read)
        want = list(range(max(start, last_read), done))
        assert new_done == done
        assert records.dtype == StepTrace.RECORD and records["seq"].tolist() == want, (capacity, done, last_read)
        assert lost == max(0, start - last_read), (capacity, done, last_read)
        assert records["opt_steps_done"].tolist() == [s + 1 for s in want]
        assert records["loss"].tolist() == [0.5 * s for s in want] and records["bad_step"].tolist() == [-1] * len(want)


def test_decode_follows_the_slot_order_of_a_capacity_that_is_no_power_of_two():
    head, ring = _bytes(3, 11)
    assert np.frombuffer(ring, dtype=StepTrace.RECORD)["seq"].tolist() == [9, 10, 8]   # slots 0, 1, 2
    records, lost, done = StepTrace.decode(head, ring, 3, 0)
    assert records["seq"].tolist() == [8, 9, 10] and lost == 8 and done == 11
    records, lost, _ = StepTrace.decode(head, ring, 3, 9)
    assert records["seq"].tolist() == [9, 10] and lost == 0
    # reading twice: the second read of the same bytes returns nothing and loses nothing
    records, lost, _ = StepTrace.decode(head, ring, 3, done)
    assert records.size == 0 and lost == 0


def test_decode_refuses_bytes_that_do_not_fit_and_rings_that_disagree_with_the_head():
    head, ring = _bytes(3, 5)
    with pytest.raises(ValueError):
        StepTrace.decode(head, ring, 4, 0)          # 3 records are not a ring of 4
    with pytest.raises(ValueError):
        StepTrace.decode(head[:8], ring, 3, 0)
    with pytest.raises(ValueError):
        StepTrace.decode(head, ring, 0, 0)
    with pytest.raises(ValueError):
        StepTrace.decode(head, ring, 3, -1)
    newer = np.array([6, 0, 0, 0], dtype="<u4").tobytes()   # a head read later than the ring
    with pytest.raises(RuntimeError, match="one point of the stream"):
        StepTrace.decode(newer, ring, 3, 0)


# ------------------------------------------------------------------ argument errors of GraphedTrainStep
def test_more_than_one_iteration_per_launch_needs_a_batch_source():
    """Raised before the model, the example batch or the device are touched: nothing here exists."""
    with pytest.raises(ValueError, match="batch_source"):
        GraphedTrainStep(None, None, None, None, None, iters_per_launch=3)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="iters_per_launch"):
            GraphedTrainStep(None, None, None, None, None, iters_per_launch=bad)


def test_more_than_one_iteration_per_launch_refuses_the_split_all_reduce():
    class Reducer:   # what the constructor looks at
        world, skip_single_rank = 2, True

    with pytest.raises(ValueError, match="graph_allreduce"):
        GraphedTrainStep(None, None, None, None, None, reducer=Reducer(), graph_allreduce=False, batch_source=object(),
                         iters_per_launch=3)
