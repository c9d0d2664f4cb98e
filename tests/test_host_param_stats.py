"""What the parameter monitor promises without a GPU: the exports of library version 521 with the block's layout, every
pinned return code (all decided on the host before any launch), the workspace rule of the header evaluated in Python,
the pure ring logic `decode` and the pure `cell_moments`, the logger's tags, and what `ParamStats` and the flat
optimizers refuse.  The blocks live in CPU tensors and nothing is launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from dctn_amd import _lib, training
from dctn_amd.param_stats import (CELL, CELL_BYTES, HEADER_BYTES, ROW_HEAD_BYTES, ParamStats, block_dtype, cell_moments, decode,
                                  workspace_bytes)

PTR = 4096   # any non-null, 16-byte aligned number: the calls below return before they would use it


def _ends(*sizes):
    return _lib.i64_array(np.cumsum(sizes).tolist())


# ------------------------------------------------------------------ the library's interface
def test_exports_version_and_block_layout():
    lib = _lib.lib()
    assert lib.dctn_version() >= 521
    for name in ("dctn_param_stats", "dctn_param_stats_block_bytes", "dctn_param_stats_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    size = lib.dctn_param_stats_block_bytes
    for n, cap in ((1, 1), (45, 64), (64, 2), (7, 1000)):
        dt = block_dtype(n, cap)
        assert size(n, cap) == dt.itemsize == 32 + cap * (16 + 64 * n) == HEADER_BYTES + cap * (ROW_HEAD_BYTES + CELL_BYTES * n)
        assert dt.fields["rows"][1] == HEADER_BYTES and dt["rows"].shape == (cap,)
        row = dt["rows"].base
        assert [row.fields[k][1] for k in ("call", "seq", "reserved", "cells")] == [0, 4, 8, 16] and row["cells"].shape == (n,)
    assert [block_dtype(1, 1).fields[k][1] for k in ("calls", "recorded", "ticket", "reserved")] == [0, 4, 8, 12]
    assert [CELL.fields[k][1] for k in ("w_sum", "w_sum_sq", "w_max_abs", "w_nonfinite", "g_sum", "g_sum_sq", "g_max_abs",
                                        "g_nonfinite")] == list(range(0, 64, 8))
    assert size(0, 4) == size(65, 4) == size(3, 0) == size(-1, -1) == 0


def test_return_codes_in_the_projects_order():
    lib = _lib.lib()

    def call(params=PTR, master=None, grads=PTR, ends=(5, 64, 130), n=None, block=PTR, capacity=4, period=1, ws=PTR,
             ws_bytes=1 << 20, dtype=_lib.F32):
        arr = None if ends is None else _lib.i64_array(list(ends))
        n = (0 if ends is None else len(ends)) if n is None else n
        return lib.dctn_param_stats(params, master, grads, arr, n, block, capacity, period, ws, ws_bytes, dtype, None)

    # (the good call itself would launch: it is never made)
    # NULL first, whatever else is wrong
    assert call(params=None) == call(grads=None) == call(ends=None, n=3) == call(block=None) == _lib.ERR_NULL
    assert call(params=None, n=0) == call(block=None, dtype=9) == call(grads=None, capacity=0) == _lib.ERR_NULL
    # shapes
    assert call(n=0) == call(n=-1) == _lib.ERR_BAD_SHAPE
    assert call(ends=(5, 5, 130)) == call(ends=(5, 4, 130)) == call(ends=(0, 4)) == call(ends=(-3, 4)) == _lib.ERR_BAD_SHAPE
    assert call(capacity=0) == call(period=0) == call(period=-20) == _lib.ERR_BAD_SHAPE
    assert call(ends=(5, 5), dtype=9) == call(capacity=0, dtype=9) == _lib.ERR_BAD_SHAPE   # shape before dtype
    # dtype
    assert call(dtype=3) == call(dtype=7) == call(dtype=-1) == _lib.ERR_BAD_DTYPE
    many = tuple(range(1, 66))
    big = (5, 5 + (1 << 31))
    assert call(ends=many, dtype=9) == call(ends=big, dtype=9) == _lib.ERR_BAD_DTYPE   # dtype before the limits
    # unsupported: the limits, alignment, a master copy of anything but bf16
    assert call(ends=many) == call(ends=big) == _lib.ERR_UNSUPPORTED
    assert call(ends=(5, 4 + (1 << 31)), ws_bytes=0) == _lib.ERR_WORKSPACE   # 2^31 - 1 elements are fine
    assert call(ends=tuple(range(1, 65)), ws_bytes=0) == _lib.ERR_WORKSPACE  # so are 64 segments
    assert call(params=PTR + 2) == call(grads=PTR + 2) == call(block=PTR + 4) == call(ws=PTR + 4) == _lib.ERR_UNSUPPORTED
    assert call(params=PTR + 4, dtype=_lib.F64) == call(grads=PTR + 4, dtype=_lib.F64) == _lib.ERR_UNSUPPORTED
    assert call(params=PTR + 1, dtype=_lib.BF16) == call(master=PTR + 2, dtype=_lib.BF16) == _lib.ERR_UNSUPPORTED
    assert call(master=PTR) == call(master=PTR, dtype=_lib.F64) == _lib.ERR_UNSUPPORTED
    assert call(master=PTR, ws_bytes=0) == _lib.ERR_UNSUPPORTED   # before the workspace's size
    # each element size's own alignment is enough
    assert call(params=PTR + 4, grads=PTR + 12, ws_bytes=0) == _lib.ERR_WORKSPACE
    assert call(params=PTR + 2, grads=PTR + 6, master=PTR + 4, dtype=_lib.BF16, ws_bytes=0) == _lib.ERR_WORKSPACE
    # the workspace comes last: three segments of one workgroup each
    assert call(ws=None) == call(ws_bytes=0) == call(ws_bytes=191) == _lib.ERR_WORKSPACE
    assert call(ws_bytes=191, block=PTR + 4) == _lib.ERR_UNSUPPORTED


def test_workspace_bytes_follow_the_headers_rule():
    """64 bytes per workgroup, min(64, ceil(c / 8192)) workgroups per segment of c elements - evaluated here."""
    need = _lib.lib().dctn_param_stats_workspace_bytes
    rng = np.random.default_rng(0)
    cases = [(1,), (8192,), (8193,), (64 * 8192,), (64 * 8192 + 1,), (63 * 8192 + 1,), ((1 << 31) - 1,),
             (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 64 * 8192 + 1), tuple([1] * 64),
             tuple(int(s) for s in rng.integers(1, 1 << 21, size=64))]
    for sizes in cases:
        want = 64 * sum(min(64, -(-c // 8192)) for c in sizes)
        assert need(_ends(*sizes), len(sizes)) == want == workspace_bytes(np.cumsum(sizes).tolist()), sizes
    assert need(_ends(8192), 1) == 64 and need(_ends(8193), 1) == 128 and need(_ends(1 << 30), 1) == 64 * 64
    assert need(None, 2) == need(_ends(3, 4), 0) == need(_ends(*([1] * 65)), 65) == 0
    assert need(_lib.i64_array([4, 4]), 2) == need(_lib.i64_array([0, 4]), 2) == need(_lib.i64_array([5, 5 + (1 << 31)]), 2) == 0


# ------------------------------------------------------------------ the ring
def _block(n_segments, capacity, recorded, period=1):
    """A block as `recorded` recorded launches of period `period` leave it: row seq holds w_sum = seq in every cell."""
    raw = np.zeros((), dtype=block_dtype(n_segments, capacity))
    raw["recorded"], raw["calls"] = recorded, (recorded - 1) * period + 1 if recorded else 0
    for seq in range(recorded):   # later rows overwrite earlier ones, as on the device
        row = raw["rows"][seq % capacity]
        row["call"], row["seq"] = seq * period, seq
        row["cells"]["w_sum"] = float(seq)
    return raw


def test_decode_wraps_counts_the_lost_rows_and_reads_nothing_twice():
    rows, lost = decode(_block(2, 4, 0), 0, 4)
    assert rows == [] and lost == 0
    rows, lost = decode(_block(2, 4, 3, period=5), 0, 4)
    assert [(int(r["call"]), int(r["seq"])) for r in rows] == [(0, 0), (5, 1), (10, 2)] and lost == 0
    rows, lost = decode(_block(2, 4, 3), 3, 4)   # again: nothing new
    assert rows == [] and lost == 0
    rows, lost = decode(_block(2, 4, 4), 3, 4)   # exactly full
    assert [int(r["seq"]) for r in rows] == [3] and lost == 0
    rows, lost = decode(_block(2, 4, 11), 3, 4)  # wrapped: 3 .. 6 were overwritten
    assert [int(r["seq"]) for r in rows] == [7, 8, 9, 10] and lost == 4
    assert [float(r["cells"]["w_sum"][1]) for r in rows] == [7.0, 8.0, 9.0, 10.0]
    rows, lost = decode(_block(1, 1, 6), 0, 1)   # a ring of one row
    assert [int(r["seq"]) for r in rows] == [5] and lost == 5
    torn = _block(2, 4, 6)
    torn["rows"][1]["seq"] = 1   # a row the device has not finished
    with pytest.raises(AssertionError):
        decode(torn, 0, 4)


def test_read_on_a_cpu_block_follows_decode():
    ps = ParamStats("cpu", ["a", "b.c"], period=5, capacity=4)
    with pytest.raises(RuntimeError):
        ps.read()
    ps.bind([3, 10])
    assert ps.ends == [3, 13] and ps.sizes == [3, 10] and ps.workspace_bytes == 128
    ps.block.copy_(torch.from_numpy(_block(2, 4, 6, period=5).reshape(1).view(np.uint8)))
    rows = ps.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(10, 2), (15, 3), (20, 4), (25, 5)] and ps.lost == 2
    assert list(rows[0]["stats"]) == ["a", "b.c"] and rows[3]["stats"]["b.c"]["weights"]["mean"] == 0.5
    assert ps.read() == [] and ps.lost == 2
    assert ps.run_regions()[0][0] == "param_stats" and ps.run_regions()[0][1] is ps.block
    host = ps.run_host()
    assert host == dict(names=["a", "b.c"], period=5, capacity=4, seen=6, lost=2)
    other = ParamStats("cpu", ["a", "b.c"], period=5, capacity=4)
    other.run_restored(host, {"param_stats": None})
    assert (other._seen, other.lost) == (6, 2)
    with pytest.raises(ValueError):
        ParamStats("cpu", ["a", "z"]).run_restored(host, {"param_stats": None})
    ps.reset(calls=7)
    raw = ps.raw()
    assert (int(raw["calls"]), int(raw["recorded"])) == (7, 0) and not raw["rows"].tobytes().strip(b"\0") and ps.lost == 0


# ------------------------------------------------------------------ the moments
def test_cell_moments_against_numpy():
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 4099):
        w, g = rng.normal(0.3, 2.0, size=n), rng.normal(size=n) * 1e-3
        cell = np.zeros((), dtype=CELL)
        for prefix, x in (("w_", w), ("g_", g)):
            cell[prefix + "sum"], cell[prefix + "sum_sq"] = x.sum(), (x * x).sum()
            cell[prefix + "max_abs"], cell[prefix + "nonfinite"] = np.abs(x).max(), 0
        got = cell_moments(n, cell)
        assert set(got) == {"weights", "grads"}
        for key, x in (("weights", w), ("grads", g)):
            st = got[key]
            assert set(st) == {"n", "sum", "sum_sq", "max_abs", "nonfinite", "norm", "mean", "std"}
            assert all(type(v) is float for v in st.values())
            assert st["n"] == n and st["sum"] == x.sum() and st["sum_sq"] == (x * x).sum() and st["max_abs"] == np.abs(x).max()
            assert st["norm"] == math.sqrt((x * x).sum()) and st["mean"] == x.sum() / n
            assert abs(st["norm"] - np.linalg.norm(x)) <= 1e-12 * np.linalg.norm(x)
            assert abs(st["mean"] - x.mean()) <= 1e-12 * abs(x).mean()
            assert abs(st["std"] - x.std()) <= 1e-9 * max(x.std(), abs(x).mean())   # numpy's default: the population std
    # a constant segment: the difference cancels, and is clamped at 0
    cell = np.zeros((), dtype=CELL)
    cell["w_sum"], cell["w_sum_sq"], cell["w_nonfinite"] = 3.0, 3.0 - 2.0 ** -50, 2   # sum_sq / n - mean^2 < 0
    st = cell_moments(3, cell)["weights"]
    assert st["std"] == 0.0 and st["nonfinite"] == 2.0 and cell_moments(3, cell)["grads"]["norm"] == 0.0


# ------------------------------------------------------------------ the logger
class _FakePS:
    """What the logger needs of a `ParamStats`: read()."""

    def __init__(self, batches):
        self.batches, self.reads = list(batches), 0

    def read(self):
        self.reads += 1
        return self.batches.pop(0) if self.batches else []


def _entry(call, seq, **norms):
    return {"call": call, "seq": seq, "stats": {name.replace("__", "."): {"weights": {"norm": w}, "grads": {"norm": g}}
                                                 for name, (w, g) in norms.items()}}


def test_the_logger_reports_two_tags_per_parameter_and_row():
    ps = _FakePS([[_entry(0, 0, layers__0__cores__3=(1.5, 0.25), bias=(2.0, 0.5)), _entry(1, 1, layers__0__cores__3=(2.5, 0.125), bias=(3.0, 1.0))],
                  [_entry(7, 2, layers__0__cores__3=(0.25, 4.0), bias=(4.0, 8.0))], []])
    seen = []
    hook = training.make_param_stats_logger(ps, 3, lambda tag, value, it: seen.append((tag, value, it)), first_iter=100)
    for launch in range(7):
        hook({}, {"num_iters_done": 100 + 8 * launch + 7})
    assert ps.reads == 2   # launches 3 and 6
    assert seen == [("weights_norm/layers/0/cores/3", 1.5, 100), ("grads_norm/layers/0/cores/3", 0.25, 100),
                    ("weights_norm/bias", 2.0, 100), ("grads_norm/bias", 0.5, 100),
                    ("weights_norm/layers/0/cores/3", 2.5, 101), ("grads_norm/layers/0/cores/3", 0.125, 101),
                    ("weights_norm/bias", 3.0, 101), ("grads_norm/bias", 1.0, 101),
                    ("weights_norm/layers/0/cores/3", 0.25, 107), ("grads_norm/layers/0/cores/3", 4.0, 107),
                    ("weights_norm/bias", 4.0, 107), ("grads_norm/bias", 8.0, 107)]
    hook.flush()
    assert ps.reads == 3 and len(seen) == 12   # nothing new: nothing reported
    named = training.make_param_stats_logger(_FakePS([[_entry(5, 0, a__b=(1.0, 2.0))]]), 1, lambda *a: seen.append(a),
                                             weight_tag="w", grad_tag="g")
    named({}, {})
    assert seen[-2:] == [("w/a/b", 1.0, 5), ("g/a/b", 2.0, 5)]


# ------------------------------------------------------------------ the host object and the optimizers
def test_param_stats_checks_its_names():
    for bad in (dict(names=[]), dict(names=["x", "x"]), dict(names=["x"], period=0), dict(names=["x"], capacity=0)):
        with pytest.raises(ValueError):
            ParamStats("cpu", **bad)
    with pytest.raises(NotImplementedError):
        ParamStats("cpu", [str(i) for i in range(65)])
    assert ParamStats("cpu", [str(i) for i in range(64)]).block_bytes == 32 + 64 * (16 + 64 * 64)
    ps = ParamStats("cpu", ["a", "b"])
    for sizes in ([3], [3, 4, 5], [3, 0]):
        with pytest.raises(ValueError):
            ps.bind(sizes)
    with pytest.raises(NotImplementedError):
        ps.bind([3, 1 << 31])
    with pytest.raises(RuntimeError):
        ps.record(torch.zeros(3), None, torch.zeros(3))   # no segments yet
    ps.bind([1, 2])
    with pytest.raises(RuntimeError):
        ps.record(torch.zeros(3), None, torch.zeros(3))   # there is no CPU form of the launch

    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    params = [model[1].bias, model[0].weight, model[1].weight, model[0].bias]
    assert ParamStats.for_parameters(model, params).names == ("1.bias", "0.weight", "1.weight", "0.bias")
    with pytest.raises(ValueError):
        ParamStats.for_parameters(model, params + [torch.nn.Parameter(torch.zeros(2))])
    with pytest.raises(ValueError):
        ParamStats.for_parameters(model, [])


def _adam(regularised, others=(), **kw):
    """A FlatAdam on the CPU: with a schedule, whose rate needs no device write at construction."""
    kw.setdefault("schedule", training.LRSchedule.constant("cpu", 1e-3))
    return training.FlatAdam(regularised, others, **kw)


def test_the_optimizers_take_one_name_per_parameter():
    def params(k=3):
        return [torch.nn.Parameter(torch.full((s,), 0.5)) for s in (5, 64, 130)[:k]]

    for names in (["a", "b"], ["a", "b", "c", "d"]):
        with pytest.raises(ValueError):
            _adam(params(), param_stats=ParamStats("cpu", names))
    with pytest.raises(TypeError):
        _adam(params(), param_stats=object())
    with pytest.raises(TypeError):
        training.FlatAdam(params(), (), 1e-3, (0.9, 0.999), 1e-8, 0.0, 0.0, False, None, None, None, None, None, None)   # keyword-only
    with pytest.raises(NotImplementedError):
        _adam([torch.nn.Parameter(torch.zeros(1)) for _ in range(65)], param_stats=ParamStats("cpu", ["a"]))
    import inspect

    # the option is taken by the constructor CALL of all three, keyword-only, and the __init__ lists stay as they were
    for cls in (training.FlatAdam, training.FlatSGD, training.FlatRMSprop):
        arg = inspect.signature(type(cls).__call__).parameters["param_stats"]
        assert arg.kind is inspect.Parameter.KEYWORD_ONLY and arg.default is None
        assert "param_stats" not in inspect.signature(cls.__init__).parameters
    for cls in (training.FlatSGD, training.FlatRMSprop):
        monitor = ParamStats("cpu", ["a", "b", "c"])
        assert cls(params(), param_stats=monitor).param_stats is monitor and monitor.sizes == [5, 64, 130]
        assert cls(params()).param_stats is None
        with pytest.raises(ValueError):
            cls(params(), param_stats=ParamStats("cpu", ["a"]))
    p = params()
    ps = ParamStats("cpu", ["a", "b", "c"])
    opt = _adam(p[:2], p[2:], param_stats=ps)
    assert opt.param_stats is ps and ps.ends == [5, 69, 199] and ps.workspace_bytes == 3 * 64
    # a run part behind sq_sum, and only with a monitor
    names = [name for name, _ in opt.run_regions()]
    plain = [name for name, _ in _adam(params()).run_regions()]
    assert names == plain + ["param_stats"] and plain[-1] == "sq_sum"
    assert opt.run_host()["param_stats"] == ps.run_host() and "param_stats" not in _adam(params()).run_host()
