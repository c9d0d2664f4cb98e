"""What the batch monitor promises without a GPU: the exports of library version 522 with the block's layout, every pinned
return code (all decided on the host before any launch), the pure ring logic `decode` on hand-built blocks, the default
table, the numpy `mirror` against independent formulations (torch.softmax, numpy.histogram, RankOneTensorsBatch,
torch.std), the logger's tags and iteration numbers, and what `BatchMonitor` and the steps refuse.  The blocks live in
CPU tensors and nothing is launched."""
import ctypes

import numpy as np
import pytest
import torch

from dctn_amd import _lib, tensor_hist, training
from dctn_amd.align import make_windows
from dctn_amd.batch_monitor import (HEADER_BYTES, ROW_HEAD_BYTES, SLOT_BYTES, TAGS, BatchMonitor, block_dtype, decode,
                                    histogram_summary, mirror, probability_edges, row_dtype, summarise)

PTR = 4096   # any non-null, 16-byte aligned number: the calls below return before they would use it


# ------------------------------------------------------------------ the library's interface
def test_exports_version_and_block_layout():
    lib = _lib.lib()
    assert lib.dctn_version() >= 522
    for name in ("dctn_batch_monitor", "dctn_batch_monitor_block_bytes", "dctn_batch_monitor_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    size = lib.dctn_batch_monitor_block_bytes
    for B, n_edges, cap in ((1, 2, 1), (3, 292, 16), (130, 292, 2), (128, 1549, 3), (7, 2048, 1), (5, 3, 4), (1024, 293, 64)):
        dt = block_dtype(B, n_edges, cap)
        row = ROW_HEAD_BYTES + 8 * (n_edges // 2) + 24 * B
        assert size(B, n_edges, cap) == dt.itemsize == HEADER_BYTES + cap * row
        assert dt.fields["rows"][1] == HEADER_BYTES and dt["rows"].shape == (cap,)
        r = dt["rows"].base
        assert r == row_dtype(B, n_edges) and r.itemsize == row
        assert [r.fields[k][1] for k in ("call", "seq", "rows", "correct", "bad_rows", "z_nonfinite", "x_nonfinite")] == [
            0, 4, 8, 12, 16, 20, 24]
        assert [r.fields[k][1] for k in ("x_sum", "x_sum_sq", "win_sum", "win_sq", "z_sum", "z_sum_sq", "z_min", "z_max")] == list(
            range(32, 96, 8))
        assert [r.fields[k][1] for k in ("below", "above", "nan", "reserved", "counts")] == [96, 100, 104, 108, 112]
        after = 112 + 8 * (n_edges // 2)
        assert [r.fields[k][1] for k in ("label", "index", "p_true", "pred")] == [after, after + 8 * B, after + 16 * B, after + 20 * B]
        assert r["counts"].shape == (n_edges - 1,) and r["p_true"].shape == (B,)
    assert [block_dtype(1, 2, 1).fields[k][1] for k in ("calls", "recorded", "ticket", "reserved")] == [0, 4, 8, 12]
    assert size(0, 292, 4) == size(3, 1, 4) == size(3, 2049, 4) == size(3, 292, 0) == size(1 << 31, 292, 1) == 0
    ws = lib.dctn_batch_monitor_workspace_bytes
    assert [ws(b) for b in (1, 3, 130, 1024)] == [SLOT_BYTES * b for b in (1, 3, 130, 1024)] and ws(0) == ws(-1) == ws(1 << 31) == 0
    assert ctypes.sizeof(_lib.BatchMonitorCall) == 8 * 9 + 4 * 12


def test_return_codes_in_the_projects_order():
    lib = _lib.lib()
    good = dict(x=PTR, logits=PTR, y=PTR, indices=None, edges=PTR, block=PTR, workspace=PTR, workspace_bytes=40 * 5, B=5, C=1,
                H=6, W=6, Q=2, K=3, L=10, n_edges=292, period=1, capacity=2, x_dtype=_lib.F32, logits_dtype=_lib.F32)

    def call(**kw):
        return lib.dctn_batch_monitor(ctypes.byref(_lib.BatchMonitorCall(**dict(good, **kw))), None)

    # (the good call itself would launch: it is never made)
    assert lib.dctn_batch_monitor(None, None) == _lib.ERR_NULL
    for name in ("x", "logits", "y", "edges", "block", "workspace"):
        assert call(**{name: None}) == _lib.ERR_NULL, name
        assert call(**{name: None}, B=0, x_dtype=9, workspace_bytes=1) == _lib.ERR_NULL, name   # NULL first, whatever else is wrong
    # shapes
    for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(Q=0), dict(K=-1), dict(K=7), dict(K=5, H=4, W=9),
                dict(K=5, W=4, H=9), dict(L=0), dict(L=1025), dict(n_edges=1), dict(n_edges=2049), dict(period=0),
                dict(capacity=0)):
        assert call(**bad) == _lib.ERR_BAD_SHAPE, bad
        assert call(**bad, x_dtype=9, workspace_bytes=1) == _lib.ERR_BAD_SHAPE, bad   # shape before dtype and the limits
    # dtypes
    assert call(x_dtype=3) == call(logits_dtype=7) == call(x_dtype=-1) == _lib.ERR_BAD_DTYPE
    assert call(x_dtype=9, workspace_bytes=1) == call(logits_dtype=9, block=PTR + 4) == _lib.ERR_BAD_DTYPE   # before the limits
    assert call(x_dtype=9, B=1 << 22, L=1024) == _lib.ERR_BAD_DTYPE
    # unsupported: B * L, alignment, the workspace's size, the LDS
    assert call(B=1 << 22, L=1024, workspace_bytes=40 << 22) == _lib.ERR_UNSUPPORTED
    assert call(x=PTR + 2) == call(logits=PTR + 2) == call(x=PTR + 4, x_dtype=_lib.F64) == _lib.ERR_UNSUPPORTED
    assert call(logits=PTR + 1, logits_dtype=_lib.BF16) == call(y=PTR + 4) == call(indices=PTR + 4) == _lib.ERR_UNSUPPORTED
    assert call(edges=PTR + 4) == call(block=PTR + 4) == call(workspace=PTR + 4) == _lib.ERR_UNSUPPORTED
    assert call(workspace_bytes=199) == call(workspace_bytes=201) == call(workspace_bytes=0) == _lib.ERR_UNSUPPORTED
    cus, lds = _lib.c_int(), _lib.c_int()
    assert lib.dctn_device_limits(cus, lds) == 0
    side = int((lds.value // 16) ** 0.5) + 1     # 16 side^2 bytes of pairs alone exceed the device's LDS
    assert call(H=side, W=side) == _lib.ERR_UNSUPPORTED
    assert call(H=side, W=side, x_dtype=9) == _lib.ERR_BAD_DTYPE


# ------------------------------------------------------------------ the ring
def _block(batch, n_edges, capacity, recorded, period=1):
    """A block as `recorded` recorded launches of period `period` leave it: row seq holds x_sum = seq."""
    raw = np.zeros((), dtype=block_dtype(batch, n_edges, capacity))
    raw["recorded"], raw["calls"] = recorded, (recorded - 1) * period + 1 if recorded else 0
    for seq in range(recorded):   # later rows overwrite earlier ones, as on the device
        row = raw["rows"][seq % capacity]
        row["call"], row["seq"], row["x_sum"] = seq * period, seq, float(seq)
        row["index"] = seq
    return raw


def test_decode_wraps_counts_the_lost_rows_and_reads_nothing_twice():
    rows, lost = decode(_block(3, 5, 4, 0), 0, 4)
    assert rows == [] and lost == 0
    rows, lost = decode(_block(3, 5, 4, 3, period=5), 0, 4)
    assert [(int(r["call"]), int(r["seq"])) for r in rows] == [(0, 0), (5, 1), (10, 2)] and lost == 0
    rows, lost = decode(_block(3, 5, 4, 3), 3, 4)   # again: nothing new
    assert rows == [] and lost == 0
    rows, lost = decode(_block(3, 5, 4, 11), 3, 4)  # wrapped: 3 .. 6 were overwritten
    assert [int(r["seq"]) for r in rows] == [7, 8, 9, 10] and lost == 4
    assert [float(r["x_sum"]) for r in rows] == [7.0, 8.0, 9.0, 10.0]
    torn = _block(3, 5, 4, 6)
    torn["rows"][1]["seq"] = 1   # a row the device has not finished
    with pytest.raises(AssertionError):
        decode(torn, 0, 4)


def test_read_on_a_cpu_block_follows_decode():
    mon = BatchMonitor("cpu", 3, 10, (1, 4, 4, 2), kernel_size=3, period=5, capacity=4)
    assert mon.n_edges == 292 and mon.block_bytes == block_dtype(3, 292, 4).itemsize and mon.workspace_bytes == 120
    assert mon.read() == [] and mon.lost == 0
    mon.block.copy_(torch.from_numpy(_block(3, 292, 4, 6, period=5).reshape(1).view(np.uint8)))
    rows = mon.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(10, 2), (15, 3), (20, 4), (25, 5)] and mon.lost == 2
    assert rows[3]["input"]["sum"] == 5.0 and rows[3]["input"]["mean"] == 5.0 / 96 and list(rows[2]["index"]) == [4, 4, 4]
    assert set(rows[0]) == {"call", "seq", "rows", "correct", "bad_rows", "input", "logits", "hist", "p_true", "pred", "label", "index"}
    assert set(rows[0]["input"]) >= {"mean", "std", "nonfinite", "window_mean", "window_std"}
    assert set(rows[0]["logits"]) >= {"min", "max", "mean", "std", "nonfinite"}
    assert set(rows[0]["hist"]) == {"counts", "below", "above", "nan"} and rows[0]["hist"]["counts"].shape == (291,)
    assert mon.read() == [] and mon.lost == 2
    mon.reset(calls=7)
    raw = mon.raw()
    assert (int(raw["calls"]), int(raw["recorded"])) == (7, 0) and not raw["rows"].tobytes().strip(b"\0") and mon.lost == 0


def test_the_default_table_is_tensorboards_buckets_where_a_probability_can_fall():
    e = probability_edges()
    assert e.shape == (292,) and e.dtype == np.float64 and e[0] == 0.0 and e[-1] == 1.0089710279437536
    assert np.array_equal(e, tensor_hist.tensorboard_edges()[774:1066]) and e[1] == 1e-12 and e[-2] < 1.0 < e[-1]
    assert (np.diff(e) > 0).all()


# ------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("shape", [(1, 3, 4, 4, 2, 3, 10), (2, 5, 5, 4, 3, 2, 3), (1, 1, 3, 3, 2, 3, 1), (1, 7, 6, 6, 4, 1, 7),
                                   (1, 4, 6, 6, 2, 0, 7)])
def test_mirror_against_independent_formulations(shape):
    C, B, H, W, Q, K, L = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(C, B, H, W, Q, generator=g, dtype=torch.float64)
    z = torch.randn(B, L, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, L, (B,), generator=g)
    idx = torch.randint(0, 1000, (B,), generator=g)
    m = mirror(x, z, y, idx, K, None)
    p = torch.softmax(z.double(), 1).numpy()
    assert np.allclose(m["p_true"], p[np.arange(B), y.numpy()])
    counts, _ = np.histogram(p, bins=probability_edges())
    assert np.array_equal(m["counts"], counts) and m["below"] == m["above"] == m["nan"] == 0 and counts.sum() == B * L
    assert np.array_equal(m["pred"], z.argmax(1).numpy()) and np.array_equal(m["label"], y.numpy())
    assert np.array_equal(m["index"], idx.numpy()) and (mirror(x, z, y, None, K)["index"] == -1).all()
    assert m["rows"] == B and m["correct"] == int((z.argmax(1) == y).sum()) and m["bad_rows"] == 0
    s = summarise(m, (C, H, W, Q), B, L, K)
    assert np.allclose(s["input"]["mean"], float(x.mean()))
    assert np.allclose(s["input"]["std"], float(torch.std(x)))
    assert np.allclose(s["logits"]["mean"], float(z.mean())) and s["logits"]["min"] == float(z.min()) and s["logits"]["max"] == float(z.max())
    if B * L > 1:
        assert np.allclose(s["logits"]["std"], float(torch.std(z)))
    else:
        assert np.isnan(s["logits"]["std"])
    if K > 0:
        windows = make_windows(x, K)
        assert np.allclose(s["input"]["window_std"], float(windows.std_over_batch()))
        assert np.allclose(s["input"]["window_mean"], float(windows.mean_over_batch()))
        assert np.allclose(m["win_sum"], float(windows.sum_over_batch()))
        assert np.allclose(m["win_sq"], float(windows.squared_fro_norm_over_batch()))
    else:
        assert s["input"]["window_std"] is None and m["win_sum"] == m["win_sq"] == 0.0


def test_mirror_special_rows_and_a_custom_table():
    x = torch.zeros(1, 4, 3, 3, 2, dtype=torch.float64)
    x[0, 1, 0, 0, 0] = float("nan")
    z = torch.tensor([[0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [float("nan"), 2.0, 3.0], [0.0, float("inf"), -4.0]], dtype=torch.float64)
    y = torch.tensor([2, -100, 1, 3])
    m = mirror(x, z, y, None, 3, [0.0, 0.25, 0.5, 1.0])
    assert m["x_nonfinite"] == 1 and m["x_sum"] == 0.0 and np.isnan(m["win_sum"])
    assert (m["rows"], m["correct"], m["bad_rows"], m["z_nonfinite"], m["nan"]) == (2, 1, 2, 2, 6)
    assert list(m["pred"]) == [2, 0, -1, -1] and np.isnan(m["p_true"][1:]).all() and m["p_true"][0] > 0.5
    assert (m["z_sum"], m["z_min"], m["z_max"]) == (4.0, -4.0, 3.0)
    # softmax([0, 0, 1]) = (0.21, 0.21, 0.58), softmax([1, 1, 0]) = (0.42, 0.42, 0.16)
    assert list(m["counts"]) == [3, 2, 1] and m["below"] == m["above"] == 0


def test_histogram_summary_hands_add_histogram_raw_its_arguments():
    e = probability_edges()
    counts = np.zeros(291, dtype=np.int64)
    counts[[100, 102, 290]] = [3, 1, 2]
    s = histogram_summary({"counts": counts, "below": 0, "above": 0, "nan": 0}, e)
    limits, kept = tensor_hist.trim_buckets(counts, e)
    assert s["bucket_limits"] == limits and s["bucket_counts"] == kept and s["num"] == 6
    assert s["min"] == e[100] and s["max"] == e[291] and set(s) == {"min", "max", "num", "sum", "sum_squares", "bucket_limits", "bucket_counts"}
    empty = histogram_summary({"counts": np.zeros(291, dtype=np.int64)}, e)
    assert empty["num"] == 0 and empty["bucket_counts"] == [0, 0]


# ------------------------------------------------------------------ the logger
class _FakeMonitor:
    """What the logger needs of a `BatchMonitor`: read() and the table."""

    def __init__(self, batches):
        self.batches, self.reads, self.edges = list(batches), 0, probability_edges()

    def read(self):
        self.reads += 1
        return self.batches.pop(0) if self.batches else []


def _entry(call, value, window=True):
    counts = np.zeros(291, dtype=np.int64)
    counts[200] = call + 1
    return {"call": call, "seq": call, "rows": 2, "correct": 1, "bad_rows": 0,
            "input": {"mean": value, "std": value + 1, "nonfinite": 0, "window_mean": 0.5, "window_std": value + 2 if window else None},
            "logits": {"min": -value, "max": value, "mean": value / 2, "std": value / 4, "nonfinite": 0},
            "hist": {"counts": counts, "below": 0, "above": 0, "nan": 0},
            "p_true": np.array([0.25, 0.5], dtype=np.float32), "pred": np.array([1, 0], dtype=np.int32),
            "label": np.array([1, 1]), "index": np.array([call, call + 1])}


def test_the_logger_reports_the_references_tags_at_first_iter_plus_call():
    mon = _FakeMonitor([[_entry(0, 1.0), _entry(20, 2.0)], [_entry(40, 4.0, window=False)], []])
    scalars, hists, samples = [], [], []
    hook = training.make_batch_monitor_logger(mon, 3, lambda tag, value, it: scalars.append((tag, value, it)),
                                              lambda tag, summary, it: hists.append((tag, summary, it)),
                                              lambda it, index, label, pred, p_true: samples.append((it, index, label, pred, p_true)),
                                              first_iter=100)
    for launch in range(7):
        hook({}, {"num_iters_done": 100 + 8 * launch + 7})
    assert mon.reads == 2   # launches 3 and 6
    out = "train_outputs_of_the_whole_model_intermediate_output_"
    assert scalars[:7] == [("train_input/dumb_mean", 1.0, 100), ("train_input/dumb_std", 2.0, 100),
                           ("train_input_intermediate_output_std_of_coordinates_of_windows/", 3.0, 100),
                           (out + "dumb_min/", -1.0, 100), (out + "dumb_max/", 1.0, 100), (out + "dumb_mean/", 0.5, 100),
                           (out + "dumb_std/", 0.25, 100)]
    assert [s[2] for s in scalars] == [100] * 7 + [120] * 7 + [140] * 6   # no window tag without windows
    assert [s[0] for s in scalars[14:]] == ["train_input/dumb_mean", "train_input/dumb_std", out + "dumb_min/", out + "dumb_max/",
                                            out + "dumb_mean/", out + "dumb_std/"]
    assert [(h[0], h[2], h[1]["num"]) for h in hists] == [(out + "logits_as_probabilities/", 100, 1),
                                                          (out + "logits_as_probabilities/", 120, 21),
                                                          (out + "logits_as_probabilities/", 140, 41)]
    assert hists[0][1] == histogram_summary(_entry(0, 1.0)["hist"], probability_edges())
    assert [s[0] for s in samples] == [100, 120, 140] and list(samples[1][1]) == [20, 21] and list(samples[1][3]) == [1, 0]
    assert samples[2][4].dtype == np.float32 and list(samples[2][2]) == [1, 1]
    hook.flush()
    assert mon.reads == 3 and len(scalars) == 20   # nothing new: nothing reported
    assert set(TAGS.values()) == {s[0] for s in scalars} | {h[0] for h in hists}
    only_scalars = training.make_batch_monitor_logger(_FakeMonitor([[_entry(5, 1.0)]]), 1, lambda *a: scalars.append(a))
    only_scalars({}, {})
    assert [s[2] for s in scalars[20:]] == [5] * 7


# ------------------------------------------------------------------ the host object and the steps
def test_batch_monitor_checks_its_arguments():
    for bad in (dict(batch=0), dict(labels=0), dict(labels=1025), dict(x_shape=(1, 4, 4)), dict(x_shape=(1, 0, 4, 2)),
                dict(kernel_size=5), dict(kernel_size=-1), dict(period=0), dict(capacity=0), dict(edges=[0.0]),
                dict(edges=[0.0, 0.5, 0.5])):
        kw = dict(batch=3, labels=10, x_shape=(1, 4, 4, 2))
        kw.update(bad)
        with pytest.raises(ValueError):
            BatchMonitor("cpu", **kw)
    with pytest.raises(NotImplementedError):
        BatchMonitor("cpu", 1 << 22, 1024, (1, 4, 4, 2))
    mon = BatchMonitor("cpu", 3, 10, (1, 4, 4, 2), edges=[0.0, 0.5, 1.0])
    assert (mon.period, mon.capacity, mon.kernel_size, mon.n_edges) == (20, 16, 3, 3)
    x, z, y = torch.zeros(1, 3, 4, 4, 2), torch.zeros(3, 10), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="QUANTUM"):
        mon.record(torch.zeros(3, 1, 4, 4), z, y)
    for args in ((torch.zeros(1, 4, 4, 4, 2), z, y), (x, torch.zeros(3, 9), y), (x, z, torch.zeros(4, dtype=torch.int64)),
                 (x, z, y, torch.zeros(2, dtype=torch.int64)), (x.transpose(2, 3), z, y)):
        with pytest.raises(ValueError):
            mon.record(*args)
    for args in ((x.half(), z, y), (x, z.to(torch.int32), y), (x, z, y.to(torch.int32)), (x, z, y, y.to(torch.int32))):
        with pytest.raises(TypeError):
            mon.record(*args)
    with pytest.raises(RuntimeError):
        mon.record(x, z, y)   # there is no CPU form of the launch


def test_the_steps_take_a_monitor_and_refuse_the_image_form():
    import inspect

    arg = inspect.signature(training.GraphedTrainStep.__init__).parameters["monitor"]
    assert arg.kind is inspect.Parameter.KEYWORD_ONLY and arg.default is None
    params = inspect.signature(training.train_step).parameters
    assert params["monitor"].default is None and params["indices"].default is None
    mon = BatchMonitor("cpu", 2, 10, (1, 8, 8, 2))
    model = torch.nn.Linear(4, 2)
    with pytest.raises(ValueError, match="QUANTUM"):
        training.train_step(model, torch.zeros(2, 1, 8, 8), torch.zeros(2, dtype=torch.int64), None, None, monitor=mon)
