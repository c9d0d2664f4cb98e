"""`dctn_batch_monitor` (csrc/batch_monitor.hip) and `batch_monitor.BatchMonitor` on the GPU (`-m gpu`).

The kernel works in float64 throughout.  On x in {0, 0.5, 1} and small integer logits every sum and window product is an
integer multiple of a power of two below 2^53 units (asserted on the host first): exact in a double in any order, so the
comparison is `==` against the numpy `mirror`.  Random inputs are held to bounds derived from the arithmetic: for a sum,
(operations on the longest path) x 2^-52 x (sum of the absolute terms), which covers the device's and the mirror's
roundings together; for the histogram no float64 probability may lie within a relative 1e-9 of an edge (asserted first),
while the device's exp and L-term sum err by a few 2^-53; `p_true` may then differ from the float32 rounding of the
mirror's value by one float32 ulp at most, because only a value on a rounding boundary can round the other way.

The plan's boundaries (csrc/batch_monitor.hip): one workgroup per sample, 256 threads over a sample's C H W pairs and over
its windows, the rows of the logits and the samples' slots in chunks of 256 - B = 130 and 28 x 28 pixels cross each."""
import ctypes

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd.batch_monitor import BatchMonitor, block_dtype, mirror, probability_edges, summarise
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EDGES = probability_edges()
SUMS = ("x_sum", "x_sum_sq", "win_sum", "win_sq", "z_sum", "z_sum_sq", "z_min", "z_max")
COUNTS = ("rows", "correct", "bad_rows", "z_nonfinite", "x_nonfinite", "below", "above", "nan")


def launch(x, logits, y, indices, K, edges=EDGES, period=1, capacity=1, launches=1, workspace_fill=0xFF, calls=0):
    """`launches` launches of the C entry point over guarded buffers; the block after each one as a structured element.
    The inputs and a decoy must come out as they went in, and the workspace is exactly as large as the library asks."""
    C, B, H, W, Q = x.shape
    n_labels = logits.shape[1]
    table = np.asarray(edges, dtype=np.float64)
    lib = L.lib()
    dt = block_dtype(B, table.size, capacity)
    block_bytes, ws_bytes = lib.dctn_batch_monitor_block_bytes(B, table.size, capacity), lib.dctn_batch_monitor_workspace_bytes(B)
    assert block_bytes == dt.itemsize and ws_bytes == 40 * B
    seen = []
    with guarded(fill=workspace_fill) as arena:
        held = [arena.place(t.to(DEV).contiguous()) for t in (x, logits, y)]
        idx = None if indices is None else arena.place(indices.to(DEV))
        e = arena.place(torch.from_numpy(table.copy()).to(DEV))
        decoy = arena.empty((4096,), torch.uint8, DEV)
        block = arena.zeros((block_bytes,), torch.uint8, DEV)
        if calls:
            block[:4] = torch.from_numpy(np.array([calls], dtype="<u4").view(np.uint8).copy()).to(DEV)
        ws = arena.empty((ws_bytes,), torch.uint8, DEV)
        inputs = held + [e] + ([] if idx is None else [idx])
        before = [t.clone() for t in inputs]
        call = L.BatchMonitorCall(x=held[0].data_ptr(), logits=held[1].data_ptr(), y=held[2].data_ptr(),
                                  indices=None if idx is None else idx.data_ptr(), edges=e.data_ptr(), block=block.data_ptr(),
                                  workspace=ws.data_ptr(), workspace_bytes=ws_bytes, B=B, C=C, H=H, W=W, Q=Q, K=K, L=n_labels,
                                  n_edges=table.size, period=period, capacity=capacity, x_dtype=L.dtype_code(held[0]),
                                  logits_dtype=L.dtype_code(held[1]))
        for _ in range(launches):
            L.check(lib.dctn_batch_monitor(ctypes.byref(call), L.stream_ptr(DEV)), "batch monitor")
            seen.append(block.cpu().numpy().view(dt)[0].copy())
            for t, b in zip(inputs, before):
                assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "an input buffer changed"
        ws_after = ws.clone()
    arena.check()
    assert bool((decoy == workspace_fill).all())
    launch.last_workspace = ws_after
    return seen


def _exact_inputs(shape, x_dtype, z_dtype, seed=1):
    C, B, H, W, Q, K, n_labels = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 3, (C, B, H, W, Q), generator=g).double() / 2).to(x_dtype)
    z = torch.randint(-4, 5, (B, n_labels), generator=g).double().to(z_dtype)
    y = torch.randint(0, n_labels, (B,), generator=g)
    idx = torch.randint(0, 1 << 40, (B,), generator=g)
    return x, z, y, idx


def _assert_row_equals_mirror(row, want, sums=SUMS):
    for key in sums:
        assert float(row[key]) == want[key], (key, float(row[key]), want[key])
    for key in COUNTS:
        assert int(row[key]) == want[key], (key, int(row[key]), want[key])
    assert np.array_equal(row["pred"], want["pred"]) and np.array_equal(row["label"], want["label"])
    assert np.array_equal(row["index"], want["index"])


# ------------------------------------------------------------------ 1. exact inputs
SHAPES = [(1, 3, 4, 4, 2, 3, 10), (2, 5, 5, 4, 3, 2, 3), (1, 1, 3, 3, 2, 3, 1), (1, 130, 28, 28, 2, 3, 10), (1, 4, 6, 6, 4, 1, 7),
          (1, 4, 6, 6, 2, 0, 7)]
EXACT = [(s, F32, F32) for s in SHAPES] + [(s, a, b) for s in SHAPES[:2]
                                            for a, b in ((F64, F64), (BF16, BF16), (F32, BF16), (F64, F32), (BF16, F64))]


@pytest.mark.parametrize("shape,x_dtype,z_dtype", EXACT, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_exact_inputs_equal_the_mirror(shape, x_dtype, z_dtype):
    C, B, H, W, Q, K, n_labels = shape
    # in units of 2^-2 per factor the largest window sum is B Ho Wo (4 Q)^(K K C); the other sums are far smaller
    windows = B * (H - K + 1) * (W - K + 1) if K else 0
    assert windows * (4 * Q) ** (K * K * C) < 2 ** 53 and 4 * C * B * H * W * Q < 2 ** 53 and 16 * B * n_labels < 2 ** 53
    x, z, y, idx = _exact_inputs(shape, x_dtype, z_dtype)
    (raw,) = launch(x, z, y, idx, K)
    assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (1, 1, 0)
    row = raw["rows"][0]
    assert (int(row["call"]), int(row["seq"])) == (0, 0)
    want = mirror(x, z, y, idx, K)
    _assert_row_equals_mirror(row, want)
    assert int(row["counts"].sum()) + int(row["below"]) + int(row["above"]) == B * n_labels and int(row["reserved"]) == 0
    assert want["bad_rows"] == 0 and want["rows"] == B
    if K == 0:
        assert float(row["win_sum"]) == float(row["win_sq"]) == 0.0
    elif B > 1:   # (a single window may hold a pixel whose values are all 0)
        assert float(row["win_sum"]) > 0


# ------------------------------------------------------------------ 2. histogram and p_true on random logits
def _edge_margin(p, edges):
    """The smallest relative distance of a probability to an edge of the table."""
    p = np.asarray(p).reshape(-1)
    at = np.clip(np.searchsorted(edges, p), 1, edges.size - 1)
    below, above = edges[at - 1], edges[at]
    return float(np.min(np.minimum(np.abs(p - below), np.abs(above - p)) / p))


@pytest.mark.parametrize("case", [(130, 10, 3), (3, 10, 3), (5, 3, 1), (1, 1, 1), (7, 64, 8)], ids=str)
def test_random_logits_histogram_and_confidence(case):
    B, n_labels, s = case
    x = torch.zeros(1, B, 3, 3, 2)
    for seed in range(5):
        torch.manual_seed(seed)
        z = torch.randn(B, n_labels) * s
        y = torch.randint(0, n_labels, (B,), generator=torch.Generator().manual_seed(seed))
        want = mirror(x, z, y, None, 0)
        z64 = z.double().numpy()
        p = np.exp(z64 - z64.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        assert _edge_margin(p[p > 0], EDGES) > 1e-9
        (raw,) = launch(x, z, y, None, 0)
        row = raw["rows"][0]
        assert np.array_equal(row["counts"], want["counts"]), (case, seed)
        assert [int(row[k]) for k in ("below", "above", "nan")] == [want[k] for k in ("below", "above", "nan")]
        assert int(row["counts"].sum()) + int(row["below"]) == B * n_labels
        rounded = want["p_true"].astype(np.float32)
        print(case, seed, "max |p_true - float32(mirror)| in ulps:",
              float(np.max(np.abs(row["p_true"].astype(np.float64) - rounded.astype(np.float64)) / np.spacing(rounded))))
        assert (np.abs(row["p_true"].astype(np.float64) - rounded.astype(np.float64)) <= np.spacing(rounded).astype(np.float64)).all()
        assert np.array_equal(row["pred"], want["pred"]) and int(row["correct"]) == want["correct"]


# ------------------------------------------------------------------ 3. random x
@pytest.mark.parametrize("shape", [(1, 130, 28, 28, 2, 3), (2, 5, 5, 4, 3, 2), (3, 7, 9, 10, 4, 2), (1, 4, 6, 6, 4, 1)], ids=str)
def test_random_x_stays_inside_the_bound_of_its_arithmetic(shape):
    C, B, H, W, Q, K = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(C, B, H, W, Q, generator=g)
    z, y = torch.zeros(B, 2), torch.zeros(B, dtype=torch.int64)
    (raw,) = launch(x, z, y, None, K)
    row, want = raw["rows"][0], mirror(x, z, y, None, K)
    u2 = 2.0 ** -52
    a = x.double().numpy()
    # a thread adds ceil(C H W / 256) pairs of Q values, the tree 6 + 3 partial sums, the last workgroup B slots
    ops = -(-C * H * W // 256) * Q + 6 + 3 + B
    for key, terms in (("x_sum", np.abs(a).sum()), ("x_sum_sq", (a * a).sum())):
        print(shape, key, abs(float(row[key]) - want[key]), "bound", ops * u2 * terms)
        assert abs(float(row[key]) - want[key]) <= ops * u2 * terms, key
    # a window: K K C factors of Q additions each, as many multiplications; then the windows of a thread, the tree, the slots
    Ho, Wo = H - K + 1, W - K + 1
    ops = K * K * C * Q + K * K * C + -(-Ho * Wo // 256) + 6 + 3 + B
    s, q = np.abs(a).sum(axis=4), (a * a).sum(axis=4)
    ps, pq = np.ones((B, Ho, Wo)), np.ones((B, Ho, Wo))
    for dh in range(K):
        for dw in range(K):
            for c in range(C):
                ps, pq = ps * s[c, :, dh:dh + Ho, dw:dw + Wo], pq * q[c, :, dh:dh + Ho, dw:dw + Wo]
    for key, terms in (("win_sum", ps.sum()), ("win_sq", pq.sum())):
        print(shape, key, abs(float(row[key]) - want[key]), "bound", ops * u2 * terms)
        assert abs(float(row[key]) - want[key]) <= ops * u2 * terms, key
    assert int(row["x_nonfinite"]) == 0


# ------------------------------------------------------------------ 4. special rows
def test_labels_outside_the_range_bad_rows_and_non_finite_inputs():
    x, z, y, _ = _exact_inputs((1, 6, 4, 4, 2, 3, 5), F32, F32, seed=2)
    x[0, 2, 1, 1, 0] = float("nan")
    x[0, 4, 0, 3, 1] = float("-inf")
    y[0], y[1] = -100, 5
    z[2, 1], z[3, 4] = float("nan"), float("inf")
    z[3, 0] = 7.0
    (raw,) = launch(x, z, y, None, 3)
    row, want = raw["rows"][0], mirror(x, z, y, None, 3)
    _assert_row_equals_mirror(row, want, sums=SUMS[:2] + SUMS[4:])
    assert np.isnan(float(row["win_sum"])) and np.isnan(want["win_sum"])   # nothing is filtered out of the window sums
    assert int(row["rows"]) == 4 and int(row["bad_rows"]) == 2 and int(row["nan"]) == 10 and int(row["z_nonfinite"]) == 2
    assert int(row["x_nonfinite"]) == 2 and float(row["x_sum"]) == float(torch.where(torch.isfinite(x), x, torch.zeros_like(x)).double().sum())
    assert list(row["pred"][2:4]) == [-1, -1] and (row["pred"][[0, 1, 4, 5]] >= 0).all()
    assert np.isnan(row["p_true"][:4]).all() and not np.isnan(row["p_true"][4:]).any()
    assert float(row["z_max"]) == 7.0   # a bad row's finite logits are still in z_*
    assert (row["index"] == -1).all() and int(row["counts"].sum()) == 4 * 5
    # no finite logit at all
    (raw,) = launch(x, torch.full((6, 5), float("nan")), y, None, 3)
    row = raw["rows"][0]
    assert float(row["z_min"]) == float("inf") and float(row["z_max"]) == float("-inf") and int(row["bad_rows"]) == 6
    assert int(row["nan"]) == 30 and not row["counts"].any() and (row["pred"] == -1).all()


# ------------------------------------------------------------------ 5. period and ring
def test_period_three_and_a_ring_of_two_rows_over_eight_launches():
    shape = (1, 3, 4, 4, 2, 3, 10)
    mon = BatchMonitor(DEV, 3, 10, (1, 4, 4, 2), kernel_size=3, period=3, capacity=2)
    raws, wants = [], {}
    for i in range(8):
        x, z, y, idx = (t.to(DEV) for t in _exact_inputs(shape, F32, F32, seed=20 + i))
        wants[i] = mirror(x, z, y, idx, 3)
        mon.record(x, z, y, idx)
        raws.append(mon.raw())
    assert [(int(r["calls"]), int(r["recorded"]), int(r["ticket"])) for r in raws] == [
        (1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 2, 0), (5, 2, 0), (6, 2, 0), (7, 3, 0), (8, 3, 0)]
    for i in (1, 2, 4, 5, 7):   # a launch that is not recorded leaves the rows' bytes untouched
        assert raws[i]["rows"].tobytes() == raws[i - 1]["rows"].tobytes()
    assert not raws[0]["rows"][1].tobytes().strip(b"\0")
    rows = mon.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(3, 1), (6, 2)] and mon.lost == 1
    for r in rows:
        want = summarise(wants[r["call"]], (1, 4, 4, 2), 3, 10, 3)
        assert r["input"] == want["input"] and r["logits"] == want["logits"] and np.array_equal(r["index"], want["index"])
    assert mon.read() == []
    mon.reset(calls=1)   # the phase shifts: calls 1 and 2 are skipped, call 3 is recorded
    for i in range(3):
        mon.record(x, z, y, idx)
        raw = mon.raw()
        assert (int(raw["calls"]), int(raw["recorded"])) == (2 + i, 1 if i == 2 else 0)
    (r,) = mon.read()
    assert (r["call"], r["seq"]) == (3, 0) and mon.lost == 0


# ------------------------------------------------------------------ 6. determinism and contract
def _without_call_and_seq(row):
    row = row.copy()
    row["call"], row["seq"] = 0, 0
    return row.tobytes()


@pytest.mark.parametrize("shape", [(2, 5, 5, 4, 3, 2, 3), (1, 130, 28, 28, 2, 3, 10)], ids=str)
def test_only_block_and_workspace_are_written_and_the_bits_repeat(shape):
    """`launch` guards every buffer, gives the workspace exactly the queried size and compares the inputs and a decoy;
    here, besides: the row does not depend on what the workspace held - NaN bytes, 0x7B bytes or the previous launch's
    content - and two recorded launches on the same inputs give identical row bytes apart from call / seq."""
    C, B, H, W, Q, K, n_labels = shape
    g = torch.Generator().manual_seed(5)
    x, z = torch.randn(C, B, H, W, Q, generator=g), torch.randn(B, n_labels, generator=g) * 3
    y, idx = torch.randint(0, n_labels, (B,), generator=g), torch.randint(0, 99, (B,), generator=g)
    poisoned = launch(x, z, y, idx, K, period=2, capacity=2, launches=3, workspace_fill=0xFF)
    large = launch(x, z, y, idx, K, period=2, capacity=2, launches=3, workspace_fill=0x7B)
    zeroed = launch(x, z, y, idx, K, period=2, capacity=2, launches=3, workspace_fill=0x00)
    for a, b, c in zip(poisoned, large, zeroed):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert [(int(r["calls"]), int(r["recorded"]), int(r["ticket"])) for r in poisoned] == [(1, 1, 0), (2, 1, 0), (3, 2, 0)]
    first, skipped, third = poisoned
    assert skipped["rows"].tobytes() == first["rows"].tobytes()
    # the third launch found the first one's slots in the workspace
    assert (int(third["rows"][1]["call"]), int(third["rows"][1]["seq"])) == (2, 1)
    assert _without_call_and_seq(third["rows"][1]) == _without_call_and_seq(first["rows"][0])
    # a launch that is not recorded leaves the workspace as it found it
    (raw,) = launch(x, z, y, idx, K, period=2, capacity=1, workspace_fill=0x7B, calls=1)
    assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (2, 0, 0) and not raw["rows"].tobytes().strip(b"\0")
    assert bool((launch.last_workspace == 0x7B).all())


# ------------------------------------------------------------------ 7. capture
def test_a_captured_record_replayed_five_times_follows_its_static_inputs():
    shape = (1, 5, 6, 6, 2, 3, 4)
    versions = [_exact_inputs(shape, F32, F32, seed=30 + i) for i in range(5)]
    mon = BatchMonitor(DEV, 5, 4, (1, 6, 6, 2), kernel_size=3, period=1, capacity=8)
    x, z, y, idx = (t.to(DEV).clone() for t in versions[0])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        mon.record(x, z, y, idx)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    mon.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mon.record(x, z, y, idx)
    assert int(mon.raw()["calls"]) == 0   # a capture runs nothing
    for v in versions:
        for static, new in zip((x, z, y, idx), v):
            static.copy_(new)
        graph.replay()
    raw = mon.raw()
    assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (5, 5, 0)
    for i, v in enumerate(versions):
        row = raw["rows"][i]
        assert (int(row["call"]), int(row["seq"])) == (i, i)
        _assert_row_equals_mirror(row, mirror(*v, 3))
    assert [r["seq"] for r in mon.read()] == [0, 1, 2, 3, 4] and mon.lost == 0


# ------------------------------------------------------------------ 8. in the step
def _eps_objects(monitored=True):
    from dctn_amd.batches import DeviceBatches
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd
    from dctn_amd.training import FlatAdam

    torch.manual_seed(3)
    model = EPSesPlusLinear(((2, 2),), UnitTheoreticalOutputStd(), 1.0, DEV, F32, image_size=6)
    g = torch.Generator().manual_seed(4)
    images, labels = torch.randint(0, 256, (12, 6, 6), generator=g, dtype=torch.uint8), torch.randint(0, 10, (12,), generator=g)
    src = DeviceBatches(images, labels, 4, dtype=F32, seed=9, device=DEV)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3)
    mon = BatchMonitor(DEV, 4, 10, (1, 6, 6, 2), kernel_size=2, period=1, capacity=8) if monitored else None
    return model, src, opt, mon


def _eps_step(model, src, opt, mon, K):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    kw = {} if mon is None else {"monitor": mon}
    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src, iters_per_launch=K, **kw)


def test_two_launches_of_one_iteration_and_one_launch_of_two_leave_the_same_block():
    model, src, opt, mon = _eps_objects()
    step = _eps_step(model, src, opt, mon, 1)
    assert int(mon.raw()["calls"]) == 1   # the warm-up iteration counts
    mon.reset()
    step()
    out = step()
    torch.cuda.synchronize(DEV)
    assert set(out) == {"output", "loss", "reg_term", "indices"}
    raw_a, rows_a = mon.raw(), mon.read()
    assert [(r["call"], r["seq"]) for r in rows_a] == [(0, 0), (1, 1)]
    for k, r in enumerate(rows_a):   # the warm-up consumed draw 0
        assert list(r["index"]) == src.expected_indices(1 + k)
    last = mirror(step.x, out["output"], step.y, out["indices"], 2)
    _assert_row_equals_mirror(raw_a["rows"][1], last, sums=("z_min", "z_max"))
    assert np.allclose(float(raw_a["rows"][1]["x_sum"]), last["x_sum"]) and np.allclose(float(raw_a["rows"][1]["win_sq"]), last["win_sq"])
    assert np.allclose(rows_a[1]["p_true"], last["p_true"], rtol=1e-6, atol=0)

    model, src, opt, mon = _eps_objects()
    step = _eps_step(model, src, opt, mon, 2)
    mon.reset(calls=0)
    # (the warm-up of a K = 2 step is one iteration as well: both sources stand at draw 1)
    assert step()["iters"] == 2
    torch.cuda.synchronize(DEV)
    assert mon.raw().tobytes() == raw_a.tobytes()

    plain = _eps_step(*_eps_objects(monitored=False), 1)
    assert plain.monitor is None and set(plain()) == {"output", "loss", "reg_term", "indices"}


def test_the_classifier_under_a_graphed_step_records_its_quantum_batches():
    from dctn_amd import batches
    from dctn_amd.conv_sbs import DumbNormalInitialization
    from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi
    from dctn_amd.training import FlatRMSprop, GraphedTrainStep, fused_cross_entropy

    g = torch.Generator().manual_seed(6)
    images, labels = torch.randint(0, 256, (8, 8, 8), generator=g, dtype=torch.uint8), torch.randint(0, 10, (8,), generator=g)
    torch.manual_seed(3)
    model = DCTNMnistModel(2, 2, False, DumbNormalInitialization(0.9), False, 1.0).to(DEV)
    src = batches.DeviceBatches(images, labels, 2, dtype=F32, seed=7, phi=quantum_phi(False), device=DEV)
    opt = FlatRMSprop(list(model.parameters()), lr=1e-4, alpha=0.9, momentum=0.9, weight_decay=1e-4)
    mon = BatchMonitor(DEV, 2, 10, (1, 8, 8, 2), kernel_size=3, period=1, capacity=8)
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src, iters_per_launch=2, monitor=mon)
    assert step.monitor is mon
    out = step()
    torch.cuda.synchronize(DEV)
    rows = mon.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(0, 0), (1, 1), (2, 2), (3, 3)] and mon.lost == 0
    for k, r in enumerate(rows):
        assert list(r["index"]) == src.expected_indices(k) and list(r["label"]) == [int(labels[i]) for i in r["index"]]
        assert r["rows"] == 2 and r["bad_rows"] == 0 and r["input"]["nonfinite"] == 0 and r["input"]["window_std"] > 0
    last = summarise(mirror(step.x, out["output"], step.y, out["indices"], 3), (1, 8, 8, 2), 2, 10, 3)
    assert np.array_equal(rows[3]["pred"], last["pred"]) and np.array_equal(rows[3]["hist"]["counts"], last["hist"]["counts"])
    for key in ("mean", "std", "window_mean", "window_std"):
        assert np.allclose(rows[3]["input"][key], last["input"][key]), key
    for key in ("min", "max", "mean", "std"):
        assert np.allclose(rows[3]["logits"][key], last["logits"][key]), key
    with pytest.raises(ValueError, match="QUANTUM"):
        GraphedTrainStep(model, torch.zeros(2, 1, 8, 8, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV),
                         fused_cross_entropy, opt, monitor=mon)
