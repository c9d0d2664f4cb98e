"""`dctn_tensor_hist` (csrc/tensor_hist.hip) and `tensor_hist.OutputHistograms` on the GPU (`-m gpu`).

Everything a block holds is an integer sum or a max, so every comparison here is `==` against ``numpy.histogram`` and its
mirror `reference_counts`: no tolerance applies anywhere.  The element counts cover one element, the four-element access
and its tail, one / two / four workgroups, the 256-workgroup cap with more than one round per workgroup, and both forms of
the load; the values cover every edge of TensorBoard's table and its neighbours in both dtypes."""
import functools
import math

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd.tensor_hist import COUNTERS, OutputHistograms, block_dtype, float_to_key, reference_counts, tensorboard_edges
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
COUNTS = [1, 3, 4, 5, 4095, 4096, 4097, 12289, 262147, 1052673]
TB = tensorboard_edges()
MASK = (1 << 64) - 1


def _launch(tensors, blocks, edges_dev, period=1):
    L.check(L.lib().dctn_tensor_hist(L.ptr_array(tensors), L.i64_array([t.numel() for t in tensors]), len(tensors),
                                     edges_dev.data_ptr(), edges_dev.numel(), blocks.data_ptr(), period, L.dtype_code(tensors[0]),
                                     L.stream_ptr(DEV)), "tensor histograms")


def _run(tensors, edges=TB, period=1, launches=1, fill=0xFF):
    """`launches` launches over guarded buffers; the blocks after each launch as structured arrays.  The tensors, the table
    and a decoy buffer of `fill` bytes must come out as they went in."""
    seen = []
    with guarded(fill=fill) as arena:
        placed = [arena.place(t) if t.storage_offset() == 0 else t for t in tensors]
        edges_dev = arena.place(torch.from_numpy(np.asarray(edges, dtype=np.float64).copy()).to(DEV))
        decoy = arena.empty((4096,), torch.uint8, DEV)
        blocks = arena.zeros((len(tensors) * block_dtype(len(edges)).itemsize,), torch.uint8, DEV)
        before = [p.clone() for p in placed]
        for _ in range(launches):
            _launch(placed, blocks, edges_dev, period)
            seen.append(blocks.cpu().numpy().view(block_dtype(len(edges))).copy())
    arena.check()
    for p, b in zip(placed, before):
        assert torch.equal(p.view(torch.uint8), b.view(torch.uint8))
    assert bool((decoy == fill).all()) and np.array_equal(edges_dev.cpu().numpy(), np.asarray(edges, dtype=np.float64))
    return seen


def _total(parts):
    """The sum of several `reference_counts` results: what the block holds after those recorded launches."""
    out = {k: sum(p[k] for p in parts) for k in ("counts",) + COUNTERS}
    out["min"], out["max"] = min(p["min"] for p in parts), max(p["max"] for p in parts)
    return out


def _assert_block(rec, want, calls=1, recorded=1):
    assert np.array_equal(rec["counts"].astype(np.int64), want["counts"]), np.flatnonzero(rec["counts"].astype(np.int64) != want["counts"])
    for key in COUNTERS:
        assert int(rec[key]) == want[key], (key, int(rec[key]), want[key])
    have = math.isfinite(want["min"])
    assert int(rec["max_key"]) == (float_to_key(want["max"]) if have else 0), (int(rec["max_key"]), want["max"])
    assert int(rec["min_key_c"]) == (~float_to_key(want["min"]) & MASK if have else 0), (int(rec["min_key_c"]), want["min"])
    assert (int(rec["calls"]), int(rec["recorded"]), int(rec["ticket"]), int(rec["reserved"])) == (calls, recorded, 0, 0)


@functools.lru_cache(maxsize=None)
def _values(n, seed=0):
    """exp(uniform(-30, 30)) with a random sign, float64: some fifty decades around 1, inside TensorBoard's table."""
    rng = np.random.default_rng(1000 * seed + n)
    v = np.exp(rng.uniform(-30.0, 30.0, n)) * rng.choice([-1.0, 1.0], n)
    v.setflags(write=False)
    return v


def _tensor(v, dtype):
    return torch.from_numpy(np.array(v)).to(dtype).to(DEV)


def test_every_edge_and_its_neighbours_in_float64():
    """The first edge closed on the left, every inner edge the start of its bin, the last bin closed on the right, and
    what lies outside counted in `below` / `above` and the three not-finite counters."""
    v = np.concatenate([TB, np.nextafter(TB, np.inf), np.nextafter(TB, -np.inf),
                        [0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300, np.inf, -np.inf, np.nan]])
    (recs,) = _run([_tensor(v, torch.float64)])
    want = reference_counts(v, TB)
    _assert_block(recs[0], want)
    inside = v[np.isfinite(v) & (v >= TB[0]) & (v <= TB[-1])]
    assert np.array_equal(recs[0]["counts"].astype(np.int64), np.histogram(inside, bins=TB)[0])
    assert (want["below"], want["above"], want["nan"], want["pos_inf"], want["neg_inf"]) == (2, 2, 1, 1, 1)
    # the first bin: its edge, the edge's upper neighbour, the next edge's lower neighbour; the last bin holds both of its
    # edges, closed on the right
    assert recs[0]["counts"][0] == 3 and recs[0]["counts"][-1] == 4
    # bin 774 starts at 0.0: both zeros, the edge itself, its upper neighbour and 5e-324 (which is that neighbour), and
    # the lower neighbour of the next edge
    assert recs[0]["counts"][774] == 6 and recs[0]["counts"][773] == 4


def test_every_edges_float32_rounding_and_its_float32_neighbours():
    e32 = TB.astype(np.float32)
    v32 = np.concatenate([e32, np.nextafter(e32, np.float32(np.inf)), np.nextafter(e32, np.float32(-np.inf))])
    (recs,) = _run([torch.from_numpy(v32).to(DEV)])
    wide = v32.astype(np.float64)
    want = reference_counts(wide, TB)
    _assert_block(recs[0], want)
    inside = wide[(wide >= TB[0]) & (wide <= TB[-1])]
    assert np.array_equal(recs[0]["counts"].astype(np.int64), np.histogram(inside, bins=TB)[0])
    assert int(recs[0]["below"]) == 1 and int(recs[0]["above"]) == 1   # as numpy has it: the outer neighbours of the ends
    # a rounding that falls below its edge lands one bin lower: every edge alone, against the table
    fell = np.flatnonzero(e32.astype(np.float64) < TB)
    assert 100 < fell.size < 1449
    bins = np.searchsorted(TB, e32.astype(np.float64), side="right") - 1
    assert np.array_equal(bins[fell], fell - 1) and np.array_equal(np.delete(bins, fell), np.delete(np.arange(1549), fell))
    (alone,) = _run([torch.from_numpy(e32[fell]).to(DEV)])
    assert np.array_equal(np.flatnonzero(alone[0]["counts"]), fell - 1) and int(alone[0]["counts"].sum()) == fell.size


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", COUNTS)
def test_every_partition_counts_what_numpy_counts(n, dtype):
    t = _tensor(_values(n), dtype)
    (recs,) = _run([t])
    wide = t.double().cpu().numpy()
    _assert_block(recs[0], reference_counts(wide, TB))
    assert np.array_equal(recs[0]["counts"].astype(np.int64), np.histogram(wide, bins=TB)[0]) and int(recs[0]["total"]) == n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 5, 4097, 262147])
def test_a_view_one_element_into_its_storage_gives_the_same_block(n, dtype):
    """The unaligned pointer: one element per access, the same block as the aligned form."""
    t = _tensor(_values(n, seed=1), dtype)
    with guarded(fill=0xFF) as arena:
        store = arena.empty((n + 1,), dtype, DEV)
    store[1:].copy_(t)
    view = store[1:]
    assert view.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    (unaligned,), (aligned,) = _run([view]), _run([t])
    arena.check()
    assert torch.isnan(store[0])
    assert unaligned.tobytes() == aligned.tobytes()
    _assert_block(unaligned[0], reference_counts(t.double().cpu().numpy(), TB))


@pytest.mark.parametrize("dtype", DTYPES)
def test_contention_one_bin_and_two_adjacent_bins(dtype):
    ones = np.ones(100000)
    pair = np.where(np.arange(100000) % 2 == 0, 1.0, 1.05)   # 1.0 and 1.05 fall in adjacent buckets
    got = _run([_tensor(ones, dtype), _tensor(pair, dtype)])[0]
    _assert_block(got[0], reference_counts(ones, TB))
    _assert_block(got[1], reference_counts(_tensor(pair, dtype).double().cpu().numpy(), TB))
    assert np.count_nonzero(got[0]["counts"]) == 1 and int(got[0]["counts"].max()) == 100000
    hit = np.flatnonzero(got[1]["counts"])
    assert hit.size == 2 and hit[1] == hit[0] + 1 and got[1]["counts"][hit].tolist() == [50000, 50000]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", ["two", "full"])
def test_the_smallest_and_the_largest_edge_table(table, dtype):
    edges = np.array([-0.5, 0.75]) if table == "two" else np.linspace(-3.0, 3.0, 2048)
    v = np.random.default_rng(5).standard_normal(20001) * 2.0
    v[:4] = [edges[0], edges[-1], np.nextafter(edges[0], -np.inf), np.nextafter(edges[-1], np.inf)]
    t = _tensor(v, dtype)
    (recs,) = _run([t], edges=edges)
    want = reference_counts(t.double().cpu().numpy(), edges)
    assert want["below"] > 100 and want["above"] > 100 and want["counts"].sum() > 1000
    _assert_block(recs[0], want)
    assert recs[0]["counts"].shape == (len(edges) - 1,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_eight_tensors_in_one_launch_and_nine_through_output_histograms(dtype):
    sizes = [1, 4097, 64, 262147, 1023, 5000, 65, 12289, 777]
    vals = [_values(n, seed=2 + i) for i, n in enumerate(sizes)]
    tensors = [_tensor(v, dtype) for v in vals]
    wants = [reference_counts(t.double().cpu().numpy(), TB) for t in tensors]
    (recs,) = _run(tensors[:8])
    for rec, want in zip(recs, wants):
        _assert_block(rec, want)
    names = [f"t{i}" for i in range(9)]
    hists = OutputHistograms(DEV, names)
    hists.record(tensors)
    for rec, want in zip(hists.raw(), wants):
        _assert_block(rec, want)
    got = hists.read()
    assert list(got) == names
    for name, want in zip(names, wants):
        entry = got[name]
        assert np.array_equal(entry["counts"], want["counts"]) and entry["counts"].dtype == np.int64
        assert {k: entry[k] for k in COUNTERS + ("min", "max")} == {k: want[k] for k in COUNTERS + ("min", "max")}
        assert (entry["calls"], entry["recorded"]) == (1, 1)
    limits, kept = hists.trimmed("t3")
    assert sum(kept) == sizes[3] and kept[0] == 0 and kept[1] > 0 and kept[-1] > 0 and len(limits) == len(kept)
    # CPU tensors are staged (the boundary rule) and give the same blocks; a strided tensor is made contiguous
    staged = OutputHistograms(torch.device("cpu"), names)
    staged.record([t.cpu() for t in tensors])
    assert staged.raw().tobytes() == hists.raw().tobytes()
    strided = OutputHistograms(DEV, ["s"])
    strided.record([tensors[1][::2]])
    _assert_block(strided.raw()[0], reference_counts(tensors[1][::2].double().cpu().numpy(), TB))
    with pytest.raises(TypeError):
        hists.record([t.bfloat16() for t in tensors])
    with pytest.raises(ValueError):
        hists.record(tensors[:8])


def test_two_records_add_up_and_reset_empties_the_block_but_keeps_calls():
    a, b = _values(12289, seed=20), np.concatenate([_values(5000, seed=21), [np.nan, np.inf, -np.inf, 1e300, -1e300]])
    wa, wb = reference_counts(a, TB), reference_counts(b, TB)
    hists = OutputHistograms(DEV, ["x"])
    hists.record([_tensor(a, torch.float64)])
    _assert_block(hists.raw()[0], wa, 1, 1)
    hists.record([_tensor(b, torch.float64)])
    _assert_block(hists.raw()[0], _total([wa, wb]), 2, 2)
    assert hists.read()["x"]["min"] == -1e300 and hists.read()["x"]["max"] == 1e300
    hists.reset()
    empty = reference_counts(np.zeros(0), TB)
    _assert_block(hists.raw()[0], empty, 2, 0)
    assert hists.read()["x"]["min"] == math.inf and hists.read()["x"]["max"] == -math.inf
    hists.record([_tensor(a, torch.float64)])
    _assert_block(hists.raw()[0], wa, 3, 1)
    assert hists.read(reset=True)["x"]["total"] == a.size
    _assert_block(hists.raw()[0], empty, 3, 0)
    # launches over guarded buffers: the raw entry point accumulates the same way, whatever the bytes around the blocks
    seen = _run([_tensor(a, torch.float32)], launches=3)
    w32 = reference_counts(_tensor(a, torch.float32).double().cpu().numpy(), TB)
    for k, recs in enumerate(seen):
        _assert_block(recs[0], _total([w32] * (k + 1)), k + 1, k + 1)


def test_a_period_of_three_records_calls_0_3_6_and_survives_a_reset():
    sizes = [4097, 70, 262147, 5, 12289, 1, 8192, 333, 4096, 40000]
    vals = [_values(n, seed=30 + i) for i, n in enumerate(sizes)]
    wants = [reference_counts(v, TB) for v in vals]
    hists = OutputHistograms(DEV, ["x"], period=3)
    for k in range(7):
        hists.record([_tensor(vals[k], torch.float64)])
    _assert_block(hists.raw()[0], _total([wants[0], wants[3], wants[6]]), 7, 3)
    got = hists.read()["x"]
    assert (got["calls"], got["recorded"], got["total"]) == (7, 3, sizes[0] + sizes[3] + sizes[6])
    hists.reset()
    hists.record([_tensor(vals[7], torch.float64)])   # call 7: not recorded
    _assert_block(hists.raw()[0], reference_counts(np.zeros(0), TB), 8, 0)
    hists.record([_tensor(vals[8], torch.float64)])   # call 8: not recorded
    hists.record([_tensor(vals[9], torch.float64)])   # call 9, the tenth: recorded
    _assert_block(hists.raw()[0], wants[9], 10, 1)


def test_replayed_from_a_captured_graph_the_counts_add_up():
    vals = [np.stack([_values(4097, seed=40 + k), _values(4097, seed=50 + k)]) for k in range(4)]
    static = _tensor(vals[0], torch.float32)
    hists = OutputHistograms(DEV, ["a", "b"])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        hists.record(list(static.unbind(0)))
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hists.record(list(static.unbind(0)))
    widened = [_tensor(v, torch.float32).double().cpu().numpy() for v in vals]
    parts = [[reference_counts(w[i], TB) for w in widened] for i in range(2)]
    for i in range(2):   # a capture runs nothing
        _assert_block(hists.raw()[i], parts[i][0], 1, 1)
    for k in range(1, 4):
        static.copy_(_tensor(vals[k], torch.float32))   # the replay reads the tensors as they are now
        graph.replay()
        for i in range(2):
            _assert_block(hists.raw()[i], _total(parts[i][:k + 1]), 1 + k, 1 + k)


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_nothing_outside_the_blocks_is_written_and_the_tensors_keep_their_bits(fill):
    """Guards of 0xFF around every tensor, the table and the blocks, a neighbour of `fill` bytes; three launches at period
    2, so that a skipped launch is held to the contract as well."""
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -1e300])
    vals = [np.concatenate([_values(4097, seed=60), special]), _values(3, seed=61), _values(262147, seed=62)]
    for dtype in DTYPES:
        tensors = [_tensor(v, dtype) for v in vals]
        wants = [reference_counts(t.double().cpu().numpy(), TB) for t in tensors]
        seen = _run(tensors, period=2, launches=3, fill=fill)
        for k, recorded in enumerate([1, 1, 2]):
            for rec, want in zip(seen[k], wants):
                _assert_block(rec, _total([want] * recorded), k + 1, recorded)


def _model(seed=3):
    from dctn_amd.conv_sbs import DumbNormalInitialization
    from dctn_amd.mnist_model import DCTNMnistModel

    torch.manual_seed(seed)
    return DCTNMnistModel(2, 2, False, DumbNormalInitialization(0.9), False, 1.0).to(DEV)


def test_the_model_records_every_strings_output_in_an_eager_training_forward():
    model, plain = _model(), _model()
    x = torch.rand(2, 1, 8, 8, generator=torch.Generator().manual_seed(4)).to(DEV)
    names = model.string_names()
    assert len(names) == 3
    model.output_histograms = OutputHistograms(DEV, names)
    model.train(), plain.train()
    with torch.no_grad():
        logits, want_logits = model(x), plain(x)
        assert torch.equal(logits, want_logits)
        outputs, stacked = [], model._quantum(x)
        for layer in model.conv_sbses:
            stacked = layer.forward_stacked(stacked)
            outputs.extend(stacked.unbind(0))
    got = model.output_histograms.read()
    assert list(got) == names
    for name, y in zip(names, outputs):
        want = reference_counts(y.double().cpu().numpy(), TB)
        entry = got[name]
        assert np.array_equal(entry["counts"], want["counts"])
        assert {k: entry[k] for k in COUNTERS + ("min", "max")} == {k: want[k] for k in COUNTERS + ("min", "max")}
        assert (entry["calls"], entry["recorded"]) == (1, 1) and entry["total"] == y.numel() > 0
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(x), want_logits)
    assert all(e["calls"] == 1 for e in model.output_histograms.read().values())   # an eval forward records nothing


def test_the_model_under_a_graphed_step_of_two_iterations_per_launch():
    from dctn_amd import batches
    from dctn_amd.mnist_model import quantum_phi
    from dctn_amd.training import FlatRMSprop, GraphedTrainStep, fused_cross_entropy

    g = torch.Generator().manual_seed(6)
    images, labels = torch.randint(0, 256, (8, 8, 8), generator=g, dtype=torch.uint8), torch.randint(0, 10, (8,), generator=g)

    def run(with_histograms):
        model = _model()
        src = batches.DeviceBatches(images, labels, 2, dtype=torch.float32, seed=7, phi=quantum_phi(False), device=DEV)
        opt = FlatRMSprop(list(model.parameters()), lr=1e-4, alpha=0.9, momentum=0.9, weight_decay=1e-4)
        if with_histograms:
            model.output_histograms = OutputHistograms(DEV, model.string_names(), period=1)
        step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src, iters_per_launch=2)
        if with_histograms:
            assert [e["recorded"] for e in model.output_histograms.read(reset=True).values()] == [2] * 3   # the warm-up
        out = step()
        torch.cuda.synchronize()
        return model, opt, float(out["loss"].detach())

    model, opt, loss = run(True)
    plain_model, plain_opt, plain_loss = run(False)
    got = model.output_histograms.read()
    elements = {"conv_sbses.0.strings.0": 2 * 6 * 6 * 2, "conv_sbses.0.strings.1": 2 * 6 * 6 * 2, "conv_sbses.1.strings.0": 2 * 4 * 4 * 10}
    for name, entry in got.items():
        assert entry["total"] == 2 * elements[name] and (entry["calls"], entry["recorded"]) == (4, 2)
        inside = int(entry["counts"].sum())
        assert inside + entry["below"] + entry["above"] + entry["nan"] + entry["pos_inf"] + entry["neg_inf"] == entry["total"]
        assert inside > 0 and entry["min"] <= entry["max"]
    assert loss == plain_loss and opt.t == plain_opt.t == 4
    for key in ("flat", "square_avg", "buf"):
        assert torch.equal(getattr(opt, key), getattr(plain_opt, key)), key
    for p, q in zip(model.parameters(), plain_model.parameters()):
        assert torch.equal(p, q)
