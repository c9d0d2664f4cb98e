"""What the output histograms promise without a GPU: the exports of library version 519 and their pinned return codes (all
decided on the host before any launch), the block's layout, TensorBoard's bucket table, the numpy mirror of the kernel's
semantics against ``numpy.histogram``, the trimming of empty buckets and the logger's summary."""
import ctypes

import numpy as np
import pytest
import torch

from dctn_amd import _lib, training
from dctn_amd.tensor_hist import (COUNTERS, HEADER_BYTES, OutputHistograms, block_dtype, float_to_key, histogram_summary,
                                  key_to_float, reference_counts, tensorboard_edges, trim_buckets)

PTR = 4096   # any non-null, 16-byte aligned number: the calls below return before they would use it


def test_exports_version_and_block_layout():
    lib = _lib.lib()
    assert lib.dctn_version() >= 519
    for name in ("dctn_tensor_hist", "dctn_tensor_hist_block_bytes", "dctn_tensor_hist_reset"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # affine in n_edges: a header, then one uint64 per bin
    size = lib.dctn_tensor_hist_block_bytes
    assert size(2) == HEADER_BYTES + 8 and size(1) == size(0) == size(-3) == 0
    assert all(size(n) - size(n - 1) == 8 for n in range(3, 2049))
    for n in (2, 3, 1549, 2048):
        dt = block_dtype(n)
        assert dt.itemsize == size(n) and dt["counts"].shape == (n - 1,) and dt.fields["counts"][1] == HEADER_BYTES
    names = block_dtype(2).names
    assert names[:6] == COUNTERS and names[6:] == ("max_key", "min_key_c", "calls", "recorded", "ticket", "reserved", "counts")
    assert [block_dtype(2).fields[k][1] for k in ("total", "max_key", "min_key_c", "calls", "recorded", "ticket")] == [0, 48, 56, 64, 68, 72]


def test_tensor_hist_return_codes():
    lib = _lib.lib()
    ptrs, counts = (ctypes.c_void_p * 9)(*[PTR] * 9), (ctypes.c_int64 * 9)(*[5] * 9)

    def call(p=ptrs, c=counts, n=8, edges=PTR, n_edges=1549, blocks=PTR, period=1, dtype=_lib.F32):
        return lib.dctn_tensor_hist(p, c, n, edges, n_edges, blocks, period, dtype, None)

    assert call(p=None) == call(c=None) == call(edges=None) == call(blocks=None) == _lib.ERR_NULL
    assert call(n=9) == call(n=0) == call(n=-1) == _lib.ERR_BAD_SHAPE
    assert call(n_edges=1) == call(n_edges=2049) == call(n_edges=0) == _lib.ERR_BAD_SHAPE
    assert call(period=0) == call(period=-20) == _lib.ERR_BAD_SHAPE
    counts[3] = 0
    assert call() == _lib.ERR_BAD_SHAPE
    assert call(dtype=_lib.BF16) == _lib.ERR_BAD_SHAPE   # shape before dtype
    counts[3] = 5
    assert call(dtype=_lib.BF16) == call(dtype=7) == _lib.ERR_BAD_DTYPE
    assert call(dtype=_lib.BF16, period=0) == _lib.ERR_BAD_SHAPE
    # unsupported comes last: a count no workgroup's 32-bit LDS counts could hold, a misaligned table or block
    counts[0] = (1 << 39) + 1
    assert call() == _lib.ERR_UNSUPPORTED and call(dtype=_lib.BF16) == _lib.ERR_BAD_DTYPE
    counts[0] = 5
    assert call(edges=PTR + 4) == call(blocks=PTR + 4) == _lib.ERR_UNSUPPORTED
    ptrs[7] = None
    assert call() == _lib.ERR_NULL and call(n=7, n_edges=1) == _lib.ERR_BAD_SHAPE   # NULL first, and only among the n given
    reset = lambda blocks=PTR, n=3, n_edges=1549: lib.dctn_tensor_hist_reset(blocks, n, n_edges, None)
    assert reset(blocks=None) == _lib.ERR_NULL
    assert reset(n=0) == reset(n_edges=1) == reset(n_edges=2049) == _lib.ERR_BAD_SHAPE
    assert reset(blocks=PTR + 4) == reset(n=65536) == _lib.ERR_UNSUPPORTED


def test_tensorboard_edges_are_the_default_bucket_set():
    e = tensorboard_edges()
    assert e.dtype == np.float64 and e.shape == (1549,)
    pos = e[e > 0]
    assert pos.size == 774 and e[774] == 0.0 and np.array_equal(e[:774], -pos[::-1])
    assert (np.diff(e) > 0).all()
    assert pos[0] == 1e-12 and pos[-1] == 9.920775621859783e+19 and pos[-1] * 1.1 >= 1e20
    assert np.unique(e.astype(np.float32)).size == 1549
    # the rule itself: each edge is the one before times 1.1, in float64
    assert np.array_equal(pos[1:], pos[:-1] * 1.1)


def _probe(edges):
    """Every edge, its neighbours both ways, both zeros and the smallest subnormals - all inside the table's range."""
    v = np.concatenate([edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf), [0.0, -0.0, 5e-324, -5e-324]])
    return v[(v >= edges[0]) & (v <= edges[-1])]


@pytest.mark.parametrize("table", ["tensorboard", "two", "uneven"])
def test_reference_counts_is_numpys_histogram_inside_the_table(table):
    edges = {"tensorboard": tensorboard_edges(), "two": np.array([-1.5, 2.25]),
             "uneven": np.array([-3.0, -1.0, -0.5, 0.0, 1e-300, 7.0, 7.000000000000001])}[table]
    v = _probe(edges)
    got = reference_counts(v, edges)
    want, _ = np.histogram(v, bins=edges)
    assert np.array_equal(got["counts"], want) and got["counts"].sum() == v.size == got["total"]
    assert [got[k] for k in COUNTERS[1:]] == [0, 0, 0, 0, 0]
    assert got["min"] == edges[0] and got["max"] == edges[-1]
    # float32 input is widened exactly: the same as numpy's histogram of the widened values
    v32 = v.astype(np.float32)
    v32 = v32[(v32 >= edges[0]) & (v32 <= edges[-1])]
    assert np.array_equal(reference_counts(v32, edges)["counts"], np.histogram(v32.astype(np.float64), bins=edges)[0])


def test_reference_counts_outside_the_table_and_not_finite():
    edges = np.array([-2.0, 0.0, 1.0, 4.0])
    v = np.array([-2.0, np.nextafter(-2.0, -np.inf), -1e300, 4.0, np.nextafter(4.0, np.inf), 1e300, np.nan, np.nan, np.inf,
                  -np.inf, -np.inf, -np.inf, -0.0, 0.5, 1.0])
    got = reference_counts(v, edges)
    assert got["counts"].tolist() == [1, 2, 2] and got["total"] == 15
    assert (got["below"], got["above"], got["nan"], got["pos_inf"], got["neg_inf"]) == (2, 2, 2, 1, 3)
    assert got["min"] == -1e300 and got["max"] == 1e300
    empty = reference_counts(np.array([np.nan, np.inf]), edges)
    assert empty["min"] == np.inf and empty["max"] == -np.inf and empty["counts"].sum() == 0
    zero = reference_counts(np.array([-0.0]), edges)
    assert zero["counts"].tolist() == [0, 1, 0] and np.signbit(zero["min"]) == np.signbit(zero["max"]) == False  # noqa: E712
    with pytest.raises(ValueError):
        reference_counts(v, [0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        reference_counts(v, [0.0])
    with pytest.raises(ValueError):
        reference_counts(v, np.arange(2049.0))


def test_keys_keep_the_order_and_leave_zero_free():
    values = [-1.7976931348623157e308, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1.7976931348623157e308]
    keys = [float_to_key(v) for v in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(0 < k < (1 << 64) - 1 for k in keys)
    assert [key_to_float(k) for k in keys] == values


def test_trim_buckets_cuts_like_make_histogram():
    edges = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    # the support starts inside the table: the bucket left of it is kept, empty, for its right limit
    assert trim_buckets([0, 0, 3, 0, 2], edges) == ([2.0, 3.0, 4.0, 5.0], [0, 3, 0, 2])
    assert trim_buckets([0, 4, 1, 0, 0], edges) == ([1.0, 2.0, 3.0], [0, 4, 1])
    # the support starts at the first bucket: an empty bucket is put in front
    assert trim_buckets([5, 0, 1, 0, 0], edges) == ([0.0, 1.0, 2.0, 3.0], [0, 5, 0, 1])
    assert trim_buckets([0, 0, 0, 0, 9], edges) == ([4.0, 5.0], [0, 9])
    # an empty histogram keeps the first bucket, as make_histogram's arithmetic does
    assert trim_buckets([0, 0, 0, 0, 0], edges) == ([0.0, 1.0], [0, 0])
    # against numpy.histogram on TensorBoard's table: what is cut holds nothing
    table = tensorboard_edges()
    v = np.random.default_rng(0).standard_normal(5000)
    counts, _ = np.histogram(v, bins=table)
    limits, kept = trim_buckets(counts, table)
    assert len(limits) == len(kept) and sum(kept) == 5000 and kept[0] == 0 and kept[1] > 0 and kept[-1] > 0
    first = int(np.flatnonzero(counts)[0])
    assert limits[0] == table[first] and limits[-1] == table[int(np.flatnonzero(counts)[-1]) + 1]


class _FakeHists:
    """What the logger needs of an `OutputHistograms`: edges, and read(reset=True)."""

    def __init__(self, edges, entries):
        self.edges, self.entries, self.reads = edges, entries, []

    def read(self, reset=False):
        self.reads.append(reset)
        return self.entries


def test_the_logger_hands_the_sink_add_histogram_raws_arguments():
    edges = np.array([-4.0, -1.0, 0.0, 1.0, 4.0, 16.0])
    v = np.array([-2.0, -2.0, 0.5, 2.0, 2.0, 2.0, 8.0, 100.0, np.nan])
    entry = dict(reference_counts(v, edges), calls=6, recorded=2)
    hists = _FakeHists(edges, {"a": entry, "b": dict(reference_counts(np.array([3.0]), edges), calls=6, recorded=2)})
    seen = []
    hook = training.make_histogram_logger(hists, 3, lambda name, summary, n: seen.append((name, summary, n)))
    for launch in range(7):
        hook({}, {"num_iters_done": 2 * launch + 1})
    assert hists.reads == [True, True] and [(n, it) for n, _, it in seen] == [("a", 5), ("b", 5), ("a", 11), ("b", 11)]
    s = seen[0][1]
    assert set(s) == {"min", "max", "num", "sum", "sum_squares", "bucket_limits", "bucket_counts"}
    assert (s["min"], s["max"], s["num"]) == (-2.0, 100.0, 9)
    assert (s["bucket_limits"], s["bucket_counts"]) == ([-4.0, -1.0, 0.0, 1.0, 4.0, 16.0], [0, 2, 0, 1, 3, 1])
    # geometric centres: -2 for [-4, -1), 0 for the buckets at 0, 2 for [1, 4), 8 for [4, 16]: here they are the values
    assert s["sum"] == 2 * -2.0 + 0.0 + 3 * 2.0 + 8.0 and s["sum_squares"] == 2 * 4.0 + 3 * 4.0 + 64.0
    assert histogram_summary(entry, edges) == s
    assert seen[1][1]["bucket_limits"] == [1.0, 4.0] and seen[1][1]["bucket_counts"] == [0, 1]
    hook.flush(99)
    assert hists.reads == [True] * 3 and seen[-1][2] == 99


def test_output_histograms_checks_its_arguments_before_it_needs_a_device():
    for bad in (dict(names=[]), dict(names=["a", "a"]), dict(names=["a"], period=0), dict(names=["a"], edges=[1.0]),
                dict(names=["a"], edges=[0.0, 1.0, 1.0]), dict(names=["a"], edges=[0.0, np.inf])):
        with pytest.raises(ValueError):
            OutputHistograms(torch.device("cpu"), **bad)


@pytest.mark.skipif(torch.cuda.is_available(), reason="what the calls do where there is no GPU")
def test_without_a_gpu_the_constructor_raises():
    with pytest.raises(RuntimeError):
        OutputHistograms(torch.device("cpu"), ["a"])
