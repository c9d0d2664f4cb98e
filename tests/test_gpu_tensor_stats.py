"""`dctn_tensor_stats` (csrc/sbs_tail.hip) and `tensor_stats.OutputStats` on the GPU (`-m gpu`).

Exact inputs are integers in [-1024, 1024] times 2^-4: every partial sum of values, squares and magnitudes is exact in
float64 in any order, so every field of the record must equal numpy's float64 values bit for bit, whatever the number of
workgroups, the form of the loads or the workgroup that happened to come last.  The counts cover one element, the wave and
workgroup edges, one / two / 65 workgroups (a lane of the last workgroup adds two slots) and the 256-workgroup cap (grid
stride)."""
import math

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd.tensor_stats import RECORD_BYTES, RECORD_DTYPE, OutputStats
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
COUNTS = [1, 63, 64, 65, 1023, 4095, 4096, 4097, 262147, 1052673]
DTYPES = [torch.float32, torch.float64]


def _exact(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, (n,), generator=g).double() / 16.0


def _launch(tensors, records, workspace):
    lib = L.lib()
    L.check(lib.dctn_tensor_stats(L.ptr_array(tensors), L.i64_array([t.numel() for t in tensors]), len(tensors),
                                  records.data_ptr(), workspace.data_ptr(), workspace.numel(), L.dtype_code(tensors[0]),
                                  L.stream_ptr(DEV)), "tensor statistics")


def _run(tensors, launches=1, fill=0xFF, workspace_fill=None):
    """`launches` launches over guarded buffers; the records of every launch as structured arrays."""
    seen = []
    with guarded(fill=fill) as arena:
        placed = [arena.place(t) if t.storage_offset() == 0 else t for t in tensors]
        records = arena.zeros((len(tensors) * RECORD_BYTES,), torch.uint8, DEV)
        workspace = arena.empty((L.lib().dctn_tensor_stats_workspace_bytes(len(tensors)),), torch.uint8, DEV)
        if workspace_fill is not None:
            workspace.copy_(workspace_fill[: workspace.numel()])
        for _ in range(launches):
            _launch(placed, records, workspace)
            seen.append(records.cpu().numpy().view(RECORD_DTYPE).copy())
    arena.check()
    for p, t in zip(placed, tensors):
        assert torch.equal(p, t) or not torch.isfinite(t).all()
    return seen


def _expected(values):
    """The record of `values` (a float64 numpy array holding the tensor's values exactly), numpy's float64 sums."""
    finite = values[np.isfinite(values)]
    a = np.abs(finite)
    return dict(n=values.size, sum=finite.sum(), sum_sq=(finite * finite).sum(), sum_abs=a.sum(),
                min_abs=np.float32(a.min()) if a.size else np.float32(np.inf), max_abs=np.float32(a.max()) if a.size else np.float32(0),
                nonfinite=values.size - finite.size)


def _assert_record(rec, want, seq):
    assert int(rec["n"]) == want["n"] and int(rec["nonfinite"]) == want["nonfinite"]
    for key in ("sum", "sum_sq", "sum_abs"):
        assert np.float64(rec[key]).tobytes() == np.float64(want[key]).tobytes(), (key, rec[key], want[key])
    for key in ("min_abs", "max_abs"):
        assert np.float32(rec[key]).tobytes() == np.float32(want[key]).tobytes(), (key, rec[key], want[key])
    assert int(rec["seq"]) == seq and int(rec["ticket"]) == 0 and not rec["reserved"].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", COUNTS)
def test_exact_inputs_give_numpys_float64_record_bit_for_bit(n, dtype):
    v = _exact(n, n)
    (recs,) = _run([v.to(dtype).to(DEV)])
    _assert_record(recs[0], _expected(v.numpy()), 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 65, 4097, 262147])
def test_a_view_one_element_into_its_storage_gives_the_same_record(n, dtype):
    """The unaligned pointer: one element per access, the same record as the aligned form."""
    v = _exact(n, 100 + n)
    with guarded(fill=0xFF) as arena:
        store = arena.empty((n + 1,), dtype, DEV)
    store[1:].copy_(v.to(dtype))
    view = store[1:]
    assert view.data_ptr() % 16 != 0
    (recs,) = _run([view])
    _assert_record(recs[0], _expected(v.numpy()), 1)
    arena.check()
    assert torch.isnan(store[0])
    r = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dtype)
    store[1:].copy_(r)
    (unaligned,), (aligned,) = _run([store[1:]]), _run([r.to(DEV)])
    assert unaligned.tobytes() == aligned.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_eight_tensors_in_one_launch_and_nine_through_output_stats(dtype):
    sizes = [1, 4097, 64, 262147, 1023, 5000, 65, 12289, 777]
    vals = [_exact(n, 200 + i) for i, n in enumerate(sizes)]
    (recs,) = _run([v.to(dtype).to(DEV) for v in vals[:8]])
    for rec, v in zip(recs, vals):
        _assert_record(rec, _expected(v.numpy()), 1)
    names = [f"t{i}" for i in range(9)]
    stats = OutputStats(DEV, names)
    tensors = [v.to(dtype).to(DEV) for v in vals]
    stats.record(tensors)
    stats.record(tensors)
    for rec, v in zip(stats.raw(), vals):
        _assert_record(rec, _expected(v.numpy()), 2)
    got = stats.read()
    for name, v, (n, s, ss) in zip(names, vals, stats.moments()):
        x = v.numpy()
        assert got[name]["n"] == x.size == n and got[name]["seq"] == 2 and got[name]["nonfinite"] == 0
        assert got[name]["mean"] == x.sum() / x.size and got[name]["mean_abs"] == np.abs(x).sum() / x.size
        assert got[name]["min_abs"] == np.abs(x).min() and got[name]["max_abs"] == np.abs(x).max()
        assert (s, ss) == (x.sum(), (x * x).sum())
        if x.size > 1:
            assert got[name]["std"] == pytest.approx(x.std(ddof=1), rel=1e-12)
        else:
            assert math.isnan(got[name]["std"])
    # CPU tensors are staged (the boundary rule) and give the same records
    staged = OutputStats(torch.device("cpu"), names)
    staged.record([v.to(dtype) for v in vals])
    staged.record([v.to(dtype) for v in vals])
    assert staged.raw().tobytes() == stats.raw().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4097, 262147, 1052673])
def test_random_inputs_are_within_the_float64_summation_bound(n, dtype):
    r = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dtype)
    (recs,) = _run([r.to(DEV)])
    x = r.double().numpy()
    rec = recs[0]
    for key, terms in (("sum", x), ("sum_sq", x * x), ("sum_abs", np.abs(x))):
        exact, bound = math.fsum(terms.tolist()), n * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
        print(f"\n{n} {key}: error {abs(float(rec[key]) - exact):.3e}, bound {bound:.3e}")
        assert abs(float(rec[key]) - exact) <= bound
    assert rec["min_abs"] == np.float32(np.abs(x).min()) and rec["max_abs"] == np.float32(np.abs(x).max())
    assert int(rec["n"]) == n and int(rec["nonfinite"]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_elements_are_counted_and_left_out(dtype):
    n = 3 * 4096 + 5
    v = _exact(n, 300)
    for at, bad in ((0, math.nan), (n - 1, math.inf), (4095, -math.inf), (4096, math.nan), (8191, math.inf)):
        v[at] = bad
    (recs,) = _run([v.to(dtype).to(DEV)])
    want = _expected(v.numpy())
    assert want["nonfinite"] == 5
    _assert_record(recs[0], want, 1)
    (recs,) = _run([torch.full((70,), math.nan, dtype=dtype, device=DEV)])
    _assert_record(recs[0], dict(n=70, sum=0.0, sum_sq=0.0, sum_abs=0.0, min_abs=np.float32(np.inf), max_abs=np.float32(0),
                                 nonfinite=70), 1)


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_five_launches_leave_five_identical_records_apart_from_seq(fill):
    """The workspace starts as NaN / as large finite values and is stale from the second launch on; the ticket reads 0
    after each launch."""
    vals = [_exact(262147, 400), _exact(4097, 401), _exact(7, 402)]
    seen = _run([v.float().to(DEV) for v in vals], launches=5, fill=fill)
    for k, recs in enumerate(seen):
        for rec, v in zip(recs, vals):
            _assert_record(rec, _expected(v.numpy()), k + 1)
    # a workspace left by a launch over OTHER tensors changes nothing either
    other = torch.randn(98304 // 4, generator=torch.Generator().manual_seed(9)).to(DEV).view(torch.uint8)
    (recs,) = _run([v.float().to(DEV) for v in vals], workspace_fill=other)
    for rec, v in zip(recs, vals):
        _assert_record(rec, _expected(v.numpy()), 1)


def test_replayed_from_a_captured_graph_seq_advances_per_replay():
    vals = [_exact(4097, 500), _exact(65, 501)]
    tensors = [v.float().to(DEV) for v in vals]
    stats = OutputStats(DEV, ["a", "b"])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        stats.record(tensors)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats.record(tensors)
    assert [r["seq"] for r in stats.read().values()] == [1, 1]   # a capture runs nothing
    for k in range(3):
        graph.replay()
        for rec, v in zip(stats.raw(), vals):
            _assert_record(rec, _expected(v.numpy()), 2 + k)
    tensors[1].mul_(2)   # the replay reads the tensors as they are now
    graph.replay()
    _assert_record(stats.raw()[1], _expected(vals[1].numpy() * 2), 5)
