"""`dctn_param_stats` (csrc/param_stats.hip) and `param_stats.ParamStats` on the GPU (`-m gpu`).

The kernel works in float64 throughout.  On values k / 64 with |k| <= 1024 (k / 8 with |k| <= 128 in bfloat16) every
partial sum of values is a multiple of 2^-6 below 2^31 and every partial sum of squares a multiple of 2^-12 below 2^40
(2^20 per element, at most 2^20 elements): exact in a double in any order, so the comparison is `==` against numpy
integer arithmetic.  The rounding tests use the standard bound for a sum in ANY order, |error| <= n 2^-53 sum |term|,
against `math.fsum` of the exact terms.

The plan's boundaries (csrc/param_stats.hip): a group is 4 elements, one pass of a workgroup 1024, a segment gains a
workgroup per 8192 elements up to 64.  Thread j of a segment's 256 W threads owns the groups j, j + 256 W, ...: the
elements 1023 | 1024 lie on either side of the boundary between workgroups 0 and 1 of a segment with W >= 2."""
import functools
import math

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd.param_stats import CELL, ParamStats, block_dtype, cell_moments, workspace_bytes
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -53
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 64 * 8192 - 1, 64 * 8192, 64 * 8192 + 1)
MODES = {"f32": (F32, False), "f64": (F64, False), "bf16": (BF16, False), "bf16_master": (BF16, True)}
HALVES = (("w_", "weights"), ("g_", "grads"))


def launch(weights, grads, sizes, dtype, master=None, period=1, capacity=1, launches=1, workspace_fill=0xFF, between=None,
           calls=0):
    """`launches` launches over guarded buffers; the block after each one as a structured element.  ``weights`` /
    ``grads`` / ``master``: numpy arrays of sum(sizes) values that `dtype` (float32 for the master) holds exactly.  The
    three buffers and a decoy must come out as they went in (``between(k, params, master)`` may rewrite them after launch
    k), and the workspace is exactly as large as the library asks."""
    ends = np.cumsum(sizes).tolist()
    n, k = ends[-1], len(sizes)
    assert len(weights) == len(grads) == n
    lib, c_ends = L.lib(), L.i64_array(ends)
    block_bytes, ws_bytes = lib.dctn_param_stats_block_bytes(k, capacity), lib.dctn_param_stats_workspace_bytes(c_ends, k)
    assert block_bytes == block_dtype(k, capacity).itemsize and ws_bytes == workspace_bytes(ends)
    seen = []
    with guarded(fill=workspace_fill) as arena:
        params = arena.place(torch.from_numpy(np.asarray(weights)).to(dtype).to(DEV))
        g = arena.place(torch.from_numpy(np.asarray(grads)).to(dtype).to(DEV))
        m = None if master is None else arena.place(torch.from_numpy(np.asarray(master)).to(F32).to(DEV))
        decoy = arena.empty((4096,), torch.uint8, DEV)
        block = arena.zeros((block_bytes,), torch.uint8, DEV)
        if calls:
            block[:4] = torch.from_numpy(np.array([calls], dtype="<u4").view(np.uint8).copy()).to(DEV)
        ws = arena.empty((ws_bytes,), torch.uint8, DEV)
        before = [t.clone() for t in (params, g) + (() if m is None else (m,))]
        for i in range(launches):
            L.check(lib.dctn_param_stats(params.data_ptr(), None if m is None else m.data_ptr(), g.data_ptr(), c_ends, k,
                                         block.data_ptr(), capacity, period, ws.data_ptr(), ws_bytes, L.dtype_code(params),
                                         L.stream_ptr(DEV)), "parameter statistics")
            seen.append(block.cpu().numpy().view(block_dtype(k, capacity))[0].copy())
            for t, b in zip((params, g) + (() if m is None else (m,)), before):
                assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "an input buffer changed"
            if between is not None:
                between(i, params, m)
                before = [t.clone() for t in (params, g) + (() if m is None else (m,))]
        ws_after = ws.clone()
    arena.check()
    assert bool((decoy == workspace_fill).all())
    launch.last_workspace = ws_after
    return seen


# ------------------------------------------------------------------ 1. exact
def _units(dtype):
    """(largest |k|, divisor): the values are k / divisor."""
    return (128, 8) if dtype == BF16 else (1024, 64)


@functools.lru_cache(maxsize=None)
def _exact_values(mode, seed=1):
    """Integer numerators (weights, grads, master) for every segment of SIZES, drawn once and shared."""
    dtype, with_master = MODES[mode]
    top, _ = _units(dtype)
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    return (rng.integers(-top, top + 1, size=n), rng.integers(-top, top + 1, size=n),
            rng.integers(-1024, 1025, size=n) if with_master else None)


def _exact_cell(kw, kg, div_w, div_g, finite_w=None, finite_g=None):
    """The cell numpy integer arithmetic gives for numerators kw / kg (int64); `finite_*`: masks of the finite elements."""
    cell = np.zeros((), dtype=CELL)
    for prefix, k, div, mask in (("w_", kw, div_w, finite_w), ("g_", kg, div_g, finite_g)):
        bad = 0 if mask is None else int((~mask).sum())
        k = k if mask is None else k[mask]
        cell[prefix + "sum"] = float(int(k.sum())) / div
        cell[prefix + "sum_sq"] = float(int((k * k).sum())) / (div * div)
        cell[prefix + "max_abs"] = float(int(np.abs(k).max())) / div if k.size else 0.0
        cell[prefix + "nonfinite"] = bad
    return cell


@pytest.mark.parametrize("mode", list(MODES))
def test_exact_values_give_numpys_integer_sums_together_and_alone(mode):
    dtype, with_master = MODES[mode]
    kw, kg, km = _exact_values(mode)
    _, div = _units(dtype)
    div_w = 64 if with_master else div
    kweights = km if with_master else kw   # with a master copy the weight cells are the master's, not the parameters'
    assert int((kweights.astype(np.int64) ** 2).sum()) < 2 ** 40 and not (with_master and np.array_equal(kw, km))
    (together,) = launch(kw / div, kg / div, SIZES, dtype, master=None if km is None else km / 64)
    assert (int(together["calls"]), int(together["recorded"]), int(together["ticket"])) == (1, 1, 0)
    assert (int(together["rows"][0]["call"]), int(together["rows"][0]["seq"]), int(together["rows"][0]["reserved"])) == (0, 0, 0)
    off = 0
    for s, c in enumerate(SIZES):
        sl = slice(off, off + c)
        off += c
        want = _exact_cell(kweights[sl].astype(np.int64), kg[sl].astype(np.int64), div_w, div)
        got = together["rows"][0]["cells"][s]
        assert got.tobytes() == want.tobytes(), (mode, c, got, want)
        (alone,) = launch(kw[sl] / div, kg[sl] / div, (c,), dtype, master=None if km is None else km[sl] / 64)
        assert alone["rows"][0]["cells"][0].tobytes() == want.tobytes(), (mode, c, "alone")


# ------------------------------------------------------------------ 2. placement
@pytest.mark.parametrize("mode", list(MODES))
def test_a_segments_cell_does_not_depend_on_where_the_segment_lies(mode):
    dtype, with_master = MODES[mode]
    rng = np.random.default_rng(2)
    a, b = 8193, 70001
    w = torch.from_numpy(rng.normal(size=a + b)).to(dtype).double().numpy()
    g = torch.from_numpy(rng.normal(size=a + b) * 1e-2).to(dtype).double().numpy()
    m = rng.normal(size=a + b).astype(np.float32).astype(np.float64) if with_master else None

    def run(sizes, at):
        """The cells of segments a and b, placed at the segment indices `at` among `sizes` (the rest: other values)."""
        ends = np.concatenate(([0], np.cumsum(sizes)))
        n = int(ends[-1])
        fill = np.random.default_rng(len(sizes))
        bufs = [torch.from_numpy(fill.normal(size=n)).to(dtype).double().numpy() for _ in range(2)]
        bufs.append(fill.normal(size=n).astype(np.float32).astype(np.float64) if with_master else None)
        for idx, sl in zip(at, (slice(0, a), slice(a, a + b))):
            if idx is not None:
                assert sizes[idx] == sl.stop - sl.start
                for buf, src in zip(bufs, (w, g, m)):
                    if buf is not None:
                        buf[ends[idx]: ends[idx + 1]] = src[sl]
        (raw,) = launch(bufs[0], bufs[1], sizes, dtype, master=bufs[2])
        return [None if idx is None else raw["rows"][0]["cells"][idx].tobytes() for idx in at]

    want = run((a,), (0, None))[0], run((b,), (None, 0))[1]
    assert want[0] != want[1]
    for lead in range(8):   # every alignment of 2-, 4- and 8-byte elements against 16 bytes; b sits lead + 8193 further
        sizes, at = ((a, b), (0, 1)) if lead == 0 else ((lead, a, b), (1, 2))
        assert tuple(run(sizes, at)) == want, (mode, "lead", lead)
    small = [int(s) for s in np.random.default_rng(3).integers(1, 300, size=64)]
    for ia, ib in ((0, 63), (31, 0), (63, 32)):   # first, middle and last of 64 segments
        sizes = list(small)
        sizes[ia], sizes[ib] = a, b
        assert tuple(run(tuple(sizes), (ia, ib))) == want, (mode, "place", ia, ib)


# ------------------------------------------------------------------ 3. rounding
def _exact_squares(x):
    """x * x as an unevaluated sum p + e of two float64 arrays (Dekker's product): fsum over both is the exact sum."""
    p = x * x
    c = 134217729.0 * x   # 2^27 + 1
    hi = c - (c - x)
    lo = x - hi
    return p, ((hi * hi - p) + 2.0 * hi * lo) + lo * lo


@pytest.mark.parametrize("dtype", [F32, F64])
def test_random_segments_stay_inside_the_bound_of_any_summation_order(dtype):
    """|sum - fsum(x)| <= n 2^-53 sum |x| and |sum_sq - fsum(x^2)| <= n 2^-53 sum x^2: derived, not measured."""
    rng = np.random.default_rng(4)
    sizes = (70001, 600001)
    w = torch.from_numpy(rng.normal(0.1, 1.0, size=sum(sizes))).to(dtype).double().numpy()
    g = torch.from_numpy(rng.normal(0.0, 1e-3, size=sum(sizes))).to(dtype).double().numpy()
    (raw,) = launch(w, g, sizes, dtype)
    off = 0
    for s, n in enumerate(sizes):
        cell = raw["rows"][0]["cells"][s]
        for prefix, x in (("w_", w[off: off + n]), ("g_", g[off: off + n])):
            p, e = _exact_squares(x)
            total, sq = math.fsum(x), math.fsum(np.concatenate((p, e)))
            abs_sum = math.fsum(np.abs(x))
            err, err_sq = abs(float(cell[prefix + "sum"]) - total), abs(float(cell[prefix + "sum_sq"]) - sq)
            print(f"{dtype} n={n} {prefix}: sum err {err:.3e} bound {n * U * abs_sum:.3e}; sum_sq err {err_sq:.3e} bound {n * U * sq:.3e}")
            assert err <= n * U * abs_sum and err_sq <= n * U * sq
            assert float(cell[prefix + "max_abs"]) == float(np.abs(x).max()) and int(cell[prefix + "nonfinite"]) == 0
        off += n


# ------------------------------------------------------------------ 4. non-finite
@pytest.mark.parametrize("mode", list(MODES))
def test_non_finite_elements_are_counted_and_left_out_of_the_sums(mode):
    dtype, with_master = MODES[mode]
    top, div = _units(dtype)
    div_w, top_w = (64, 1024) if with_master else (div, top)
    sizes = (1025, 2 * 8192 + 5, 64, 7)   # the second owns three workgroups; the last gets no finite element at all
    rng = np.random.default_rng(5)
    n, ends = sum(sizes), np.concatenate(([0], np.cumsum(sizes)))
    kw, kg = rng.integers(-top_w, top_w + 1, size=n), rng.integers(-top, top + 1, size=n)
    b0, b1 = int(ends[1]), int(ends[2])
    nan, inf = float("nan"), float("inf")
    # first and last element, and either side of the boundary between workgroups 0 and 1 (and of the first whole pass)
    bad_w = {b0: nan, b0 + 1023: -inf, b0 + 1024: inf, b1 - 1: inf}
    bad_g = {b0: -inf, b0 + 1024: nan, b0 + 3 * 1024 - 1: nan, b0 + 3 * 1024: inf, b1 - 2: -inf, b1 - 1: nan}
    for i in range(int(ends[3]), int(ends[4])):
        bad_w[i], bad_g[i] = (nan, inf, -inf)[i % 3], (inf, nan)[i % 2]

    def buffers(with_bad):
        w, g = kw / div_w, kg / div
        if with_bad:
            for i, v in bad_w.items():
                w[i] = v
            for i, v in bad_g.items():
                g[i] = v
        if with_master:   # the parameters themselves are finite and different: they are not read
            return dict(weights=kg / div, grads=g, master=w)
        return dict(weights=w, grads=g)

    (clean,) = launch(sizes=sizes, dtype=dtype, **buffers(False))
    (dirty,) = launch(sizes=sizes, dtype=dtype, **buffers(True))
    fw, fg = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    fw[list(bad_w)], fg[list(bad_g)] = False, False
    for s in range(4):
        sl = slice(int(ends[s]), int(ends[s + 1]))
        want = _exact_cell(kw[sl].astype(np.int64), kg[sl].astype(np.int64), div_w, div, fw[sl], fg[sl])
        assert dirty["rows"][0]["cells"][s].tobytes() == want.tobytes(), (mode, s, dirty["rows"][0]["cells"][s], want)
    for s in (0, 2):   # the neighbours do not notice
        assert dirty["rows"][0]["cells"][s].tobytes() == clean["rows"][0]["cells"][s].tobytes()
    assert (int(dirty["rows"][0]["cells"][1]["w_nonfinite"]), int(dirty["rows"][0]["cells"][1]["g_nonfinite"])) == (4, 6)
    empty = dirty["rows"][0]["cells"][3]
    assert [float(empty[k]) for k in ("w_sum", "w_sum_sq", "w_max_abs", "g_sum", "g_sum_sq", "g_max_abs")] == [0.0] * 6
    assert not any(np.signbit(float(empty[k])) for k in ("w_sum", "w_max_abs", "g_sum", "g_max_abs"))
    assert (int(empty["w_nonfinite"]), int(empty["g_nonfinite"])) == (7, 7)
    # -0.0 counts as 0
    (zero,) = launch(np.array([-0.0, -0.0, -0.0]), np.array([-0.0, 0.0, -0.0]), (3,), dtype,
                     master=np.array([-0.0] * 3) if with_master else None)
    assert zero["rows"][0]["cells"][0].tobytes() == np.zeros((), dtype=CELL).tobytes()


# ------------------------------------------------------------------ 5. period and ring
def test_period_three_and_a_ring_of_four_rows_over_fourteen_launches():
    sizes = (5, 8193, 64)
    rng = np.random.default_rng(6)
    kw, kg = rng.integers(-1024, 1025, size=sum(sizes)), rng.integers(-1024, 1025, size=sum(sizes))

    def double(i, params, master):   # exactly: the sums double, the sums of squares quadruple
        params.mul_(2.0)

    seen = launch(kw / 64, kg / 64, sizes, F32, period=3, capacity=4, launches=14, between=double)
    ends = np.concatenate(([0], np.cumsum(sizes)))
    base = [_exact_cell(kw[ends[s]: ends[s + 1]].astype(np.int64), kg[ends[s]: ends[s + 1]].astype(np.int64), 64, 64)
            for s in range(3)]
    rows = {}   # slot -> (call, seq), as the launches so far should have left the ring
    for i, raw in enumerate(seen):
        if i % 3 == 0:
            rows[(i // 3) % 4] = (i, i // 3)
        assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (i + 1, i // 3 + 1, 0), i
        assert not raw["reserved"].any()
        for slot in range(4):
            row = raw["rows"][slot]
            if slot not in rows:
                assert not row.tobytes().strip(b"\0"), (i, slot)
                continue
            call, seq = rows[slot]
            assert (int(row["call"]), int(row["seq"]), int(row["reserved"])) == (call, seq, 0), (i, slot)
            for s in range(3):
                cell = row["cells"][s]
                assert float(cell["w_sum"]) == float(base[s]["w_sum"]) * 2.0 ** call
                assert float(cell["w_sum_sq"]) == float(base[s]["w_sum_sq"]) * 4.0 ** call
                assert float(cell["w_max_abs"]) == float(base[s]["w_max_abs"]) * 2.0 ** call
                assert bytes(cell.tobytes()[32:]) == base[s].tobytes()[32:]   # the gradients never changed
        if i % 3 != 0:   # a skipped launch leaves every row's bytes as they were
            assert raw["rows"].tobytes() == seen[i - 1]["rows"].tobytes(), i
    assert [int(r["seq"]) for r in seen[-1]["rows"]] == [4, 1, 2, 3]


# ------------------------------------------------------------------ 6. buffer contract
@pytest.mark.parametrize("mode", ["f32", "bf16_master"])
def test_only_block_and_workspace_are_written_and_the_workspace_need_not_be_initialised(mode):
    """`launch` guards every buffer, gives the workspace exactly the queried size and compares params, master, grads and a
    decoy; here, besides: the block does not depend on what the workspace held, and a launch that is not recorded leaves
    the workspace as it found it."""
    dtype, with_master = MODES[mode]
    sizes = (5, 3 * 8192 + 1, 64, 1025)
    rng = np.random.default_rng(7)
    n = sum(sizes)
    w = torch.from_numpy(rng.normal(size=n)).to(dtype).double().numpy()
    g = torch.from_numpy(rng.normal(size=n)).to(dtype).double().numpy()
    m = rng.normal(size=n).astype(np.float32).astype(np.float64) if with_master else None
    poisoned = launch(w, g, sizes, dtype, master=m, period=2, capacity=3, launches=3, workspace_fill=0xFF)
    zeroed = launch(w, g, sizes, dtype, master=m, period=2, capacity=3, launches=3, workspace_fill=0x00)
    for a, b in zip(poisoned, zeroed):
        assert a.tobytes() == b.tobytes()
    assert [(int(r["calls"]), int(r["recorded"]), int(r["ticket"])) for r in poisoned] == [(1, 1, 0), (2, 1, 0), (3, 2, 0)]
    first, skipped, third = poisoned
    assert skipped["rows"].tobytes() == first["rows"].tobytes()
    assert third["rows"][1]["cells"].tobytes() == first["rows"][0]["cells"].tobytes()
    assert not third["rows"][2].tobytes().strip(b"\0")
    (raw,) = launch(w, g, sizes, dtype, master=m, period=2, capacity=1, workspace_fill=0x7B, calls=1)
    assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (2, 0, 0) and not raw["rows"].tobytes().strip(b"\0")
    assert bool((launch.last_workspace == 0x7B).all())


# ------------------------------------------------------------------ 7. capture
def test_a_captured_launch_replayed_six_times_equals_six_eager_launches():
    sizes = (5, 8193, 130)
    ends = np.cumsum(sizes).tolist()
    n = ends[-1]
    g0 = torch.Generator().manual_seed(8)
    versions = [torch.randn(n, generator=g0).to(DEV) for _ in range(6)]
    grads = torch.randn(n, generator=g0).to(DEV)
    blocks = []
    for captured in (False, True):
        ps = ParamStats(DEV, ["a", "b", "c"], period=1, capacity=8)
        ps.bind(sizes)
        params = torch.empty(n, device=DEV)
        params.copy_(versions[0])
        if captured:
            side = torch.cuda.Stream(DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                ps.record(params, None, grads)
            torch.cuda.current_stream(DEV).wait_stream(side)
            torch.cuda.synchronize(DEV)
            ps.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ps.record(params, None, grads)
            assert int(ps.raw()["calls"]) == 0   # a capture runs nothing
        for v in versions:
            params.copy_(v)
            if captured:
                graph.replay()
            else:
                ps.record(params, None, grads)
        blocks.append(ps.raw())
        rows = ps.read()
        assert [(r["call"], r["seq"]) for r in rows] == [(i, i) for i in range(6)] and ps.lost == 0
        assert len({r["stats"]["b"]["weights"]["sum"] for r in rows}) == 6
    assert blocks[0].tobytes() == blocks[1].tobytes()


# ------------------------------------------------------------------ 8. through the optimizers
def _optimizer(kind, params, **kw):
    from dctn_amd import training as T

    if kind == "adam":
        return T.FlatAdam(params[:2], params[2:], lr=1e-2, weight_decay=1e-3, l2=1e-2, **kw)
    if kind == "sgd":
        return T.FlatSGD(params[:2], params[2:], lr=1e-2, momentum=0.9, l2=1e-2, **kw)
    return T.FlatRMSprop(params[:2], params[2:], lr=1e-2, alpha=0.9, momentum=0.9, weight_decay=1e-3, l2=1e-2, **kw)


def _fsum_bounds(x):
    """(fsum x, n u sum |x|, fsum x^2, n u sum x^2) of a float64 array."""
    p, e = _exact_squares(x)
    sq = math.fsum(np.concatenate((p, e)))
    return math.fsum(x), x.size * U * math.fsum(np.abs(x)), sq, x.size * U * sq


@pytest.mark.parametrize("mode", ["f32", "bf16_master"])
@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_every_step_records_the_weights_it_wrote_and_the_gradients_it_read(kind, mode):
    dtype, master = MODES[mode]
    sizes = (5, 64, 130)
    top, div = _units(dtype)
    rng = np.random.default_rng(9)
    w0 = [rng.integers(-top, top + 1, size=c) / div for c in sizes]
    grads = [[rng.integers(-top, top + 1, size=c) for c in sizes] for _ in range(2)]

    def run(with_monitor):
        params = [torch.nn.Parameter(torch.from_numpy(w).to(dtype).to(DEV)) for w in w0]
        ps = ParamStats(DEV, ["a", "b.c", "d"], capacity=4) if with_monitor else None
        opt = _optimizer(kind, params, master_weights=master, param_stats=ps)
        assert (opt.master is not None) == master
        kept = []
        for step_grads in grads:
            for p, k in zip(params, step_grads):
                p.grad = torch.from_numpy(k / div).to(dtype).to(DEV)
            opt.step()
            torch.cuda.synchronize(DEV)
            kept.append((opt.master if master else opt.flat).detach().double().cpu().numpy())
        state = {"flat": opt.flat, "master": opt.master, "state": opt._state, "sq_sum": opt.sq_sum}
        state.update({name: getattr(opt, name) for name in opt._MOMENTS})
        return ps, kept, {k: None if v is None else v.clone() for k, v in state.items()}

    ps, kept, state = run(True)
    _, _, plain = run(False)
    assert list(state) == list(plain)
    for key in state:   # no other buffer changes a bit
        assert (state[key] is None) == (plain[key] is None), key
        if state[key] is not None:
            assert torch.equal(state[key].view(torch.uint8), plain[key].view(torch.uint8)), (kind, mode, key)
    rows = ps.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(0, 0), (1, 1)] and list(rows[0]["stats"]) == ["a", "b.c", "d"]
    ends = np.concatenate(([0], np.cumsum(sizes)))
    for row, flat, step_grads in zip(rows, kept, grads):
        for s, name in enumerate(ps.names):
            st = row["stats"][name]
            x = flat[ends[s]: ends[s + 1]]
            total, bound, sq, bound_sq = _fsum_bounds(x)   # the step's arithmetic leaves inexact values: case 3's bounds
            assert abs(st["weights"]["sum"] - total) <= bound and abs(st["weights"]["sum_sq"] - sq) <= bound_sq, (kind, mode, name)
            assert st["weights"]["max_abs"] == float(np.abs(x).max()) and st["weights"]["nonfinite"] == 0.0
            k = step_grads[s].astype(np.int64)   # the gradients are case 1's kind of values: ==
            assert st["grads"]["sum"] == float(int(k.sum())) / div and st["grads"]["sum_sq"] == float(int((k * k).sum())) / div ** 2
            assert st["grads"]["max_abs"] == float(int(np.abs(k).max())) / div and st["grads"]["n"] == float(sizes[s])
    assert rows[0]["stats"]["d"]["weights"]["sum"] != rows[1]["stats"]["d"]["weights"]["sum"]


# ------------------------------------------------------------------ 9. K iterations per launch; 11. snapshots
def _recipe_objects(period=1, model_seed=None, capacity=16):
    """The smallest case of tests/recipe_reference.py (two cores, 10 x 10 images, 37 samples in batches of 8) in float32
    with a batch source, its FlatAdam holding a monitor."""
    from dctn_amd.batches import DeviceBatches
    from dctn_amd.training import FlatAdam
    from tests import recipe_reference as RR

    case = RR.CASES["two_layer"]
    model = RR.initial_model(case, F32, DEV, model_seed)
    model.use_fused_dropout(case.dropout_seed)
    params = list(model.epses) + [model.linear.weight, model.linear.bias]
    ps = ParamStats.for_parameters(model, params, period=period, capacity=capacity)
    opt = FlatAdam(params[:-1], params[-1:], lr=case.lr, weight_decay=case.weight_decay, param_stats=ps)
    images, labels = RR.make_data(case)
    src = DeviceBatches(images, labels, RR.GLOBAL_BATCH, dtype=F32, seed=case.batch_seed, scale=case.scale)
    return case, model, opt, src, ps


def _recipe_step(case, model, opt, src, K):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, reg_fn=lambda m: m.epses_composition_l2_regularizer(),
                            reg_coeff=case.reg_coeff, warmup=1, batch_source=src, iters_per_launch=K)


def _cells(rows_raw, seqs):
    return [rows_raw["rows"][s]["cells"].tobytes() for s in seqs]


@functools.lru_cache(maxsize=None)
def _six_launches_of_one():
    case, model, opt, src, ps = _recipe_objects()
    step = _recipe_step(case, model, opt, src, 1)
    assert int(ps.raw()["calls"]) == 1   # the warm-up step counts
    ps.reset()
    for _ in range(6):
        step()
    torch.cuda.synchronize(DEV)
    return ps.raw(), ps.read(), {k: getattr(opt, k).clone() for k in ("flat", "m", "v", "_state")}


def test_two_launches_of_three_iterations_leave_the_six_rows_of_six_launches_of_one():
    raw_a, rows_a, state_a = _six_launches_of_one()
    assert [(r["call"], r["seq"]) for r in rows_a] == [(i, i) for i in range(6)]
    assert list(rows_a[0]["stats"]) == ["epses.0", "epses.1", "linear.weight", "linear.bias"]
    assert len({r["stats"]["epses.0"]["weights"]["sum"] for r in rows_a}) == 6   # the parameters moved
    case, model, opt, src, ps = _recipe_objects()
    step = _recipe_step(case, model, opt, src, 3)
    ps.reset()
    assert step()["iters"] == 3
    step()
    torch.cuda.synchronize(DEV)
    assert ps.raw().tobytes() == raw_a.tobytes() and ps.read() == rows_a
    for key, want in state_a.items():
        assert torch.equal(getattr(opt, key).view(torch.uint8), want.view(torch.uint8)), key
    # period 2: the rows kept are the calls 0, 2, 4 after reset()
    case, model, opt, src, ps = _recipe_objects(period=2)
    step = _recipe_step(case, model, opt, src, 3)
    ps.reset()
    step(), step()
    raw = ps.raw()
    assert (int(raw["calls"]), int(raw["recorded"])) == (6, 3)
    assert [(r["call"], r["seq"]) for r in ps.read()] == [(0, 0), (2, 1), (4, 2)]
    assert _cells(raw, (0, 1, 2)) == _cells(raw_a, (0, 2, 4))


def test_a_resumed_run_continues_calls_recorded_and_the_ring(tmp_path):
    from dctn_amd import checkpoint as C

    case, model, opt, src, ps = _recipe_objects(capacity=4)   # the ring wraps: 1 warm-up + 6 rows in 4 slots
    step = _recipe_step(case, model, opt, src, 1)
    run = C.RunState(model, opt, batch_source=src)
    assert "optimizer.param_stats" in run.names and run.names.index("optimizer.param_stats") == run.names.index("optimizer.sq_sum") + 1
    for _ in range(3):
        step()
    path = run.snapshot({"num_iters_done": 4}).save(str(tmp_path / "monitor.dctn"))
    for _ in range(3):
        step()
    want_raw, want_rows, want_lost = ps.raw(), ps.read(), ps.lost
    assert (int(want_raw["calls"]), int(want_raw["recorded"])) == (7, 7) and want_lost == 3
    case2, model2, opt2, src2, ps2 = _recipe_objects(capacity=4, model_seed=5)
    step2 = _recipe_step(case2, model2, opt2, src2, 1)
    step2(), ps2.read()
    run2 = C.RunState(model2, opt2, batch_source=src2)
    assert run2.load(path) == {"num_iters_done": 4}
    assert int(ps2.raw()["calls"]) == 4 and ps2._seen == 0
    for _ in range(3):
        step2()
    assert ps2.raw().tobytes() == want_raw.tobytes()
    assert ps2.read() == want_rows and ps2.lost == want_lost
    assert [(r["call"], r["seq"]) for r in want_rows] == [(3, 3), (4, 4), (5, 5), (6, 6)]
    # a run without a monitor keeps the region list it had, and refuses the file
    from dctn_amd.training import FlatAdam
    from tests import recipe_reference as RR

    plain_model = RR.initial_model(case, F32, DEV)
    plain_params = list(plain_model.epses) + [plain_model.linear.weight, plain_model.linear.bias]
    plain = C.RunState(plain_model, FlatAdam(plain_params[:-1], plain_params[-1:], lr=case.lr))
    assert [n for n in plain.names if "param_stats" in n] == [] and plain.names[plain.names.index("optimizer.sq_sum") - 1] == "optimizer.state"
    with pytest.raises(ValueError):
        plain.load(path)


# ------------------------------------------------------------------ 10. the classifier
def test_the_classifiers_norms_agree_with_float64_torch_norm_after_one_eager_step():
    """|norm - ref| <= (n + 2) 2^-53 ref: the device's sum of squares and torch's float64 one each lie within n 2^-53 of the
    exact one in relative terms (any order), the square root halves a relative error, and each side rounds it once."""
    from dctn_amd import batches
    from dctn_amd.conv_sbs import DumbNormalInitialization
    from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi
    from dctn_amd.training import FlatRMSprop, fused_cross_entropy, train_step

    g = torch.Generator().manual_seed(16)
    images, labels = torch.randint(0, 256, (8, 8, 8), generator=g, dtype=torch.uint8), torch.randint(0, 10, (8,), generator=g)
    torch.manual_seed(17)
    model = DCTNMnistModel(3, 2, False, DumbNormalInitialization(0.5), True, 1.0).to(DEV)
    src = batches.DeviceBatches(images, labels, 4, dtype=F32, seed=18, phi=quantum_phi(True), device=DEV)
    with torch.no_grad():   # the reference's calibration: without it three layers underflow and every gradient is 0
        model.scale_layers_using_batch((images.float() / 255.0).unsqueeze(1).to(DEV))
    params = list(model.parameters())
    ps = ParamStats.for_parameters(model, params)
    assert list(ps.names) == [name for name, _ in model.named_parameters()] and len(ps.names) == 45
    opt = FlatRMSprop(params, lr=1e-3, alpha=0.9, momentum=0.9, weight_decay=1e-4, param_stats=ps)
    x, y, idx = src.empty_batch()
    src.draw_into(x, y, idx)
    train_step(model, x, y, fused_cross_entropy, opt)
    assert opt._grads() is opt.flat_grad   # the gradients come from several buffers and were gathered
    assert len({p.grad.untyped_storage().data_ptr() for p in params}) >= 5
    (row,) = ps.read()
    assert (row["call"], row["seq"]) == (0, 0)
    for name, p in model.named_parameters():
        for key, t in (("weights", p.detach()), ("grads", p.grad)):
            ref = float(torch.norm(t.double()))
            st = row["stats"][name][key]
            assert (ref > 0.0 or key == "grads") and st["nonfinite"] == 0.0 and st["n"] == float(p.numel())   # (a gradient may be all zeros)
            assert abs(st["norm"] - ref) <= (p.numel() + 2) * U * ref, (name, key, st["norm"], ref)
            assert st["max_abs"] == float(t.abs().max())
    assert any(row["stats"][name]["grads"]["norm"] > 0.0 for name in ps.names)
    first = cell_moments(params[0].numel(), ps.raw()["rows"][0]["cells"][0])
    assert first == row["stats"][ps.names[0]]
