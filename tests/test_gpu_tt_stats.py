"""`dctn_tt_stats` (csrc/tt_stats.hip) and `tt_stats.TTStats` on the GPU (`-m gpu`).

The kernel works in float64 throughout, so on small-integer cores every partial sum is an integer below 2^53 and the
comparison is `==` against an integer evaluation; the rounding tests use positive cores, where the standard bound for a
chain of inner products is a statement about the result's own magnitude."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd.conv_sbs import ConvSBS, DumbNormalInitialization
from dctn_amd.conv_sbs_spec import SBSSpecCore, SBSSpecString
from dctn_amd.pos2d import Pos2D
from dctn_amd.tt_stats import TTStats, block_dtype, moments, reference_moments
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
SNAKE_OUTS = lambda o: tuple(o if i == 4 else 1 for i in range(9))   # noqa: E731


class Str:
    """One string as the raw entry point takes it: numpy cores (o, l, r, q, ..., q), cyclic bonds."""

    def __init__(self, cores, C, q):
        self.cores, self.C, self.q = [np.ascontiguousarray(c) for c in cores], C, q
        self.bonds = [c.shape[1] for c in self.cores]
        self.outs = [c.shape[0] for c in self.cores]
        n = len(self.cores)
        assert all(c.shape[2] == self.bonds[(i + 1) % n] and c.shape[3:] == (q,) * C for i, c in enumerate(self.cores))

    def descriptor(self):
        d = L.TTString()
        d.n_cores, d.C, d.q = len(self.cores), self.C, self.q
        for c in range(len(self.cores)):
            d.out_sizes[c], d.bond_sizes[c] = self.outs[c], self.bonds[c]
        return d

    def bound_n(self):
        """The issue's n = 2 sum_c (l_c r_c + o_c q^C): the dependent length of the doubled chain, taken for both sides."""
        N, P = len(self.cores), self.q ** self.C
        return 2 * sum(self.bonds[c] * self.bonds[(c + 1) % N] + self.outs[c] * P for c in range(N))

    def kernel_n(self):
        """The kernel's own longest dependent sum: per core one chain over (slice, k) of length o_c P l_c whose terms hold
        an inner product of length l_c (tt_step), then l_0 terms per workgroup and l_0 slots (a ring)."""
        P = self.q ** self.C
        return sum(l * (o * P + 1) for l, o in zip(self.bonds, self.outs)) + 2 * self.bonds[0]


def shapes(bonds, outs, C, q):
    n = len(bonds)
    return [(outs[c], bonds[c], bonds[(c + 1) % n]) + (q,) * C for c in range(n)]


def launch(strings, dtype, period=1, capacity=1, launches=1, workspace_fill=0xFF, check_contract=True):
    """`launches` launches over guarded buffers; the block after each one as a structured element.  The cores and a decoy
    must come out as they went in, and the workspace is exactly as large as the library asks."""
    descs = (L.TTString * len(strings))(*[s.descriptor() for s in strings])
    lib = L.lib()
    block_bytes = lib.dctn_tt_stats_block_bytes(len(strings), capacity)
    ws_bytes = lib.dctn_tt_stats_workspace_bytes(descs, len(strings))
    assert block_bytes == block_dtype(len(strings), capacity).itemsize and ws_bytes == 16 * sum(s.bonds[0] for s in strings)
    seen = []
    with guarded(fill=workspace_fill) as arena:
        cores = [arena.place(torch.from_numpy(c).to(dtype).to(DEV)) for s in strings for c in s.cores]
        before = [c.clone() for c in cores]
        decoy = arena.empty((4096,), torch.uint8, DEV)
        block = arena.zeros((block_bytes,), torch.uint8, DEV)
        ws = arena.empty((ws_bytes,), torch.uint8, DEV)
        for _ in range(launches):
            L.check(lib.dctn_tt_stats(L.ptr_array(cores), descs, len(strings), block.data_ptr(), capacity, period, ws.data_ptr(),
                                      ws_bytes, L.dtype_code(cores[0]), L.stream_ptr(DEV)), "TT statistics")
            seen.append(block.cpu().numpy().view(block_dtype(len(strings), capacity))[0].copy())
    arena.check()
    if check_contract:
        for c, b in zip(cores, before):
            assert torch.equal(c.view(torch.uint8), b.view(torch.uint8))
        assert bool((decoy == workspace_fill).all())
    return seen


# ------------------------------------------------------------------ exact
def _integer_string(bonds, outs, C, q, seed):
    """Every slice A[o, p] a signed, scaled permutation-like matrix - max(l, r) non-zeros of +-1 / +-2 along a random
    permutation of the rows and one of the columns, drawn anew per (o, p), so that all (k, b) are touched over the slices."""
    rng = np.random.default_rng(seed)
    cores = []
    for o_n, l, r, *qs in shapes(bonds, outs, C, q):
        P = q ** C
        a = np.zeros((o_n, l, r, P), dtype=np.int64)
        for o in range(o_n):
            for p in range(P):
                rows, cols = rng.permutation(l), rng.permutation(r)
                m = np.arange(max(l, r))
                a[o, rows[m % l], cols[m % r], p] = rng.choice([-2, -1, 1, 2], size=m.size)
        cores.append(a.reshape((o_n, l, r) + tuple(qs)))
    return Str(cores, C, q)


def _magnitude_bound(s):
    """Python integers that bound EVERY partial sum the kernel forms for `sq_norm` and for `sum`, from the cores' absolute
    values: the max row sum is submultiplicative and bounds every entry of every prefix of the chain; the transfer matrix
    E_c = sum_{o,p} |A| (x) |A| has max row sum max_{a,a'} sum_{o,p} rowsum(a) rowsum(a'), S_c = sum_{o,p} |A| has
    max_a sum_{o,p} rowsum(a); l_0^2 (l_0) such terms are added at the end."""
    sq, total = 1, 1
    for c in s.cores:
        a = np.abs(c.astype(np.int64)).reshape(c.shape[0], c.shape[1], c.shape[2], -1)
        rs = a.sum(axis=2).transpose(1, 0, 2).reshape(a.shape[1], -1)   # (l, o p) row sums
        sq *= int((rs @ rs.T).max())
        total *= int(rs.sum(axis=1).max())
    return s.bonds[0] ** 2 * sq, s.bonds[0] * total


def _integer_moments(s):
    """(sum, sq_norm) in int64 arithmetic (exact: `_magnitude_bound` is asserted below 2^53).  A string of few elements
    is evaluated from the definition - its elements are the traces tr(A_0[x_0] ... A_{N-1}[x_{N-1}]) -, any other through
    the chain of S_c and of transfer matrices, left to right."""
    mats = [c.astype(np.int64).reshape(c.shape[0], c.shape[1], c.shape[2], -1) for c in s.cores]
    if math.prod(m.shape[0] * m.shape[3] for m in mats) <= 4096:
        prods = [np.eye(mats[0].shape[1], dtype=np.int64)]
        for m in mats:
            slices = m.transpose(0, 3, 1, 2).reshape(-1, m.shape[1], m.shape[2])
            prods = [x @ a for x in prods for a in slices]
        traces = [int(np.trace(x)) for x in prods]
        return sum(traces), sum(t * t for t in traces)
    row = chain = None
    for m in mats:
        o, l, r, p = m.shape
        flat = m.transpose(1, 2, 0, 3).reshape(l * r, o * p)
        e = (flat @ flat.T).reshape(l, r, l, r).transpose(0, 2, 1, 3).reshape(l * l, r * r)
        sm = m.sum(axis=(0, 3))
        row, chain = (sm, e) if row is None else (row @ sm, chain @ e)
    return int(np.trace(row)), int(np.trace(chain))


@functools.lru_cache(maxsize=None)
def _exact_strings():
    return (
        _integer_string((1,) + (2,) * 8, SNAKE_OUTS(2), 1, 2, seed=1),    # the row snake of the first layer
        _integer_string((1,) + (4,) * 8, SNAKE_OUTS(10), 2, 2, seed=2),   # the ten-label string
        _integer_string((5, 5, 5), (1, 1, 1), 1, 3, seed=3),              # a ring
        _integer_string((1, 32, 32), (1, 1, 1), 2, 2, seed=4),            # an open chain at the largest bond
        _integer_string((1, 7), (1, 3), 1, 2, seed=5),                    # two cores
        _integer_string((1, 3, 6, 2), (1, 2, 1, 3), 2, 2, seed=6),        # non-uniform bonds
        _integer_string((32, 32, 32), (1, 1, 1), 1, 2, seed=7),           # a ring at the largest bond: 32 workgroups
    )


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_integer_cores_give_the_integer_values_alone_together_and_reversed(dtype):
    strings = _exact_strings()
    want = []
    for s in strings:
        assert all(b < 2 ** 53 for b in _magnitude_bound(s)), _magnitude_bound(s)
        total, sq = _integer_moments(s)
        assert sq > 0 and abs(total) < 2 ** 53 and sq < 2 ** 53
        want.append(np.array([float(total), float(sq)]))
    (together,) = launch(strings, dtype)
    (backwards,) = launch(strings[::-1], dtype)
    assert (int(together["calls"]), int(together["recorded"]), int(together["ticket"])) == (1, 1, 0)
    assert (int(together["rows"][0]["call"]), int(together["rows"][0]["seq"])) == (0, 0)
    for k, s in enumerate(strings):
        (alone,) = launch([s], dtype)
        got = [together["rows"][0]["stats"][k], backwards["rows"][0]["stats"][len(strings) - 1 - k], alone["rows"][0]["stats"][0]]
        for g in got:
            assert g.tolist() == want[k].tolist(), (k, g.tolist(), want[k].tolist())
            assert g.tobytes() == got[0].tobytes()


# ------------------------------------------------------------------ golden
@pytest.mark.parametrize("name", ["sbs_2x2_ring_perm0", "sbs_2x2_ring_perm1"])
def test_the_references_ring_fixtures_in_float64(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    s = Str([g[f"core{i}"] for i in range(4)], int(g["C"]), int(g["q"]))
    assert s.bonds == [int(b) for b in g["bond_sizes"]] and s.outs == [int(o) for o in g["out_sizes"]]
    (got,) = launch([s], torch.float64)
    total, sq = (float(v) for v in got["rows"][0]["stats"][0])
    assert abs(total - float(g["tt_sum"])) <= 1e-10 * abs(float(g["tt_sum"]))
    assert abs(sq - float(g["tt_sqnorm"])) <= 1e-10 * abs(float(g["tt_sqnorm"]))
    n = math.prod(o * s.q ** s.C for o in s.outs)
    assert abs(moments(n, total, sq)["var"] - float(g["tt_var"])) <= 1e-9 * abs(float(g["tt_var"]))


# ------------------------------------------------------------------ rounding
_SNAKE_COLUMNS = ((0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1), (0, 2), (1, 2), (2, 2))


def _spec(bonds, outs, C, q, positions=None):
    positions = positions or [(0, i) for i in range(len(bonds))]
    return SBSSpecString(tuple(SBSSpecCore(Pos2D(h, w), o) for (h, w), o in zip(positions, outs)), tuple(bonds), C, q)


@pytest.mark.parametrize("case", ["bond-16 column snake", "bond-32 ring"])
def test_positive_float32_cores_against_the_float64_torch_path(case):
    """|dev - ref| <= 4 n 2^-53 |ref| with n = 2 sum_c (l_c r_c + o_c q^C): the gamma_n bound of a chain of inner products,
    taken for both sides and doubled; derived, not measured.  Nothing cancels in positive cores, so |ref| is the scale.
    The kernel's own longest dependent sum (`Str.kernel_n`: sum_c l_c (o_c q^C + 1) + 2 l_0) is shorter than n / 2 here."""
    spec = {"bond-16 column snake": _spec((1,) + (16,) * 8, SNAKE_OUTS(2), 2, 2, _SNAKE_COLUMNS),
            "bond-32 ring": _spec((32, 32, 32), (1, 1, 1), 1, 2)}[case]
    rng = np.random.default_rng(8)
    cores = [rng.uniform(0.5, 1.5, size=sh.as_tuple()).astype(np.float32) for sh in spec.shapes]
    s = Str(cores, spec.in_num_channels, spec.in_quantum_dim_size)
    assert s.kernel_n() <= s.bound_n() // 2
    m = ConvSBS(spec, DumbNormalInitialization(0.1)).double()
    with torch.no_grad():
        for p, c in zip(m.cores, cores):
            p.copy_(torch.from_numpy(c).double())
        ref = (float(m.sum()), float(m.squared_fro_norm()))
    (got,) = launch([s], torch.float32)
    for dev, want, what in zip(got["rows"][0]["stats"][0], ref, ("sum", "sq_norm")):
        err = abs(float(dev) - want)
        print(f"{case} {what}: dev {float(dev)!r} ref {want!r} rel {err / abs(want):.3e} bound {4 * s.bound_n() * U:.3e}")
        assert err <= 4 * s.bound_n() * U * abs(want), (what, float(dev), want)


# ------------------------------------------------------------------ period, ring of rows, capture
def _module(spec, dtype, seed):
    torch.manual_seed(seed)
    return ConvSBS(spec, DumbNormalInitialization(0.7)).to(dtype).to(DEV)


def _assert_within_the_bound(got, cores, spec):
    """(sum, sq_norm) against the mirror at the model test's bound: 4 n 2^-53 times the statistic of the absolute cores."""
    s = Str([np.asarray(c, dtype=np.float64) for c in cores], spec.in_num_channels, spec.in_quantum_dim_size)
    ref, scale = reference_moments(s.cores), reference_moments([np.abs(c) for c in s.cores])
    for value, key in zip(got, ("sum", "sq_norm")):
        assert abs(float(value) - ref[key]) <= 4 * s.bound_n() * U * scale[key], (key, float(value), ref[key])


def test_a_period_of_twenty_keeps_the_last_two_rows_and_counts_the_lost_one():
    m = _module(_spec((1, 3, 3), (1, 2, 1), 2, 2), torch.float32, 12)
    tt = TTStats(DEV, [m], ["s"], period=20, capacity=2)
    base = None
    for k in range(45):
        tt.record()
        if k == 0:
            raw = tt.raw()
            assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (1, 1, 0)
            base = raw["rows"][0]["stats"][0].copy()   # the row of call 0
        m.cores[1].data.mul_(2.0)   # exactly: the sum doubles, the squared norm quadruples
    _assert_within_the_bound(base, [c.detach().double().cpu().numpy() * (0.5 ** 45 if i == 1 else 1.0) for i, c in enumerate(m.cores)],
                             m.spec)
    raw = tt.raw()
    assert (int(raw["calls"]), int(raw["recorded"]), int(raw["ticket"])) == (45, 3, 0)
    rows = tt.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(20, 1), (40, 2)] and tt.lost == 1
    for r in rows:
        st = r["stats"]["s"]
        assert st["sum"] == base[0] * 2.0 ** r["call"] and st["sq_norm"] == base[1] * 4.0 ** r["call"]
        assert st == dict(moments(m.spec.nelement, st["sum"], st["sq_norm"]), sum=st["sum"], sq_norm=st["sq_norm"])
    assert tt.read() == [] and tt.lost == 1
    tt.reset(calls=19)
    tt.record(), tt.record()   # calls 19 and 20
    rows = tt.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(20, 0)] and tt.lost == 0 and int(tt.raw()["calls"]) == 21
    assert rows[0]["stats"]["s"]["sum"] == base[0] * 2.0 ** 45


def test_five_records_in_one_captured_graph_go_on_where_the_last_replay_stopped():
    ring, chain = _module(_spec((3, 2, 4), (2, 1, 1), 1, 2), torch.float64, 13), _module(_spec((1, 4), (1, 3), 1, 3), torch.float64, 14)
    tt = TTStats(DEV, [ring, chain], period=2, capacity=8)
    assert tt.names == ("0", "1")
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        tt.record()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    tt.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(5):
            tt.record()
    assert int(tt.raw()["calls"]) == 0   # a capture runs nothing
    def check(rows, calls):
        assert [r["call"] for r in rows] == calls
        for r in rows:
            for name, m in zip(tt.names, (ring, chain)):
                st = r["stats"][name]
                _assert_within_the_bound((st["sum"], st["sq_norm"]), [c.detach().cpu().numpy() for c in m.cores], m.spec)
            assert r["stats"] == rows[0]["stats"]   # the same cores: the same bits

    graph.replay()
    check(tt.read(), [0, 2, 4])
    graph.replay()
    rows = tt.read()
    check(rows, [6, 8])
    assert [r["seq"] for r in rows] == [3, 4] and int(tt.raw()["calls"]) == 10 and tt.lost == 0
    tt.reset()
    graph.replay()
    check(tt.read(), [0, 2, 4])


# ------------------------------------------------------------------ buffer contract
def test_nothing_outside_block_and_workspace_is_written_and_the_workspace_need_not_be_initialised():
    """`launch` guards every buffer and compares the cores and a decoy; here, besides: the rows do not depend on what the
    workspace held (NaN bytes against zero bytes), and a launch that is not recorded changes the header alone."""
    strings = [_integer_string((4, 3, 5), (2, 1, 1), 1, 2, seed=20), _integer_string((1, 6, 2), (1, 3, 1), 2, 2, seed=21)]
    for dtype in (torch.float32, torch.float64):
        poisoned = launch(strings, dtype, period=2, capacity=3, launches=3, workspace_fill=0xFF)
        zeroed = launch(strings, dtype, period=2, capacity=3, launches=3, workspace_fill=0x00)
        for a, b in zip(poisoned, zeroed):
            assert a.tobytes() == b.tobytes()
        first, skipped, third = poisoned
        assert [(int(r["calls"]), int(r["recorded"]), int(r["ticket"])) for r in poisoned] == [(1, 1, 0), (2, 1, 0), (3, 2, 0)]
        assert skipped["rows"].tobytes() == first["rows"].tobytes() and not skipped["reserved"].any()
        assert third["rows"][0].tobytes() == first["rows"][0].tobytes()
        assert (int(third["rows"][1]["call"]), int(third["rows"][1]["seq"])) == (2, 1)
        assert third["rows"][1]["stats"].tobytes() == first["rows"][0]["stats"].tobytes()
        assert not third["rows"][2].tobytes().strip(b"\0")   # the third row was never written
        for k, s in enumerate(strings):
            assert first["rows"][0]["stats"][k].tolist() == [float(v) for v in _integer_moments(s)]
    # an unrecorded launch leaves the workspace as it found it
    descs = (L.TTString * 2)(*[s.descriptor() for s in strings])
    ws_bytes = L.lib().dctn_tt_stats_workspace_bytes(descs, 2)
    with guarded(fill=0x7B) as arena:
        cores = [arena.place(torch.from_numpy(c).float().to(DEV)) for s in strings for c in s.cores]
        block = arena.zeros((L.lib().dctn_tt_stats_block_bytes(2, 1),), torch.uint8, DEV)
        block[:4] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device=DEV)   # calls = 1: odd, not recorded at period 2
        ws = arena.empty((ws_bytes,), torch.uint8, DEV)
        L.check(L.lib().dctn_tt_stats(L.ptr_array(cores), descs, 2, block.data_ptr(), 1, 2, ws.data_ptr(), ws_bytes, L.F32,
                                      L.stream_ptr(DEV)), "TT statistics")
    arena.check()
    assert bool((ws == 0x7B).all())
    got = block.cpu().numpy().view(block_dtype(2, 1))[0]
    assert (int(got["calls"]), int(got["recorded"]), int(got["ticket"])) == (2, 0, 0) and not got["rows"].tobytes().strip(b"\0")


# ------------------------------------------------------------------ the model
def test_the_model_records_its_five_strings_in_front_of_every_graphed_iteration():
    """Row k against `reference_moments` of the parameters as replay k found them: |dev - ref| <= 4 n 2^-53 M with the
    n of the rounding test and M the same statistic of the ABSOLUTE cores (these cores have signs: the magnitude scale is
    the bound's honest one).  The kernel's own dependent sum is longer than n / 2 for the ten-label string (its chain runs
    over l_c o_c q^C terms per core): `Str.kernel_n` <= 2 n there, and with the mirror's n / 2 it stays inside the
    bound's fourfold margin."""
    from dctn_amd import batches
    from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi
    from dctn_amd.training import FlatRMSprop, GraphedTrainStep, fused_cross_entropy

    g = torch.Generator().manual_seed(16)
    images, labels = torch.randint(0, 256, (8, 8, 8), generator=g, dtype=torch.uint8), torch.randint(0, 10, (8,), generator=g)

    def run(with_tt):
        torch.manual_seed(17)
        model = DCTNMnistModel(3, 2, False, DumbNormalInitialization(0.5), True, 1.0).to(DEV)
        src = batches.DeviceBatches(images, labels, 4, dtype=torch.float32, seed=18, phi=quantum_phi(True), device=DEV)
        opt = FlatRMSprop(list(model.parameters()), lr=1e-3, alpha=0.9, momentum=0.9, weight_decay=1e-4)
        if with_tt:
            model.tt_stats = TTStats.for_model(model, period=1)
            assert list(model.tt_stats.names) == model.string_names() and len(model.tt_stats.names) == 5
        step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src)
        snapshots, out = [], None
        if with_tt:
            assert int(model.tt_stats.raw()["calls"]) >= 2   # the warm-up forwards count
            model.tt_stats.reset()
        for _ in range(3):
            snapshots.append([[c.detach().clone() for c in s.cores] for s in (model.tt_stats.strings if with_tt else [])])
            out = step()
        torch.cuda.synchronize()
        return model, opt, {k: v.detach().clone() for k, v in out.items() if isinstance(v, torch.Tensor)}, snapshots

    model, opt, out, snapshots = run(True)
    rows = model.tt_stats.read()
    assert [(r["call"], r["seq"]) for r in rows] == [(0, 0), (1, 1), (2, 2)] and model.tt_stats.lost == 0
    for row, snapshot in zip(rows, snapshots):
        for name, string, cores in zip(model.tt_stats.names, model.tt_stats.strings, snapshot):
            s = Str([c.cpu().numpy() for c in cores], string.spec.in_num_channels, string.spec.in_quantum_dim_size)
            assert s.kernel_n() <= 2 * s.bound_n()
            ref, scale = reference_moments(s.cores), reference_moments([np.abs(c) for c in s.cores])
            for key in ("sum", "sq_norm"):
                err = abs(row["stats"][name][key] - ref[key])
                assert err <= 4 * s.bound_n() * U * scale[key], (name, key, row["stats"][name][key], ref[key])
            st = row["stats"][name]
            assert st["mean"] == st["sum"] / string.spec.nelement
    assert rows[0]["stats"] != rows[1]["stats"] != rows[2]["stats"]   # the parameters moved in between

    plain_model, plain_opt, plain_out, _ = run(False)
    assert set(out) == set(plain_out) and "output" in out
    for key in out:
        assert torch.equal(out[key], plain_out[key]), key
    for key in ("flat", "square_avg", "buf"):
        assert torch.equal(getattr(opt, key), getattr(plain_opt, key)), key
    for p, q in zip(model.parameters(), plain_model.parameters()):
        assert torch.equal(p, q)
    # an eval forward and the calibration record nothing
    calls = int(model.tt_stats.raw()["calls"])
    model.eval()
    with torch.no_grad():
        model(torch.rand(2, 1, 8, 8).to(DEV))
        model.scale_layers_using_batch(torch.rand(2, 1, 8, 8).to(DEV))
    assert int(model.tt_stats.raw()["calls"]) == calls
