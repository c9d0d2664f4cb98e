"""What the TT-tensor statistics promise without a GPU: the numpy mirror `reference_moments` against the reference's
fixtures and against the torch contractions of `ConvSBS`, the reference's moment formula in Python floats, the exports of
library version 520 with the block's layout and every pinned return code (all decided on the host before any launch),
the logger's tags, and what `TTStats` refuses before it needs a device."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from dctn_amd import _lib, training
from dctn_amd.conv_sbs import ConvSBS
from dctn_amd.conv_sbs_spec import SBSSpecCore, SBSSpecString
from dctn_amd.pos2d import Pos2D
from dctn_amd.tt_stats import HEADER_BYTES, ROW_HEAD_BYTES, TTStats, block_dtype, moments, reference_moments

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PTR = 4096   # any non-null, 16-byte aligned number: the calls below return before they would use it


def _rel(got, want):
    return abs(got - want) / abs(want)


def _chain(bonds, outs, C, q):
    """A string whose cores sit in one row; only bonds, out sizes, C and q matter to the parameter-only contractions."""
    return SBSSpecString(tuple(SBSSpecCore(Pos2D(0, i), o) for i, o in enumerate(outs)), tuple(bonds), C, q)


# ------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("name", ["sbs_2x2_ring_perm0", "sbs_2x2_ring_perm1"])
def test_the_mirror_gives_the_references_sum_norm_and_variance_of_a_ring(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    bonds = [int(b) for b in g["bond_sizes"]]
    assert sorted(bonds) == [3, 4, 5, 6] and int(g["C"]) == 2 and int(g["q"]) == 2
    cores = [g[f"core{i}"] for i in range(len(bonds))]
    got = reference_moments(cores, bonds)
    assert _rel(got["sum"], float(g["tt_sum"])) <= 1e-10
    assert _rel(got["sq_norm"], float(g["tt_sqnorm"])) <= 1e-10
    n = math.prod(c.size // (c.shape[1] * c.shape[2]) for c in cores)
    assert n == (1 * 4) * (3 * 4) * (2 * 4) * (4 * 4)
    assert _rel(moments(n, got["sum"], got["sq_norm"])["var"], float(g["tt_var"])) <= 1e-9
    with pytest.raises(ValueError):
        reference_moments(cores, bonds[1:] + bonds[:1])
    with pytest.raises(ValueError):
        reference_moments(cores[:2])   # the ring does not close


@pytest.mark.parametrize("case", ["open snake", "non-uniform open chain"])
def test_the_mirror_gives_what_the_torch_contractions_give(case):
    spec = {"open snake": _chain((1,) + (3,) * 8, [2 if i == 4 else 1 for i in range(9)], 1, 2),
            "non-uniform open chain": _chain((1, 3, 6, 2), (1, 2, 1, 3), 2, 2)}[case]
    torch.manual_seed(11)
    m = ConvSBS(spec).double()
    with torch.no_grad():
        for c in m.cores:
            c.copy_(torch.randn(c.shape, dtype=torch.float64))
        total, sq, var = float(m.sum()), float(m.squared_fro_norm()), float(m.var())
    got = reference_moments(list(m.cores), spec.bond_sizes)
    assert _rel(got["sum"], total) <= 1e-10 and _rel(got["sq_norm"], sq) <= 1e-10
    st = moments(spec.nelement, got["sum"], got["sq_norm"])
    assert _rel(st["var"], var) <= 1e-9 and st["mean"] == got["sum"] / spec.nelement and st["std"] == st["var"] ** 0.5


# ------------------------------------------------------------------ the formula
def test_moments_is_the_references_formula_in_its_operation_order():
    # the elements 0, 1, 2, 3: sum 6, squares 14, unbiased variance 5 / 3
    st = moments(4, 6.0, 14.0)
    assert st["mean"] == 1.5 and st["var"] == 14.0 / 3 - 2 * 6.0 / 3 * 1.5 + 4 / 3 * 1.5**2 and st["std"] == st["var"] ** 0.5
    assert abs(st["var"] - 5.0 / 3) < 1e-15
    assert moments(4, 6.0, 14.0, unbiased=False)["var"] == 14.0 / 4 - 2 * 6.0 / 4 * 1.5 + 4 / 4 * 1.5**2 == 1.25
    # numbers that round at every step: each operation spelled out, and torch's float64 evaluation of the same line
    n, total, sq = 7, 0.1, 0.7
    mean = total / n
    d = n - 1
    want = ((sq / d) - (((2 * total) / d) * mean)) + ((n / d) * (mean**2))
    assert moments(n, total, sq)["var"] == want
    t_total, t_sq = torch.tensor(total, dtype=torch.float64), torch.tensor(sq, dtype=torch.float64)
    t_mean = t_total / n
    assert moments(n, total, sq)["var"] == float(t_sq / d - 2 * t_total / d * t_mean + n / d * t_mean**2)
    assert moments(n, total, sq)["mean"] == float(t_mean)


def test_a_negative_variance_gives_a_nan_std():
    st = moments(10, 10.0, 9.0)   # sq < total^2 / n: no real tensor, but cancellation gets there
    assert st["var"] < 0 and math.isnan(st["std"]) and st["mean"] == 1.0
    assert moments(10, 0.0, 0.0)["std"] == 0.0
    assert math.isnan(moments(1, 2.0, 4.0)["var"]) and math.isnan(moments(1, 2.0, 4.0)["std"])


# ------------------------------------------------------------------ the library's interface
def test_exports_version_and_block_layout():
    lib = _lib.lib()
    assert lib.dctn_version() >= 520
    for name in ("dctn_tt_stats", "dctn_tt_stats_block_bytes", "dctn_tt_stats_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    size = lib.dctn_tt_stats_block_bytes
    for n, cap in ((1, 1), (5, 64), (16, 2), (7, 1000)):
        dt = block_dtype(n, cap)
        assert size(n, cap) == dt.itemsize == HEADER_BYTES + cap * (ROW_HEAD_BYTES + 16 * n)
        assert dt.fields["rows"][1] == HEADER_BYTES and dt["rows"].shape == (cap,)
        row = dt["rows"].base
        assert [row.fields[k][1] for k in ("call", "seq", "reserved", "stats")] == [0, 4, 8, 16] and row["stats"].shape == (n, 2)
    assert [block_dtype(1, 1).fields[k][1] for k in ("calls", "recorded", "ticket", "reserved")] == [0, 4, 8, 12]
    assert size(0, 4) == size(17, 4) == size(3, 0) == size(-1, -1) == 0
    assert ctypes.sizeof(_lib.TTString) == 4 * (4 + 16 + 16)


def _string(bonds, outs=None, C=1, q=2):
    d = _lib.TTString()
    d.n_cores, d.C, d.q = len(bonds), C, q
    for c, b in enumerate(bonds):
        d.bond_sizes[c], d.out_sizes[c] = b, 1 if outs is None else outs[c]
    return d


def test_tt_stats_return_codes_and_workspace_size():
    lib = _lib.lib()
    good = [_string((1, 4, 4), (1, 10, 1), C=2), _string((5, 5, 5), q=3)]

    def descs(*strings):
        return (_lib.TTString * len(strings))(*strings)

    def call(cores=6, strings=None, n=2, block=PTR, capacity=4, period=1, ws=PTR, ws_bytes=1 << 20, dtype=_lib.F32, hole=None):
        ptrs = None
        if cores is not None:
            ptrs = (ctypes.c_void_p * 64)(*[PTR] * 64)
            if hole is not None:
                ptrs[hole] = None
            if isinstance(cores, dict):
                for k, v in cores.items():
                    ptrs[k] = v
        strings = descs(*good) if strings is None else strings
        return lib.dctn_tt_stats(ptrs, strings, n, block, capacity, period, ws, ws_bytes, dtype, None)

    # (the good call itself would launch: it is never made)
    # NULL first
    assert call(cores=None) == call(block=None) == _lib.ERR_NULL
    assert lib.dctn_tt_stats((ctypes.c_void_p * 6)(*[PTR] * 6), None, 2, PTR, 4, 1, PTR, 1 << 20, _lib.F32, None) == _lib.ERR_NULL
    assert call(hole=5) == call(hole=0) == _lib.ERR_NULL and call(hole=5, dtype=_lib.BF16) == _lib.ERR_NULL
    assert call(hole=6, ws_bytes=0) == _lib.ERR_WORKSPACE   # only the six entries the strings own are looked at
    # shapes
    assert call(n=0) == call(n=17) == call(n=-1) == _lib.ERR_BAD_SHAPE
    assert call(capacity=0) == call(period=0) == call(period=-20) == _lib.ERR_BAD_SHAPE
    too_many = _string((1,) * 16)
    too_many.n_cores = 17
    none = _string((1,))
    none.n_cores = 0
    for bad in (too_many, none, _string((1, 2), C=0), _string((1, 2), q=0), _string((1, 2), (1, 0)), _string((1, 0)),
                _string((0, 2)), _string((1, -3))):
        assert call(strings=descs(good[0], bad)) == _lib.ERR_BAD_SHAPE
        assert call(strings=descs(good[0], bad), dtype=_lib.BF16) == _lib.ERR_BAD_SHAPE   # shape before dtype
    # a bad n_cores is seen before a NULL entry behind it (the walk over the entries needs it), a bad out size after
    assert call(strings=descs(good[0], too_many), hole=1) == _lib.ERR_BAD_SHAPE
    assert call(strings=descs(good[0], _string((1, 2), (1, 0))), hole=1) == _lib.ERR_NULL
    # dtype
    assert call(dtype=_lib.BF16) == call(dtype=7) == call(dtype=-1) == _lib.ERR_BAD_DTYPE
    # unsupported comes after the dtype: the limits, then alignment
    for big in (_string((1, 33)), _string((33, 33, 33)), _string((1, 2), C=9), _string((1, 2), C=2, q=17),
                _string((1, 32, 32), (1, 1 << 22, 1), C=1)):
        assert call(strings=descs(good[0], big)) == _lib.ERR_UNSUPPORTED
        assert call(strings=descs(good[0], big), dtype=_lib.BF16) == _lib.ERR_BAD_DTYPE
        assert lib.dctn_tt_stats_workspace_bytes(descs(good[0], big), 2) == 0
    assert call(cores={2: PTR + 2}) == call(block=PTR + 4) == call(ws=PTR + 4) == _lib.ERR_UNSUPPORTED
    assert call(cores={2: PTR + 4}, dtype=_lib.F64) == _lib.ERR_UNSUPPORTED
    assert call(cores={2: PTR + 4}, ws_bytes=0) == _lib.ERR_WORKSPACE   # float32 cores are 4-byte aligned
    assert call(strings=descs(_string((1, 32, 32)), _string((32, 32, 32), C=8)), ws_bytes=0) == _lib.ERR_WORKSPACE   # at the limits
    # the workspace: 16 bytes per workgroup, one workgroup per value of the first bond
    need = lib.dctn_tt_stats_workspace_bytes
    assert need(descs(*good), 2) == 16 * (1 + 5) and need(descs(good[0]), 1) == 16 and need(descs(_string((32, 32, 32))), 1) == 512
    assert need(None, 2) == need(descs(*good), 0) == need(descs(*good), 17) == need(descs(none), 1) == 0
    assert call(ws_bytes=95) == call(ws=None) == call(ws_bytes=0) == _lib.ERR_WORKSPACE
    assert call(ws_bytes=95, block=PTR + 4) == _lib.ERR_UNSUPPORTED   # the workspace's size comes last


# ------------------------------------------------------------------ the logger
class _FakeTT:
    """What the logger needs of a `TTStats`: read()."""

    def __init__(self, batches):
        self.batches, self.reads = list(batches), 0

    def read(self):
        self.reads += 1
        return self.batches.pop(0) if self.batches else []


def _entry(call, seq, **means):
    return {"call": call, "seq": seq, "stats": {name: {"sum": 0.0, "sq_norm": 0.0, "mean": m, "var": m * m, "std": abs(m)}
                                                 for name, m in means.items()}}


def test_the_logger_reports_the_references_two_tags_per_string_and_row():
    tt = _FakeTT([[_entry(0, 0, a=1.5, b=-2.0), _entry(20, 1, a=2.5, b=-3.0)], [_entry(40, 2, a=0.25, b=4.0)], []])
    seen = []
    hook = training.make_tt_stats_logger(tt, 3, lambda tag, value, it: seen.append((tag, value, it)), first_iter=100)
    for launch in range(7):
        hook({}, {"num_iters_done": 100 + 8 * launch + 7})
    assert tt.reads == 2   # launches 3 and 6
    assert seen == [("mean_of_tt_tensor/a", 1.5, 100), ("std_of_tt_tensor/a", 1.5, 100),
                    ("mean_of_tt_tensor/b", -2.0, 100), ("std_of_tt_tensor/b", 2.0, 100),
                    ("mean_of_tt_tensor/a", 2.5, 120), ("std_of_tt_tensor/a", 2.5, 120),
                    ("mean_of_tt_tensor/b", -3.0, 120), ("std_of_tt_tensor/b", 3.0, 120),
                    ("mean_of_tt_tensor/a", 0.25, 140), ("std_of_tt_tensor/a", 0.25, 140),
                    ("mean_of_tt_tensor/b", 4.0, 140), ("std_of_tt_tensor/b", 4.0, 140)]
    hook.flush()
    assert tt.reads == 3 and len(seen) == 12   # nothing new: nothing reported
    plain = training.make_tt_stats_logger(_FakeTT([[_entry(5, 0, s=1.0)]]), 1, lambda *a: seen.append(a))
    plain({}, {})
    assert seen[-2:] == [("mean_of_tt_tensor/s", 1.0, 5), ("std_of_tt_tensor/s", 1.0, 5)]


# ------------------------------------------------------------------ the host object
def test_tt_stats_checks_its_arguments_before_it_needs_a_device():
    cpu = torch.device("cpu")
    a, b = ConvSBS(_chain((1, 2), (1, 2), 1, 2)), ConvSBS(_chain((3, 2, 2), (1, 1, 1), 2, 2))
    for bad in (dict(strings=[]), dict(strings=[a, b], names=["x", "x"]), dict(strings=[a, b], names=["x"]),
                dict(strings=[a], period=0), dict(strings=[a], capacity=0), dict(strings=[a] * 17)):
        with pytest.raises(ValueError):
            TTStats(cpu, **bad)
    with pytest.raises(TypeError):
        TTStats(cpu, [a, ConvSBS(_chain((1, 2), (1, 2), 1, 2)).double()])
    with pytest.raises(TypeError):
        TTStats(cpu, [ConvSBS(_chain((1, 2), (1, 2), 1, 2)).bfloat16()])
    for spec in (_chain((1, 33), (1, 1), 1, 2), _chain((1, 2), (1, 1), 9, 2), _chain((1,) * 17, (1,) * 17, 1, 2)):
        with pytest.raises(NotImplementedError):
            TTStats(cpu, [ConvSBS(spec)])
    with pytest.raises(ValueError):
        TTStats.for_model(torch.nn.Linear(2, 2))


@pytest.mark.skipif(torch.cuda.is_available(), reason="what the calls do where there is no GPU")
def test_without_a_gpu_the_constructor_raises():
    with pytest.raises(RuntimeError):
        TTStats(torch.device("cpu"), [ConvSBS(_chain((1, 2), (1, 2), 1, 2))])
