"""The parameter-group table on the host: the exported interface, the block's layout, the validation in Python and in
`dctn_param_groups_check`, the numpy mirror `segment_of`, and `RunState`'s region list with and without a table.  No GPU:
the blocks live in CPU tensors and no step is launched."""
import inspect
import json
import os
import re
import subprocess
from ctypes import c_double, c_float, c_int, c_int64 as c_i64, c_size_t as c_size, c_void_p as c_void

import numpy as np
import pytest
import torch

from dctn_amd import _lib
from dctn_amd.training import FlatAdam, FlatSGD, ParamGroup, ParamGroups, param_groups_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0   # DCTN_OK
SIZES = [4099, 1, 3000, 5, 4096, 1094]


def _params(sizes=SIZES):
    return [torch.nn.Parameter(torch.full((k,), 0.5)) for k in sizes]


def _adam(regularised, others=(), **kw):
    """A FlatAdam on the CPU: with a schedule, whose rate needs no device write at construction."""
    from dctn_amd.training import LRSchedule

    kw.setdefault("schedule", LRSchedule.constant("cpu", 1e-3))
    return FlatAdam(regularised, others, **kw)


# ------------------------------------------------------------------ interface
EXPECTED = {
    "dctn_param_groups_bytes": (c_size, []),
    "dctn_param_groups_check": (c_int, [c_void, c_i64]),
    "dctn_adam_l2_step_grouped": (c_int, [c_void] * 10 + [c_i64, c_i64, c_double, c_double, c_float, c_float, c_int, c_void]),
    "dctn_sgd_l2_step_grouped": (c_int, [c_void] * 9 + [c_i64, c_i64, c_float, c_float, c_int, c_void]),
}


def test_entry_points_are_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    declared = set(re.findall(r"\b(dctn_[a-z0-9_]+)\s*\(", header))
    exported = set()
    for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "T":
            exported.add(parts[2])
    for name, (res, args) in EXPECTED.items():
        assert name in declared, f"{name} is not declared in include/dctn_amd.h"
        assert name in exported, f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and list(got_args) == args, name
        fn = getattr(_lib.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert declared == set(_lib.SIGNATURES)
    assert _lib.lib().dctn_version() >= 511
    assert _lib.lib().dctn_param_groups_bytes() == 1552 == 4 * ParamGroups.WORDS
    # the grouped steps are the scheduled ones with the table behind the schedule; Adam's loses weight_decay
    adam = list(_lib.SIGNATURES["dctn_adam_l2_step_scheduled"][1])
    assert EXPECTED["dctn_adam_l2_step_grouped"][1] == adam[:9] + [c_void] + adam[9:14] + adam[15:]
    sgd = list(_lib.SIGNATURES["dctn_sgd_l2_step_scheduled"][1])
    assert EXPECTED["dctn_sgd_l2_step_grouped"][1] == sgd[:8] + [c_void] + sgd[8:]


def test_the_steps_refuse_missing_pointers_and_bad_shapes_on_the_host():
    adam, sgd = _lib.lib().dctn_adam_l2_step_grouped, _lib.lib().dctn_sgd_l2_step_grouped
    tail = (0.9, 0.999, 1e-8, 0.0)
    #          master params grads m  v  sq    state guard sched groups
    assert adam(None, 8, 8, 8, 8, None, 8, None, None, None, 4, 2, *tail, _lib.F32, None) == _lib.ERR_NULL   # no table
    assert adam(None, 8, 8, 8, 8, None, None, None, None, 8, 4, 2, *tail, _lib.F32, None) == _lib.ERR_NULL   # no state
    assert adam(None, 8, 8, 8, 8, None, 8, None, None, 8, 4, 5, *tail, _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert adam(8, 8, 8, 8, 8, None, 8, None, None, 8, 4, 2, *tail, _lib.F32, None) == _lib.ERR_BAD_DTYPE
    assert adam(None, 8, 8, 8, 8, None, 8, None, None, 8, 4, 2, *tail, _lib.F64, None) == _lib.ERR_BAD_DTYPE
    #         master params grads buf sq   state guard sched groups
    assert sgd(None, 8, 8, 8, None, 8, None, None, None, 4, 2, 0.9, 0.0, _lib.F32, None) == _lib.ERR_NULL
    assert sgd(None, 8, 8, 8, None, None, None, None, 8, 4, 2, 0.9, 0.0, _lib.F32, None) == _lib.ERR_NULL
    assert sgd(None, 8, 8, 8, None, 8, None, None, 8, 0, 0, 0.9, 0.0, _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert sgd(8, 8, 8, 8, None, 8, None, None, 8, 4, 2, 0.9, 0.0, _lib.F32, None) == _lib.ERR_BAD_DTYPE


# ------------------------------------------------------------------ the block and the host check
def _check(words, n):
    words = np.ascontiguousarray(words, dtype=np.int32)
    return _lib.lib().dctn_param_groups_check(words.ctypes.data_as(c_void), n)


def test_the_block_layout_and_the_librarys_check():
    params = _params()
    g = ParamGroups(params, [ParamGroup([params[1], params[3]], lr_scale=0.5, weight_decay=1e-2),
                             ParamGroup(params[4], frozen=True)])
    words = g.host_block([3, 0, 1, 0, 7, 2])
    n = sum(SIZES)
    assert words.dtype == np.int32 and words.size == 388
    assert words[0] == 6 and not words[1:4].any()
    assert words[4:132].view(np.int64)[:6].tolist() == np.cumsum(SIZES).tolist() == g.ends
    assert not words[4:132].view(np.int64)[6:].any()
    assert words.view(np.float32)[132:138].tolist() == [1.0, 0.5, 1.0, 0.5, 1.0, 1.0]
    wd = float(np.float32(1e-2))
    assert words.view(np.float32)[196:202].tolist() == [0.0, wd, 0.0, wd, 0.0, 0.0]
    assert words[260:266].tolist() == [0, 0, 0, 0, 1, 0] and words[324:330].tolist() == [3, 0, 1, 0, 7, 2]
    assert np.array_equal(g._block.numpy(), g.host_block())                  # the "device" block (a CPU tensor here)
    assert _check(words, n) == OK
    assert _lib.lib().dctn_param_groups_check(None, n) == _lib.ERR_NULL
    assert _check(words, n + 1) == _lib.ERR_BAD_SHAPE                        # the last end is not n
    assert _check(words, 0) == _lib.ERR_BAD_SHAPE

    def broken(edit):
        w = words.copy()
        edit(w)
        return _check(w, n)

    ends = lambda w: w[4:132].view(np.int64)   # noqa: E731
    assert broken(lambda w: w.__setitem__(0, 0)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: w.__setitem__(0, 65)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: ends(w).__setitem__(1, 4099)) == _lib.ERR_BAD_SHAPE      # an empty segment
    assert broken(lambda w: ends(w).__setitem__(2, 4000)) == _lib.ERR_BAD_SHAPE      # decreasing
    assert broken(lambda w: ends(w).__setitem__(0, 0)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: ends(w).__setitem__(0, -5)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: ends(w).__setitem__(5, n + 4)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: w.view(np.float32).__setitem__(133, np.nan)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: w.view(np.float32).__setitem__(133, -1.0)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: w.view(np.float32).__setitem__(197, np.inf)) == _lib.ERR_BAD_SHAPE
    assert broken(lambda w: w.__setitem__(261, 2)) == _lib.ERR_BAD_SHAPE             # an unknown flag
    assert broken(lambda w: w.__setitem__(325, -1)) == _lib.ERR_BAD_SHAPE            # a negative count
    # slots past n_segments may hold anything
    assert broken(lambda w: (ends(w).__setitem__(slice(6, 64), -1), w.__setitem__(slice(138, 196), -1),
                             w.__setitem__(slice(266, 324), -1))) == OK
    # a full table of 64 one-element segments
    full = ParamGroups(_params([1] * 64))
    assert _check(full.host_block(), 64) == OK


def test_validation_errors_of_the_table():
    params = _params()
    with pytest.raises(NotImplementedError, match="64"):
        ParamGroups(_params([2] * 65))
    assert len(ParamGroups(_params([2] * 64))) == 64
    with pytest.raises(ValueError, match="not one of the optimizer's"):
        ParamGroups(params, [ParamGroup([torch.nn.Parameter(torch.ones(3))], lr_scale=0.5)])
    with pytest.raises(ValueError, match="two entries"):
        ParamGroups(params, [ParamGroup([params[0]]), ParamGroup([params[0]], lr_scale=2.0)])
    with pytest.raises(ValueError, match="twice"):
        ParamGroups([params[0], params[0]])
    with pytest.raises(ValueError):
        ParamGroups([])
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="lr_scale"):
            ParamGroups(params, [ParamGroup([params[0]], lr_scale=bad)])
        with pytest.raises(ValueError, match="weight_decay"):
            ParamGroups(params, [ParamGroup([params[0]], weight_decay=bad)])
    with pytest.raises(TypeError):
        ParamGroups(params, [dict(params=[params[0]])])
    # an equal tensor is not the same parameter: entries match by identity
    twin = torch.nn.Parameter(params[1].detach().clone())
    with pytest.raises(ValueError, match="not one of the optimizer's"):
        ParamGroups(params, [ParamGroup([twin])])


def test_the_optimizers_take_a_table_over_their_own_parameters_only():
    for cls in (FlatAdam, FlatSGD):
        p = inspect.signature(cls.__init__).parameters["groups"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(ParamGroup.__init__).parameters) == ["self", "params", "lr_scale", "weight_decay", "frozen"]
    assert list(inspect.signature(ParamGroups.__init__).parameters) == ["self", "params", "entries"]
    assert list(inspect.signature(param_groups_for).parameters) == ["model", "freeze_eps", "head_lr_scale"]
    params = _params()
    g = ParamGroups(params, [ParamGroup([params[2]], lr_scale=0.1, weight_decay=1e-2)])
    adam = _adam(params[:3], params[3:], weight_decay=1e-3, groups=g)
    assert adam.groups is g
    wd = float(np.float32(1e-3))
    assert g.weight_decays == [wd, wd, float(np.float32(1e-2)), wd, wd, wd]       # None became the optimizer's value
    assert g._block.view(torch.float32)[196:202].tolist() == g.weight_decays
    with pytest.raises(ValueError, match="flat order"):
        _adam(params[:3], params[3:], groups=ParamGroups(params[::-1]))
    with pytest.raises(ValueError, match="flat order"):
        _adam(params[:3], params[3:], groups=ParamGroups(params[:5]))
    with pytest.raises(TypeError):
        _adam(params[:3], params[3:], groups=object())
    # FlatSGD has no weight decay
    sgd_params = _params()
    with pytest.raises(ValueError, match="weight_decay=None"):
        FlatSGD(sgd_params, groups=ParamGroups(sgd_params, [ParamGroup([sgd_params[0]], weight_decay=1e-3)]))
    sgd_params = _params()
    gs = ParamGroups(sgd_params, [ParamGroup([sgd_params[0]], lr_scale=2.0)])
    sgd = FlatSGD(sgd_params, lr=0.25, groups=gs)
    with pytest.raises(ValueError, match="no weight decay"):
        gs.set(sgd_params[1], weight_decay=1e-3)
    # a grouped FlatSGD owns the step block; assigning the rate writes its cell
    assert sgd._state is not None and sgd._state.view(torch.float32)[1].item() == 0.25 and sgd.t == 0
    sgd.lr = 0.5
    assert sgd.lr == 0.5 and sgd._state.view(torch.float32)[1].item() == 0.5 and sgd._state[0].item() == 0
    # without a table nothing changed
    plain = FlatSGD(_params(), lr=0.25)
    assert plain.groups is None and plain._state is None
    assert _adam(_params()).groups is None


def test_set_freeze_steps_and_the_state_dict():
    params = _params()
    params[2].requires_grad_(False)
    g = ParamGroups.from_requires_grad(params, [ParamGroup([params[5]], lr_scale=0.25)])
    assert g.frozen == [False, False, True, False, False, False] and g.lr_scales[5] == 0.25
    assert g._block[260:266].tolist() == [0, 0, 1, 0, 0, 0]
    g.freeze(params[0])
    g.freeze(2, False)
    g.set(params[3], lr_scale=2.0, weight_decay=1e-3)
    assert g.frozen == [True, False, False, False, False, False]
    assert np.array_equal(g._block.numpy(), g.host_block())                       # the cell writes equal a full upload
    g._block[324:330] = torch.tensor([7, 12, 7, 12, 12, 12], dtype=torch.int32)   # what a kernel would leave
    assert g.steps == [7, 12, 7, 12, 12, 12]
    g.set(params[1], lr_scale=0.5)                                                # an edit keeps the counts
    assert g.steps == [7, 12, 7, 12, 12, 12]
    state = g.state_dict()
    assert json.loads(json.dumps(state)) == state
    other = ParamGroups(_params())
    other.load_state_dict(state)
    assert other.state_dict() == state and np.array_equal(other._block.numpy(), g._block.numpy())
    with pytest.raises(ValueError, match="end at"):
        ParamGroups(_params([5, 5])).load_state_dict(state)
    mirror = ParamGroups(_params())
    mirror.run_restored(None, {"groups": g._block.numpy()})
    assert mirror.lr_scales == g.lr_scales and mirror.frozen == g.frozen and mirror.weight_decays == g.weight_decays
    with pytest.raises(ValueError, match="not one of"):
        g.freeze(torch.nn.Parameter(torch.ones(1)))
    with pytest.raises(ValueError):
        g.set(6, lr_scale=1.0)


def test_edits_are_refused_during_a_capture(monkeypatch):
    params = _params()
    g = ParamGroups(params)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    g.device = torch.device("cuda:0")             # (only the check looks at it here)
    for edit in (lambda: g.set(0, lr_scale=0.5), lambda: g.freeze(params[0]), lambda: g.load_state_dict({})):
        with pytest.raises(RuntimeError, match="capture"):
            edit()
    assert g.lr_scales[0] == 1.0 and g.frozen[0] is False


@pytest.mark.parametrize("sizes", [SIZES, [1] * 64, [3, 1, 1, 70000, 2]])
def test_segment_of_against_a_brute_force_scan(sizes):
    g = ParamGroups(_params(sizes))
    owner = np.repeat(np.arange(len(sizes)), sizes)
    n = int(owner.size)
    probes = set(range(min(n, 300))) | set(range(max(n - 300, 0), n))
    for e in g.ends:
        probes |= {e - 2, e - 1, e, e + 1}
    rng = np.random.default_rng(5)
    probes |= set(int(i) for i in rng.integers(0, n, 500))
    for i in sorted(p for p in probes if 0 <= p < n):
        assert g.segment_of(i) == owner[i], i
    for i in (-1, n):
        with pytest.raises(IndexError):
            g.segment_of(i)


# ------------------------------------------------------------------ the runner's helper and RunState's regions
class _Head(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.epses = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(4, 3)) for _ in range(3)])
        self.linear = torch.nn.Linear(6, 2)


def test_param_groups_for_follows_the_runners_flags():
    model = _Head()
    model.epses[2].requires_grad_(False)
    g = param_groups_for(model, freeze_eps=(0,), head_lr_scale=0.1)
    assert [p is q for p, q in zip(g.params, list(model.epses) + [model.linear.weight, model.linear.bias])] == [True] * 5
    assert g.frozen == [True, False, True, False, False]
    s = float(np.float32(0.1))
    assert g.lr_scales == [1.0, 1.0, 1.0, s, s]
    opt = _adam(list(model.epses) + [model.linear.weight], [model.linear.bias], weight_decay=1e-3, groups=g)
    assert opt.groups is g and g.ends[-1] == opt.n
    with pytest.raises(ValueError, match="freeze_eps"):
        param_groups_for(model, freeze_eps=(3,))
    assert param_groups_for(_Head()).frozen == [False] * 5


def test_run_state_lists_the_table_behind_the_schedule_and_nothing_new_without_one():
    from dctn_amd import checkpoint as C
    from dctn_amd.training import LRSchedule

    def names(**kw):
        model = _Head()
        params = list(model.epses) + [model.linear.weight, model.linear.bias]
        if kw.pop("grouped"):
            kw["groups"] = ParamGroups(params)
        cls = kw.pop("cls")
        opt = cls(params[:4], params[4:], **kw)
        regions, _ = C.run_regions(model, opt, None, None)
        if "groups" in kw:
            assert next(t for name, t in regions if name == "optimizer.groups") is kw["groups"]._block
        return [name for name, _ in regions]

    # (a FlatAdam on the CPU needs a schedule: without one its constructor writes the rate on the device)
    schedule = LRSchedule.constant("cpu", 1e-3)
    assert names(cls=FlatAdam, grouped=False, schedule=schedule) == [
        "optimizer.flat", "optimizer.m", "optimizer.v", "optimizer.schedule", "optimizer.state", "optimizer.sq_sum"]
    assert names(cls=FlatAdam, grouped=True, schedule=schedule) == [
        "optimizer.flat", "optimizer.m", "optimizer.v", "optimizer.schedule", "optimizer.groups", "optimizer.state",
        "optimizer.sq_sum"]
    assert names(cls=FlatSGD, grouped=False) == ["optimizer.flat", "optimizer.buf", "optimizer.sq_sum"]
    assert names(cls=FlatSGD, grouped=True) == ["optimizer.flat", "optimizer.buf", "optimizer.groups", "optimizer.state",
                                                "optimizer.sq_sum"]
