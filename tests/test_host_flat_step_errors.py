"""The return code of every flat-optimizer entry point for every kind of bad argument, pinned as a literal table.

The twelve dctn_adam_l2_step* / dctn_sgd_l2_step* entry points are conveniences over dctn_adam_flat_step /
dctn_sgd_flat_step (include/dctn_amd.h, version 512); which error a call with SEVERAL bad arguments answers differs
between them on purpose, and TABLE holds what the library of version 511 - the last one in which each entry point
validated its own arguments - returned.  `python -m tests.test_host_flat_step_errors LIBRARY` prints the table of any
library.  Every call here returns before a launch: no GPU."""
import ctypes
import sys

import pytest

from dctn_amd import _lib

P = 8   # a non-null dummy pointer: no call here gets as far as using one
NULL, SHAPE, DTYPE = _lib.ERR_NULL, _lib.ERR_BAD_SHAPE, _lib.ERR_BAD_DTYPE

_ADAM_TAIL = ("beta1", "beta2", "eps", "weight_decay", "l2")
_SGD_TAIL = ("lr", "momentum", "l2", "first_step")
# entry point -> (its arguments in order, the pointers it requires)
ENTRY = {
    "dctn_adam_l2_step": (("params", "grads", "exp_avg", "exp_avg_sq", "sq_sum", "state", "n", "n_reg") + _ADAM_TAIL
                          + ("dtype", "stream"), ("params", "grads", "exp_avg", "exp_avg_sq", "state")),
    "dctn_adam_l2_step_master": (("master", "params", "grads", "exp_avg", "exp_avg_sq", "sq_sum", "state", "n", "n_reg")
                                 + _ADAM_TAIL + ("stream",),
                                 ("master", "params", "grads", "exp_avg", "exp_avg_sq", "state")),
    "dctn_adam_l2_step_guarded": (("params", "grads", "exp_avg", "exp_avg_sq", "sq_sum", "state", "guard", "n", "n_reg")
                                  + _ADAM_TAIL + ("dtype", "stream"),
                                  ("params", "grads", "exp_avg", "exp_avg_sq", "state", "guard")),
    "dctn_adam_l2_step_master_guarded": (("master", "params", "grads", "exp_avg", "exp_avg_sq", "sq_sum", "state", "guard",
                                          "n", "n_reg") + _ADAM_TAIL + ("stream",),
                                         ("master", "params", "grads", "exp_avg", "exp_avg_sq", "state", "guard")),
    "dctn_adam_l2_step_scheduled": (("master", "params", "grads", "exp_avg", "exp_avg_sq", "sq_sum", "state", "guard",
                                     "schedule", "n", "n_reg") + _ADAM_TAIL + ("dtype", "stream"),
                                    ("params", "grads", "exp_avg", "exp_avg_sq", "state", "schedule")),
    "dctn_adam_l2_step_grouped": (("master", "params", "grads", "exp_avg", "exp_avg_sq", "sq_sum", "state", "guard",
                                   "schedule", "groups", "n", "n_reg", "beta1", "beta2", "eps", "l2", "dtype", "stream"),
                                  ("params", "grads", "exp_avg", "exp_avg_sq", "state", "groups")),
    "dctn_sgd_l2_step": (("params", "grads", "momentum_buf", "sq_sum", "n", "n_reg") + _SGD_TAIL + ("dtype", "stream"),
                         ("params", "grads", "momentum_buf")),
    "dctn_sgd_l2_step_master": (("master", "params", "grads", "momentum_buf", "sq_sum", "n", "n_reg") + _SGD_TAIL
                                + ("stream",), ("master", "params", "grads", "momentum_buf")),
    "dctn_sgd_l2_step_guarded": (("params", "grads", "momentum_buf", "sq_sum", "guard", "n", "n_reg") + _SGD_TAIL
                                 + ("dtype", "stream"), ("params", "grads", "momentum_buf", "guard")),
    "dctn_sgd_l2_step_master_guarded": (("master", "params", "grads", "momentum_buf", "sq_sum", "guard", "n", "n_reg")
                                        + _SGD_TAIL + ("stream",), ("master", "params", "grads", "momentum_buf", "guard")),
    "dctn_sgd_l2_step_scheduled": (("master", "params", "grads", "momentum_buf", "sq_sum", "state", "guard", "schedule",
                                    "n", "n_reg", "momentum", "l2", "dtype", "stream"),
                                   ("params", "grads", "momentum_buf", "state", "schedule")),
    "dctn_sgd_l2_step_grouped": (("master", "params", "grads", "momentum_buf", "sq_sum", "state", "guard", "schedule",
                                  "groups", "n", "n_reg", "momentum", "l2", "dtype", "stream"),
                                 ("params", "grads", "momentum_buf", "state", "groups")),
}
# a valid call but for the overrides of a case: every pointer the entry point requires is there, every optional one is not
VALID = dict(sq_sum=None, stream=None, n=4, n_reg=2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, l2=0.0, lr=0.1,
             momentum=0.9, first_step=1, dtype=_lib.F32)


def cases(name):
    """case -> the arguments it breaks.  One bad argument each, then the pairs that decide which check comes first."""
    args, required = ENTRY[name]
    adam, has_dtype = "beta1" in args, "dtype" in args
    either = has_dtype and "master" in args   # the _scheduled / _grouped forms: a master copy beside a dtype argument
    out = {f"null:{p}": {p: None} for p in required}
    out.update({"n=0": dict(n=0), "n_reg>n": dict(n_reg=5), "n_reg<0": dict(n_reg=-1)})
    if adam:
        out.update({"beta1=1": dict(beta1=1.0), "beta2=1": dict(beta2=1.0)})
    if has_dtype:
        out["f64"] = dict(dtype=_lib.F64)
    if either:
        out["master+f32"] = dict(master=P, dtype=_lib.F32)
        out["null:params & master+f32"] = dict(params=None, master=P, dtype=_lib.F32)
        out[f"null:{required[-1]} & master+f32"] = {required[-1]: None, "master": P, "dtype": _lib.F32}
        out["n=0 & master+f32"] = dict(n=0, master=P, dtype=_lib.F32)
    out["null:params & n=0"] = dict(params=None, n=0)
    out[f"null:{required[-1]} & n_reg>n"] = {required[-1]: None, "n_reg": 5}
    if has_dtype:
        out["n=0 & f64"] = dict(n=0, dtype=_lib.F64)
        out["null:grads & f64"] = dict(grads=None, dtype=_lib.F64)
    if adam and has_dtype:
        out["beta2=1 & f64"] = dict(beta2=1.0, dtype=_lib.F64)
    if adam:
        out["null:state & beta1=1"] = dict(state=None, beta1=1.0)
    return out


def values(name, broken):
    args, required = ENTRY[name]
    v = dict(VALID, master=None, guard=None, schedule=None, groups=None, state=None)
    v.update({p: P for p in required})
    v.update(broken)
    return v


def legacy_call(lib, name, broken):
    v = values(name, broken)
    return getattr(lib, name)(*[v[a] for a in ENTRY[name][0]])


# what version 511 returned
TABLE = {
    "dctn_adam_l2_step": {
        "null:params": -6,
        "null:grads": -6,
        "null:exp_avg": -6,
        "null:exp_avg_sq": -6,
        "null:state": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "beta1=1": -1,
        "beta2=1": -1,
        "f64": -2,
        "null:params & n=0": -6,
        "null:state & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
        "beta2=1 & f64": -1,
        "null:state & beta1=1": -6,
    },
    "dctn_adam_l2_step_master": {
        "null:master": -6,
        "null:params": -6,
        "null:grads": -6,
        "null:exp_avg": -6,
        "null:exp_avg_sq": -6,
        "null:state": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "beta1=1": -1,
        "beta2=1": -1,
        "null:params & n=0": -6,
        "null:state & n_reg>n": -6,
        "null:state & beta1=1": -6,
    },
    "dctn_adam_l2_step_guarded": {
        "null:params": -6,
        "null:grads": -6,
        "null:exp_avg": -6,
        "null:exp_avg_sq": -6,
        "null:state": -6,
        "null:guard": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "beta1=1": -1,
        "beta2=1": -1,
        "f64": -2,
        "null:params & n=0": -6,
        "null:guard & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
        "beta2=1 & f64": -1,
        "null:state & beta1=1": -6,
    },
    "dctn_adam_l2_step_master_guarded": {
        "null:master": -6,
        "null:params": -6,
        "null:grads": -6,
        "null:exp_avg": -6,
        "null:exp_avg_sq": -6,
        "null:state": -6,
        "null:guard": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "beta1=1": -1,
        "beta2=1": -1,
        "null:params & n=0": -6,
        "null:guard & n_reg>n": -6,
        "null:state & beta1=1": -6,
    },
    "dctn_adam_l2_step_scheduled": {
        "null:params": -6,
        "null:grads": -6,
        "null:exp_avg": -6,
        "null:exp_avg_sq": -6,
        "null:state": -6,
        "null:schedule": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "beta1=1": -1,
        "beta2=1": -1,
        "f64": -2,
        "master+f32": -2,
        "null:params & master+f32": -2,
        "null:schedule & master+f32": -6,
        "n=0 & master+f32": -2,
        "null:params & n=0": -6,
        "null:schedule & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
        "beta2=1 & f64": -1,
        "null:state & beta1=1": -6,
    },
    "dctn_adam_l2_step_grouped": {
        "null:params": -6,
        "null:grads": -6,
        "null:exp_avg": -6,
        "null:exp_avg_sq": -6,
        "null:state": -6,
        "null:groups": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "beta1=1": -1,
        "beta2=1": -1,
        "f64": -2,
        "master+f32": -2,
        "null:params & master+f32": -2,
        "null:groups & master+f32": -6,
        "n=0 & master+f32": -2,
        "null:params & n=0": -6,
        "null:groups & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
        "beta2=1 & f64": -1,
        "null:state & beta1=1": -6,
    },
    "dctn_sgd_l2_step": {
        "null:params": -6,
        "null:grads": -6,
        "null:momentum_buf": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "f64": -2,
        "null:params & n=0": -6,
        "null:momentum_buf & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
    },
    "dctn_sgd_l2_step_master": {
        "null:master": -6,
        "null:params": -6,
        "null:grads": -6,
        "null:momentum_buf": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "null:params & n=0": -6,
        "null:momentum_buf & n_reg>n": -6,
    },
    "dctn_sgd_l2_step_guarded": {
        "null:params": -6,
        "null:grads": -6,
        "null:momentum_buf": -6,
        "null:guard": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "f64": -2,
        "null:params & n=0": -6,
        "null:guard & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
    },
    "dctn_sgd_l2_step_master_guarded": {
        "null:master": -6,
        "null:params": -6,
        "null:grads": -6,
        "null:momentum_buf": -6,
        "null:guard": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "null:params & n=0": -6,
        "null:guard & n_reg>n": -6,
    },
    "dctn_sgd_l2_step_scheduled": {
        "null:params": -6,
        "null:grads": -6,
        "null:momentum_buf": -6,
        "null:state": -6,
        "null:schedule": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "f64": -2,
        "master+f32": -2,
        "null:params & master+f32": -6,
        "null:schedule & master+f32": -6,
        "n=0 & master+f32": -1,
        "null:params & n=0": -6,
        "null:schedule & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
    },
    "dctn_sgd_l2_step_grouped": {
        "null:params": -6,
        "null:grads": -6,
        "null:momentum_buf": -6,
        "null:state": -6,
        "null:groups": -6,
        "n=0": -1,
        "n_reg>n": -1,
        "n_reg<0": -1,
        "f64": -2,
        "master+f32": -2,
        "null:params & master+f32": -6,
        "null:groups & master+f32": -6,
        "n=0 & master+f32": -1,
        "null:params & n=0": -6,
        "null:groups & n_reg>n": -6,
        "n=0 & f64": -1,
        "null:grads & f64": -6,
    },
}


def _bound(path):
    lib = ctypes.CDLL(path)
    for name in ENTRY:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_the_older_entry_points_answer_as_they_did(name):
    assert sorted(TABLE[name]) == sorted(cases(name))
    got = {case: legacy_call(_lib.lib(), name, broken) for case, broken in cases(name).items()}
    assert got == TABLE[name]
    assert all(code in (NULL, SHAPE, DTYPE) for code in got.values())   # nothing here reached a launch


def test_the_table_holds_each_precedence_the_entry_points_differ_in():
    for name in ENTRY:
        adam, late = "adam" in name, name.endswith(("_scheduled", "_grouped"))
        if late:   # the master / dtype check: in front of everything in Adam's forms, inside the dtype check in SGD's
            assert TABLE[name]["master+f32"] == DTYPE
            assert TABLE[name]["null:params & master+f32"] == (DTYPE if adam else NULL)
            assert TABLE[name]["n=0 & master+f32"] == (DTYPE if adam else SHAPE)
            assert TABLE[name][f"null:{ENTRY[name][1][-1]} & master+f32"] == NULL   # the block the form exists for is first
        assert TABLE[name]["null:params & n=0"] == NULL
        if "dtype" in ENTRY[name][0]:
            assert TABLE[name]["n=0 & f64"] == SHAPE and TABLE[name]["null:grads & f64"] == NULL
        if adam and "dtype" in ENTRY[name][0]:
            assert TABLE[name]["beta2=1 & f64"] == SHAPE


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_the_descriptor_entry_points_answer_the_same(name):
    """The same broken arguments through dctn_flat_step_t.  A case that only takes away a block the descriptor holds as an
    option (the guard of a _guarded form, ...) describes a valid step there and is left out; the descriptor entry points
    have the precedence of the plain forms, so a null pointer or a bad shape is answered in front of master + f32 in
    Adam's too."""
    lib = _lib.lib()
    assert lib.dctn_flat_step_bytes() == ctypes.sizeof(_lib.FlatStep) == 88
    adam = "adam" in name
    options = ("master", "guard", "schedule", "groups")
    ran = 0
    for case, broken in cases(name).items():
        if any(broken.get(o, P) is None for o in options):
            continue
        v = values(name, broken)
        if "dtype" not in ENTRY[name][0]:
            v["dtype"] = _lib.BF16   # the _master forms have no dtype argument: it is bf16
        step = _lib.FlatStep(**{f: v[f] for f, _ in _lib.FlatStep._fields_})
        if adam:
            got = lib.dctn_adam_flat_step(ctypes.byref(step), v["exp_avg"], v["exp_avg_sq"], v["beta1"], v["beta2"], v["eps"],
                                          v["weight_decay"], None)
        else:
            got = lib.dctn_sgd_flat_step(ctypes.byref(step), v["momentum_buf"], v["lr"], v["momentum"], v["first_step"], None)
        want = TABLE[name][case]
        if adam and case.endswith(" & master+f32"):   # the other bad argument is answered first here
            want = TABLE[name][case[:-len(" & master+f32")]]
        assert got == want, (name, case)
        ran += 1
    assert ran >= 7
    assert lib.dctn_adam_flat_step(None, P, P, 0.9, 0.999, 1e-8, 0.0, None) == NULL
    assert lib.dctn_sgd_flat_step(None, P, 0.1, 0.9, 1, None) == NULL


if __name__ == "__main__":
    library = _bound(sys.argv[1])
    for entry in ENTRY:
        print(f'    "{entry}": {{')
        for case_name, broken_args in cases(entry).items():
            print(f'        "{case_name}": {legacy_call(library, entry, broken_args)},')
        print("    },")
