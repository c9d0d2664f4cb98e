"""Host-side checks of the master-weight forms of the Adam and SGD steps: they are declared, exported and bound, and
they validate their arguments before any launch (no GPU needed)."""
import inspect
import os
import re
import subprocess

from dctn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dctn_adam_l2_step_master", "dctn_sgd_l2_step_master")


def test_master_entry_points_are_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    exported = set()
    for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "T":
            exported.add(parts[2])
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(void\*\s+master\b", header), f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    # one more pointer in front, no dtype argument; everything else is the sibling's signature
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        sib_res, sib_args = _lib.SIGNATURES[name[: -len("_master")]]
        assert res is sib_res
        assert args == [_lib.c_void] + sib_args[:-2] + sib_args[-1:]
    assert _lib.lib().dctn_version() >= 501


def test_adam_master_step_validates_its_arguments_without_a_device():
    step = _lib.lib().dctn_adam_l2_step_master
    ok = dict(master=8, params=8, grads=8, m=8, v=8, sq=None, state=8, n=4, n_reg=2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0,
              l2=0.0)

    def call(**kw):
        a = {**ok, **kw}
        return step(a["master"], a["params"], a["grads"], a["m"], a["v"], a["sq"], a["state"], a["n"], a["n_reg"],
                    a["b1"], a["b2"], a["eps"], a["wd"], a["l2"], None)

    for name in ("master", "params", "grads", "m", "v", "state"):
        assert call(**{name: None}) == _lib.ERR_NULL, name
    assert call(n=0) == _lib.ERR_BAD_SHAPE
    assert call(n=-3) == _lib.ERR_BAD_SHAPE
    assert call(n_reg=5) == _lib.ERR_BAD_SHAPE
    assert call(n_reg=-1) == _lib.ERR_BAD_SHAPE
    assert call(b1=1.0) == _lib.ERR_BAD_SHAPE and call(b2=-0.1) == _lib.ERR_BAD_SHAPE


def test_sgd_master_step_validates_its_arguments_without_a_device():
    step = _lib.lib().dctn_sgd_l2_step_master
    ok = dict(master=8, params=8, grads=8, buf=8, sq=None, n=4, n_reg=2)

    def call(**kw):
        a = {**ok, **kw}
        return step(a["master"], a["params"], a["grads"], a["buf"], a["sq"], a["n"], a["n_reg"], 1e-3, 0.9, 0.0, 1, None)

    for name in ("master", "params", "grads", "buf"):
        assert call(**{name: None}) == _lib.ERR_NULL, name
    assert call(n=0) == _lib.ERR_BAD_SHAPE
    assert call(n=-3) == _lib.ERR_BAD_SHAPE
    assert call(n_reg=5) == _lib.ERR_BAD_SHAPE
    assert call(n_reg=-1) == _lib.ERR_BAD_SHAPE


def test_flat_optimizers_take_master_weights_and_default_to_off():
    from dctn_amd.training import FlatAdam, FlatSGD

    for cls in (FlatAdam, FlatSGD):
        assert inspect.signature(cls.__init__).parameters["master_weights"].default is False
        for name in ("refresh_master", "state_dict", "load_state_dict"):
            assert callable(getattr(cls, name)), f"{cls.__name__}.{name}"


def test_train_refreshes_the_master_copy_after_its_broadcast():
    """`train` receives the optimizer already built and broadcasts rank 0's model afterwards: the refresh must come
    after the broadcast and before the loop (the GPU test with two ranks shows what happens otherwise)."""
    from dctn_amd import training

    src = inspect.getsource(training.train)
    assert src.index("broadcast_parameters(") < src.index("refresh_master()") < src.index("batches_forever(")
