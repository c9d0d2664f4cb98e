"""Host-side checks of the Adam step and the fused scoring entry points: they are declared, exported and bound, and
they validate their arguments before any launch (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from dctn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dctn_adam_l2_step", "dctn_adam_state_bytes", "dctn_adam_l2_num_partials", "dctn_ce_score_accumulate")


def test_new_entry_points_are_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    declared = set(re.findall(r"\b(dctn_[a-z0-9_]+)\s*\(", header))
    exported = set()
    for line in subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] == "T":
            exported.add(parts[2])
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/dctn_amd.h"
        assert name in exported, f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"


def test_adam_state_block_size_is_the_documented_one():
    assert _lib.lib().dctn_adam_state_bytes() == 16
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    assert "dctn_adam_state_bytes() = 16" in header


def test_adam_partials_count_is_one_slot_per_workgroup():
    count = _lib.lib().dctn_adam_l2_num_partials
    assert [count(n) for n in (-1, 0, 1, 4096, 4097, 29_000, 1_900_000, 1 << 40)] == [0, 0, 1, 1, 2, 8, 256, 256]


def test_adam_step_validates_its_arguments_without_a_device():
    step = _lib.lib().dctn_adam_l2_step
    ok = dict(params=8, grads=8, m=8, v=8, sq=None, state=8, n=4, n_reg=2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, l2=0.0,
              dtype=_lib.F32)

    def call(**kw):
        a = {**ok, **kw}
        return step(a["params"], a["grads"], a["m"], a["v"], a["sq"], a["state"], a["n"], a["n_reg"], a["b1"], a["b2"],
                    a["eps"], a["wd"], a["l2"], a["dtype"], None)

    for name in ("params", "grads", "m", "v", "state"):
        assert call(**{name: None}) == _lib.ERR_NULL, name
    assert call(n=0) == _lib.ERR_BAD_SHAPE
    assert call(n=-3) == _lib.ERR_BAD_SHAPE
    assert call(n_reg=5) == _lib.ERR_BAD_SHAPE
    assert call(n_reg=-1) == _lib.ERR_BAD_SHAPE
    assert call(b1=1.0) == _lib.ERR_BAD_SHAPE and call(b2=-0.1) == _lib.ERR_BAD_SHAPE
    assert call(dtype=_lib.F64) == _lib.ERR_BAD_DTYPE      # float32 / bfloat16 only
    assert call(dtype=7) == _lib.ERR_BAD_DTYPE


def test_score_accumulate_validates_its_arguments_without_a_device():
    acc = _lib.lib().dctn_ce_score_accumulate
    assert acc(None, 8, 8, 4, 10, _lib.F32, None) == _lib.ERR_NULL
    assert acc(8, None, 8, 4, 10, _lib.F32, None) == _lib.ERR_NULL
    assert acc(8, 8, None, 4, 10, _lib.F32, None) == _lib.ERR_NULL
    assert acc(8, 8, 8, 0, 10, _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert acc(8, 8, 8, 4, 0, _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert acc(8, 8, 8, 4, 10, _lib.F64, None) == _lib.ERR_BAD_DTYPE


def test_score_fused_needs_a_gpu_device():
    import torch

    from dctn_amd.evaluation import score_fused

    with pytest.raises(RuntimeError, match="MI355X"):
        score_fused(lambda x: x, [], torch.device("cpu"))


def test_flat_optimizers_share_their_construction():
    from dctn_amd.training import FlatAdam, FlatSGD, _FlatOptimizer

    assert issubclass(FlatAdam, _FlatOptimizer) and issubclass(FlatSGD, _FlatOptimizer)
    for name in ("zero_grad", "step", "reg_value", "state_dict", "load_state_dict"):
        assert callable(getattr(FlatAdam, name))
    assert isinstance(FlatAdam.lr, property) and FlatAdam.lr.fset is not None
