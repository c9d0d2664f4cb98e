"""Host-side checks of the gradient guard: the entry points are declared, exported and bound with the registered
signatures, the guard block is 32 bytes, the entry points validate their arguments before any launch, and the Python
mirror of the kernel's decision agrees with torch.nn.utils.clip_grad_norm_ (no GPU needed)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from dctn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_void, c_i64, c_int, c_size = _lib.c_void, _lib.c_i64, _lib.c_int, _lib.c_size
c_float, c_double = ctypes.c_float, ctypes.c_double
ADAM_TAIL = [c_i64, c_i64, c_double, c_double, c_float, c_float, c_float]
SGD_TAIL = [c_i64, c_i64, c_float, c_float, c_float, c_int]
EXPECTED = {
    "dctn_grad_guard_state_bytes": (c_size, []),
    "dctn_grad_guard_num_partials": (c_int, [c_i64]),
    "dctn_grad_guard_check": (c_int, [c_void, c_i64, c_int, c_void, c_void, c_void, c_void]),
    "dctn_adam_l2_step_guarded": (c_int, [c_void] * 7 + ADAM_TAIL + [c_int, c_void]),
    "dctn_adam_l2_step_master_guarded": (c_int, [c_void] * 8 + ADAM_TAIL + [c_void]),
    "dctn_sgd_l2_step_guarded": (c_int, [c_void] * 5 + SGD_TAIL + [c_int, c_void]),
    "dctn_sgd_l2_step_master_guarded": (c_int, [c_void] * 6 + SGD_TAIL + [c_void]),
}


def test_guard_entry_points_are_in_header_library_and_bindings():
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
    # a guarded step is its unguarded sibling with one more pointer (the guard block) behind the last buffer
    for name, at in (("dctn_adam_l2_step", 6), ("dctn_adam_l2_step_master", 7), ("dctn_sgd_l2_step", 4),
                     ("dctn_sgd_l2_step_master", 5)):
        sib = list(_lib.SIGNATURES[name][1])
        assert list(_lib.SIGNATURES[name + "_guarded"][1]) == sib[:at] + [c_void] + sib[at:]


def test_version_and_block_size():
    lib = _lib.lib()
    assert lib.dctn_version() >= 505
    assert lib.dctn_grad_guard_state_bytes() == 32
    header = open(os.path.join(ROOT, "include", "dctn_amd.h")).read()
    for field in ("max_norm", "last_norm", "halted", "bad_step", "seen", "clipped", "ticket", "coef"):
        assert re.search(r"\*\s+(float|uint32|int32)\s+" + field + r"\b", header), f"the header does not document `{field}`"


def test_num_partials_follows_the_grid_rule():
    """Workgroups of 1024 threads with one 4-element access per lane, at most 256 of them (the rule of flat_step_k's 1024-thread geometry)."""
    lib = _lib.lib()
    for n, want in ((-1, 0), (0, 0), (1, 1), (4096, 1), (4097, 2), (262147, 65), (256 * 4096, 256), (1048581, 256),
                    (1 << 40, 256)):
        assert lib.dctn_grad_guard_num_partials(n) == want, n
        assert lib.dctn_grad_guard_num_partials(n) == lib.dctn_adam_l2_num_partials(n)


def test_entry_points_validate_their_arguments_without_a_device():
    lib = _lib.lib()
    check = lib.dctn_grad_guard_check
    assert check(None, 4, _lib.F32, None, 8, 8, None) == _lib.ERR_NULL
    assert check(8, 4, _lib.F32, None, None, 8, None) == _lib.ERR_NULL
    assert check(8, 4, _lib.F32, None, 8, None, None) == _lib.ERR_NULL
    assert check(8, 0, _lib.F32, None, 8, 8, None) == _lib.ERR_BAD_SHAPE
    assert check(8, -2, _lib.BF16, None, 8, 8, None) == _lib.ERR_BAD_SHAPE
    assert check(8, 4, _lib.F64, None, 8, 8, None) == _lib.ERR_BAD_DTYPE
    adam, adam_m = lib.dctn_adam_l2_step_guarded, lib.dctn_adam_l2_step_master_guarded
    tail = (4, 2, 0.9, 0.999, 1e-8, 0.0, 0.0)
    assert adam(8, 8, 8, 8, None, 8, None, *tail, _lib.F32, None) == _lib.ERR_NULL        # no guard block
    assert adam(None, 8, 8, 8, None, 8, 8, *tail, _lib.F32, None) == _lib.ERR_NULL
    assert adam(8, 8, 8, 8, None, 8, 8, 0, 0, *tail[2:], _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert adam(8, 8, 8, 8, None, 8, 8, *tail, _lib.F64, None) == _lib.ERR_BAD_DTYPE
    assert adam_m(None, 8, 8, 8, 8, None, 8, 8, *tail, None) == _lib.ERR_NULL            # no master
    assert adam_m(8, 8, 8, 8, 8, None, 8, None, *tail, None) == _lib.ERR_NULL            # no guard block
    assert adam_m(8, 8, 8, 8, 8, None, 8, 8, 4, 5, *tail[2:], None) == _lib.ERR_BAD_SHAPE
    sgd, sgd_m = lib.dctn_sgd_l2_step_guarded, lib.dctn_sgd_l2_step_master_guarded
    stail = (4, 2, 1e-3, 0.9, 0.0, 1)
    assert sgd(8, 8, 8, None, None, *stail, _lib.F32, None) == _lib.ERR_NULL
    assert sgd(8, 8, 8, None, 8, 0, 0, *stail[2:], _lib.F32, None) == _lib.ERR_BAD_SHAPE
    assert sgd(8, 8, 8, None, 8, *stail, _lib.F64, None) == _lib.ERR_BAD_DTYPE
    assert sgd_m(None, 8, 8, 8, None, 8, *stail, None) == _lib.ERR_NULL
    assert sgd_m(8, 8, 8, 8, None, None, *stail, None) == _lib.ERR_NULL
    assert sgd_m(8, 8, 8, 8, None, 8, 4, -1, *stail[2:], None) == _lib.ERR_BAD_SHAPE


@pytest.mark.parametrize("case, max_norm", [("below", 7.0), ("above", 2.0), ("exactly at", 5.0), ("never", float("inf"))])
def test_decision_mirror_matches_clip_grad_norm(case, max_norm):
    """float64 gradients on the CPU through torch.nn.utils.clip_grad_norm_: what it multiplied them by is the mirror's
    coefficient up to the mirror's two float32 roundings (the norm, the quotient): a relative 2^-22."""
    from dctn_amd.training import GradGuard

    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(301, dtype=torch.float64, generator=g), torch.randn(7, 11, dtype=torch.float64, generator=g)]
    scale = 5.0 / float(torch.cat([t.reshape(-1) for t in grads]).norm())
    grads = [t * scale for t in grads]
    flat = torch.cat([t.reshape(-1) for t in grads])
    if case == "exactly at":   # a norm that IS the threshold, in float64 and float32: (3, 4, 0, ...)
        grads = [torch.zeros(301, dtype=torch.float64), torch.zeros(7, 11, dtype=torch.float64)]
        grads[0][0], grads[1][2, 3] = 3.0, 4.0
        flat = torch.cat([t.reshape(-1) for t in grads])
        assert float(flat.norm()) == 5.0
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in grads]
    for p, t in zip(params, grads):
        p.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    big = int(flat.abs().argmax())
    torch_coef = float(torch.cat([p.grad.reshape(-1) for p in params])[big] / flat[big])
    apply, coef, norm = GradGuard.decide(float((flat * flat).sum()), max_norm)
    print(f"\n{case}: torch coef={torch_coef!r} mirror coef={coef!r} norm torch={float(total)!r} mirror={norm!r}")
    assert apply
    assert abs(norm - float(total)) <= 2.0 ** -23 * float(total)
    assert abs(coef - torch_coef) <= 2.0 ** -22 * torch_coef
    if case in ("below", "never"):
        assert coef == 1.0 and torch_coef == 1.0
    else:
        assert coef < 1.0 and torch_coef < 1.0


def test_decision_mirror_halts_on_non_finite_values_and_on_the_latch():
    from dctn_amd.training import GradGuard

    for total in (float("inf"), float("nan")):
        assert GradGuard.decide(total, 1.0)[:2] == (False, 0.0)
    assert GradGuard.decide(4.0, 1.0, loss=float("nan"))[:2] == (False, 0.0)
    assert GradGuard.decide(4.0, 1.0, loss=float("-inf"))[:2] == (False, 0.0)
    assert GradGuard.decide(4.0, 1.0, halted_before=True)[:2] == (False, 0.0)
    assert GradGuard.decide(4.0, 1.0, loss=0.25) == (True, float(torch.tensor(1.0 / (2.0 + 1e-6), dtype=torch.float32)), 2.0)
    # 2^20 squares of 3e19: beyond float32, far inside float64 - finite, so the step is applied
    assert GradGuard.decide(float(2 ** 20) * 3e19 ** 2, float("inf")) == (True, 1.0, float(torch.tensor(1024 * 3e19, dtype=torch.float32)))


def test_optimizers_and_hooks_take_a_guard_and_default_to_none():
    from dctn_amd import training

    for cls in (training.FlatAdam, training.FlatSGD):
        params = inspect.signature(cls.__init__).parameters
        assert params["guard"].default is None and params["guard_loss"].default is None
    for name in ("read", "reset", "state_dict", "load_state_dict", "check", "decide"):
        assert callable(getattr(training.GradGuard, name)), name
    assert isinstance(training.GradGuard.max_norm, property) and isinstance(training.GradGuard.halted, property)
    assert list(inspect.signature(training.make_stopper_on_device_halt).parameters) == ["dir", "guard", "every"]
    assert training.GradGuard.FIELDS == ("max_norm", "last_norm", "halted", "bad_step", "seen", "clipped", "ticket", "coef")
