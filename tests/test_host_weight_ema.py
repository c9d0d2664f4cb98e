"""The weight average (EMA) of the flat optimizers on the host: exports and sizes, the per-launch weight of the library
against `WeightEMA.weight` bit for bit, the return codes of the four launching entry points in their stated order (every
call returns before a launch: the device pointers are dummy integers), the float32 mirror of the element update against
a float64 recurrence, and the refusals that need no device.  (``apply()`` twice needs a first launch: it is in
tests/test_gpu_weight_ema.py.)"""
import ctypes
import math

import numpy as np
import pytest
import torch

from dctn_amd import _lib

P = 8   # a non-null dummy pointer: no call here gets as far as using one
NULL, SHAPE, DTYPE, OK = _lib.ERR_NULL, _lib.ERR_BAD_SHAPE, _lib.ERR_BAD_DTYPE, 0
DECAYS = [0.0, 0.5, 0.9, 0.999, 0.9999, 1.0 - 2.0 ** -24]
NEW = ["dctn_weight_ema_bytes", "dctn_weight_ema_weight", "dctn_adam_flat_step_ema", "dctn_sgd_flat_step_ema",
       "dctn_weight_ema_apply", "dctn_weight_ema_restore"]


def _block(decay, flags=0, updates=0, last_omd=0.0):
    words = np.zeros(8, dtype=np.int32)
    words.view(np.float32)[0] = decay
    words.view(np.uint32)[1] = flags
    words[2] = updates
    words.view(np.float32)[3] = last_omd
    return words


def _library_weight(words, updates):
    out = ctypes.c_float(-1.0)
    rc = _lib.lib().dctn_weight_ema_weight(words.ctypes.data, updates, ctypes.byref(out))
    return rc, out.value


def test_exports_and_sizes():
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.dctn_version() >= 513
    assert lib.dctn_weight_ema_bytes() == 32
    assert ctypes.sizeof(_lib.WeightEma) == 16
    assert lib.dctn_flat_step_bytes() == ctypes.sizeof(_lib.FlatStep) == 88


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
def test_the_librarys_weight_is_the_python_mirror_bit_for_bit(warmup):
    from dctn_amd.training import WeightEMA

    counts = list(range(2001)) + [2 ** k for k in range(11, 31)]
    assert counts[-1] == 2 ** 30
    for decay in DECAYS:
        words = _block(decay, flags=1 if warmup else 0)
        for u in counts:
            rc, got = _library_weight(words, u)
            want = WeightEMA.weight(decay, warmup, u)
            assert rc == OK and np.float32(got).tobytes() == np.float32(want).tobytes(), (decay, warmup, u, got, want)
    # what the numbers are: without warm-up one value; with it the ramp (1 + u) / (10 + u) until it passes the decay
    assert WeightEMA.weight(0.999, False, 0) == WeightEMA.weight(0.999, False, 10 ** 6) == float(np.float32(1.0 - float(np.float32(0.999))))
    assert WeightEMA.weight(0.999, True, 0) == float(np.float32(0.9))
    assert WeightEMA.weight(0.0, True, 5) == 1.0 and WeightEMA.weight(0.0, False, 5) == 1.0
    assert WeightEMA.weight(0.999, True, 10 ** 6) == WeightEMA.weight(0.999, False, 0)


def test_the_librarys_weight_rejects_a_bad_block():
    for decay in (1.0, -0.1, float("nan"), float("inf"), -float("inf"), 1.5):
        assert _library_weight(_block(decay), 0)[0] == SHAPE, decay
    for flags in (2, 3, 1 << 31):
        assert _library_weight(_block(0.9, flags=flags), 0)[0] == SHAPE, flags
    assert _library_weight(_block(0.9, updates=-1), 0)[0] == SHAPE
    assert _library_weight(_block(0.9), -1)[0] == SHAPE
    assert _library_weight(_block(0.9, flags=1, updates=7, last_omd=0.25), 7)[0] == OK
    out = ctypes.c_float()
    lib = _lib.lib()
    assert lib.dctn_weight_ema_weight(None, 0, ctypes.byref(out)) == NULL
    assert lib.dctn_weight_ema_weight(_block(0.9).ctypes.data, 0, None) == NULL
    assert lib.dctn_weight_ema_weight(None, -1, None) == NULL            # NULL in front of the shape


def _step(**broken):
    v = dict(params=P, master=None, grads=P, sq_sum=None, state=P, guard=None, schedule=None, groups=None, n=4, n_reg=2,
             l2=0.0, dtype=_lib.F32)
    v.update(broken)
    return _lib.FlatStep(**v)


def _adam(step, ema, exp_avg=P, exp_avg_sq=P, beta1=0.9):
    return _lib.lib().dctn_adam_flat_step_ema(None if step is None else ctypes.byref(step),
                                              None if ema is None else ctypes.byref(ema), exp_avg, exp_avg_sq, beta1, 0.999,
                                              1e-8, 0.0, None)


def _sgd(step, ema, buf=P):
    return _lib.lib().dctn_sgd_flat_step_ema(None if step is None else ctypes.byref(step),
                                             None if ema is None else ctypes.byref(ema), buf, 0.1, 0.9, 1, None)


def test_the_step_entry_points_answer_null_then_shape_then_dtype():
    good = _lib.WeightEma(ema=P, block=P)
    no_values, no_block = _lib.WeightEma(ema=None, block=P), _lib.WeightEma(ema=P, block=None)
    for call in (_adam, _sgd):
        assert call(None, good) == NULL
        for bad in (no_values, no_block):
            assert call(_step(), bad) == NULL
            assert call(_step(n=0), bad) == NULL                          # NULL in front of the shape
            assert call(_step(dtype=_lib.F64), bad) == NULL               # and of the dtype
        assert call(_step(params=None), good) == NULL
        assert call(_step(grads=None, n=0), good) == NULL
        assert call(_step(state=None), good) == NULL                      # SGD: the step block is required with an average
        assert call(_step(state=None, n_reg=5), good) == NULL
        for shape in (dict(n=0), dict(n_reg=5), dict(n_reg=-1)):
            assert call(_step(**shape), good) == SHAPE
            assert call(_step(dtype=_lib.F64, **shape), good) == SHAPE    # the shape in front of the dtype
        assert call(_step(dtype=_lib.F64), good) == DTYPE
        assert call(_step(master=P, dtype=_lib.F32), good) == DTYPE       # a master copy goes with bf16
        # ema_or_null == NULL is the plain entry point: the same answers, and SGD then does not look at the step block
        assert call(_step(n=0), None) == SHAPE and call(_step(params=None), None) == NULL
        assert call(_step(dtype=_lib.F64), None) == DTYPE
    assert _adam(_step(), good, exp_avg=None) == NULL and _adam(_step(), good, beta1=1.0) == SHAPE
    assert _adam(_step(state=None), None) == NULL
    assert _sgd(_step(), good, buf=None) == NULL
    assert _sgd(_step(state=None, n=0), None) == SHAPE                    # no average, no schedule, no table: not required


def test_apply_and_restore_answer_null_then_shape_then_dtype():
    lib = _lib.lib()
    assert lib.dctn_weight_ema_apply(None, P, P, 4, _lib.F32, None) == NULL
    assert lib.dctn_weight_ema_apply(P, None, P, 0, _lib.F32, None) == NULL
    assert lib.dctn_weight_ema_apply(P, P, None, 4, _lib.F64, None) == NULL
    assert lib.dctn_weight_ema_apply(P, P, P, 0, _lib.F32, None) == SHAPE
    assert lib.dctn_weight_ema_apply(P, P, P, -3, _lib.F64, None) == SHAPE
    assert lib.dctn_weight_ema_apply(P, P, P, 4, _lib.F64, None) == DTYPE
    assert lib.dctn_weight_ema_apply(P, P, P, 4, 7, None) == DTYPE
    assert lib.dctn_weight_ema_restore(None, P, 4, _lib.BF16, None) == NULL
    assert lib.dctn_weight_ema_restore(P, None, 0, _lib.F64, None) == NULL
    assert lib.dctn_weight_ema_restore(P, P, 0, _lib.F64, None) == SHAPE
    assert lib.dctn_weight_ema_restore(P, P, 4, _lib.F64, None) == DTYPE


@pytest.mark.parametrize("decay", [0.0, 0.9, 0.999, 0.9999])
def test_the_mirror_stays_within_three_roundings_per_update_of_float64(decay):
    """200 updates on n = 12295 random weights.  The float64 recurrence takes the same float32 omd.  Each of the three
    float32 roundings of an update is at most 2^-24 * 2M (M: the largest |w| or |ema| seen so far; the difference is at
    most 2M, the product no larger, the sum at most M), and the recurrence does not amplify an error already made
    (its factor is d <= 1): after T updates the distance is at most 3 * T * M * 2^-23."""
    from dctn_amd.training import WeightEMA

    n, T = 12295, 200
    rng = np.random.default_rng(97)
    w = (rng.standard_normal(n) * 0.02).astype(np.float32)
    ema32, ema64 = w.copy(), w.astype(np.float64)
    M = float(np.abs(w).max())
    worst = 0.0
    for t in range(T):
        w = (w + rng.standard_normal(n).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
        omd = WeightEMA.weight(decay, True, t)
        ema32 = WeightEMA.mirror(ema32, w, omd)
        assert ema32.dtype == np.float32
        ema64 = ema64 + float(omd) * (w.astype(np.float64) - ema64)
        M = max(M, float(np.abs(w).max()), float(np.abs(ema32).max()))
        bound = 3.0 * (t + 1) * M * 2.0 ** -23
        err = float(np.abs(ema32.astype(np.float64) - ema64).max())
        worst = max(worst, err / bound)
        assert err <= bound, (decay, t, err, bound)
    print(f"decay {decay}: worst ratio to the bound {worst:.3f}")
    assert worst > 0.0 or decay == 0.0


def test_the_mirror_is_three_rounded_float32_operations():
    from dctn_amd.training import WeightEMA

    ema = np.array([1.0, 3.0, -2.5, 1e-8], dtype=np.float32)
    w = np.array([1.0000001, -1.0, 7.25, 1.0], dtype=np.float32)
    omd = np.float32(0.1)
    got = WeightEMA.mirror(ema, w, float(omd))
    want = np.array([np.float32(e + np.float32(omd * np.float32(x - e))) for e, x in zip(ema, w)], dtype=np.float32)
    assert got.tobytes() == want.tobytes()
    assert WeightEMA.mirror(ema, w, 1.0).dtype == np.float32


def _params(dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    return [torch.nn.Parameter(torch.randn(7, 3, generator=g).to(dtype)), torch.nn.Parameter(torch.randn(5, generator=g).to(dtype))]


def _cpu_adam(ema, dtype=torch.float32, **kw):
    """A FlatAdam on the CPU: with a schedule, whose rate needs no device write at construction."""
    from dctn_amd.training import FlatAdam, LRSchedule

    return FlatAdam(_params(dtype), [], schedule=LRSchedule.constant("cpu", 1e-3), ema=ema, **kw)


def test_binding_allocates_the_values_from_the_weights_the_optimizer_keeps():
    from dctn_amd.training import FlatSGD, WeightEMA

    e = WeightEMA("cpu", decay=0.99, warmup=False)
    assert e.values is None and e.decay == float(np.float32(0.99)) and not e.is_applied
    assert np.array_equal(e._block.numpy(), e.host_block()) and e.updates == 0 and e.last_omd == 0.0
    opt = _cpu_adam(e, torch.bfloat16, master_weights=True)
    assert e.values.dtype == torch.float32 and e.values.shape == (26,) and torch.equal(e.values, opt.master)
    assert e._stash.dtype == torch.bfloat16 and e._stash.shape == (26,)
    assert [name for name, _ in opt.run_regions()] == ["flat", "m", "v", "master", "ema", "ema_block", "schedule", "state", "sq_sum"]
    plain = WeightEMA("cpu")
    sgd = FlatSGD(_params(torch.bfloat16), [], lr=0.25, ema=plain)
    assert torch.equal(plain.values, sgd.flat.float())                         # no master copy: the exact widening
    assert sgd._state is not None and float(sgd._state.view(torch.float32)[1]) == 0.25   # the step block, with the rate
    assert [name for name, _ in sgd.run_regions()] == ["flat", "buf", "ema", "ema_block", "state", "sq_sum"]
    sgd.lr = 0.125
    assert float(sgd._state.view(torch.float32)[1]) == 0.125
    assert "weight average" in sgd._what and "weight average" in opt._what
    state = opt.state_dict()
    assert torch.equal(state["ema"]["values"], e.values) and state["ema"]["updates"] == 0
    e.decay = 0.5
    assert e.decay == 0.5 and e._block.view(torch.float32)[0] == 0.5
    for bad in (1.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="decay"):
            e.decay = bad
        with pytest.raises(ValueError, match="decay"):
            WeightEMA("cpu", decay=bad)


def test_host_only_refusals():
    from dctn_amd.training import FlatAdam, FlatSGD, LRSchedule, WeightEMA

    e = WeightEMA("cpu")
    with pytest.raises(RuntimeError, match="not applied"):
        e.restore()
    with pytest.raises(RuntimeError, match="not bound"):
        e.apply()
    with pytest.raises(RuntimeError, match="not bound"):
        e.reset()
    for not_one in (0.999, "ema", LRSchedule.constant("cpu", 1e-3)):
        with pytest.raises(TypeError, match="WeightEMA"):
            _cpu_adam(not_one)
        with pytest.raises(TypeError, match="WeightEMA"):
            FlatSGD(_params(), [], ema=not_one)
    elsewhere = WeightEMA("cpu")
    elsewhere.device = torch.device("cuda:0")     # (only the check looks at it here)
    with pytest.raises(ValueError, match="is on cuda:0"):
        _cpu_adam(elsewhere)
    opt = _cpu_adam(e)
    with pytest.raises(RuntimeError, match="not applied"):
        e.restore()
    with pytest.raises(ValueError, match="already belongs"):
        _cpu_adam(e)
    # while applied (the flag alone: no launch here) the step, a second apply, reset and the state are refused
    e._applied = True
    for p in opt.params:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="while the weight average is applied"):
        opt.step()
    with pytest.raises(RuntimeError, match="already applied"):
        e.apply()
    with pytest.raises(RuntimeError, match="applied"):
        e.reset()
    with pytest.raises(RuntimeError, match="applied"):
        e.load_state_dict(e.state_dict())
    e._applied = False
    assert isinstance(opt, FlatAdam) and math.isfinite(e.decay)


def test_a_state_without_the_average_resets_it_from_the_parameters():
    from dctn_amd.training import WeightEMA

    e = WeightEMA("cpu", decay=0.9)
    opt = _cpu_adam(e)
    state = opt.state_dict()
    saved = state["ema"]
    saved["values"] = saved["values"] + 1.0
    saved["updates"], saved["last_omd"], saved["decay"], saved["warmup"] = 17, 0.25, 0.75, False
    opt.load_state_dict(state)
    assert torch.equal(e.values, saved["values"]) and (e.updates, e.last_omd, e.decay, e.warmup) == (17, 0.25, 0.75, False)
    del state["ema"]
    opt.load_state_dict(state)
    assert torch.equal(e.values, opt.flat) and e.updates == 0 and e.last_omd == 0.0
    with pytest.raises(ValueError, match="averaged values"):
        e.load_state_dict(dict(saved, values=torch.zeros(3)))
    # the run-state mirror follows the block's bytes
    e.run_restored(None, {"ema_block": WeightEMA("cpu", decay=0.5, warmup=False).host_block(3, 0.5).view(np.uint8)})
    assert e.decay == 0.5 and e.warmup is False
