"""What `FlatRMSprop` and `FlatSGD(weight_decay=...)` promise without a GPU: the exports of version 515, the return codes
of dctn_rmsprop_flat_step and dctn_sgd_flat_step_decay in the order include/dctn_amd.h states (every call here returns
before a launch), the signatures of the two constructors, and `LRSchedule.per_epoch`."""
import ctypes
import inspect
import math

import numpy as np
import pytest

from dctn_amd import _lib

P = 8   # a non-null dummy pointer: no call here gets as far as using one
NULL, SHAPE, DTYPE = _lib.ERR_NULL, _lib.ERR_BAD_SHAPE, _lib.ERR_BAD_DTYPE
NAN, INF = float("nan"), float("inf")


def test_the_exports_exist():
    lib = _lib.lib()
    assert lib.dctn_version() >= 515
    for name in ("dctn_rmsprop_flat_step", "dctn_rmsprop_num_partials", "dctn_sgd_flat_step_decay"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    # Adam's geometry of flat_step_k: one workgroup per 4096 elements, at most 256
    for n, want in ((-1, 0), (0, 0), (1, 1), (4096, 1), (4097, 2), (20007, 5), (256 * 4096, 256), (1 << 33, 256)):
        assert lib.dctn_rmsprop_num_partials(n) == want == lib.dctn_adam_l2_num_partials(n)


def _step(**broken):
    v = dict(params=P, master=None, grads=P, sq_sum=None, state=P, guard=None, schedule=None, groups=None, n=4, n_reg=2,
             l2=0.0, dtype=_lib.F32)
    v.update(broken)
    return _lib.FlatStep(**v)


def _rms(step=None, ema="none", square_avg=P, buf=P, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.9, **broken):
    step = _step(**broken) if step is None else step
    ema_ref = None if ema == "none" else ctypes.byref(_lib.WeightEma(ema=ema[0], block=ema[1]))
    return _lib.lib().dctn_rmsprop_flat_step(None if step == "null" else ctypes.byref(step), ema_ref, square_avg, buf,
                                             alpha, eps, weight_decay, momentum, None)


def _sgd(step=None, ema="none", buf=P, lr=0.1, momentum=0.9, weight_decay=0.0, first_step=1, **broken):
    step = _step(**dict(dict(state=None), **broken)) if step is None else step
    ema_ref = None if ema == "none" else ctypes.byref(_lib.WeightEma(ema=ema[0], block=ema[1]))
    return _lib.lib().dctn_sgd_flat_step_decay(None if step == "null" else ctypes.byref(step), ema_ref, buf, lr, momentum,
                                               weight_decay, first_step, None)


RMS_NULL = [dict(step="null"), dict(params=None), dict(grads=None), dict(square_avg=None), dict(state=None),
            dict(ema=(None, P)), dict(ema=(P, None)), dict(buf=None, momentum=0.9), dict(buf=None, momentum=1e-30)]
RMS_SHAPE = [dict(n=0), dict(n=-3), dict(n_reg=-1), dict(n_reg=5), dict(alpha=1.0), dict(alpha=-0.1), dict(alpha=NAN),
             dict(alpha=INF), dict(alpha=-INF), dict(momentum=-0.5), dict(momentum=NAN), dict(eps=-1e-8), dict(eps=NAN),
             dict(weight_decay=-1e-3), dict(weight_decay=NAN)]
RMS_DTYPE = [dict(dtype=_lib.F64), dict(dtype=99), dict(master=P, dtype=_lib.F32)]


def test_rmsprop_return_codes_in_their_stated_order():
    for bad in RMS_NULL:
        assert _rms(**bad) == NULL, bad
    for bad in RMS_SHAPE:
        assert _rms(**bad) == SHAPE, bad
    for bad in RMS_DTYPE:
        assert _rms(**bad) == DTYPE, bad
    # a null pointer is answered in front of a bad shape, a bad shape in front of a bad dtype
    for first in RMS_NULL[1:]:
        for later in RMS_SHAPE + RMS_DTYPE:
            if not set(first) & set(later):
                assert _rms(**first, **later) == NULL, (first, later)
    for first in RMS_SHAPE:
        for later in RMS_DTYPE:
            assert _rms(**first, **later) == SHAPE, (first, later)
    # momentum 0: no buffer exists, so none is missed (the call fails later, on the dtype, and never launches)
    assert _rms(buf=None, momentum=0.0, dtype=_lib.F64) == DTYPE
    assert _rms(buf=None, momentum=0.5, dtype=_lib.F64) == NULL
    # with a group table the weight_decay argument is still validated; sq_sum and the options are optional
    assert _rms(groups=P, weight_decay=-1.0) == SHAPE
    assert _rms(sq_sum=None, guard=P, schedule=P, groups=P, ema=(P, P), dtype=_lib.F64) == DTYPE
    assert _rms(master=P, dtype=_lib.BF16, n=0) == SHAPE


SGD_NULL = [dict(step="null"), dict(params=None), dict(grads=None), dict(buf=None), dict(schedule=P), dict(groups=P),
            dict(ema=(P, P)), dict(ema=(None, P), state=P), dict(ema=(P, None), state=P)]
SGD_SHAPE = [dict(n=0), dict(n_reg=-1), dict(n_reg=5), dict(weight_decay=-1e-3), dict(weight_decay=NAN)]
SGD_DTYPE = [dict(dtype=_lib.F64), dict(master=P, dtype=_lib.F32)]


def test_decayed_sgd_return_codes_are_the_ema_entry_points_plus_the_decay():
    lib = _lib.lib()
    for bad in SGD_NULL:   # (a schedule, a table or an average without the step block: the block is missing)
        assert _sgd(**bad) == NULL, bad
    for bad in SGD_SHAPE:
        assert _sgd(**bad) == SHAPE, bad
    for bad in SGD_DTYPE:
        assert _sgd(**bad) == DTYPE, bad
    for first in SGD_NULL[1:]:
        for later in SGD_SHAPE + SGD_DTYPE:
            if not set(first) & set(later):
                assert _sgd(**first, **later) == NULL, (first, later)
    for first in SGD_SHAPE:
        for later in SGD_DTYPE:
            assert _sgd(**first, **later) == SHAPE, (first, later)
    # every other bad argument is answered as dctn_sgd_flat_step_ema answers it
    for bad in SGD_NULL[1:] + SGD_SHAPE[:3] + SGD_DTYPE:
        v = dict(bad)
        ema, buf = v.pop("ema", "none"), v.pop("buf", P)
        step = _step(**dict(dict(state=None), **v))
        ema_ref = None if ema == "none" else ctypes.byref(_lib.WeightEma(ema=ema[0], block=ema[1]))
        assert lib.dctn_sgd_flat_step_ema(ctypes.byref(step), ema_ref, buf, 0.1, 0.9, 1, None) == _sgd(**bad), bad


def test_the_constructors_signatures_and_defaults():
    from dctn_amd.training import FlatAdam, FlatRMSprop, FlatSGD, _FlatOptimizer

    sig = inspect.signature(FlatRMSprop.__init__)
    assert list(sig.parameters) == ["self", "regularised", "others", "lr", "alpha", "eps", "weight_decay", "momentum", "l2",
                                    "master_weights", "guard", "guard_loss", "schedule", "groups", "ema"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(others=(), lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, l2=0.0,
                            master_weights=False, guard=None, guard_loss=None, schedule=None, groups=None, ema=None)
    kinds = {k: p.kind for k, p in sig.parameters.items()}
    assert all(kinds[k] == inspect.Parameter.KEYWORD_ONLY for k in ("schedule", "groups", "ema"))
    assert kinds["guard_loss"] == inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert "centered" not in sig.parameters and issubclass(FlatRMSprop, _FlatOptimizer)
    sgd = inspect.signature(FlatSGD.__init__)
    assert list(sgd.parameters)[-1] == "weight_decay" and sgd.parameters["weight_decay"].default is None
    assert sgd.parameters["weight_decay"].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(sgd.parameters)[:-1] == ["self", "regularised", "others", "lr", "momentum", "l2", "master_weights", "guard",
                                         "guard_loss", "schedule", "groups", "ema"]
    assert list(inspect.signature(FlatAdam.__init__).parameters)[3:5] == ["lr", "betas"]   # (untouched)


def test_the_optimizers_on_the_cpu_refuse_what_they_must():
    """Construction needs no GPU: the buffers are torch tensors wherever the parameters live."""
    import torch

    from dctn_amd.training import FlatRMSprop, FlatSGD, ParamGroup, ParamGroups

    def params():
        return [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3))]

    for bad in (dict(alpha=1.0), dict(alpha=-0.1), dict(lr=-1.0), dict(eps=-1.0), dict(weight_decay=-1.0), dict(momentum=-0.1)):
        with pytest.raises(ValueError, match="RMSprop"):
            FlatRMSprop(params(), **bad)
    with pytest.raises(TypeError):
        FlatRMSprop(params(), centered=True)
    plain, heavy = FlatRMSprop(params()), FlatRMSprop(params(), momentum=0.9)
    assert plain.buf is None and plain._MOMENTS == ("square_avg",) and [n for n, _ in plain.run_regions()] == \
        ["flat", "square_avg", "state", "sq_sum"]
    assert heavy.buf is not None and heavy._MOMENTS == ("square_avg", "buf")
    assert plain.run_host() == dict(kind="FlatRMSprop", lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, l2=0.0)
    assert plain.sq_sum.numel() == 1 and plain.t == 0 and plain.lr == 1e-2
    # a table takes the optimizer's decay as its default, and may name its own
    ps = params()
    table = ParamGroups(ps, [ParamGroup(ps[1], weight_decay=0.5)])
    FlatRMSprop(ps, weight_decay=0.25, groups=table)
    assert table.weight_decays == [0.25, 0.5]
    # FlatSGD: None keeps the refusal and the keys; a float binds the table and adds the key
    ps = params()
    with pytest.raises(ValueError, match="FlatSGD has no weight decay: a ParamGroup for it must leave weight_decay=None"):
        FlatSGD(ps, groups=ParamGroups(ps, [ParamGroup(ps[1], weight_decay=0.5)]))
    ps = params()
    table = ParamGroups(ps, [ParamGroup(ps[1], weight_decay=0.5)])
    decayed = FlatSGD(ps, groups=table, weight_decay=0.0)
    assert table.weight_decays == [0.0, 0.5] and decayed.weight_decay == 0.0
    table.set(ps[0], weight_decay=0.125)
    assert table.weight_decays == [0.125, 0.5]
    old = FlatSGD(params())
    assert old.weight_decay is None and sorted(old.state_dict()) == ["buf", "l2", "lr", "momentum", "steps"]
    assert sorted(old.run_host()) == ["kind", "l2", "lr", "momentum", "steps"]
    new = FlatSGD(params(), weight_decay=0.0)
    assert sorted(new.state_dict()) == ["buf", "l2", "lr", "momentum", "steps", "weight_decay"]
    assert sorted(new.run_host()) == ["kind", "l2", "lr", "momentum", "steps", "weight_decay"]
    for bad in (-1e-3, NAN):
        with pytest.raises(ValueError, match="weight_decay"):
            FlatSGD(params(), weight_decay=bad)


def test_per_epoch_holds_one_rate_per_epoch():
    from dctn_amd.training import LRSchedule

    # the reference's classifier: lr * initial_multiplier ** ((W - epoch) / W) during W warm-up epochs, then lr
    lr, mult, W, epochs, spe = 1e-3, 1e-2, 10, 40, 7
    rates = [lr * mult ** (max(W - e, 0) / W) for e in range(epochs)]
    s = LRSchedule.per_epoch("cpu", rates, spe)
    assert s.hold == [1] * epochs and [k for k, _ in s.knots] == [e * spe for e in range(epochs)]
    lib = _lib.lib()
    block = s.host_block()
    out = ctypes.c_float()
    for step in list(range(0, epochs * spe + 3 * spe)) + [10 ** 6]:
        want = np.float32(rates[min(step // spe, epochs - 1)])
        assert np.float32(s.value(step)).tobytes() == want.tobytes(), step
        assert lib.dctn_lr_schedule_value(block.ctypes.data, step, ctypes.byref(out)) == 0
        assert np.float32(out.value).tobytes() == want.tobytes(), step
    assert len({s.value(e * spe) for e in range(epochs)}) == W + 1
    LRSchedule.per_epoch("cpu", [0.1] * 64, 1)
    assert LRSchedule.per_epoch("cpu", [0.5], 3).value(100) == 0.5
    with pytest.raises(ValueError, match="64"):
        LRSchedule.per_epoch("cpu", [0.1] * 65, 1)
    for bad in ([], ):
        with pytest.raises(ValueError):
            LRSchedule.per_epoch("cpu", bad, 1)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            LRSchedule.per_epoch("cpu", [0.1], bad)
    assert math.isfinite(s.value(0))
