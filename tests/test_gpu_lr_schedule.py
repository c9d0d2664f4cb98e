"""The device-side learning-rate schedule on the GPU (`-m gpu`).  Every comparison here is exact.

The yardstick throughout is the UNSCHEDULED kernel driven by the host: an optimizer without a schedule whose ``lr`` the
test assigns to ``schedule.value(step)`` - the numpy mirror, which tests/test_host_lr_schedule.py holds to the library -
in front of each step.

  1. twelve scheduled steps = twelve host-driven steps, every buffer and the step block, bit for bit;
  2. the same with a gradient guard that clips about half the steps and halts on a NaN gradient at step 5;
  3. table ends and sizes: 64 knots, one knot, k[0] = 3, steps past the last knot;
  4. graphs: K = 5 and K = 1 launches of a scheduled `FlatAdam` = K = 1 replays with a host-set rate; a captured
     scheduled `FlatSGD` changes its rate from replay to replay, a captured unscheduled one cannot;
  5. `schedule.set` and `schedule.scale` between replays;
  6. a run resumed through `RunState`;
  7. the buffer contract under tests/guarded_buffers.py.

Tests 4 - 6 use the model, source and trace of tests/test_gpu_step_trace.py's K-equivalence test (cfg2 of
tests/recipe_reference.py: 37 samples in batches of 8, fused dropout)."""
import functools
import os

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from tests import recipe_reference as RR
from tests import test_gpu_step_trace as ST
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
LR, WD, L2 = 2e-3, 1e-3, 1e-2
N, N_REG = 4099, 2050   # two workgroups of Adam's flat_step_k (the ticket is real), a vector body and a scalar tail
STEPS = 12
# eight knots: a warm-up from 0, a hold, a drop, a linear decay
KNOTS = [(0, 0.0), (2, 1e-3), (3, 2e-3), (5, 2e-3), (6, 5e-4), (8, 4e-4), (10, 1e-4), (11, 5e-5)]
HOLD = [0, 0, 1, 0, 0, 0, 0, 0]
VARIANTS = {"float32": (F32, False), "bf16": (BF16, False), "bf16+master": (BF16, True)}


def _schedule(device=DEV, knots=KNOTS, hold=HOLD):
    from dctn_amd.training import LRSchedule

    return LRSchedule(device, knots, hold)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _synthetic(n, dtype, steps, seed=4321):
    """Initial weights and `steps` gradients (flat, CPU, float32 values representable in `dtype`).  Shared, never written."""
    g = torch.Generator().manual_seed(seed)
    w0 = (torch.randn(n, generator=g) * 0.05).to(dtype).float()
    grads = tuple((torch.randn(n, generator=g) * (0.5 + i % 3)).to(dtype).float() for i in range(steps))
    return w0, grads


def _optimizer(kind, w0, n_reg, dtype, master, **kw):
    from dctn_amd.training import FlatAdam, FlatSGD

    params = [torch.nn.Parameter(w0[:n_reg].clone().to(dtype).to(DEV)), torch.nn.Parameter(w0[n_reg:].clone().to(dtype).to(DEV))]
    if kind == "adam":
        opt = FlatAdam(params[:1], params[1:], lr=LR, weight_decay=WD, l2=L2, master_weights=master, **kw)
    else:
        opt = FlatSGD(params[:1], params[1:], lr=LR, momentum=0.9, l2=L2, master_weights=master, **kw)
    return opt, params


def _give(params, g_dev):
    """The gradients back to back in one buffer: the step reads them in place (at the buffer's alignment)."""
    k = params[0].numel()
    params[0].grad, params[1].grad = g_dev[:k], g_dev[k:]


def _owned(opt):
    torch.cuda.synchronize()
    bufs = {"flat": opt.flat, "sq_sum": opt.sq_sum}
    if hasattr(opt, "m"):
        bufs.update(m=opt.m, v=opt.v)
    else:
        bufs.update(buf=opt.buf)
    if opt.master is not None:
        bufs["master"] = opt.master
    return {k: v.clone() for k, v in bufs.items()}


def _assert_same_owned(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert _same_bits(got[k], want[k]), f"{what}: {k} differs"


def _block(opt):
    """The 16-byte step block as (steps_done, bits of lr, ticket, reserved)"""
    words = opt._state.cpu().numpy().view(np.uint32)
    return int(words[0]), int(words[1]), int(words[2]), int(words[3])


def _drive(kind, dtype, master, schedule, grads_dev, w0, n_reg, guards=(None, None), events=None):
    """Steps a scheduled optimizer and the host-driven yardstick side by side through `grads_dev` and compares after
    every step.  `events`: {step number: callable(scheduled optimizer, yardstick)} run in front of that step.  Returns
    the two optimizers.  `applied` counts the steps the guard let through: the index the next step evaluates."""
    sched_opt, sched_params = _optimizer(kind, w0, n_reg, dtype, master, schedule=schedule, guard=guards[0])
    plain, plain_params = _optimizer(kind, w0, n_reg, dtype, master, guard=guards[1])
    assert plain.schedule is None and sched_opt.schedule is schedule
    applied, last_rate = 0, 0.0
    for i, g_dev in enumerate(grads_dev):
        if events and i in events:
            events[i](sched_opt, plain)
        rate = schedule.value(applied)
        plain.lr = rate                      # what a user does today: a host write in front of the step
        _give(plain_params, g_dev)
        _give(sched_params, g_dev)
        plain.step()
        sched_opt.step()
        halted = guards[0] is not None and guards[0].halted
        if not halted:
            applied, last_rate = applied + 1, rate
        what = f"{kind} step {i} (applied {applied})"
        _assert_same_owned(_owned(sched_opt), _owned(plain), what)
        assert _block(sched_opt) == (applied, _bits(last_rate), 0, 0), f"{what}: block {_block(sched_opt)}"
        assert sched_opt.t == applied
        if kind == "adam":
            assert plain.t == applied
        if guards[0] is not None:
            a, b = (repr(g.read()) for g in guards)       # by their text: last_norm is NaN after the halt
            assert a == b, f"{what}: the two guards disagree: {a} != {b}"
    return sched_opt, plain


# ------------------------------------------------------------------ 1. step equivalence
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_twelve_scheduled_steps_are_twelve_host_driven_steps(kind, variant):
    dtype, master = VARIANTS[variant]
    w0, grads = _synthetic(N, dtype, STEPS)
    schedule = _schedule()
    sched_opt, plain = _drive(kind, dtype, master, schedule, [g.to(dtype).to(DEV) for g in grads], w0, N_REG)
    assert sched_opt.t == STEPS and sched_opt.lr == schedule.value(STEPS)
    assert (sched_opt.master is not None) == master
    assert not torch.equal(sched_opt.flat.float().cpu(), w0)
    assert len({schedule.value(s) for s in range(STEPS)}) >= 9    # the rate really moved
    with pytest.raises(RuntimeError):
        sched_opt.lr = 1.0
    if kind == "sgd":
        assert sched_opt.state_dict()["steps"] == STEPS


@pytest.mark.parametrize("variant", ["float32", "bf16+master"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_an_unaligned_gradient_view_takes_the_scalar_kernels(kind, variant):
    """n = 1023 at an element offset of 1: the gradients are not aligned for a vector access"""
    dtype, master = VARIANTS[variant]
    n = 1023
    w0, grads = _synthetic(n, dtype, STEPS)
    stores = [torch.zeros(n + 1, dtype=dtype, device=DEV) for _ in grads]
    views = []
    for store, g in zip(stores, grads):
        store[1:] = g.to(dtype).to(DEV)
        views.append(store[1:])
        assert views[-1].data_ptr() % 16 != 0 and views[-1].data_ptr() % (4 * store.element_size()) != 0
    sched_opt, _ = _drive(kind, dtype, master, _schedule(), views, w0, 511)
    assert sched_opt.t == STEPS


# ------------------------------------------------------------------ 2. with a guard
@pytest.mark.parametrize("variant", ["float32", "bf16+master"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_guard_clips_half_the_steps_and_a_nan_gradient_holds_the_schedule(kind, variant):
    from dctn_amd.training import GradGuard

    dtype, master = VARIANTS[variant]
    w0, grads = _synthetic(N, dtype, STEPS)
    norms = sorted(float(g.double().norm()) for g in grads)
    max_norm = 0.5 * (norms[5] + norms[6])       # the median: about half the steps clip
    grads_dev = [g.to(dtype).to(DEV) for g in grads]
    grads_dev[5] = grads_dev[5].clone()
    grads_dev[5][1234] = float("nan")
    guards = (GradGuard(DEV, max_norm), GradGuard(DEV, max_norm))
    schedule = _schedule()
    seen = {}

    def after_the_halt(sched_opt, plain):     # in front of step 8: steps 5, 6, 7 were skipped
        seen["block"] = _block(sched_opt)
        assert guards[0].halted and guards[1].halted
        guards[0].reset()
        guards[1].reset()

    sched_opt, plain = _drive(kind, dtype, master, schedule, grads_dev, w0, N_REG, guards, {8: after_the_halt})
    # steps 0 .. 4 were applied; the NaN at step 5 froze the count at 5 and the block's rate at the value of step 4
    assert seen["block"] == (5, _bits(schedule.value(4)), 0, 0)
    state = guards[0].read()
    assert state["seen"] == STEPS and state["halted"] == 0
    clipped_and_applied = sum(float(grads[i].double().norm()) > max_norm for i in (0, 1, 2, 3, 4, 8, 9, 10, 11))
    assert 2 <= clipped_and_applied <= 7 and state["clipped"] >= clipped_and_applied, (state, clipped_and_applied)
    assert sched_opt.t == STEPS - 3             # 5 before the halt, 4 after the reset: the table position moved with them


# ------------------------------------------------------------------ 3. table ends and size
TABLES = {
    "64 knots": ([(i + i // 4, 1e-3 * (1.0 + 0.5 * np.sin(i)) + 1e-6) for i in range(64)], [i % 5 == 0 for i in range(64)]),
    "one knot": ([(4, 7e-4)], None),
    "k[0] = 3": ([(3, 1e-4), (6, 1e-3), (9, 2e-4)], [0, 1, 0]),
}


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_the_block_reports_the_mirrors_rate_after_every_step(table, kind):
    knots, hold = TABLES[table]
    schedule = _schedule(knots=knots, hold=hold)
    steps = knots[-1][0] + 4                     # past the last knot
    n = 257
    w0, grads = _synthetic(n, F32, 3)
    opt, params = _optimizer(kind, w0, 100, F32, False, schedule=schedule)
    blocks = []
    for i in range(steps):
        _give(params, grads[i % 3].to(DEV))
        opt.step()
        blocks.append(opt._state.clone())
    got = torch.stack(blocks).cpu().numpy().view(np.uint32)
    want = np.array([(i + 1, _bits(schedule.value(i)), 0, 0) for i in range(steps)], dtype=np.uint32)
    assert np.array_equal(got, want), f"{table}: first difference at step {int(np.argmax((got != want).any(axis=1)))}"
    assert torch.isfinite(opt.flat).all()
    assert opt.lr == schedule.value(steps) == float(np.float32(knots[-1][1]))


# ------------------------------------------------------------------ 4. - 6. graphs
GRAPH_KNOTS = [(0, 2e-4), (3, 1e-3), (5, 1e-3), (6, 4e-4), (10, 1e-4)]     # a 10-step schedule: warm-up, hold, drop, decay
GRAPH_HOLD = [0, 1, 0, 0, 0]
OTHER_KNOTS = [(0, 5e-4), (8, 5e-5), (20, 1e-3)]


def _objects(mode, schedule=None, knots=None, **seeds):
    """The objects of tests/test_gpu_step_trace.py's runs, the optimizer with a schedule when one is given."""
    from dctn_amd.batches import DeviceBatches
    from dctn_amd.training import FlatAdam

    case = RR.CASES["cfg2"]
    dtype, master = ST.MODES[mode]
    model = ST._model(case, dtype, seeds.get("model_seed"))
    model.use_fused_dropout(seeds.get("dropout_seed", case.dropout_seed))
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=case.lr,
                   weight_decay=case.weight_decay, l2=case.reg_coeff, master_weights=master, schedule=schedule)
    images, labels = RR.make_data(case)
    src = DeviceBatches(images, labels, RR.GLOBAL_BATCH, dtype=dtype, seed=seeds.get("batch_seed", case.batch_seed),
                        scale=case.scale)
    return model, opt, src


def _apply(edit, schedule):
    if edit[0] == "set":
        schedule.set(edit[1], edit[2])
    else:
        schedule.scale = edit[1]


@functools.lru_cache(maxsize=None)
def _host_driven(mode, total, edits=()):
    """1 warm-up + `total` K = 1 replays of an UNSCHEDULED FlatAdam whose rate the host sets to the mirror's value in
    front of every iteration.  `edits`: ((step index, edit), ...) applied to the host mirror in front of that step.
    Shared; nobody writes into it."""
    from dctn_amd.training import StepTrace

    mirror = _schedule("cpu", GRAPH_KNOTS, GRAPH_HOLD)
    model, opt, src = _objects(mode)
    opt.lr = mirror.value(0)                    # the warm-up iteration is step 0
    trace = StepTrace(DEV, capacity=32)
    step = ST._step(RR.CASES["cfg2"], model, opt, src, trace, 1)
    states, rates = {}, [mirror.value(0)]
    for i in range(1, total + 1):
        for at, edit in edits:
            if at == i:
                _apply(edit, mirror)
        opt.lr = mirror.value(i)
        rates.append(mirror.value(i))
        step()
        states[i] = ST._state(model, opt, src)
    return states, trace.read(), rates, (model, opt, src, trace)


def _scheduled_run(mode, K, launches, edits=(), snapshot_after=None):
    from dctn_amd import checkpoint as C
    from dctn_amd.training import StepTrace

    schedule = _schedule(DEV, GRAPH_KNOTS, GRAPH_HOLD)
    model, opt, src = _objects(mode, schedule)
    trace = StepTrace(DEV, capacity=32)
    step = ST._step(RR.CASES["cfg2"], model, opt, src, trace, K)
    states, path = {}, None
    for launch in range(launches):
        for at, edit in edits:
            if at == 1 + launch * K:
                _apply(edit, schedule)
        step()
        states[(launch + 1) * K] = ST._state(model, opt, src)
        if snapshot_after == (launch + 1) * K:
            run = C.RunState(model, opt, batch_source=src, trace=trace)
            assert "optimizer.schedule" in run.names and run.names.index("optimizer.schedule") + 1 == run.names.index("optimizer.state")
            path = run.snapshot({"num_iters_done": snapshot_after}).save(
                os.path.join(ST._tmp_dir(), f"lr_schedule_{mode}_{K}_{snapshot_after}.dctn"))
            saved_schedule = schedule.state_dict()
    out = dict(states=states, records=trace.read(), schedule=schedule, opt=opt, path=path)
    if path is not None:
        out["saved_schedule"] = saved_schedule
    return out


@pytest.mark.parametrize("mode", ["f32", "bf16_master"])
@pytest.mark.parametrize("K", [5, 1])
def test_scheduled_launches_equal_host_driven_replays(K, mode):
    states, records, rates, _ = _host_driven(mode, 10)
    got = _scheduled_run(mode, K, 10 // K)
    for i in sorted(got["states"]):
        assert got["states"][i]["counters"] == (i + 1, i + 1, i + 1)
        ST._assert_same_state(got["states"][i], states[i], f"{mode} K={K}: after iteration {i + 1}")
    assert records["seq"].tolist() == list(range(11))
    ST._assert_same_records(got["records"], records, f"{mode} K={K}")
    want = np.array([_schedule("cpu", GRAPH_KNOTS, GRAPH_HOLD).value(i) for i in range(11)], dtype="<f4")
    assert got["records"]["lr"].tobytes() == want.tobytes() == np.array(rates, dtype="<f4").tobytes()
    assert got["records"]["opt_steps_done"].tolist() == list(range(1, 12))
    assert len(set(want.tolist())) >= 8
    assert got["opt"].lr == want[-1]            # past the last knot


def test_a_captured_scheduled_sgd_changes_its_rate_and_an_unscheduled_one_cannot():
    w0, grads = _synthetic(N, F32, 1)
    g_dev = grads[0].to(DEV)
    schedule = _schedule()

    def captured(**kw):
        opt, params = _optimizer("sgd", w0, N_REG, F32, False, **kw)
        _give(params, g_dev)
        opt.step()                               # step 0, eager: first_step
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
        return opt, graph

    eager, eager_params = _optimizer("sgd", w0, N_REG, F32, False)
    frozen, frozen_params = _optimizer("sgd", w0, N_REG, F32, False)
    for opt, params in ((eager, eager_params), (frozen, frozen_params)):
        _give(params, g_dev)
    sched_opt, sched_graph = captured(schedule=schedule)
    plain_opt, plain_graph = captured()
    eager.lr = schedule.value(0)
    eager.step()
    frozen.step()
    rates = []
    for i in range(1, 5):
        sched_graph.replay()
        eager.lr = schedule.value(i)
        eager.step()
        assert _same_bits(sched_opt.flat, eager.flat) and _same_bits(sched_opt.buf, eager.buf), f"replay {i}"
        rates.append(_block(sched_opt)[1])
        assert _block(sched_opt) == (i + 1, _bits(schedule.value(i)), 0, 0)
        plain_opt.lr = schedule.value(i)         # the host's write does not reach the captured launch argument
        plain_graph.replay()
        frozen.step()                            # LR throughout
        assert _same_bits(plain_opt.flat, frozen.flat), f"replay {i}: the unscheduled graph followed the assignment"
    assert len(set(rates)) == 3                  # steps 1, 2 warm up, steps 3 and 4 hold
    assert not _same_bits(plain_opt.flat, sched_opt.flat)


# ------------------------------------------------------------------ 5. between replays
EDITS = ((6, ("set", tuple(OTHER_KNOTS), None)), (11, ("scale", 0.5)))


def test_set_and_scale_take_effect_on_the_next_replay(monkeypatch):
    """Launch 1 (steps 1 - 5) on the first table, `schedule.set` in front of launch 2, `scale = 0.5` in front of launch 3:
    no new capture, and the bits of the host-driven run that follows the same mirror"""
    states, records, rates, _ = _host_driven("bf16_master", 15, EDITS)
    got = _scheduled_run("bf16_master", 5, 3, EDITS)
    for i in (5, 10, 15):
        ST._assert_same_state(got["states"][i], states[i], f"after iteration {i + 1}")
    ST._assert_same_records(got["records"], records, "set / scale between replays")
    other = _schedule("cpu", OTHER_KNOTS, None)
    assert rates[5] == _schedule("cpu", GRAPH_KNOTS, GRAPH_HOLD).value(5) and rates[6] == other.value(6)
    assert rates[10] == other.value(10) and rates[11] == float(np.float32(other.value(11)) * np.float32(0.5))
    assert got["records"]["lr"].tobytes() == np.array(rates, dtype="<f4").tobytes()
    # neither while a capture is under way (the write would become a node of somebody's graph)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        got["schedule"].scale = 0.25
    with pytest.raises(RuntimeError, match="capture"):
        got["schedule"].set(GRAPH_KNOTS, GRAPH_HOLD)
    assert got["schedule"].scale == 0.5 and got["schedule"].knots == _schedule("cpu", OTHER_KNOTS, None).knots


# ------------------------------------------------------------------ 6. resume
def test_a_resumed_run_continues_its_schedule_bit_for_bit():
    from dctn_amd import checkpoint as C
    from dctn_amd.training import StepTrace

    mode = "bf16_master"
    states, records, rates, plain_objects = _host_driven(mode, 10)
    saved = _scheduled_run(mode, 1, 10, snapshot_after=3)      # warm-up + 3 replays: 4 steps done, the next is step 4
    ST._assert_same_state(saved["states"][10], states[10], "the uninterrupted scheduled run")
    # fresh objects that share nothing with the saved run but the data; their schedule was built with other knots
    schedule = _schedule(DEV, OTHER_KNOTS, None)
    schedule.scale = 0.3
    model, opt, src = _objects(mode, schedule, model_seed=RR.CASES["cfg2"].model_seed + 1, dropout_seed=99, batch_seed=77)
    trace = StepTrace(DEV, capacity=32)
    step = ST._step(RR.CASES["cfg2"], model, opt, src, trace, 1)
    step()
    run = C.RunState(model, opt, batch_source=src, trace=trace)
    assert run.load(saved["path"]) == {"num_iters_done": 3}
    ST._assert_same_state(ST._state(model, opt, src), states[3], "after the load")
    assert schedule.state_dict() == saved["saved_schedule"] and schedule.scale == 1.0
    assert schedule.knots == _schedule("cpu", GRAPH_KNOTS, GRAPH_HOLD).knots
    assert opt.lr == rates[4]
    for i in range(4, 11):
        step()
    ST._assert_same_state(ST._state(model, opt, src), states[10], "the resumed run after iteration 11")
    got = trace.read()
    assert got["seq"].tolist() == list(range(4, 11))
    ST._assert_same_records(got, records[4:], "records 4 - 10 of the resumed run")
    # a file from a run without a schedule is refused at that entry, before anything is written
    plain_model, plain_opt, plain_src, plain_trace = plain_objects
    plain_run = C.RunState(plain_model, plain_opt, batch_source=plain_src, trace=plain_trace)
    assert "optimizer.schedule" not in plain_run.names
    assert plain_run.names[:6] == ["optimizer.flat", "optimizer.m", "optimizer.v", "optimizer.master", "optimizer.state",
                                   "optimizer.sq_sum"]                                        # what it always was
    plain_path = plain_run.snapshot({}).save(os.path.join(ST._tmp_dir(), "lr_schedule_unscheduled.dctn"))
    before = ST._state(model, opt, src)
    with pytest.raises(ValueError, match="optimizer.schedule"):
        run.load(plain_path)
    with pytest.raises(ValueError, match="optimizer.schedule"):
        plain_run.load(saved["path"])
    ST._assert_same_state(ST._state(model, opt, src), before, "a refused load wrote something")


def test_a_scheduled_sgd_run_state_carries_schedule_and_step_block():
    from dctn_amd import checkpoint as C

    w0, grads = _synthetic(N, F32, 3)
    model = torch.nn.Linear(1, 1).to(DEV)        # RunState wants a module; its two values ride as regions of their own

    def fresh(knots, hold):
        opt, params = _optimizer("sgd", w0, N_REG, F32, False, schedule=_schedule(DEV, knots, hold))
        return opt, params, C.RunState(model, opt)

    opt, params, run = fresh(KNOTS, HOLD)
    assert run.names[:5] == ["optimizer.flat", "optimizer.buf", "optimizer.schedule", "optimizer.state", "optimizer.sq_sum"]
    for g in grads[:2]:
        _give(params, g.to(DEV))
        opt.step()
    path = run.snapshot({}).save(os.path.join(ST._tmp_dir(), "lr_schedule_sgd.dctn"))
    _give(params, grads[2].to(DEV))
    opt.step()
    other, other_params, other_run = fresh(OTHER_KNOTS, None)
    other_run.load(path)
    assert other.t == 2 and other.schedule.state_dict() == opt.schedule.state_dict()
    _give(other_params, grads[2].to(DEV))
    other.step()
    _assert_same_owned(_owned(other), _owned(opt), "resumed scheduled SGD")
    assert _block(other) == _block(opt) == (3, _bits(opt.schedule.value(2)), 0, 0)
    unscheduled, _ = _optimizer("sgd", w0, N_REG, F32, False)
    with pytest.raises(ValueError, match="optimizer.schedule"):
        C.RunState(model, unscheduled).load(path)


# ------------------------------------------------------------------ 7. the buffer contract
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_nothing_outside_the_buffers_is_touched_and_unused_slots_do_not_matter(kind):
    """Every buffer of the optimizer and the schedule block of exactly dctn_lr_schedule_bytes() inside a guarded arena
    filled with 0xFF; one knot, the 63 unused slots hold INT32_MAX / NaN / all ones"""
    from dctn_amd.training import LRSchedule

    assert L.lib().dctn_lr_schedule_bytes() == 784
    dtype, master = VARIANTS["bf16+master"]
    w0, grads = _synthetic(N, dtype, 3)
    with guarded(fill=0xFF) as arena:
        schedule = LRSchedule(DEV, [(0, 1e-3)])
        assert schedule._block.numel() * 4 == 784
        assert any(r.nbytes == 784 for r in arena.records)          # the block is an arena allocation of exactly that size
        schedule._block[5:68] = 0x7FFFFFFF                          # k
        schedule._block[69:132] = 0x7FC00000                        # lr: NaN
        schedule._block[133:196] = -1                               # hold
        opt, params = _optimizer(kind, w0, N_REG, dtype, master, schedule=schedule)
        placed = [arena.place(g.to(dtype).to(DEV)) for g in grads]
        for g_dev in placed:
            _give(params, g_dev)
            opt.step()
    arena.check()   # synchronises; every guard byte around every buffer is intact
    plain, plain_params = _optimizer(kind, w0, N_REG, dtype, master)
    plain.lr = float(np.float32(1e-3))
    for g in grads:
        _give(plain_params, g.to(dtype).to(DEV))
        plain.step()
    _assert_same_owned(_owned(opt), _owned(plain), f"{kind} in the arena")
    assert _block(opt) == (3, _bits(1e-3), 0, 0)
    for name, buf in _owned(opt).items():
        assert torch.isfinite(buf.float()).all(), name
    for g_dev, g in zip(placed, grads):
        assert _same_bits(g_dev.cpu(), g.to(dtype)), "a gradient buffer changed"
    words = schedule._block.cpu().numpy()
    assert words[0] == 1 and (words[5:68] == 0x7FFFFFFF).all() and (words[133:] == -1).all()   # only read


def test_the_step_trace_records_a_scheduled_sgds_block():
    """`StepTrace.record` passes the step block of a scheduled FlatSGD as it passes FlatAdam's; an unscheduled one has none"""
    from dctn_amd.training import StepTrace

    w0, grads = _synthetic(N, F32, 3)
    schedule = _schedule()
    logits = torch.randn(8, 10, device=DEV)
    labels = torch.arange(8, device=DEV) % 10
    loss = torch.tensor(0.5, device=DEV)
    trace = StepTrace(DEV, capacity=8)
    opt, params = _optimizer("sgd", w0, N_REG, F32, False, schedule=schedule)
    for g in grads:
        _give(params, g.to(DEV))
        opt.step()
        trace.record(logits, labels, loss, optimizer=opt)
    plain, plain_params = _optimizer("sgd", w0, N_REG, F32, False)
    _give(plain_params, grads[0].to(DEV))
    plain.step()
    trace.record(logits, labels, loss, optimizer=plain)
    records = trace.read()
    assert records["present"].tolist() == [L.TRACE_HAS_ADAM] * 3 + [0]
    assert records["opt_steps_done"].tolist() == [1, 2, 3, 0]
    assert records["lr"].tobytes() == np.array([schedule.value(0), schedule.value(1), schedule.value(2), 0.0], dtype="<f4").tobytes()
