"""The protocol by which a run's components describe their own snapshot regions and host mirrors to
`checkpoint.RunState` (``run_regions`` / ``run_host`` / ``run_check`` / ``run_restored``), for the parts that build on the
CPU.  No GPU: the blocks live in CPU tensors, nothing is launched, and `run_restored` is handed the bytes a kernel would
have left.  `DeviceBatches` and the model's fused dropout need the device: tests/test_gpu_run_state_format.py."""
import json

import numpy as np
import pytest
import torch

from dctn_amd.training import FlatAdam, FlatSGD, GradGuard, LRSchedule, ParamGroup, ParamGroups, StepTrace

SIZES = [7, 1, 30, 5]


def f32(x) -> float:
    return float(np.float32(x))


def _params():
    return [torch.nn.Parameter(torch.full((k,), 0.5)) for k in SIZES]


def _bytes(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().copy()


def _own_blocks(part):
    return {name: _bytes(t) for name, t in part.run_regions()}


def _scattered(block: torch.Tensor, words: np.ndarray) -> None:
    """What `RunState.load`'s scatter does to a block before the part hears of it: the file's words stand in it."""
    block.copy_(torch.from_numpy(words))


def _check_regions(part, names, tensors):
    regions = part.run_regions()
    assert [name for name, _ in regions] == names
    assert all(got is want for (_, got), want in zip(regions, tensors)) and len(regions) == len(tensors)


def _same(a, b) -> bool:
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


def _second_round_keeps_the_state(part):
    """Restoring a part from its own host scalars and its own regions' bytes changes nothing."""
    before = part.state_dict()
    part.run_restored(part.run_host(), _own_blocks(part))
    assert _same(part.state_dict(), before)


# ------------------------------------------------------------------ guard, trace
def test_guard_lists_its_block_and_follows_max_norm():
    g = GradGuard("cpu", 3.0)
    _check_regions(g, ["block"], [g._block])
    assert g.run_host() == {"max_norm": 3.0} and not hasattr(g, "run_check")
    g.run_restored({"max_norm": 7.5}, _own_blocks(g))
    assert g.max_norm == 7.5 and g.run_host() == {"max_norm": 7.5}
    assert GradGuard("cpu").run_host() == {"max_norm": float("inf")}
    _second_round_keeps_the_state(g)


def test_trace_lists_head_and_ring_and_counts_the_records_before_the_head_as_read():
    t = StepTrace("cpu", 8)
    _check_regions(t, ["head", "ring"], [t._head, t._ring])
    assert t.run_host() is None and not hasattr(t, "run_check")
    t.lost = 3
    head = np.array([5, 0, 0, 0], dtype="<u4").view(np.uint8)   # records_done = 5
    t.run_restored(None, {"head": head, "ring": np.zeros(8 * 64, dtype=np.uint8)})
    assert (t._last_read, t.lost) == (5, 0)
    big = np.array([0xFFFFFFF0, 0, 0, 0], dtype="<u4").view(np.uint8)   # the head is unsigned
    t.run_restored(None, {"head": big, "ring": np.zeros(8 * 64, dtype=np.uint8)})
    assert t._last_read == 0xFFFFFFF0
    _second_round_keeps_the_state(StepTrace("cpu", 8))


# ------------------------------------------------------------------ schedule, group table
def _schedule():
    s = LRSchedule("cpu", [(0, 0.0), (2, 1e-3), (5, 5e-4)], [0, 1, 0])
    s.scale = 0.7
    return s


def test_schedule_lists_its_block_and_decodes_its_mirror_from_the_bytes():
    a = _schedule()
    c = LRSchedule.constant("cpu", 1.0)
    _check_regions(c, ["schedule"], [c._block])
    assert c.run_host() is None and not hasattr(c, "run_check")
    c.run_restored(None, {"schedule": a.host_block().view(np.uint8)})   # a schedule with a changed scale
    assert c.knots == a.knots == [(0, 0.0), (2, f32(1e-3)), (5, f32(5e-4))]
    assert c.hold == [0, 1, 0] and c.scale == f32(0.7) and c.state_dict() == a.state_dict()
    assert c.value(3) == a.value(3)
    _second_round_keeps_the_state(a)


def _table(params, adam=True):
    return ParamGroups(params, [ParamGroup([params[0]], lr_scale=0.5, weight_decay=1e-3 if adam else None),
                                ParamGroup([params[3]], frozen=True)])


def test_group_table_lists_its_block_and_decodes_its_mirror_from_the_bytes():
    g = _table(_params())
    g._bind(1e-2, "FlatAdam")
    mirror = ParamGroups(_params())
    mirror._bind(1e-2, "FlatAdam")
    _check_regions(mirror, ["groups"], [mirror._block])
    assert mirror.run_host() is None and not hasattr(mirror, "run_check")
    left = g.host_block(steps=[7, 12, 7, 0]).view(np.uint8)   # a table with step counts, as a kernel leaves it
    mirror.run_restored(None, {"groups": left})
    assert mirror.lr_scales == [0.5, 1.0, 1.0, 1.0] and mirror.frozen == [False, False, False, True]
    assert mirror.weight_decays == [f32(1e-3), f32(1e-2), f32(1e-2), f32(1e-2)]
    assert mirror.state_dict()["weight_decay"] == [f32(1e-3), None, None, None]   # a None stays a None
    assert mirror.steps == [0, 0, 0, 0]   # the counts are the device block's, not a host mirror
    with pytest.raises(ValueError, match="segments"):
        ParamGroups(_params()[:2]).run_restored(None, {"groups": left})
    g._block[g._STEPS: g._STEPS + 4] = torch.tensor([7, 12, 7, 0], dtype=torch.int32)
    _second_round_keeps_the_state(g)


# ------------------------------------------------------------------ the optimizers
SGD_HOST = dict(kind="FlatSGD", lr=0.5, momentum=0.25, l2=0.125, steps=9)
ADAM_HOST = dict(kind="FlatAdam", lr=0.5, betas=[0.5, 0.75], eps=0.25, weight_decay=0.125, l2=0.0625)


def test_flat_sgd_lists_its_buffers_and_follows_its_host_scalars():
    p = _params()
    opt = FlatSGD(p[:3], p[3:], lr=1e-3, momentum=0.9, l2=1e-4)
    _check_regions(opt, ["flat", "buf", "sq_sum"], [opt.flat, opt.buf, opt.sq_sum])
    host = opt.run_host()
    assert host == dict(kind="FlatSGD", lr=1e-3, momentum=0.9, l2=1e-4, steps=0)
    assert list(host) == ["kind", "lr", "momentum", "l2", "steps"] and json.loads(json.dumps(host)) == host
    opt.run_check(host)
    with pytest.raises(ValueError) as e:
        opt.run_check(ADAM_HOST)
    assert str(e.value) == "snapshot: entry 'optimizer' is FlatAdam in the file, FlatSGD in the run"
    opt.run_restored(SGD_HOST, _own_blocks(opt))
    assert (opt.lr, opt.momentum, opt.l2, opt._steps, opt.t) == (0.5, 0.25, 0.125, 9, 9)
    assert opt.run_host() == SGD_HOST
    _second_round_keeps_the_state(opt)


def test_a_grouped_scheduled_flat_sgd_forwards_the_blocks_to_its_schedule_and_table():
    p = _params()
    schedule, groups = LRSchedule.constant("cpu", 1.0), ParamGroups(p)
    opt = FlatSGD(p[:3], p[3:], schedule=schedule, groups=groups)
    _check_regions(opt, ["flat", "buf", "schedule", "groups", "state", "sq_sum"],
                   [opt.flat, opt.buf, schedule._block, groups._block, opt._state, opt.sq_sum])
    grouped = FlatSGD(_p := _params(), groups=ParamGroups(_p))
    assert [n for n, _ in grouped.run_regions()] == ["flat", "buf", "groups", "state", "sq_sum"]
    _scattered(schedule._block, _schedule().host_block())
    _scattered(groups._block, _table(_params(), adam=False).host_block(steps=[3, 3, 3, 0]))
    opt.run_restored(SGD_HOST, _own_blocks(opt))
    assert schedule.state_dict() == _schedule().state_dict()
    assert groups.lr_scales == [0.5, 1.0, 1.0, 1.0] and groups.frozen == [False, False, False, True]
    assert groups.weight_decays == [0.0] * 4 and (opt.momentum, opt.l2, opt._steps) == (0.25, 0.125, 9)
    _second_round_keeps_the_state(opt)


def test_flat_adam_lists_its_buffers_follows_its_host_scalars_and_forwards_the_blocks():
    p = _params()
    schedule, groups = LRSchedule.constant("cpu", 1.0), ParamGroups(p)
    opt = FlatAdam(p[:3], p[3:], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, l2=1e-4, schedule=schedule,
                   groups=groups)
    _check_regions(opt, ["flat", "m", "v", "schedule", "groups", "state", "sq_sum"],
                   [opt.flat, opt.m, opt.v, schedule._block, groups._block, opt._state, opt.sq_sum])
    plain = FlatAdam(q := _params(), schedule=LRSchedule.constant("cpu", 1.0))
    _check_regions(plain, ["flat", "m", "v", "schedule", "state", "sq_sum"],
                   [plain.flat, plain.m, plain.v, plain.schedule._block, plain._state, plain.sq_sum])
    assert q[0].data_ptr() == plain.flat.data_ptr()
    host = opt.run_host()
    assert host == dict(kind="FlatAdam", lr=1e-3, betas=[0.9, 0.99], eps=1e-8, weight_decay=1e-2, l2=1e-4)
    assert list(host) == ["kind", "lr", "betas", "eps", "weight_decay", "l2"] and json.loads(json.dumps(host)) == host
    opt.run_check(host)
    with pytest.raises(ValueError) as e:
        opt.run_check(SGD_HOST)
    assert str(e.value) == "snapshot: entry 'optimizer' is FlatSGD in the file, FlatAdam in the run"
    table = _table(_params())
    table._bind(1e-2, "FlatAdam")
    _scattered(schedule._block, _schedule().host_block())
    _scattered(groups._block, table.host_block(steps=[3, 3, 3, 0]))
    opt.run_restored(ADAM_HOST, _own_blocks(opt))
    assert (opt._lr, opt.betas, opt.eps, opt.weight_decay, opt.l2) == (0.5, (0.5, 0.75), 0.25, 0.125, 0.0625)
    assert opt.run_host() == ADAM_HOST
    assert schedule.state_dict() == _schedule().state_dict() and opt.lr == schedule.value(0)
    assert groups.lr_scales == [0.5, 1.0, 1.0, 1.0] and groups.frozen == [False, False, False, True]
    assert groups.weight_decays == [f32(1e-3), f32(1e-2), f32(1e-2), f32(1e-2)]
    _second_round_keeps_the_state(opt)


# ------------------------------------------------------------------ RunState's walk over the parts
def test_run_parts_take_the_slots_in_file_order_and_refuse_another_optimizer():
    from dctn_amd import checkpoint as C

    model = torch.nn.Linear(3, 2)
    p = list(model.parameters())
    opt, guard, trace = FlatSGD(p[:1], p[1:]), GradGuard("cpu"), StepTrace("cpu", 8)
    assert C.run_parts(model, opt, None, guard, trace) == [("optimizer", opt), ("guard", guard), ("trace", trace)]
    assert C.run_parts(model, None, None, None) == []   # a plain module is a part for nothing
    regions, entries = C.run_regions(model, opt, None, guard, trace)
    assert [name for name, _ in regions] == ["optimizer.flat", "optimizer.buf", "optimizer.sq_sum", "guard.block",
                                             "trace.head", "trace.ring"]
    assert [(e["key"], e["region"], e["offset"]) for e in entries] == [("weight", "optimizer.flat", 0),
                                                                       ("bias", "optimizer.flat", 24)]
    regions, entries = C.run_regions(model, None, None, None)
    assert [name for name, _ in regions] == ["model.weight", "model.bias"]
    with pytest.raises(TypeError, match="RunState takes a FlatAdam or a FlatSGD, got SGD: a snapshot gathers FIXED"):
        C.run_parts(model, torch.optim.SGD(model.parameters(), lr=0.1), None, None)
