"""The parameter-group table on the GPU (`-m gpu`): `FlatAdam(..., groups=g)` / `FlatSGD(..., groups=g)`.

  1. twelve grouped steps against CPU `torch.optim` in float64 with ``param_groups`` and a parameter without a gradient,
     judged per segment of at least 1000 elements by tests/test_gpu_flat_adam.py's criterion;
  2. bit for bit against separate UNGROUPED optimizers, one per segment; all-default groups against the ungrouped
     optimizer, every owned buffer and both blocks;
  3. staged freezing, eagerly and through one captured `GraphedTrainStep` edited between replays;
  4. frozen means untouched, nothing outside any buffer is written, unused table slots do not matter;
  5. the guard: one coefficient for every unfrozen segment, a halted step advances no count;
  6. end to end: a two-layer model with a frozen core and a slower head in a `GraphedTrainStep`, against a plain-torch
     float64 loop of the reference's recipe, and a `RunState` resume.

Synthetic sizes: n = 12295 in segments [4099, 1, 3000, 5, 4096, 1094] with n_reg = 7102 inside a segment (ends at vector
offsets 3, 0, 0, 1, 1 and the tail of n; a one-element segment; four Adam workgroups), and n = 2 * 1048576 + 4096 + 3 in
64 uneven segments (every lane's cursor crosses segments over several grid strides), both with aligned and odd-offset
gradient views."""
import functools
import os

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LR, WD, L2, MOMENTUM, STEPS = 5e-4, 1e-3, 1e-2, 0.9, 12
VARIANTS = {"float32": (F32, False), "bf16": (BF16, False), "bf16+master": (BF16, True)}
SCALES6 = [1, .5, .1, 2, 1, .25]
WDS6 = [1e-3, 0, 1e-2, 1e-3, 0, 1e-3]
NAN_BITS = 0x7FC12345   # a NaN with a payload


def _full_sizes():
    n = 2 * 1048576 + 4096 + 3
    rng = np.random.default_rng(7)
    weight = rng.random(64) ** 3 + 1e-4
    sizes = np.floor(weight / weight.sum() * (n - 64)).astype(np.int64) + 1
    sizes[5], sizes[17], sizes[40] = 1, 2, 3
    sizes[int(np.argmax(sizes))] += n - int(sizes.sum())
    assert int(sizes.sum()) == n and sizes.min() >= 1 and len(set(sizes.tolist())) > 50
    return [int(s) for s in sizes]


class Case:
    def __init__(self, sizes, n_reg):
        self.sizes, self.n, self.n_reg = sizes, sum(sizes), n_reg
        self.ends = np.cumsum(sizes).tolist()
        self.starts = [0] + self.ends[:-1]
        k = len(sizes)
        self.scales = [SCALES6[i % 6] for i in range(k)]
        self.wds = [WDS6[i % 6] for i in range(k)]
        self.frozen = [i % 6 == 4 for i in range(k)]
        assert n_reg not in self.ends and 0 < n_reg < self.n          # the regularised prefix ends inside a segment
        self.judged = [i for i in range(k) if sizes[i] >= 1000 and not self.frozen[i]]


CASES = {"small": Case([4099, 1, 3000, 5, 4096, 1094], 7102), "full": Case(_full_sizes(), 1048576 + 2049)}
assert [e % 4 for e in CASES["small"].ends] == [3, 0, 0, 1, 1, 3] and CASES["small"].n == 12295
assert len(CASES["small"].judged) == 3 and len(CASES["full"].judged) >= 20


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _synthetic(case_name, dtype):
    """Initial weights and STEPS gradients (flat, CPU, float32 values representable in `dtype`).  Shared, never written.
    Three random vectors, rescaled per step."""
    n = CASES[case_name].n
    g = torch.Generator().manual_seed(2468)
    w0 = (torch.randn(n, generator=g) * 0.02).to(dtype).float()
    base = [torch.randn(n, generator=g) for _ in range(3)]
    grads = tuple((base[i % 3] * (0.25 + 0.5 * (i % 4))).to(dtype).float() for i in range(STEPS))
    return w0, grads


def _seg_rate(rate, scale):
    """The kernel's rate of a segment: ONE rounded float32 product"""
    return float(np.float32(rate) * np.float32(scale))


# ------------------------------------------------------------------ building optimizers
def _grouped(kind, case, variant, w0, scales=None, wds=None, frozen=None, groups=True, **kw):
    """One optimizer over the whole flat vector, one parameter per segment, the regularised prefix ending inside a
    segment (the optimizers take n_reg from their parameter lists; the kernel takes any prefix)."""
    from dctn_amd.training import FlatAdam, FlatSGD, ParamGroup, ParamGroups

    dtype, master = VARIANTS[variant]
    params = [torch.nn.Parameter(c.clone().to(dtype).to(DEV)) for c in w0.split(case.sizes)]
    table = None
    if groups:
        k = len(params)
        scales = case.scales if scales is None else scales
        wds = case.wds if wds is None else wds
        frozen = case.frozen if frozen is None else frozen
        table = ParamGroups(params, [ParamGroup([params[i]], lr_scale=scales[i], weight_decay=wds[i] if kind == "adam" else None,
                                                frozen=frozen[i]) for i in range(k)])
        kw["groups"] = table
    if kind == "adam":
        opt = FlatAdam(params, [], lr=LR, weight_decay=WD, l2=L2, master_weights=master, **kw)
    else:
        opt = FlatSGD(params, [], lr=LR, momentum=MOMENTUM, l2=L2, master_weights=master, **kw)
    opt.n_reg = case.n_reg
    return opt, params, table


def _give(params, grads_flat, case, offset, place=None):
    """The gradients back to back in one buffer at an element offset of 0 (aligned) or 1: read in place.  `place`: moves
    the buffer (into a guarded arena)."""
    store = torch.empty(case.n + offset, dtype=grads_flat.dtype, device=DEV)
    store[offset:] = grads_flat
    if place is not None:
        store = place(store)
    for p, a, b in zip(params, case.starts, case.ends):
        p.grad = store[offset + a: offset + b]
    if offset:
        assert params[0].grad.data_ptr() % (4 * store.element_size()) != 0
    return store


def _owned(opt):
    torch.cuda.synchronize()
    bufs = {"flat": opt.flat}
    if hasattr(opt, "m"):
        bufs.update(m=opt.m, v=opt.v)
    else:
        bufs.update(buf=opt.buf)
    if opt.master is not None:
        bufs["master"] = opt.master
    return {k: v.clone() for k, v in bufs.items()}


class _PerSegment:
    """What a user has today: one UNGROUPED optimizer per segment with lr = float32(rate * scale) and the segment's weight
    decay, stepped only on the segment's unfrozen steps."""

    def __init__(self, kind, case, variant, w0, scales, wds):
        from dctn_amd.training import FlatAdam, FlatSGD

        dtype, master = VARIANTS[variant]
        self.kind, self.case, self.scales = kind, case, scales
        self.opts, self.params = [], []
        for i, c in enumerate(w0.split(case.sizes)):
            p = torch.nn.Parameter(c.clone().to(dtype).to(DEV))
            if kind == "adam":
                opt = FlatAdam([p], [], lr=_seg_rate(LR, scales[i]), weight_decay=wds[i], l2=L2, master_weights=master)
            else:
                opt = FlatSGD([p], [], lr=_seg_rate(LR, scales[i]), momentum=MOMENTUM, l2=L2, master_weights=master)
            opt.n_reg = min(max(case.n_reg - case.starts[i], 0), case.sizes[i])
            self.opts.append(opt)
            self.params.append(p)

    def step(self, grads_flat, frozen, rate=None):
        for i, (opt, p) in enumerate(zip(self.opts, self.params)):
            if frozen[i]:
                continue
            if rate is not None:
                opt.lr = _seg_rate(rate, self.scales[i])
            p.grad = grads_flat[self.case.starts[i]: self.case.ends[i]].clone()
            opt.step()

    def owned(self):
        torch.cuda.synchronize()
        names = ["flat"] + (["m", "v"] if self.kind == "adam" else ["buf"]) + (["master"] if self.opts[0].master is not None else [])
        return {name: torch.cat([getattr(o, name) for o in self.opts]) for name in names}

    @property
    def steps(self):
        return [o.t for o in self.opts]


def _assert_same_owned(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        if not _same_bits(got[k], want[k]):
            bad = torch.nonzero(got[k].view(torch.int16 if got[k].dtype == BF16 else torch.int32)
                                != want[k].view(torch.int16 if want[k].dtype == BF16 else torch.int32)).flatten()
            raise AssertionError(f"{what}: {k} differs at {bad.numel()} elements, the first {bad[:8].tolist()}")


# ------------------------------------------------------------------ 1. against torch
def _torch_run(kind, case_name, data_dtype, dtype, frozen_at):
    """torch.optim on the CPU in `dtype`, on the data drawn for `data_dtype`, with one param group per segment; `frozen_at(step)`: the segments whose gradient
    is None at that step.  The 2 * l2 * w term of the regularised prefix is added by hand, as
    tests/test_gpu_flat_adam.py::_run_torch_adam does.  Returns the final flat weights (float64), l2 * sum w^2 over the
    WHOLE prefix (frozen elements included) before the last update, and torch's per-parameter step counts."""
    case = CASES[case_name]
    w0, grads = _synthetic(case_name, data_dtype)
    params = [torch.nn.Parameter(c.clone().to(dtype)) for c in w0.split(case.sizes)]
    if kind == "adam":
        opt = torch.optim.Adam([dict(params=[p], lr=LR * s, weight_decay=wd) for p, s, wd in zip(params, case.scales, case.wds)],
                               lr=LR)
    else:
        opt = torch.optim.SGD([dict(params=[p], lr=LR * s) for p, s in zip(params, case.scales)], lr=LR, momentum=MOMENTUM)
    work = F64 if dtype == F64 else F32
    reg = None
    for step, g in enumerate(grads):
        flat_w = torch.cat([p.detach().reshape(-1) for p in params])
        reg = L2 * float((flat_w[:case.n_reg].double() ** 2).sum())
        full = g.to(work).clone()
        full[:case.n_reg] += 2 * L2 * flat_w[:case.n_reg].to(work)
        frozen = frozen_at(step)
        for i, (p, gp) in enumerate(zip(params, full.to(dtype).split(case.sizes))):
            p.grad = None if frozen[i] else gp.clone()
        opt.step()
    counts = [int(opt.state[p]["step"]) if "step" in opt.state.get(p, {}) else None for p in params]
    return torch.cat([p.detach().reshape(-1) for p in params]).double(), reg, counts


@functools.lru_cache(maxsize=None)
def _torch_reference(kind, case_name, data_dtype, run_dtype, staging):
    return _torch_run(kind, case_name, data_dtype, run_dtype, STAGINGS[staging](CASES[case_name]))


def _constant(case):
    return lambda step: case.frozen


def _staged(case):
    """Steps 0 - 4 freeze segments 0 and 2; nothing else is frozen"""
    return lambda step: [step < 5 and i in (0, 2) for i in range(len(case.sizes))]


STAGINGS = {"constant": _constant, "staged": _staged}


def _judge(case, segments, w_flat, w0, data_dtype, kind, case_name, staging, what):
    """e = |w - w_ref| / |w_ref - w_0| per segment: e_flat <= 2 * e_torch32 (float32), <= 1.5 * e_torch_bf16 (bf16);
    e_torch > 0, so the bound is never vacuous"""
    w_ref, _, _ = _torch_reference(kind, case_name, data_dtype, F64, staging)
    w_torch, _, _ = _torch_reference(kind, case_name, data_dtype, data_dtype, staging)
    factor = 2.0 if data_dtype == F32 else 1.5
    failures = []
    for i in segments:
        a, b = case.starts[i], case.ends[i]
        moved = float((w_ref[a:b] - w0[a:b].double()).norm())
        assert moved > 0.0, f"{what}: segment {i} did not move in the reference"
        e_torch = float((w_torch[a:b] - w_ref[a:b]).norm()) / moved
        e_flat = float((w_flat[a:b] - w_ref[a:b]).norm()) / moved
        print(f"{what}: segment {i} ({b - a} elements): e_flat={e_flat:.4e} e_torch={e_torch:.4e} bound={factor * e_torch:.4e}")
        assert e_torch > 0.0, f"{what}: segment {i}: torch's own error is 0, the bound would be vacuous"
        if not e_flat <= factor * e_torch:
            failures.append((i, e_flat, e_torch))
    assert not failures, f"{what}: (segment, e_flat, e_torch) beyond {factor} * e_torch: {failures}"


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_offset"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bf16"])
@pytest.mark.parametrize("case_name", ["small", "full"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_twelve_grouped_steps_match_torch_param_groups(kind, case_name, dtype, offset):
    """Segment 4 (of every six) is frozen and its gradient is None (the step gathers, as it does for a model with a frozen
    core; the other gradients are views at `offset`)."""
    case = CASES[case_name]
    w0, grads = _synthetic(case_name, dtype)
    opt, params, table = _grouped(kind, case, "float32" if dtype == F32 else "bf16", w0)
    own_reg = None
    for g in grads:
        _give(params, g.to(dtype).to(DEV), case, offset)
        for i, p in enumerate(params):
            if case.frozen[i]:
                p.grad = None
        own_reg = L2 * float((opt.flat[:case.n_reg].double() ** 2).sum())
        opt.step()
    assert opt.t == STEPS
    assert table.steps == [0 if f else STEPS for f in case.frozen]
    w_flat = opt.flat.double().cpu()
    for i in range(len(case.sizes)):
        if case.frozen[i]:
            a, b = case.starts[i], case.ends[i]
            assert _same_bits(opt.flat[a:b].cpu(), w0[a:b].to(dtype)), f"frozen segment {i} moved"
    what = f"{kind} {case_name} {dtype} offset {offset}"
    _judge(case, case.judged, w_flat, w0, dtype, kind, case_name, "constant", what)
    # the regulariser's value as of the last step, the frozen regularised elements included
    _, reg_ref, counts = _torch_reference(kind, case_name, dtype, F64, "constant")
    reg = float(opt.reg_value())
    print(f"{what}: reg_value={reg:.8e} own weights={own_reg:.8e} float64 reference={reg_ref:.8e}")
    assert abs(reg - own_reg) <= 1e-4 * max(1.0, own_reg)
    if dtype == F32:
        assert abs(reg - reg_ref) <= 1e-4 * max(1.0, reg_ref)
    frozen_sq = sum(float((w0[case.starts[i]: min(case.ends[i], case.n_reg)].double() ** 2).sum())
                    for i in range(len(case.sizes)) if case.frozen[i] and case.starts[i] < case.n_reg)
    if case_name == "full":   # (the small case's frozen segment lies behind n_reg: the test of the value's frozen share
        assert L2 * frozen_sq > 1e-3 * reg                           # is below) a visible share of the value
    if kind == "adam":                                               # torch kept no state for the parameter without gradient
        assert [c is None for c in counts] == case.frozen


# ------------------------------------------------------------------ 2. bit for bit against ungrouped optimizers
def _drive_against_per_segment(kind, case_name, variant, offset, staging, schedule=None, after_step=None):
    case = CASES[case_name]
    dtype, _ = VARIANTS[variant]
    w0, grads = _synthetic(case_name, dtype)
    frozen_at = STAGINGS[staging](case)
    opt, params, table = _grouped(kind, case, variant, w0, frozen=frozen_at(0), schedule=schedule)
    yard = _PerSegment(kind, case, variant, w0, case.scales, case.wds)
    applied = 0
    for step, g in enumerate(grads):
        frozen = frozen_at(step)
        for i in range(len(case.sizes)):
            if frozen[i] != table.frozen[i]:
                table.freeze(params[i], frozen[i])
        g_dev = g.to(dtype).to(DEV)
        poisoned = g_dev.clone()
        for i in range(len(case.sizes)):                             # a frozen segment's gradient is not read
            if frozen[i]:
                poisoned[case.starts[i]: case.ends[i]] = float("nan")
        _give(params, poisoned, case, offset)
        rate = None if schedule is None else schedule.value(applied)
        opt.step()
        yard.step(g_dev, frozen, rate)
        applied += 1
        if step in (0, 4, 5, STEPS - 1):
            _assert_same_owned(_owned(opt), yard.owned(), f"{kind} {case_name} {variant} offset {offset} step {step}")
            assert table.steps == yard.steps and opt.t == applied
        if after_step is not None:
            after_step(step, opt)
    return opt, table, yard


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_offset"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case_name", ["small", "full"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_grouped_run_equals_one_ungrouped_optimizer_per_segment(kind, case_name, variant, offset):
    opt, table, yard = _drive_against_per_segment(kind, case_name, variant, offset, "constant")
    case = CASES[case_name]
    assert table.steps == [0 if f else STEPS for f in case.frozen]
    assert (opt.master is not None) == VARIANTS[variant][1]


@pytest.mark.parametrize("variant", ["float32", "bf16+master"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_with_a_schedule_the_segments_scale_the_global_steps_rate(kind, variant):
    from dctn_amd.training import LRSchedule

    schedule = LRSchedule(DEV, [(0, 0.0), (2, 1e-3), (3, 2e-3), (5, 2e-3), (6, 5e-4), (11, 5e-5)], [0, 0, 1, 0, 0, 0])
    seen = []

    def block(step, opt):   # the block reports the GLOBAL rate of the step just taken, before any segment's scale
        words = opt._state.cpu().numpy().view(np.uint32)
        seen.append((int(words[0]), int(words[1]), int(words[2])))

    _drive_against_per_segment(kind, "small", variant, 0, "staged", schedule, block)
    want = [(s + 1, int(np.float32(schedule.value(s)).view(np.uint32)), 0) for s in range(STEPS)]
    assert seen == want


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_offset"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case_name", ["small", "full"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_all_default_groups_leave_the_ungrouped_bits(kind, case_name, variant, offset):
    """Scale 1, the optimizer's weight decay, nothing frozen, counts equal to steps_done: every owned buffer, the sq_sum
    slots and the step block are the ungrouped optimizer's"""
    case = CASES[case_name]
    dtype, _ = VARIANTS[variant]
    w0, grads = _synthetic(case_name, dtype)
    k = len(case.sizes)
    opt, params, table = _grouped(kind, case, variant, w0, scales=[1.0] * k, wds=[WD] * k, frozen=[False] * k)
    plain, plain_params, _ = _grouped(kind, case, variant, w0, groups=False)
    for step, g in enumerate(grads[:4]):
        g_dev = g.to(dtype).to(DEV)
        _give(params, g_dev, case, offset)
        _give(plain_params, g_dev, case, offset)
        opt.step()
        plain.step()
        got, want = _owned(opt), _owned(plain)
        got["sq_sum"], want["sq_sum"] = opt.sq_sum.clone(), plain.sq_sum.clone()
        if kind == "adam":                      # (an ungrouped FlatSGD has no step block)
            got["state"], want["state"] = opt._state.clone(), plain._state.clone()
        _assert_same_owned(got, want, f"{kind} {case_name} {variant} offset {offset} step {step}")
    assert table.steps == [4] * k and opt.t == 4
    if kind == "sgd":
        words = opt._state.cpu().numpy()
        assert words[0] == 4 and words.view(np.float32)[1] == np.float32(LR) and words[2] == 0


# ------------------------------------------------------------------ 3. staged freezing
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bf16"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_staged_freezing_counts_per_segment_and_matches_torch(kind, dtype):
    """Steps 0 - 4 freeze segments 0 and 2; `groups.freeze(..., False)` in front of step 5"""
    variant = "float32" if dtype == F32 else "bf16"
    opt, table, yard = _drive_against_per_segment(kind, "small", variant, 0, "staged")
    assert table.steps == [7, 12, 7, 12, 12, 12] and opt.t == STEPS
    case = CASES["small"]
    w0, _ = _synthetic("small", dtype)
    _, _, counts = _torch_reference(kind, "small", dtype, F64, "staged")
    if kind == "adam":
        assert counts == table.steps
    _judge(case, [0, 2, 4, 5], opt.flat.double().cpu(), w0, dtype, kind, "small", "staged", f"staged {kind} {dtype}")


def _tiny_model(seed=3, dtype=F32, freeze_first=False):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    model = EPSesPlusLinear(((2, 3), (2, 4)), UnitTheoreticalOutputStd(), 1.0, DEV, dtype, image_size=8)
    if freeze_first:
        model.epses[0].requires_grad_(False)
    return model


@functools.lru_cache(maxsize=None)
def _batches(count, B=16, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        u = torch.rand(1, B, 8, 8, generator=g)
        x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1)
        out.append((x, torch.randint(0, 10, (B,), generator=g)))
    return tuple(out)


def _model_optimizer(model, groups):
    from dctn_amd.training import FlatAdam

    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3, l2=1e-2,
                    groups=groups)


def _model_state(opt):
    torch.cuda.synchronize()
    return dict(flat=opt.flat.clone(), m=opt.m.clone(), v=opt.v.clone(), state=opt._state.clone(),
                groups=opt.groups._block.clone(), sq_sum=opt.sq_sum.clone())


def _assert_same_model_state(got, want, what):
    for k in want:
        assert _same_bits(got[k], want[k]), f"{what}: {k} differs"


def test_staging_through_one_captured_graph_equals_the_eager_run():
    """The table freezes core 0 for the warm-up and four replays and releases it by `groups.freeze` between replays: no
    new capture, and the eager run's bits"""
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy, param_groups_for, train_step

    batches = [(x.to(DEV), y.to(DEV)) for x, y in _batches(13)]

    def run(graphed):
        model = _tiny_model()
        groups = param_groups_for(model, freeze_eps=(0,), head_lr_scale=0.5)
        opt = _model_optimizer(model, groups)
        core0 = model.epses[0].detach().clone()
        if graphed:
            step = GraphedTrainStep(model, *batches[0], fused_cross_entropy, opt, warmup=1)
        else:
            train_step(model, *batches[0], fused_cross_entropy, opt)
        states = []
        for i, (x, y) in enumerate(batches[1:], start=1):
            if i == 5:
                torch.cuda.synchronize()
                assert _same_bits(model.epses[0].detach(), core0), "the frozen core moved"
                groups.freeze(model.epses[0], False)
            if graphed:
                step(x, y)
            else:
                train_step(model, x, y, fused_cross_entropy, opt)
            states.append(_model_state(opt))
        assert groups.steps == [8, 13, 13, 13] and opt.t == 13
        assert not _same_bits(model.epses[0].detach(), core0)
        return states

    eager, graphed = run(False), run(True)
    for i, (a, b) in enumerate(zip(graphed, eager)):
        _assert_same_model_state(a, b, f"replay {i + 1}")


# ------------------------------------------------------------------ 4. frozen means untouched
@pytest.mark.parametrize("fill", [0xFF, 0x7B], ids=["nan_fill", "0x7b_fill"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_frozen_segments_keep_their_bits_and_nothing_outside_the_buffers_is_written(kind, fill):
    """bf16 parameters with a master copy; frozen segments 1 (one element), 2 and 4 hold NaN gradients, NaN-payload
    moments and stale bf16 parameters that are NOT the master's rounding; weight_decay > 0 and l2 > 0.  Every buffer, the
    16-byte block and the table of exactly dctn_param_groups_bytes() sit in a guarded arena; the table's unused slots hold
    garbage."""
    assert L.lib().dctn_param_groups_bytes() == 1552
    case = CASES["small"]
    dtype = BF16
    w0, grads = _synthetic("small", dtype)
    frozen = [False, True, True, False, True, False]
    wds = [1e-3, 1e-2, 1e-2, 1e-3, 1e-2, 1e-3]

    def poison(opt):
        names = ("m", "v") if kind == "adam" else ("buf",)
        for i in range(len(case.sizes)):
            if frozen[i]:
                a, b = case.starts[i], case.ends[i]
                for name in names:
                    getattr(opt, name)[a:b].view(torch.int32).fill_(NAN_BITS)
                opt.flat[a:b] = (opt.master[a:b] * 1.5).to(dtype)       # stale: not the master's rounding
        torch.cuda.synchronize()
        return _owned(opt)

    def run(arena):
        opt, params, table = _grouped(kind, case, "bf16+master", w0, wds=wds, frozen=frozen)
        if arena is not None:
            assert any(r.nbytes == 1552 for r in arena.records)          # the table is an arena allocation of exactly that size
            table._block[4 + 2 * 6: 132] = -1                            # end: -1
            table._block[132 + 6: 196] = 0x7FC00000                      # lr_scale: NaN
            table._block[196 + 6: 260] = -1                              # weight_decay
            table._block[260 + 6: 324] = 0                               # flags: "not frozen"
            table._block[324 + 6: 388] = 0x7FFFFFFF                      # steps
        before = poison(opt)
        stores = []
        for g in grads[:3]:
            g_dev = g.to(dtype).to(DEV)
            for i in range(len(case.sizes)):
                if frozen[i]:
                    g_dev[case.starts[i]: case.ends[i]] = float("nan")
            stores.append((_give(params, g_dev, case, 0, None if arena is None else arena.place), g_dev))
            opt.step()
        return opt, table, before, stores

    with guarded(fill=fill) as arena:
        opt, table, before, stores = run(arena)
    arena.check()   # synchronises; every guard byte around every buffer is intact
    after = _owned(opt)
    for i in range(len(case.sizes)):
        a, b = case.starts[i], case.ends[i]
        for name in after:
            same = _same_bits(after[name][a:b], before[name][a:b])
            assert same == frozen[i], f"{name} of segment {i}: frozen {frozen[i]}, kept its bits {same}"
    for i in range(len(case.sizes)):
        if not frozen[i]:
            for name in after:
                assert torch.isfinite(after[name][case.starts[i]: case.ends[i]].float()).all(), (name, i)
    assert table.steps == [3, 0, 0, 3, 0, 3] and opt.t == 3
    assert torch.isfinite(opt.sq_sum).all()
    for store, g_dev in stores:
        assert _same_bits(store, g_dev), "a gradient buffer changed"
    words = table._block.cpu().numpy()
    assert (words[4 + 12: 132] == -1).all() and (words[324 + 6:] == 0x7FFFFFFF).all()   # the unused slots were only read
    # the same run outside the arena, with clean unused slots: the same bits
    plain, _, _, _ = run(None)
    _assert_same_owned(after, _owned(plain), f"{kind} in the arena")
    assert _same_bits(opt.sq_sum, plain.sq_sum) and _same_bits(opt._state, plain._state)


def test_the_regularisers_value_counts_frozen_elements():
    case = CASES["small"]
    w0, grads = _synthetic("small", F32)
    opt, params, table = _grouped("adam", case, "float32", w0, frozen=[True] * 4 + [False] * 2)
    _give(params, grads[0].to(DEV), case, 0)
    opt.step()
    want = L2 * float((w0[:case.n_reg].double() ** 2).sum())
    assert abs(float(opt.reg_value()) - want) <= 1e-4 * max(1.0, want) and want > 0.01
    assert _same_bits(opt.flat[:case.starts[4]].cpu(), w0[:case.starts[4]])


# ------------------------------------------------------------------ 5. the guard
GUARD_RUNS = [("float32", False), ("float32", True), ("bf16", False), ("bf16+master", True)]


@pytest.mark.parametrize("variant,scheduled", GUARD_RUNS, ids=[f"{v}{'-scheduled' if s else ''}" for v, s in GUARD_RUNS])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_clipped_step_clips_every_unfrozen_segment_and_a_halted_step_advances_nothing(kind, variant, scheduled):
    """A guarded grouped step equals the unguarded grouped step on gradients multiplied by the guard's coefficient.  In
    float32 that product is the kernel's (one rounded float32 product), and the threshold is the median norm: about half
    the steps clip.  A bf16 gradient is widened before the product and not rounded back, which no gradient buffer can
    hold: those runs never clip (the coefficient is 1) and check the rest.  The NaN gradient at step 5 halts: neither
    steps_done nor any segment's count advances - with a schedule, it holds its place - and nothing is written until the
    reset in front of step 8."""
    from dctn_amd.training import GradGuard, LRSchedule

    case = CASES["small"]
    dtype, _ = VARIANTS[variant]
    w0, grads = _synthetic("small", dtype)
    norms = sorted(float(g.double().norm()) for g in grads)
    guard = GradGuard(DEV, 0.5 * (norms[5] + norms[6]) if dtype == F32 else None)
    knots = [(0, 2e-4), (3, 1e-3), (5, 1e-3), (8, 1e-4)]
    kw = [dict(schedule=LRSchedule(DEV, knots, [0, 1, 0, 0])) if scheduled else {} for _ in range(2)]
    opt, params, table = _grouped(kind, case, variant, w0, guard=guard, **kw[0])
    plain, plain_params, plain_table = _grouped(kind, case, variant, w0, **kw[1])
    applied, clipped = 0, 0
    for step, g in enumerate(grads):
        g_dev = g.to(dtype).to(DEV)
        if step == 5:
            g_dev[10] = float("nan")             # in unfrozen segment 0
        if step == 8:
            assert guard.halted
            guard.reset()
        _give(params, g_dev, case, 0)
        before = (_owned(opt), table.steps, opt.t, opt._state.clone())
        opt.step()
        state = guard.read()
        if state["halted"]:
            after = (_owned(opt), table.steps, opt.t, opt._state.clone())
            _assert_same_owned(after[0], before[0], f"halted step {step}")
            assert after[1:3] == before[1:3] == ([applied if not f else 0 for f in case.frozen], applied)
            assert _same_bits(after[3], before[3])
            continue
        clipped += state["coef"] < 1.0
        if dtype == F32:
            g_dev = g_dev * torch.tensor(state["coef"], dtype=F32, device=DEV)
        else:
            assert state["coef"] == 1.0
        _give(plain_params, g_dev, case, 0)
        plain.step()
        applied += 1
        _assert_same_owned(_owned(opt), _owned(plain), f"{kind} {variant} step {step} coef {state['coef']}")
        assert _same_bits(opt._state, plain._state) and _same_bits(opt.sq_sum, plain.sq_sum)
        assert table.steps == plain_table.steps == [0 if f else applied for f in case.frozen] and opt.t == applied
    assert applied == STEPS - 3
    if dtype == F32:
        assert 2 <= clipped <= 7
    assert guard.read()["seen"] == STEPS


# ------------------------------------------------------------------ 6. end to end
def _torch_recipe(params0, batches, dtype, lr, head_scale, wd, l2):
    """The reference's recipe in plain torch: core 0 has requires_grad = False, Adam with param groups skips it; the
    regulariser sums every core."""
    from oracle import ref_cpu as R

    leaves = [p.detach().cpu().clone().to(dtype) for p in params0]
    for t in leaves[1:]:
        t.requires_grad_(True)
    opt = torch.optim.Adam([dict(params=leaves[1:-2], lr=lr), dict(params=leaves[-2:], lr=lr * head_scale)], lr=lr,
                           weight_decay=wd)
    for x, y in batches:
        logits = R.eps_plus_linear_forward(leaves[:-2], leaves[-2], leaves[-1], x.to(dtype))
        loss = torch.nn.functional.cross_entropy(logits, y)
        reg = (leaves[-2] ** 2).sum() + sum((c ** 2).sum() for c in leaves[:-2])
        opt.zero_grad(set_to_none=True)
        (loss + l2 * reg).backward()
        opt.step()
    return [t.detach().double() for t in leaves]


def _tmp_dir():
    import atexit
    import shutil
    import tempfile

    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="dctn_param_groups_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    return _TMP[0]


_TMP = []


def test_a_frozen_core_and_a_slower_head_in_a_graphed_run_with_resume():
    """Fails without the feature.  epses[0].requires_grad = False, the head at a tenth of the rate, warm-up + 20 replays."""
    from dctn_amd import checkpoint as C
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy, param_groups_for

    cpu_batches = _batches(21)
    batches = [(x.to(DEV), y.to(DEV)) for x, y in cpu_batches]

    def objects(seed):
        model = _tiny_model(seed, freeze_first=True)
        groups = param_groups_for(model, freeze_eps=(0,), head_lr_scale=0.1)
        opt = _model_optimizer(model, groups)
        return model, groups, opt

    model, groups, opt = objects(3)
    params = list(model.epses) + [model.linear.weight, model.linear.bias]
    params0 = [p.detach().clone() for p in params]
    assert groups.frozen == [True, False, False, False]
    step = GraphedTrainStep(model, *batches[0], fused_cross_entropy, opt, warmup=1)
    states, path = [], None
    for i, (x, y) in enumerate(batches[1:], start=1):
        step(x, y)
        states.append(_model_state(opt))
        if i == 10:
            run = C.RunState(model, opt)
            assert run.names[:6] == ["optimizer.flat", "optimizer.m", "optimizer.v", "optimizer.groups", "optimizer.state",
                                     "optimizer.sq_sum"]
            path = run.snapshot({"num_iters_done": 10}).save(os.path.join(_tmp_dir(), "groups.dctn"))
    assert opt.t == 21 and groups.steps == [0, 21, 21, 21]
    assert _same_bits(model.epses[0].detach(), params0[0]), "the frozen core moved"
    assert float(opt.m[:params0[0].numel()].abs().max()) == 0.0
    # against the plain-torch float64 loop, judged by that loop's float32 run
    w_ref = _torch_recipe(params0, cpu_batches, F64, 2e-3, 0.1, 1e-3, 1e-2)
    w_t32 = _torch_recipe(params0, cpu_batches, F32, 2e-3, 0.1, 1e-3, 1e-2)
    assert torch.equal(w_ref[0], params0[0].double().cpu())

    def err(ws, idx):
        num = torch.cat([(ws[i].double().cpu() - w_ref[i]).reshape(-1) for i in idx]).norm()
        den = torch.cat([(w_ref[i] - params0[i].double().cpu()).reshape(-1) for i in idx]).norm()
        return float(num / den)

    got = [p.detach() for p in params]
    for idx in [(1, 2, 3)] + [(i,) for i in (1, 2, 3) if params0[i].numel() >= 1000]:
        e_flat, e_torch = err(got, idx), err(w_t32, idx)
        print(f"end to end, parameters {idx}: e_flat={e_flat:.4e} e_torch32={e_torch:.4e} bound={2 * e_torch:.4e}")
        assert e_torch > 0.0
        assert e_flat <= 2.0 * e_torch
    # resume: fresh objects that share nothing with the saved run but the batches
    model2, groups2, opt2 = objects(4)
    step2 = GraphedTrainStep(model2, *batches[0], fused_cross_entropy, opt2, warmup=1)
    step2(*batches[1])
    groups2.set(model2.linear.weight, lr_scale=3.0)
    run2 = C.RunState(model2, opt2)
    assert run2.load(path) == {"num_iters_done": 10}
    _assert_same_model_state(_model_state(opt2), states[9], "after the load")
    assert groups2.steps == [0, 11, 11, 11] and groups2.lr_scales == groups.lr_scales and groups2.frozen == groups.frozen
    for i, (x, y) in enumerate(batches[11:], start=11):
        step2(x, y)
        _assert_same_model_state(_model_state(opt2), states[i - 1], f"the resumed run after replay {i}")
    assert groups2.steps == [0, 21, 21, 21] and opt2.t == 21
    # a file from a run without a table is refused at that entry, and the other way round
    plain_model = _tiny_model(3)
    plain_run = C.RunState(plain_model, _model_optimizer(plain_model, None))
    assert "optimizer.groups" not in plain_run.names
    with pytest.raises(ValueError, match="optimizer.groups"):
        plain_run.load(path)
