"""The weight average (EMA) in the flat step on the GPU (`-m gpu`): `FlatAdam(..., ema=e)` / `FlatSGD(..., ema=e)`.

  1. the step is unchanged: with and without ``ema=`` every other buffer and block ends with the same bits, for every
     combination of guard, schedule and groups;
  2. the average is `WeightEMA.mirror` of the weights read back after every step, bit for bit, with the block's cells;
  3. a halted guarded step leaves the average alone, a clipped step averages the clipped step's weights;
  4. a frozen segment's average stays; a grouped run equals one ungrouped optimizer with an average per segment;
  5. nothing outside any buffer is written (guarded arenas), the stash needs nothing of its previous content;
  6. apply / restore;  7. graphs: K = 1, K = 5 and the eager loop;  8. scoring under the average;  9. resume.

Synthetic sizes are those of tests/test_gpu_param_groups.py's small case: n = 12295 in segments [4099, 1, 3000, 5, 4096,
1094] with n_reg = 7102 (segment ends at vector offsets 3, 0, 0, 1, 1 and a tail of n not divisible by 4; four Adam
workgroups, 49 SGD workgroups), gradients as aligned and odd-offset views, the average's values at a 16-byte boundary
and 4 bytes past one (the scalar form)."""
import functools
import os

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from tests import test_gpu_param_groups as PG
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
LR, WD, L2, MOMENTUM, STEPS = PG.LR, PG.WD, PG.L2, PG.MOMENTUM, PG.STEPS
VARIANTS = PG.VARIANTS
CASE = PG.CASES["small"]
KNOTS, HOLD = [(0, 2e-4), (3, 1e-3), (5, 1e-3), (8, 1e-4)], [0, 1, 0, 0]
LAYOUTS = [(0, 0), (1, 1)]   # (element offset of the gradient view, elements the average's values start past a boundary)
_same_bits = PG._same_bits
assert STEPS == 12 and CASE.n == 12295 and CASE.n_reg == 7102


def _ema(decay=0.999, warmup=True, misalign=0):
    from dctn_amd.training import WeightEMA

    e = WeightEMA(DEV, decay=decay, warmup=warmup)
    e.test_misalign = misalign   # (this file's own note: `_build` moves the values that many elements past a boundary)
    return e


def _move_values(e, misalign):
    """The average's values, once bound, into a buffer that starts `misalign` elements past a 16-byte boundary, and the
    descriptor told: 4 bytes past one, the launcher has to take the scalar form."""
    values = torch.empty(e.values.numel() + misalign, dtype=F32, device=DEV)[misalign:]
    values.copy_(e.values)
    e.values = values
    e._desc.ema = values.data_ptr()


def _build(kind, variant, w0, ema=None, guard=None, scheduled=False, grouped=False, frozen=None, sizes=None, lr=LR, wd=WD,
           n_reg=None):
    """One optimizer over the flat vector, one parameter per segment; the regularised prefix ends inside a segment."""
    from dctn_amd.training import FlatAdam, FlatSGD, LRSchedule, ParamGroup, ParamGroups

    dtype, master = VARIANTS[variant]
    sizes = CASE.sizes if sizes is None else sizes
    params = [torch.nn.Parameter(c.clone().to(dtype).to(DEV)) for c in w0.split(sizes)]
    kw = dict(ema=ema, guard=guard)
    if scheduled:
        kw["schedule"] = LRSchedule(DEV, KNOTS, HOLD)
    if grouped:
        frozen = CASE.frozen if frozen is None else frozen
        kw["groups"] = ParamGroups(params, [ParamGroup([params[i]], lr_scale=CASE.scales[i],
                                                       weight_decay=CASE.wds[i] if kind == "adam" else None,
                                                       frozen=frozen[i]) for i in range(len(params))])
    if kind == "adam":
        opt = FlatAdam(params, [], lr=lr, weight_decay=wd, l2=L2, master_weights=master, **kw)
    else:
        opt = FlatSGD(params, [], lr=lr, momentum=MOMENTUM, l2=L2, master_weights=master, **kw)
    opt.n_reg = CASE.n_reg if n_reg is None else n_reg
    if ema is not None:
        if ema.test_misalign:
            _move_values(ema, ema.test_misalign)
        assert (ema.values.data_ptr() % 16 == 0) == (ema.test_misalign == 0) and ema.values.numel() == opt.n
    return opt, params


def _everything(opt):
    """Every buffer and block of the step but the average's own."""
    torch.cuda.synchronize()
    bufs = PG._owned(opt)
    bufs["sq_sum"] = opt.sq_sum.clone()
    if opt._state is not None:
        bufs["state"] = opt._state.clone()
    if opt.groups is not None:
        bufs["groups"] = opt.groups._block.clone()
    if opt.guard is not None:
        bufs["guard"] = opt.guard._block.clone()
    return bufs


def _kept(opt):
    """The weights the optimizer keeps, as float32 on the CPU: the master copy, else the widened parameters."""
    return (opt.flat.float() if opt.master is None else opt.master).cpu().numpy()


def _cells(e):
    words = e._block.cpu().numpy()
    return int(words[2]), words.view(np.float32)[3].tobytes()


def _median_norm(grads):
    norms = sorted(float(g.double().norm()) for g in grads)
    return 0.5 * (norms[5] + norms[6])


# ------------------------------------------------------------------ 1. the step is unchanged
COMBOS = [(g, s, p) for g in (False, True) for s in (False, True) for p in (False, True)]


@pytest.mark.parametrize("combo", COMBOS, ids=["+".join(n for n, on in zip(("guard", "schedule", "groups"), c) if on) or "plain"
                                               for c in COMBOS])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_the_step_is_unchanged_by_the_average(kind, variant, combo):
    from dctn_amd.training import GradGuard

    guarded_step, scheduled, grouped = combo
    dtype, _ = VARIANTS[variant]
    w0, grads = PG._synthetic("small", dtype)

    def run(ema, offset):
        guard = GradGuard(DEV, _median_norm(grads) if dtype == F32 else None) if guarded_step else None
        opt, params = _build(kind, variant, w0, ema=ema, guard=guard, scheduled=scheduled, grouped=grouped)
        for g in grads:
            PG._give(params, g.to(dtype).to(DEV), CASE, offset)
            opt.step()
        return opt, _everything(opt)

    for offset, misalign in LAYOUTS:
        # (Adam's vector and scalar forms add a workgroup's squares in another order: sq_sum is compared form by form, and
        # an odd-offset gradient view takes the plain optimizer to the scalar form that the misaligned average forces)
        plain, want = run(None, offset)
        assert plain.t == STEPS
        e = _ema(misalign=misalign)
        opt, got = run(e, offset)
        # (a FlatSGD without a schedule or a table has no step block of its own: the average brings one)
        assert set(got) - set(want) == ({"state"} if kind == "sgd" and not (scheduled or grouped) else set())
        PG._assert_same_owned({k: got[k] for k in want}, want, f"{kind} {variant} {combo} layout {(offset, misalign)}")
        assert e.updates == STEPS and opt.t == STEPS
        assert not _same_bits(e.values, (opt.flat.float() if opt.master is None else opt.master))   # it did average


# ------------------------------------------------------------------ 2. the average is the mirror
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_the_average_is_the_mirror_of_the_weights_read_back(kind, variant):
    from dctn_amd.training import WeightEMA

    dtype, _ = VARIANTS[variant]
    w0, grads = PG._synthetic("small", dtype)
    for warmup in (True, False):
        for decay in (0.0, 0.999):
            finals = []
            for offset, misalign in LAYOUTS:
                e = _ema(decay, warmup, misalign)
                opt, params = _build(kind, variant, w0, ema=e)
                mirror = _kept(opt)
                assert e.values.cpu().numpy().tobytes() == mirror.tobytes() and _cells(e) == (0, np.float32(0).tobytes())
                for t, g in enumerate(grads):
                    PG._give(params, g.to(dtype).to(DEV), CASE, offset)
                    opt.step()
                    omd = WeightEMA.weight(decay, warmup, t)
                    mirror = WeightEMA.mirror(mirror, _kept(opt), omd)
                    got = e.values.cpu().numpy()
                    assert got.tobytes() == mirror.tobytes(), (kind, variant, warmup, decay, misalign, t,
                                                               int((got.view(np.int32) != mirror.view(np.int32)).sum()))
                    assert _cells(e) == (t + 1, np.float32(omd).tobytes())
                    assert e.last_omd == omd
                finals.append(mirror)
            assert finals[0].tobytes() == finals[1].tobytes()


# ------------------------------------------------------------------ 3. the guard
@pytest.mark.parametrize("variant", ["float32", "bf16+master"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_halted_step_leaves_the_average_and_a_clipped_step_averages_its_weights(kind, variant):
    from dctn_amd.training import GradGuard, WeightEMA

    dtype, _ = VARIANTS[variant]
    w0, grads = PG._synthetic("small", dtype)
    guard = GradGuard(DEV, _median_norm(grads))
    e = _ema(0.999, True)
    opt, params = _build(kind, variant, w0, ema=e, guard=guard, scheduled=True)
    mirror, applied, clipped = _kept(opt), 0, 0
    for step, g in enumerate(grads):
        g_dev = g.to(dtype).to(DEV)
        if step == 5:
            g_dev[10] = float("nan")
        if step == 8:
            assert guard.halted
            guard.reset()
        PG._give(params, g_dev, CASE, 0)
        before = (e.values.clone(), _cells(e))
        opt.step()
        state = guard.read()
        if state["halted"]:
            assert 5 <= step < 8 and _same_bits(e.values, before[0]) and _cells(e) == before[1], f"halted step {step}"
            continue
        clipped += state["coef"] < 1.0
        omd = WeightEMA.weight(0.999, True, applied)
        mirror = WeightEMA.mirror(mirror, _kept(opt), omd)
        applied += 1
        assert e.values.cpu().numpy().tobytes() == mirror.tobytes(), f"step {step} coef {state['coef']}"
        assert _cells(e) == (applied, np.float32(omd).tobytes())
    assert applied == STEPS - 3 and opt.t == applied and 2 <= clipped <= 7


# ------------------------------------------------------------------ 4. groups
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_frozen_segments_average_stays_and_a_grouped_run_equals_one_optimizer_per_segment(kind, variant):
    dtype, _ = VARIANTS[variant]
    w0, grads = PG._synthetic("small", dtype)
    frozen = [False, True, False, False, True, False]
    for offset, misalign in LAYOUTS:
        e = _ema(0.999, True, misalign)
        opt, params = _build(kind, variant, w0, ema=e, grouped=True, frozen=frozen)
        before = e.values.clone()
        # what a user has without a table: one ungrouped optimizer, with an average of its own, per unfrozen segment
        singles = []
        for i, c in enumerate(w0.split(CASE.sizes)):
            one = _ema(0.999, True)
            single, p = _build(kind, variant, c, ema=one, sizes=[CASE.sizes[i]], lr=PG._seg_rate(LR, CASE.scales[i]),
                               wd=CASE.wds[i], n_reg=min(max(CASE.n_reg - CASE.starts[i], 0), CASE.sizes[i]))
            singles.append((single, p[0], one))
        for g in grads:
            PG._give(params, g.to(dtype).to(DEV), CASE, offset)
            opt.step()
            for i, (single, p, one) in enumerate(singles):
                if not frozen[i]:
                    p.grad = g[CASE.starts[i]: CASE.ends[i]].to(dtype).to(DEV)
                    single.step()
        torch.cuda.synchronize()
        for i, (single, p, one) in enumerate(singles):
            a, b = CASE.starts[i], CASE.ends[i]
            if frozen[i]:
                assert _same_bits(e.values[a:b], before[a:b]), f"the average of frozen segment {i} moved"
                assert one.updates == 0
            else:
                assert _same_bits(e.values[a:b], one.values), f"segment {i}: the grouped average is not the ungrouped one's"
                assert not _same_bits(e.values[a:b], before[a:b])
                assert _cells(one) == _cells(e), f"segment {i} took another omd sequence"
        assert e.updates == STEPS and opt.groups.steps == [0 if f else STEPS for f in frozen]


# ------------------------------------------------------------------ 5. buffer contract
@functools.lru_cache(maxsize=None)
def _contract_run(kind, fill):
    """bf16 parameters with a master copy, a guard, a schedule and a table with frozen segments: three steps, apply,
    restore, every buffer allocated inside the arena at exactly its size."""
    from dctn_amd.training import GradGuard

    w0, grads = PG._synthetic("small", BF16)
    n = CASE.n
    with guarded(fill=fill) as arena:
        e = _ema(0.999, True)
        opt, params = _build(kind, "bf16+master", w0, ema=e, guard=GradGuard(DEV, None), scheduled=True, grouped=True)
        # (the master copy is made by Tensor.to, which the arena does not see: moved there, and the descriptor told)
        opt.master = arena.place(opt.master)
        opt._desc.master = opt.master.data_ptr()
        sizes = [r.nbytes for r in arena.records]
        assert sizes.count(4 * n) >= 3 and 32 in sizes and sizes.count(2 * n) >= 3   # values, master, moments; block; flat, gradients, stash
        assert e.values.numel() == n and e._stash.numel() == n and e._stash.dtype == BF16
        stash_before = e._stash.clone()
        stores = []
        for g in grads[:3]:
            g_dev = g.to(BF16).to(DEV)
            stores.append((PG._give(params, g_dev, CASE, 0, arena.place), g_dev))
            opt.step()
        live, master, values = opt.flat.clone(), opt.master.clone(), e.values.clone()
        e.apply()
        applied = opt.flat.clone()
        assert _same_bits(e._stash, live)
        e.restore()
    arena.check()   # synchronises; every guard byte around every buffer is intact
    for store, g_dev in stores:
        assert _same_bits(store, g_dev), "a gradient buffer changed"
    assert _same_bits(opt.flat, live) and _same_bits(opt.master, master) and _same_bits(e.values, values)
    assert _same_bits(applied, values.to(BF16)) and e.updates == 3
    for i, f in enumerate(CASE.frozen):
        a, b = CASE.starts[i], CASE.ends[i]
        assert _same_bits(values[a:b], w0[a:b].to(DEV)) == f, f"the average of segment {i}: frozen {f}"
    return dict(PG._owned(opt), values=values, applied=applied, block=e._block.clone(), stash=e._stash.clone(),
                stash_before=stash_before)


@pytest.mark.parametrize("fill", [0xFF, 0x7B], ids=["nan_fill", "0x7b_fill"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_nothing_outside_any_buffer_is_written(kind, fill):
    got = _contract_run(kind, fill)
    assert torch.isfinite(got["values"]).all() and torch.isfinite(got["applied"].float()).all()


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_the_stash_does_not_depend_on_what_it_held(kind):
    a, b = _contract_run(kind, 0xFF), _contract_run(kind, 0x7B)
    assert not _same_bits(a["stash_before"], b["stash_before"])
    for name in a:
        if name != "stash_before":
            assert _same_bits(a[name], b[name]), name


# ------------------------------------------------------------------ 6. apply / restore
@pytest.mark.parametrize("n", [5, 4099])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_apply_puts_the_rounded_average_in_place_and_restore_the_old_bits(kind, variant, n):
    dtype, master = VARIANTS[variant]
    g = torch.Generator().manual_seed(n)
    w0 = (torch.randn(n, generator=g) * 0.02).to(dtype).float()
    e = _ema(0.9, False)
    opt, params = _build(kind, variant, w0, ema=e, sizes=[n], n_reg=n)
    for _ in range(3):
        params[0].grad = torch.randn(n, generator=g).to(dtype).to(DEV)
        opt.step()
    torch.cuda.synchronize()
    live, values = opt.flat.clone(), e.values.clone()
    kept = None if opt.master is None else opt.master.clone()
    assert (kept is not None) == master
    e.apply()
    assert e.is_applied
    assert _same_bits(opt.flat, values.to(dtype)) and _same_bits(params[0].detach().reshape(-1), values.to(dtype))
    assert not _same_bits(opt.flat, live)
    assert _same_bits(e.values, values) and (kept is None or _same_bits(opt.master, kept))
    with pytest.raises(RuntimeError, match="applied"):
        opt.step()
    with pytest.raises(RuntimeError, match="already applied"):
        e.apply()
    e.restore()
    assert not e.is_applied and _same_bits(opt.flat, live) and _same_bits(e.values, values)
    with pytest.raises(RuntimeError, match="not applied"):
        e.restore()
    with e.applied():
        assert _same_bits(opt.flat, values.to(dtype))
    assert _same_bits(opt.flat, live) and e.updates == 3
    opt.step()   # and the run goes on
    assert e.updates == 4


# ------------------------------------------------------------------ the recipe's objects (7 - 9)
SIZE, B, N_TRAIN = 10, 16, 64


@functools.lru_cache(maxsize=None)
def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, SIZE, SIZE), dtype=torch.uint8, generator=g), torch.randint(0, 10, (n,), generator=g)


def _model(seed=3, dtype=BF16):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, DEV, dtype, image_size=SIZE)


def _params(model):
    return list(model.epses) + [model.linear.weight, model.linear.bias]


def _source(n=N_TRAIN, seed=0, **kw):
    from dctn_amd.batches import DeviceBatches

    images, labels = _data(n, seed)
    return DeviceBatches(images, labels, B, dtype=BF16, seed=77, **kw)


def _objects(with_ema=True, model_seed=3):
    from dctn_amd.training import FlatAdam, LRSchedule

    model = _model(model_seed)
    e = _ema(0.99, True) if with_ema else None
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3, l2=1e-2,
                   master_weights=True, schedule=LRSchedule(DEV, [(0, 5e-4), (4, 2e-3), (9, 2e-3), (18, 2e-4)], HOLD), ema=e)
    return model, opt, _source(), e


def _graphed(model, opt, src, K=1):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src, iters_per_launch=K)


def _regions(run):
    torch.cuda.synchronize()
    return {name: t.clone().reshape(-1) for name, t in zip(run.names, run.tensors)}   # (the model's `p` has no dimension)


def _assert_same_regions(got, want, what):
    assert list(got) == list(want), what
    for name in want:
        assert _same_bits(got[name], want[name]), f"{what}: region {name} differs"


# ------------------------------------------------------------------ 7. graphs
def test_one_and_five_iterations_per_launch_and_the_eager_loop_leave_the_same_average():
    """The warm-up iteration plus 20: as 20 launches of one, as 4 launches of five, and eagerly with the CPU mirror."""
    from dctn_amd import checkpoint as C
    from dctn_amd.training import WeightEMA, fused_cross_entropy, train_step

    ends = []
    for K, launches in ((1, 20), (5, 4)):
        model, opt, src, e = _objects()
        step = _graphed(model, opt, src, K)
        for _ in range(launches):
            out = step()
        assert out.get("iters", 1) == K
        run = C.RunState(model, opt, batch_source=src)
        assert run.names[:8] == ["optimizer.flat", "optimizer.m", "optimizer.v", "optimizer.master", "optimizer.ema",
                                 "optimizer.ema_block", "optimizer.schedule", "optimizer.state"]
        ends.append(_regions(run))
        assert e.updates == 21 == opt.t
    _assert_same_regions(ends[1], ends[0], "K = 5 against K = 1")
    model, opt, src, e = _objects()
    mirror = opt.master.cpu().numpy()
    for t in range(21):
        x, y, idx = src.empty_batch()
        src.draw_into(x, y, idx)
        train_step(model, x, y, fused_cross_entropy, opt)
        mirror = WeightEMA.mirror(mirror, opt.master.cpu().numpy(), WeightEMA.weight(0.99, True, t))
    assert e.values.cpu().numpy().tobytes() == mirror.tobytes(), "the eager loop's average is not its mirror"
    assert ends[0]["optimizer.ema"].cpu().numpy().tobytes() == mirror.tobytes(), "the graphed average is not the eager one"
    assert _same_bits(ends[0]["optimizer.ema_block"], e._block) and _same_bits(ends[0]["optimizer.master"], opt.master)


# ------------------------------------------------------------------ 8. scoring
def test_scoring_under_the_average_and_the_training_run_afterwards():
    from dctn_amd import checkpoint as C
    from dctn_amd.evaluation import GraphedScore, make_evaluation_hook
    from dctn_amd.training import train_graphed

    def val_source():
        return _source(37, seed=1, shuffle=False)

    # a run that never scored
    model0, opt0, src0, e0 = _objects()
    step0 = _graphed(model0, opt0, src0)
    for _ in range(11):
        step0()
    want = _regions(C.RunState(model0, opt0, batch_source=src0))

    model, opt, src, e = _objects()
    step = _graphed(model, opt, src)
    scorer = GraphedScore(model, val_source())
    for _ in range(10):
        step()
    live = scorer()
    with e.applied():
        averaged = scorer()
        with pytest.raises(RuntimeError, match="applied"):
            step()
        with pytest.raises(RuntimeError, match="applied"):
            train_graphed(step, 1)
        with pytest.raises(RuntimeError, match="applied"):
            C.RunState(model, opt, batch_source=src).snapshot()
    # a fresh model whose parameters were assigned the rounded average by plain copies
    fresh = _model(seed=9)
    with torch.no_grad():
        off = 0
        for p in _params(fresh):
            p.copy_(e.values[off: off + p.numel()].to(BF16).view_as(p))
            off += p.numel()
    assert off == opt.n
    assert GraphedScore(fresh, val_source())() == averaged
    assert averaged != live and scorer() == live
    # the hook: the four old keys as without the average, the two new ones those numbers
    plain_it, ema_it = {}, {}
    train_scorer = GraphedScore(model, _source(N_TRAIN, shuffle=False))
    make_evaluation_hook(train_scorer, scorer)(None, plain_it)
    make_evaluation_hook(train_scorer, scorer, ema=e)(None, ema_it)
    assert sorted(plain_it) == ["train_acc", "train_mean_ce", "val_acc", "val_mean_ce"]
    assert {k: ema_it[k] for k in plain_it} == plain_it and (plain_it["val_mean_ce"], plain_it["val_acc"]) == live
    assert (ema_it["ema_val_mean_ce"], ema_it["ema_val_acc"]) == averaged and len(ema_it) == 6
    assert not e.is_applied
    step()
    _assert_same_regions(_regions(C.RunState(model, opt, batch_source=src)), want, "the launch after scoring")


# ------------------------------------------------------------------ 9. resume
_TMP = []


def _tmp_dir():
    import atexit
    import shutil
    import tempfile

    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="dctn_weight_ema_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    return _TMP[0]


def test_a_resumed_run_continues_the_average_bit_for_bit():
    from dctn_amd import checkpoint as C

    model, opt, src, e = _objects()
    step = _graphed(model, opt, src)          # the warm-up is iteration 1
    run = C.RunState(model, opt, batch_source=src)
    states, path, plain_path = [], None, None
    for i in range(2, 13):
        step()
        states.append(_regions(run))
        if i == 6:
            path = run.snapshot({"num_iters_done": 6}).save(os.path.join(_tmp_dir(), "ema.dctn"))
            saved_values = e.values.clone()
    assert e.updates == 12
    model2, opt2, src2, e2 = _objects(model_seed=4)
    step2 = _graphed(model2, opt2, src2)
    step2()
    e2.decay = 0.5
    run2 = C.RunState(model2, opt2, batch_source=src2)
    assert run2.load(path) == {"num_iters_done": 6}
    assert e2.decay == e.decay and e2.warmup == e.warmup and e2.updates == 6
    _assert_same_regions(_regions(run2), states[4], "after the load")
    for i in range(7, 13):
        step2()
        _assert_same_regions(_regions(run2), states[i - 2], f"the resumed run after iteration {i}")
    # a file and a run that disagree about the option are refused before the device is touched
    plain_model, plain_opt, plain_src, _ = _objects(with_ema=False)
    plain_run = C.RunState(plain_model, plain_opt, batch_source=plain_src)
    assert "optimizer.ema" not in plain_run.names
    untouched = _regions(plain_run)
    with pytest.raises(ValueError, match="optimizer.ema"):
        plain_run.load(path)
    _assert_same_regions(_regions(plain_run), untouched, "a refused load")
    plain_path = plain_run.snapshot().save(os.path.join(_tmp_dir(), "plain.dctn"))
    untouched = _regions(run2)
    with pytest.raises(ValueError, match="optimizer.ema"):
        run2.load(plain_path)
    _assert_same_regions(_regions(run2), untouched, "a refused load")
    # the averaged model of the file
    state = C.read_model_state(path, ema=True)
    live_state = C.read_model_state(path)
    assert list(state) == list(live_state)
    off = 0
    for key, p in (("epses.0", model.epses[0]), ("linear.weight", model.linear.weight), ("linear.bias", model.linear.bias)):
        want = saved_values[off: off + p.numel()].to(BF16).view_as(p).cpu()
        assert state[key].dtype == BF16 and _same_bits(state[key], want), key
        assert not _same_bits(state[key], live_state[key]) or p.numel() < 16, key
        off += p.numel()
    assert off == opt.n
    with pytest.raises(ValueError, match="without a weight average"):
        C.read_model_state(plain_path, ema=True)
    assert list(C.read_model_state(plain_path)) == list(live_state)
