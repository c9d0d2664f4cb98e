"""`FlatAdam.step()` / `FlatSGD.step()` against the older entry points, bit for bit (`-m gpu`).

``step()`` describes its step once in a dctn_flat_step_t and calls dctn_adam_flat_step / dctn_sgd_flat_step; the twelve
older entry points take the same buffers as positional arguments and launch the same kernels.  For every combination of
dtype (float32, bf16, bf16 + master), guard, schedule and group table, one optimizer takes three steps through ``step()``
and a twin with equal buffers is stepped by calling the matching older entry point with raw pointers.  Both sides run the
same kernel on the same values, so every owned buffer and block must hold the same bits: a difference is a marshalling
bug - an argument swapped, dropped or stale in the descriptor.

n = 8199, n_reg = 5000: for Adam three workgroups, a vector body up to 8196 and a scalar tail of 3; for SGD 33
workgroups.  Three parameters with ends 1001 (inside a vector of four), 5000 (aligned) and 8199; with a table the first
steps at half the rate, the second is frozen and the third has its own weight decay (Adam).  The schedule's first linear
segment covers steps 0 to 2, and the guard clips on step 1 only.  One more case per optimizer reads its gradients at an
offset of one element, where the launcher must choose the scalar kernel on both sides."""
import pytest
import torch

from dctn_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES, N, N_REG, STEPS = [1001, 3999, 3199], 8199, 5000, 3
LR, BETAS, EPS, WD, L2, MOMENTUM = 1e-3, (0.9, 0.999), 1e-8, 1e-3, 1e-2, 0.9
VARIANTS = {"float32": (torch.float32, False), "bf16": (torch.bfloat16, False), "bf16+master": (torch.bfloat16, True)}
KNOTS = [(0, 2e-4), (4, 1e-3), (8, 5e-4)]
GRAD_SCALES = (1.0, 4.0, 1.0)   # the guard's threshold lies between the norms: only step 1 is clipped


def _inputs(dtype):
    g = torch.Generator().manual_seed(1357)
    w0 = (torch.randn(N, generator=g) * 0.05).to(dtype)
    base = (torch.randn(N, generator=g) * 0.01).to(dtype)
    grads = [(base.float() * s).to(dtype) for s in GRAD_SCALES]
    return w0, grads, 2.0 * float(base.double().norm())


def _build(kind, variant, guard, schedule, groups, w0, max_norm):
    from dctn_amd.training import FlatAdam, FlatSGD, GradGuard, LRSchedule, ParamGroup, ParamGroups

    dtype, master = VARIANTS[variant]
    params = [torch.nn.Parameter(c.clone().to(DEV)) for c in w0.split(SIZES)]
    kw = {}
    if guard:
        kw["guard"] = GradGuard(DEV, max_norm=max_norm)
    if schedule:
        kw["schedule"] = LRSchedule(DEV, KNOTS)
    if groups:
        kw["groups"] = ParamGroups(params, [ParamGroup(params[0], lr_scale=0.5), ParamGroup(params[1], frozen=True),
                                            ParamGroup(params[2], weight_decay=1e-2 if kind == "adam" else None)])
    if kind == "adam":
        opt = FlatAdam(params[:2], params[2:], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, l2=L2, master_weights=master, **kw)
    else:
        opt = FlatSGD(params[:2], params[2:], lr=LR, momentum=MOMENTUM, l2=L2, master_weights=master, **kw)
    assert opt.n == N and opt.n_reg == N_REG and (opt.master is not None) == master
    return opt, params


def _ptr(t):
    return None if t is None else t.data_ptr()


def _legacy_step(kind, opt, g, step):
    """The call `step()` made before the descriptor: the guard's check, then the entry point of the options in use."""
    lib, st = L.lib(), L.stream_ptr(DEV)
    if opt.guard is not None:
        opt.guard.check(g, None)
    master, guard = _ptr(opt.master), _ptr(opt.guard and opt.guard._block)
    sched = None if opt.schedule is None else opt.schedule._block.data_ptr()
    table = None if opt.groups is None else opt.groups._block.data_ptr()
    code = L.dtype_code(opt.flat)
    head = (opt.flat.data_ptr(), g.data_ptr())
    if kind == "adam":
        bufs = head + (opt.m.data_ptr(), opt.v.data_ptr(), opt.sq_sum.data_ptr(), opt._state.data_ptr())
        tail = (N, N_REG, BETAS[0], BETAS[1], EPS)
        if table is not None:
            rc = lib.dctn_adam_l2_step_grouped(master, *bufs, guard, sched, table, *tail, L2, code, st)
        elif sched is not None:
            rc = lib.dctn_adam_l2_step_scheduled(master, *bufs, guard, sched, *tail, WD, L2, code, st)
        elif guard is not None and master is not None:
            rc = lib.dctn_adam_l2_step_master_guarded(master, *bufs, guard, *tail, WD, L2, st)
        elif guard is not None:
            rc = lib.dctn_adam_l2_step_guarded(*bufs, guard, *tail, WD, L2, code, st)
        elif master is not None:
            rc = lib.dctn_adam_l2_step_master(master, *bufs, *tail, WD, L2, st)
        else:
            rc = lib.dctn_adam_l2_step(*bufs, *tail, WD, L2, code, st)
    else:
        bufs = head + (opt.buf.data_ptr(), opt.sq_sum.data_ptr())
        first = 1 if step == 0 else 0
        if table is not None:
            rc = lib.dctn_sgd_l2_step_grouped(master, *bufs, opt._state.data_ptr(), guard, sched, table, N, N_REG, MOMENTUM, L2, code, st)
        elif sched is not None:
            rc = lib.dctn_sgd_l2_step_scheduled(master, *bufs, opt._state.data_ptr(), guard, sched, N, N_REG, MOMENTUM, L2, code, st)
        elif guard is not None and master is not None:
            rc = lib.dctn_sgd_l2_step_master_guarded(master, *bufs, guard, N, N_REG, LR, MOMENTUM, L2, first, st)
        elif guard is not None:
            rc = lib.dctn_sgd_l2_step_guarded(*bufs, guard, N, N_REG, LR, MOMENTUM, L2, first, code, st)
        elif master is not None:
            rc = lib.dctn_sgd_l2_step_master(master, *bufs, N, N_REG, LR, MOMENTUM, L2, first, st)
        else:
            rc = lib.dctn_sgd_l2_step(*bufs, N, N_REG, LR, MOMENTUM, L2, first, code, st)
    assert rc == 0


def _owned(kind, opt):
    bufs = {"flat": opt.flat, "sq_sum": opt.sq_sum}
    bufs.update({"m": opt.m, "v": opt.v} if kind == "adam" else {"buf": opt.buf})
    for name, t in (("master", opt.master), ("state", opt._state), ("guard", opt.guard and opt.guard._block),
                    ("groups", None if opt.groups is None else opt.groups._block)):
        if t is not None:
            bufs[name] = t
    return bufs


def _run(kind, variant, guard, schedule, groups, offset=0):
    dtype = VARIANTS[variant][0]
    w0, grads, max_norm = _inputs(dtype)
    new, params = _build(kind, variant, guard, schedule, groups, w0, max_norm)
    old, _ = _build(kind, variant, guard, schedule, groups, w0, max_norm)
    store = torch.empty(N + offset, dtype=dtype, device=DEV)
    g = store[offset:]
    for p, view in zip(params, g.split(SIZES)):   # back to back: `step()` reads them in place, where the twin reads them
        p.grad = view
    assert (g.data_ptr() % (4 * g.element_size()) != 0) == bool(offset)
    for step in range(STEPS):
        g.copy_(grads[step])
        new.step()
        assert new._desc.grads == g.data_ptr()
        _legacy_step(kind, old, g, step)
    torch.cuda.synchronize()
    got, want = _owned(kind, new), _owned(kind, old)
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name].dtype == want[name].dtype and torch.equal(got[name], want[name]), name
        assert torch.equal(got[name].contiguous().view(torch.uint8), want[name].contiguous().view(torch.uint8)), name
    # the steps were taken, and the options did what the case is built around
    touched = (new.m if kind == "adam" else new.buf).cpu() != 0   # (a bf16 weight may well stay where it was)
    assert touched[:SIZES[0]].any() and touched[N_REG:].any() and touched[SIZES[0]:N_REG].any() == (not groups)
    assert new.t == STEPS
    if guard:
        assert new.guard.read()["clipped"] == 1 and new.guard.read()["seen"] == STEPS
    if groups:
        assert new.groups.steps == [STEPS, 0, STEPS]
    if schedule:
        assert new._state.view(torch.float32)[1].item() == new.schedule.value(STEPS - 1) != new.schedule.value(0)


@pytest.mark.parametrize("groups", [False, True], ids=["", "groups"])
@pytest.mark.parametrize("schedule", [False, True], ids=["", "schedule"])
@pytest.mark.parametrize("guard", [False, True], ids=["", "guard"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_step_and_the_older_entry_point_leave_the_same_bits(kind, variant, guard, schedule, groups):
    _run(kind, variant, guard, schedule, groups)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_the_same_at_an_odd_gradient_offset(kind):
    """Gradients one element past an aligned address: Adam's launcher takes the scalar kernel, on both sides."""
    _run(kind, "bf16+master", True, True, True, offset=1)
    _run(kind, "float32", False, False, False, offset=1)
