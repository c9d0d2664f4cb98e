"""`FlatSGD(..., weight_decay=...)`: torch.optim.SGD's coupled weight decay in the flat step kernel (`-m gpu`).

The arithmetic is held against torch.optim.SGD with the yardstick of tests/test_gpu_flat_adam.py; a table's per-segment
decays and the combination with the other options are held, bit for bit, against one optimizer per segment; and a
`FlatSGD` built without the keyword is held against the entry points that are older than the descriptor, on the cases of
tests/test_gpu_flat_step_twin.py.  Every measured figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------ against torch
SHAPES_REG, SHAPES_OTHER = [(12001,), (50, 100)], [(2999,), (7,)]
LR, WD, L2, STEPS = 5e-4, 1e-3, 1e-2, 12


def _synthetic(dtype):
    """The set of tests/test_gpu_flat_adam.py."""
    g = torch.Generator().manual_seed(1234)
    n = sum(torch.Size(s).numel() for s in SHAPES_REG + SHAPES_OTHER)
    w0 = (torch.randn(n, generator=g) * 0.02).to(dtype).float()
    q = (n + 3) // 4
    scale = torch.cat([torch.full((q,), s) for s in (1e-6, 1.0, 30.0, 0.0)])[:n]
    grads = [(torch.randn(n, generator=g) * scale).to(dtype).float() for _ in range(STEPS)]
    return n, w0, grads


def _split(flat, shapes):
    out, off = [], 0
    for s in shapes:
        k = torch.Size(s).numel()
        out.append(flat[off: off + k].reshape(s))
        off += k
    return out


@functools.lru_cache(maxsize=None)
def _run_torch(dtype, run_dtype, momentum):
    n, w0, grads = _synthetic(dtype)
    n_reg = sum(torch.Size(s).numel() for s in SHAPES_REG)
    params = [torch.nn.Parameter(p.clone().to(run_dtype)) for p in _split(w0, SHAPES_REG + SHAPES_OTHER)]
    opt = torch.optim.SGD(params, lr=LR, momentum=momentum, weight_decay=WD)
    for g in grads:
        flat_w = torch.cat([p.detach().reshape(-1) for p in params])
        full = g.to(torch.float64 if run_dtype == torch.float64 else torch.float32).clone()
        full[:n_reg] += 2 * L2 * flat_w[:n_reg].to(full.dtype)
        for p, gp in zip(params, _split(full.to(run_dtype), SHAPES_REG + SHAPES_OTHER)):
            p.grad = gp.clone()
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in params]).double()


@pytest.mark.parametrize("layout", ["separate", "back_to_back_offset"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_decayed_flat_sgd_matches_torch_sgd_within_torchs_own_error(dtype, momentum, layout):
    """12 steps on 20 007 synthetic parameters against torch.optim.SGD(momentum, weight_decay=1e-3) in float64 (CPU):
    e_flat <= 2 * e_torch32 (float32), <= 1.5 * e_torch_bf16 (bfloat16), with e = |w - w_ref| / |w_ref - w_0|."""
    from dctn_amd.training import FlatSGD

    n, w0, grads = _synthetic(dtype)
    w_ref, w_torch = _run_torch(dtype, torch.float64, momentum), _run_torch(dtype, dtype, momentum)
    params = [torch.nn.Parameter(p.clone().to(dtype).to(DEV)) for p in _split(w0, SHAPES_REG + SHAPES_OTHER)]
    k = len(SHAPES_REG)
    opt = FlatSGD(params[:k], params[k:], lr=LR, momentum=momentum, l2=L2, weight_decay=WD)
    for g in grads:
        if layout == "separate":
            for p, gp in zip(params, _split(g.to(dtype).to(DEV), SHAPES_REG + SHAPES_OTHER)):
                p.grad = gp.clone()
        else:
            buf = torch.zeros(n + 1, dtype=dtype, device=DEV)
            buf[1:] = g.to(dtype).to(DEV)
            for p, gp in zip(params, _split(buf[1:], SHAPES_REG + SHAPES_OTHER)):
                p.grad = gp
        opt.step()
    assert opt.t == STEPS
    w_flat = torch.cat([p.detach().reshape(-1) for p in params]).double().cpu()
    moved = float((w_ref - w0.double()).norm())
    e_torch, e_flat = float((w_torch - w_ref).norm()) / moved, float((w_flat - w_ref).norm()) / moved
    factor = 2.0 if dtype == F32 else 1.5
    print(f"\nFlatSGD(weight_decay) {dtype} momentum={momentum} {layout}: e_flat={e_flat:.4e} e_torch={e_torch:.4e} "
          f"ratio={e_flat / e_torch:.4f} bound={factor * e_torch:.4e}")
    assert e_flat <= factor * e_torch


# ------------------------------------------------------------------ per segment, bit for bit
SIZES = [1001, 3999, 3199]   # ends 1001, 5000, 8199; 33 workgroups of 256
N = sum(SIZES)
KNOTS = [(0, 2e-4), (3, 1e-3), (5, 5e-4)]
SEG_WD = (5e-2, None, 0.0)       # an own decay, the optimizer's, none
SEG_SCALE = (1.0, 0.5, 1.0)


def _problem(dtype, steps):
    g = torch.Generator().manual_seed(4242)
    w0 = (torch.randn(N, generator=g) * 0.05).to(dtype)
    return w0, [(torch.randn(N, generator=g) * 0.01).to(dtype) for _ in range(steps)]


def _make(w0, sizes, n_reg_params, **kw):
    from dctn_amd.training import FlatSGD

    params = [torch.nn.Parameter(c.clone().to(DEV)) for c in w0.split(sizes)]
    args = dict(lr=1e-3, momentum=0.9, l2=L2, weight_decay=WD)
    args.update({k: (v(params) if callable(v) else v) for k, v in kw.items()})
    opt = FlatSGD(params[:n_reg_params], params[n_reg_params:], **args)
    store = torch.zeros(w0.numel(), dtype=w0.dtype, device=DEV)
    for p, view in zip(params, store.split(sizes)):
        p.grad = view
    return opt, store


def _table(ps):
    from dctn_amd.training import ParamGroup, ParamGroups

    return ParamGroups(ps, [ParamGroup(p, lr_scale=s, weight_decay=w) for p, s, w in zip(ps, SEG_SCALE, SEG_WD)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_a_table_with_per_segment_decays_is_one_decayed_optimizer_per_segment(dtype):
    w0, grads = _problem(dtype, 3)
    whole, sw = _make(w0, SIZES, 2, groups=_table)
    twins = []
    for i, piece in enumerate(w0.split(SIZES)):
        lr = float(np.float32(1e-3) * np.float32(SEG_SCALE[i]))
        twins.append(_make(piece, [SIZES[i]], 1 if i < 2 else 0, lr=lr, weight_decay=WD if SEG_WD[i] is None else SEG_WD[i]))
    for g in grads:
        sw.copy_(g)
        whole.step()
        for (opt, store), piece in zip(twins, g.split(SIZES)):
            store.copy_(piece)
            opt.step()
    torch.cuda.synchronize()
    for name in ("flat", "buf"):
        assert _bits(getattr(whole, name), torch.cat([getattr(t[0], name) for t in twins])), name
    assert whole.groups.steps == [3, 3, 3] and not _bits(whole.flat, w0.to(DEV))
    # and the decays did differ: the same table with one decay for all ends elsewhere in segment 0
    from dctn_amd.training import ParamGroups
    same, ss = _make(w0, SIZES, 2, groups=lambda ps: ParamGroups(ps))
    for g in grads:
        ss.copy_(g)
        same.step()
    torch.cuda.synchronize()
    assert not _bits(same.flat[:SIZES[0]], whole.flat[:SIZES[0]])


def test_guard_schedule_average_and_master_together_split_per_segment():
    """bf16 parameters on master weights, a guard that lets every step through (its norm covers the whole buffer, so a
    clipped step has no per-segment twin), a schedule, an average and a table of decays and rates, in one launch: against
    one optimizer with the same options per segment, whose schedule carries the segment's rate scale."""
    from dctn_amd.training import GradGuard, LRSchedule, WeightEMA

    w0, grads = _problem(BF16, 6)
    opts = lambda: dict(master_weights=True, guard=GradGuard(DEV, None), schedule=LRSchedule(DEV, KNOTS),   # noqa: E731
                        ema=WeightEMA(DEV, 0.9))
    whole, sw = _make(w0, SIZES, 2, groups=_table, **opts())
    twins = []
    for i, piece in enumerate(w0.split(SIZES)):
        kw = opts()
        kw["schedule"].scale = SEG_SCALE[i]
        twins.append(_make(piece, [SIZES[i]], 1 if i < 2 else 0, weight_decay=WD if SEG_WD[i] is None else SEG_WD[i], **kw))
    for g in grads:
        sw.copy_(g)
        whole.step()
        for (opt, store), piece in zip(twins, g.split(SIZES)):
            store.copy_(piece)
            opt.step()
    torch.cuda.synchronize()
    for name in ("flat", "master", "buf"):
        assert _bits(getattr(whole, name), torch.cat([getattr(t[0], name) for t in twins])), name
    assert _bits(whole.ema.values, torch.cat([t[0].ema.values for t in twins]))
    assert whole.t == 6 and whole.ema.updates == 6 and whole.guard.read()["seen"] == 6
    assert float(whole._state.view(F32)[1]) == whole.schedule.value(5)
    assert not _bits(whole.master, w0.float().to(DEV))


def test_a_clipped_decayed_step_is_the_unguarded_one_on_scaled_gradients():
    from dctn_amd.training import GradGuard

    w0, grads = _problem(F32, 2)
    guard = GradGuard(DEV, 0.5 * float(grads[0].double().norm()))
    guarded, sg = _make(w0, SIZES, 2, guard=guard)
    twin, st = _make(w0, SIZES, 2)
    for g in grads:
        sg.copy_(g)
        guarded.step()
        coef = guard.read()["coef"]
        assert 0.0 < coef < 1.0
        st.copy_(torch.from_numpy(g.numpy() * np.float32(coef)))
        twin.step()
    torch.cuda.synchronize()
    for name in ("flat", "buf", "sq_sum"):
        assert _bits(getattr(guarded, name), getattr(twin, name)), name


def test_a_decay_of_zero_leaves_the_bits_of_no_decay_and_is_kept_in_the_state():
    w0, grads = _problem(F32, 3)
    a, sa = _make(w0, SIZES, 2, weight_decay=0.0)
    b, sb = _make(w0, SIZES, 2, weight_decay=None)
    c, sc = _make(w0, SIZES, 2)   # WD
    for g in grads:
        for opt, store in ((a, sa), (b, sb), (c, sc)):
            store.copy_(g)
            opt.step()
    torch.cuda.synchronize()
    for name in ("flat", "buf", "sq_sum"):
        assert _bits(getattr(a, name), getattr(b, name)), name
    assert not _bits(a.flat, c.flat)
    assert a.state_dict()["weight_decay"] == 0.0 and a.run_host()["weight_decay"] == 0.0
    assert "weight_decay" not in b.state_dict() and "weight_decay" not in b.run_host()
    d, _ = _make(w0, SIZES, 2, weight_decay=0.25)
    d.load_state_dict(c.state_dict())
    assert d.weight_decay == WD and _bits(d.buf, c.buf)


# ------------------------------------------------------------------ without the keyword: the parent's entry points
@pytest.mark.parametrize("groups", [False, True], ids=["", "groups"])
@pytest.mark.parametrize("schedule", [False, True], ids=["", "schedule"])
@pytest.mark.parametrize("guard", [False, True], ids=["", "guard"])
@pytest.mark.parametrize("variant", ["bf16", "bf16+master", "float32"])
def test_without_the_keyword_step_leaves_the_bits_of_the_older_entry_points(variant, guard, schedule, groups):
    """The cases of tests/test_gpu_flat_step_twin.py for SGD: `FlatSGD` built as before this option existed against
    dctn_sgd_l2_step* called with raw pointers."""
    from tests import test_gpu_flat_step_twin as twin

    twin._run("sgd", variant, guard, schedule, groups)


def test_without_the_keyword_at_an_odd_gradient_offset():
    from tests import test_gpu_flat_step_twin as twin

    twin._run("sgd", "bf16+master", True, True, True, offset=1)
    twin._run("sgd", "float32", False, False, False, offset=1)
