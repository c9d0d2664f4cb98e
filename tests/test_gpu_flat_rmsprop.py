"""`FlatRMSprop` (one HIP launch per RMSprop step over the flat parameter buffer) on the GPU (`-m gpu`).

The arithmetic is held against torch.optim.RMSprop with the yardstick of tests/test_gpu_flat_adam.py: torch's own error
in the test dtype against a float64 reference bounds the kernel's.  Everything else is bit for bit: the vector form
against the scalar form, one launch against a split of the buffer, every option against the run that does the option's
work on the host, captured graphs against eager steps, and resumed runs against uninterrupted ones.  Every measured
figure is printed before it is asserted (run with -s to see them)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------ 1. against torch
SHAPES_REG, SHAPES_OTHER = [(12001,), (50, 100)], [(2999,), (7,)]   # 12001 * 4 (or * 2) bytes: not a multiple of 16
LR, ALPHA, EPS, WD, L2, STEPS = 5e-4, 0.99, 1e-8, 1e-3, 1e-2, 12


def _synthetic(dtype):
    """The set of tests/test_gpu_flat_adam.py: initial weights and STEPS gradients (flat, CPU, float32 values
    representable in `dtype`); the gradient scale is 1e-6 / 1 / 30 / exactly 0 by quarter of the flat vector."""
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
    """torch.optim.RMSprop on the CPU in `run_dtype` on the `dtype` set, the 2 * l2 * w term of the regularised prefix
    added by hand.  Returns the final flat weights (float64) and l2 * sum w^2 over the prefix before the last update."""
    n, w0, grads = _synthetic(dtype)
    n_reg = sum(torch.Size(s).numel() for s in SHAPES_REG)
    params = [torch.nn.Parameter(p.clone().to(run_dtype)) for p in _split(w0, SHAPES_REG + SHAPES_OTHER)]
    opt = torch.optim.RMSprop(params, lr=LR, alpha=ALPHA, eps=EPS, weight_decay=WD, momentum=momentum)
    reg_before_last = None
    for g in grads:
        flat_w = torch.cat([p.detach().reshape(-1) for p in params])
        reg_before_last = L2 * float((flat_w[:n_reg].double() ** 2).sum())
        full = g.to(torch.float64 if run_dtype == torch.float64 else torch.float32).clone()
        full[:n_reg] += 2 * L2 * flat_w[:n_reg].to(full.dtype)
        for p, gp in zip(params, _split(full.to(run_dtype), SHAPES_REG + SHAPES_OTHER)):
            p.grad = gp.clone()
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in params]).double(), reg_before_last


@pytest.mark.parametrize("layout", ["separate", "back_to_back_offset"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_flat_rmsprop_matches_torch_rmsprop_within_torchs_own_error(dtype, momentum, layout):
    """12 steps on 20 007 synthetic parameters against torch.optim.RMSprop in float64 (CPU).  With
    e = |w - w_ref| / |w_ref - w_0|: e_flat <= 2 * e_torch32 for float32 parameters and <= 1.5 * e_torch_bf16 for
    bfloat16 ones, the Adam test's factors.  `layout`: gradients in separate tensors (gathered by the step) or back to
    back at an odd element offset (read in place, the one-element-per-lane form of the kernel)."""
    from dctn_amd.training import FlatRMSprop

    n, w0, grads = _synthetic(dtype)
    n_reg = sum(torch.Size(s).numel() for s in SHAPES_REG)
    w_ref, reg_ref = _run_torch(dtype, torch.float64, momentum)
    w_torch, _ = _run_torch(dtype, dtype, momentum)

    params = [torch.nn.Parameter(p.clone().to(dtype).to(DEV)) for p in _split(w0, SHAPES_REG + SHAPES_OTHER)]
    k = len(SHAPES_REG)
    opt = FlatRMSprop(params[:k], params[k:], lr=LR, alpha=ALPHA, eps=EPS, weight_decay=WD, momentum=momentum, l2=L2)
    assert params[1].data_ptr() % 16 != 0   # re-pointed behind the 12001-element parameter
    assert (opt.buf is None) == (momentum == 0.0)
    own_reg = None
    for g in grads:
        if layout == "separate":
            for p, gp in zip(params, _split(g.to(dtype).to(DEV), SHAPES_REG + SHAPES_OTHER)):
                p.grad = gp.clone()
        else:
            buf = torch.zeros(n + 1, dtype=dtype, device=DEV)
            buf[1:] = g.to(dtype).to(DEV)
            for p, gp in zip(params, _split(buf[1:], SHAPES_REG + SHAPES_OTHER)):
                p.grad = gp
        own_reg = L2 * float((opt.flat[:n_reg].double() ** 2).sum())
        opt.step()
    assert opt.t == STEPS
    w_flat = torch.cat([p.detach().reshape(-1) for p in params]).double().cpu()
    moved = float((w_ref - w0.double()).norm())
    e_torch, e_flat = float((w_torch - w_ref).norm()) / moved, float((w_flat - w_ref).norm()) / moved
    factor = 2.0 if dtype == F32 else 1.5
    print(f"\nFlatRMSprop {dtype} momentum={momentum} {layout}: e_flat={e_flat:.4e} e_torch={e_torch:.4e} "
          f"ratio={e_flat / e_torch:.4f} bound={factor * e_torch:.4e}")
    assert e_flat <= factor * e_torch
    reg = float(opt.reg_value())
    print(f"reg_value={reg:.8e} own weights={own_reg:.8e} float64 reference={reg_ref:.8e}")
    assert abs(reg - own_reg) <= 1e-4 * max(1.0, own_reg)
    if dtype == F32:
        assert abs(reg - reg_ref) <= 1e-4 * max(1.0, reg_ref)


# ------------------------------------------------------------------ shared: small flat problems
def _problem(n, dtype, steps, seed=97, gscale=0.01):
    """(w0, [g_0 ...]) on the CPU in `dtype`."""
    g = torch.Generator().manual_seed(seed + n % 1000)
    w0 = (torch.randn(n, generator=g) * 0.05).to(dtype)
    return w0, [(torch.randn(n, generator=g) * gscale).to(dtype) for _ in range(steps)]


def _make(w0, sizes, n_reg_params, **kw):
    """A FlatRMSprop over `w0` cut into `sizes`, the first `n_reg_params` of them regularised, and its gradient store:
    one flat tensor whose pieces are the parameters' .grad, so that `store.copy_(g)` sets the next step's gradients."""
    from dctn_amd.training import FlatRMSprop

    params = [torch.nn.Parameter(c.clone().to(DEV)) for c in w0.split(sizes)]
    args = dict(lr=1e-3, alpha=ALPHA, eps=EPS, weight_decay=WD, momentum=0.9, l2=L2)
    make_kw = {k: (v(params) if callable(v) else v) for k, v in kw.items()}
    args.update(make_kw)
    opt = FlatRMSprop(params[:n_reg_params], params[n_reg_params:], **args)
    store = torch.zeros(w0.numel(), dtype=w0.dtype, device=DEV)
    for p, view in zip(params, store.split(sizes)):
        p.grad = view
    return opt, store, params


def _owned(opt):
    torch.cuda.synchronize()
    out = {"flat": opt.flat, "square_avg": opt.square_avg, "sq_sum": opt.sq_sum, "state": opt._state}
    if opt.buf is not None:
        out["buf"] = opt.buf
    if opt.master is not None:
        out["master"] = opt.master
    return {k: v.clone() for k, v in out.items()}


def _assert_same(got, want, what, skip=()):
    for name in want:
        if name not in skip:
            assert _bits(got[name], want[name]), f"{what}: {name} differs"


VARIANTS = {"float32": (F32, False), "bf16+master": (BF16, True)}
SIZES = [1001, 3999, 3199]   # ends 1001 (inside a vector of four), 5000, 8199: three workgroups, a tail of 3
N = sum(SIZES)


# ------------------------------------------------------------------ 2. master weights
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_the_master_copy_follows_the_float32_optimizer_bit_for_bit(momentum):
    w0, grads = _problem(N, BF16, 4)
    a, sa, _ = _make(w0, SIZES, 2, master_weights=True, momentum=momentum)
    b, sb, _ = _make(w0.float(), SIZES, 2, momentum=momentum)
    assert a.master is not None and b.master is None
    for g in grads:
        sa.copy_(g), sb.copy_(g.float())
        a.step(), b.step()
    A, B = _owned(a), _owned(b)
    assert _bits(A["master"], B["flat"]) and _bits(A["square_avg"], B["square_avg"]) and _bits(A["sq_sum"], B["sq_sum"])
    assert momentum == 0.0 or _bits(A["buf"], B["buf"])
    assert _bits(A["flat"], B["flat"].to(BF16)) and not _bits(B["flat"], w0.float().to(DEV))


# ------------------------------------------------------------------ 3. forms and sizes
def _raw_run(w0, grads, offset, momentum, dtype):
    """Two steps through the C entry point with every buffer `offset` elements past an aligned address."""
    n = w0.numel()

    def at(t):
        store = torch.zeros(n + offset, dtype=t.dtype, device=DEV)
        store[offset:] = t.to(DEV)
        return store[offset:]

    w, g = at(w0), at(grads[0])
    sq, buf = at(torch.zeros(n)), at(torch.zeros(n)) if momentum > 0 else None
    sq_sum = torch.zeros(L.lib().dctn_rmsprop_num_partials(n), dtype=F32, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    state.view(F32)[1] = 1e-3
    assert (w.data_ptr() % 16 != 0) == bool(offset) and (sq.data_ptr() % 16 != 0) == bool(offset)
    desc = L.FlatStep(params=w.data_ptr(), master=None, grads=g.data_ptr(), sq_sum=sq_sum.data_ptr(), state=state.data_ptr(),
                      guard=None, schedule=None, groups=None, n=n, n_reg=n - 5, l2=L2, dtype=L.dtype_code(w))
    for step in grads:
        g.copy_(step)
        rc = L.lib().dctn_rmsprop_flat_step(ctypes.byref(desc), None, sq.data_ptr(), None if buf is None else buf.data_ptr(), ALPHA,
                                            EPS, WD, momentum, L.stream_ptr(DEV))
        assert rc == 0
    torch.cuda.synchronize()
    assert int(state[0]) == len(grads) and int(state[2]) == 0
    return w.clone(), sq.clone(), None if buf is None else buf.clone(), sq_sum.clone()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_aligned_and_odd_addresses_leave_the_same_bits(dtype, momentum):
    """The vector form (aligned pointers) against the scalar form (every pointer one element past): n = 8199, three
    workgroups."""
    w0, grads = _problem(N, dtype, 2)
    vec, scalar = _raw_run(w0, grads, 0, momentum, dtype), _raw_run(w0, grads, 1, momentum, dtype)
    for a, b, name in zip(vec, scalar, ("params", "square_avg", "buf", "sq_sum")):
        if a is not None and name != "sq_sum":   # the slots sum the same squares in another order
            assert _bits(a, b), name
    assert torch.allclose(vec[3].sum(), scalar[3].sum(), rtol=1e-5)
    assert not _bits(vec[0], w0.to(DEV))


@pytest.mark.parametrize("n", [3, 4099, 256 * 4096 + 4 * 1024 + 3])
def test_one_launch_equals_launches_over_a_split_of_the_buffer(n):
    """n = 3: the tail only; 4 099: two workgroups, one ticket hand-over; 256 * 4096 + 4 * 1024 + 3: every lane takes a
    second trip, and there is a tail.  An element's result does not depend on where in a launch it lies."""
    w0, grads = _problem(n, F32, 2)
    cut = n // 2 + 1 if (n // 2 + 1) % 2 else n // 2 + 2   # an odd cut: the second piece starts a vector elsewhere
    cut = min(cut, n - 1)
    whole, sw, _ = _make(w0, [n], 1)
    parts = [_make(piece, [piece.numel()], 1) for piece in (w0[:cut], w0[cut:])]
    for g in grads:
        sw.copy_(g)
        whole.step()
        for (opt, store, _), piece in zip(parts, (g[:cut], g[cut:])):
            store.copy_(piece)
            opt.step()
    torch.cuda.synchronize()
    assert whole.t == 2 and all(p[0].t == 2 for p in parts)
    assert whole.sq_sum.numel() == L.lib().dctn_rmsprop_num_partials(n) == min(256, (n + 4095) // 4096)
    for name in ("flat", "square_avg", "buf"):
        assert _bits(getattr(whole, name), torch.cat([getattr(p[0], name) for p in parts])), name
    assert not _bits(whole.flat, w0.to(DEV))
    # sq_sum: the squares before the last step, of the same weights on both sides, summed in another order
    total, split = float(whole.sq_sum.double().sum()), sum(float(p[0].sq_sum.double().sum()) for p in parts)
    print(f"\nn={n}: sq_sum total={total:.8e} over the split={split:.8e}")
    assert total > 0.0 and abs(total - split) <= 1e-5 * total


# ------------------------------------------------------------------ 4. options
def _steps(opt, store, grads):
    for g in grads:
        store.copy_(g)
        opt.step()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_an_unclipped_guarded_step_is_the_unguarded_step(variant):
    from dctn_amd.training import GradGuard

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 3)
    plain, sp, _ = _make(w0, SIZES, 2, master_weights=master)
    guard = GradGuard(DEV, None)
    guarded, sg, _ = _make(w0, SIZES, 2, master_weights=master, guard=guard)
    _steps(plain, sp, grads), _steps(guarded, sg, grads)
    _assert_same(_owned(guarded), _owned(plain), "unclipped")
    assert guard.read()["seen"] == 3 and guard.read()["clipped"] == 0


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_clipped_step_is_the_unguarded_step_on_scaled_gradients(variant):
    """The twin is a float32 optimizer given float32(g) * coef, one rounded product (a clipped bf16 gradient is widened
    and not rounded back); with master weights the master copy is that optimizer's parameter buffer, bit for bit."""
    from dctn_amd.training import GradGuard

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 2)
    max_norm = 0.5 * float(grads[0].double().norm())
    guard = GradGuard(DEV, max_norm)
    guarded, sg, _ = _make(w0, SIZES, 2, master_weights=master, guard=guard)
    twin, st, _ = _make(w0.float(), SIZES, 2)
    for g in grads:
        sg.copy_(g)
        guarded.step()
        coef = guard.read()["coef"]
        print(f"\nclipped step: norm={guard.read()['last_norm']:.6f} coef={coef:.8f}")
        assert 0.0 < coef < 1.0
        st.copy_(torch.from_numpy(g.float().numpy() * np.float32(coef)))   # float32 * float32: one rounded product
        twin.step()
    G, T = _owned(guarded), _owned(twin)
    assert _bits(G["master"] if master else G["flat"], T["flat"])
    for name in ("square_avg", "buf", "sq_sum"):
        assert _bits(G[name], T[name]), name
    assert guard.read()["clipped"] == 2


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_halted_step_changes_nothing(variant):
    from dctn_amd.training import GradGuard, ParamGroup, ParamGroups, WeightEMA

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 2)
    guard, ema = GradGuard(DEV, None), WeightEMA(DEV, 0.9, warmup=False)
    opt, store, params = _make(w0, SIZES, 2, master_weights=master, guard=guard, ema=ema,
                               groups=lambda ps: ParamGroups(ps, [ParamGroup(ps[0], lr_scale=0.5)]))
    _steps(opt, store, grads[:1])
    opt.sq_sum.fill_(float("nan"))   # pre-poisoned slots: a halted launch must not store to them
    before = _owned(opt)
    ema_before, table_before = ema.values.clone(), opt.groups._block.clone()
    bad = grads[1].clone()
    bad[4321] = float("inf")
    _steps(opt, store, [bad])
    assert guard.halted and opt.t == 1 and ema.updates == 1 and opt.groups.steps == [1, 1, 1]
    _assert_same(_owned(opt), before, "halted")
    assert _bits(ema.values, ema_before) and _bits(opt.groups._block, table_before)
    _steps(opt, store, [grads[1]])   # the latch holds for a finite gradient too
    _assert_same(_owned(opt), before, "halted, finite gradient")


KNOTS = [(0, 2e-4), (3, 1e-3), (5, 5e-4)]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_scheduled_run_is_the_run_whose_rate_the_host_sets(variant):
    from dctn_amd.training import LRSchedule

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 6)
    sched = LRSchedule(DEV, KNOTS)
    a, sa, _ = _make(w0, SIZES, 2, master_weights=master, schedule=sched)
    b, sb, _ = _make(w0, SIZES, 2, master_weights=master)
    for t, g in enumerate(grads):
        rate = sched.value(t)
        assert a.lr == rate
        b.lr = rate
        sa.copy_(g), sb.copy_(g)
        a.step(), b.step()
        torch.cuda.synchronize()
        assert float(a._state.view(F32)[1]) == rate and a.t == t + 1   # the block's rate cell holds the rate used
    _assert_same(_owned(a), _owned(b), "scheduled")
    assert len({sched.value(t) for t in range(6)}) > 3
    with pytest.raises(RuntimeError):
        a.lr = 1.0


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_an_all_default_table_is_no_table(variant):
    from dctn_amd.training import ParamGroups

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 3)
    a, sa, _ = _make(w0, SIZES, 2, master_weights=master, groups=lambda ps: ParamGroups(ps))
    b, sb, _ = _make(w0, SIZES, 2, master_weights=master)
    _steps(a, sa, grads), _steps(b, sb, grads)
    _assert_same(_owned(a), _owned(b), "all-default table")
    assert a.groups.steps == [3, 3, 3]


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_three_segment_table_is_one_optimizer_per_segment(variant, momentum):
    """Segments end at 1001 (no multiple of 4: one vector straddles it), 5000 and 8199: the first frozen, the second at
    a tenth of the rate, the third with its own weight decay.  n_reg = 5000."""
    from dctn_amd.training import ParamGroup, ParamGroups

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 3)
    lr, own_wd = 1e-3, 5e-2
    whole, sw, _ = _make(w0, SIZES, 2, master_weights=master, momentum=momentum, lr=lr, groups=lambda ps: ParamGroups(
        ps, [ParamGroup(ps[0], frozen=True), ParamGroup(ps[1], lr_scale=0.1), ParamGroup(ps[2], weight_decay=own_wd)]))
    pieces = w0.split(SIZES)
    tenth = float(np.float32(lr) * np.float32(0.1))   # the segment's rate: one rounded float32 product
    second, s2, _ = _make(pieces[1], [SIZES[1]], 1, master_weights=master, momentum=momentum, lr=tenth)
    third, s3, _ = _make(pieces[2], [SIZES[2]], 0, master_weights=master, momentum=momentum, lr=lr, weight_decay=own_wd)
    for g in grads:
        sw.copy_(g), s2.copy_(g.split(SIZES)[1]), s3.copy_(g.split(SIZES)[2])
        whole.step(), second.step(), third.step()
    torch.cuda.synchronize()
    names = ["flat", "square_avg"] + (["buf"] if momentum else []) + (["master"] if master else [])
    for name in names:
        got = getattr(whole, name).split(SIZES)
        start = (w0.to(DEV) if name == "flat" else w0.float().to(DEV) if name == "master" else torch.zeros(N, device=DEV))
        assert _bits(got[0], start.split(SIZES)[0]), f"frozen segment: {name} was touched"
        assert _bits(got[1], getattr(second, name)) and _bits(got[2], getattr(third, name)), name
    assert not _bits(whole.flat[SIZES[0]:], w0.to(DEV)[SIZES[0]:])
    assert whole.groups.steps == [0, 3, 3] and whole.t == 3
    # the frozen segment's squares still count: the regularised prefix is segments 0 and 1
    kept = whole.master if master else whole.flat
    own = float((w0[:SIZES[0]].double() ** 2).sum())
    total = float(whole.sq_sum.double().sum())
    print(f"\nsq_sum total={total:.8e} frozen segment's share={own:.8e} second optimizer's={float(second.sq_sum.sum()):.8e}")
    assert abs(total - (own + float(second.sq_sum.double().sum()))) <= 1e-5 * total
    assert kept is not None


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_average_is_the_host_mirror_and_changes_nothing_else(variant):
    from dctn_amd.training import WeightEMA

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 4)
    ema = WeightEMA(DEV, 0.9, warmup=True)
    a, sa, _ = _make(w0, SIZES, 2, master_weights=master, ema=ema)
    b, sb, _ = _make(w0, SIZES, 2, master_weights=master)
    mirror = w0.float().numpy().copy()
    for u, g in enumerate(grads):
        sa.copy_(g), sb.copy_(g)
        a.step(), b.step()
        torch.cuda.synchronize()
        kept = (a.master if master else a.flat.float()).cpu().numpy()
        omd = WeightEMA.weight(0.9, True, u)
        mirror = WeightEMA.mirror(mirror, kept, omd)
        assert ema.last_omd == omd and ema.updates == u + 1
        assert _bits(ema.values.cpu(), torch.from_numpy(mirror)), f"average after update {u}"
    _assert_same(_owned(a), _owned(b), "with an average")


# ------------------------------------------------------------------ 5. capture  (the 10 x 10 model of the Adam tests)
SIZE, B, N_TRAIN = 10, 16, 64


def _model(dtype=F32, seed=3):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, DEV, dtype, image_size=SIZE)


def _batches(count, dtype=F32, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        u = torch.rand(1, B, SIZE, SIZE, generator=g)
        x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype).to(DEV)
        out.append((x, torch.randint(0, 10, (B,), generator=g).to(DEV)))
    return out


def _rms(model, **kw):
    from dctn_amd.training import FlatRMSprop

    args = dict(lr=1e-3, weight_decay=1e-3, momentum=0.9, l2=1e-2)
    args.update(kw)
    return FlatRMSprop(list(model.epses) + [model.linear.weight], [model.linear.bias], **args)


def _source(seed=77):
    from dctn_amd.batches import DeviceBatches

    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (N_TRAIN, SIZE, SIZE), dtype=torch.uint8, generator=g)
    return DeviceBatches(images, torch.randint(0, 10, (N_TRAIN,), generator=g), B, dtype=F32, seed=seed, device=DEV)


def test_eager_steps_and_replays_of_a_captured_step_leave_the_same_bits():
    from dctn_amd.training import GraphedTrainStep, StepTrace, fused_cross_entropy, train_step

    batches = _batches(6)
    change = (3, 2.5e-4)   # the rate assigned before that step
    m1 = _model()
    eager = _rms(m1)
    train_step(m1, *batches[0], fused_cross_entropy, eager)   # the graphed run's warm-up iteration
    ends = []
    for i, (x, y) in enumerate(batches):
        if i == change[0]:
            eager.lr = change[1]
        train_step(m1, x, y, fused_cross_entropy, eager)
        ends.append(_owned(eager))
    m2 = _model()
    graphed = _rms(m2)
    trace = StepTrace(DEV)
    step = GraphedTrainStep(m2, batches[0][0], batches[0][1], fused_cross_entropy, graphed, warmup=1, trace=trace)
    for i, (x, y) in enumerate(batches):
        if i == change[0]:
            graphed.lr = change[1]
        step(x, y)
        _assert_same(_owned(graphed), ends[i], f"replay {i}")
    assert graphed.t == 7 and graphed.lr == change[1]
    records = trace.read()
    assert [int(r["opt_steps_done"]) for r in records] == list(range(1, 8))
    assert [float(r["lr"]) for r in records] == [float(np.float32(1e-3))] * 4 + [float(np.float32(change[1]))] * 3
    # the assignment took effect: the same replays without it end elsewhere
    m3 = _model()
    unchanged = _rms(m3)
    step3 = GraphedTrainStep(m3, batches[0][0], batches[0][1], fused_cross_entropy, unchanged, warmup=1)
    for x, y in batches:
        step3(x, y)
    torch.cuda.synchronize()
    assert not _bits(unchanged.flat, graphed.flat)


def test_three_iterations_per_launch_are_three_launches_of_one():
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    ends = []
    for K, launches in ((1, 6), (3, 2)):
        model = _model()
        opt = _rms(model)
        step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=_source(),
                                iters_per_launch=K)
        for _ in range(launches):
            out = step()
        assert out.get("iters", 1) == K and opt.t == 7
        ends.append(_owned(opt))
    _assert_same(ends[1], ends[0], "K = 3 against K = 1")


# ------------------------------------------------------------------ 6. resume
def test_state_dict_resumes_bit_identically():
    from dctn_amd.training import WeightEMA, fused_cross_entropy, train_step

    batches = _batches(8)
    m1 = _model(BF16)
    whole = _rms(m1, master_weights=True, ema=WeightEMA(DEV, 0.9))
    for x, y in batches:
        train_step(m1, x.to(BF16), y, fused_cross_entropy, whole)
    m2 = _model(BF16)
    first = _rms(m2, master_weights=True, ema=WeightEMA(DEV, 0.9))
    for x, y in batches[:4]:
        train_step(m2, x.to(BF16), y, fused_cross_entropy, first)
    state = copy.deepcopy(first.state_dict())
    assert state["t"] == 4 and set(state) == {"t", "lr", "square_avg", "buf", "alpha", "eps", "weight_decay", "momentum",
                                              "l2", "master", "ema"}
    weights = copy.deepcopy(m2.state_dict())
    m3 = _model(BF16, seed=77)
    m3.load_state_dict(weights)
    resumed = _rms(m3, lr=1.0, alpha=0.5, eps=1e-3, weight_decay=0.5, l2=0.25, master_weights=True, ema=WeightEMA(DEV, 0.9))
    resumed.load_state_dict(state)
    assert resumed.t == 4 and resumed.lr == 1e-3 and resumed.alpha == ALPHA
    for x, y in batches[4:]:
        train_step(m3, x.to(BF16), y, fused_cross_entropy, resumed)
    _assert_same(_owned(resumed), _owned(whole), "resumed from state_dict")
    assert _bits(resumed.ema.values, whole.ema.values) and resumed.ema.updates == 8
    with pytest.raises(ValueError, match="momentum"):
        _rms(_model(BF16), momentum=0.0).load_state_dict(state)


def test_a_snapshot_resumes_bit_identically_under_a_captured_graph(tmp_path):
    from dctn_amd import checkpoint as C
    from dctn_amd.training import GraphedTrainStep, LRSchedule, fused_cross_entropy

    def objects(model_seed, source_seed):
        model = _model(seed=model_seed)
        opt = _rms(model, schedule=LRSchedule(DEV, KNOTS))
        src = _source(source_seed)
        run = C.RunState(model, opt, batch_source=src)
        return model, opt, src, run, GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src)

    model, opt, src, run, step = objects(3, 77)
    for _ in range(3):
        step()
    path = run.snapshot({"done": 4}).save(str(tmp_path / "rms.dctn"))
    for _ in range(3):
        step()
    want = _owned(opt)
    model2, opt2, src2, run2, step2 = objects(9, 123)   # another run, already under its own graph
    step2()
    assert run2.load(path) == {"done": 4}
    assert opt2.t == 4 and opt2.lr == opt2.schedule.value(4)
    for _ in range(3):
        step2()
    _assert_same(_owned(opt2), want, "resumed from a snapshot")
    assert opt2.t == 7


# ------------------------------------------------------------------ 7. buffer contract
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_step_touches_nothing_outside_its_buffers(variant, momentum):
    """Every buffer of the optimizer in its own guarded allocation, the guards NaN bytes at the very next byte after the
    n elements: n = 8199 leaves a tail of 3 behind the last vector."""
    from tests.guarded_buffers import guarded

    from dctn_amd.training import WeightEMA

    dtype, master = VARIANTS[variant]
    w0, grads = _problem(N, dtype, 2)
    with guarded(fill=0xFF) as arena:
        opt, store, _ = _make(w0, SIZES, 2, master_weights=master, momentum=momentum, ema=WeightEMA(DEV, 0.9))
        zeros = arena.count["zeros"]
        store = arena.place(store)
        for p, view in zip(opt.params, store.split(SIZES)):
            p.grad = view
        opt.sq_sum.fill_(float("nan"))   # overwritten whatever it held
        for g in grads:
            store.copy_(g)
            opt.step()
    arena.check()
    assert torch.isfinite(opt.sq_sum).all() and opt.t == 2
    for name in ("flat", "square_avg") + (("buf",) if momentum else ()) + (("master",) if master else ()):
        assert torch.isfinite(getattr(opt, name).float()).all(), name
    assert (opt.buf is None) == (momentum == 0.0)
    # momentum 0: one float32 buffer of n elements fewer is asked for
    if momentum == 0.0:
        with guarded(fill=0xFF) as other:
            _make(w0, SIZES, 2, master_weights=master, momentum=0.9, ema=WeightEMA(DEV, 0.9))
        assert other.count["zeros"] == zeros + 1
