"""The device-side gradient guard on the GPU: `dctn_grad_guard_check` on its own (norm, fixed summation order, stale and
poisoned scratch, non-finite detection, the latch), the guarded `FlatAdam` / `FlatSGD` steps against the unguarded ones
and against torch's `clip_grad_norm_` recipe, and the guard inside `GraphedTrainStep`.  Every measured figure is printed
before it is asserted (run with -s)."""
import os
import socket

import pytest
import torch

from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
INF, NAN = float("inf"), float("nan")
FIELDS = ("max_norm", "last_norm", "halted", "bad_step", "seen", "clipped", "ticket", "coef")


def _bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ 1. the check kernel on its own
def _new_block(max_norm=INF, seen=0):
    host = torch.zeros(8, dtype=torch.int32)
    host.view(torch.float32)[0] = max_norm
    host[3], host[4] = -1, seen
    return host.to(DEV)


def _read(block):
    host = block.cpu()
    f = host.view(torch.float32)
    return {name: (float(f[i]) if i in (0, 1, 7) else int(host[i])) for i, name in enumerate(FIELDS)}


def _launch(g, block, partials, loss=None, n=None):
    from dctn_amd import _lib as L

    rc = L.lib().dctn_grad_guard_check(g.data_ptr(), g.numel() if n is None else n, L.dtype_code(g),
                                       None if loss is None else loss.data_ptr(), partials.data_ptr(), block.data_ptr(),
                                       L.stream_ptr(DEV))
    assert rc == 0, rc


def _num_partials(n):
    from dctn_amd import _lib as L

    return L.lib().dctn_grad_guard_num_partials(n)


def _values(n, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(n, generator=g) * 0.37).to(dtype)


SIZES = [1, 3, 4095, 4096, 4097, 262147, 1048581]   # the last: past 256 * 4096 (the grid-stride loop wraps), n % 4 = 1


OFFSET_SIZES = [3, 4097, 1048581]
NORM_CASES = ([(n, dtype, 0) for n in SIZES for dtype in (torch.float32, BF16)]
              + [(n, dtype, 1) for n in OFFSET_SIZES for dtype in (torch.float32, BF16)])


def _sum_in_kernel_order(partials):
    """Lane j adds slots j, j + 64, ... in that order, then the xor butterfly 32, 16, ..., 1 (float64, on the CPU)."""
    p = partials.cpu()
    lanes = torch.zeros(64, dtype=torch.float64)
    for j in range(p.numel()):
        lanes[j % 64] = lanes[j % 64] + p[j]
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ off]
    return float(lanes[0])


@pytest.mark.parametrize("n, dtype, offset", NORM_CASES)
def test_check_norm_is_exact_to_one_float32_rounding_and_repeats_its_bits(n, dtype, offset):
    """last_norm against g.double().norm(): the float64 accumulation of up to 2^20 terms contributes below 1e-9, the one
    float32 rounding of the result is the bound, a relative 2^-23.  Partials are exactly P doubles full of NaN and the
    block exactly 32 bytes, all inside guarded allocations; a second launch on the same data gives the same bits.
    offset = 1: the gradient pointer one element off, which takes the one-element-per-lane form."""
    host = _values(n + offset, dtype)
    want = float(host[offset:].double().norm())
    P = _num_partials(n)
    assert P == min(256, (n + 4095) // 4096)
    with guarded(0xFF) as arena:
        g = arena.place(host.to(DEV))[offset:]
        partials = arena.empty((P,), torch.float64, DEV)
        block = arena.place(_new_block(max_norm=0.5 * want, seen=6))
        assert partials.numel() * 8 == 8 * P and block.numel() * 4 == 32 and bool(torch.isnan(partials).all())
        assert (g.data_ptr() % (4 * g.element_size()) != 0) == bool(offset)
        _launch(g, block, partials)
        first, first_partials = _read(block), partials.clone()
        _launch(g, block, partials)
        second, second_partials = _read(block), partials.clone()
    arena.check()
    rel = abs(first["last_norm"] - want) / want
    print(f"\nn={n} {dtype} offset={offset}: last_norm={first['last_norm']!r} float64 norm={want!r} rel={rel:.3e} "
          f"bound={2.0 ** -23:.3e} coef={first['coef']!r}")
    assert rel <= 2.0 ** -23
    assert bool(torch.isfinite(first_partials).all()) and _same_bits(first_partials, second_partials)
    assert abs(float(first_partials.sum().sqrt()) - want) <= 1e-9 * want
    assert first["last_norm"] == second["last_norm"] and first["coef"] == second["coef"]
    assert (first["halted"], first["bad_step"], first["seen"], first["clipped"], first["ticket"]) == (0, -1, 7, 1, 0)
    assert (second["halted"], second["bad_step"], second["seen"], second["clipped"], second["ticket"]) == (0, -1, 8, 2, 0)
    from dctn_amd.training import GradGuard

    apply, coef, norm = GradGuard.decide(_sum_in_kernel_order(first_partials), first["max_norm"])
    assert apply and coef == first["coef"] and norm == first["last_norm"] and 0.49 < coef < 0.51


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_check_needs_nothing_of_the_previous_content_of_its_scratch(dtype):
    """Partials and ticket as a previous, LARGER launch left them (256 used slots, the ticket counted up to 256 and reset),
    partials full of NaN, and partials full of large finite values: the same bits as from zeroed scratch."""
    small, large = _values(4097, dtype, seed=1).to(DEV), _values(1048581, dtype, seed=2).to(DEV)
    fresh_block, fresh_partials = _new_block(), torch.zeros(256, dtype=torch.float64, device=DEV)
    _launch(small, fresh_block, fresh_partials)
    want = _read(fresh_block)
    assert want["ticket"] == 0 and want["seen"] == 1
    block, partials = _new_block(), torch.zeros(256, dtype=torch.float64, device=DEV)
    _launch(large, block, partials)
    after_large = _read(block)
    assert after_large["ticket"] == 0 and bool((partials != 0).all())
    _launch(small, block, partials)
    got = _read(block)
    assert got["last_norm"] == want["last_norm"] and got["coef"] == want["coef"] and got["ticket"] == 0 and got["seen"] == 2
    assert _same_bits(partials[:2], fresh_partials[:2])
    assert bool((partials[2:] != 0).all())        # the slots of workgroups that did not run are left alone
    for poison in (NAN, 1e300):
        block, partials = _new_block(), torch.full((2,), poison, dtype=torch.float64, device=DEV)
        _launch(small, block, partials)
        got = _read(block)
        assert got["last_norm"] == want["last_norm"] and got["halted"] == 0 and _same_bits(partials, fresh_partials[:2])


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_check_finds_one_non_finite_value_wherever_it_sits(dtype):
    """One NaN, +inf or -inf at index 0, at n - 1 (n % 4 = 1: the scalar tail), at the first element of the last workgroup
    and at an index only the second trip of the grid-stride loop reaches: the latch is set, coef = 0 and bad_step is the
    value `seen` had at that launch.  The same buffer without the bad value does not halt."""
    n = SIZES[-1]
    positions = {"index 0": 0, "n - 1": n - 1, "first of the last workgroup": 255 * 4096, "second trip only": 256 * 4096 + 1}
    assert n % 4 == 1 and _num_partials(n) == 256 and positions["second trip only"] < (n & ~3)
    g = _values(n, dtype, seed=3).to(DEV)
    partials = torch.empty(256, dtype=torch.float64, device=DEV)
    block = _new_block(seen=11)
    _launch(g, block, partials)
    clean = _read(block)
    assert (clean["halted"], clean["bad_step"], clean["coef"], clean["seen"]) == (0, -1, 1.0, 12)
    for where, index in positions.items():
        for bad in (NAN, INF, -INF):
            keep = g[index].clone()
            g[index] = bad
            block = _new_block(seen=11)
            _launch(g, block, partials)
            got = _read(block)
            g[index] = keep
            assert (got["halted"], got["bad_step"], got["coef"], got["seen"], got["ticket"]) == (1, 11, 0.0, 12, 0), (where, bad, got)
            assert got["last_norm"] != got["last_norm"] or got["last_norm"] == INF, (where, bad, got)
    _launch(g, block := _new_block(seen=11), partials)
    assert _read(block)["halted"] == 0
    # the small sizes too: the only element, and the scalar tail behind one vector access
    for n_small, index in ((1, 0), (4097, 4096), (4097, 0), (3, 2)):
        gs = _values(n_small, dtype, seed=4).to(DEV)
        gs[index] = NAN
        _launch(gs, block := _new_block(seen=2), partials)
        got = _read(block)
        assert (got["halted"], got["bad_step"], got["coef"]) == (1, 2, 0.0), (n_small, index, got)


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_check_does_not_halt_on_large_finite_gradients(dtype):
    """4097 values of 3e19: each square is beyond float32 (9e38 > 3.4e38) but far inside float64, and the norm, 1.9e21, is
    a finite float32 - no halt."""
    g = torch.full((4097,), 3e19, dtype=dtype, device=DEV)
    assert not bool(torch.isfinite(g.float() * g.float()).any())
    block, partials = _new_block(max_norm=1e21), torch.empty(2, dtype=torch.float64, device=DEV)
    _launch(g, block, partials)
    got = _read(block)
    want = float(g.double().norm())
    print(f"\n3e19 x 4097 {dtype}: last_norm={got['last_norm']!r} want={want!r} coef={got['coef']!r}")
    assert got["halted"] == 0 and got["bad_step"] == -1 and abs(got["last_norm"] - want) <= 2.0 ** -23 * want
    assert abs(got["coef"] - 1e21 / want) <= 2.0 ** -22 * (1e21 / want) and got["clipped"] == 1


def test_check_counts_a_non_finite_loss_and_the_latch_persists_until_reset():
    from dctn_amd.training import GradGuard

    g = _values(4097, torch.float32, seed=5).to(DEV)
    with guarded(0xFF) as arena:     # GradGuard's own block and partials come from the arena
        guard = GradGuard(DEV, max_norm=None)
        good, bad = torch.tensor(0.25, device=DEV), torch.tensor(NAN, device=DEV)
        guard.check(g, good)
        state = guard.read()
        assert (state["halted"], state["coef"], state["seen"], state["bad_step"]) == (0, 1.0, 1, -1) and not guard.halted
        guard.check(g, bad)          # finite gradients, NaN loss
        state = guard.read()
        assert (state["halted"], state["coef"], state["seen"], state["bad_step"]) == (1, 0.0, 2, 1) and guard.halted
        assert abs(state["last_norm"] - float(g.double().norm())) <= 2.0 ** -23 * float(g.double().norm())
        guard.check(g, good)         # a clean launch behind it: the latch persists, bad_step keeps the first occasion
        guard.check(g, torch.tensor(-INF, device=DEV))
        state = guard.read()
        assert (state["halted"], state["coef"], state["seen"], state["bad_step"]) == (1, 0.0, 4, 1)
        guard.reset()
        state = guard.read()
        assert (state["halted"], state["bad_step"], state["seen"]) == (0, -1, 4)
        guard.check(g)
        state = guard.read()
        assert (state["halted"], state["coef"], state["seen"], state["bad_step"]) == (0, 1.0, 5, -1)
        saved = guard.state_dict()
        other = GradGuard(DEV, max_norm=3.0)
        other.load_state_dict(saved)
        assert other.read() == saved and other.max_norm == INF
        guard.reset(counters=True)
        assert guard.read()["seen"] == 0
    arena.check()
    with pytest.raises(TypeError):
        guard.check(g, torch.tensor(0.25, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------ 2. the guarded steps
LR, WD, L2 = 5e-4, 1e-3, 1e-2


def _synthetic(n, dtype, steps):
    """Initial weights and `steps` gradients (flat, CPU, float32 values representable in `dtype`); the gradient scale is
    1e-6 / 1 / 30 / exactly 0 by quarter of the flat vector."""
    g = torch.Generator().manual_seed(1234)
    w0 = (torch.randn(n, generator=g) * 0.02).to(dtype).float()
    q = (n + 3) // 4
    scale = torch.cat([torch.full((q,), s) for s in (1e-6, 1.0, 30.0, 0.0)])[:n]
    grads = [(torch.randn(n, generator=g) * scale).to(dtype).float() for _ in range(steps)]
    return w0, grads


def _n_reg(n):
    return n - n // 4 - 1     # a regularised prefix that ends inside a vector access; the rest is "others"


def _optimizer(kind, w0, dtype, master, guard=None, **kw):
    from dctn_amd.training import FlatAdam, FlatSGD

    n_reg = _n_reg(w0.numel())
    params = [torch.nn.Parameter(w0[:n_reg].clone().to(dtype).to(DEV)), torch.nn.Parameter(w0[n_reg:].clone().to(dtype).to(DEV))]
    if kind == "adam":
        opt = FlatAdam(params[:1], params[1:], lr=LR, weight_decay=WD, l2=L2, master_weights=master, guard=guard, **kw)
    else:
        opt = FlatSGD(params[:1], params[1:], lr=LR, momentum=0.9, l2=L2, master_weights=master, guard=guard, **kw)
    return opt, params


def _give(params, g_dev):
    """The gradients back to back in one buffer: the step reads them in place."""
    k = params[0].numel()
    params[0].grad, params[1].grad = g_dev[:k], g_dev[k:]


def _owned(opt):
    """Every buffer the optimizer owns, and its step count."""
    torch.cuda.synchronize()
    bufs = {"flat": opt.flat, "sq_sum": opt.sq_sum}
    if hasattr(opt, "m"):
        bufs.update(m=opt.m, v=opt.v, t=opt._state.clone())
    else:
        bufs.update(buf=opt.buf)
    if opt.master is not None:
        bufs["master"] = opt.master
    return {k: v.clone() for k, v in bufs.items()}


def _assert_same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k], b[k]), f"{what}: {k} differs"


VARIANTS = {"float32": (torch.float32, False), "bf16": (BF16, False), "bf16+master": (BF16, True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("n", [4097, 30011])
def test_unclipped_guarded_steps_are_the_unguarded_steps_bit_for_bit(n, kind, variant):
    from dctn_amd.training import GradGuard

    dtype, master = VARIANTS[variant]
    w0, grads = _synthetic(n, dtype, 5)
    guard = GradGuard(DEV, max_norm=1e6)     # every norm is far below: coef == 1
    plain, plain_params = _optimizer(kind, w0, dtype, master)
    guarded_opt, guarded_params = _optimizer(kind, w0, dtype, master, guard=guard)
    for g in grads:
        g_dev = g.to(dtype).to(DEV)
        _give(plain_params, g_dev)
        _give(guarded_params, g_dev)
        plain.step()
        guarded_opt.step()
        _assert_same_state(_owned(plain), _owned(guarded_opt), f"{kind} {variant} n={n}")
    state = guard.read()
    assert (state["seen"], state["clipped"], state["halted"], state["coef"]) == (5, 0, 0, 1.0)
    if kind == "adam":
        assert guarded_opt.t == plain.t == 5
    assert not torch.equal(guarded_opt.flat.float().cpu(), w0)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("n", [4097, 30011])
def test_clipped_float32_steps_are_the_unguarded_steps_on_g_times_coef(n, kind):
    """The guarded optimizer against the unguarded one fed g * coef, a float32 multiply on the host tensor with the coef
    the guard reports: bit-identical after every step.  coef itself against clip_grad_norm_ on float64 copies of the
    gradients: 2^-22 (the float32 roundings of the norm and of the quotient)."""
    from dctn_amd.training import GradGuard

    w0, grads = _synthetic(n, torch.float32, 5)
    guard = GradGuard(DEV, max_norm=10.0)
    plain, plain_params = _optimizer(kind, w0, torch.float32, False)
    guarded_opt, guarded_params = _optimizer(kind, w0, torch.float32, False, guard=guard)
    for i, g in enumerate(grads):
        _give(guarded_params, g.to(DEV))
        guarded_opt.step()
        coef = guard.read()["coef"]
        p64 = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        p64.grad = g.double()
        torch.nn.utils.clip_grad_norm_([p64], 10.0)
        big = int(g.abs().argmax())
        torch_coef = float(p64.grad[big] / g.double()[big])
        print(f"\n{kind} n={n} step {i}: coef={coef!r} clip_grad_norm_={torch_coef!r} rel={abs(coef - torch_coef) / torch_coef:.3e}")
        assert 0.0 < coef < 0.1 and abs(coef - torch_coef) <= 2.0 ** -22 * torch_coef
        _give(plain_params, (g * torch.tensor(coef, dtype=torch.float32)).to(DEV))   # one rounded float32 product each
        plain.step()
        _assert_same_state(_owned(plain), _owned(guarded_opt), f"{kind} n={n} step {i}")
    assert guard.read()["clipped"] == 5


def _torch_clipped_adam(w0, grads, dtype, n_reg, max_norm):
    """clip_grad_norm_ on the loss gradient, then the 2 * l2 * w term of the regularised prefix by hand, then
    torch.optim.Adam(weight_decay) - on the CPU in `dtype`."""
    p = torch.nn.Parameter(w0.clone().to(dtype))
    opt = torch.optim.Adam([p], lr=LR, weight_decay=WD)
    for g in grads:
        p.grad = g.to(dtype).clone()
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        with torch.no_grad():
            p.grad[:n_reg] += 2 * L2 * p[:n_reg]
        opt.step()
    return p.detach().double()


@pytest.mark.parametrize("n", [4097, 30011])
def test_clipped_bf16_master_steps_match_torchs_recipe_within_torchs_own_error(n):
    """20 steps of bf16 parameters with a float32 master copy against clip_grad_norm_ + torch.optim.Adam in float64, judged
    as test_flat_adam_matches_torch_adam_within_torchs_own_error judges float32: with e = |w - w_ref| / |w_ref - w_0|,
    e_master <= 2 * e_torch32, torch's own float32 run of the same recipe."""
    from dctn_amd.training import GradGuard

    max_norm = 10.0
    w0, grads = _synthetic(n, BF16, 20)
    n_reg = _n_reg(n)
    w_ref = _torch_clipped_adam(w0, grads, torch.float64, n_reg, max_norm)
    w_torch = _torch_clipped_adam(w0, grads, torch.float32, n_reg, max_norm)
    guard = GradGuard(DEV, max_norm=max_norm)
    opt, params = _optimizer("adam", w0, BF16, True, guard=guard)
    for g in grads:
        _give(params, g.to(BF16).to(DEV))
        opt.step()
    assert opt.t == 20 and guard.read()["clipped"] == 20
    moved = float((w_ref - w0.double()).norm())
    e_torch = float((w_torch - w_ref).norm()) / moved
    e_master = float((opt.master.double().cpu() - w_ref).norm()) / moved
    print(f"\nclipped bf16 + master n={n}: e_master={e_master:.4e} e_torch32={e_torch:.4e} bound={2 * e_torch:.4e}")
    assert e_master <= 2.0 * e_torch
    assert _same_bits(opt.flat, opt.master.to(BF16))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("n", [4097, 30011])
def test_a_halted_step_writes_nothing(n, kind, variant):
    """Two good steps, then a gradient with one NaN, then a clean gradient: after the second step every buffer the
    optimizer owns keeps its bits and t does not advance.  The same with finite gradients and a NaN `guard_loss`."""
    from dctn_amd.training import GradGuard

    dtype, master = VARIANTS[variant]
    w0, grads = _synthetic(n, dtype, 4)
    for through_loss in (False, True):
        guard = GradGuard(DEV, max_norm=10.0)
        loss = torch.tensor(0.5, device=DEV)
        opt, params = _optimizer(kind, w0, dtype, master, guard=guard, guard_loss=(lambda: loss) if through_loss else None)
        for g in grads[:2]:
            _give(params, g.to(dtype).to(DEV))
            opt.step()
        before = _owned(opt)
        bad = grads[2].clone()
        if through_loss:
            loss.fill_(NAN)
        else:
            bad[n - 1] = NAN
        _give(params, bad.to(dtype).to(DEV))
        opt.step()
        _assert_same_state(before, _owned(opt), f"{kind} {variant} n={n}: the non-finite step")
        loss.fill_(0.5)
        _give(params, grads[3].to(dtype).to(DEV))
        opt.step()
        _assert_same_state(before, _owned(opt), f"{kind} {variant} n={n}: the clean step behind it")
        state = guard.read()
        assert (state["halted"], state["bad_step"], state["seen"], state["coef"]) == (1, 2, 4, 0.0)
        if kind == "adam":
            assert opt.t == 2
        assert bool(torch.isfinite(opt.flat.float()).all())


@pytest.mark.parametrize("master", [False, True])
def test_flat_sgd_after_a_skipped_step_0_matches_a_run_that_never_saw_it(master):
    """FlatSGD's `first` flag is the host's count of launches.  The skipped step 0 leaves the momentum buffer zero, so the
    next launch, with first = 0, forms momentum * 0 + g = g: the update of a first step."""
    from dctn_amd.training import GradGuard

    n, dtype = 4097, BF16 if master else torch.float32
    w0, grads = _synthetic(n, dtype, 4)
    guard = GradGuard(DEV)
    opt, params = _optimizer("sgd", w0, dtype, master, guard=guard)
    bad = grads[0].clone()
    bad[0] = INF
    _give(params, bad.to(dtype).to(DEV))
    opt.step()
    assert guard.read()["bad_step"] == 0 and torch.equal(opt.buf, torch.zeros_like(opt.buf))
    guard.reset()
    control, control_params = _optimizer("sgd", w0, dtype, master)
    for g in grads[1:]:
        _give(params, g.to(dtype).to(DEV))
        _give(control_params, g.to(dtype).to(DEV))
        opt.step()
        control.step()
    a, b = _owned(opt), _owned(control)
    for k in a:
        assert torch.equal(a[k], b[k]), k      # (values: a zero gradient leaves +0 here and -0 there in `buf`)
    assert _same_bits(a["flat"], b["flat"]) and not torch.equal(opt.flat.float().cpu(), w0.to(dtype).float())


# ------------------------------------------------------------------ 3. inside GraphedTrainStep
WARMUP = 2


def _model(dtype=torch.float32, spec=((3, 4),), seed=3):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(spec, UnitTheoreticalOutputStd(), 1.0, DEV, dtype, image_size=10)


def _batches(count, dtype=torch.float32, seed=11, B=16):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        u = torch.rand(1, B, 10, 10, generator=g)
        x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype).to(DEV)
        out.append((x, torch.randint(0, 10, (B,), generator=g).to(DEV)))
    return out


def _with_nan_pixel(batch):
    x, y = batch
    x = x.clone()
    x[0, 3, 4, 5, 0] = NAN
    return x, y


def _flat_adam(model, **kw):
    from dctn_amd.training import FlatAdam

    args = dict(lr=2e-3, weight_decay=1e-3, l2=1e-2)
    args.update(kw)
    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], **args)


def _snapshot(opt):
    torch.cuda.synchronize()
    return opt.flat.clone(), opt.m.clone(), opt.v.clone(), opt.t


def _same(a, b):
    return all(_same_bits(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


def _graphed(first_batch, max_norm=None):
    """A GraphedTrainStep with a guarded FlatAdam: WARMUP eager iterations on `first_batch`, then the counters are zeroed
    so that `bad_step` counts replays."""
    from dctn_amd.training import GradGuard, GraphedTrainStep, fused_cross_entropy

    model = _model()
    guard = GradGuard(DEV, max_norm=max_norm)
    opt = _flat_adam(model, guard=guard)
    step = GraphedTrainStep(model, first_batch[0], first_batch[1], fused_cross_entropy, opt, warmup=WARMUP)
    assert guard.read()["seen"] == WARMUP           # the eager warm-up iterations; the capture itself runs nothing
    return model, guard, opt, step


def test_graphed_step_halts_at_the_nan_batch_and_resumes_after_reset(tmp_path):
    """Eight batches, batch 4 carries one NaN pixel: the parameters after the run are those after batch 3, bad_step = 4,
    t = 4 + warm-up.  After reset(), batches 5-7 give the parameters of a control run that was never shown batch 4.  The
    device-halt stopper (every = 2) raises the stop flag within two iterations and writes the artefact."""
    from dctn_amd.training import make_stopper_on_device_halt

    batches = _batches(8)
    shown = list(batches)
    shown[4] = _with_nan_pixel(batches[4])
    model, guard, opt, step = _graphed(batches[0])
    guard.reset(counters=True)
    hook = make_stopper_on_device_halt(str(tmp_path), guard, every=2)
    snaps, stopped_at = [], None
    for i, (x, y) in enumerate(shown):
        out = step(x, y)
        snaps.append(_snapshot(opt))
        st_it = dict(num_iters_done=i, stop=False, x=x, y=y, loss=out["loss"], reg_term=out["reg_term"], output=out["output"])
        hook(dict(model=model), st_it)
        if st_it["stop"] and stopped_at is None:
            stopped_at = i
    state = guard.read()
    print(f"\nguard after the run: {state}, stop flag raised at iteration {stopped_at}")
    assert state["halted"] == 1 and state["bad_step"] == 4 and state["seen"] == 8 and state["coef"] == 0.0
    assert opt.t == 4 + WARMUP
    assert not _same(snaps[2], snaps[3])
    for later in snaps[4:]:
        assert _same(later, snaps[3])
    assert bool(torch.isfinite(opt.flat).all()) and bool(torch.isfinite(opt.m).all()) and bool(torch.isfinite(opt.v).all())
    assert stopped_at is not None and 4 <= stopped_at <= 5
    target = tmp_path / "nan_loss_stop"
    names = sorted(os.listdir(target))
    assert "guard.pth" in names and {"x.pth", "y.pth", "output.pth"} <= set(names)
    model_files = [f for f in names if f.startswith("model_nitd=")]
    assert len(model_files) == 1 and "_bad_step=4_" in model_files[0] and "_last_norm=" in model_files[0]
    assert torch.load(target / "guard.pth")["bad_step"] == 4
    saved = torch.load(target / model_files[0])
    for name, value in model.state_dict().items():
        assert torch.equal(saved[name], value)        # the parameters of the last good step, intact
    # on from there
    guard.reset()
    for x, y in batches[5:]:
        step(x, y)
    resumed = _snapshot(opt)
    assert guard.read()["halted"] == 0 and resumed[3] == 7 + WARMUP
    _, control_guard, control_opt, control_step = _graphed(batches[0])
    for x, y in batches[:4] + batches[5:]:
        control_step(x, y)
    assert _same(resumed, _snapshot(control_opt)) and control_guard.read()["halted"] == 0


def test_max_norm_assigned_between_replays_is_used_by_the_next_replay(monkeypatch):
    batches = _batches(8)
    _, guard, opt, step = _graphed(batches[0])
    _, free_guard, free_opt, free_step = _graphed(batches[0])
    guard.reset(counters=True)
    graph = step.g_main
    norms = []
    for i, (x, y) in enumerate(batches):
        if i == 4:
            guard.max_norm = 1e-3
        step(x, y)
        free_step(x, y)
        state = guard.read()
        norms.append(state["last_norm"])
        assert state["clipped"] == max(0, i - 3), (i, state)
        assert (state["coef"] == 1.0) == (i < 4)
        same = _same(_snapshot(opt), _snapshot(free_opt))
        assert same == (i < 4), i
    print(f"\ngradient norms of the eight replays: {norms}")
    assert min(norms) > 1e-3 and step.g_main is graph and step.g_opt is None and guard.max_norm == 1e-3
    guard.max_norm = None
    step(*batches[0])
    assert guard.read()["coef"] == 1.0 and guard.read()["clipped"] == 4
    # no assignment while a capture is under way (the write would become a node of somebody's graph)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        guard.max_norm = 1.0
    with pytest.raises(RuntimeError, match="capture"):
        guard.reset()
    assert guard.max_norm == INF


# ------------------------------------------------------------------ 4. data parallel: two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.training import GradGuard, GraphedTrainStep, fused_cross_entropy

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    model = _model(BF16, seed=5 + rank)   # different seeds on purpose: the broadcast makes them rank 0's
    ddp.broadcast_parameters(model.parameters())
    shards = []
    for i, (x, y) in enumerate(_batches(5, BF16, seed=17, B=32)):
        xs, ys = ddp.shard_batch(x, rank, world).clone(), y[rank * 16: rank * 16 + 16]
        if i == 2 and rank == 1:          # the NaN pixel is in rank 1's shard only
            xs[0, 3, 4, 5, 0] = NAN
        shards.append((xs, ys))
    guard = GradGuard(DEV, max_norm=1.0)
    opt = _flat_adam(model, guard=guard)
    red = ddp.FlatGradAllReducer(model.parameters(), average=True)
    step = GraphedTrainStep(model, shards[0][0], shards[0][1], fused_cross_entropy, opt, reducer=red, warmup=1)
    guard.reset(counters=True)
    before_bad = None
    for i, (xs, ys) in enumerate(shards):
        if i == 2:
            torch.cuda.synchronize(DEV)
            before_bad = opt.flat.float().cpu().numpy()
        step(xs, ys)
    torch.cuda.synchronize(DEV)
    q.put((rank, step.g_opt is not None, opt.t, guard.read(), before_bad, opt.flat.float().cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_latch_at_the_same_step_and_stay_equal():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")   # fresh child processes
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        rank, *rest = q.get(timeout=300)
        got[rank] = rest
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank in (0, 1):
        split, t, state, before_bad, final = got[rank]
        assert split                          # the check sits in the optimizer's graph, behind the eager all-reduce
        assert (state["halted"], state["bad_step"], state["seen"], state["coef"]) == (1, 2, 5, 0.0), (rank, state)
        assert t == 1 + 2                     # the warm-up and the two good replays
        assert (before_bad == final).all()    # nothing moved from the bad batch on
    assert got[0][2] == got[1][2]             # the whole block: the ranks saw the same norms and took the same decisions
    assert (got[0][4] == got[1][4]).all()
    start = torch.cat([p.detach().float().reshape(-1) for p in _flat_adam(_model(BF16, seed=5)).params]).cpu().numpy()
    assert not (got[0][4] == start).all()     # and they did train before it
