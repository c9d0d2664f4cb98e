"""Float32 master weights in `FlatAdam` / `FlatSGD` for bfloat16 parameters (`master_weights=True`), on the GPU.

The step kernel reads and writes a float32 copy of the flat parameter buffer and leaves its round-to-nearest-even in the
bfloat16 parameters, which it never reads.  The element arithmetic is the float32 instantiation's, so the master copy
follows, bit for bit, what the same optimizer does on float32 parameters given the same gradients; that is the
reference of the arithmetic tests here.  Every measured figure is printed before it is asserted (run with -s)."""
import copy
import os

import pytest
import torch

from tests import test_gpu_flat_adam as FA
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = FA.DEV
BF16 = torch.bfloat16


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _is_rounded_master(opt):
    return _same_bits(opt.flat, opt.master.to(BF16))


# ------------------------------------------------------------------ 1. the master trajectory is the float32 optimizer's
def _give_grads(params, g, dtype, layout):
    shapes = FA.SHAPES_REG + FA.SHAPES_OTHER
    if layout == "separate":
        for p, gp in zip(params, FA._split(g.to(dtype).to(DEV), shapes)):
            p.grad = gp.clone()
    else:   # back to back at an odd element offset: read in place by the one-element-per-lane form
        buf = torch.zeros(g.numel() + 1, dtype=dtype, device=DEV)
        buf[1:] = g.to(dtype).to(DEV)
        for p, gp in zip(params, FA._split(buf[1:], shapes)):
            p.grad = gp


def _pair(cls, w0, **kw):
    """(float32 optimizer on float32 parameters, master-weight optimizer on bfloat16 parameters), same start."""
    k = len(FA.SHAPES_REG)
    out = []
    for dtype, master in ((torch.float32, False), (BF16, True)):
        params = [torch.nn.Parameter(p.clone().to(dtype).to(DEV)) for p in FA._split(w0, FA.SHAPES_REG + FA.SHAPES_OTHER)]
        out.append((cls(params[:k], params[k:], master_weights=master, **kw), params))
    return out


@pytest.mark.parametrize("layout", ["separate", "back_to_back_offset"])
def test_adam_master_trajectory_is_the_float32_optimizers_bit_for_bit(layout):
    """The synthetic case of test_gpu_flat_adam.py (~20 000 parameters, 12 steps, gradient scales 1e-6 / 1 / 30 / 0) with
    bf16-representable weights and gradients: FlatAdam on float32 parameters fed the gradients as float32 against
    FlatAdam(master_weights=True) on bfloat16 parameters fed them as bfloat16.  After EVERY step master, m, v, t and
    every sq_sum slot are the same bits and the bfloat16 parameters are the rounded master.  The float32 bound of the
    existing test against float64 Adam (e <= 2 * e_torch32) then holds by construction; asserted as well."""
    from dctn_amd.training import FlatAdam

    n, w0, grads = FA._synthetic(BF16)
    n_reg = sum(torch.Size(s).numel() for s in FA.SHAPES_REG)
    (o32, p32), (om, pm) = _pair(FlatAdam, w0, lr=FA.LR, weight_decay=FA.WD, l2=FA.L2)
    assert o32.master is None and om.master.dtype == torch.float32 and om.master.numel() == n
    assert _same_bits(om.master, o32.flat) and _is_rounded_master(om)   # exact widening of the bfloat16 start
    for step, g in enumerate(grads):
        _give_grads(p32, g, torch.float32, layout)
        _give_grads(pm, g, BF16, layout)
        o32.step()
        om.step()
        torch.cuda.synchronize()
        assert _same_bits(om.master, o32.flat), f"step {step}: master differs from the float32 parameters"
        assert _same_bits(om.m, o32.m) and _same_bits(om.v, o32.v), f"step {step}: moments differ"
        assert _same_bits(om.sq_sum, o32.sq_sum), f"step {step}: sq_sum slots differ"
        assert om.t == o32.t == step + 1
        assert _is_rounded_master(om), f"step {step}: the bfloat16 parameters are not the rounded master"
    assert om.sq_sum.numel() > 1 and float(om.sq_sum.sum()) > 0
    w_ref, _ = FA._run_torch_adam(w0, grads, torch.float64, n_reg)
    w_torch, _ = FA._run_torch_adam(w0, grads, torch.float32, n_reg)
    moved = float((w_ref - w0.double()).norm())
    e_torch = float((w_torch - w_ref).norm()) / moved
    e_master = float((om.master.double().cpu() - w_ref).norm()) / moved
    e_bf16 = float((om.flat.double().cpu() - w_ref).norm()) / moved
    print(f"\nFlatAdam master {layout}: e_master={e_master:.4e} e_torch32={e_torch:.4e} bound={2 * e_torch:.4e} "
          f"(the rounded bfloat16 parameters: {e_bf16:.4e})")
    assert e_master <= 2 * e_torch


@pytest.mark.parametrize("layout", ["separate", "back_to_back_offset"])
def test_sgd_master_trajectory_is_the_float32_optimizers_bit_for_bit(layout):
    """The same for FlatSGD with momentum: master, momentum buffer and sq_sum slots after every step."""
    from dctn_amd.training import FlatSGD

    n, w0, grads = FA._synthetic(BF16)
    (o32, p32), (om, pm) = _pair(FlatSGD, w0, lr=FA.LR, momentum=0.9, l2=FA.L2)
    assert o32.master is None and om.master.dtype == torch.float32 and om.master.numel() == n
    for step, g in enumerate(grads):
        _give_grads(p32, g, torch.float32, layout)
        _give_grads(pm, g, BF16, layout)
        o32.step()
        om.step()
        torch.cuda.synchronize()
        assert _same_bits(om.master, o32.flat), f"step {step}: master differs from the float32 parameters"
        assert _same_bits(om.buf, o32.buf), f"step {step}: momentum buffers differ"
        assert _same_bits(om.sq_sum, o32.sq_sum), f"step {step}: sq_sum slots differ"
        assert _is_rounded_master(om), f"step {step}: the bfloat16 parameters are not the rounded master"
    assert not _same_bits(om.master, w0.to(DEV)) and float(om.buf.abs().sum()) > 0


# ------------------------------------------------------------------ 2. the stall, where it is arithmetic
STALL_CASES = {"A": ([0.75, -0.75, 0.625, 0.875], 1e-3), "B": ([0.046875, -0.046875, 0.0390625, 0.0546875], 1.11e-4)}


@pytest.mark.parametrize("case", sorted(STALL_CASES))
def test_bf16_weights_stall_without_master_weights_and_move_with_them(case):
    """Every value lies inside its binade and an Adam step of `lr` (gradient sign(w), default betas, no decay) is below
    half an ulp of the bfloat16 value (A: 2^-9 = 1.95e-3 > 1e-3; B: 2^-13 = 1.22e-4 > 1.11e-4).  Without master weights
    100 steps leave every bfloat16 value bit-unchanged - today's behaviour, stated as a fact.  With them every value
    moves, the float32 master is within 1e-5 relative of w0 - 100 * lr * sign(w0) and the bfloat16 value is the
    master rounded."""
    from dctn_amd.training import FlatAdam

    values, lr = STALL_CASES[case]
    w0 = torch.tensor(values, dtype=torch.float32)
    assert torch.equal(w0.to(BF16).float(), w0)
    g = torch.sign(w0).to(BF16).to(DEV)
    got = {}
    for master in (False, True):
        p = torch.nn.Parameter(w0.to(BF16).to(DEV))
        opt = FlatAdam([p], lr=lr, master_weights=master)
        for _ in range(100):
            p.grad = g
            opt.step()
        torch.cuda.synchronize()
        assert opt.t == 100
        got[master] = (p.detach().clone(), opt)
    stalled, moving = got[False][0], got[True][0]
    master = got[True][1].master
    want = w0.double() - 100 * lr * torch.sign(w0).double()
    rel = ((master.double().cpu() - want).abs() / want.abs()).max()
    print(f"\ncase {case}: bf16-only {stalled.float().tolist()}  master {master.tolist()}  bf16 of it "
          f"{moving.float().tolist()}  want {want.tolist()}  worst relative distance {float(rel):.3e}")
    assert got[False][1].master is None
    assert _same_bits(stalled, w0.to(BF16).to(DEV)), "a bfloat16-only weight moved: the premise of this test is wrong"
    assert bool((_bits(moving) != _bits(w0.to(BF16).to(DEV))).all()), "a weight did not move under master weights"
    assert float(rel) <= 1e-5
    assert _is_rounded_master(got[True][1])


# ------------------------------------------------------------------ 3. against the recipe the suite hand-rolls
class _NoStep:
    def __init__(self, params):
        self.params = params

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def step(self):
        pass


def _flat(model, master_weights, **kw):
    from dctn_amd.training import FlatAdam

    args = dict(lr=2e-3, weight_decay=1e-3, l2=1e-2)
    args.update(kw)
    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], master_weights=master_weights, **args)


def _flat_values(params):
    return torch.cat([p.detach().double().reshape(-1) for p in params]).cpu()


def test_master_weights_match_the_hand_rolled_mixed_precision_recipe():
    """The bfloat16 loop of test_train_step_end_to_end_loss_goes_down (float32 torch copies of the parameters,
    torch.optim.Adam on them, copy back rounded) against FlatAdam(master_weights=True) from the same initial values: 5
    iterations at the reference's lr = 1.11e-4 on test_gpu_flat_adam's model and batches in bfloat16.  Both sides take
    bfloat16 gradients from the same kernels and differ only as float32 Adam implementations do: the masters are held
    to the tolerances of test_flat_adam_end_to_end_matches_the_reference_recipe (parameters rtol 2e-4 / atol 2e-6,
    loss 1e-4).  With e = |w - w_ref| / |w_ref - w0| against that torch loop, the run WITHOUT master weights must be
    further away than the run with them."""
    from dctn_amd.training import fused_cross_entropy, train_step

    lr = 1.11e-4
    a = FA._model(BF16)
    b = copy.deepcopy(a)
    c = copy.deepcopy(a)
    pa = list(a.epses) + [a.linear.weight, a.linear.bias]          # the order of the flat buffer
    w0 = _flat_values(pa)
    masters = [p.detach().float().clone().requires_grad_(True) for p in pa]
    oa = torch.optim.Adam(masters, lr=lr)
    idle = _NoStep(pa)
    ob = _flat(b, True, lr=lr, weight_decay=0.0, l2=0.0)
    oc = _flat(c, False, lr=lr, weight_decay=0.0, l2=0.0)
    for x, y in FA._batches(5, BF16, seed=29):
        ra = train_step(a, x, y, fused_cross_entropy, idle)
        for m, p in zip(masters, pa):
            m.grad = p.grad.float()
        oa.step()
        with torch.no_grad():
            for m, p in zip(masters, pa):
                p.copy_(m.to(p.dtype))
        rb = train_step(b, x, y, fused_cross_entropy, ob)
        train_step(c, x, y, fused_cross_entropy, oc)
        print(f"\nloss torch recipe={float(ra['loss']):.7f} master weights={float(rb['loss']):.7f}")
        assert abs(float(ra["loss"]) - float(rb["loss"])) < 1e-4
    torch.cuda.synchronize()
    w_ref = _flat_values(masters)
    moved = float((w_ref - w0).norm())
    e_master = float((ob.master.double().cpu() - w_ref).norm()) / moved
    e_plain = float((oc.flat.double().cpu() - w_ref).norm()) / moved
    ref_flat = torch.cat([m.detach().reshape(-1) for m in masters])
    worst = float(((ob.master - ref_flat).abs() - 2e-4 * ref_flat.abs()).max())
    unmoved = float((_bits(oc.flat) == _bits(w0.to(BF16).to(DEV))).float().mean())
    print(f"e_master={e_master:.4e} e_without_master={e_plain:.4e} worst |master - ref| - rtol*|ref| = {worst:.3e} "
          f"bf16-only weights that never moved: {unmoved:.1%}")
    assert torch.allclose(ob.master, ref_flat, rtol=2e-4, atol=2e-6)
    assert _is_rounded_master(ob)
    assert e_plain > e_master


# ------------------------------------------------------------------ 4. replay, resume, refresh
WARMUP = 2


def _snapshot(opt):
    torch.cuda.synchronize()
    return opt.master.clone(), opt.flat.clone(), opt.m.clone(), opt.v.clone(), opt.t


def _same(a, b):
    return all(_same_bits(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


def _run(batches, graphed, lr_change=None):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy, train_step

    model = FA._model(BF16)
    opt = _flat(model, True)
    if graphed:
        step = GraphedTrainStep(model, batches[0][0], batches[0][1], fused_cross_entropy, opt, warmup=WARMUP)
    else:
        for _ in range(WARMUP):
            train_step(model, batches[0][0], batches[0][1], fused_cross_entropy, opt)
        step = lambda x, y: train_step(model, x, y, fused_cross_entropy, opt)   # noqa: E731
    snaps = []
    for i, (x, y) in enumerate(batches):
        if lr_change is not None and i == lr_change[0]:
            opt.lr = lr_change[1]
        step(x, y)
        snaps.append(_snapshot(opt))
    return snaps, opt, model


def test_graph_replays_equal_eager_steps_and_follow_an_assigned_lr():
    batches = FA._batches(8, BF16)
    eager, _, _ = _run(batches, False, lr_change=(4, 5e-4))
    graphed, opt, _ = _run(batches, True, lr_change=(4, 5e-4))
    unchanged, _, _ = _run(batches, True)
    assert opt.lr == 5e-4 and opt.t == WARMUP + 8
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert a[4] == b[4] == WARMUP + i + 1
        assert _same(a, b), f"replay {i} differs from the eager step"
        assert _same_bits(b[1], b[0].to(BF16))
    assert _same(graphed[3], unchanged[3]) and not _same_bits(graphed[4][0], unchanged[4][0])
    assert not _same_bits(graphed[0][0], graphed[1][0])


def test_state_dict_carries_the_master_copy_and_resumes_bit_identically():
    from dctn_amd.training import fused_cross_entropy, train_step

    batches = FA._batches(8, BF16)
    whole, _, _ = _run(batches, False)
    half, opt, model = _run(batches[:4], False)
    state = copy.deepcopy(opt.state_dict())
    assert state["t"] == WARMUP + 4 and _same_bits(state["master"], opt.master)
    assert state["master"].data_ptr() != opt.master.data_ptr()
    weights = copy.deepcopy(model.state_dict())
    fresh = FA._model(BF16, seed=77)
    fresh.load_state_dict(weights)
    opt2 = _flat(fresh, True, lr=1.0, weight_decay=0.5, l2=0.25, betas=(0.5, 0.5), eps=1e-3)   # all overwritten by the load
    opt2.load_state_dict(state)
    assert opt2.t == WARMUP + 4 and _same_bits(opt2.master, state["master"])
    for x, y in batches[4:]:
        train_step(fresh, x, y, fused_cross_entropy, opt2)
    assert _same(_snapshot(opt2), whole[-1])
    # the master copy holds more than the bfloat16 parameters do: a resume without it is a different run
    assert not _same_bits(state["master"], state["master"].to(BF16).float())

    # a state without `master` (a run without the option): rebuilt from the parameters
    other = FA._model(BF16, seed=78)
    opt3 = _flat(other, True)                      # its master copy: seed 78's values
    other.load_state_dict(weights)                 # behind the optimizer's back
    assert not _same_bits(opt3.master, opt3.flat.float())
    opt3.load_state_dict({k: v for k, v in state.items() if k != "master"})
    assert _same_bits(opt3.master, opt3.flat.float()) and opt3.t == WARMUP + 4
    # and a state WITH one loaded into an optimizer without the option is simply not used
    plain = _flat(FA._model(BF16, seed=79), False)
    plain.load_state_dict(state)
    assert plain.master is None and "master" not in plain.state_dict()


def test_refresh_master_after_the_parameters_were_loaded_from_outside():
    from dctn_amd.training import fused_cross_entropy, train_step

    (x, y), = FA._batches(1, BF16)
    other = copy.deepcopy(FA._model(BF16, seed=21).state_dict())

    def one_step(refresh, load_after_construction):
        model = FA._model(BF16, seed=20)
        if not load_after_construction:
            model.load_state_dict(other)
        opt = _flat(model, True)
        if load_after_construction:
            model.load_state_dict(other)
            if refresh:
                opt.refresh_master()
                assert _same_bits(opt.master, opt.flat.float())
        train_step(model, x, y, fused_cross_entropy, opt)
        return _snapshot(opt)

    want = one_step(False, False)                  # built on `other` from the start
    assert _same(one_step(True, True), want)
    stale = one_step(False, True)                  # the step ran on seed 20's master and overwrote what was loaded
    assert not _same_bits(stale[0], want[0]) and not _same_bits(stale[1], want[1])


def test_sgd_state_dict_resumes_bit_identically_and_float32_is_untouched():
    from dctn_amd.training import FlatAdam, FlatSGD, fused_cross_entropy, train_step

    batches = FA._batches(6, BF16)

    def sgd(model):
        return FlatSGD(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-3, momentum=0.9, l2=1e-2,
                       master_weights=True)

    def snap(opt):
        torch.cuda.synchronize()
        return opt.master.clone(), opt.flat.clone(), opt.buf.clone()

    model = FA._model(BF16)
    opt = sgd(model)
    for x, y in batches[:3]:
        train_step(model, x, y, fused_cross_entropy, opt)
    state, weights = copy.deepcopy(opt.state_dict()), copy.deepcopy(model.state_dict())
    assert state["steps"] == 3 and set(state) >= {"steps", "lr", "momentum", "l2", "buf", "master"}
    for x, y in batches[3:]:
        train_step(model, x, y, fused_cross_entropy, opt)
    fresh = FA._model(BF16, seed=77)
    fresh.load_state_dict(weights)
    opt2 = FlatSGD(list(fresh.epses) + [fresh.linear.weight], [fresh.linear.bias], lr=1.0, momentum=0.1, l2=0.5,
                   master_weights=True)
    opt2.load_state_dict(state)
    for x, y in batches[3:]:
        train_step(fresh, x, y, fused_cross_entropy, opt2)
    assert _same(snap(opt2), snap(opt))
    assert _same_bits(opt.flat, opt.master.to(BF16)) and not _same_bits(opt.master, opt.flat.float())
    # float32 parameters: the option changes nothing
    for cls in (FlatAdam, FlatSGD):
        m32 = FA._model(torch.float32)
        o = cls(list(m32.epses) + [m32.linear.weight], [m32.linear.bias], master_weights=True)
        assert o.master is None and "master" not in o.state_dict()
        o.refresh_master()


# ------------------------------------------------------------------ 5. two ranks on one GPU through train()
def _train_worker(rank, world, port, q, refresh):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy, make_stopper_after_n_iters, train

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    model = FA._model(BF16, seed=5 + rank)          # different seeds on purpose: train() broadcasts rank 0's
    opt = _flat(model, True)                        # built BEFORE train(), as train() expects
    if not refresh:
        opt.refresh_master = None                   # what train() did before it knew of master copies
    x, y = FA._batches(1, BF16, seed=17, B=32)[0]
    xs, ys = ddp.shard_batch(x, rank, world), y[rank * 16: rank * 16 + 16]
    dl = [(xs, ys, torch.arange(16))]
    zero = torch.zeros((), device=DEV)
    train(dl, model, opt, DEV, fused_cross_entropy, lambda st_x, st_it: zero, 0.0, [], [],
          [make_stopper_after_n_iters(2)])
    torch.cuda.synchronize(DEV)
    result = [rank, opt.t, opt.master.cpu().numpy(), opt.flat.float().cpu().numpy()]
    if refresh:   # and on from there in the split form: forward + backward graph, eager all-reduce, optimizer graph
        red = ddp.FlatGradAllReducer(model.parameters(), average=True)
        step = GraphedTrainStep(model, xs, ys, fused_cross_entropy, opt, reducer=red, warmup=1)
        for _ in range(3):
            step(xs, ys)
        torch.cuda.synchronize(DEV)
        result += [step.g_opt is not None, opt.t, opt.master.cpu().numpy(), opt.flat.float().cpu().numpy()]
    q.put(tuple(result))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(refresh):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")   # fresh child processes
    q = ctx.Queue()
    port = FA._free_port()
    procs = [ctx.Process(target=_train_worker, args=(r, 2, port, q, refresh)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        rank, *rest = q.get(timeout=300)
        got[rank] = tuple(torch.from_numpy(v) if hasattr(v, "shape") else v for v in rest)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return got


def test_two_ranks_through_train_keep_equal_masters_and_parameters():
    """The ranks build models from different seeds and their optimizers before train(), which then broadcasts rank 0's
    model: train() must refresh the master copies after that broadcast.  Three iterations later masters and parameters
    are equal across the ranks, and stay so through the split form of GraphedTrainStep; with the refresh taken away
    (the second run) they are not."""
    got = _two_ranks(True)
    assert got[0][0] == got[1][0] == 3
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])
    start = torch.cat([p.detach().float().reshape(-1) for p in _flat(FA._model(BF16, seed=5), True).params]).cpu()
    assert not torch.equal(got[0][2], start)                      # and they did train
    assert torch.equal(got[0][2], got[0][1].to(BF16).float())
    # the same optimizer captured in the split form of GraphedTrainStep: 1 warm-up + 3 replays of the optimizer graph
    assert got[0][3] and got[1][3] and got[0][4] == got[1][4] == 7
    assert torch.equal(got[0][5], got[1][5]) and torch.equal(got[0][6], got[1][6])
    assert torch.equal(got[0][6], got[0][5].to(BF16).float()) and not torch.equal(got[0][5], got[0][1])
    without = _two_ranks(False)
    assert not torch.equal(without[0][1], without[1][1]) and not torch.equal(without[0][2], without[1][2])


# ------------------------------------------------------------------ 6. buffer contract
N_ARENA, N_REG_ARENA = 9001, 6000     # three Adam workgroups, 36 SGD ones; 9001 = 4 * 2250 + 1: a tail after the vector form


def _arena_inputs():
    g = torch.Generator().manual_seed(99)
    w = (torch.randn(N_ARENA, generator=g) * 0.05).to(BF16).float()
    grads = [(torch.randn(N_ARENA + 1, generator=g) * 0.1).to(BF16) for _ in range(2)]
    return w.to(DEV), [t.to(DEV) for t in grads]


def _entry_points_under(fill):
    """Two steps of each entry point with every buffer inside a guarded allocation: step one reads the gradients at an
    aligned address (four elements per lane + tail), step two one element further (one per lane).  `params` goes in
    full of NaN; sq_sum comes poisoned with `fill`; moments, momentum and the state block are zeroed (they are read)."""
    from dctn_amd import _lib as L

    lib = L.lib()
    w, grads = _arena_inputs()
    out = {}
    with guarded(fill) as arena:
        for kind in ("adam", "sgd"):
            master = arena.place(w)
            params = arena.place(torch.full((N_ARENA,), float("nan"), dtype=BF16, device=DEV))
            placed = [arena.place(t) for t in grads]
            bufs = [arena.zeros((N_ARENA,), torch.float32, DEV) for _ in range(2 if kind == "adam" else 1)]
            parts = lib.dctn_adam_l2_num_partials(N_ARENA) if kind == "adam" else lib.dctn_sgd_l2_num_partials(N_ARENA)
            sq_sum = arena.empty((parts,), torch.float32, DEV)
            state = arena.zeros((4,), torch.int32, DEV)
            state.view(torch.float32)[1] = 1e-3
            for step, offset in enumerate((0, 1)):
                gp = placed[step].data_ptr() + 2 * offset
                if kind == "adam":
                    rc = lib.dctn_adam_l2_step_master(master.data_ptr(), params.data_ptr(), gp, bufs[0].data_ptr(),
                                                      bufs[1].data_ptr(), sq_sum.data_ptr(), state.data_ptr(), N_ARENA,
                                                      N_REG_ARENA, 0.9, 0.999, 1e-8, 1e-3, 1e-2, L.stream_ptr(DEV))
                else:
                    rc = lib.dctn_sgd_l2_step_master(master.data_ptr(), params.data_ptr(), gp, bufs[0].data_ptr(),
                                                     sq_sum.data_ptr(), N_ARENA, N_REG_ARENA, 1e-3, 0.9, 1e-2,
                                                     1 if step == 0 else 0, L.stream_ptr(DEV))
                assert rc == 0, (kind, step, rc)
                if step == 0:
                    torch.cuda.synchronize()
                    assert bool(torch.isfinite(params.float()).all()), f"{kind}: params was read, or not fully written"
            torch.cuda.synchronize()
            out[kind] = [t.clone() for t in (master, params, *bufs, sq_sum)] + ([state[0].clone()] if kind == "adam" else [])
    arena.check()
    return out


def test_master_entry_points_keep_their_buffer_contract_under_every_fill():
    """Nothing outside the buffers is touched, `params` full of NaN comes back fully defined (it is never read), the
    poisoned sq_sum is overwritten, and the results are the bits of the zero-filled run under every fill."""
    runs = {fill: _entry_points_under(fill) for fill in (0x00, 0xFF, 0x7B)}
    for kind in ("adam", "sgd"):
        master, params, *rest = runs[0x00][kind]
        assert bool(torch.isfinite(master).all()) and _same_bits(params, master.to(BF16))
        assert all(bool(torch.isfinite(t.float()).all()) for t in rest)
        w, _ = _arena_inputs()
        assert not _same_bits(master, w)
        for fill in (0xFF, 0x7B):
            for a, b in zip(runs[fill][kind], runs[0x00][kind]):
                assert _same_bits(a, b), f"{kind}: fill 0x{fill:02X} changed a result"
    assert int(runs[0x00]["adam"][-1]) == 2
