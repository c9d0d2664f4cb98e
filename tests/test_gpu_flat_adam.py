"""`FlatAdam` (one HIP launch per Adam step over the flat parameter buffer, step count and learning rate on the device)
and the fused scoring kernel, on the GPU.

The tolerances of the arithmetic checks are yardsticks measured in the same test: the error of torch's own float32
(or bfloat16) result against a float64 reference bounds the error the fused kernels may have against the same
reference.  Every measured figure is printed before it is asserted (run with -s to see them)."""
import copy
import os
import socket

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------ optimizer arithmetic on synthetic gradients
SHAPES_REG, SHAPES_OTHER = [(12001,), (50, 100)], [(2999,), (7,)]   # 12001 * 4 (or * 2) bytes: not a multiple of 16
LR, WD, L2, STEPS = 5e-4, 1e-3, 1e-2, 12


def _synthetic(dtype):
    """Initial weights and STEPS gradients (flat, CPU, float32 values representable in `dtype`); the gradient scale is
    1e-6 / 1 / 30 / exactly 0 by quarter of the flat vector."""
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
        out.append(flat[off : off + k].reshape(s))
        off += k
    return out


def _run_torch_adam(w0, grads, dtype, n_reg):
    """torch.optim.Adam on the CPU in `dtype`, the 2 * l2 * w term of the regularised prefix added by hand.  Returns the
    final flat weights and l2 * sum w^2 over the prefix before the last update (float64)."""
    params = [torch.nn.Parameter(p.clone().to(dtype)) for p in _split(w0, SHAPES_REG + SHAPES_OTHER)]
    opt = torch.optim.Adam(params, lr=LR, weight_decay=WD)
    reg_before_last = None
    for g in grads:
        flat_w = torch.cat([p.detach().reshape(-1) for p in params])
        reg_before_last = L2 * float((flat_w[:n_reg].double() ** 2).sum())
        full = g.to(torch.float64 if dtype == torch.float64 else torch.float32).clone()
        full[:n_reg] += 2 * L2 * flat_w[:n_reg].to(full.dtype)
        for p, gp in zip(params, _split(full.to(dtype), SHAPES_REG + SHAPES_OTHER)):
            p.grad = gp.clone()
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in params]).double(), reg_before_last


@pytest.mark.parametrize("layout", ["separate", "back_to_back_offset"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_flat_adam_matches_torch_adam_within_torchs_own_error(dtype, layout):
    """12 steps on ~20 000 synthetic parameters against torch.optim.Adam in float64 (CPU).  With
    e = |w - w_ref| / |w_ref - w_0|: float32 parameters must satisfy e_flat <= 2 * e_torch32 (a different but equally
    valid float32 evaluation order), bfloat16 parameters e_flat <= 1.5 * e_torch_bf16 (torch keeps bfloat16 moments;
    weight rounding dominates both sides).  `layout`: gradients in separate tensors (gathered by the step) or back to
    back at an odd element offset (read in place, the one-element-per-lane form of the kernel)."""
    from dctn_amd.training import FlatAdam

    n, w0, grads = _synthetic(dtype)
    n_reg = sum(torch.Size(s).numel() for s in SHAPES_REG)
    w_ref, reg_ref = _run_torch_adam(w0, grads, torch.float64, n_reg)
    w_torch, _ = _run_torch_adam(w0, grads, dtype, n_reg)

    params = [torch.nn.Parameter(p.clone().to(dtype).to(DEV)) for p in _split(w0, SHAPES_REG + SHAPES_OTHER)]
    k = len(SHAPES_REG)
    opt = FlatAdam(params[:k], params[k:], lr=LR, weight_decay=WD, l2=L2)
    assert params[1].data_ptr() % 16 != 0   # re-pointed behind the 12001-element parameter
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
    factor = 2.0 if dtype == torch.float32 else 1.5
    print(f"\nFlatAdam {dtype} {layout}: e_flat={e_flat:.4e} e_torch={e_torch:.4e} bound={factor * e_torch:.4e}")
    assert e_flat <= factor * e_torch
    # the regulariser's value as of the last step: l2 * sum w^2 BEFORE that update - of the optimizer's own weights,
    # and (float32: same weights up to rounding) of the float64 reference
    reg = float(opt.reg_value())
    print(f"reg_value={reg:.8e} own weights={own_reg:.8e} float64 reference={reg_ref:.8e}")
    assert abs(reg - own_reg) <= 1e-4 * max(1.0, own_reg)
    if dtype == torch.float32:
        assert abs(reg - reg_ref) <= 1e-4 * max(1.0, reg_ref)


# ------------------------------------------------------------------ step counter and learning rate under replay
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


def _flat_adam(model, **kw):
    from dctn_amd.training import FlatAdam

    args = dict(lr=2e-3, weight_decay=1e-3, l2=1e-2)
    args.update(kw)
    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], **args)


def _snapshot(opt):
    torch.cuda.synchronize()
    return opt.flat.clone(), opt.m.clone(), opt.v.clone(), opt.t


def _same(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


WARMUP = 2


def _run_graphed(batches, lr_change=None):
    """WARMUP eager iterations on the first batch inside GraphedTrainStep, then one replay per batch; `lr_change` =
    (index, value): the rate assigned before that replay.  Returns the snapshots after every replay."""
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    model = _model()
    opt = _flat_adam(model)
    step = GraphedTrainStep(model, batches[0][0], batches[0][1], fused_cross_entropy, opt, warmup=WARMUP)
    snaps = []
    for i, (x, y) in enumerate(batches):
        if lr_change is not None and i == lr_change[0]:
            opt.lr = lr_change[1]
        step(x, y)
        snaps.append(_snapshot(opt))
    return snaps, opt, step


def _run_eager(batches, lr_change=None):
    from dctn_amd.training import fused_cross_entropy, train_step

    model = _model()
    opt = _flat_adam(model)
    for _ in range(WARMUP):
        train_step(model, batches[0][0], batches[0][1], fused_cross_entropy, opt)
    snaps = []
    for i, (x, y) in enumerate(batches):
        if lr_change is not None and i == lr_change[0]:
            opt.lr = lr_change[1]
        train_step(model, x, y, fused_cross_entropy, opt)
        snaps.append(_snapshot(opt))
    return snaps, opt


def test_step_count_advances_under_graph_replay_bit_identically_to_eager():
    batches = _batches(8)
    eager, _ = _run_eager(batches)
    graphed, opt, _ = _run_graphed(batches)
    assert graphed[-1][3] == WARMUP + 8 and opt.t == WARMUP + 8
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert a[3] == b[3] == WARMUP + i + 1
        assert _same(a, b), f"replay {i} differs from the eager step"
    # the bias correction did change from step to step: a frozen t would repeat the first step's scale
    assert not torch.equal(graphed[0][0], graphed[1][0])


def test_lr_assigned_between_replays_is_used_by_the_next_replay(monkeypatch):
    batches = _batches(8)
    eager, _ = _run_eager(batches, lr_change=(4, 5e-4))
    graphed, opt, step = _run_graphed(batches, lr_change=(4, 5e-4))
    unchanged, _, _ = _run_graphed(batches)
    assert opt.lr == 5e-4
    for a, b in zip(eager, graphed):
        assert _same(a, b)
    assert _same(graphed[3], unchanged[3]) and not torch.equal(graphed[4][0], unchanged[4][0])
    # a rate of exactly 0: the replay leaves every parameter as it is, while moments and step count move on
    opt.lr = 0.0
    step(*batches[0])
    after = _snapshot(opt)
    assert torch.equal(after[0], graphed[-1][0]) and not torch.equal(after[1], graphed[-1][1])
    assert after[3] == graphed[-1][3] + 1
    # no assignment while a capture is under way (the write would become a node of somebody's graph)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        opt.lr = 1e-3
    assert opt.lr == 0.0


def test_state_dict_resumes_bit_identically():
    from dctn_amd.training import fused_cross_entropy, train_step

    batches = _batches(8)
    whole, _ = _run_eager(batches)
    model = _model()
    opt = _flat_adam(model)
    for _ in range(WARMUP):
        train_step(model, batches[0][0], batches[0][1], fused_cross_entropy, opt)
    for x, y in batches[:4]:
        train_step(model, x, y, fused_cross_entropy, opt)
    state = copy.deepcopy(opt.state_dict())
    assert state["t"] == WARMUP + 4 and state["lr"] == 2e-3 and set(state) >= {"t", "lr", "m", "v", "betas", "eps",
                                                                              "weight_decay", "l2"}
    weights = copy.deepcopy(model.state_dict())
    fresh = _model(seed=77)
    fresh.load_state_dict(weights)
    opt2 = _flat_adam(fresh, lr=1.0, weight_decay=0.5, l2=0.25, betas=(0.5, 0.5), eps=1e-3)   # all overwritten by the load
    opt2.load_state_dict(state)
    assert opt2.t == WARMUP + 4 and opt2.lr == 2e-3
    for x, y in batches[4:]:
        train_step(fresh, x, y, fused_cross_entropy, opt2)
    assert _same(_snapshot(opt2), whole[-1])


def test_two_runs_from_the_same_seed_are_bit_identical():
    batches = _batches(8)
    first, _, _ = _run_graphed(batches)
    second, _, _ = _run_graphed(batches)
    for a, b in zip(first, second):
        assert _same(a, b)


# ------------------------------------------------------------------ end to end against the reference's recipe
def _rel_err(model, ref_model, w0):
    w = torch.cat([p.detach().double().reshape(-1) for p in model.parameters()])
    r = torch.cat([p.detach().double().reshape(-1) for p in ref_model.parameters()])
    return float((w - r).norm() / (r - w0).norm())


def test_flat_adam_end_to_end_matches_the_reference_recipe():
    """torch.optim.Adam(model.parameters(), lr, weight_decay) + F.cross_entropy + epswise_l2_regularizer through
    autograd (the reference's recipe) against FlatAdam(l2=...) + fused_cross_entropy, 5 float32 iterations, at the
    FlatSGD test's tolerances: 1e-4 on the loss, rtol 2e-4 / atol 2e-6 on the parameters."""
    from dctn_amd.training import fused_cross_entropy, train_step

    lr, wd, l2 = 1e-3, 1e-3, 1e-2
    a = _model()
    b = copy.deepcopy(a)
    c = copy.deepcopy(a).double()
    w0 = torch.cat([p.detach().double().reshape(-1) for p in a.parameters()])
    oa = torch.optim.Adam(a.parameters(), lr=lr, weight_decay=wd)
    oc = torch.optim.Adam(c.parameters(), lr=lr, weight_decay=wd)
    ob = _flat_adam(b, lr=lr, weight_decay=wd, l2=l2)
    reg = lambda m: m.epswise_l2_regularizer()   # noqa: E731
    for x, y in _batches(5, seed=29):
        ra = train_step(a, x, y, F.cross_entropy, oa, reg_fn=reg, reg_coeff=l2)
        train_step(c, x.double(), y, F.cross_entropy, oc, reg_fn=reg, reg_coeff=l2)
        rb = train_step(b, x, y, fused_cross_entropy, ob)
        print(f"\nloss torch={float(ra['loss']):.7f} flat={float(rb['loss'].detach()):.7f} "
              f"reg torch={float(ra['reg_term']) * l2:.7f} flat={float(ob.reg_value()):.7f}")
        assert abs(float(ra["loss"]) - float(rb["loss"].detach())) < 1e-4
        assert abs(float(ra["reg_term"]) * l2 - float(ob.reg_value())) < 1e-4 * max(1.0, float(ra["reg_term"]) * l2)
    worst = max(float(((pa - pb).abs() - 2e-4 * pb.abs()).max().detach()) for pa, pb in zip(a.parameters(), b.parameters()))
    print(f"e_torch32={_rel_err(a, c, w0):.4e} e_flat={_rel_err(b, c, w0):.4e} worst |a-b| - rtol*|b| = {worst:.3e}")
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=2e-4, atol=2e-6)


def test_flat_adam_with_the_epses_composition_regulariser_in_a_graph():
    """The reference recipe's other reg-type on a two-layer spec: the regulariser goes through autograd as `reg_fn`
    (l2 = 0 in the optimizer), the whole iteration is replayed from a graph; against train_step with torch Adam."""
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy, train_step

    lr, wd, coeff = 1e-3, 1e-3, 1e-2
    a = _model(spec=((2, 3), (2, 4)), seed=6)
    b = copy.deepcopy(a)
    c = copy.deepcopy(a).double()
    w0 = torch.cat([p.detach().double().reshape(-1) for p in a.parameters()])
    oa = torch.optim.Adam(a.parameters(), lr=lr, weight_decay=wd)
    oc = torch.optim.Adam(c.parameters(), lr=lr, weight_decay=wd)
    ob = _flat_adam(b, lr=lr, weight_decay=wd, l2=0.0)
    reg = lambda m: m.epses_composition_l2_regularizer()   # noqa: E731
    batches = _batches(6, seed=31)
    step = GraphedTrainStep(b, batches[0][0], batches[0][1], fused_cross_entropy, ob, reg_fn=reg, reg_coeff=coeff, warmup=1)
    train_step(a, batches[0][0], batches[0][1], F.cross_entropy, oa, reg_fn=reg, reg_coeff=coeff)   # the warm-up's twin
    train_step(c, batches[0][0].double(), batches[0][1], F.cross_entropy, oc, reg_fn=reg, reg_coeff=coeff)
    for x, y in batches[1:]:
        ra = train_step(a, x, y, F.cross_entropy, oa, reg_fn=reg, reg_coeff=coeff)
        train_step(c, x.double(), y, F.cross_entropy, oc, reg_fn=reg, reg_coeff=coeff)
        rb = step(x, y)
        print(f"\nloss torch={float(ra['loss']):.7f} flat={float(rb['loss'].detach()):.7f} "
              f"reg torch={float(ra['reg_term']):.7f} flat={float(rb['reg_term'].detach()):.7f}")
        assert abs(float(ra["loss"]) - float(rb["loss"].detach())) < 1e-4
        assert abs(float(ra["reg_term"]) - float(rb["reg_term"].detach())) < 1e-4 * max(1.0, float(ra["reg_term"]))
    torch.cuda.synchronize()
    assert ob.t == 6
    worst = max(float(((pa - pb).abs() - 2e-4 * pb.abs()).max().detach()) for pa, pb in zip(a.parameters(), b.parameters()))
    print(f"e_torch32={_rel_err(a, c, w0):.4e} e_flat={_rel_err(b, c, w0):.4e} worst |a-b| - rtol*|b| = {worst:.3e}")
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=2e-4, atol=2e-6)


# ------------------------------------------------------------------ data parallel: two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    model = _model(torch.bfloat16, seed=5 + rank)   # different seeds on purpose: the broadcast makes them rank 0's
    ddp.broadcast_parameters(model.parameters())
    x, y = _batches(1, torch.bfloat16, seed=17, B=32)[0]
    xs, ys = ddp.shard_batch(x, rank, world), y[rank * 16 : rank * 16 + 16]
    opt = _flat_adam(model)
    red = ddp.FlatGradAllReducer(model.parameters(), average=True)
    step = GraphedTrainStep(model, xs, ys, fused_cross_entropy, opt, reducer=red, warmup=1)
    for _ in range(3):
        step(xs, ys)
    torch.cuda.synchronize(DEV)
    q.put((rank, step.g_opt is not None, opt.t, [p.detach().float().cpu().numpy() for p in model.parameters()]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_flat_adam_in_the_graphed_step_stay_equal():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")   # fresh child processes
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        rank, split, t, arrs = q.get(timeout=300)
        got[rank] = (split, t, [torch.from_numpy(a) for a in arrs])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert got[0][0] and got[1][0]            # forward + backward graph, eager all-reduce, optimizer graph
    assert got[0][1] == got[1][1] == 4        # 1 warm-up + 3 replays of the optimizer graph
    start = [p.detach().float().cpu() for p in _model(torch.bfloat16, seed=5).parameters()]
    for a, b, s in zip(got[0][2], got[1][2], start):
        assert torch.equal(a, b)
        assert not torch.equal(a, s)          # and they did train


# ------------------------------------------------------------------ fused scoring
def _score_case(dtype, B, C, seed=0):
    g = torch.Generator().manual_seed(1000 * B + C + seed)
    logits = (torch.randn(B, C, generator=g) * 3).to(dtype)
    labels = torch.randint(0, C, (B,), generator=g)
    rows = torch.arange(B)
    tie = rows % 5 == 0            # two maxima, the label's index among them: correct only when it is the lower one
    other = (labels + 1) % C
    top = logits.max(dim=1).values
    logits[rows[tie], labels[tie]] = top[tie]
    logits[rows[tie], other[tie]] = top[tie]
    if B > 1:
        labels[rows % 7 == 3] = -100
    return logits.to(DEV), labels.to(DEV)


def _accumulate(logits, labels, acc):
    from dctn_amd import _lib as L

    L.check(L.lib().dctn_ce_score_accumulate(logits.data_ptr(), labels.data_ptr(), acc.data_ptr(), logits.shape[0],
                                             logits.shape[1], L.dtype_code(logits), L.stream_ptr(DEV)), "score")
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("C", [2, 10, 16])
@pytest.mark.parametrize("B", [1, 77, 1024, 10000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_score_accumulate_matches_torch(dtype, B, C):
    """Counts equal torch's exactly (argmax = lowest index among the maxima; rows labelled -100 skipped); the summed
    loss is at most twice as far from F.cross_entropy on float64 logits as F.cross_entropy on float32 logits is."""
    logits, labels = _score_case(dtype, B, C)
    acc = _accumulate(logits, labels, torch.zeros(3, dtype=torch.float64, device=DEV))
    lg = logits.float()
    counted = labels != -100
    want_rows = int(counted.sum())
    want_correct = int(((lg.argmax(dim=1) == labels) & counted).sum())
    ref = float(F.cross_entropy(logits.double(), labels, reduction="sum"))
    e_torch = abs(float(F.cross_entropy(lg, labels, reduction="sum").double()) - ref)
    e_fused = abs(float(acc[0]) - ref)
    print(f"\nscore {dtype} B={B} C={C}: e_fused={e_fused:.3e} e_torch={e_torch:.3e} sum={ref:.6f} "
          f"correct={int(acc[1])}/{want_correct} rows={int(acc[2])}/{want_rows}")
    assert float(acc[1]) == want_correct and float(acc[2]) == want_rows
    assert 0 < want_correct < want_rows or B == 1
    assert e_fused <= 2 * e_torch
    # the same call again from zero: the same bits; a second batch into the same block: the sum of the two
    again = _accumulate(logits, labels, torch.zeros(3, dtype=torch.float64, device=DEV))
    assert torch.equal(acc, again)
    logits2, labels2 = _score_case(dtype, B, C, seed=5)
    alone = _accumulate(logits2, labels2, torch.zeros(3, dtype=torch.float64, device=DEV))
    both = _accumulate(logits2, labels2, acc.clone())
    assert torch.equal(both, acc + alone)


def test_score_accumulate_out_of_range_label_poisons_the_loss():
    logits, labels = _score_case(torch.float32, 77, 10)
    clean = _accumulate(logits, labels, torch.zeros(3, dtype=torch.float64, device=DEV)).clone()
    row = int((labels != -100).nonzero()[1])
    was_correct = bool(logits[row].argmax() == labels[row])
    labels[row] = 10
    acc = _accumulate(logits, labels, torch.zeros(3, dtype=torch.float64, device=DEV))
    assert torch.isnan(acc[0])
    assert float(acc[2]) == float(clean[2]) and float(acc[1]) == float(clean[1]) - (1.0 if was_correct else 0.0)
    labels[row] = -7
    assert torch.isnan(_accumulate(logits, labels, torch.zeros(3, dtype=torch.float64, device=DEV))[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_score_fused_agrees_with_score(dtype):
    from dctn_amd.evaluation import score, score_fused

    model = _model(dtype)
    dl = [(x, y, torch.arange(len(y))) for x, y in _batches(4, dtype, seed=41, B=64)]
    loss_a, acc_a = score(model, dl, DEV)
    loss_b, acc_b = score_fused(model, dl, DEV)
    with torch.no_grad():
        ref = sum(float(F.cross_entropy(model(x).double(), y, reduction="sum")) for x, y, _ in dl) / (4 * 64)
    print(f"\nscore_fused {dtype}: loss score={loss_a!r} fused={loss_b!r} ref={ref!r} accuracy {acc_a} {acc_b}")
    assert acc_a == acc_b
    assert abs(loss_b - ref) <= 2 * abs(loss_a - ref)
    with pytest.raises(RuntimeError):
        score_fused(model, dl, torch.device("cpu"))
