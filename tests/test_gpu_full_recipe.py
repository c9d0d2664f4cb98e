"""The whole graphed training recipe on the GPU (`-m gpu`) against tests/recipe_reference.py.

Every test builds the same step, "the full step": ONE graph that draws its batch (`DeviceBatches`), masks the cores (fused
component dropout), runs forward, loss, regulariser and backward and steps `FlatAdam` (on float32 master weights in the
bfloat16 runs).  Three device counters advance inside it - Adam's t, dropout's draws_done, the source's batches_done - and
its warm-up iteration is a real step.  37 samples in batches of 8 are 4 batches an epoch, so the 7 iterations of a run
(1 warm-up + 6 replays) cross an epoch boundary and its dropped remainder inside the graph.

  a. the float32 trajectory against the float64 reference, judged by the reference's own float32 run;
  b. bfloat16 with master weights: the one graph equals the pieces driven by hand, bit for bit;
  c. a run resumed after iteration 3 through fresh objects and a new graph continues bit-identically;
  d. scoring between two replays leaves the training counters alone;
  e. two ranks draw equal masks and disjoint shards and stay equal - in the graphed step and in `training.train`.

`GraphedTrainStep` returns nothing from its warm-up, and after the capture `model.dropout_record` is the graph's own
buffer, which the first replay fills: the loss, the logits and the draw record of a warm-up iteration are not seen.
Everything else (parameters, Adam state, sample numbers) is compared after every iteration, the warm-up included.
Every measured figure is printed before it is asserted (run with -s)."""
import copy
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dctn_amd import batches
from dctn_amd import dropout as D
from oracle import ref_cpu as R
from tests import recipe_reference as RR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
N_IT = RR.ITERATIONS
MODES = {"f32": (torch.float32, False), "bf16_master": (BF16, True)}


# ------------------------------------------------------------------ the objects and the full step
def _params(model):
    return list(model.epses) + [model.linear.weight, model.linear.bias]


def _model(case, dtype, seed=None):
    """The case's model on the device: with `seed` None the very numbers the reference starts from, otherwise some other
    model (a resumed run's fresh objects, rank 1)."""
    model = RR.initial_model(case, dtype, DEV, seed)
    if seed is None:
        with torch.no_grad():
            for p, value in zip(_params(model), RR.initial_parameters(case, dtype)):
                p.copy_(value)
    return model


def _source(case, dtype, seed=None, **kw):
    from dctn_amd.batches import DeviceBatches

    images, labels = RR.make_data(case)
    return DeviceBatches(images, labels, RR.GLOBAL_BATCH, dtype=dtype, seed=case.batch_seed if seed is None else seed,
                         scale=case.scale, **kw)


def _objects(case, mode, model_seed=None, dropout_seed=None, batch_seed=None, rank=None, world=None):
    from dctn_amd.training import FlatAdam

    dtype, master = MODES[mode]
    model = _model(case, dtype, model_seed)
    model.use_fused_dropout(case.dropout_seed if dropout_seed is None else dropout_seed)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=case.lr,
                   weight_decay=case.weight_decay, l2=case.reg_coeff if case.reg == "epswise" else 0.0,
                   master_weights=master)
    return model, opt, _source(case, dtype, batch_seed, rank=rank, world=world)


def _composition(model):
    return model.epses_composition_l2_regularizer()


def _full_step(case, model, opt, src, reducer=None):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    through_autograd = case.reg == "composition"
    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, reg_fn=_composition if through_autograd else None,
                            reg_coeff=case.reg_coeff if through_autograd else 0.0, reducer=reducer, warmup=1,
                            batch_source=src)


STATE_KEYS = ("flat", "master", "m", "v", "indices")


def _snap(model, opt, indices, out=None):
    """Clones of everything the tests compare; `out`: what a replay (or `train_step`) returned."""
    torch.cuda.synchronize()
    snap = dict(flat=opt.flat.clone(), master=None if opt.master is None else opt.master.clone(), m=opt.m.clone(),
                v=opt.v.clone(), indices=indices.clone())
    snap["record"] = None if out is None else model.dropout_record.clone()
    snap["loss"] = None if out is None else out["loss"].detach().clone()
    snap["logits"] = None if out is None else out["output"].detach().clone()
    return snap


def _assert_same(got, want, what):
    for key in STATE_KEYS:
        if want[key] is None:
            assert got[key] is None, f"{what}: {key}"
        else:
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), f"{what}: {key} differs"
    for key in ("loss", "logits", "record"):   # a warm-up shows none of them
        if got[key] is not None and want[key] is not None:
            assert torch.equal(got[key], want[key]), f"{what}: {key} differs"


def _counters(model, opt, src):
    return opt.t, model.dropout_state_dict()["draws_done"], src.state_dict()["batches_done"]


@functools.lru_cache(maxsize=None)
def _uninterrupted(name, mode):
    """The 7 iterations of the full step: one snapshot per iteration, and the three counters at the end.  Computed once
    per (case, mode) and shared; nobody writes into it."""
    case = RR.CASES[name]
    model, opt, src = _objects(case, mode)
    step = _full_step(case, model, opt, src)
    snaps = [_snap(model, opt, step.indices)]
    for _ in range(1, N_IT):
        out = step()
        snaps.append(_snap(model, opt, out["indices"], out))
    return snaps, _counters(model, opt, src)


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    case = RR.CASES[name]
    if kind == "f64":                  # the reference of the float32 runs
        return RR.run_case(case, torch.float64)
    if kind == "f32":                  # its float32 twin: the yardstick
        return RR.run_case(case, torch.float32)
    if kind == "f64_from_bf16":        # the reference of the bfloat16 runs: the same recipe from the bfloat16 start
        return RR.run_case(case, torch.float64, params_dtype=BF16)
    if kind == "bf16_master":          # bfloat16 parameters, float32 masters, torch Adam - all in torch on the CPU
        return RR.run_case(case, BF16, master_dtype=torch.float32)
    raise ValueError(kind)


def _trajectory_bound(label, w_hip, losses_hip, ref64, ref32, w0, upto, loss_ks):
    """The bound of (a): with e = |w - w64| / |w64 - w0| after iteration `upto`, e_hip <= 4 e_torch32; and over the
    iterations `loss_ks` max |loss_hip - loss64| <= 4 max |loss_torch32 - loss64|, with a floor of one float32 ulp of the
    loss.  The factor allows for summation order: both are float32 runs of the same arithmetic, and Adam's g / sqrt(v)
    amplifies their rounding equally but not identically."""
    e_hip = RR.rel_err(w_hip, ref64[upto - 1]["params"], w0)
    e_torch = RR.rel_err(ref32[upto - 1]["params"], ref64[upto - 1]["params"], w0)
    d_hip = max(abs(losses_hip[k] - ref64[k]["loss"]) for k in loss_ks)
    d_torch = max(abs(ref32[k]["loss"] - ref64[k]["loss"]) for k in loss_ks)
    ulp = float(np.spacing(np.float32(max(ref64[k]["loss"] for k in loss_ks))))
    print(f"\n{label}: e_hip={e_hip:.4e} e_torch32={e_torch:.4e} (bound {4 * e_torch:.4e}); loss: hip {d_hip:.4e} "
          f"torch32 {d_torch:.4e} (bound {max(4 * d_torch, ulp):.4e}, ulp {ulp:.2e})")
    assert e_hip <= 4 * e_torch
    assert d_hip <= max(4 * d_torch, ulp)


# ------------------------------------------------------------------ a. float32 against the float64 reference
@pytest.mark.parametrize("name", list(RR.CASES))
def test_float32_trajectory_against_the_float64_reference(name):
    """Measured on an MI355X - cfg2: e_hip = 3.956e-07, e_torch32 = 3.978e-07; two_layer: e_hip = 1.297e-06,
    e_torch32 = 1.286e-06 ("Whole recipe")."""
    case = RR.CASES[name]
    snaps, counters = _uninterrupted(name, "f32")
    ref64, ref32 = _reference(name, "f64"), _reference(name, "f32")
    for k, snap in enumerate(snaps):
        want = batches.expected_indices(case.batch_seed, k, RR.N_SAMPLES, RR.GLOBAL_BATCH)
        assert snap["indices"].tolist() == want == ref64[k]["indices"]
        if k > 0:
            assert D.read_state(snap["record"]) == {"seed": case.dropout_seed, "draws_done": k}
    assert counters == (N_IT, N_IT, N_IT)
    assert sorted(snaps[4]["indices"].tolist()) != sorted(snaps[0]["indices"].tolist())   # a new epoch, a new order
    losses = {k: float(snaps[k]["loss"]) for k in range(1, N_IT)}
    _trajectory_bound(f"{name} float32, 7 iterations", [snaps[-1]["flat"]], losses, ref64, ref32,
                      RR.initial_parameters(case, torch.float32), N_IT, range(1, N_IT))


# ------------------------------------------------------------------ b. bf16 + master weights: the graph equals the pieces
def test_bf16_master_weight_graph_equals_the_pieces_driven_by_hand_bit_for_bit():
    """Measured on an MI355X: e of the master copy against the float64 reference 2.070e-02, of the hand-rolled torch
    recipe (bfloat16 parameters and arithmetic, float32 masters, torch Adam) 2.658e-02."""
    from dctn_amd.training import fused_cross_entropy, train_step

    case = RR.CASES["cfg2"]
    snaps, counters = _uninterrupted("cfg2", "bf16_master")
    model, opt, hand_src = _objects(case, "bf16_master")
    for k in range(N_IT):
        x, y, ind = hand_src.gather(torch.tensor(hand_src.expected_indices(k), device=DEV))
        out = train_step(model, x, y, fused_cross_entropy, opt)
        _assert_same(_snap(model, opt, ind, out), snaps[k], f"iteration {k + 1}")
        assert torch.equal(opt.flat, opt.master.to(BF16)) and torch.equal(snaps[k]["flat"], snaps[k]["master"].to(BF16))
        assert snaps[k]["flat"].dtype == BF16 and snaps[k]["master"].dtype == torch.float32
    assert counters == (N_IT, N_IT, N_IT) == (opt.t, model.dropout_state_dict()["draws_done"], N_IT)
    assert hand_src.state_dict()["batches_done"] == 0   # gather reads no state
    assert not torch.equal(snaps[0]["master"], snaps[1]["master"])
    ref64, hand = _reference("cfg2", "f64_from_bf16"), _reference("cfg2", "bf16_master")
    w0 = RR.initial_parameters(case, BF16)
    e_hip = RR.rel_err([snaps[-1]["master"]], ref64[-1]["params"], w0)
    e_torch = RR.rel_err(hand[-1]["masters"], ref64[-1]["params"], w0)
    print(f"\ncfg2 bf16 + master weights, 7 iterations: e_hip={e_hip:.4e} e_torch_bf16_recipe={e_torch:.4e}")
    assert e_hip <= e_torch


# ------------------------------------------------------------------ c. resume
@pytest.mark.parametrize("name,mode", [("two_layer", "f32"), ("cfg2", "bf16_master")])
def test_a_resumed_run_continues_bit_identically_through_a_new_graph(name, mode):
    case = RR.CASES[name]
    whole, _ = _uninterrupted(name, mode)
    model, opt, src = _objects(case, mode)
    step = _full_step(case, model, opt, src)
    step()
    out = step()
    _assert_same(_snap(model, opt, out["indices"], out), whole[2], "iteration 3 of the run that stops")
    saved = copy.deepcopy(dict(model=model.state_dict(), opt=opt.state_dict(), dropout=model.dropout_state_dict(),
                               src=src.state_dict()))
    assert saved["opt"]["t"] == saved["dropout"]["draws_done"] == saved["src"]["batches_done"] == 3
    assert ("master" in saved["opt"]) == MODES[mode][1]
    del step, model, opt, src
    # fresh objects that share nothing with the saved run but the data
    model, opt, src = _objects(case, mode, model_seed=case.model_seed + 1, dropout_seed=99, batch_seed=77)
    assert not torch.equal(opt.flat, whole[2]["flat"])
    model.load_state_dict(saved["model"])   # first the parameters (written behind the optimizer's back) ...
    opt.load_state_dict(saved["opt"])       # ... then the optimizer, whose state carries the master copy
    model.load_dropout_state_dict(saved["dropout"])
    src.load_state_dict(saved["src"])
    step = _full_step(case, model, opt, src)   # its warm-up is iteration 4
    _assert_same(_snap(model, opt, step.indices), whole[3], "iteration 4 (the new graph's warm-up)")
    for k in range(4, N_IT):
        out = step()
        _assert_same(_snap(model, opt, out["indices"], out), whole[k], f"iteration {k + 1} after the resume")
        assert out["indices"].tolist() == src.expected_indices(k)
    assert _counters(model, opt, src) == (N_IT, N_IT, N_IT)
    assert src.state_dict()["seed"] == case.batch_seed and model.dropout_state_dict()["seed"] == case.dropout_seed


# ------------------------------------------------------------------ d. scoring between replays
def test_scoring_between_replays_leaves_the_training_counters_alone():
    from dctn_amd.evaluation import score, score_fused

    case = RR.CASES["cfg2"]
    whole, _ = _uninterrupted("cfg2", "bf16_master")
    model, opt, src = _objects(case, "bf16_master")
    step = _full_step(case, model, opt, src)
    for _ in range(3):
        out = step()
    _assert_same(_snap(model, opt, out["indices"], out), whole[3], "iteration 4")
    sequential = _source(case, BF16, shuffle=False, drop_last=False)
    before = (model.dropout_state_dict(), src.state_dict(), opt.t)
    model.eval()
    loss_fused, acc_fused = score_fused(model, sequential, DEV)
    loss_torch, acc_torch = score(model, sequential, DEV)
    assert (model.dropout_state_dict(), src.state_dict(), opt.t) == before
    assert before == ({"seed": case.dropout_seed, "draws_done": 4}, {"seed": case.batch_seed, "batches_done": 4}, 4)
    # the float64 oracle on the unmasked parameters of this moment and the inputs the model saw
    *cores, weight, bias = [p.detach().cpu().double() for p in _params(model)]
    sum_ce, sure, maybe, rows = 0.0, 0, 0, 0
    with torch.no_grad():
        for x, y, _ in sequential:
            want = R.eps_plus_linear_forward(cores, weight, bias, x.cpu().double())
            y = y.cpu()
            sum_ce += float(F.cross_entropy(want, y, reduction="sum"))
            # a row is free of ties when the oracle's best class leads by more than twice the model's error on that row
            err = (model(x).cpu().double() - want).abs().max(dim=1).values
            top = want.max(dim=1).values
            near = want >= (top - 2 * err).unsqueeze(1)                 # the classes an argmax within `err` may pick
            labelled = near.gather(1, y.unsqueeze(1)).squeeze(1)
            alone = near.sum(dim=1) == 1
            sure += int((labelled & alone).sum())
            maybe += int((labelled & ~alone).sum())
            rows += len(y)
    ref = sum_ce / rows
    print(f"\nscore after iteration 4: fused {loss_fused!r} torch {loss_torch!r} float64 oracle {ref!r}; accuracy fused "
          f"{acc_fused} torch {acc_torch}, oracle {sure}/{rows} correct with {maybe} near-ties")
    assert rows == RR.N_SAMPLES
    assert abs(loss_fused - ref) <= 2 * abs(loss_torch - ref)          # test_score_fused_agrees_with_score's tolerance
    assert acc_fused == acc_torch
    assert sure <= round(acc_fused * rows) <= sure + maybe             # equal wherever there is no tie
    # the mode is left as it is: the replays do not look at it
    for k in range(4, N_IT):
        out = step()
        _assert_same(_snap(model, opt, out["indices"], out), whole[k], f"iteration {k + 1} after the scoring")
    assert not model.training and _counters(model, opt, src) == (N_IT, N_IT, N_IT)


# ------------------------------------------------------------------ e. two ranks on one GPU
RANK_ITERATIONS = {"graph": 4, "train": 3}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q, variant):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.training import fused_cross_entropy, make_stopper_after_n_iters, train

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    case = RR.CASES["cfg2"]
    # every rank its own parameters and its own dropout seed: the broadcast must make them rank 0's, which are the case's
    model, opt, src = _objects(case, "f32", model_seed=None if rank == 0 else case.model_seed + rank,
                               dropout_seed=case.dropout_seed + rank, rank=rank, world=world)
    rows = []

    def note(indices, loss, warmup=False):   # after a warm-up the model's draw record is the graph's, not yet written
        torch.cuda.synchronize(DEV)
        rows.append((indices.tolist(), None if warmup else D.read_state(model.dropout_record),
                     None if loss is None else float(loss.detach())))

    if variant == "graph":
        ddp.broadcast_parameters(list(model.parameters()) + list(model.buffers()))   # as training.train does
        model._refresh_p()
        opt.refresh_master()
        reducer = ddp.FlatGradAllReducer(model.parameters(), average=True)
        step = _full_step(case, model, opt, src, reducer=reducer)
        note(step.indices, None, warmup=True)
        for _ in range(RANK_ITERATIONS[variant] - 1):
            out = step()
            note(out["indices"], out["loss"])
    else:
        zero = torch.zeros((), device=DEV)
        train(src, model, opt, DEV, fused_cross_entropy, lambda st_x, st_it: zero, 0.0, [],
              [lambda st_x, st_it: note(st_it["indices"], st_it["loss"])],
              [make_stopper_after_n_iters(RANK_ITERATIONS[variant] - 1)])
    torch.cuda.synchronize(DEV)
    q.put((rank, rows, _counters(model, opt, src), model.dropout_state_dict()["seed"],
           [t.cpu().numpy() for t in (opt.flat, opt.m, opt.v)]))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(variant):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")   # fresh child processes
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, variant)) for r in range(2)]
    for p in procs:
        p.start()
    got = {rank: rest for rank, *rest in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return got


def _assert_ranks_agree(got, variant):
    """Per iteration the two shards are disjoint and together the global batch, the draw records are equal (rank 0's
    seed, draw k); at the end the counters, the parameters and the Adam state are equal."""
    case, n = RR.CASES["cfg2"], RANK_ITERATIONS[variant]
    (rows0, counters0, seed0, state0), (rows1, counters1, seed1, state1) = got[0], got[1]
    assert len(rows0) == len(rows1) == n
    for k in range(n):
        (ind0, record0, _), (ind1, record1, _) = rows0[k], rows1[k]
        assert ind0 + ind1 == batches.expected_indices(case.batch_seed, k, RR.N_SAMPLES, RR.GLOBAL_BATCH)
        assert len(ind0) == len(ind1) == RR.GLOBAL_BATCH // 2 and not set(ind0) & set(ind1)
        seen = variant != "graph" or k > 0   # (the graphed step's warm-up shows no record)
        assert record0 == record1 == ({"seed": case.dropout_seed, "draws_done": k} if seen else None)
    assert counters0 == counters1 == (n, n, n) and seed0 == seed1 == case.dropout_seed
    for a, b in zip(state0, state1):
        assert np.array_equal(a, b)
    w0 = RR.flat(RR.initial_parameters(case, torch.float32)).float().numpy()
    assert not np.array_equal(state0[0], w0)   # and they did train


def test_two_ranks_in_the_full_step_draw_equal_masks_and_disjoint_shards():
    """4 iterations of the full step with a `FlatGradAllReducer` over gloo (forward + backward graph, eager all-reduce,
    optimizer graph).  The float32 trajectory meets the bound of (a) against the float64 reference of the GLOBAL batch.
    Measured on an MI355X: e_hip = 4.298e-07, e_torch32 = 4.285e-07."""
    case = RR.CASES["cfg2"]
    got = _two_ranks("graph")
    _assert_ranks_agree(got, "graph")
    n = RANK_ITERATIONS["graph"]
    losses = {k: 0.5 * (got[0][0][k][2] + got[1][0][k][2]) for k in range(1, n)}   # equal shards: the mean of the means
    _trajectory_bound("cfg2 float32, two ranks, 4 iterations", [torch.from_numpy(got[0][3][0])], losses,
                      _reference("cfg2", "f64"), _reference("cfg2", "f32"), RR.initial_parameters(case, torch.float32), n,
                      range(1, n))


def test_two_ranks_in_the_eager_train_loop_with_source_and_dropout_together():
    """3 iterations of `training.train(dl=src)` (its own broadcast and reducer) with the fused dropout on: the same
    equalities."""
    _assert_ranks_agree(_two_ranks("train"), "train")
