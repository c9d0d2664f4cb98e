"""The step trace and K iterations per graph launch on the GPU (`-m gpu`).  Every comparison here is exact.

  1. `dctn_step_trace_record` against a CPU restatement of its counting rules, every field of the record;
  2. the ring with a capacity that is no power of two;
  3. the buffer contract under tests/guarded_buffers.py, and the return codes;
  4. `GraphedTrainStep(iters_per_launch=3)`: two launches equal six launches of one iteration, state and records;
  5. a gradient guard that halts inside a launch;
  6. a run resumed through `RunState(..., trace=trace)` continues its records;
  7. `GraphedScore.with_batches_per_launch`;
  8. two ranks on one GPU with the all-reduce inside the graph.

Tests 4 - 8 build the objects of tests/test_gpu_full_recipe.py from tests/recipe_reference.py in the same way: 37 samples in
batches of 8, fused dropout, `FlatAdam`; 1 warm-up iteration + 6 more cross an epoch boundary inside the graph."""
import functools
import os
import shutil
import socket
import tempfile
import atexit

import numpy as np
import pytest
import torch

from dctn_amd import _lib as L
from dctn_amd import batches
from tests import recipe_reference as RR
from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
MODES = {"f32": (F32, False), "bf16_master": (BF16, True)}
NAN_BITS = 0x7FC01234   # a NaN with a payload: floats travel as bit patterns


def _record_type():
    from dctn_amd.training import StepTrace

    return StepTrace.RECORD


def _assert_same_records(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape[0]} records, expected {want.shape[0]}"
    for field in _record_type().names:   # by their bytes: NaN-safe, and -0.0 is not 0.0
        assert got[field].tobytes() == want[field].tobytes(), f"{what}: field {field!r}: {got[field]} != {want[field]}"


# ------------------------------------------------------------------ 1. the kernel against a CPU restatement
def _inputs(B, C, dtype):
    """Logits with many ties (multiples of 0.5), rows labelled -100, C and -1, all-equal rows, a NaN in the last class of a
    row labelled with that class, and rows of nothing but NaN - wherever the shape has room for them."""
    g = torch.Generator().manual_seed(100 * B + C)
    logits = torch.randint(-3, 4, (B, C), generator=g).float() * 0.5
    labels = torch.randint(0, C, (B,), generator=g)
    for i in range(B):
        if i % 5 == 0:
            logits[i] = 1.5                       # every class ties: the lowest index wins
            labels[i] = 0 if i % 10 == 0 else C - 1
        if i % 9 == 2:
            logits[i, C - 1] = float("nan")       # never the maximum, whatever the label says
            labels[i] = C - 1
        if i % 17 == 4:
            logits[i] = float("nan")              # no maximum at all: a wrong row
        if i % 7 == 3:
            labels[i] = -100
        if i % 11 == 5:
            labels[i] = C
        if i % 13 == 1:
            labels[i] = -1
    return logits.to(dtype), labels


def _count(logits, labels):
    """`dctn_ce_score_accumulate`'s rules in numpy: rows labelled -100 are skipped; the maximum is taken with fmax (a NaN
    is never it); a row is correct when its label is the lowest index that holds the maximum (argmax of the hits)."""
    x = logits.float().numpy()
    rows = correct = 0
    C = x.shape[1]
    for row, y in zip(x, labels.tolist()):
        if y == -100:
            continue
        rows += 1
        hits = row == np.fmax.reduce(row, initial=-np.inf)
        if hits.any() and 0 <= y < C and y == int(np.argmax(hits)):
            correct += 1
    return rows, correct


def _blocks():
    """(reg, guard, adam, source) blocks with recognisable words, as int32 host tensors."""
    as_i32 = lambda words: torch.tensor(np.array(words, dtype=np.uint32).view(np.int32))
    f = lambda v: int(np.float32(v).view(np.uint32))
    reg = as_i32([f(-0.0)])
    guard = as_i32([f(105.0), NAN_BITS, 1, 0xFFFFFFFE, 9, 4, 0, f(0.3125)])   # last_norm NaN, halted, bad_step -2, coef
    adam = as_i32([41, f(3e-3), 0, 0])
    source = as_i32([0xDEADBEEF, 0x01234567, 0x80000005, 0])                  # a counter above 2^31: it is unsigned
    return reg, guard, adam, source


def _expected_words(seq, present, loss_bits, rows, correct):
    reg, guard, adam, source = (b.numpy().view(np.uint32) for b in _blocks())
    w = np.zeros(16, dtype=np.uint32)
    w[0], w[1], w[2] = seq, present, loss_bits
    w[3] = reg[0] if present & 1 else 0
    w[4], w[5] = rows, correct
    if present & 2:
        w[6], w[7], w[8], w[9] = guard[1], guard[7], guard[2], guard[3]
    if present & 4:
        w[10], w[11] = adam[0], adam[1]
    if present & 8:
        w[12] = source[2]
    return w


def _launch(logits, labels, loss, blocks, present, head, ring, capacity, B=None, C=None, dtype=None):
    ptr = lambda t, bit: t.data_ptr() if present & bit else None
    reg, guard, adam, source = blocks
    return L.lib().dctn_step_trace_record(
        logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), ptr(reg, 1), ptr(guard, 2), ptr(adam, 4), ptr(source, 8),
        head.data_ptr(), ring.data_ptr(), capacity, logits.shape[0] if B is None else B,
        logits.shape[1] if C is None else C, L.dtype_code(logits) if dtype is None else dtype, L.stream_ptr(DEV))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 2), (64, 10), (1025, 10), (257, 17)])
def test_every_field_of_the_record_equals_the_cpu_restatement(B, C, dtype):
    logits, labels = _inputs(B, C, dtype)
    rows, correct = _count(logits, labels)
    if B >= 64:
        assert 0 < correct < rows < B                       # skipped rows, wrong rows and right rows are all there
        assert bool(torch.isnan(logits.float()).any()) and bool((labels == C).any()) and bool((labels == -100).any())
    d_logits, d_labels = logits.to(DEV), labels.to(DEV)
    blocks = tuple(b.to(DEV) for b in _blocks())
    loss_bits = NAN_BITS if B == 3 else int(np.float32(2.302585).view(np.uint32))
    loss = torch.tensor(np.array([loss_bits], dtype=np.uint32).view(np.int32)).to(DEV).view(F32)
    capacity = 7
    head = torch.zeros(4, dtype=I32, device=DEV)
    ring = torch.full((16 * capacity,), 0x55, dtype=I32, device=DEV)
    masks = (15, 0, 1, 2, 4, 8)                             # every optional block present, absent, and each one alone
    for present in masks:
        assert _launch(d_logits, d_labels, loss.view(I32), blocks, present, head, ring, capacity) == 0
    torch.cuda.synchronize(DEV)
    assert head.cpu().tolist() == [len(masks), 0, 0, 0]
    got = np.frombuffer(ring.cpu().numpy().tobytes(), dtype=_record_type())
    want = np.frombuffer(np.concatenate([_expected_words(seq, present, loss_bits, rows, correct)
                                         for seq, present in enumerate(masks)]).tobytes(), dtype=_record_type())
    print(f"\nB={B} C={C} {dtype}: rows {rows} correct {correct}")
    _assert_same_records(got[: len(masks)], want, f"B={B} C={C}")
    assert ring.cpu()[16 * len(masks):].eq(0x55).all()      # the slot no launch addressed


# ------------------------------------------------------------------ 2. the ring
def test_a_ring_of_three_after_eleven_launches():
    from dctn_amd.training import StepTrace

    trace = StepTrace(DEV, capacity=3)
    logits = torch.tensor([[0.0, 1.0], [2.0, 1.0]], device=DEV)
    labels = torch.tensor([1, 1], device=DEV)
    losses = torch.arange(11, dtype=F32, device=DEV)
    for i in range(11):
        trace.record(logits, labels, losses[i])
    torch.cuda.synchronize(DEV)
    slots = np.frombuffer(trace._ring.cpu().numpy().tobytes(), dtype=StepTrace.RECORD)
    assert slots["seq"].tolist() == [9, 10, 8]               # slot order: seq % 3
    assert trace._head.cpu().tolist() == [11, 0, 0, 0] and trace.state_dict() == {"records_done": 11, "capacity": 3}
    records = trace.read()
    assert records["seq"].tolist() == [8, 9, 10] and trace.lost == 8
    assert records["loss"].tolist() == [8.0, 9.0, 10.0] and records["rows"].tolist() == [2] * 3
    assert records["correct"].tolist() == [1] * 3 and records["present"].tolist() == [0] * 3
    assert trace.read().size == 0 and trace.lost == 0        # nothing new
    trace.record(logits, labels, losses[0])
    again = trace.read()
    assert again["seq"].tolist() == [11] and trace.lost == 0


# ------------------------------------------------------------------ 3. the buffer contract
@functools.lru_cache(maxsize=None)
def _contract_run(fill):
    """One launch with every buffer inside the guarded arena: (slot bytes, other ring bytes, head, inputs unchanged?)."""
    B, C, capacity, done = 257, 17, 5, 7
    logits, labels = _inputs(B, C, BF16)
    loss = torch.tensor([0.75])
    host = (logits, labels, loss) + _blocks()
    with guarded(fill=fill) as arena:
        placed = [arena.place(t.to(DEV)) for t in host]
        head = arena.zeros((4,), I32, DEV)
        ring = arena.empty((16 * capacity,), I32, DEV)
        head[0] = done
        rc = _launch(placed[0], placed[1], placed[2], tuple(placed[3:]), 15, head, ring, capacity)
        # bad arguments: their codes, and nothing is launched (head and ring are compared below)
        bad = [_launch(placed[0], placed[1], placed[2], tuple(placed[3:]), 15, head, ring, capacity, **kw)
               for kw in (dict(B=0), dict(C=0), dict(dtype=L.F64))]
        bad.append(_launch(placed[0], placed[1], placed[2], tuple(placed[3:]), 15, head, ring, 0))
        bad.append(L.lib().dctn_step_trace_record(placed[0].data_ptr(), placed[1].data_ptr(), placed[2].data_ptr(), None,
                                                  None, None, None, None, ring.data_ptr(), capacity, B, C, L.BF16,
                                                  L.stream_ptr(DEV)))
    arena.check()   # synchronises; every guard byte around every buffer is intact
    ring_bytes = ring.cpu().numpy().view(np.uint8).reshape(capacity, 64)
    untouched = all(torch.equal(p.cpu().view(torch.uint8), t.contiguous().view(torch.uint8)) for p, t in zip(placed, host))
    return rc, bad, ring_bytes, head.cpu().tolist(), untouched, (done, capacity, _count(logits, labels))


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_only_the_head_and_the_addressed_slot_change(fill):
    rc, bad, ring_bytes, head, untouched, (done, capacity, (rows, correct)) = _contract_run(fill)
    assert rc == 0
    assert bad == [L.ERR_BAD_SHAPE, L.ERR_BAD_SHAPE, L.ERR_BAD_DTYPE, L.ERR_BAD_SHAPE, L.ERR_NULL]
    assert head == [done + 1, 0, 0, 0]                       # one launch, not six
    slot = done % capacity
    for s in range(capacity):
        if s != slot:
            assert (ring_bytes[s] == fill).all(), f"slot {s} was written"
    got = np.frombuffer(ring_bytes[slot].tobytes(), dtype=_record_type())
    want = np.frombuffer(_expected_words(done, 15, int(np.float32(0.75).view(np.uint32)), rows, correct).tobytes(),
                         dtype=_record_type())
    _assert_same_records(got, want, f"fill 0x{fill:02x}")
    assert untouched, "an input buffer changed"


def test_the_slot_does_not_depend_on_what_the_ring_held():
    a, b = _contract_run(0xFF), _contract_run(0x7B)
    slot = a[5][0] % a[5][1]
    assert a[2][slot].tobytes() == b[2][slot].tobytes()


# ------------------------------------------------------------------ the recipe's objects (tests 4 - 8)
def _params(model):
    return list(model.epses) + [model.linear.weight, model.linear.bias]


def _model(case, dtype, seed=None):
    model = RR.initial_model(case, dtype, DEV, seed)
    if seed is None:
        with torch.no_grad():
            for p, value in zip(_params(model), RR.initial_parameters(case, dtype)):
                p.copy_(value)
    return model


def _objects(case, mode, model_seed=None, dropout_seed=None, batch_seed=None, rank=None, world=None, guard=None,
             features=None):
    from dctn_amd.batches import DeviceBatches
    from dctn_amd.training import FlatAdam

    dtype, master = MODES[mode]
    model = _model(case, dtype, model_seed)
    model.use_fused_dropout(case.dropout_seed if dropout_seed is None else dropout_seed)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=case.lr,
                   weight_decay=case.weight_decay, l2=case.reg_coeff if case.reg == "epswise" else 0.0,
                   master_weights=master, guard=guard)
    images, labels = RR.make_data(case)
    seed = case.batch_seed if batch_seed is None else batch_seed
    if features is not None:
        src = DeviceBatches.from_features(features.to(DEV), labels, RR.GLOBAL_BATCH, seed=seed, rank=rank, world=world)
    else:
        src = DeviceBatches(images, labels, RR.GLOBAL_BATCH, dtype=dtype, seed=seed, scale=case.scale, rank=rank,
                            world=world)
    return model, opt, src


def _composition(model):
    return model.epses_composition_l2_regularizer()


def _step(case, model, opt, src, trace, K, reducer=None, graph_allreduce=None):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    through_autograd = case.reg == "composition"
    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, reg_fn=_composition if through_autograd else None,
                            reg_coeff=case.reg_coeff if through_autograd else 0.0, reducer=reducer, warmup=1,
                            graph_allreduce=graph_allreduce, batch_source=src, iters_per_launch=K, trace=trace)


def _state(model, opt, src):
    torch.cuda.synchronize(DEV)
    return dict(flat=opt.flat.clone(), master=None if opt.master is None else opt.master.clone(), m=opt.m.clone(),
                v=opt.v.clone(), counters=(opt.t, model.dropout_state_dict()["draws_done"], src.state_dict()["batches_done"]))


def _assert_same_state(got, want, what):
    for key in ("flat", "master", "m", "v"):
        if want[key] is None:
            assert got[key] is None, f"{what}: {key}"
        else:
            assert got[key].dtype == want[key].dtype, f"{what}: {key}"
            assert torch.equal(got[key].view(torch.uint8), want[key].view(torch.uint8)), f"{what}: {key} differs"
    assert got["counters"] == want["counters"], f"{what}: counters {got['counters']} != {want['counters']}"


_TMP = []


def _tmp_dir():
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="dctn_step_trace_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    return _TMP[0]


RUNS = [("cfg2", "f32"), ("cfg2", "bf16_master"), ("two_layer", "f32")]   # the last: the composition regulariser


@functools.lru_cache(maxsize=None)
def _run_a(name, mode):
    """1 warm-up + 6 launches of ONE iteration, with a trace.  Computed once per case and shared; nobody writes into it."""
    from dctn_amd.training import StepTrace

    case = RR.CASES[name]
    labels = RR.make_data(case)[1]
    model, opt, src = _objects(case, mode)
    trace = StepTrace(DEV, capacity=16)
    step = _step(case, model, opt, src, trace, 1)
    states, seen = {}, []
    for i in range(1, 7):
        out = step()
        assert "iters" not in out and step.iters_per_launch == 1   # one iteration per launch: the keys it always returned
        torch.cuda.synchronize(DEV)
        logits = out["output"].detach().float().cpu().numpy()
        y = labels[out["indices"].cpu()].numpy()
        seen.append((out["loss"].detach().cpu().numpy().tobytes(), int((logits.argmax(axis=1) == y).sum()), len(y),
                     out["reg_term"].detach().float().cpu().numpy().tobytes()))
        if i in (3, 6):
            states[i] = _state(model, opt, src)
    return states, trace.read(), trace.lost, seen


@functools.lru_cache(maxsize=None)
def _run_b(name, mode):
    """Fresh objects, 1 warm-up + 2 launches of THREE iterations; a whole-run snapshot (trace included) after launch 1."""
    from dctn_amd import checkpoint as C
    from dctn_amd.training import StepTrace

    case = RR.CASES[name]
    model, opt, src = _objects(case, mode)
    trace = StepTrace(DEV, capacity=16)
    step = _step(case, model, opt, src, trace, 3)
    run = C.RunState(model, opt, batch_source=src, trace=trace)
    assert run.names[-2:] == ["trace.head", "trace.ring"]
    states = {}
    out = step()
    assert out["iters"] == 3
    snap = run.snapshot({"num_iters_done": 3})
    states[3] = _state(model, opt, src)
    step()
    states[6] = _state(model, opt, src)
    path = snap.save(os.path.join(_tmp_dir(), f"run_b_{name}_{mode}.dctn"))
    return states, trace.read(), trace.lost, path


# ------------------------------------------------------------------ 4. K iterations per launch = K launches of one
@pytest.mark.parametrize("name,mode", RUNS)
def test_two_launches_of_three_iterations_equal_six_launches_of_one(name, mode):
    states_a, records_a, lost_a, seen = _run_a(name, mode)
    states_b, records_b, lost_b, _ = _run_b(name, mode)
    for i in (3, 6):
        assert states_a[i]["counters"] == (i + 1, i + 1, i + 1)
        _assert_same_state(states_b[i], states_a[i], f"{name} {mode}: after iteration {i + 1}")
    assert lost_a == lost_b == 0 and records_a["seq"].tolist() == list(range(7))      # the warm-up's record included
    _assert_same_records(records_b, records_a, f"{name} {mode}")
    case = RR.CASES[name]
    has_reg = case.reg == "composition"
    assert records_a["present"].tolist() == [(1 if has_reg else 0) | 4 | 8] * 7
    assert records_a["opt_steps_done"].tolist() == list(range(1, 8)) == records_a["batches_done"].tolist()
    assert records_a["lr"].tobytes() == np.full(7, case.lr, dtype="<f4").tobytes()
    for i, (loss_bytes, correct, rows, reg_bytes) in enumerate(seen, 1):               # replay i wrote record i
        assert records_a["loss"][i].tobytes() == loss_bytes, f"record {i}: loss"
        assert (int(records_a["rows"][i]), int(records_a["correct"][i])) == (rows, correct), f"record {i}: counts"
        if has_reg:
            assert records_a["reg"][i].tobytes() == reg_bytes, f"record {i}: reg"
    print(f"\n{name} {mode}: losses {records_a['loss'].tolist()} correct {records_a['correct'].tolist()}")
    assert len({bytes(b) for b, *_ in seen}) == 6                                      # six different batches


# ------------------------------------------------------------------ 5. a guard that halts inside a launch
def test_a_guard_that_halts_in_the_second_iteration_of_a_launch():
    from dctn_amd.training import GradGuard, StepTrace

    case = RR.CASES["cfg2"]
    images, labels = RR.make_data(case)
    features = RR.make_batch(images, labels, range(RR.N_SAMPLES), F32, case.scale)[0]   # (1, n, H, W, 2)
    # iteration 0 is the warm-up, the launch holds iterations 1, 2, 3; the four batches of an epoch are disjoint
    order = [batches.expected_indices(case.batch_seed, k, RR.N_SAMPLES, RR.GLOBAL_BATCH) for k in range(4)]
    victim = order[2][0]
    assert all(victim not in order[k] for k in (0, 1, 3))
    poisoned = features.clone()
    poisoned[0, victim, 3, 4, 1] = float("nan")   # a non-finite value in the data: the loss and the gradients become NaN

    def run(x_full, K, launches, guarded_opt):
        guard = GradGuard(DEV, None) if guarded_opt else None
        model, opt, src = _objects(case, "f32", guard=guard, features=x_full)
        trace = StepTrace(DEV, capacity=8)
        step = _step(case, model, opt, src, trace, K)
        for _ in range(launches):
            step()
        return _state(model, opt, src), trace.read(), guard

    halted_state, records, guard = run(poisoned, 3, 1, True)
    good_state, good_records, _ = run(features, 1, 1, True)      # warm-up + iteration 1 on clean data: the last good step
    assert records["seq"].tolist() == [0, 1, 2, 3]
    assert records["halted"].tolist() == [0, 0, 1, 1]
    assert records["bad_step"].tolist() == [-1, -1, 2, 2]          # the guard's check number 2 = iteration 2
    assert records["opt_steps_done"].tolist() == [1, 2, 2, 2]      # frozen from the halting iteration on
    assert records["batches_done"].tolist() == [1, 2, 3, 4]        # the source goes on drawing
    assert records["coef"].tolist() == [1.0, 1.0, 0.0, 0.0] and records["present"].tolist() == [2 | 4 | 8] * 4
    assert np.isnan(records["loss"][2]) and np.isnan(records["grad_norm"][2])
    assert np.isfinite(records["loss"][[0, 1, 3]]).all() and np.isfinite(records["grad_norm"][[0, 1, 3]]).all()
    state = guard.read()
    assert state["halted"] == 1 and state["bad_step"] == 2 and state["seen"] == 4
    _assert_same_records(records[:2], good_records, "the records before the halt")
    for key in ("flat", "m", "v"):
        assert torch.equal(halted_state[key], good_state[key]), f"{key} moved after the halt"
    assert halted_state["counters"] == (2, 4, 4) and good_state["counters"] == (2, 2, 2)


# ------------------------------------------------------------------ 6. resume
@pytest.mark.parametrize("name,mode", [("cfg2", "bf16_master")])
def test_a_run_resumed_from_a_snapshot_continues_its_records(name, mode):
    from dctn_amd import checkpoint as C
    from dctn_amd.training import StepTrace

    case = RR.CASES[name]
    states_b, records_b, _, path = _run_b(name, mode)
    # fresh objects that share nothing with the saved run but the data
    model, opt, src = _objects(case, mode, model_seed=case.model_seed + 1, dropout_seed=99, batch_seed=77)
    trace = StepTrace(DEV, capacity=16)
    step = _step(case, model, opt, src, trace, 3)        # its warm-up trains and records
    step()                                               # and a launch of its own: 4 records of another run in the ring
    run = C.RunState(model, opt, batch_source=src, trace=trace)
    assert not torch.equal(opt.flat, states_b[3]["flat"])
    assert run.load(path) == {"num_iters_done": 3}
    _assert_same_state(_state(model, opt, src), states_b[3], "after the load")
    assert trace.state_dict()["records_done"] == 4 and trace.read().size == 0     # the saved run's records count as read
    out = step()
    assert out["iters"] == 3
    _assert_same_state(_state(model, opt, src), states_b[6], "launch 2 of the resumed run")
    records = trace.read()
    assert records["seq"].tolist() == [4, 5, 6] and trace.lost == 0
    _assert_same_records(records, records_b[4:], "records 4 - 6 of the resumed run")
    # without the argument the region list is what it was
    assert [n for n in C.RunState(model, opt, batch_source=src).names if n.startswith("trace")] == []


# ------------------------------------------------------------------ 7. GraphedScore, several batches per launch
def test_graphed_score_with_five_batches_per_launch_equals_one_per_launch():
    from dctn_amd.batches import DeviceBatches
    from dctn_amd.evaluation import GraphedScore

    case = RR.CASES["cfg2"]
    images, labels = RR.make_data(case)
    model = _model(case, F32)

    def source():
        return DeviceBatches(images, labels, RR.GLOBAL_BATCH, dtype=F32, seed=1, scale=case.scale, shuffle=False)

    assert source().padded_steps == 5
    one = GraphedScore.with_batches_per_launch(model, source(), 1)
    five = GraphedScore.with_batches_per_launch(model, source(), 5)
    plain = GraphedScore(model, source())
    assert (one.batches_per_launch, five.batches_per_launch, plain.batches_per_launch) == (1, 5, 1)
    results = []
    for scorer in (one, five, plain):
        scorer.launch()
        torch.cuda.synchronize(DEV)
        sums = scorer.acc.cpu().numpy().tobytes()
        results.append((sums, scorer.read(), scorer.rows, scorer.correct, scorer.src.state_dict()["batches_done"]))
    print(f"\nscore: {results[0][1]} rows {results[0][2]} correct {results[0][3]}")
    assert results[0] == results[1] == results[2]
    assert results[0][2] == RR.N_SAMPLES and results[0][4] == 5
    five.launch()                                          # a second pass walks the same batches
    assert five.read() == results[0][1] and five.src.state_dict()["batches_done"] == 10
    with pytest.raises(ValueError, match="padded_steps"):
        GraphedScore.with_batches_per_launch(model, source(), 2)


# ------------------------------------------------------------------ train_graphed and the trace logger
def test_train_graphed_runs_whole_launches_and_hands_the_records_to_the_logger():
    from dctn_amd.training import StepTrace, make_stopper_after_n_iters, make_trace_logger, train_graphed

    _, records_a, _, _ = _run_a("cfg2", "f32")
    case = RR.CASES["cfg2"]
    model, opt, src = _objects(case, "f32")
    trace = StepTrace(DEV, capacity=16)
    step = _step(case, model, opt, src, trace, 3)
    got, iters = [], []
    logger = make_trace_logger(trace, 2, lambda records, lost: got.append((records, lost)))
    st_x, st_it = train_graphed(step, 5, after_launch=[logger, lambda st_x, st_it: iters.append(st_it["num_iters_done"])],
                                first_iter=1)             # iteration 0 was the warm-up
    assert iters == [3, 6] and st_it["num_iters_done"] == 6 and st_it["iters"] == 3 and st_x["step"] is step
    assert len(got) == 1 and got[0][1] == 0               # read once, after the second launch
    _assert_same_records(got[0][0], records_a, "the logger's records")
    # a hook that asks to stop ends the loop at that launch boundary
    _, st_it = train_graphed(step, 30, after_launch=[make_stopper_after_n_iters(8)], first_iter=7)
    assert st_it["num_iters_done"] == 9 and st_it["stop"] is True
    logger.flush()
    assert got[-1][0]["seq"].tolist() == [7, 8, 9]


# ------------------------------------------------------------------ 8. two ranks on one GPU, the all-reduce in the graph
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.training import StepTrace

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    case = RR.CASES["cfg2"]
    out = {"rank": rank}
    try:
        def run(K, launches):
            model, opt, src = _objects(case, "f32", model_seed=None if rank == 0 else case.model_seed + rank,
                                       dropout_seed=case.dropout_seed + rank, rank=rank, world=world)
            ddp.broadcast_parameters(list(model.parameters()) + list(model.buffers()))   # as training.train does
            model._refresh_p()
            opt.refresh_master()
            # the direct all-reduce is a plain kernel launch: it is captured without a probe
            reducer = ddp.FlatGradAllReducer(model.parameters(), average=True, algorithm="direct")
            trace = StepTrace(DEV, capacity=8)
            try:
                step = _step(case, model, opt, src, trace, K, reducer=reducer, graph_allreduce=True)
            except RuntimeError as e:
                if "capturing the all-reduce" in str(e):
                    return None, f"{type(e).__name__}: {e}"
                raise
            assert step.allreduce_in_graph and step.g_opt is None
            for _ in range(launches):
                dist.barrier()                     # the ranks enter every launch together (the kernel's wait is bounded)
                step()
            torch.cuda.synchronize(DEV)
            reducer.check()                        # raises on every rank if a wait timed out
            state = _state(model, opt, src)
            return ([state[k].cpu().numpy() for k in ("flat", "m", "v")], state["counters"], trace.read().tobytes()), None

        one, why = run(1, 3)
        three, why3 = (None, why) if why else run(3, 1)
        out.update(one=one, three=three, no_capture=why or why3)
        # the split form cannot run K iterations in a launch: refused before anything is captured
        model, opt, src = _objects(case, "f32", rank=rank, world=world)
        reducer = ddp.FlatGradAllReducer(model.parameters(), average=True)
        try:
            _step(case, model, opt, src, None, 3, reducer=reducer, graph_allreduce=False)
            out["refused"] = None
        except ValueError as e:
            out["refused"] = str(e)
        out["counters_after_refusal"] = (opt.t, src.state_dict()["batches_done"])
    except Exception as e:   # noqa: BLE001
        out["error"] = f"{type(e).__name__}: {e}"
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_three_iterations_per_launch_equal_one_per_launch():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")   # fresh child processes
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted((q.get(timeout=300) for _ in procs), key=lambda o: o["rank"])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for o in outs:
        assert "error" not in o, o["error"]
        assert o["refused"] is not None and "graph_allreduce" in o["refused"], o["refused"]
        assert o["counters_after_refusal"] == (0, 0)        # raised before the warm-up
    if any(o["no_capture"] for o in outs):
        pytest.skip(f"the all-reduce cannot be captured into a graph on this machine: {outs[0]['no_capture']}")
    for o in outs:
        (state1, counters1, records1), (state3, counters3, records3) = o["one"], o["three"]
        assert counters1 == counters3 == (4, 4, 4)
        for a, b in zip(state1, state3):
            assert a.tobytes() == b.tobytes(), f"rank {o['rank']}: K = 3 differs from K = 1"
        got, want = (np.frombuffer(r, dtype=_record_type()) for r in (records3, records1))
        _assert_same_records(got, want, f"rank {o['rank']}")
        assert got["seq"].tolist() == [0, 1, 2, 3]
    for a, b in zip(outs[0]["three"][0], outs[1]["three"][0]):
        assert a.tobytes() == b.tobytes(), "the ranks diverged"
    # every rank records its own shard: 4 of the 8 rows, and its own loss
    r0, r1 = (np.frombuffer(o["three"][2], dtype=_record_type()) for o in outs)
    assert r0["rows"].tolist() == r1["rows"].tolist() == [RR.GLOBAL_BATCH // 2] * 4
    assert r0["loss"].tobytes() != r1["loss"].tobytes()
