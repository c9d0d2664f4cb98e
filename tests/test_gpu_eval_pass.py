"""The padded sequential draw (DCTN_BATCH_PAD_TAIL) and the graphed evaluation pass on the GPU (`-m gpu`).

Part 1, the raw C-ABI inside guarded buffers, bit for bit against torch's own indexing on the CPU and
`batches.expected_padded_indices`: both source kinds, the three dtypes, both access forms of each kernel, two shards, the
row loop's stride, the counter over two wraps, and the refusal of the flag without the identity order.

Part 2, `evaluation.GraphedScore` and `evaluation.make_evaluation_hook`.  Every check is made against something else
than the graphed pass itself: `score_fused` over an eager loader of the same padded batches, `score` (torch ops) over the
eager short-batch source, a float64 oracle, a twin that never evaluates, a clone of the weights.

Every measured figure is printed before it is asserted (run with -s)."""
import functools
import os
import socket

import pytest
import torch
import torch.nn.functional as F

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd import batches as B
from oracle import ref_cpu as R
from tests import recipe_reference as RR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234567890ABCDEF
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
NAME = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16"}
GUARD, GUARD_BYTE, STALE_BYTE = 256, 0xA5, 0xFF   # guard bytes on both sides; what an output holds before the launch
PADDED = L.BATCH_IDENTITY_ORDER | L.BATCH_PAD_TAIL


class Framed:
    """A tensor inside a guarded byte allocation (as tests/test_gpu_batches.py builds it).  An output (``values`` None)
    starts as 0xFF bytes (NaN in every float dtype, -1 in int64); ``shift`` moves the base off its 256-byte alignment by
    that many bytes."""

    def __init__(self, shape, dtype, values=None, shift=0):
        numel = 1
        for s in shape:
            numel *= s
        self.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + self.nbytes + 16,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + shift
        body = self.raw[self.lo : self.lo + self.nbytes]
        body.fill_(STALE_BYTE)
        self.view = body.view(dtype).view(shape)
        if values is not None:
            self.view.copy_(values)
        self.before = self.raw.clone()

    def guards_intact(self):
        a, b = self.raw, self.before
        return torch.equal(a[: self.lo], b[: self.lo]) and torch.equal(a[self.lo + self.nbytes :], b[self.lo + self.nbytes :])

    def untouched(self):
        return torch.equal(self.raw, self.before)


def _words(t):
    return [int(v) & 0xFFFFFFFF for v in t.cpu().tolist()]


def _bits(t):
    """Bit-for-bit comparison key (NaN-safe)."""
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def _state(k=0):
    return Framed((4,), torch.int32, torch.tensor(B._state_words(SEED, k), dtype=torch.int32))


# ------------------------------------------------------------------ 1. the raw ABI
def _check_padded_draws(kind, n, G, row_len, width, dtype, world=1, draws=None):
    """Draws k = 0 .. 2 S (two wraps of the counter) for every rank of `world`, each rank on its own state block and
    every draw into fresh guarded outputs."""
    g = torch.Generator().manual_seed(n * 131 + row_len)
    labels = torch.randint(0, 10, (n,), generator=g)
    if kind == L.BATCH_SRC_U8_TABLE:
        data = torch.randint(0, 256, (n, row_len), dtype=torch.uint8, generator=g)
        table = torch.randn(256, width, generator=g, dtype=torch.float64).to(dtype)
        src, tab = Framed((n, row_len), torch.uint8, data), Framed((256, width), dtype, table)
        x_shape = lambda count: (1, count, row_len, width)
        rows_of = lambda idx: table[data[idx].long()].unsqueeze(0)
        name = f"batch_draw_u8_{NAME[dtype]}"
    else:
        data = torch.randn(width, n, row_len, generator=g, dtype=torch.float64).to(dtype)
        src, tab = Framed((width, n, row_len), dtype, data), None
        x_shape = lambda count: (width, count, row_len)
        rows_of = lambda idx: data[:, idx]
        name = f"batch_draw_rows_{NAME[dtype]}"
    lab = Framed((n,), torch.int64, labels)
    S, Bl = -(-n // G), G // world
    states = [_state() for _ in range(world)]
    for k in range(2 * S + 1) if draws is None else draws:
        for r in range(world):
            x, y, ind = Framed(x_shape(Bl), dtype), Framed((Bl,), torch.int64), Framed((Bl,), torch.int64)
            rc = L.lib().dctn_batch_draw(src.view.data_ptr(), None if tab is None else tab.view.data_ptr(),
                                         lab.view.data_ptr(), x.view.data_ptr(), y.view.data_ptr(), ind.view.data_ptr(),
                                         states[r].view.data_ptr(), n, G, Bl, r * Bl, row_len, width, kind, PADDED,
                                         L.dtype_code(data if tab is None else table), L.stream_ptr(DEV))
            assert rc == 0 and dctn_amd.last_kernel() == name
            torch.cuda.synchronize()
            first = (k % S) * G + r * Bl
            idx = [p if p < n else -1 for p in range(first, first + Bl)]      # the definition, written out
            assert idx == B.expected_padded_indices(k, n, G, r, world)
            read = torch.tensor([i if i >= 0 else n - 1 for i in idx])         # a padding slot shows sample n - 1
            assert torch.equal(_bits(x.view.cpu()), _bits(rows_of(read))), f"x of draw {k}, rank {r}"
            assert y.view.cpu().tolist() == [int(labels[i]) if i >= 0 else -100 for i in idx], f"y of draw {k}, rank {r}"
            assert ind.view.cpu().tolist() == idx
            assert x.guards_intact() and y.guards_intact() and ind.guards_intact()
            assert _words(states[r].view) == [SEED & 0xFFFFFFFF, SEED >> 32, k + 1, 0] and states[r].guards_intact()
    assert src.untouched() and lab.untouched() and (tab is None or tab.untouched())
    return S


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("n,G,P,Q", [(10, 4, 8, 2), (10, 4, 9, 3), (5, 4, 4, 1), (12, 4, 8, 2)],
                         ids=["vector_path", "element_path_odd_Q", "one_sample_tail", "no_tail"])
def test_padded_draw_u8_table(n, G, P, Q, dtype):
    _check_padded_draws(L.BATCH_SRC_U8_TABLE, n, G, P, Q, dtype)


@pytest.mark.parametrize("R_,dtype", [(8, torch.float32), (5, torch.float32), (5, torch.float64), (5, torch.bfloat16)],
                         ids=["R8_f32_16_byte_path", "R5_f32_elements", "R5_f64_elements", "R5_bf16_elements"])
def test_padded_draw_rows(R_, dtype):
    _check_padded_draws(L.BATCH_SRC_ROWS, 10, 4, R_, 2, dtype)


@pytest.mark.parametrize("n", [10, 9], ids=["one_shard_all_padding", "one_shard_half_padding"])
def test_padded_draw_two_shards(n):
    last = [B.expected_padded_indices(2, n, 4, r, 2) for r in range(2)]
    assert last == ([[8, 9], [-1, -1]] if n == 10 else [[8, -1], [-1, -1]])
    _check_padded_draws(L.BATCH_SRC_U8_TABLE, n, 4, 8, 2, torch.float32, world=2)
    _check_padded_draws(L.BATCH_SRC_ROWS, n, 4, 8, 2, torch.bfloat16, world=2)


def test_padded_draw_with_more_rows_than_one_sweep_of_the_grid():
    """1100 rows a launch against at most 256 workgroups of 4 waves: waves take a second row.  The last batch has 100
    samples and 1000 padding rows."""
    idx = B.expected_padded_indices(2, 2300, 1100)
    assert idx[:100] == list(range(2200, 2300)) and idx[100:] == [-1] * 1000
    assert _check_padded_draws(L.BATCH_SRC_U8_TABLE, 2300, 1100, 4, 2, torch.bfloat16, draws=range(4)) == 3


def test_pad_tail_without_the_identity_order_is_refused_and_nothing_is_written():
    n, G, P, Q = 10, 4, 8, 2
    src, tab = Framed((n, P), torch.uint8, torch.zeros(n, P, dtype=torch.uint8)), Framed((256, Q), torch.float32)
    lab = Framed((n,), torch.int64, torch.zeros(n, dtype=torch.int64))
    x, y, ind, state = Framed((1, G, P, Q), torch.float32), Framed((G,), torch.int64), Framed((G,), torch.int64), _state(2)
    rc = L.lib().dctn_batch_draw(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(), x.view.data_ptr(),
                                 y.view.data_ptr(), ind.view.data_ptr(), state.view.data_ptr(), n, G, G, 0, P, Q,
                                 L.BATCH_SRC_U8_TABLE, L.BATCH_PAD_TAIL, L.F32, L.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == L.ERR_BAD_SHAPE
    for frame in (src, tab, lab, x, y, ind, state):
        assert frame.untouched()


# ------------------------------------------------------------------ 2. GraphedScore
GLOBAL, SIZE, SCALE = 16, 28, 0.8
BF16 = torch.bfloat16


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, SIZE, SIZE), dtype=torch.uint8, generator=g), torch.randint(0, 10, (n,), generator=g)


def _model(name, dtype=torch.float32, p=RR.P_KEEP, seed=None):
    """The model case `name` of tests/test_gpu_full_recipe.py (its spec and its model seed) at 28 x 28."""
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    case = RR.CASES[name]
    torch.manual_seed(case.model_seed if seed is None else seed)
    return EPSesPlusLinear(case.spec, UnitTheoreticalOutputStd(), p, DEV, dtype, image_size=SIZE)


def _params(model):
    return list(model.epses) + [model.linear.weight, model.linear.bias]


def _source(n, dtype=torch.float32, batch=GLOBAL, data_seed=0, **kw):
    images, labels = _data(n, data_seed)
    kw.setdefault("shuffle", False)
    return B.DeviceBatches(images, labels, batch, dtype=dtype, seed=SEED, scale=SCALE, **kw)


def _padded_batches(src):
    """An eager loader of one padded pass: fresh tensors per batch, from a counter at 0 (mod padded_steps)."""
    assert src.state_dict()["batches_done"] % src.padded_steps == 0
    for _ in range(src.padded_steps):
        out = src.empty_batch()
        src.draw_padded_into(*out)
        yield out


def _eager_padded_score(model, n, dtype=torch.float32, train_mode=False, **kw):
    """`score_fused` over the padded batches of a source of its own, with the model in eval mode (or, on request, in
    train mode); the model's mode is put back."""
    from dctn_amd.evaluation import score_fused

    was = model.training
    model.train(train_mode)
    try:
        return score_fused(model, _padded_batches(_source(n, dtype, **kw)), DEV)
    finally:
        model.train(was)


def _graphed(model, n, dtype=torch.float32, **kw):
    from dctn_amd.evaluation import GraphedScore

    return GraphedScore(model, _source(n, dtype, **kw))


@pytest.mark.parametrize("n", [37, 48], ids=["tail_of_5", "no_tail"])
@pytest.mark.parametrize("name", list(RR.CASES))
def test_graphed_pass_equals_the_eager_padded_pass_bit_for_bit(name, n):
    model = _model(name)
    scorer = _graphed(model, n)
    assert scorer.src.padded_steps == 3 and scorer.src.state_dict()["batches_done"] == 0   # the warm-up batch is undone
    got = scorer()
    want = _eager_padded_score(model, n)
    print(f"\n{name} n={n}: graphed {got!r} eager padded {want!r}; rows {scorer.rows} correct {scorer.correct}")
    assert got == want
    assert scorer.rows == n and isinstance(scorer.rows, int) and isinstance(scorer.correct, int)
    assert scorer.correct / n == want[1]
    assert scorer() == want and scorer.src.state_dict()["batches_done"] == 2 * 3      # a second pass: the same walk


def _all_inputs(n, batch=GLOBAL):
    """(x, y) of all n samples on the CPU, x being the very float32 values the source hands the model."""
    short = list(_source(n, batch=batch, drop_last=False))
    return torch.cat([b[0] for b in short], dim=1).cpu(), torch.cat([b[1] for b in short]).cpu()


@functools.lru_cache(maxsize=None)
def _oracle(name, n):
    """Float64 logits of the model case on all n samples (CPU), computed once and shared; nobody writes into it."""
    model = _model(name)
    x, y = _all_inputs(n)
    *cores, weight, bias = [p.detach().cpu().double() for p in _params(model)]
    with torch.no_grad():
        return R.eps_plus_linear_forward(cores, weight, bias, x.double()), y, x


@pytest.mark.parametrize("name", list(RR.CASES))
def test_padding_rows_count_for_nothing_against_torch_on_the_short_batches(name):
    """`score` (torch ops) over the eager `drop_last=False` source sees a last batch of 5 rows; the graphed pass sees 16
    with 11 labelled -100.  Accuracy: equal exactly where no logit row has tied maxima.  That is checked here, for the
    models and data of this test, on the float64 logits: in every row the best class leads the second by more than twice
    the largest error of the model's float32 logits in that row, so every argmax within that error picks the same class
    (the seeds are the cases' own; a seed that brought a tie would fail this assertion, not the comparison).  Loss: the
    rule of test_scoring_between_replays_leaves_the_training_counters_alone - the distance from the float64 oracle's
    mean cross-entropy is at most twice that of torch's own float32 arithmetic - and the same rule against the float64
    cross-entropy of the very logits both scored."""
    from dctn_amd.evaluation import score

    n = 37
    model = _model(name)
    want64, y, x = _oracle(name, n)
    with torch.no_grad():
        logits = model.eval()(x.to(DEV)).cpu().double()
    model.train()
    err = (logits - want64).abs().max(dim=1).values
    top2 = want64.topk(2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    print(f"\n{name}: smallest lead of the best class {float(margin.min()):.3e}, largest logit error {float(err.max()):.3e}")
    assert bool((margin > 2 * err).all())
    correct64 = int((want64.argmax(dim=1) == y).sum())
    ref = float(F.cross_entropy(want64, y, reduction="sum")) / n
    scorer = _graphed(model, n)
    loss_graphed, acc_graphed = scorer()
    sequential = _source(n, drop_last=False)
    assert [len(b[1]) for b in sequential] == [16, 16, 5]
    model.eval()
    loss_torch, acc_torch = score(model, sequential, DEV)
    ce_of_logits = float(F.cross_entropy(logits, y, reduction="sum")) / n
    print(f"{name}: graphed {loss_graphed!r} torch {loss_torch!r} float64 oracle {ref!r} (float64 CE of the model's own "
          f"logits {ce_of_logits!r}); accuracy graphed {acc_graphed} torch {acc_torch} oracle {correct64}/{n}")
    assert scorer.rows == n and scorer.correct == correct64
    assert acc_graphed == acc_torch == correct64 / n
    assert abs(loss_graphed - ref) <= 2 * abs(loss_torch - ref)
    assert abs(loss_graphed - ce_of_logits) <= 2 * abs(loss_torch - ce_of_logits)   # the same rule on the model's own logits


@pytest.mark.parametrize("name", list(RR.CASES))
def test_without_a_tail_the_pass_is_the_whole_batch_walk_of_the_plain_draw(name):
    """n = 48: the same kernels on the same shapes in the same order as `score_fused` over a sequential source that drops
    its (empty) remainder."""
    from dctn_amd.evaluation import score_fused

    model = _model(name)
    got = _graphed(model, 48)()
    plain = _source(48, drop_last=True)
    assert len(plain) == 3
    want = score_fused(model.eval(), plain, DEV)
    assert got == want


def _training(dtype=BF16, p=0.9, n=37):
    """cfg2 in bfloat16 with fused dropout, `FlatAdam` on master weights and a training source of its own, as one
    `GraphedTrainStep`."""
    from dctn_amd.training import FlatAdam, GraphedTrainStep, fused_cross_entropy

    case = RR.CASES["cfg2"]
    model = _model("cfg2", dtype, p)
    model.use_fused_dropout(case.dropout_seed)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-2, weight_decay=1e-3, l2=1e-2,
                   master_weights=dtype == BF16)
    train_src = _source(n, dtype, shuffle=True, data_seed=5)
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=train_src)
    return model, opt, train_src, step


def _counters(model, opt, train_src):
    return opt.t, model.dropout_state_dict()["draws_done"], train_src.state_dict()["batches_done"]


def test_the_graph_reads_the_live_weights():
    model, opt, train_src, step = _training()
    scorer = _graphed(model, 37, BF16)
    first = scorer()
    assert first == _eager_padded_score(model, 37, BF16)
    for _ in range(3):
        step()
    second = scorer()
    print(f"\nbefore {first!r}, after three training replays {second!r}")
    assert second == _eager_padded_score(model, 37, BF16)
    assert second != first
    assert model.training and _counters(model, opt, train_src) == (4, 4, 4)


def test_passes_between_training_replays_change_nothing_of_the_training():
    model, opt, train_src, step = _training()
    twin_model, twin_opt, twin_src, twin_step = _training()
    scorer = _graphed(model, 37, BF16)
    for k in range(6):
        step()
        twin_step()
        if k % 2 == 1:
            scorer()
    torch.cuda.synchronize()
    for a, b in ((opt.flat, twin_opt.flat), (opt.master, twin_opt.master), (opt.m, twin_opt.m), (opt.v, twin_opt.v)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for a, b in zip(_params(model), _params(twin_model)):
        assert torch.equal(a, b)
    assert _counters(model, opt, train_src) == _counters(twin_model, twin_opt, twin_src) == (7, 7, 7)
    assert model.dropout_state_dict() == twin_model.dropout_state_dict()
    done = scorer.src.state_dict()["batches_done"]
    assert done == 3 * scorer.src.padded_steps and done % scorer.src.padded_steps == 0


@pytest.mark.parametrize("training", [True, False], ids=["from_train_mode", "from_eval_mode"])
def test_the_pass_runs_in_eval_mode_and_restores_the_mode(training):
    from dctn_amd.evaluation import GraphedScore

    model = _model("cfg2")           # p = 0.75
    model.use_fused_dropout(77)
    model.train(training)
    scorer = GraphedScore(model, _source(37))
    assert model.training is training
    got = scorer()
    assert model.training is training and model.dropout_state_dict() == {"seed": 77, "draws_done": 0}
    in_eval = _eager_padded_score(model, 37)
    in_train = _eager_padded_score(model, 37, train_mode=True)
    print(f"\ngraphed {got!r}, eager in eval mode {in_eval!r}, eager in train mode {in_train!r}")
    assert got == in_eval and got != in_train
    assert model.training is training


def test_launch_does_not_block_and_scores_the_weights_of_its_moment():
    model, opt, train_src, step = _training()
    scorer = _graphed(model, 37, BF16)
    step()
    saved = [p.detach().clone() for p in _params(model)]
    scorer.launch()
    step()
    step()
    got = scorer.read()
    frozen = _model("cfg2", BF16, 0.9, seed=99)
    with torch.no_grad():
        for p, value in zip(_params(frozen), saved):
            p.copy_(value)
    want = _eager_padded_score(frozen, 37, BF16)
    now = _eager_padded_score(model, 37, BF16)
    print(f"\nread after two more replays {got!r}; eager on the clone {want!r}; eager on the weights now {now!r}")
    assert got == want and got != now and scorer.rows == 37


# ------------------------------------------------------------------ two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.evaluation import GraphedScore

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    scorer = GraphedScore(_model("cfg2"), _source(10, batch=4, rank=rank, world=world))
    result = scorer()
    local = scorer.src.expected_padded_indices(2)
    q.put((rank, result, scorer.rows, scorer.correct, local))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_a_pass_whose_last_batch_leaves_one_of_them_only_padding():
    import torch.multiprocessing as mp

    n = 10
    ctx = mp.get_context("spawn")   # fresh child processes
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {rank: rest for rank, *rest in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    model = _model("cfg2")
    single = _graphed(model, n, batch=4)
    loss, acc = single()
    x, y = _all_inputs(n, batch=4)
    with torch.no_grad():
        ce = F.cross_entropy(model.eval()(x.to(DEV)).cpu().double(), y, reduction="none")
    bound = n * 2.0 ** -52 * float(ce.abs().sum())   # re-association of n float64 terms
    print(f"\nsingle process {loss!r} {acc}; ranks {got[0][0]!r} {got[1][0]!r}; |difference| "
          f"{abs(got[0][0][0] - loss):.3e}, bound {bound:.3e}")
    assert got[0][3] == [8, 9] and got[1][3] == [-1, -1]
    assert got[0][:3] == got[1][:3]
    assert got[0][1] == single.rows == n and got[0][2] == single.correct and got[0][0][1] == acc
    assert abs(got[0][0][0] - loss) <= bound


# ------------------------------------------------------------------ the hook
def test_the_hook_fills_the_four_keys_the_checkpointers_read(tmp_path):
    from dctn_amd.evaluation import GraphedScore, make_evaluation_hook
    from dctn_amd.training import (FlatAdam, LastModelsCheckpointer, _checkpoint_tag, every_n_iters_intervals,
                                   fused_cross_entropy, make_stopper_after_n_iters, train)

    model = _model("cfg2", p=1.0)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-2)
    at_start = (_eager_padded_score(model, 37), _eager_padded_score(model, 48, data_seed=1))
    hook = make_evaluation_hook(GraphedScore(model, _source(37)), GraphedScore(model, _source(48, data_seed=1)))
    schedule = every_n_iters_intervals((None, 2))
    seen = []

    def note(st_x, st_it):
        seen.append({k: st_it.get(k) for k in ("num_iters_done", "train_mean_ce", "train_acc", "val_mean_ce", "val_acc")})

    zero = torch.zeros((), device=DEV)
    train(_source(37, shuffle=True, data_seed=5), model, opt, DEV, fused_cross_entropy, lambda st_x, st_it: zero, 0.0,
          [schedule(hook), note], [], [schedule(LastModelsCheckpointer(str(tmp_path), 2)), make_stopper_after_n_iters(3)])
    assert [s["num_iters_done"] for s in seen] == [0, 1, 2, 3]
    assert all(v is None for k, v in seen[1].items() if k != "num_iters_done") and seen[3]["val_acc"] is None
    assert (seen[0]["train_mean_ce"], seen[0]["train_acc"]) == at_start[0]
    assert (seen[0]["val_mean_ce"], seen[0]["val_acc"]) == at_start[1]
    assert (seen[2]["train_mean_ce"], seen[2]["val_mean_ce"]) != (seen[0]["train_mean_ce"], seen[0]["val_mean_ce"])
    assert sorted(os.listdir(tmp_path)) == [f"model_{_checkpoint_tag(seen[k])}.pth" for k in (0, 2)]
