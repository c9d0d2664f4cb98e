"""The device batch source on the GPU (`-m gpu`): the raw C-ABI against the Python restatement of the order and torch's
own indexing on the CPU (bit for bit, inside guarded buffers), the device counter across an epoch boundary, the
reference's formulation of the feature map, two shards of one global batch, graph replay (alone and as the first node of
a GraphedTrainStep), resume, the sequential form under `score_fused`, and `training.train(dl=src)`."""
import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd import batches as B
from dctn_amd.window_stats import φ_cos_sin_squared_1 as PHI

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234567890ABCDEF
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
NAME = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16"}
GUARD, GUARD_BYTE, STALE_BYTE = 256, 0xA5, 0xFF   # guard bytes on both sides; what an output holds before the launch


class Framed:
    """A tensor inside a guarded byte allocation.  An output (``values`` None) starts as 0xFF bytes (NaN in every float
    dtype, -1 in int64); ``shift`` moves the base off its 256-byte alignment by that many bytes."""

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


def _data(n, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, generator=g)
    images[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    return images, torch.randint(0, 10, (n,), generator=g)


def _table(Q, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(256, Q, generator=g, dtype=torch.float64).to(dtype)


# ------------------------------------------------------------------ 1. the raw ABI
N, G, K0 = 37, 8, 6   # draw 6 of S = 4: epoch 1, second batch


@pytest.mark.parametrize("op", ["draw", "gather"])
@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("Q", [2, 3])
@pytest.mark.parametrize("size,shift", [(5, 0), (28, 0), (28, 1)], ids=["5x5_bytes", "28x28_words", "28x28_base_off_by_one"])
def test_raw_abi_u8_table(size, shift, Q, dtype, op):
    images, labels = _data(N, size, size)
    table = _table(Q, dtype)
    P = size * size
    idx = B.expected_indices(SEED, K0, N, G)
    src = Framed((N, P), torch.uint8, images.view(N, P), shift=shift)
    tab, lab = Framed((256, Q), dtype, table), Framed((N,), torch.int64, labels)
    x, y, ind = Framed((1, G, P, Q), dtype), Framed((G,), torch.int64), Framed((G,), torch.int64)
    state = B._new_state(SEED, DEV, K0)
    if op == "draw":
        rc = L.lib().dctn_batch_draw(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(), x.view.data_ptr(),
                                     y.view.data_ptr(), ind.view.data_ptr(), state.data_ptr(), N, G, G, 0, P, Q,
                                     L.BATCH_SRC_U8_TABLE, 0, L.dtype_code(table), L.stream_ptr(DEV))
    else:
        given = Framed((G,), torch.int64, torch.tensor(idx))
        rc = L.lib().dctn_batch_gather(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(),
                                       given.view.data_ptr(), x.view.data_ptr(), y.view.data_ptr(), ind.view.data_ptr(),
                                       N, G, P, Q, L.BATCH_SRC_U8_TABLE, L.dtype_code(table), L.stream_ptr(DEV))
    assert rc == 0
    assert dctn_amd.last_kernel() == f"batch_{op}_u8_{NAME[dtype]}"
    torch.cuda.synchronize()
    want = table[images[idx].view(G, P).long()].unsqueeze(0)
    assert torch.equal(_bits(x.view.cpu()), _bits(want))
    assert y.view.cpu().tolist() == labels[idx].tolist() and ind.view.cpu().tolist() == idx
    assert x.guards_intact() and y.guards_intact() and ind.guards_intact()
    assert src.untouched() and tab.untouched() and lab.untouched()
    if op == "draw":
        assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, K0 + 1, 0]
    else:
        assert given.untouched() and _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, K0, 0]


@pytest.mark.parametrize("op", ["draw", "gather"])
@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
# 18: no dtype but float64 has rows of whole 16-byte pieces; 16: all have; 2104: more pieces than one pass of a wave takes
@pytest.mark.parametrize("R", [18, 16, 2104])
def test_raw_abi_rows(R, dtype, op):
    C = 2
    g = torch.Generator().manual_seed(2)
    x_full = torch.randn(C, N, R, generator=g, dtype=torch.float64).to(dtype)
    labels = torch.randint(0, 10, (N,), generator=g)
    idx = B.expected_indices(SEED, K0, N, G)
    src, lab = Framed((C, N, R), dtype, x_full), Framed((N,), torch.int64, labels)
    x, y, ind = Framed((C, G, R), dtype), Framed((G,), torch.int64), Framed((G,), torch.int64)
    state = B._new_state(SEED, DEV, K0)
    if op == "draw":
        rc = L.lib().dctn_batch_draw(src.view.data_ptr(), None, lab.view.data_ptr(), x.view.data_ptr(), y.view.data_ptr(),
                                     ind.view.data_ptr(), state.data_ptr(), N, G, G, 0, R, C, L.BATCH_SRC_ROWS, 0,
                                     L.dtype_code(x_full), L.stream_ptr(DEV))
    else:
        given = Framed((G,), torch.int64, torch.tensor(idx))
        rc = L.lib().dctn_batch_gather(src.view.data_ptr(), None, lab.view.data_ptr(), given.view.data_ptr(),
                                       x.view.data_ptr(), y.view.data_ptr(), ind.view.data_ptr(), N, G, R, C,
                                       L.BATCH_SRC_ROWS, L.dtype_code(x_full), L.stream_ptr(DEV))
    assert rc == 0
    assert dctn_amd.last_kernel() == f"batch_{op}_rows_{NAME[dtype]}"
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.view.cpu()), _bits(x_full[:, idx]))
    assert y.view.cpu().tolist() == labels[idx].tolist() and ind.view.cpu().tolist() == idx
    assert x.guards_intact() and y.guards_intact() and ind.guards_intact()
    assert src.untouched() and lab.untouched()
    assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, K0 + (op == "draw"), 0]


def test_identity_flag_and_a_shard_offset():
    images, labels = _data(N, 5, 5)
    src = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED, shuffle=False, rank=1, world=2)
    src.load_state_dict({"seed": SEED, "batches_done": 6})   # (6 % 4) * 8 + 1 * 4
    _, y, ind = src.draw()
    assert ind.tolist() == [20, 21, 22, 23] == src.expected_indices(6) and y.tolist() == labels[20:24].tolist()


def test_more_samples_than_waves_and_single_column_tables():
    """2100 samples in one launch: the grid is capped, so waves take several samples; Q = 1 and Q = 4."""
    n, Gb = 2500, 2100
    images, labels = _data(n, 6, 6, seed=3)
    for Q, dtype in ((1, torch.bfloat16), (4, torch.float64), (1, torch.float32), (4, torch.bfloat16)):
        phi = tuple((lambda u, c=c: u * (c + 1.0) - 0.25) for c in range(Q))
        src = B.DeviceBatches(images, labels, Gb, dtype=dtype, seed=5, phi=phi)
        x, y, ind = src.draw()
        idx = B.expected_indices(5, 0, n, Gb)
        assert ind.tolist() == idx and y.tolist() == labels[idx].tolist()
        want = B.feature_table(phi, 1.0, dtype)[images[idx].long()].unsqueeze(0)
        assert x.shape == (1, Gb, 6, 6, Q) and torch.equal(_bits(x.cpu()), _bits(want))
        assert _words(src._state)[2:] == [1, 0]


def test_rows_beyond_four_gibibytes():
    """The byte offset of a row is 64-bit arithmetic: a source of more than 2^32 bytes, rows at both ends."""
    P = 4096
    n = (1 << 20) + 8
    src = torch.empty((n, P), dtype=torch.uint8, device=DEV)
    picks = [0, n - 1, (1 << 20) + 3, 77]
    g = torch.Generator().manual_seed(4)
    rows = torch.randint(0, 256, (len(picks), P), dtype=torch.uint8, generator=g)
    src[torch.tensor(picks, device=DEV)] = rows.to(DEV)
    labels = torch.zeros(n, dtype=torch.int64, device=DEV)
    labels[torch.tensor(picks, device=DEV)] = torch.tensor([3, 1, 4, 1], device=DEV)
    table = _table(2, torch.bfloat16).to(DEV)
    given = torch.tensor(picks, device=DEV)
    x = torch.empty((1, 4, P, 2), dtype=torch.bfloat16, device=DEV)
    y, ind = torch.empty(4, dtype=torch.int64, device=DEV), torch.empty(4, dtype=torch.int64, device=DEV)
    assert L.lib().dctn_batch_gather(src.data_ptr(), table.data_ptr(), labels.data_ptr(), given.data_ptr(), x.data_ptr(),
                                     y.data_ptr(), ind.data_ptr(), n, 4, P, 2, L.BATCH_SRC_U8_TABLE, L.BF16,
                                     L.stream_ptr(DEV)) == 0
    assert torch.equal(_bits(x.cpu()), _bits(table.cpu()[rows.long()].unsqueeze(0)))
    assert y.tolist() == [3, 1, 4, 1] and ind.tolist() == picks


# ------------------------------------------------------------------ 2. the epoch boundary
def test_ten_draws_cross_two_epoch_boundaries():
    images, labels = _data(N, 5, 5)
    src = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED)
    assert len(src) == 4
    draws = [src.draw()[2].tolist() for _ in range(10)]
    assert draws == [src.expected_indices(k) for k in range(10)]
    first_epoch = sum(draws[:4], [])
    assert len(set(first_epoch)) == 32
    assert draws[4] == B.order(SEED, 1, N)[:8] and draws[8] == B.order(SEED, 2, N)[:8]
    assert src.state_dict() == {"seed": SEED, "batches_done": 10} and _words(src._state)[3] == 0


def test_one_step_per_epoch_gives_a_full_permutation_every_draw():
    n = 1000
    images, labels = _data(n, 2, 2)
    src = B.DeviceBatches(images, labels, n, dtype=torch.bfloat16, seed=SEED)
    assert len(src) == 1
    seen = []
    for epoch in range(3):
        ind = src.draw()[2].tolist()
        assert sorted(ind) == list(range(n)) and ind == B.order(SEED, epoch, n)
        seen.append(ind)
    assert seen[0] != seen[1] != seen[2]


# ------------------------------------------------------------------ 3. the reference's formulation
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.float64, 2e-6), (torch.bfloat16, 2 ** -7)],
                         ids=list(NAME.values()))
def test_against_the_feature_map_applied_to_the_whole_data_set(dtype, tol):
    nu = 1.46
    images, labels = _data(N, 28, 28)
    src = B.DeviceBatches(images, labels, G, dtype=dtype, seed=SEED, scale=nu)
    x, _, ind = src.draw()
    idx = ind.tolist()
    # dctn/dataset_loading.py:60-63, the runner's `x *= scale`, the cast, then the batch
    full = (torch.stack(tuple(f(images.float() / 255.0) for f in PHI), dim=3).unsqueeze(0) * nu).to(dtype)
    want = full[:, idx]
    err = float((x.cpu().double() - want.double()).abs().max())
    print(f"{NAME[dtype]}: max abs difference {err:.3e}, bound {2 * tol * nu:.3e}")
    assert x.shape == (1, G, 28, 28, 2) and err <= 2 * tol * nu


# ------------------------------------------------------------------ 4. two shards
def test_two_shards_make_the_global_batch():
    images, labels = _data(N, 5, 5)
    kw = dict(dtype=torch.float32, seed=SEED)
    whole = B.DeviceBatches(images, labels, G, **kw)
    parts = [B.DeviceBatches(images, labels, G, rank=r, world=2, **kw) for r in range(2)]
    assert [p.local_batch for p in parts] == [4, 4]
    for k in range(5):   # crosses the epoch boundary
        x, y, ind = whole.draw()
        xs, ys, inds = zip(*(p.draw() for p in parts))
        assert torch.equal(torch.cat(xs, dim=1), x) and torch.equal(torch.cat(ys), y) and torch.equal(torch.cat(inds), ind)
        assert ind.tolist() == whole.expected_indices(k) and inds[1].tolist() == parts[1].expected_indices(k)
    with pytest.raises(ValueError):
        B.DeviceBatches(images, labels, 9, rank=0, world=2, **kw)


def test_from_features_moves_the_rows():
    g = torch.Generator().manual_seed(6)
    x_full = torch.randn(3, N, 4, 4, 2, generator=g).to(torch.bfloat16)
    labels = torch.randint(0, 10, (N,), generator=g)
    src = B.DeviceBatches.from_features(x_full, labels, G, seed=SEED)
    for k in range(5):
        x, y, ind = src.draw()
        idx = src.expected_indices(k)
        assert ind.tolist() == idx and y.tolist() == labels[idx].tolist()
        assert x.shape == (3, G, 4, 4, 2) and torch.equal(_bits(x.cpu()), _bits(x_full[:, idx]))
    assert dctn_amd.last_kernel() == "batch_draw_rows_bf16"


# ------------------------------------------------------------------ 5. graphs
def test_a_captured_draw_follows_the_counter_on_its_replays():
    images, labels = _data(N, 28, 28)
    kw = dict(dtype=torch.bfloat16, seed=SEED)
    src, eager = B.DeviceBatches(images, labels, G, **kw), B.DeviceBatches(images, labels, G, **kw)
    x, y, ind = src.empty_batch()
    src.draw_into(x, y, ind)                  # draw 0, eagerly
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        src.draw_into(x, y, ind)
    assert src.state_dict()["batches_done"] == 1          # the capture itself launches nothing
    eager.draw()
    for k in range(1, 6):
        graph.replay()
        ex, ey, eind = eager.draw()
        assert ind.tolist() == src.expected_indices(k) == eind.tolist()
        assert torch.equal(_bits(x), _bits(ex)) and torch.equal(y, ey)
    assert src.state_dict() == eager.state_dict() == {"seed": SEED, "batches_done": 6}


def _model(seed=3):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, DEV, torch.float32, image_size=28)


def _flat_adam(model):
    from dctn_amd.training import FlatAdam

    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3, l2=1e-2)


def test_graphed_train_step_with_a_batch_source_equals_the_same_steps_fed_by_hand():
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    images, labels = _data(N, 28, 28)
    kw = dict(dtype=torch.float32, seed=SEED, scale=0.8)
    src, hand_src = B.DeviceBatches(images, labels, G, **kw), B.DeviceBatches(images, labels, G, **kw)
    m = _model()
    opt = _flat_adam(m)
    step = GraphedTrainStep(m, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src)
    assert src.state_dict()["batches_done"] == 1          # the warm-up trained on draw 0
    seen = []
    for _ in range(3):
        out = step()
        seen.append(out["indices"].tolist())
    assert set(out) == {"output", "loss", "reg_term", "indices"}
    assert seen == [src.expected_indices(k) for k in (1, 2, 3)]
    assert src.state_dict() == {"seed": SEED, "batches_done": 4}
    with pytest.raises(TypeError):
        step(step.x, step.y)

    def by_hand(k):
        return hand_src.gather(torch.tensor(hand_src.expected_indices(k), device=DEV))[:2]

    h = _model()
    hopt = _flat_adam(h)
    hstep = GraphedTrainStep(h, *by_hand(0), fused_cross_entropy, hopt, warmup=1)
    for k in (1, 2, 3):
        hout = hstep(*by_hand(k))
    with pytest.raises(TypeError):
        hstep()
    torch.cuda.synchronize()
    assert set(hout) == {"output", "loss", "reg_term"}
    assert hopt.t == opt.t == 4
    assert torch.equal(hopt.flat, opt.flat) and torch.equal(hopt.m, opt.m) and torch.equal(hopt.v, opt.v)
    assert torch.equal(hout["loss"], out["loss"])


# ------------------------------------------------------------------ 6. resume
def test_a_loaded_state_repeats_the_next_batches():
    images, labels = _data(N, 5, 5)
    kw = dict(dtype=torch.float32)
    src = B.DeviceBatches(images, labels, G, seed=SEED, **kw)
    for _ in range(3):
        src.draw()
    saved = src.state_dict()
    assert saved == {"seed": SEED, "batches_done": 3}
    nxt = [src.draw() for _ in range(3)]
    fresh = B.DeviceBatches(images, labels, G, seed=99, **kw)
    fresh.load_state_dict(saved)
    assert fresh.state_dict() == saved and fresh.expected_indices(3) == nxt[0][2].tolist()
    for x, y, ind in nxt:
        fx, fy, find = fresh.draw()
        assert torch.equal(fx, x) and torch.equal(fy, y) and torch.equal(find, ind)
    buffers = fresh.empty_batch()
    fresh.draw_into(*buffers)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fresh.draw_into(*buffers)
        with pytest.raises(RuntimeError, match="capture"):
            fresh.load_state_dict(saved)
    graph.replay()
    assert fresh.state_dict()["batches_done"] == 8


# ------------------------------------------------------------------ 7. the sequential form
def test_sequential_passes_and_fused_scoring():
    from dctn_amd.evaluation import score_fused

    images, labels = _data(N, 28, 28)
    src = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED, shuffle=False, drop_last=False)
    assert len(src) == 5
    for _ in range(2):   # every pass is the same walk
        batches = list(src)
        assert [len(b[1]) for b in batches] == [8, 8, 8, 8, 5]
        assert torch.cat([b[2] for b in batches]).tolist() == list(range(N))
        assert torch.equal(torch.cat([b[1] for b in batches]).cpu(), labels)
    x_full = B.feature_table(PHI, 1.0, torch.float32)[images.long()].unsqueeze(0)
    assert torch.equal(torch.cat([b[0] for b in batches], dim=1).cpu(), x_full)
    by_hand = [(x_full[:, a : a + G].to(DEV), labels[a : a + G].to(DEV), torch.arange(a, min(a + G, N))) for a in range(0, N, G)]
    m = _model().eval()
    assert score_fused(m, src, DEV) == score_fused(m, by_hand, DEV)
    # two ranks split every batch, the short one too: together they see each sample once
    halves = [B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED, shuffle=False, drop_last=False, rank=r,
                              world=2) for r in range(2)]
    seen = sorted(i for h in halves for b in h for i in b[2].tolist())
    assert seen == list(range(N))
    # the shuffled source drops the remainder: 4 batches a pass, the counter runs on
    train_src = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED)
    assert [b[2].tolist() for b in train_src] == [train_src.expected_indices(k) for k in range(4)]
    assert [b[2].tolist() for b in train_src] == [train_src.expected_indices(k) for k in range(4, 8)]


# ------------------------------------------------------------------ 8. training.train
def test_train_takes_the_source_as_its_loader():
    from dctn_amd.training import fused_cross_entropy, make_stopper_after_n_iters, train

    images, labels = _data(N, 28, 28)
    src = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED)
    m = _model()
    opt = _flat_adam(m)
    before = opt.flat.clone()
    zero = torch.zeros((), device=DEV)
    _, st_it = train(src, m, opt, DEV, fused_cross_entropy, lambda st_x, st_it: zero, 0.0, [], [],
                     [make_stopper_after_n_iters(2)])
    assert st_it["num_iters_done"] == 2 and st_it["indices"].tolist() == src.expected_indices(2)
    assert st_it["x"].shape == (1, G, 28, 28, 2) and st_it["y"].tolist() == labels[src.expected_indices(2)].tolist()
    assert src.state_dict()["batches_done"] == 3 and not torch.equal(opt.flat, before)
    assert bool(torch.isfinite(st_it["loss"]))
