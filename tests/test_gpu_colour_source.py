"""The colour batch source on the GPU (`-m gpu`): the raw C-ABI of dctn_batch_draw_cols / dctn_batch_gather_cols against
the Python restatement of the order and torch's own indexing on the CPU (bit for bit, inside guarded buffers, on every
path of the kernel), the flags and the shards, more samples than waves, the reference's colour pipeline applied to the
whole expanded data set, graph replay, resume, and the source as the first node of a GraphedTrainStep and under
GraphedScore."""
import functools

import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd import batches as B

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234567890ABCDEF
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
NAME = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16"}
GUARD, GUARD_BYTE, STALE_BYTE = 256, 0xA5, 0xFF   # guard bytes on both sides; what an output holds before the launch


class Framed:
    """A tensor inside a guarded byte allocation (the pattern of tests/test_gpu_batches.py).  An output (``values`` None)
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


def _data(n, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * C)
    images = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, generator=g)
    images[0, 0, 0, :] = 0
    images[0, 0, 1, :] = 255
    return images, torch.randint(0, 10, (n,), generator=g)


def _table(W, dtype, seed=1):
    """(W, 256) of unrelated values: every (channel, byte) pair has its own, so a mixed-up channel or byte shows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(W, 256, generator=g, dtype=torch.float64).to(dtype)


def _lookup(table, images):
    """(count, H, W, C) bytes -> (1, count, H * W, Wout) on the CPU: x[0, j, p, c] = table[c][byte], table[c][0] for c >= C."""
    count, C = images.shape[0], images.shape[-1]
    flat = images.reshape(count, -1, C).long()
    cols = [table[c][flat[..., c]] for c in range(C)]
    cols += [table[c][torch.zeros_like(flat[..., 0])] for c in range(C, table.shape[0])]
    return torch.stack(cols, dim=-1).unsqueeze(0)


# ------------------------------------------------------------------ 1. the raw ABI
N, G, K0 = 37, 8, 6   # draw 6 of S = 4: epoch 1, second batch

# 5x5: P odd, the pixel path; 8x8: 16 groups of four pixels, fewer than a wave; 36x36: 324 groups, one full unrolled pass of
# a wave (256) and a ragged one; 8x8 with the source one byte off its alignment: an aligned shape on the pixel path
SHAPES = [(5, 0, 3, 3), (5, 0, 3, 4), (8, 0, 3, 3), (8, 0, 3, 4), (36, 0, 3, 3), (36, 0, 3, 4), (8, 1, 3, 3), (8, 1, 3, 4),
          (8, 0, 1, 1), (8, 0, 1, 2), (8, 0, 2, 3), (8, 0, 4, 4)]


@pytest.mark.parametrize("op", ["draw", "gather"])
@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("size,shift,C,W", SHAPES,
                         ids=[f"{s}x{s}_C{c}_W{w}" + ("_base_off_by_one" if sh else "") for s, sh, c, w in SHAPES])
def test_raw_abi(size, shift, C, W, dtype, op):
    images, labels = _data(N, size, size, C)
    table = _table(W, dtype)
    P = size * size
    idx = B.expected_indices(SEED, K0, N, G)
    src = Framed((N, P, C), torch.uint8, images.view(N, P, C), shift=shift)
    tab, lab = Framed((W, 256), dtype, table), Framed((N,), torch.int64, labels)
    x, y, ind = Framed((1, G, P, W), dtype), Framed((G,), torch.int64), Framed((G,), torch.int64)
    state = B._new_state(SEED, DEV, K0)
    if op == "draw":
        rc = L.lib().dctn_batch_draw_cols(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(), x.view.data_ptr(),
                                          y.view.data_ptr(), ind.view.data_ptr(), state.data_ptr(), N, G, G, 0, P, C, W, 0,
                                          L.dtype_code(table), L.stream_ptr(DEV))
    else:
        given = Framed((G,), torch.int64, torch.tensor(idx))
        rc = L.lib().dctn_batch_gather_cols(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(),
                                            given.view.data_ptr(), x.view.data_ptr(), y.view.data_ptr(),
                                            ind.view.data_ptr(), N, G, P, C, W, L.dtype_code(table), L.stream_ptr(DEV))
    assert rc == 0
    assert dctn_amd.last_kernel() == f"colour_{op}_{NAME[dtype]}"
    torch.cuda.synchronize()
    want = _lookup(table, images[idx])
    assert want.shape == (1, G, P, W)
    assert torch.equal(_bits(x.view.cpu()), _bits(want))
    assert y.view.cpu().tolist() == labels[idx].tolist() and ind.view.cpu().tolist() == idx
    assert x.guards_intact() and y.guards_intact() and ind.guards_intact()
    assert src.untouched() and tab.untouched() and lab.untouched()
    if op == "draw":
        assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, K0 + 1, 0]
    else:
        assert given.untouched() and _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, K0, 0]


def test_x_off_its_store_alignment_takes_the_pixel_path():
    """bf16 with W = 3 stores 8 bytes at a time: an x base 2 bytes off (its element size) must still come out right."""
    images, labels = _data(N, 8, 8, 3)
    table = _table(3, torch.bfloat16)
    idx = B.expected_indices(SEED, K0, N, G)
    src, tab = Framed((N, 64, 3), torch.uint8, images.view(N, 64, 3)), Framed((3, 256), torch.bfloat16, table)
    lab = Framed((N,), torch.int64, labels)
    x, y, ind = Framed((1, G, 64, 3), torch.bfloat16, shift=2), Framed((G,), torch.int64), Framed((G,), torch.int64)
    state = B._new_state(SEED, DEV, K0)
    assert L.lib().dctn_batch_draw_cols(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(), x.view.data_ptr(),
                                        y.view.data_ptr(), ind.view.data_ptr(), state.data_ptr(), N, G, G, 0, 64, 3, 3, 0,
                                        L.BF16, L.stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.view.cpu()), _bits(_lookup(table, images[idx]))) and ind.view.cpu().tolist() == idx
    assert x.guards_intact() and src.untouched() and tab.untouched()


# ------------------------------------------------------------------ 2. the flags and the shards
NU = (1.46, 0.83, 1.21)


def test_identity_flag_and_a_shard_offset():
    images, labels = _data(N, 5, 5, 3)
    src = B.DeviceBatches.from_colour(images, labels, G, dtype=torch.float32, seed=SEED, nu=NU, shuffle=False, rank=1,
                                      world=2)
    src.load_state_dict({"seed": SEED, "batches_done": 6})   # (6 % 4) * 8 + 1 * 4
    x, y, ind = src.draw()
    assert ind.tolist() == [20, 21, 22, 23] == src.expected_indices(6) and y.tolist() == labels[20:24].tolist()
    want = _lookup(B.colour_table(3, nu=NU, dtype=torch.float32), images[20:24]).view(1, 4, 5, 5, 3)
    assert torch.equal(_bits(x.cpu()), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
def test_padded_pass_raw_abi(dtype):
    """n = 10, G = 4: S = 3 draws a pass; the third has two padding slots (the row of sample n - 1, label -100, index -1),
    and three draws leave the counter at 0 mod 3 again."""
    n, Gp, C, W, P = 10, 4, 3, 4, 16
    images, labels = _data(n, 4, 4, C, seed=5)
    table = _table(W, dtype)
    src, tab = Framed((n, P, C), torch.uint8, images.view(n, P, C)), Framed((W, 256), dtype, table)
    lab = Framed((n,), torch.int64, labels)
    state = B._new_state(SEED, DEV, 3)   # 3 = 0 mod S
    flags = L.BATCH_IDENTITY_ORDER | L.BATCH_PAD_TAIL
    for k in range(3):
        x, y, ind = Framed((1, Gp, P, W), dtype), Framed((Gp,), torch.int64), Framed((Gp,), torch.int64)
        assert L.lib().dctn_batch_draw_cols(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(),
                                            x.view.data_ptr(), y.view.data_ptr(), ind.view.data_ptr(), state.data_ptr(), n,
                                            Gp, Gp, 0, P, C, W, flags, L.dtype_code(table), L.stream_ptr(DEV)) == 0
        assert dctn_amd.last_kernel() == f"colour_draw_{NAME[dtype]}"
        torch.cuda.synchronize()
        idx = B.expected_padded_indices(k, n, Gp)
        rows = [i if i >= 0 else n - 1 for i in idx]
        assert torch.equal(_bits(x.view.cpu()), _bits(_lookup(table, images[rows]))), f"draw {k}"
        assert y.view.cpu().tolist() == [int(labels[i]) if i >= 0 else -100 for i in idx]
        assert ind.view.cpu().tolist() == idx
        assert x.guards_intact() and y.guards_intact() and ind.guards_intact()
    assert idx == [8, 9, -1, -1]
    assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, 6, 0] and 6 % 3 == 0
    assert src.untouched() and tab.untouched() and lab.untouched()
    # the flag rules of dctn_batch_draw
    assert L.lib().dctn_batch_draw_cols(src.view.data_ptr(), tab.view.data_ptr(), lab.view.data_ptr(), x.view.data_ptr(),
                                        y.view.data_ptr(), ind.view.data_ptr(), state.data_ptr(), n, Gp, Gp, 0, P, C, W,
                                        L.BATCH_PAD_TAIL, L.dtype_code(table), L.stream_ptr(DEV)) == L.ERR_BAD_SHAPE


def test_padded_pass_through_the_class():
    n, Gp = 10, 4
    images, labels = _data(n, 4, 4, 3, seed=5)
    src = B.DeviceBatches.from_colour(images, labels, Gp, dtype=torch.float32, seed=SEED, nu=NU, constant_channel=0.5,
                                      shuffle=False)
    assert src.padded_steps == 3
    seen = []
    for k in range(3):
        out = src.empty_batch()
        src.draw_padded_into(*out)
        assert out[2].tolist() == src.expected_padded_indices(k)
        seen += out[2].tolist()
    assert seen == list(range(10)) + [-1, -1] and out[1].tolist()[2:] == [-100, -100]
    assert torch.equal(out[0][0, 2], out[0][0, 1]) and torch.equal(out[0][0, 3], out[0][0, 1])   # sample n - 1 again
    assert src.state_dict()["batches_done"] == 3
    shuffled = B.DeviceBatches.from_colour(images, labels, Gp, dtype=torch.float32, seed=SEED, nu=NU)
    with pytest.raises(ValueError):
        shuffled.draw_padded_into(*shuffled.empty_batch())


def test_two_shards_make_the_global_batch():
    images, labels = _data(N, 5, 5, 3)
    kw = dict(dtype=torch.float32, seed=SEED, nu=NU, constant_channel=1.0)
    whole = B.DeviceBatches.from_colour(images, labels, G, **kw)
    parts = [B.DeviceBatches.from_colour(images, labels, G, rank=r, world=2, **kw) for r in range(2)]
    assert [p.local_batch for p in parts] == [4, 4]
    for k in range(5):   # crosses the epoch boundary
        x, y, ind = whole.draw()
        xs, ys, inds = zip(*(p.draw() for p in parts))
        assert torch.equal(torch.cat(xs, dim=1), x) and torch.equal(torch.cat(ys), y) and torch.equal(torch.cat(inds), ind)
        assert ind.tolist() == whole.expected_indices(k) and inds[1].tolist() == parts[1].expected_indices(k)


def test_more_samples_than_the_launch_has_waves():
    """1100 samples in one launch: the grid is capped at the number of CUs, so waves take several samples."""
    n, Gb = 1300, 1100
    images, labels = _data(n, 2, 2, 3, seed=3)
    src = B.DeviceBatches.from_colour(images, labels, Gb, dtype=torch.bfloat16, seed=5, nu=NU, constant_channel=0.25)
    x, y, ind = src.draw()
    idx = B.expected_indices(5, 0, n, Gb)
    assert ind.tolist() == idx and y.tolist() == labels[idx].tolist()
    table = B.colour_table(3, nu=NU, constant_channel=0.25, dtype=torch.bfloat16)
    assert x.shape == (1, Gb, 2, 2, 4) and torch.equal(_bits(x.cpu()), _bits(_lookup(table, images[idx]).view(x.shape)))
    assert _words(src._state)[2:] == [1, 0] and dctn_amd.last_kernel() == "colour_draw_bf16"


# ------------------------------------------------------------------ 3. the reference's formulation
def _pipeline(images, nu, mean, std, constant_channel):
    """The published formula on the WHOLE expanded tensor in the reference's order (dataset_loading.py:349-375): to_tensor's
    float32 u8 / 255 as (1, n, H, W, C); in place, minus the float64 channel means, over the float64 channel deviations; a
    concatenated constant channel; in place, times the float32 nu with 1.0 for the constant channel."""
    x = images.float().div(255).unsqueeze(0)
    x -= mean
    x /= std
    x = torch.cat((x, constant_channel * torch.ones_like(x[:, :, :, :, :1])), dim=4)
    x *= torch.tensor(nu + (1.0,))
    return x


@functools.lru_cache(maxsize=None)
def _expanded():
    """The data of section 3 and 6 and its float32 expansion on the CPU, computed once and shared; nobody writes into it."""
    images, labels = _data(N, 6, 6, 3, seed=9)
    mean, std = B.channel_moments(images)
    return images, labels, mean, std, _pipeline(images, NU, mean, std, 0.5)


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
def test_against_the_colour_pipeline_applied_to_the_whole_data_set(dtype):
    """Bit for bit: the table is built by the pipeline's own ops, so no tolerance is needed."""
    images, labels, mean, std, full = _expanded()
    on_device = B.channel_moments(images.to(DEV))
    assert torch.allclose(on_device[0].cpu(), mean, rtol=1e-12, atol=0) and torch.allclose(on_device[1].cpu(), std, rtol=1e-12, atol=0)
    src = B.DeviceBatches.from_colour(images, labels, G, dtype=dtype, seed=SEED, nu=NU, mean=mean, std=std,
                                      constant_channel=0.5)
    want = full.to(dtype)
    for k in range(5):   # crosses the epoch boundary
        x, y, ind = src.draw()
        idx = src.expected_indices(k)
        assert ind.tolist() == idx and y.tolist() == labels[idx].tolist()
        assert x.shape == (1, G, 6, 6, 4) and torch.equal(_bits(x.cpu()), _bits(want[:, idx]))
    # the sequential form: every sample once, the last batch short, through the gather
    seq = B.DeviceBatches.from_colour(images, labels, G, dtype=dtype, seed=SEED, nu=NU, mean=mean, std=std,
                                      constant_channel=0.5, shuffle=False, drop_last=False)
    batches = list(seq)
    assert [len(b[1]) for b in batches] == [8, 8, 8, 8, 5] and dctn_amd.last_kernel() == f"colour_gather_{NAME[dtype]}"
    assert torch.equal(_bits(torch.cat([b[0] for b in batches], dim=1).cpu()), _bits(want))
    assert torch.cat([b[2] for b in batches]).tolist() == list(range(N))


# ------------------------------------------------------------------ 4. graphs and resume
def test_a_captured_draw_follows_the_counter_on_its_replays():
    images, labels = _data(N, 8, 8, 3)
    kw = dict(dtype=torch.bfloat16, seed=SEED, nu=NU, constant_channel=1.0)
    src, eager = B.DeviceBatches.from_colour(images, labels, G, **kw), B.DeviceBatches.from_colour(images, labels, G, **kw)
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


def test_a_loaded_state_repeats_the_next_batches():
    images, labels = _data(N, 5, 5, 3)
    kw = dict(dtype=torch.float32, nu=NU)
    src = B.DeviceBatches.from_colour(images, labels, G, seed=SEED, **kw)
    for _ in range(3):
        src.draw()
    saved = src.state_dict()
    assert saved == {"seed": SEED, "batches_done": 3}
    nxt = [src.draw() for _ in range(3)]
    fresh = B.DeviceBatches.from_colour(images, labels, G, seed=99, **kw)
    fresh.load_state_dict(saved)
    assert fresh.state_dict() == saved and fresh.expected_indices(3) == nxt[0][2].tolist()
    for x, y, ind in nxt:
        fx, fy, find = fresh.draw()
        assert torch.equal(fx, x) and torch.equal(fy, y) and torch.equal(find, ind)


# ------------------------------------------------------------------ 5. the training step and the evaluation pass
def _model(seed=3):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(((2, 3),), UnitTheoreticalOutputStd(), 1.0, DEV, torch.float32, image_size=6, Q_0=4)


def _flat_adam(model):
    from dctn_amd.training import FlatAdam

    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3, l2=1e-2)


def test_graphed_train_step_with_a_colour_source_equals_the_same_steps_fed_by_hand():
    """The by-hand side draws from a `from_features` source over the expanded tensor, which wants (channels = 1, n, H, W, 4):
    the very layout `_pipeline` gives."""
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    images, labels, mean, std, full = _expanded()
    assert full.shape == (1, N, 6, 6, 4)
    src = B.DeviceBatches.from_colour(images, labels, G, dtype=torch.float32, seed=SEED, nu=NU, mean=mean, std=std,
                                      constant_channel=0.5)
    hand_src = B.DeviceBatches.from_features(full.clone(), labels, G, seed=SEED)
    m = _model()
    opt = _flat_adam(m)
    step = GraphedTrainStep(m, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src)
    assert src.state_dict()["batches_done"] == 1          # the warm-up trained on draw 0
    seen = []
    for _ in range(3):
        out = step()
        seen.append(out["indices"].tolist())
    assert seen == [src.expected_indices(k) for k in (1, 2, 3)]
    assert src.state_dict() == {"seed": SEED, "batches_done": 4}
    assert step.x.shape == (1, G, 6, 6, 4)

    def by_hand(k):
        return hand_src.gather(torch.tensor(hand_src.expected_indices(k), device=DEV))[:2]

    h = _model()
    hopt = _flat_adam(h)
    hstep = GraphedTrainStep(h, *by_hand(0), fused_cross_entropy, hopt, warmup=1)
    for k in (1, 2, 3):
        hout = hstep(*by_hand(k))
    torch.cuda.synchronize()
    assert hopt.t == opt.t == 4
    assert torch.equal(hopt.flat, opt.flat) and torch.equal(hopt.m, opt.m) and torch.equal(hopt.v, opt.v)
    assert torch.equal(hout["loss"], out["loss"]) and bool(torch.isfinite(out["loss"]))


def test_graphed_score_over_a_colour_source_meets_fused_scoring_of_the_short_batches():
    """n = 37, G = 8: the graphed pass makes 5 padded draws (the last with 3 padding rows), the eager drop_last=False
    iteration 4 batches of 8 and one of 5, both summed in float64 by the same score kernel.  The correct count is equal.
    The mean cross-entropy gets the bound tests/test_gpu_eval_pass.py uses where two fused passes cut the same rows into
    different batches (its two-rank test): n * 2^-52 * sum |ce|, the re-association of n float64 terms."""
    import torch.nn.functional as F

    from dctn_amd.evaluation import GraphedScore, score_fused

    images, labels, mean, std, full = _expanded()
    kw = dict(dtype=torch.float32, seed=SEED, nu=NU, mean=mean, std=std, constant_channel=0.5, shuffle=False)
    model = _model()
    scorer = GraphedScore(model, B.DeviceBatches.from_colour(images, labels, G, **kw))
    assert scorer.src.padded_steps == 5 and scorer.src.state_dict()["batches_done"] == 0
    loss, acc = scorer()
    assert scorer.rows == N and scorer.src.state_dict()["batches_done"] == 5
    eager = B.DeviceBatches.from_colour(images, labels, G, drop_last=False, **kw)
    assert len(eager) == 5
    want_loss, want_acc = score_fused(model.eval(), eager, DEV)
    with torch.no_grad():
        ce = F.cross_entropy(model(full.to(DEV)).cpu().double(), labels, reduction="none")
    bound = N * 2.0 ** -52 * float(ce.abs().sum())
    print(f"\ngraphed {loss!r} {acc}; fused over the short batches {want_loss!r} {want_acc}; |difference| "
          f"{abs(loss - want_loss):.3e}, bound {bound:.3e}")
    assert scorer.correct == round(want_acc * N) and acc == want_acc
    assert abs(loss - want_loss) <= bound
