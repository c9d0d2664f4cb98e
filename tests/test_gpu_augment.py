"""The augmented draws on the GPU (`-m gpu`): the raw C-ABI of dctn_batch_draw_aug / dctn_batch_draw_cols_aug against the
Python restatement of the order and of the augmentation (`expected_indices`, `augment_params`, `augment_bytes`) and torch's
own indexing on the CPU - bit for bit, inside guarded buffers, on every path of the kernels - the identity with the
unaugmented draws at max_shift = 0, the alignment fallbacks, shards, more samples than waves, graph replays across epoch
boundaries, resume, the classes, and an augmented source as the first node of a GraphedTrainStep."""
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
FILLS = (11, 140, 255, 64)                        # a non-zero fill byte per source channel


class Framed:
    """A tensor inside a guarded byte allocation (the pattern of tests/test_gpu_colour_source.py).  An output (``values``
    None) starts as 0xFF bytes (NaN in every float dtype, -1 in int64); ``shift`` moves the base off its 256-byte
    alignment by that many bytes."""

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


@functools.lru_cache(maxsize=None)
def _data(n, H, Wd, C, seed=0):
    """(n, H, Wd) bytes for C = 0 (grey), (n, H, Wd, C) otherwise, and labels; shared, nobody writes into it."""
    g = torch.Generator().manual_seed(seed + 17 * C + 1000 * H + Wd)
    images = torch.randint(0, 256, (n, H, Wd) + ((C,) if C else ()), dtype=torch.uint8, generator=g)
    images[0, 0, 0] = 0
    images[0, 0, 1] = 255
    return images, torch.randint(0, 10, (n,), generator=g)


@functools.lru_cache(maxsize=None)
def _table(grey, W, dtype, seed=1):
    """Unrelated values: (256, Q) for the grey form, (W, 256) for the colour one - a mixed-up byte or channel shows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((256, W) if grey else (W, 256), generator=g, dtype=torch.float64).to(dtype)


def _lookup(table, images):
    """CPU indexing.  Grey (count, H, Wd) through (256, Q) -> (1, count, H, Wd, Q); colour (count, H, Wd, C) through
    (W, 256) -> (1, count, H, Wd, W): table[c][byte] for c < C, table[c][0] for the constant column."""
    if images.ndim == 3:
        return table[images.long()].unsqueeze(0)
    C = images.shape[-1]
    cols = [table[c][images[..., c].long()] for c in range(C)]
    cols += [table[c][torch.zeros_like(images[..., 0]).long()] for c in range(C, table.shape[0])]
    return torch.stack(cols, dim=-1).unsqueeze(0)


def _fill(C):
    fills = FILLS[: max(C, 1)]
    return fills, sum(v << (8 * c) for c, v in enumerate(fills))


N, G, K0 = 37, 8, 6   # draw 6 of S = 4: epoch 1, positions 16 .. 23


def _params(m, hflip, first=16, count=G, epoch=1):
    return [B.augment_params(SEED, epoch, first + j, m, hflip) for j in range(count)]


class Case:
    """Framed inputs of one shape, reused over the launches of a test; `draw` makes one launch into fresh framed
    outputs from a fresh state block at K0 and returns them."""

    def __init__(self, H, Wd, C, W, dtype, src_shift=0, x_shift=0):
        self.H, self.Wd, self.C, self.W, self.dtype, self.x_shift = H, Wd, C, W, dtype, x_shift
        self.images, self.labels = _data(N, H, Wd, C)
        self.table = _table(C == 0, W, dtype)
        self.src = Framed(tuple(self.images.shape), torch.uint8, self.images, shift=src_shift)
        self.tab = Framed(tuple(self.table.shape), dtype, self.table)
        self.lab = Framed((N,), torch.int64, self.labels)

    def draw(self, m, aug_flags, fill, flags=0, count=G, offset=0, unaugmented=False):
        H, Wd, C, W = self.H, self.Wd, self.C, self.W
        x = Framed((1, count, H, Wd, W), self.dtype, shift=self.x_shift)
        y, ind = Framed((count,), torch.int64), Framed((count,), torch.int64)
        state = B._new_state(SEED, DEV, K0)
        head = (self.src.view.data_ptr(), self.tab.view.data_ptr(), self.lab.view.data_ptr(), x.view.data_ptr(),
                y.view.data_ptr(), ind.view.data_ptr(), state.data_ptr(), N, G, count, offset)
        code, st = L.dtype_code(self.table), L.stream_ptr(DEV)
        if unaugmented and C:
            rc = L.lib().dctn_batch_draw_cols(*head, H * Wd, C, W, flags, code, st)
        elif unaugmented:
            rc = L.lib().dctn_batch_draw(*head, H * Wd, W, L.BATCH_SRC_U8_TABLE, flags, code, st)
        elif C:
            rc = L.lib().dctn_batch_draw_cols_aug(*head, H, Wd, C, W, flags, code, m, aug_flags, fill, st)
        else:
            rc = L.lib().dctn_batch_draw_aug(*head, H, Wd, W, flags, code, m, aug_flags, fill, st)
        assert rc == 0
        torch.cuda.synchronize()
        assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, K0 + 1, 0]
        assert x.guards_intact() and y.guards_intact() and ind.guards_intact()
        assert self.src.untouched() and self.tab.untouched() and self.lab.untouched()
        return x, y, ind

    def check(self, m, hflip, fills, packed, idx=None, first=16, count=G, flags=0, offset=0):
        idx = B.expected_indices(SEED, K0, N, G)[offset : offset + count] if idx is None else idx
        x, y, ind = self.draw(m, L.AUG_HFLIP if hflip else 0, packed, flags=flags, count=count, offset=offset)
        kind = "cols" if self.C else "u8"
        assert dctn_amd.last_kernel() == f"aug_draw_{kind}_{NAME[self.dtype]}"
        params = _params(m, hflip, first=first, count=count)
        want = _lookup(self.table, B.augment_bytes(self.images[idx], params, fills if self.C else fills[0]))
        assert want.shape == x.view.shape
        assert torch.equal(_bits(x.view.cpu()), _bits(want)), f"m={m} hflip={hflip} params={params}"
        assert y.view.cpu().tolist() == self.labels[idx].tolist() and ind.view.cpu().tolist() == idx
        return params


# ------------------------------------------------------------------ 1. the raw ABI
# (H, Wd, C, W); C = 0 is the grey form with W = Q table columns.  5x7: an odd pixel count (the pixel path), not square
# (H / Wd swaps show); 6x6: groups of four pixels that run over a row's end; 28x28: more than one step of a wave;
# 36x36x3: 324 groups, more than one unrolled pass of a wave (256), and 3888 bytes staged in several steps
SHAPES = [(5, 7, 0, 2), (8, 12, 0, 2), (28, 28, 0, 2), (8, 12, 0, 3), (6, 6, 0, 2), (5, 7, 3, 3), (6, 6, 3, 4), (4, 8, 1, 2),
          (8, 8, 4, 4), (36, 36, 3, 4)]


def _shape_id(s):
    H, Wd, C, W = s
    return f"grey_{H}x{Wd}_Q{W}" if C == 0 else f"colour_{H}x{Wd}x{C}_W{W}"


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("shape", SHAPES, ids=[_shape_id(s) for s in SHAPES])
def test_raw_abi(shape, dtype):
    H, Wd, C, W = shape
    case = Case(H, Wd, C, W, dtype)
    fills, packed = _fill(C)
    for m in (0, 1, 3):
        for hflip in (False, True):
            case.check(m, hflip, fills, packed)
    case.check(3, True, (0,) * max(C, 1), 0)   # the zero fill


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("C,W", [(0, 2), (3, 4)], ids=["grey", "colour"])
def test_samples_shifted_out_entirely_are_the_fill_entry(C, W, dtype):
    """4 x 8 images with max_shift = 4: slots 3 and 7 of draw 6 have dy = -4, so none of their rows is inside the image."""
    params = _params(4, True)
    out = [j for j, (dy, dx, _) in enumerate(params) if abs(dy) >= 4 or abs(dx) >= 8]
    assert out == [3, 7] and params[3][0] == params[7][0] == -4
    case = Case(4, 8, C, W, dtype)
    fills, packed = _fill(C)
    assert case.check(4, True, fills, packed) == params
    x, _, _ = case.draw(4, L.AUG_HFLIP, packed)
    if C:   # one value per column: the fill byte's entry of every source channel, then the constant column
        entry = torch.stack([case.table[c][fills[c] if c < C else 0] for c in range(W)])
    else:
        entry = case.table[fills[0]]
    for j in out:
        assert torch.equal(_bits(x.view[0, j].cpu()), _bits(entry.expand(4, 8, W)))


# ------------------------------------------------------------------ 2. identity against the unaugmented draws
@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("shape", [(8, 12, 0, 2), (5, 7, 0, 3), (6, 6, 3, 4), (5, 7, 3, 3)], ids=_shape_id)
def test_no_shift_and_no_flip_is_the_unaugmented_draw(shape, dtype):
    case = Case(*shape, dtype)
    for flags in (0, L.BATCH_IDENTITY_ORDER):
        x, y, ind = case.draw(0, 0, _fill(shape[2])[1], flags=flags)
        ux, uy, uind = case.draw(0, 0, 0, flags=flags, unaugmented=True)
        assert torch.equal(_bits(x.view), _bits(ux.view)) and torch.equal(y.view, uy.view) and torch.equal(ind.view, uind.view)


# ------------------------------------------------------------------ 3. the alignment fallbacks
@pytest.mark.parametrize("shape", [(8, 12, 0, 2), (6, 6, 3, 4)], ids=_shape_id)
def test_a_source_one_byte_off_its_alignment(shape):
    case = Case(*shape, torch.float32, src_shift=1)
    fills, packed = _fill(shape[2])
    case.check(3, True, fills, packed)


@pytest.mark.parametrize("shape", [(8, 8, 3, 3), (8, 12, 0, 3)], ids=_shape_id)
def test_x_off_its_store_alignment_takes_the_pixel_path(shape):
    """bf16 with three columns stores 8 bytes at a time: an x base 2 bytes off (its element size) must still come out
    right."""
    case = Case(*shape, torch.bfloat16, x_shift=2)
    fills, packed = _fill(shape[2])
    case.check(3, True, fills, packed)
    case.check(1, False, fills, packed)


# ------------------------------------------------------------------ 4. shards and the identity order
@pytest.mark.parametrize("shape", [(8, 12, 0, 2), (6, 6, 3, 4)], ids=_shape_id)
def test_two_shards_make_the_global_batch(shape):
    """The parameters come from the GLOBAL position: the second shard's slot 0 is position 20, not 16."""
    case = Case(*shape, torch.float32)
    fills, packed = _fill(shape[2])
    whole = case.check(2, True, fills, packed)
    lo = case.check(2, True, fills, packed, count=4, offset=0, first=16)
    hi = case.check(2, True, fills, packed, count=4, offset=4, first=20)
    assert lo + hi == whole and lo != hi


@pytest.mark.parametrize("shape", [(5, 7, 0, 2), (6, 6, 3, 4)], ids=_shape_id)
def test_identity_order_with_a_shard_offset(shape):
    case = Case(*shape, torch.float32)
    fills, packed = _fill(shape[2])
    case.check(2, True, fills, packed, idx=[20, 21, 22, 23], first=20, count=4, offset=4, flags=L.BATCH_IDENTITY_ORDER)


# ------------------------------------------------------------------ 5. more samples than waves
def test_more_samples_than_the_launch_has_waves():
    """A local batch of 1030 in one launch: the grid is capped at the number of CUs, so waves take several samples and reuse
    their LDS region."""
    n, Gb = 1300, 1030
    images, labels = _data(n, 4, 4, 0, seed=3)
    aug = B.Augment(2, True, 9)
    src = B.DeviceBatches(images, labels, Gb, dtype=torch.bfloat16, seed=5, augment=aug)
    x, y, ind = src.draw()
    idx = B.expected_indices(5, 0, n, Gb)
    assert ind.tolist() == idx and y.tolist() == labels[idx].tolist()
    params = src.expected_augment(0)
    assert len(params) == Gb and len(set(params)) == 50
    want = _lookup(B.feature_table(src_phi(), 1.0, torch.bfloat16), B.augment_bytes(images[idx], params, 9))
    assert x.shape == (1, Gb, 4, 4, 2) and torch.equal(_bits(x.cpu()), _bits(want))
    assert _words(src._state)[2:] == [1, 0] and dctn_amd.last_kernel() == "aug_draw_u8_bf16"


def src_phi():
    from dctn_amd.window_stats import φ_cos_sin_squared_1

    return φ_cos_sin_squared_1


# ------------------------------------------------------------------ 6. replays, 7. resume, 8. the classes
NU = (1.46, 0.83, 1.21)


def _colour_source(aug, dtype=torch.float32, seed=SEED, **kw):
    images, labels = _data(N, 6, 6, 3)
    return B.DeviceBatches.from_colour(images, labels, G, dtype=dtype, seed=seed, nu=NU, constant_channel=0.5, augment=aug,
                                       **kw)


def _colour_want(src, k, dtype=torch.float32):
    images, _ = _data(N, 6, 6, 3)
    table = B.colour_table(3, nu=NU, constant_channel=0.5, dtype=dtype)
    return _lookup(table, B.augment_bytes(images[src.expected_indices(k)], src.expected_augment(k), src.augment.fill))


def test_a_captured_draw_is_augmented_anew_on_every_replay():
    """S = 4: nine replays after the eager draw 0 cross two epoch boundaries."""
    src = _colour_source(B.Augment(2, True, (125, 123, 114)), dtype=torch.bfloat16)
    assert src.steps == 4
    x, y, ind = src.empty_batch()
    src.draw_into(x, y, ind)                  # draw 0, eagerly
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.cpu()), _bits(_colour_want(src, 0, torch.bfloat16)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        src.draw_into(x, y, ind)
    assert src.state_dict()["batches_done"] == 1          # the capture itself launches nothing
    for k in range(1, 10):
        graph.replay()
        assert ind.tolist() == src.expected_indices(k)
        assert torch.equal(_bits(x.cpu()), _bits(_colour_want(src, k, torch.bfloat16))), f"replay {k}"
    assert src.state_dict() == {"seed": SEED, "batches_done": 10}
    # the same positions, other parameters: epoch 0, 1 and 2
    assert src.expected_augment(1) != src.expected_augment(5) != src.expected_augment(9) != src.expected_augment(1)


def test_a_loaded_state_repeats_the_next_batches_with_their_augmentations():
    images, labels = _data(N, 8, 12, 0)
    aug = B.Augment(3, True, 40)
    src = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=SEED, augment=aug)
    for _ in range(3):
        src.draw()
    saved = src.state_dict()
    assert saved == {"seed": SEED, "batches_done": 3}
    nxt = [src.draw() for _ in range(3)]
    fresh = B.DeviceBatches(images, labels, G, dtype=torch.float32, seed=99, augment=aug)
    assert fresh.expected_augment(3) != src.expected_augment(3)
    fresh.load_state_dict(saved)
    assert fresh.state_dict() == saved and fresh.expected_augment(3) == src.expected_augment(3)
    for x, y, ind in nxt:
        fx, fy, find = fresh.draw()
        assert torch.equal(fx, x) and torch.equal(fy, y) and torch.equal(find, ind)


def test_through_the_classes():
    images, labels = _data(N, 5, 7, 0)
    aug = B.Augment(2, True, 200)
    grey = B.DeviceBatches(images, labels, G, dtype=torch.float64, seed=SEED, scale=1.5, augment=aug, rank=1, world=2)
    table = B.feature_table(src_phi(), 1.5, torch.float64)
    for k in range(6):   # crosses the epoch boundary
        x, y, ind = grey.draw()
        idx, params = grey.expected_indices(k), grey.expected_augment(k)
        first = (k % 4) * G + 4
        assert params == [B.augment_params(SEED, k // 4, first + j, 2, True) for j in range(4)]
        assert ind.tolist() == idx and y.tolist() == labels[idx].tolist()
        assert torch.equal(_bits(x.cpu()), _bits(_lookup(table, B.augment_bytes(images[idx], params, 200))))
    assert dctn_amd.last_kernel() == "aug_draw_u8_f64"
    # gather is never augmented
    gx, gy, gind = grey.gather(torch.tensor(idx, device=DEV))
    assert torch.equal(_bits(gx.cpu()), _bits(_lookup(table, images[idx]))) and gind.tolist() == idx
    assert dctn_amd.last_kernel() == "batch_gather_u8_f64"

    colour = _colour_source(B.Augment(1, False, (1, 2, 3)))
    for k in range(5):
        x, y, ind = colour.draw()
        assert ind.tolist() == colour.expected_indices(k) and torch.equal(_bits(x.cpu()), _bits(_colour_want(colour, k)))
        assert all(f == 0 for _, _, f in colour.expected_augment(k))
    assert dctn_amd.last_kernel() == "aug_draw_cols_f32"
    gx, _, _ = colour.gather(ind)
    cimages, _ = _data(N, 6, 6, 3)
    ctable = B.colour_table(3, nu=NU, constant_channel=0.5, dtype=torch.float32)
    assert torch.equal(_bits(gx.cpu()), _bits(_lookup(ctable, cimages[ind.cpu()])))

    # evaluation is not augmented: the padded pass raises, and a second source over the SAME device bytes serves it
    seq = _colour_source(B.Augment(1, True), shuffle=False)
    with pytest.raises(ValueError):
        seq.draw_padded_into(*seq.empty_batch())
    plain = B.DeviceBatches.from_colour(seq.src, seq.labels, G, dtype=torch.float32, seed=SEED, nu=NU, constant_channel=0.5,
                                        shuffle=False)
    assert plain.src.data_ptr() == seq.src.data_ptr() and plain.labels.data_ptr() == seq.labels.data_ptr()
    out = plain.empty_batch()
    plain.draw_padded_into(*out)
    assert out[2].tolist() == list(range(8)) and plain.expected_augment(0) == [(0, 0, 0)] * 8
    # the identity order is augmented too
    x, _, ind = seq.draw()
    assert ind.tolist() == list(range(8)) and torch.equal(_bits(x.cpu()), _bits(_colour_want(seq, 0)))


# ------------------------------------------------------------------ 9. training
def _model(seed=3):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(((2, 3),), UnitTheoreticalOutputStd(), 1.0, DEV, torch.float32, image_size=6, Q_0=4)


def _flat_adam(model):
    from dctn_amd.training import FlatAdam

    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3, l2=1e-2)


def test_graphed_train_step_with_an_augmented_source_equals_the_same_steps_fed_by_hand():
    """Bitwise, as tests/test_gpu_colour_source.py's: the by-hand side gets batches that are augmented and expanded on the
    CPU (`augment_bytes`, then the colour table indexed by the bytes)."""
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    images, labels = _data(N, 6, 6, 3)
    mean, std = B.channel_moments(images)
    fill = tuple(int(round(255 * float(v))) for v in mean)
    kw = dict(dtype=torch.float32, seed=SEED, nu=NU, mean=mean, std=std, constant_channel=0.5)
    src = B.DeviceBatches.from_colour(images, labels, G, augment=B.Augment(2, True, fill), **kw)
    table = B.colour_table(3, nu=NU, mean=mean, std=std, constant_channel=0.5, dtype=torch.float32)
    m = _model()
    opt = _flat_adam(m)
    step = GraphedTrainStep(m, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src)
    assert src.state_dict()["batches_done"] == 1          # the warm-up trained on draw 0
    seen = []
    for _ in range(4):   # draws 1 .. 4: into the second epoch
        out = step()
        seen.append(out["indices"].tolist())
    assert seen == [src.expected_indices(k) for k in (1, 2, 3, 4)]
    assert src.state_dict() == {"seed": SEED, "batches_done": 5}
    assert step.x.shape == (1, G, 6, 6, 4)
    assert any(p != (0, 0, 0) for p in src.expected_augment(4))

    def by_hand(k):
        idx = src.expected_indices(k)
        x = _lookup(table, B.augment_bytes(images[idx], src.expected_augment(k), fill))
        return x.to(DEV), labels[idx].to(DEV)

    assert torch.equal(_bits(step.x), _bits(by_hand(4)[0]))
    h = _model()
    hopt = _flat_adam(h)
    hstep = GraphedTrainStep(h, *by_hand(0), fused_cross_entropy, hopt, warmup=1)
    for k in (1, 2, 3, 4):
        hout = hstep(*by_hand(k))
    torch.cuda.synchronize()
    assert hopt.t == opt.t == 5
    assert torch.equal(hopt.flat, opt.flat) and torch.equal(hopt.m, opt.m) and torch.equal(hopt.v, opt.v)
    assert torch.equal(hout["loss"], out["loss"]) and bool(torch.isfinite(out["loss"]))
