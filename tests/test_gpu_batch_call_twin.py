"""dctn_batch_draw_call / dctn_batch_gather_call against the six older entry points on the GPU (`-m gpu`): the same launch
described both ways, from equal state blocks into equal-sized buffers, gives the same bits of x, the same y and indices,
the same 16-byte block afterwards and the same kernel name - for every kind, operation, width, dtype and flag, on the
vector paths (4 x 6 images) and the element paths (5 x 5).  Then `DeviceBatches`, which builds its descriptor once: three
consecutive draws, a gather, a loaded state and the replays of a captured draw against the Python restatement."""
import ctypes
import functools
import zlib

import pytest
import torch

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd import batches as B
from tests.test_gpu_augment import _bits, _lookup
from tests.test_host_batch_call_errors import ENTRY

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234567890ABCDEF
DTYPES = [torch.float32, torch.bfloat16, torch.float64]
IDS = ["f32", "bf16", "f64"]
U8, ROWS, COLOUR = L.BATCH_SRC_U8_TABLE, L.BATCH_SRC_ROWS, L.BATCH_SRC_COLOUR
N, G = 37, 8                      # S = 4 batches per epoch: counter 5 is in the second
SHARD = dict(count=4, rank_offset=4)
IMAGES = [(4, 6), (5, 5)]         # P = 24: four pixels per step; P = 25: pixel by pixel
GATHERED = [36, 0, 7, 7]


@functools.lru_cache(maxsize=None)
def _device(kind, shape, dtype):
    """Random device data of a shape, made once and never written: bytes, a table or rows, and the labels."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, shape, dtype)).encode()))
    if dtype == torch.uint8:
        t = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    elif dtype == torch.int64:
        t = torch.randint(0, 10, shape, generator=g)
    else:
        t = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
    return t.to(DEV)


def _fields(kind, dtype, row_len, width, channels=0, **more):
    """The source's part of a descriptor: the kind's data set, table and shapes."""
    if kind == ROWS:
        src, table = _device("rows", (width, N, row_len), dtype), None
    elif kind == COLOUR:
        src, table = _device("bytes", (N, row_len, channels), torch.uint8), _device("table", (width, 256), dtype)
    else:
        src, table = _device("bytes", (N, row_len), torch.uint8), _device("table", (256, width), dtype)
    f = dict(src=src.data_ptr(), table=None if table is None else table.data_ptr(),
             labels=_device("labels", (N,), torch.int64).data_ptr(), n=N, global_batch=G, row_len=row_len, src_kind=kind,
             src_channels=channels, width=width, dtype=L.dtype_code(torch.empty(0, dtype=dtype)), flags=0, **SHARD)
    f.update(more)
    return f, dtype


def _launch(fields, dtype, draw, counter, older):
    """One launch into fresh buffers (0xFF bytes) from a fresh block; (x bits, y, indices, block, kernel name)."""
    f = dict(fields)
    nbytes = f["count"] * f["row_len"] * f["width"] * torch.empty(0, dtype=dtype).element_size()
    x = torch.full((nbytes,), -1, dtype=torch.int8, device=DEV)
    y, ind = (torch.full((f["count"],), -1, dtype=torch.int64, device=DEV) for _ in range(2))
    state, picked = B._new_state(SEED, DEV, counter), torch.tensor(GATHERED, device=DEV)
    f.update(x=x.data_ptr(), y=y.data_ptr(), indices=ind.data_ptr(), stream=L.stream_ptr(DEV))
    if draw:
        f["state"] = state.data_ptr()
    else:
        f["sample_idx"] = picked.data_ptr()
    cols = "_cols" if f["src_kind"] == COLOUR else ""
    name = f"dctn_batch_draw{cols}_aug" if f.get("augment") else f"dctn_batch_{'draw' if draw else 'gather'}{cols}"
    if older:
        rc = getattr(L.lib(), name)(*[f[a] for a in ENTRY[name]])
    else:
        call = L.BatchCall(**{k: f.get(k, 0) for k, _ in L.BatchCall._fields_})
        rc = (L.lib().dctn_batch_draw_call if draw else L.lib().dctn_batch_gather_call)(ctypes.byref(call), f["stream"])
        ctypes.memset(ctypes.addressof(call), 0xEE, ctypes.sizeof(call))   # read during the call only
    assert rc == 0, (name, older, rc)
    kernel = dctn_amd.last_kernel()
    torch.cuda.synchronize()
    return x.cpu(), y.cpu(), ind.cpu(), state.cpu(), kernel


def _twin(fields_dtype, draw=True, counter=0, kernel=None):
    fields, dtype = fields_dtype
    old, new = (_launch(fields, dtype, draw, counter, older) for older in (True, False))
    for a, b, what in zip(old, new, ("x", "y", "indices", "state block", "kernel name")):
        assert (a == b if isinstance(a, str) else torch.equal(a, b)), (what, fields, draw, counter)
    x, y, ind, state, name = new
    assert name == kernel, name
    assert not bool((x == -1).all()) and state.tolist()[2:] == [counter + 1 if draw else counter, 0]
    return y.tolist(), ind.tolist()


def _drawn(counter, shuffle=True):
    return B.expected_indices(SEED, counter, N, G, rank=1, world=2, shuffle=shuffle)


def _labels(idx):
    labels = _device("labels", (N,), torch.int64).cpu()
    return [int(labels[i]) if i >= 0 else -100 for i in idx]


# ------------------------------------------------------------------ 1. both descriptions of every launch
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grey_table(dtype):
    dt = IDS[DTYPES.index(dtype)]
    for H, Wd in IMAGES:
        for Q in (1, 2, 3, 4):
            f = _fields(U8, dtype, H * Wd, Q)
            for counter in (0, 5):
                y, ind = _twin(f, counter=counter, kernel=f"batch_draw_u8_{dt}")
                assert ind == _drawn(counter) and y == _labels(ind)
            identity = _fields(U8, dtype, H * Wd, Q, flags=L.BATCH_IDENTITY_ORDER)
            assert _twin(identity, counter=5, kernel=f"batch_draw_u8_{dt}")[1] == [12, 13, 14, 15]
            y, ind = _twin(f, draw=False, kernel=f"batch_gather_u8_{dt}")
            assert ind == GATHERED and y == _labels(GATHERED)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows(dtype):
    dt = IDS[DTYPES.index(dtype)]
    for C in (1, 4):
        for R in (24, 5):
            f = _fields(ROWS, dtype, R, C)
            assert _twin(f, counter=5, kernel=f"batch_draw_rows_{dt}")[1] == _drawn(5)
            assert _twin(f, draw=False, kernel=f"batch_gather_rows_{dt}")[1] == GATHERED


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_colour(dtype):
    dt = IDS[DTYPES.index(dtype)]
    for H, Wd in IMAGES:
        for C, W in ((1, 1), (1, 2), (3, 3), (3, 4), (4, 4)):
            f = _fields(COLOUR, dtype, H * Wd, W, C)
            for counter in (0, 5):
                assert _twin(f, counter=counter, kernel=f"colour_draw_{dt}")[1] == _drawn(counter)
            assert _twin(f, draw=False, kernel=f"colour_gather_{dt}")[1] == GATHERED


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padded_tail(dtype):
    """Counter 4 of S = ceil(37 / 8) = 5: samples 32 .. 36 and three padding slots."""
    dt = IDS[DTYPES.index(dtype)]
    whole = dict(count=8, rank_offset=0, flags=L.BATCH_IDENTITY_ORDER | L.BATCH_PAD_TAIL)
    for H, Wd in IMAGES:
        for f, kernel in ((_fields(U8, dtype, H * Wd, 2, **whole), f"batch_draw_u8_{dt}"),
                          (_fields(COLOUR, dtype, H * Wd, 4, 3, **whole), f"colour_draw_{dt}")):
            y, ind = _twin(f, counter=4, kernel=kernel)
            assert ind == [32, 33, 34, 35, 36, -1, -1, -1] == B.expected_padded_indices(4, N, G) and y == _labels(ind)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_augmented(dtype):
    dt = IDS[DTYPES.index(dtype)]
    for H, Wd in IMAGES:
        for m in (0, 2):
            for aug_flags in (0, L.AUG_HFLIP):
                aug = dict(augment=1, height=H, width_px=Wd, max_shift=m, aug_flags=aug_flags)
                for f, kernel in ((_fields(U8, dtype, H * Wd, 2, fill=1, **aug), f"aug_draw_u8_{dt}"),
                                  (_fields(COLOUR, dtype, H * Wd, 4, 3, fill=0x030201, **aug), f"aug_draw_cols_{dt}")):
                    for counter in (0, 5):
                        assert _twin(f, counter=counter, kernel=kernel)[1] == _drawn(counter)


# ------------------------------------------------------------------ 2. the descriptor a source builds once
NU = (1.46, 0.83, 1.21)


def _sources():
    g = torch.Generator().manual_seed(5)
    grey = torch.randint(0, 256, (N, 5, 5), dtype=torch.uint8, generator=g)
    colour = torch.randint(0, 256, (N, 4, 6, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (N,), generator=g)
    phi = B.φ_cos_sin_squared_1
    kw = dict(dtype=torch.float32, seed=SEED, rank=1, world=2)
    return {
        "grey": (B.DeviceBatches(grey, labels, G, scale=1.5, **kw), grey, B.feature_table(phi, 1.5, torch.float32)),
        "colour": (B.DeviceBatches.from_colour(colour, labels, G, nu=NU, constant_channel=0.5, **kw), colour,
                   B.colour_table(3, nu=NU, constant_channel=0.5, dtype=torch.float32)),
        "augmented": (B.DeviceBatches.from_colour(colour, labels, G, nu=NU, constant_channel=0.5,
                                                  augment=B.Augment(2, True, (1, 2, 3)), **kw), colour,
                      B.colour_table(3, nu=NU, constant_channel=0.5, dtype=torch.float32)),
    }, labels


def _check_draw(src, images, table, labels, k, out):
    x, y, ind = out
    idx = src.expected_indices(k)
    fill = src.augment.fill if src.augment is not None else 0
    want = _lookup(table, B.augment_bytes(images[idx], src.expected_augment(k), fill))
    assert ind.tolist() == idx and y.tolist() == labels[idx].tolist(), k
    assert torch.equal(_bits(x.cpu()), _bits(want)), k


@pytest.mark.parametrize("which", ["grey", "colour", "augmented"])
def test_a_source_draws_and_gathers_from_its_one_descriptor(which):
    sources, labels = _sources()
    src, images, table = sources[which]
    assert (src.channels, src.height * src.width_px, src._call.count) == (images[0, 0, 0].numel(), src.row_len, 4)
    for k in range(3):
        _check_draw(src, images, table, labels, k, src.draw())
    picked = torch.tensor(GATHERED, device=DEV)
    for _ in range(2):   # a gather writes its own count into the descriptor; it is never augmented
        x, y, ind = src.gather(picked)
        assert ind.tolist() == GATHERED and y.tolist() == labels[GATHERED].tolist()
        assert torch.equal(_bits(x.cpu()), _bits(_lookup(table, images[GATHERED])))
        assert dctn_amd.last_kernel() == ("batch_gather_u8_f32" if which == "grey" else "colour_gather_f32")
    _check_draw(src, images, table, labels, 3, src.draw())          # and the draw after it is a draw of 4 again
    state = src._call.state
    src.load_state_dict({"seed": SEED + 1, "batches_done": 6})      # in place: the descriptor's pointer still holds
    assert src._call.state == state == src._state.data_ptr() and src.seed == SEED + 1
    for k in (6, 7, 8):                                             # epoch 1 into epoch 2
        _check_draw(src, images, table, labels, k, src.draw())
    assert src.state_dict() == {"seed": SEED + 1, "batches_done": 9}


def test_a_captured_draw_does_not_need_the_descriptor_again():
    sources, labels = _sources()
    src, images, table = sources["augmented"]
    x, y, ind = src.empty_batch()
    src.draw_into(x, y, ind)              # draw 0, eagerly: the kernel is loaded
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        src.draw_into(x, y, ind)
    torch.cuda.synchronize()
    assert src.state_dict()["batches_done"] == 1
    src.gather(torch.tensor(GATHERED, device=DEV))   # other outputs, another count and operation in the descriptor
    for k in (1, 2):
        graph.replay()
        _check_draw(src, images, table, labels, k, (x, y, ind))
    ctypes.memset(ctypes.addressof(src._call), 0, ctypes.sizeof(src._call))   # the launch kept its arguments by value
    graph.replay()
    _check_draw(src, images, table, labels, 3, (x, y, ind))
    assert src.state_dict()["batches_done"] == 4
