"""Whole-run snapshots on the GPU (`-m gpu`): the contract of `dctn_state_gather` / `dctn_state_scatter` under the guarded,
poisoned arena of tests/guarded_buffers.py (the two launches report no kernel name, so this file holds their contract),
and runs resumed through `checkpoint.RunState`.  Every comparison is bit for bit: there is no tolerance anywhere.

Resume: run A is 8 replays of the whole graphed recipe (bf16, `DeviceBatches` with `Augment`, fused dropout,
`FlatAdam` on master weights behind a `GradGuard` that clips some of the steps) with a `snapshot()` after replay 4 and no
synchronisation before replay 5; run B builds everything afresh from other seeds, captures its own graph (three warm-up
iterations advance every counter), loads A's file in place and replays 4 times.  None of this exists on the parent commit."""
import atexit
import functools
import os
import shutil
import socket
import tempfile

import numpy as np
import pytest
import torch

from tests.guarded_buffers import guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
U8, F32, F64, I32 = torch.uint8, torch.float32, torch.float64, torch.int32


def _lib():
    from dctn_amd import _lib as L

    return L


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(U8)


def _digest(t):
    from dctn_amd import checkpoint as C

    return C.digest(_bytes(t).cpu().numpy())


# ------------------------------------------------------------------ 1. the kernel contract
# (bytes, dtype, elements skipped in front: the region then starts at a multiple of 4 that is no multiple of 16).
# 1 .. 4 and 15 .. 17: the tail forms and the edges of a 16-byte chunk; 4095 .. 4097: the edges of a workgroup's tile of
# 4096 bytes, 4097 crossing it by a single byte; 2^20 + 5: 257 tiles, many workgroups, a one-byte tail behind a dword.
REGIONS = [(1, U8, 0), (2, BF16, 0), (3, U8, 0), (4, I32, 0), (15, U8, 0), (16, F32, 0), (17, U8, 0), (4095, U8, 0),
           (4096, F64, 0), (4097, U8, 0), ((1 << 20) + 5, U8, 0),
           (3996, F32, 1),     # float32 t[1:]: aligned to 4 bytes, not to 16
           (4098, BF16, 0),    # a two-byte tail
           (4100, I32, 3),     # int32 t[3:], base + 12: dword accesses over a tile edge
           (800, F64, 1),      # float64 t[1:], base + 8
           (4099, U8, 4)]      # bytes at base + 4: the dword path with a three-byte tail
assert len(REGIONS) == 16


def _make_regions(seed=11):
    """The 16 sources on the device (views into torch allocations) and their bytes on the CPU."""
    g = torch.Generator().manual_seed(seed)
    tensors, raws = [], []
    for nbytes, dtype, skip in REGIONS:
        item = torch.empty((), dtype=dtype).element_size()
        host = torch.randint(0, 256, (nbytes + skip * item,), dtype=U8, generator=g)
        t = host.to(DEV).view(dtype)[skip:]
        assert t.numel() * item == nbytes and t.data_ptr() % 4 == 0 and (t.data_ptr() % 16 == 0) == (skip == 0)
        tensors.append(t)
        raws.append(host[skip * item:].numpy().copy())
    return tensors, raws


def _counts(tensors):
    return [t.numel() * t.element_size() for t in tensors]


def _expected_arena(raws, pad=0):
    from dctn_amd import checkpoint as C

    offsets, total = C.arena_layout([r.size for r in raws])
    arena = np.full(total, pad, dtype=np.uint8)
    for off, r in zip(offsets, raws):
        arena[off: off + r.size] = r
    return arena, offsets


def _gather(tensors, arena, digests, nbytes=None):
    L = _lib()
    return L.lib().dctn_state_gather(L.ptr_array(tensors), L.i64_array(_counts(tensors)), len(tensors), arena.data_ptr(),
                                     arena.numel() if nbytes is None else nbytes, digests.data_ptr(), L.stream_ptr(DEV))


def _scatter(arena, tensors, digests):
    L = _lib()
    return L.lib().dctn_state_scatter(arena.data_ptr(), L.ptr_array(tensors), L.i64_array(_counts(tensors)), len(tensors),
                                      digests.data_ptr(), L.stream_ptr(DEV))


def _pairs(digests):
    return [tuple(int(v) for v in row) for row in digests.cpu().numpy().view(np.uint64).reshape(-1, 2)]


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_gather_of_16_regions_under_the_guarded_arena(fill):
    """The arena is the regions and their ZERO padding whatever it held before (NaN fill, 0x7B fill), the digests are
    `checkpoint.digest` of the same bytes, and nothing outside the two buffers is written."""
    from dctn_amd import checkpoint as C

    tensors, raws = _make_regions()
    want, _ = _expected_arena(raws)
    with guarded(fill=fill) as arena:
        out = arena.empty((want.size,), U8, DEV)
        digests = arena.empty((2 * len(tensors),), torch.int64, DEV)
        assert _gather(tensors, out, digests) == 0
    arena.check()
    assert np.array_equal(out.cpu().numpy(), want)
    assert _pairs(digests) == [C.digest(r) for r in raws]
    for t, r in zip(tensors, raws):   # the sources are only read
        assert np.array_equal(t.view(U8).cpu().numpy(), r)


@pytest.mark.parametrize("fill", [0xFF, 0x7B])
def test_scatter_of_16_regions_never_writes_past_a_region(fill):
    """Every destination is its own guarded allocation that ENDS at the region's last byte (the guard starts at the
    next one); the unaligned ones start 4, 8 or 12 bytes into theirs.  The arena's padding holds garbage here: it is
    neither written out nor part of the digest."""
    from dctn_amd import checkpoint as C

    _, raws = _make_regions(seed=12)
    image, _ = _expected_arena(raws, pad=0xA5)
    with guarded(fill=fill) as arena:
        src = arena.place(torch.from_numpy(image).to(DEV))
        digests = arena.empty((2 * len(raws),), torch.int64, DEV)
        dsts, fronts = [], []
        for (nbytes, dtype, skip), r in zip(REGIONS, raws):
            item = torch.empty((), dtype=dtype).element_size()
            whole = arena.empty((nbytes + skip * item,), U8, DEV)
            fronts.append(whole[: skip * item])
            dsts.append(whole[skip * item:].view(dtype))
        assert _scatter(src, dsts, digests) == 0
    arena.check()
    for d, front, r in zip(dsts, fronts, raws):
        assert np.array_equal(d.view(U8).cpu().numpy(), r)
        assert bool((front == fill).all())   # the bytes in front of an unaligned region
    assert _pairs(digests) == [C.digest(r) for r in raws]
    assert np.array_equal(src.cpu().numpy(), image)   # the arena is only read


def test_a_bf16_view_at_an_odd_element_is_refused_and_nothing_is_written():
    L = _lib()
    tensors, raws = _make_regions()
    odd = torch.zeros(9, dtype=BF16, device=DEV)[1:]
    assert odd.data_ptr() % 4 == 2
    bad = tensors[:3] + [odd] + tensors[3:15]
    total = _expected_arena([np.zeros(n, np.uint8) for n in _counts(bad)])[0].size
    with guarded(fill=0x7B) as arena:
        out = arena.empty((total,), U8, DEV)
        digests = arena.empty((2 * len(bad),), torch.int64, DEV)
        assert _gather(bad, out, digests) == L.ERR_UNSUPPORTED
        assert _scatter(out, bad, digests) == L.ERR_UNSUPPORTED
    arena.check()
    assert bool((out == 0x7B).all()) and bool((digests.view(U8) == 0x7B).all())
    for t, r in zip(tensors, raws):
        assert np.array_equal(t.view(U8).cpu().numpy(), r)
    # and through RunState: a parameter that is such a view
    from dctn_amd import checkpoint as C

    model = torch.nn.Module()
    model.w = torch.nn.Parameter(torch.zeros(9, dtype=BF16, device=DEV)[1:].detach())
    with pytest.raises(NotImplementedError, match="model.w.*multiple of 4"):
        C.RunState(model).snapshot()


def test_both_launches_are_capturable_and_replay_the_same_bytes():
    from dctn_amd import checkpoint as C

    tensors, raws = _make_regions(seed=13)
    want, _ = _expected_arena(raws)
    out = torch.empty(want.size, dtype=U8, device=DEV)
    dsts = [torch.empty_like(t) for t in tensors]
    d_gather = torch.empty(2 * len(tensors), dtype=torch.int64, device=DEV)
    d_scatter = torch.empty_like(d_gather)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):   # once eagerly: the capture must not be the first launch of a kernel
        assert _gather(tensors, out, d_gather) == 0 and _scatter(out, dsts, d_scatter) == 0
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        assert _gather(tensors, out, d_gather) == 0
        assert _scatter(out, dsts, d_scatter) == 0
    for round_ in range(2):   # other source bytes before every replay: the graph reads the regions, not a copy
        g = torch.Generator().manual_seed(50 + round_)
        for i, t in enumerate(tensors):
            fresh = torch.randint(0, 256, (raws[i].size,), dtype=U8, generator=g)
            raws[i] = fresh.numpy().copy()
            t.view(U8).copy_(fresh)
        out.fill_(0xEE)
        graph.replay()
        torch.cuda.synchronize(DEV)
        assert np.array_equal(out.cpu().numpy(), _expected_arena(raws)[0])
        for d, r in zip(dsts, raws):
            assert np.array_equal(d.view(U8).cpu().numpy(), r)
        assert _pairs(d_gather) == _pairs(d_scatter) == [C.digest(r) for r in raws]


def test_17_regions_go_through_run_state_in_two_launches(tmp_path):
    """A model without an optimizer: every parameter is a region of its own."""
    from dctn_amd import checkpoint as C

    torch.manual_seed(3)
    model = torch.nn.Module()
    sizes = [1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 1025, 4097, 3]
    for i, n in enumerate(sizes):
        model.register_parameter(f"w{i:02}", torch.nn.Parameter(torch.randn(n, device=DEV).to(BF16 if i % 3 == 0 else F32)))
    run = C.RunState(model)
    assert len(run.tensors) == 17 > C.MAX_REGIONS
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    snap = run.snapshot({"note": "seventeen"})
    with torch.no_grad():
        for p in model.parameters():   # stream-ordered behind the gather: the snapshot holds the values from before
            p.zero_()
    path = snap.save(str(tmp_path / "17.dctn"))
    manifest, arena = C.read_file(path)
    assert [r["name"] for r in manifest["regions"]] == [f"model.w{i:02}" for i in range(17)]
    for r, (k, v) in zip(manifest["regions"], before.items()):
        assert (r["s1"], r["s2"]) == _digest(v) and r["dtype"] == str(v.dtype).replace("torch.", "")
    assert all(not bool(p.any()) for p in model.parameters())
    assert run.load(path) == {"note": "seventeen"}
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    state = C.read_model_state(path)
    assert list(state) == list(before) and all(torch.equal(state[k], before[k].cpu()) for k in before)


# ------------------------------------------------------------------ 2. resumed runs
N_SAMPLES, GLOBAL_BATCH, IMAGE = 64, 16, 28
# The gradient norms of run A's 11 steps without clipping, measured on an MI355X: 98.5, 102.1, 110.3, 111.1, 107.5, 115.9,
# 111.7, 104.2, 106.9, 98.1, 86.2.  A threshold between them: the first two steps pass unclipped, the third is clipped.
MAX_NORM = 105.0
SEEDS_A = dict(model=1, dropout=77, batch=5)
SEEDS_B = dict(model=2, dropout=1234567, batch=99)
_TMP = []


def _tmp_dir():
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="dctn_run_state_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    return _TMP[0]


def _data():
    g = torch.Generator().manual_seed(2026)
    return (torch.randint(0, 256, (N_SAMPLES, IMAGE, IMAGE), dtype=U8, generator=g),
            torch.randint(0, 10, (N_SAMPLES,), generator=g))


def _objects(seeds, kind="adam", max_norm=MAX_NORM, rank=None, world=None):
    """Model, optimizer, source, guard and their RunState: bf16 + FlatAdam on master weights, or float32 + FlatSGD."""
    from dctn_amd import checkpoint as C
    from dctn_amd.batches import Augment, DeviceBatches
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd
    from dctn_amd.training import FlatAdam, FlatSGD, GradGuard

    dtype = BF16 if kind == "adam" else F32
    torch.manual_seed(seeds["model"])
    model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 0.9, DEV, dtype, image_size=IMAGE)
    model.use_fused_dropout(seeds["dropout"])
    images, labels = _data()
    src = DeviceBatches(images, labels, GLOBAL_BATCH, dtype=dtype, seed=seeds["batch"], augment=Augment(max_shift=2),
                        rank=rank, world=world, device=DEV)
    guard = GradGuard(DEV, max_norm)
    reg, others = list(model.epses) + [model.linear.weight], [model.linear.bias]
    if kind == "adam":
        opt = FlatAdam(reg, others, lr=3e-3, l2=1e-4, master_weights=True, guard=guard)
    else:
        opt = FlatSGD(reg, others, lr=1e-3, momentum=0.9, l2=1e-4, guard=guard)
    run = C.RunState(model, opt, batch_source=src)
    return model, opt, src, guard, run


def _graph(model, opt, src):
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, batch_source=src)   # 3 warm-up iterations


def _final(model, opt, src, guard, out=None, kind="adam"):
    torch.cuda.synchronize(DEV)
    state = dict(flat=opt.flat.clone(), sq_sum=opt.sq_sum.clone(), p=model.p.clone(), guard=guard.read(),
                 dropout=model.dropout_state_dict(), source=src.state_dict(), host_seed=src.seed)
    if kind == "adam":
        state.update(master=opt.master.clone(), m=opt.m.clone(), v=opt.v.clone(), t=opt.t, lr=opt.lr)
    else:
        state.update(buf=opt.buf.clone(), steps=opt._steps)
    if out is not None:
        state.update(indices=out["indices"].clone(), loss=out["loss"].detach().clone())
    return state


def _assert_same_state(got, want, what):
    assert got.keys() == want.keys()
    for key, w in want.items():
        g = got[key]
        if isinstance(w, torch.Tensor):
            assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {key}"
            assert torch.equal(_bytes(g), _bytes(w)), f"{what}: {key} differs"
        elif isinstance(w, dict) and "last_norm" in w:   # NaN-safe: compare the floats by their bits
            assert {k: np.float32(v).tobytes() if isinstance(v, float) else v for k, v in g.items()} == \
                   {k: np.float32(v).tobytes() if isinstance(v, float) else v for k, v in w.items()}, f"{what}: {key}"
        else:
            assert g == w, f"{what}: {key}: {g} != {w}"


@functools.lru_cache(maxsize=None)
def _run_a():
    """Run A, computed once and shared: (path of the file, final state, guard block at the end)."""
    model, opt, src, guard, run = _objects(SEEDS_A)
    step = _graph(model, opt, src)
    for _ in range(4):
        step()
    snap = run.snapshot({"num_iters_done": 4, "best": 0.25})   # nothing synchronises between replay 4 and replay 5
    for _ in range(4):
        out = step()
    path = snap.save(os.path.join(_tmp_dir(), "run_a.dctn"))
    final = _final(model, opt, src, guard, out)
    print(f"run A: guard {final['guard']}, t = {final['t']}, source {final['source']}")
    return path, final


def test_run_a_clips_some_steps_and_not_others():
    _, final = _run_a()
    g = final["guard"]
    assert g["seen"] == 11 and g["halted"] == 0 and 0 < g["clipped"] < g["seen"], g
    assert final["t"] == 11 and final["source"]["batches_done"] == 11 and final["dropout"]["draws_done"] == 11


def test_a_graphed_run_resumes_bit_for_bit_under_its_new_graph():
    from dctn_amd import checkpoint as C

    path, want = _run_a()
    model, opt, src, guard, run = _objects(SEEDS_B, max_norm=None)
    step = _graph(model, opt, src)   # first: its warm-up trains and advances every counter of run B
    assert not torch.equal(opt.flat, want["flat"]) and src.state_dict()["seed"] == SEEDS_B["batch"]
    assert run.load(path) == {"num_iters_done": 4, "best": 0.25}
    assert (opt.t, model.dropout_state_dict()["draws_done"], src.state_dict()["batches_done"]) == (7, 7, 7)
    assert guard.max_norm == MAX_NORM and src.seed == SEEDS_A["batch"] and guard.read()["seen"] == 7
    # the file's model state is what now stands in the model
    state = C.read_model_state(path)
    live = model.state_dict()
    assert list(state) == list(live) and set(live) == {"epses.0", "linear.weight", "linear.bias", "p"}
    for k in live:
        assert state[k].dtype == live[k].dtype and torch.equal(state[k], live[k].cpu()), k
    for _ in range(4):
        out = step()
    _assert_same_state(_final(model, opt, src, guard, out), want, "resumed graphed run")


def test_read_model_state_feeds_load_state_dict():
    from dctn_amd import checkpoint as C
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    path, _ = _run_a()
    state = C.read_model_state(path)
    torch.manual_seed(9)
    model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, DEV, BF16, image_size=IMAGE)
    model.load_state_dict(state)
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), state[k]), k
    assert model._p_float == float(state["p"]) != 1.0


def test_one_flipped_arena_byte_raises_before_anything_is_written(tmp_path):
    from dctn_amd import checkpoint as C

    path, _ = _run_a()
    raw = bytearray(open(path, "rb").read())
    manifest, _ = C.read_file(path)
    region = next(r for r in manifest["regions"] if r["name"] == "optimizer.v")
    raw[len(raw) - manifest["arena_bytes"] + region["offset"] + region["bytes"] // 2] ^= 0x01
    bad = str(tmp_path / "flipped.dctn")
    open(bad, "wb").write(bytes(raw))
    model, opt, src, guard, run = _objects(SEEDS_B)
    before = [t.clone() for t in run.tensors]
    mirrors = (opt.lr, guard.max_norm, src.seed)
    with pytest.raises(ValueError, match="'optimizer.v' is damaged"):
        run.load(bad)
    torch.cuda.synchronize(DEV)
    for name, t, b in zip(run.names, run.tensors, before):
        assert torch.equal(_bytes(t), _bytes(b)), name
    assert (opt.lr, guard.max_norm, src.seed) == mirrors


def test_a_mismatched_run_is_refused_by_name():
    path, _ = _run_a()
    *_, run = _objects(SEEDS_B, kind="sgd")
    with pytest.raises(ValueError, match="optimizer"):
        run.load(path)


def test_a_halted_guard_stays_halted_after_a_load(tmp_path):
    from dctn_amd.training import fused_cross_entropy, train_step

    model, opt, src, guard, run = _objects(SEEDS_A)
    x, y, _ = src.draw()
    train_step(model, x, y, fused_cross_entropy, opt)
    x, y, _ = src.draw()
    x[0, 0, 0, 0, 0] = float("nan")
    train_step(model, x, y, fused_cross_entropy, opt)
    want = guard.read()
    assert want["halted"] == 1 and want["bad_step"] == 1
    path = run.snapshot().save(str(tmp_path / "halted.dctn"))
    model, opt, src, guard, run = _objects(SEEDS_B)
    assert guard.read()["halted"] == 0
    run.load(path)
    got = guard.read()
    assert got["halted"] == 1 and got["bad_step"] == 1 and got["seen"] == 2 and guard.halted
    flat, t = opt.flat.clone(), opt.t
    x, y, _ = src.draw()
    train_step(model, x, y, fused_cross_entropy, opt)   # a halted guard: the step is not applied
    assert torch.equal(opt.flat.view(torch.int16), flat.view(torch.int16)) and opt.t == t == 1


def _train_sgd(seeds, stop_after, first_iter=0, load=None, hook_dir=None):
    from dctn_amd import checkpoint as C
    from dctn_amd.training import fused_cross_entropy, make_stopper_after_n_iters, train

    model, opt, src, guard, run = _objects(seeds, kind="sgd")
    extras = run.load(load) if load is not None else None
    zero = torch.zeros((), device=DEV)
    hooks = [make_stopper_after_n_iters(stop_after)]
    saver = None
    if hook_dir is not None:
        saver = C.RunCheckpointer(hook_dir, run, 2, extras=lambda st_x, st_it: {"loss": float(st_it["loss"].detach())})
        hooks.insert(0, saver)
    _, st_it = train(src, model, opt, DEV, fused_cross_entropy, lambda st_x, st_it: zero, 0.0, [], [], hooks,
                     first_iter=first_iter)
    newest = saver.flush() if saver is not None else None
    out = dict(indices=st_it["indices"], loss=st_it["loss"])
    return _final(model, opt, src, guard, out, kind="sgd"), st_it["num_iters_done"], extras, newest


def test_flat_sgd_resumes_through_train_and_the_hook_keeps_two_files(tmp_path):
    """Float32, eager: 4 iterations with a `RunCheckpointer` hook, then fresh objects from other seeds load the newest
    file and `train(first_iter=4)` runs iterations 4 .. 7; an uninterrupted run of 8 is the reference."""
    want, last, _, _ = _train_sgd(SEEDS_A, stop_after=7)
    assert last == 7 and want["steps"] == 8
    hook_dir = str(tmp_path)
    _, last, _, newest = _train_sgd(SEEDS_A, stop_after=3, hook_dir=hook_dir)
    assert last == 3 and sorted(os.listdir(hook_dir)) == ["run_nitd=0000002.dctn", "run_nitd=0000003.dctn"]
    assert newest == os.path.join(hook_dir, "run_nitd=0000003.dctn")
    got, last, extras, _ = _train_sgd(SEEDS_B, stop_after=7, first_iter=4, load=newest)
    assert last == 7 and extras["num_iters_done"] == 3 and isinstance(extras["loss"], float)
    _assert_same_state(got, want, "resumed FlatSGD run")


# ------------------------------------------------------------------ 3. two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q, path):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist

    from dctn_amd import ddp
    from dctn_amd.training import fused_cross_entropy, train_step

    torch.cuda.set_device(DEV)
    ddp.init_from_env("gloo")
    # every rank its own parameters and seeds, and an explicit shard: nothing is broadcast at construction
    seeds = dict(model=10 + rank, dropout=20 + rank, batch=30 + rank)
    model, opt, src, guard, run = _objects(seeds, rank=rank, world=world)
    if rank == 0:
        for _ in range(2):
            x, y, _ = src.draw()
            train_step(model, x, y, fused_cross_entropy, opt)
        run.snapshot({"num_iters_done": 1}).save(path)
    dist.barrier()
    extras = run.load(path)
    _, _, indices = src.draw()
    torch.cuda.synchronize(DEV)
    q.put((rank, extras, indices.tolist(), src.state_dict(), src.seed, model.dropout_state_dict(), opt.t,
           opt.flat.view(torch.int16).cpu().numpy(), opt.master.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_load_rank_0s_file_and_draw_their_shards(tmp_path):
    import torch.multiprocessing as mp

    from dctn_amd import batches

    ctx = mp.get_context("spawn")   # fresh child processes
    q, port, path = ctx.Queue(), _free_port(), str(tmp_path / "rank0.dctn")
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, path)) for r in range(2)]
    for p in procs:
        p.start()
    got = {rank: rest for rank, *rest in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank in range(2):
        extras, indices, state, seed, drop, t, flat, master = got[rank]
        assert extras == {"num_iters_done": 1} and seed == 30 and state == {"seed": 30, "batches_done": 3}
        assert indices == batches.expected_indices(30, 2, N_SAMPLES, GLOBAL_BATCH, rank, 2)
        assert drop == {"seed": 20, "draws_done": 2} and t == 2
    assert np.array_equal(got[0][6], got[1][6]) and np.array_equal(got[0][7], got[1][7])
    assert not set(got[0][1]) & set(got[1][1])
