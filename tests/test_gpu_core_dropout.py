"""Fused component dropout on the GPU (`-m gpu`): the raw C-ABI against the Python restatement of the mask and torch's
own arithmetic on the CPU (bit for bit), the device draw counter, the model path against the float64 oracle on the
masked cores, gradients that stay in place for the flat optimizers, graph replay, the gate, and two ranks."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import dctn_amd
from dctn_amd import _lib as L
from dctn_amd import dropout as D
from oracle import ref_cpu as R
from tests.test_gpu_parity import bf16_close, close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x0123456789ABCDEF
MARGIN = 64          # elements: a multiple of 16 bytes for every dtype, so a view at MARGIN keeps the base's alignment
SENTINEL = 12345.0   # finite and unlike anything the kernels write
DTYPES = [torch.float32, torch.float64, torch.bfloat16]


class Framed:
    """`n` elements inside a sentinel-filled allocation; `off` = 1 puts the base one element past a 16-byte boundary."""

    def __init__(self, n, dtype, off=0, values=None):
        self.base = torch.full((2 * MARGIN + n + 8,), SENTINEL, dtype=dtype, device=DEV)
        self.lo, self.n = MARGIN + off, n
        self.view = self.base[self.lo : self.lo + n]
        if values is None:
            self.view.fill_(float("nan"))   # an output: whatever it held must not matter
        else:
            self.view.copy_(values)
        assert self.view.data_ptr() % 16 == (off * self.base.element_size()) % 16
        self.before = self.base.clone()

    def margins_intact(self):
        b, a = self.before, self.base
        return torch.equal(a[: self.lo], b[: self.lo]) and torch.equal(a[self.lo + self.n :], b[self.lo + self.n :])

    def untouched(self):   # an input: bit for bit what it was (NaN-free)
        return torch.equal(self.base, self.before)


def _raw(fn, *args):
    L.check(fn(*args), "core dropout")


def _fwd(cores, outs, p, state, record):
    _raw(L.lib().dctn_core_dropout_fwd, L.ptr_array(cores), L.ptr_array(outs), L.i64_array([c.numel() for c in cores]),
         len(cores), p.data_ptr(), state.data_ptr(), record.data_ptr(), L.dtype_code(p), L.stream_ptr(DEV))


def _bwd(gs, outs, p, record):
    _raw(L.lib().dctn_core_dropout_bwd, L.ptr_array(gs), L.ptr_array(outs), L.i64_array([g.numel() for g in gs]), len(gs),
         p.data_ptr(), record.data_ptr(), L.dtype_code(p), L.stream_ptr(DEV))


def _mask(outs, p, record):
    _raw(L.lib().dctn_core_dropout_mask, L.ptr_array(outs), L.i64_array([m.numel() for m in outs]), len(outs), p.data_ptr(),
         record.data_ptr(), L.dtype_code(p), L.stream_ptr(DEV))


def _words(t):
    return [int(v) & 0xFFFFFFFF for v in t.cpu().tolist()]


# three segments (a 2048-element core, a 5-element core, an odd size with a partial last block) and one whose base is one
# element past a 16-byte boundary (element-wise path; what a view into FlatAdam's flat buffer looks like); then 1, 3, 4
LAYOUTS = {"mixed": ((2048, 0), (5, 0), (1031, 0), (77, 1)), "tiny": ((1, 0), (3, 0), (4, 0)),
           "several_workgroups": ((4099, 0), (4101, 1))}   # 2051 blocks of 4: more than two workgroups of 1024 lanes


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("pval", [0.5, 0.9])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64", "bf16"])
def test_raw_abi_against_the_restatement_and_torch_on_the_cpu(dtype, pval, layout):
    segs = LAYOUTS[layout]
    name = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16"}[dtype]
    gen = torch.Generator().manual_seed(1000 + len(segs))
    p_cpu = torch.tensor(pval, dtype=dtype)          # the value the tensor dtype stores: bf16 0.9 is 0.8984375
    if dtype == torch.bfloat16 and pval == 0.9:
        assert float(p_cpu) == 0.8984375
    p = p_cpu.to(DEV)
    draw = 7
    state = D.new_state(SEED, DEV, draws_done=draw)
    record = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    cores_cpu = [torch.randn(n, generator=gen).to(dtype) for n, _ in segs]
    grads_cpu = [torch.randn(n, generator=gen).to(dtype) for n, _ in segs]
    cores = [Framed(n, dtype, off, c) for (n, off), c in zip(segs, cores_cpu)]
    outs = [Framed(n, dtype, off) for n, off in segs]
    _fwd([c.view for c in cores], [o.view for o in outs], p, state, record)
    assert dctn_amd.last_kernel() == f"core_dropout_fwd_{name}"
    masks = [Framed(n, dtype, off) for n, off in segs]
    _mask([m.view for m in masks], p, record)
    assert dctn_amd.last_kernel() == f"core_dropout_mask_{name}"
    d_out = [Framed(n, dtype, off, g) for (n, off), g in zip(segs, grads_cpu)]
    d_core = [Framed(n, dtype, off) for n, off in segs]
    _bwd([g.view for g in d_out], [o.view for o in d_core], p, record)
    assert dctn_amd.last_kernel() == f"core_dropout_bwd_{name}"
    in_place = [Framed(n, dtype, off, g) for (n, off), g in zip(segs, grads_cpu)]
    _bwd([g.view for g in in_place], [g.view for g in in_place], p, record)
    torch.cuda.synchronize()
    assert _words(record) == [SEED & 0xFFFFFFFF, SEED >> 32, draw, 0]
    assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, draw + 1, 0]   # one forward; bwd and mask left it alone
    kept = 0
    for s, (n, _) in enumerate(segs):
        want_mask = torch.tensor(D.expected_keep(SEED, draw, s, n, float(p_cpu))).to(dtype)
        kept += int(want_mask.sum())
        assert torch.equal(masks[s].view.cpu(), want_mask), f"mask of segment {s}"
        # the reference's expression, evaluated by torch on the CPU in the tensor dtype
        assert torch.equal(outs[s].view.cpu(), want_mask * cores_cpu[s] / p_cpu), f"forward of segment {s}"
        want_grad = (grads_cpu[s] / p_cpu) * want_mask
        assert torch.equal(d_core[s].view.cpu(), want_grad), f"backward of segment {s}"
        assert torch.equal(in_place[s].view.cpu(), want_grad), f"in-place backward of segment {s}"
        assert bool((outs[s].view.cpu()[want_mask == 0] == 0).all())
    if layout != "tiny":
        assert 0 < kept < sum(n for n, _ in segs)
    for f in outs + masks + d_core + in_place:
        assert f.margins_intact()
    for f in cores + d_out:
        assert f.untouched()


def test_backward_skips_a_core_without_a_gradient_and_keeps_the_numbering():
    p = torch.tensor(0.5, device=DEV)
    state, record = D.new_state(SEED, DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    cores = [torch.randn(40, device=DEV), torch.randn(24, device=DEV)]
    outs = [torch.empty_like(c) for c in cores]
    _fwd(cores, outs, p, state, record)
    g = torch.randn(24, device=DEV)
    want = (g.cpu() / 0.5) * torch.tensor(D.expected_keep(SEED, 0, 1, 24, 0.5)).float()
    _raw(L.lib().dctn_core_dropout_bwd, L.ptr_array([None, g]), L.ptr_array([None, g]), L.i64_array([1, 24]), 2,
         p.data_ptr(), record.data_ptr(), L.F32, L.stream_ptr(DEV))
    assert torch.equal(g.cpu(), want)


def test_counter_advances_per_forward_and_a_reloaded_state_repeats_the_masks():
    dtype = torch.float32
    p = torch.tensor(0.5, dtype=dtype, device=DEV)
    state = D.new_state(SEED, DEV, draws_done=41)
    cores = [torch.randn(9000, device=DEV), torch.randn(129, device=DEV)]   # 2283 blocks: three workgroups draw tickets
    runs = []
    for k in range(2):
        outs = [torch.full_like(c, float("nan")) for c in cores]
        record = torch.zeros(4, dtype=torch.int32, device=DEV)
        _fwd(cores, outs, p, state, record)
        masks = D.keep_masks(record, p, [c.shape for c in cores], dtype)
        _bwd([torch.ones_like(c) for c in cores], [torch.empty_like(c) for c in cores], p, record)
        assert D.read_state(record) == {"seed": SEED, "draws_done": 41 + k}
        assert _words(state) == [SEED & 0xFFFFFFFF, SEED >> 32, 42 + k, 0]   # +1 per forward only; ticket back at 0
        runs.append((outs, masks))
    assert not torch.equal(runs[0][1][0], runs[1][1][0]) and not torch.equal(runs[0][1][1], runs[1][1][1])
    # a resumed run: {"seed", "draws_done"} as saved before the first of the two launches
    resumed = D.new_state(SEED, DEV, draws_done=41)
    for k in range(2):
        outs = [torch.full_like(c, float("nan")) for c in cores]
        record = torch.zeros(4, dtype=torch.int32, device=DEV)
        _fwd(cores, outs, p, resumed, record)
        for a, b in zip(outs, runs[k][0]):
            assert torch.equal(a, b)
    assert _words(resumed) == _words(state)


# ------------------------------------------------------------------ the model
def _model(spec, dtype, p, seed=5):
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd

    torch.manual_seed(seed)
    return EPSesPlusLinear(spec, UnitTheoreticalOutputStd(), p, DEV, dtype, image_size=10)


def _images(B, dtype, seed=17):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(1, B, 10, 10, generator=g)
    x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype).to(DEV)
    return x, torch.randint(0, 10, (B,), generator=g).to(DEV)


@pytest.mark.parametrize("spec,dtype,B", [(((3, 4), (2, 3)), torch.float32, 6), (((3, 4),), torch.bfloat16, 8)],
                         ids=["f32_two_layers", "bf16_fused_head"])
def test_model_against_the_oracle_on_the_masked_cores(spec, dtype, B, monkeypatch):
    same = close if dtype == torch.float32 else (lambda got, want, _dtype: bf16_close(got, want))
    m = _model(spec, dtype, 0.5)
    keys = set(m.state_dict())
    m.use_fused_dropout(SEED)
    assert set(m.state_dict()) == keys and m.dropout_state_dict() == {"seed": SEED, "draws_done": 0}
    seen = []
    real = D.core_dropout

    def spy(*args):
        out = real(*args)
        seen.append(dctn_amd.last_kernel())
        return out

    monkeypatch.setattr(D, "core_dropout", spy)
    m.train()
    x, _ = _images(B, dtype)
    out = m(x)
    assert seen == ["core_dropout_fwd_" + ("f32" if dtype == torch.float32 else "bf16")]
    out.float().logsumexp(1).sum().backward()
    assert m.dropout_state_dict()["draws_done"] == 1
    assert D.read_state(m.dropout_record) == {"seed": SEED, "draws_done": 0}
    masks = [mk.cpu() for mk in D.keep_masks(m.dropout_record, m.p, [c.shape for c in m.epses], dtype)]
    for s, mk in enumerate(masks):
        want = torch.tensor(D.expected_keep(SEED, 0, s, mk.numel(), float(m.p))).to(dtype).view(mk.shape)
        assert torch.equal(mk, want)
    cores64 = [c.detach().cpu().double().requires_grad_(True) for c in m.epses]
    w64 = m.linear.weight.detach().cpu().double().requires_grad_(True)
    b64 = m.linear.bias.detach().cpu().double().requires_grad_(True)
    want = R.eps_plus_linear_forward([c * mk.double() / float(m.p) for c, mk in zip(cores64, masks)], w64, b64,
                                     x.cpu().double())
    assert same(out, want.detach(), dtype)
    want.logsumexp(1).sum().backward()
    for got, ref, mk in zip(m.epses, cores64, masks):
        assert same(got.grad, ref.grad, dtype)
        assert bool((got.grad.cpu()[mk == 0] == 0).all())          # dropped components get exactly zero gradient
        assert bool((got.grad.cpu()[mk == 1] != 0).any())
    assert same(m.linear.weight.grad, w64.grad, dtype) and same(m.linear.bias.grad, b64.grad, dtype)


def _flat_adam(model):
    from dctn_amd.training import FlatAdam

    return FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=2e-3, weight_decay=1e-3, l2=1e-2)


@pytest.mark.parametrize("p,fused", [(1.0, False), (0.5, True)], ids=["p1", "p05_fused"])
def test_gradients_stay_back_to_back_for_the_flat_optimizer(p, fused):
    from dctn_amd.training import fused_cross_entropy, train_step

    m = _model(((3, 4),), torch.float32, p, seed=3)
    if fused:
        m.use_fused_dropout(SEED)
    opt = _flat_adam(m)
    x, y = _images(16, torch.float32)
    train_step(m, x, y, fused_cross_entropy, opt)
    g = opt._grads()
    assert g.data_ptr() != opt.flat_grad.data_ptr()           # read in place, not gathered
    assert g.data_ptr() == m.epses[0].grad.data_ptr() and g.numel() == opt.n
    if fused:
        assert m.dropout_state_dict()["draws_done"] == 1
        mk = D.keep_masks(m.dropout_record, m.p, [m.epses[0].shape], torch.float32)[0]
        assert bool((m.epses[0].grad[mk == 0] == 0).all())


WARMUP, REPLAYS = 2, 3


def test_graph_replay_draws_one_mask_per_replay_and_matches_eager():
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy, train_step

    x, y = _images(16, torch.float32)
    m = _model(((3, 4),), torch.float32, 0.5, seed=3)
    m.use_fused_dropout(SEED)
    opt = _flat_adam(m)
    step = GraphedTrainStep(m, x, y, fused_cross_entropy, opt, warmup=WARMUP)
    assert m.dropout_state_dict()["draws_done"] == WARMUP      # the capture itself launches nothing
    draws = []
    for _ in range(REPLAYS):
        step(x, y)
        draws.append(D.read_state(m.dropout_record)["draws_done"])
    assert draws == [WARMUP + k for k in range(REPLAYS)]
    assert m.dropout_state_dict() == {"seed": SEED, "draws_done": WARMUP + REPLAYS}
    assert _words(m._dropout_state)[3] == 0
    # eager, from the same seed and state: bit for bit (what tests/test_gpu_flat_adam.py asks of graphed against eager)
    e = _model(((3, 4),), torch.float32, 0.5, seed=3)
    e.use_fused_dropout(SEED)
    eopt = _flat_adam(e)
    for _ in range(WARMUP + REPLAYS):
        train_step(e, x, y, fused_cross_entropy, eopt)
    torch.cuda.synchronize()
    assert e.dropout_state_dict() == m.dropout_state_dict()
    assert eopt.t == opt.t == WARMUP + REPLAYS
    assert torch.equal(eopt.flat, opt.flat) and torch.equal(eopt.m, opt.m) and torch.equal(eopt.v, opt.v)


def test_gate_launches_nothing_at_p_one_or_in_eval_mode():
    x, _ = _images(4, torch.float32)
    one = _model(((3, 4),), torch.float32, 1.0)
    one.use_fused_dropout(SEED)
    one.train()
    one(x)
    assert one.dropout_state_dict()["draws_done"] == 0 and one.dropout_record is None
    half = _model(((3, 4),), torch.float32, 0.5)
    half.use_fused_dropout(SEED)
    half.eval()
    a, b = half(x), half(x)
    assert half.dropout_state_dict()["draws_done"] == 0 and torch.equal(a, b)
    half.train()
    half(x)
    assert half.dropout_state_dict()["draws_done"] == 1
    # the default path is still the torch ops with the pinned-mask hook
    plain = _model(((3, 4),), torch.float32, 0.5)
    plain.train()
    calls = []
    plain.dropout_mask = lambda core, p: calls.append(1) or torch.ones_like(core)
    plain(x)
    assert calls == [1]


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
    from dctn_amd.training import FlatSGD, fused_cross_entropy, make_stopper_after_n_iters, train

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ddp.init_from_env("gloo")
    model = _model(((3, 4),), torch.float32, 0.5, seed=5 + rank)
    model.use_fused_dropout(100 + rank)            # every rank its own seed: the broadcast must make them rank 0's
    x, y = _images(16, torch.float32)
    xs, ys = ddp.shard_batch(x, rank, world), y[rank * 8 : rank * 8 + 8]
    opt = FlatSGD(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=0.05, momentum=0.9)
    records = []
    zero = torch.zeros((), device=dev)
    train([(xs, ys, torch.arange(8))], model, opt, dev, fused_cross_entropy, lambda st_x, st_it: zero, 0.0, [],
          [lambda st_x, st_it: records.append(D.read_state(model.dropout_record))], [make_stopper_after_n_iters(1)])
    mask = D.keep_masks(model.dropout_record, model.p, [model.epses[0].shape], torch.float32)[0]
    q.put((rank, model.dropout_state_dict(), records, mask.cpu().numpy(),
           [p.detach().cpu().numpy() for p in model.parameters()]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_draw_the_same_masks_after_the_broadcast():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: rest for r, *rest in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (state0, records0, mask0, params0), (state1, records1, mask1, params1) = got[0], got[1]
    assert state0 == state1 == {"seed": 100, "draws_done": 2}            # rank 0's seed, two iterations
    assert records0 == records1 == [{"seed": 100, "draws_done": 0}, {"seed": 100, "draws_done": 1}]
    assert (mask0 == mask1).all() and 0 < mask0.sum() < mask0.size
    want = torch.tensor(D.expected_keep(100, 1, 0, mask0.size, 0.5)).float().view(mask0.shape)
    assert torch.equal(torch.from_numpy(mask0), want)
    for a, b in zip(params0, params1):
        assert (a == b).all()
