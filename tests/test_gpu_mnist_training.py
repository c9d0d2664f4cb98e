"""The ConvSBS classifier under the graphed training recipe on the GPU (`-m gpu`): `DCTNMnistModel` with a device batch
source, `FlatRMSprop`, the per-epoch rate schedule and the output statistics, as ONE graph per iteration (or per two).

64 random 10 x 10 byte images in global batches of 16, three layers at bond 2, calibrated on the first batch.  The graphed
iterations are held bit for bit against eager `train_step` calls on the same draws, and the float32 trajectory against a
float64 restatement in plain torch on the CPU (tests/mnist_reference.py: `oracle.ref_cpu.convsbs_forward`,
`torch.optim.RMSprop`), judged by that restatement's own float32 run.  On so small a random data set the calibrated
model answers the first batch only (the outputs of nine-core strings are heavy-tailed: the loss of the later batches is
ln 10), and RMSprop divides gradients that float32 flushes to zero, so the float32 yardstick itself is some tenths of the
distance moved; the figures are printed before they are asserted (run with -s)."""
import functools

import pytest
import torch

from dctn_amd import batches
from dctn_amd.conv_sbs import DumbNormalInitialization
from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi
from dctn_amd.tensor_stats import OutputStats
from tests import mnist_reference as MR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N, BATCH, SIZE, ITERATIONS = 64, 16, 10, 4
MODEL_SEED, DATA_SEED, BATCH_SEED = 8, 108, 5
MULTIPLIER = 1.0
RATES, STEPS_PER_EPOCH = [2e-5, 1e-4], N // BATCH
HYPER = dict(alpha=0.9, momentum=0.9, weight_decay=1e-4)


@functools.lru_cache(maxsize=None)
def _data():
    g = torch.Generator().manual_seed(DATA_SEED)
    return torch.randint(0, 256, (N, SIZE, SIZE), generator=g, dtype=torch.uint8), torch.randint(0, 10, (N,), generator=g)


def _initial_model():
    torch.manual_seed(MODEL_SEED)
    return DCTNMnistModel(3, 2, False, DumbNormalInitialization(0.65), False, MULTIPLIER)


def _source(**kw):
    images, labels = _data()
    return batches.DeviceBatches(images, labels, BATCH, dtype=torch.float32, seed=BATCH_SEED, scale=MULTIPLIER,
                                 phi=quantum_phi(False), device=DEV, **kw)


def _objects():
    """Model (calibrated on the first batch), optimizer, source; the statistics attached."""
    from dctn_amd.training import FlatRMSprop, LRSchedule

    model = _initial_model().to(DEV)
    src = _source()
    x0, _, _ = src.gather(torch.tensor(src.expected_indices(0), device=DEV))
    model.scale_layers_using_batch(x0)
    opt = FlatRMSprop(list(model.parameters()), lr=RATES[0], schedule=LRSchedule.per_epoch(DEV, RATES, STEPS_PER_EPOCH), **HYPER)
    model.output_stats = OutputStats(DEV, model.string_names())
    return model, opt, src


def _state(model, opt):
    torch.cuda.synchronize()
    return dict(flat=opt.flat.clone(), square_avg=opt.square_avg.clone(), buf=opt.buf.clone(), t=opt.t,
                stats=model.output_stats.raw().tobytes())


@functools.lru_cache(maxsize=None)
def _eager():
    """Four eager `train_step` calls on the batches the source will draw: the state after each, and the losses."""
    from dctn_amd.training import fused_cross_entropy, train_step

    model, opt, src = _objects()
    states, losses = [], []
    for k in range(ITERATIONS):
        x, y, _ = src.gather(torch.tensor(src.expected_indices(k), device=DEV))
        out = train_step(model, x, y, fused_cross_entropy, opt)
        states.append(_state(model, opt))
        losses.append(float(out["loss"]))
    assert src.state_dict()["batches_done"] == 0   # gather reads no state
    return states, losses


def _assert_same(got, want, what):
    for key in ("flat", "square_avg", "buf"):
        assert torch.equal(got[key], want[key]), f"{what}: {key} differs"
    assert got["t"] == want["t"] and got["stats"] == want["stats"], f"{what}: step count or statistics record differ"


def test_four_graphed_iterations_equal_four_eager_ones_bit_for_bit():
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    eager, eager_losses = _eager()
    model, opt, src = _objects()
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src)
    _assert_same(_state(model, opt), eager[0], "iteration 1 (the warm-up)")
    for k in range(1, ITERATIONS):
        out = step()
        assert out["indices"].tolist() == src.expected_indices(k)
        _assert_same(_state(model, opt), eager[k], f"iteration {k + 1}")
        assert float(out["loss"].detach()) == eager_losses[k]
    stats = model.output_stats.read()
    assert [s["seq"] for s in stats.values()] == [ITERATIONS] * 5 and opt.t == ITERATIONS
    assert src.state_dict()["batches_done"] == ITERATIONS
    assert not torch.equal(eager[0]["flat"], eager[-1]["flat"])
    for name, s in stats.items():
        print(f"{name}: std {s['std']:.4e} mean |y| {s['mean_abs']:.4e} max |y| {s['max_abs']:.4e} nonfinite {s['nonfinite']}")
        assert s["n"] > 0 and s["nonfinite"] == 0


def test_two_iterations_per_launch_leave_the_same_state():
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    eager, eager_losses = _eager()
    model, opt, src = _objects()
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src, iters_per_launch=2)
    _assert_same(_state(model, opt), eager[1], "iteration 2 (the second warm-up)")
    out = step()
    assert out["iters"] == 2 and out["indices"].tolist() == src.expected_indices(3)
    _assert_same(_state(model, opt), eager[3], "iteration 4 (the end of the launch)")
    assert float(out["loss"].detach()) == eager_losses[3]
    assert [s["seq"] for s in model.output_stats.read().values()] == [ITERATIONS] * 5


def test_the_float32_trajectory_against_the_float64_restatement():
    eager, losses = _eager()
    images, labels = _data()
    table = batches.feature_table(quantum_phi(False), MULTIPLIER, torch.float32)
    template = _initial_model()
    lay = MR.layout(template)
    initial = [p.detach().clone() for p in template.parameters()]

    def batch(k, dtype):
        idx = torch.tensor(batches.expected_indices(BATCH_SEED, k, N, BATCH))
        return table[images[idx].long()].unsqueeze(0).to(dtype), labels[idx]

    runs = {}
    for dtype in (torch.float64, torch.float32):
        start = MR.calibrate([c.to(dtype) for c in initial], lay, batch(0, dtype)[0])
        run_losses, final = MR.train(start, lay, [batch(k, dtype) for k in range(ITERATIONS)], RATES, STEPS_PER_EPOCH, **HYPER)
        runs[dtype] = dict(start=start, losses=run_losses, final=final)
    ref64, ref32 = runs[torch.float64], runs[torch.float32]
    flat = lambda cores: torch.cat([c.detach().cpu().double().flatten() for c in cores])
    moved = float((flat(ref64["final"]) - flat(ref64["start"])).norm())
    e_hip = float((eager[-1]["flat"].cpu().double() - flat(ref64["final"])).norm()) / moved
    e_ref = float((flat(ref32["final"]) - flat(ref64["final"])).norm()) / moved
    d_hip = max(abs(a - b) for a, b in zip(losses, ref64["losses"]))
    d_ref = max(abs(a - b) for a, b in zip(ref32["losses"], ref64["losses"]))
    ulp = MR.ulp32(max(ref64["losses"]))
    print(f"\nlosses (float64): {ref64['losses']}\nparameters: e_hip={e_hip:.4e} e_torch32={e_ref:.4e} (bound {4 * e_ref:.4e}); "
          f"loss: hip {d_hip:.4e} torch32 {d_ref:.4e} (bound {max(4 * d_ref, ulp):.4e}, ulp {ulp:.2e})")
    assert e_hip <= 4 * e_ref
    assert d_hip <= max(4 * d_ref, ulp)


def test_graphed_score_over_a_padded_source_equals_score_fused():
    from dctn_amd.evaluation import GraphedScore, score_fused
    from dctn_amd.training import GraphedTrainStep, fused_cross_entropy

    model, opt, src = _objects()
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=1, batch_source=src)
    images, labels = _data()
    val = lambda: batches.DeviceBatches(images[:40], labels[:40], BATCH, dtype=torch.float32, seed=1, scale=MULTIPLIER,
                                        phi=quantum_phi(False), device=DEV, shuffle=False)
    scorer = GraphedScore(model, val())
    assert scorer.src.padded_steps == 3
    before = (model.output_stats.raw().tobytes(), src.state_dict()["batches_done"], opt.flat.clone())
    got = scorer()
    eager_src = val()

    def padded_batches():
        for _ in range(eager_src.padded_steps):
            out = eager_src.empty_batch()
            eager_src.draw_padded_into(*out)
            yield out

    model.eval()
    want = score_fused(model, padded_batches(), DEV)
    model.train()
    print(f"\nscore over 40 samples in 3 padded batches: graphed {got}, eager {want}")
    assert got == want and scorer.rows == 40
    assert model.training
    assert (model.output_stats.raw().tobytes(), src.state_dict()["batches_done"]) == before[:2] and torch.equal(opt.flat, before[2])
    step()
    assert [s["seq"] for s in model.output_stats.read().values()] == [2] * 5 and src.state_dict()["batches_done"] == 2
