"""What the ConvSBS classifier costs as a model, in one process.

Three layers, B = 128, 28 x 28, float32, at each bond of `--bonds`; every variant is a captured graph:

  helper     `tests/sbs_classifier.ConvSBSClassifier(reference_form=True)`, forward + cross-entropy + backward: torch ops for
             the mean over positions, a `torch.stack` between the layers (what tools/time_sbs_classifier.py times)
  model      `DCTNMnistModel`, the same: one stacked buffer per layer, `position_mean`
  stats      `model` with `output_stats` attached: one `dctn_tensor_stats` launch more per forward
  step       the whole `GraphedTrainStep`: batch drawn from a `DeviceBatches(phi=quantum_phi(False))`, forward, fused
             cross-entropy, backward, `FlatRMSprop(alpha=0.9, momentum=0.9, weight_decay=1e-4)`
  step_stats `step` with `output_stats` attached

Each variant is timed over `--repeats` blocks of `--steps` replays with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per bond and
variant the median, min and max of the per-replay time over the blocks (us), their spread, and the differences
model - helper, stats - model, step_stats - step.

    python tools/time_mnist_model.py [--steps 2000] [--repeats 5] [--bonds 2,4] [--samples 4096] [--variants ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd import _lib as L  # noqa: E402
from dctn_amd import batches, training  # noqa: E402
from dctn_amd.conv_sbs import DumbNormalInitialization  # noqa: E402
from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi  # noqa: E402
from dctn_amd.tensor_stats import OutputStats  # noqa: E402
from tests.sbs_classifier import ConvSBSClassifier  # noqa: E402

BATCH, SIZE = 128, 28
ALL = ("helper", "model", "stats", "step", "step_stats")


def graphed(fn, dev):
    """`fn` captured after two eager runs; returns the replay."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def make_variant(name, bond, images, labels, dev):
    torch.manual_seed(0)
    src = batches.DeviceBatches(images, labels, BATCH, dtype=torch.float32, seed=2024, phi=quantum_phi(False), device=dev)
    x, y, _ = src.gather(torch.arange(BATCH, device=dev))
    if name == "helper":
        model = ConvSBSClassifier(bond=bond, reference_form=True).to(dev)
        model.calibrate(x)
    else:
        model = DCTNMnistModel(3, bond, False, DumbNormalInitialization((2 * bond) ** -0.5 * 1.3), False, 1.0).to(dev)
        model.scale_layers_using_batch(x)
        if name in ("stats", "step_stats"):
            model.output_stats = OutputStats(dev, model.string_names())
    if name in ("step", "step_stats"):
        opt = training.FlatRMSprop(list(model.parameters()), lr=1e-5, alpha=0.9, momentum=0.9, weight_decay=1e-4)
        return training.GraphedTrainStep(model, None, None, training.fused_cross_entropy, opt, warmup=2, batch_source=src)

    def forward_backward():
        for p in model.parameters():
            p.grad = None
        F.cross_entropy(model(x), y).backward()

    model.train()
    return graphed(forward_backward, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bonds", default="2,4")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    assert all(v in ALL for v in names)
    result = {"workload": f"ConvSBS classifier, three layers, float32, B={BATCH}, {SIZE}x{SIZE}, graphed", "steps": args.steps,
              "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev),
              "torch": torch.__version__, "version": L.lib().dctn_version(), "bond": {}}
    for bond in [int(b) for b in args.bonds.split(",")]:
        runs = {v: make_variant(v, bond, images, labels, dev) for v in names}
        times = {v: [] for v in names}
        for v in names:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
            for _ in range(min(args.steps, 200)):
                runs[v]()
        for r in range(args.repeats):
            for v in names:   # alternating
                run = runs[v]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run()
                torch.cuda.synchronize(dev)
                times[v].append((time.perf_counter() - t0) * 1e6 / args.steps)
                print(f"bond {bond} repeat {r} {v}: {times[v][-1]:.2f} us", file=sys.stderr, flush=True)
        entry = {"variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                                  "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                              for v, t in times.items()}}
        med = {v: entry["variants"][v]["median_us"] for v in names}
        for hi, lo in (("model", "helper"), ("stats", "model"), ("step_stats", "step")):
            if hi in med and lo in med:
                entry[f"{hi}_minus_{lo}_us"] = med[hi] - med[lo]
        result["bond"][str(bond)] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
