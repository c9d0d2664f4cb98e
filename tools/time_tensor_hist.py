"""What the output histograms cost a graphed training step, in one process.

Three layers, B = 128, 28 x 28, float32, at each bond of `--bonds`; every variant is the whole `GraphedTrainStep`: batch
drawn from a `DeviceBatches(phi=quantum_phi(False))`, forward, fused cross-entropy, backward,
`FlatRMSprop(alpha=0.9, momentum=0.9, weight_decay=1e-4)`:

  none       no histograms (the parent's step)
  period1    `model.output_histograms = OutputHistograms(dev, names, period=1)`: one `dctn_tensor_hist` launch more per
             forward, every launch recorded
  period20   the same with `period=20`: nineteen launches of twenty read nothing
  torch      the only capturable torch formulation: per string `torch.bucketize(y.double(), edges, right=True)` and an
             `index_add_` of ones into a fixed int64 count tensor (uniform-bin `histc` cannot hold these buckets,
             `torch.histogram` has no GPU kernel, `bincount` synchronises)

Each variant is timed over `--repeats` blocks of `--steps` replays with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per bond and
variant the median, min and max of the per-replay time over the blocks (us), their spread, and the differences to `none`.

    python tools/time_tensor_hist.py [--steps 2000] [--repeats 5] [--bonds 2,4] [--samples 4096] [--variants ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd import _lib as L  # noqa: E402
from dctn_amd import batches, training  # noqa: E402
from dctn_amd.conv_sbs import DumbNormalInitialization  # noqa: E402
from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi  # noqa: E402
from dctn_amd.tensor_hist import OutputHistograms, tensorboard_edges  # noqa: E402

BATCH, SIZE = 128, 28
ALL = ("none", "period1", "period20", "torch")


class TorchHistograms:
    """`OutputHistograms`' ``record`` in torch ops: counts[k] = elements with exactly k edges <= v (k = 0: below the
    table; k = n_edges: at or above the last edge), NaN where bucketize puts it."""

    def __init__(self, dev, names):
        self.edges = torch.from_numpy(tensorboard_edges()).to(dev)
        self.counts = [torch.zeros(self.edges.numel() + 1, dtype=torch.int64, device=dev) for _ in names]
        self.ones = {}

    def record(self, tensors):
        for counts, t in zip(self.counts, tensors):
            flat = t.detach().reshape(-1)
            ones = self.ones.get(flat.numel())
            if ones is None:   # made in the eager warm-up, never inside the capture
                ones = self.ones[flat.numel()] = torch.ones(flat.numel(), dtype=torch.int64, device=flat.device)
            counts.index_add_(0, torch.bucketize(flat.double(), self.edges, right=True), ones)


def make_variant(name, bond, images, labels, dev):
    torch.manual_seed(0)
    src = batches.DeviceBatches(images, labels, BATCH, dtype=torch.float32, seed=2024, phi=quantum_phi(False), device=dev)
    x, _, _ = src.gather(torch.arange(BATCH, device=dev))
    model = DCTNMnistModel(3, bond, False, DumbNormalInitialization((2 * bond) ** -0.5 * 1.3), False, 1.0).to(dev)
    model.scale_layers_using_batch(x)
    if name in ("period1", "period20"):
        model.output_histograms = OutputHistograms(dev, model.string_names(), period=1 if name == "period1" else 20)
    elif name == "torch":
        model.output_histograms = TorchHistograms(dev, model.string_names())
    opt = training.FlatRMSprop(list(model.parameters()), lr=1e-5, alpha=0.9, momentum=0.9, weight_decay=1e-4)
    return training.GraphedTrainStep(model, None, None, training.fused_cross_entropy, opt, warmup=2, batch_source=src)


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
    result = {"workload": f"ConvSBS classifier, three layers, float32, B={BATCH}, {SIZE}x{SIZE}, graphed step, FlatRMSprop",
              "steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "version": L.lib().dctn_version(), "bond": {}}
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
        for v in names:
            if v != "none" and "none" in med:
                entry[f"{v}_minus_none_us"] = med[v] - med["none"]
        for v in ("period1", "period20"):   # what the device says it did
            if v in runs:
                got = runs[v].model.output_histograms.read()
                entry[f"{v}_calls_recorded"] = sorted({(e["calls"], e["recorded"]) for e in got.values()})
        result["bond"][str(bond)] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
