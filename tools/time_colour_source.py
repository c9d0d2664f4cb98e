"""Training iteration of the colour model with its input: the raw-bytes colour source against the expanded tensor, in one
process.

cfg4_eps36 (EPSesPlusLinear(((3, 6),), Q_0 = 4, image_size = 32), float32, B = 128, FlatAdam) as a GraphedTrainStep over
`--samples` synthetic (n, 32, 32, 3) uint8 images with a constant channel, per-channel moments and nu:

  A   `GraphedTrainStep(batch_source=DeviceBatches.from_colour(...))`: the bytes stay bytes on the device, the draw is the
      first node of the graph and looks every value up in the per-channel tables
  B   the same with `DeviceBatches.from_features` over the data set expanded on the host to (1, n, 32, 32, 4) float32:
      the draw is a row copy
  C   the replay alone, on a fixed batch that already sits in the static buffers (no input at all: the floor)

Each variant is timed over `--repeats` blocks of `--steps` iterations with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per variant the
median, min and max of the per-iteration time over the blocks (us) and their spread (max - min), A - B and A - C, and the
bytes each source holds on the device (data set, table, labels).  There is no threshold: the step takes milliseconds and
the draw microseconds, so A = B within the spread is the expected outcome; what the colour source gains is memory and a
constructor that takes the raw data.

    python tools/time_colour_source.py [--steps 2000] [--repeats 5] [--samples 45000] [--variants A,B,C]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.batches import DeviceBatches, channel_moments, colour_table  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, fused_cross_entropy  # noqa: E402

SPEC, SIZE, Q0, DTYPE, BATCH = ((3, 6),), 32, 4, torch.float32, 128
NU, CONSTANT = (1.2, 1.1, 1.3), 1.0


def make_model(dev):
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE, Q_0=Q0)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4)
    return model, opt


def footprint(src):
    tensors = [src.src, src.labels] + ([] if src.table is None else [src.table])
    return sum(t.numel() * t.element_size() for t in tensors)


def expand(images, mean, std):
    """(1, n, 32, 32, 4) float32 on the host: the per-channel tables indexed by the bytes (bit for bit the reference's
    pipeline on the expanded tensor; tests/test_host_colour_source.py)."""
    table = colour_table(3, nu=NU, mean=mean, std=std, constant_channel=CONSTANT, dtype=DTYPE)
    cols = [table[c][images[..., c].long()] for c in range(3)] + [table[3][torch.zeros_like(images[..., 0]).long()]]
    return torch.stack(cols, dim=-1).unsqueeze(0)


def make_variant(name, images, labels, mean, std, dev):
    """Returns a callable that runs one iteration, the source (or None) and whatever must stay alive."""
    model, opt = make_model(dev)
    if name == "A":
        src = DeviceBatches.from_colour(images, labels, BATCH, dtype=DTYPE, seed=2024, nu=NU, mean=mean, std=std,
                                        constant_channel=CONSTANT)
        return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src), src
    if name == "B":
        src = DeviceBatches.from_features(expand(images, mean, std), labels, BATCH, seed=2024)
        return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src), src
    if name == "C":
        x = expand(images[:BATCH], mean, std).to(dev)
        step = GraphedTrainStep(model, x, labels[:BATCH].to(dev), fused_cross_entropy, opt, warmup=2)
        return (lambda: step(step.x, step.y)), None, step
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=45000)
    ap.add_argument("--variants", default="A,B,C")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    mean, std = channel_moments(images)
    names = args.variants.split(",")
    runs = {v: make_variant(v, images, labels, mean, std, dev) for v in names}
    times = {v: [] for v in names}
    for v in names:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
        for _ in range(min(args.steps, 200)):
            runs[v][0]()
    for r in range(args.repeats):
        for v in names:   # alternating
            run = runs[v][0]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            torch.cuda.synchronize(dev)
            times[v].append((time.perf_counter() - t0) * 1e6 / args.steps)
            print(f"repeat {r} {v}: {times[v][-1]:.2f} us/step", file=sys.stderr, flush=True)
    result = {"workload": "cfg4_eps36 f32 B=128 FlatAdam graphed", "samples": args.samples, "steps": args.steps,
              "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev),
              "variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                               "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                           for v, t in times.items()},
              "source_bytes": {v: footprint(runs[v][1]) for v in names if runs[v][1] is not None}}
    med = {v: result["variants"][v]["median_us"] for v in names}
    for a, b in (("A", "B"), ("A", "C"), ("B", "C")):
        if a in med and b in med:
            result[f"{a}_minus_{b}_us"] = med[a] - med[b]
    if "A" in med and "B" in med:
        result["largest_spread_A_B_us"] = max(result["variants"]["A"]["spread_us"], result["variants"]["B"]["spread_us"])
    for v in names:
        if runs[v][1] is not None:
            result[f"batches_done_{v}"] = runs[v][1].state_dict()["batches_done"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
