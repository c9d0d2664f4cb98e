"""What the gradient guard costs a graphed training iteration, three ways, in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) as a GraphedTrainStep whose graph draws its own batches from a
`DeviceBatches` source over `--samples` synthetic 28 x 28 uint8 images:

  U   unguarded: the iteration as it is without a guard (one optimizer launch)
  G   guarded: `FlatAdam(..., guard=GradGuard(dev, max_norm))` - the check and the guarded step, two launches, and
      nothing read by the host
  S   unguarded, with the per-iteration read of the stop-on-NaN-loss hook (`bool(torch.isfinite(loss))` after every
      replay): what a run pays today for the reference's stopper

Each variant is timed over `--repeats` blocks of `--steps` iterations with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per variant the
median, min and max of the per-iteration time over the blocks (us) and their spread, G - U (the cost of the guard) and
S - U (the cost of the host read), the run's own spread beside them, and the guard's block at the end.

    python tools/time_grad_guard.py [--steps 10000] [--repeats 5] [--samples 50000] [--max-norm 1.0] [--variants U,G,S]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.batches import DeviceBatches  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GradGuard, GraphedTrainStep, fused_cross_entropy  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024


def make_variant(name, images, labels, dev, max_norm):
    """Returns (callable that runs one iteration, the guard or None)."""
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    guard = GradGuard(dev, max_norm=max_norm) if name == "G" else None
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4, master_weights=True,
                   guard=guard)
    src = DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src)
    if name in ("U", "G"):
        return step, guard
    if name == "S":
        def run():
            if not bool(torch.isfinite(step()["loss"])):
                raise RuntimeError("non-finite loss")

        return run, None
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--variants", default="U,G,S")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    runs = {v: make_variant(v, images, labels, dev, args.max_norm) for v in names}
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
    result = {"workload": "cfg2 bf16 B=1024 FlatAdam(master) graphed, batch source", "samples": args.samples,
              "steps": args.steps, "repeats": args.repeats, "max_norm": args.max_norm, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev),
              "variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                               "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                           for v, t in times.items()}}
    med = {v: result["variants"][v]["median_us"] for v in names}
    result["largest_spread_us"] = max(result["variants"][v]["spread_us"] for v in names)
    if "G" in med and "U" in med:
        result["G_minus_U_us"] = med["G"] - med["U"]
    if "S" in med and "U" in med:
        result["S_minus_U_us"] = med["S"] - med["U"]
    if "G" in runs:
        result["guard"] = runs["G"][1].read()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
