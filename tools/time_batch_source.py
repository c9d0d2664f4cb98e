"""Training iteration with its input: where the batch comes from, four ways, in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) as a GraphedTrainStep over `--samples` synthetic 28 x 28 uint8 images:

  C   the replay alone, on a fixed batch that already sits in the static buffers (no input at all: the floor)
  A   the reference's way with real data: the expanded data set as a CPU tensor, a host `randperm` per epoch, a slice of
      it, CPU indexing, a pinned copy, `step(x, y)`
  A2  the best without the batch source: the expanded data set resident on the device, a device `randperm` per epoch,
      eager `torch.index_select` into `step.x` / `step.y`, then the replay
  B   `GraphedTrainStep(batch_source=DeviceBatches(...))`: the draw is the first node of the graph

Each variant is timed over `--repeats` blocks of `--steps` iterations with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per variant the
median, min and max of the per-iteration time over the blocks (us), the spread (max - min) of each, B - C (the cost of the
draw inside the graph) with A2 - C beside it, and whether B is below A and below A2 by more than the run's own spread (the
largest spread among the variants compared).  The draw kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with `--variants B`.

    python tools/time_batch_source.py [--steps 10000] [--repeats 5] [--samples 50000] [--variants C,A,A2,B]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.batches import DeviceBatches, feature_table  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, fused_cross_entropy  # noqa: E402
from dctn_amd.window_stats import φ_cos_sin_squared_1  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024


def make_model(dev):
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4, master_weights=True)
    return model, opt


def make_variant(name, images, labels, dev):
    """Returns a callable that runs one iteration (and whatever object must stay alive)."""
    n = images.shape[0]
    model, opt = make_model(dev)
    if name == "B":
        src = DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
        step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src)
        return step, src
    x_cpu = feature_table(φ_cos_sin_squared_1, 1.0, DTYPE)[images.long()].unsqueeze(0)   # (1, n, 28, 28, 2)
    step = GraphedTrainStep(model, x_cpu[:, :BATCH].to(dev), labels[:BATCH].to(dev), fused_cross_entropy, opt, warmup=2)
    steps_per_epoch = n // BATCH
    if name == "C":
        return (lambda: step(step.x, step.y)), step
    if name == "A":
        state = {"k": 0, "perm": None}
        pin_x = torch.empty((1, BATCH, SIZE, SIZE, 2), dtype=DTYPE).pin_memory()
        pin_y = torch.empty(BATCH, dtype=torch.int64).pin_memory()

        def run():
            k = state["k"] % steps_per_epoch
            if k == 0:
                state["perm"] = torch.randperm(n)
            idx = state["perm"][k * BATCH : (k + 1) * BATCH]
            torch.index_select(x_cpu, 1, idx, out=pin_x)
            torch.index_select(labels, 0, idx, out=pin_y)
            step(pin_x, pin_y)   # the step's copies into its static buffers are the host-to-device copies
            torch.cuda.current_stream(dev).synchronize()   # the pinned buffers are rewritten by the next iteration
            state["k"] += 1

        return run, step
    if name == "A2":
        x_dev, y_dev = x_cpu.to(dev), labels.to(dev)
        state = {"k": 0, "perm": None}

        def run():
            k = state["k"] % steps_per_epoch
            if k == 0:
                state["perm"] = torch.randperm(n, device=dev)
            idx = state["perm"][k * BATCH : (k + 1) * BATCH]
            torch.index_select(x_dev, 1, idx, out=step.x)
            torch.index_select(y_dev, 0, idx, out=step.y)
            step(step.x, step.y)
            state["k"] += 1

        return run, step
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--variants", default="C,A,A2,B")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    runs = {v: make_variant(v, images, labels, dev) for v in names}
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
    result = {"workload": "cfg2 bf16 B=1024 FlatAdam(master) graphed", "samples": args.samples, "steps": args.steps,
              "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev),
              "variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                               "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                           for v, t in times.items()}}
    med = {v: result["variants"][v]["median_us"] for v in names}
    spread = {v: result["variants"][v]["spread_us"] for v in names}
    if "B" in med and "C" in med:
        result["B_minus_C_us"] = med["B"] - med["C"]
    if "A2" in med and "C" in med:
        result["A2_minus_C_us"] = med["A2"] - med["C"]
    for other in ("A", "A2"):
        if "B" in med and other in med:
            result[f"B_below_{other}_beyond_spread"] = med[other] - med["B"] > max(spread["B"], spread[other])
    if "B" in runs:
        result["batches_done_B"] = runs["B"][1].state_dict()["batches_done"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
