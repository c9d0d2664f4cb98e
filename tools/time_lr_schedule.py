"""What the device-side learning-rate schedule costs a graphed training iteration, and what it buys, in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) as a GraphedTrainStep whose graph draws its own batches from a
`DeviceBatches` source over `--samples` synthetic 28 x 28 uint8 images, at K = `--iters-per-launch` iterations per launch
(several values: each gets its own set of variants):

  A   the parent's loop, unscheduled.  With `--parent-lib PATH` (a libdctn_amd.so built from the parent commit) its graph
      is captured over that library's kernels; without it A is a second instance of this build's unscheduled loop
      ("parent_lib": null in the result) - the existing instantiations are the parent's instruction for instruction, so
      either way A against B shows the run's own noise
  B   this build, unscheduled: `FlatAdam(lr=...)`, nothing written by the host
  C   this build, scheduled: `FlatAdam(..., schedule=LRSchedule.warmup_cosine(...))` over 64 knots - every iteration
      evaluates the table on the device
  D   this build, unscheduled, with a host write of `opt.lr` in front of every launch: what a user does today, and at
      K > 1 only a staircase of K-iteration treads

Each variant is timed over `--repeats` blocks of `--steps` iterations (`steps / K` launches) with device synchronisation
around each block; the variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one
JSON line: per K and variant the median, min and max of the per-iteration time over the blocks (us) and their spread, and
B - A (must sit inside A's spread), C - B (the feature's price) and C - D (what it buys).

    python tools/time_lr_schedule.py [--steps 10000] [--repeats 5] [--samples 50000] [--iters-per-launch 1,20]
                                     [--variants A,B,C,D] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd import _lib as L  # noqa: E402
from dctn_amd.batches import DeviceBatches  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, LRSchedule, fused_cross_entropy  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024
PEAK, WARMUP = 1e-4, 500


def parent_library(path):
    """The parent's library bound with the signatures it has (the entry points this build added are not in it)."""
    handle = ctypes.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return handle


def make_variant(name, K, images, labels, dev, total, parent):
    """Returns a callable that runs one launch (K iterations)."""
    ours = L.lib()
    if name == "A" and parent is not None:
        L._lib = parent   # construction, warm-up and capture go through the parent's kernels; replays need no binding
    try:
        torch.manual_seed(0)
        model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
        schedule = LRSchedule.warmup_cosine(dev, PEAK, WARMUP, total, final=PEAK / 100) if name == "C" else None
        opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=PEAK, l2=1e-4,
                       master_weights=True, schedule=schedule)
        src = DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
        step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src,
                                iters_per_launch=K)
    finally:
        L._lib = ours
    if name in ("A", "B", "C"):
        return step
    if name == "D":
        mirror = LRSchedule.warmup_cosine("cpu", PEAK, WARMUP, total, final=PEAK / 100)
        done = [2]

        def run():
            opt.lr = mirror.value(done[0])   # the numpy mirror and one tiny device write per launch
            done[0] += K
            step()

        return run
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--iters-per-launch", default="1,20")
    ap.add_argument("--variants", default="A,B,C,D")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    total = args.steps * (args.repeats + 1)
    result = {"workload": "cfg2 bf16 B=1024 FlatAdam(master) graphed, batch source", "samples": args.samples,
              "steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "parent_lib": args.parent_lib,
              "parent_version": None if parent is None else parent.dctn_version(), "version": L.lib().dctn_version(),
              "schedule": f"warmup_cosine, 64 knots, {WARMUP} warm-up steps of {total}", "by_iters_per_launch": {}}
    for K in [int(k) for k in args.iters_per_launch.split(",")]:
        launches = max(args.steps // K, 1)
        runs = {v: make_variant(v, K, images, labels, dev, total, parent) for v in names}
        times = {v: [] for v in names}
        for v in names:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
            for _ in range(max(min(args.steps, 200) // K, 1)):
                runs[v]()
        for r in range(args.repeats):
            for v in names:   # alternating
                run = runs[v]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(launches):
                    run()
                torch.cuda.synchronize(dev)
                times[v].append((time.perf_counter() - t0) * 1e6 / (launches * K))
                print(f"K={K} repeat {r} {v}: {times[v][-1]:.2f} us/iteration", file=sys.stderr, flush=True)
        entry = {"variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                                  "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                              for v, t in times.items()}}
        med = {v: entry["variants"][v]["median_us"] for v in names}
        for hi, lo in (("B", "A"), ("C", "B"), ("C", "D")):
            if hi in med and lo in med:
                entry[f"{hi}_minus_{lo}_us"] = med[hi] - med[lo]
        if "A" in med:
            entry["A_spread_us"] = entry["variants"]["A"]["spread_us"]
        result["by_iters_per_launch"][str(K)] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
