"""What the device-side weight average (EMA) costs a graphed training iteration, and what it buys, in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) as a GraphedTrainStep whose graph draws its own batches from a
`DeviceBatches` source over `--samples` synthetic 28 x 28 uint8 images, with K = 1 and K = 20 iterations per launch:

  A   the parent's loop, no average.  With `--parent-lib PATH` (a libdctn_amd.so built from the parent commit, in the
      dctn_amd directory of a checkout of that commit) A is that tree's Python over that library's kernels, imported
      beside this build under another name; without it A is a second instance of this build's loop ("parent_lib": null
      in the result) - either way A against B shows the run's own noise
  B   this build, no average: `FlatAdam(...)`
  C   this build, the average in the step: `FlatAdam(..., ema=WeightEMA(dev, 0.999))`
  D   the alternative a user has today: the average as captured torch ops behind `opt.step()` - one `lerp_` of a float32
      copy of the master towards the master, one more graph node per iteration

Each variant is timed over `--repeats` blocks of `--steps` iterations with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per K and
variant the median, min and max of the per-iteration time over the blocks (us) and their spread, and B - A (must sit
inside A's spread: the same machine code), C - B (the feature's price) and C - D (what fusing buys over the extra node).

    python tools/time_weight_ema.py [--steps 10000] [--repeats 5] [--samples 50000] [--variants A,B,C,D] [--iters 1,20]
                                    [--parent-lib PATH]
"""
import argparse
import importlib
import importlib.util
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
from dctn_amd.training import FlatAdam, GraphedTrainStep, WeightEMA, fused_cross_entropy  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024
LR, L2, DECAY = 1e-4, 1e-4, 0.999


def parent_package(lib_path):
    """The `dctn_amd` package that holds the parent's library, imported as `dctn_parent`: its own Python over its own
    library (this build's `step()` calls entry points the parent's library does not have)."""
    path = os.path.dirname(os.path.abspath(lib_path))
    spec = importlib.util.spec_from_file_location("dctn_parent", os.path.join(path, "__init__.py"),
                                                  submodule_search_locations=[path])
    module = importlib.util.module_from_spec(spec)
    sys.modules["dctn_parent"] = module
    spec.loader.exec_module(module)
    assert os.path.samefile(module._lib.LIB_PATH, lib_path)
    return module


class TorchOpsEMA:
    """A FlatAdam and, behind its step, the average as torch ops on a float32 copy of the master: what a GraphedTrainStep
    captures as one more node per iteration"""

    def __init__(self, optimizer, decay):
        self.optimizer, self.weight = optimizer, 1.0 - decay
        self.shadow = optimizer.master.clone()

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none)

    def step(self):
        self.optimizer.step()
        self.shadow.lerp_(self.optimizer.master, self.weight)


def make_variant(name, K, images, labels, dev, parent):
    """Returns a callable that runs one launch (K iterations)."""
    if name == "A" and parent is not None:   # the parent's classes: construction, warm-up and capture go through its library
        T, M = importlib.import_module("dctn_parent.training"), importlib.import_module("dctn_parent.eps_plus_linear")
        src = importlib.import_module("dctn_parent.batches").DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
        torch.manual_seed(0)
        model = M.EPSesPlusLinear(SPEC, M.UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
        opt = T.FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=LR, l2=L2, master_weights=True)
        return T.GraphedTrainStep(model, None, None, T.fused_cross_entropy, opt, warmup=2, batch_source=src,
                                  iters_per_launch=K)
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    kw = {"ema": WeightEMA(dev, DECAY, warmup=False)} if name == "C" else {}
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=LR, l2=L2, master_weights=True, **kw)
    if name == "D":
        opt = TorchOpsEMA(opt, DECAY)
    src = DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
    return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src, iters_per_launch=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--variants", default="A,B,C,D")
    ap.add_argument("--iters", default="1,20")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    parent = parent_package(args.parent_lib) if args.parent_lib else None
    result = {"workload": "cfg2 bf16 B=1024 FlatAdam(master) graphed, batch source", "samples": args.samples,
              "steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "parent_lib": args.parent_lib,
              "parent_version": None if parent is None else parent._lib.lib().dctn_version(), "version": L.lib().dctn_version(),
              "ema": f"decay {DECAY}, no warm-up; D: lerp_ on a float32 copy of the master behind opt.step()", "K": {}}
    for K in [int(k) for k in args.iters.split(",")]:
        launches = max(args.steps // K, 1)
        runs = {v: make_variant(v, K, images, labels, dev, parent) for v in names}
        times = {v: [] for v in names}
        for v in names:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
            for _ in range(min(launches, max(200 // K, 1))):
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
                print(f"K {K} repeat {r} {v}: {times[v][-1]:.2f} us/iteration", file=sys.stderr, flush=True)
        entry = {"variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                                  "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                              for v, t in times.items()}}
        med = {v: entry["variants"][v]["median_us"] for v in names}
        for hi, lo in (("B", "A"), ("C", "B"), ("C", "D")):
            if hi in med and lo in med:
                entry[f"{hi}_minus_{lo}_us"] = med[hi] - med[lo]
        if "A" in med:
            entry["A_spread_us"] = entry["variants"]["A"]["spread_us"]
        result["K"][str(K)] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
