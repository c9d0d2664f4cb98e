"""What one eager `draw_into` and one eager `gather` of a `DeviceBatches` cost the HOST - Python marshalling plus the C
dispatch - in this build and in another tree.

Three sources over 64 images of 8 x 8 pixels, global batch 8, float32: a grey one, a colour one (3 channels and a
constant one) and the colour one augmented (shift 2, flip).  The shapes are small on purpose: a launch is over long
before the host has made the next one, so the queue never pushes back and the clock sees the host alone.  A block is
`--steps` calls timed on the host clock with the device synchronised before the block and after the clock stops.  With
`--other-tree PATH` (a checkout of another commit with its library built) that tree's `dctn_amd` package is imported
beside this one, under another name, and the two alternate block by block, so that clock drift falls on both alike.
Prints one JSON line: per source, operation and build the median, min, max and spread of the per-call time over the
blocks (us), and this build's median minus the other's.

    python tools/time_batch_draw_host.py [--steps 3000] [--repeats 7] [--other-tree PATH]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_flat_step_host import ROOT, package   # noqa: E402

N, SIZE, BATCH, SEED = 64, 8, 8, 1234
NU = (1.46, 0.83, 1.21)


def sources(pkg_name, dev):
    B = importlib.import_module(pkg_name + ".batches")
    g = torch.Generator().manual_seed(0)
    grey = torch.randint(0, 256, (N, SIZE, SIZE), dtype=torch.uint8, generator=g).to(dev)
    colour = torch.randint(0, 256, (N, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, 10, (N,), generator=g).to(dev)
    kw = dict(dtype=torch.float32, seed=SEED)
    return {"grey": B.DeviceBatches(grey, labels, BATCH, **kw),
            "colour": B.DeviceBatches.from_colour(colour, labels, BATCH, nu=NU, constant_channel=0.5, **kw),
            "colour augmented": B.DeviceBatches.from_colour(colour, labels, BATCH, nu=NU, constant_channel=0.5,
                                                            augment=B.Augment(2, True, (125, 123, 114)), **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--other-tree", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    builds = {"this": package(ROOT, "dctn_this")}
    if args.other_tree:
        builds["other"] = package(os.path.abspath(args.other_tree), "dctn_other")
    result = {"workload": f"eager draw_into / gather, {N} images of {SIZE} x {SIZE}, batch {BATCH}, float32",
              "steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev),
              "versions": {b: m._lib.lib().dctn_version() for b, m in builds.items()}, "cases": {}}
    made = {b: sources(m.__name__, dev) for b, m in builds.items()}
    picked = torch.arange(BATCH, dtype=torch.int64, device=dev)
    for name in next(iter(made.values())):
        for op in ("draw_into", "gather"):
            calls = {}
            for b in builds:
                src = made[b][name]
                if op == "draw_into":
                    calls[b] = (src.draw_into, src.empty_batch())
                else:
                    calls[b] = (src.gather, (picked,))
            times = {b: [] for b in calls}
            for fn, fn_args in calls.values():   # an untimed block each
                for _ in range(200):
                    fn(*fn_args)
            for _ in range(args.repeats):
                for b, (fn, fn_args) in calls.items():   # alternating
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        fn(*fn_args)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize(dev)
                    times[b].append((t1 - t0) * 1e6 / args.steps)
            case = {b: {"median_us": round(statistics.median(t), 3), "min_us": round(min(t), 3), "max_us": round(max(t), 3),
                        "spread_us": round(max(t) - min(t), 3)} for b, t in times.items()}
            if "other" in case:
                case["this_minus_other_us"] = round(case["this"]["median_us"] - case["other"]["median_us"], 3)
            result["cases"][f"{name} {op}"] = case
    print(json.dumps(result))


if __name__ == "__main__":
    main()
