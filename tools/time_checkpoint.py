"""What saving costs a graphed training iteration, three ways, in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) as a GraphedTrainStep whose graph draws its own batches from a
`DeviceBatches` source over `--samples` synthetic 28 x 28 uint8 images:

  N   no saving
  M   `LastModelsCheckpointer`-style: a blocking `torch.save(model.state_dict())` every `--every` iterations, the newest
      two files kept (the model alone: it saves LESS than R)
  R   `checkpoint.RunCheckpointer` every `--every` iterations: the whole run (parameters, moments, master copy, step
      block, dropout and source counters), gathered by one launch, copied on a side stream, the previous snapshot's file
      written while the stream goes on

Each variant is timed over `--repeats` blocks of `--steps` iterations with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per variant the
median, min and max of the per-iteration time over the blocks (us) and their spread, M - N and R - N.  There is no
threshold: M and R save different things, the comparison is informative only.

    python tools/time_checkpoint.py [--steps 10000] [--repeats 5] [--samples 50000] [--every 100] [--variants N,M,R]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from collections import deque

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd import checkpoint  # noqa: E402
from dctn_amd.batches import DeviceBatches  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, fused_cross_entropy  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024


def make_variant(name, images, labels, dev, every, directory):
    """Returns (callable that runs one iteration, callable that finishes pending writes)."""
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4, master_weights=True)
    src = DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src)
    count = [0]
    if name == "N":
        return step, lambda: None
    if name == "M":
        names = deque()

        def run():
            step()
            count[0] += 1
            if count[0] % every == 0:
                path = os.path.join(directory, f"model_nitd={count[0]:07}.pth")
                torch.save(model.state_dict(), path)
                names.appendleft(path)
                while len(names) > 2:
                    os.remove(names.pop())

        return run, lambda: None
    if name == "R":
        saver = checkpoint.RunCheckpointer(directory, checkpoint.RunState(model, opt, batch_source=src), 2)

        def run():
            step()
            count[0] += 1
            if count[0] % every == 0:
                saver({}, {"num_iters_done": count[0]})

        return run, saver.flush
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--variants", default="N,M,R")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    with tempfile.TemporaryDirectory(prefix="dctn_time_checkpoint_") as directory:
        runs = {}
        for v in names:
            os.mkdir(os.path.join(directory, v))
            runs[v] = make_variant(v, images, labels, dev, args.every, os.path.join(directory, v))
        times = {v: [] for v in names}
        for v in names:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
            for _ in range(min(args.steps, 200)):
                runs[v][0]()
            runs[v][1]()
        for r in range(args.repeats):
            for v in names:   # alternating
                run, finish = runs[v]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run()
                finish()   # the last file belongs to the block that asked for it
                torch.cuda.synchronize(dev)
                times[v].append((time.perf_counter() - t0) * 1e6 / args.steps)
                print(f"repeat {r} {v}: {times[v][-1]:.2f} us/step", file=sys.stderr, flush=True)
        sizes = {v: sorted(os.path.getsize(os.path.join(directory, v, f)) for f in os.listdir(os.path.join(directory, v)))
                 for v in names}
    result = {"workload": "cfg2 bf16 B=1024 FlatAdam(master) graphed, batch source", "samples": args.samples,
              "steps": args.steps, "repeats": args.repeats, "every": args.every, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "file_bytes": {v: s[-1] if s else 0 for v, s in sizes.items()},
              "variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                               "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                           for v, t in times.items()}}
    med = {v: result["variants"][v]["median_us"] for v in names}
    result["largest_spread_us"] = max(result["variants"][v]["spread_us"] for v in names)
    if "M" in med and "N" in med:
        result["M_minus_N_us"] = med["M"] - med["N"]
    if "R" in med and "N" in med:
        result["R_minus_N_us"] = med["R"] - med["N"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
