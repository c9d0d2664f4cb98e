"""The augmented draw against the unaugmented draw of the same library, alone and inside the graphed training iteration,
in one process.

Two workloads, each over synthetic bytes:

  cfg2        EPSesPlusLinear(((3, 4),), image_size = 28), bf16, B = 1024, FlatAdam with master weights; 28 x 28 grey
              images; `Augment(max_shift=2)`
  cfg4_eps36  EPSesPlusLinear(((3, 6),), Q_0 = 4, image_size = 32), float32, B = 128, FlatAdam; 32 x 32 x 3 colour images
              with a constant channel and per-channel moments; `Augment(max_shift=4, hflip=True, fill=round(255 mean))`

and for each of them four variants:

  draw_plain / draw_aug   the draw alone: a captured graph of `--chain` consecutive `draw_into` launches, replayed; the time
                          is per launch.  The unaugmented launch is the kernel the library had before the augmentation
                          existed, unchanged: the baseline.
  step_plain / step_aug   `GraphedTrainStep(batch_source=src)`: the draw as the first node of the iteration's graph

Every timed block ends in a device synchronise and runs under a time limit of its own (`--limit` seconds, SIGALRM with its
default action: a block that hangs ends the process).  The variants alternate block by block, so that clock and thermal
drift fall on all alike.  Prints one JSON line: per variant the median, min, max and spread (max - min) of the time per
launch or per iteration over the blocks (us), and aug - plain with the larger of the two spreads beside it.  There is no
threshold.

    python tools/time_augment.py [--repeats 5] [--draws 200] [--chain 20] [--steps 1000] [--samples 20000] [--only cfg2]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.batches import Augment, DeviceBatches, channel_moments  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, fused_cross_entropy  # noqa: E402

NU, CONSTANT = (1.2, 1.1, 1.3), 1.0


def limited(seconds, fn):
    """One GPU step under its own time limit."""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(seconds)
    try:
        return fn()
    finally:
        signal.alarm(0)


class Cfg2:
    name, batch, dtype = "cfg2 bf16 B=1024 28x28 grey, max_shift=2", 1024, torch.bfloat16

    def __init__(self, samples):
        g = torch.Generator().manual_seed(1)
        self.images = torch.randint(0, 256, (samples, 28, 28), dtype=torch.uint8, generator=g)
        self.labels = torch.randint(0, 10, (samples,), generator=g)
        self.augment = Augment(max_shift=2)

    def source(self, dev, augment):
        return DeviceBatches(self.images.to(dev), self.labels.to(dev), self.batch, dtype=self.dtype, seed=2024,
                             augment=augment)

    def model(self, dev):
        torch.manual_seed(0)
        model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, dev, self.dtype, image_size=28)
        return model, FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4,
                               master_weights=True)


class Cfg4Eps36:
    name, batch, dtype = "cfg4_eps36 f32 B=128 32x32x3 + constant channel, max_shift=4, hflip", 128, torch.float32

    def __init__(self, samples):
        g = torch.Generator().manual_seed(2)
        self.images = torch.randint(0, 256, (samples, 32, 32, 3), dtype=torch.uint8, generator=g)
        self.labels = torch.randint(0, 10, (samples,), generator=g)
        self.mean, self.std = channel_moments(self.images)
        self.augment = Augment(max_shift=4, hflip=True, fill=tuple(int(round(255 * float(v))) for v in self.mean))

    def source(self, dev, augment):
        return DeviceBatches.from_colour(self.images.to(dev), self.labels.to(dev), self.batch, dtype=self.dtype, seed=2024,
                                         nu=NU, mean=self.mean, std=self.std, constant_channel=CONSTANT, augment=augment)

    def model(self, dev):
        torch.manual_seed(0)
        model = EPSesPlusLinear(((3, 6),), UnitTheoreticalOutputStd(), 1.0, dev, self.dtype, image_size=32, Q_0=4)
        return model, FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4)


def chained_draws(src, chain, dev):
    """A graph of `chain` consecutive draws into one set of buffers; returns (replay, what must stay alive)."""
    out = src.empty_batch()
    src.draw_into(*out)   # loads the code object before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            src.draw_into(*out)
    return graph.replay, (graph, out, src)


def measure(cfg, args, dev):
    runs = {}   # variant -> (callable, units of work per call, calls per block, alive)
    for tag, augment in (("plain", None), ("aug", cfg.augment)):
        replay, alive = limited(args.limit, lambda: chained_draws(cfg.source(dev, augment), args.chain, dev))
        runs[f"draw_{tag}"] = (replay, args.chain, args.draws, alive)

        def build_step(augment=augment):
            model, opt = cfg.model(dev)
            src = cfg.source(dev, augment)
            return GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=2, batch_source=src), src

        step, src = limited(args.limit, build_step)
        runs[f"step_{tag}"] = (step, 1, args.steps, src)
    times = {v: [] for v in runs}

    def block(v):
        run, units, calls, _ = runs[v]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            run()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e6 / (calls * units)

    for v in runs:   # one untimed block each: clocks, allocator and caches settle before the first timed one
        limited(args.limit, lambda: block(v))
    for r in range(args.repeats):
        for v in runs:   # alternating
            times[v].append(limited(args.limit, lambda: block(v)))
            print(f"{cfg.name}: repeat {r} {v}: {times[v][-1]:.2f} us", file=sys.stderr, flush=True)
    out = {"workload": cfg.name,
           "variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t),
                            "blocks_us": [round(b, 2) for b in t]} for v, t in times.items()}}
    for kind in ("draw", "step"):
        a, p = out["variants"][f"{kind}_aug"], out["variants"][f"{kind}_plain"]
        out[f"{kind}_aug_minus_plain_us"] = a["median_us"] - p["median_us"]
        out[f"{kind}_aug_over_plain"] = a["median_us"] / p["median_us"]
        out[f"{kind}_largest_spread_us"] = max(a["spread_us"], p["spread_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--draws", type=int, default=200, help="graph replays per timed block of a draw variant")
    ap.add_argument("--chain", type=int, default=20, help="draws per graph")
    ap.add_argument("--steps", type=int, default=1000, help="iterations per timed block of a step variant")
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--limit", type=int, default=120, help="seconds one GPU step may take")
    ap.add_argument("--only", default="", help="cfg2 or cfg4_eps36")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_augment.py measures on an MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    cfgs = [c for c in (Cfg2, Cfg4Eps36) if not args.only or c.__name__.lower() == args.only.replace("_", "").lower()]
    result = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev), "repeats": args.repeats,
              "draws": args.draws, "chain": args.chain, "steps": args.steps, "samples": args.samples,
              "results": [measure(c(args.samples), args, dev) for c in cfgs]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
