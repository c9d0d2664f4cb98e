"""What the TT-tensor statistics cost a graphed training step, and what the launch costs alone, in one process.

Three layers, B = 128, 28 x 28, float32, at each bond of `--bonds`; every variant is the whole `GraphedTrainStep`: batch
drawn from a `DeviceBatches(phi=quantum_phi(False))`, forward, fused cross-entropy, backward,
`FlatRMSprop(alpha=0.9, momentum=0.9, weight_decay=1e-4)`:

  none       no monitor (the parent's step)
  period1    `model.tt_stats = TTStats.for_model(model, period=1)`: one `dctn_tt_stats` launch more per forward, every
             launch recorded
  period20   the same with `period=20`: nineteen launches of twenty read no core
  host_hook  what the monitor replaces: the step of `none`, replayed from a host loop that every 20 iterations calls
             `string.mean().item()` and `(string.var() ** 0.5).item()` on the five strings (the reference's
             add_conv_sbs_tt_tensor_statistics_logging; it cannot run inside a launch of several iterations at all)

Each variant is timed over `--repeats` blocks of `--steps` replays with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Then the launch alone, as the
median over the blocks of one graph of `--chain` `record()` calls divided by `--chain`: the five strings of the model
at bonds 4 and 16, recorded and skipped, and one ring of three cores at bond 32.  Prints one JSON line.

    python tools/time_tt_stats.py [--steps 2000] [--repeats 5] [--bonds 2,4] [--samples 4096] [--variants ...] [--chain 50]
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
from dctn_amd.conv_sbs import ConvSBS, DumbNormalInitialization  # noqa: E402
from dctn_amd.conv_sbs_spec import SBSSpecCore, SBSSpecString  # noqa: E402
from dctn_amd.mnist_model import DCTNMnistModel, quantum_phi  # noqa: E402
from dctn_amd.pos2d import Pos2D  # noqa: E402
from dctn_amd.tt_stats import TTStats  # noqa: E402

BATCH, SIZE = 128, 28
ALL = ("none", "period1", "period20", "host_hook")
HOOK_EVERY = 20


def make_model(bond, dev):
    torch.manual_seed(0)
    return DCTNMnistModel(3, bond, False, DumbNormalInitialization((2 * bond) ** -0.5 * 1.3), False, 1.0).to(dev)


class Variant:
    def __init__(self, name, bond, images, labels, dev):
        src = batches.DeviceBatches(images, labels, BATCH, dtype=torch.float32, seed=2024, phi=quantum_phi(False), device=dev)
        x, _, _ = src.gather(torch.arange(BATCH, device=dev))
        self.model = model = make_model(bond, dev)
        model.scale_layers_using_batch(x)
        opt = training.FlatRMSprop(list(model.parameters()), lr=1e-5, alpha=0.9, momentum=0.9, weight_decay=1e-4)
        if name in ("period1", "period20"):   # behind the optimizer: the parameters now live in its flat buffer
            model.tt_stats = TTStats.for_model(model, period=1 if name == "period1" else 20, capacity=8)
        self.step = training.GraphedTrainStep(model, None, None, training.fused_cross_entropy, opt, warmup=2, batch_source=src)
        self.hook = name == "host_hook"
        self.strings = [m for m in model.modules() if isinstance(m, ConvSBS)]
        self.done, self.seen = 0, []

    def __call__(self):
        if self.hook and self.done % HOOK_EVERY == 0:
            with torch.no_grad():
                self.seen = [(s.mean().item(), (s.var() ** 0.5).item()) for s in self.strings]
        self.done += 1
        self.step()


def time_launch(tt, chain, repeats, dev):
    """us per `record()` of `tt`, replayed from one graph of `chain` of them."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        tt.record()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            tt.record()
    for _ in range(3):
        graph.replay()
    blocks = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            graph.replay()
        torch.cuda.synchronize(dev)
        blocks.append((time.perf_counter() - t0) * 1e6 / (20 * chain))
    return {"median_us": statistics.median(blocks), "min_us": min(blocks), "max_us": max(blocks)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bonds", default="2,4")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--chain", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = [v for v in args.variants.split(",") if v]
    assert all(v in ALL for v in names)
    result = {"workload": f"ConvSBS classifier, three layers, float32, B={BATCH}, {SIZE}x{SIZE}, graphed step, FlatRMSprop",
              "steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "version": L.lib().dctn_version(),
              "bond": {}, "launch_alone": {}}
    for bond in [int(b) for b in args.bonds.split(",")] if names else []:
        runs = {v: Variant(v, bond, images, labels, dev) for v in names}
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
        if "host_hook" in med and "none" in med:
            entry["host_hook_us_per_hook"] = (med["host_hook"] - med["none"]) * HOOK_EVERY
        for v in ("period1", "period20"):   # what the device says it did
            if v in runs:
                raw = runs[v].model.tt_stats.raw()
                entry[f"{v}_calls_recorded"] = [int(raw["calls"]), int(raw["recorded"])]
        result["bond"][str(bond)] = entry
        del runs
    for bond in (4, 16):
        model = make_model(bond, dev)
        result["launch_alone"][f"five strings, bond {bond}, recorded"] = time_launch(TTStats.for_model(model, period=1), args.chain,
                                                                                   args.repeats, dev)
        result["launch_alone"][f"five strings, bond {bond}, skipped"] = time_launch(TTStats.for_model(model, period=1 << 30),
                                                                                  args.chain, args.repeats, dev)
    spec = SBSSpecString(tuple(SBSSpecCore(Pos2D(0, i), 1) for i in range(3)), (32, 32, 32), 1, 2)
    ring = ConvSBS(spec, DumbNormalInitialization(0.1)).to(dev)
    result["launch_alone"]["one ring of three cores, bond 32, recorded"] = time_launch(TTStats(dev, [ring]), 4, args.repeats, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
