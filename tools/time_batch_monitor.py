"""What the batch monitor costs a graphed training step, and what the launch costs alone, in one process.

Two workloads, every variant the whole `GraphedTrainStep` with the batch drawn inside the graph:

  classifier  three layers, B = 128, 28 x 28, float32, at each bond of `--bonds`: `DeviceBatches(phi=quantum_phi(False))`,
              forward, fused cross-entropy, backward, `FlatRMSprop(alpha=0.9, momentum=0.9, weight_decay=1e-4)`
  cfg2        `EPSesPlusLinear(((3, 4),))`, bf16, B = 1024, `FlatAdam(master_weights=True)`

  none       no monitor
  none2      a second instance of `none`: what two instances of one graph differ by in this process
  period1    `monitor=BatchMonitor(dev, B, 10, (1, 28, 28, 2), kernel_size=3, period=1)`: one `dctn_batch_monitor` launch
             more per step, every launch recorded
  period20   the same with `period=20`: nineteen launches of twenty read no element
  host_hook  what the monitor replaces: the step of `none`, replayed from a host loop that after every iteration reads
             the same quantities with torch - mean and std of the batch, min, max, mean and std of the logits (one
             `.item()` each), `softmax(logits, 1)` to the host for the histogram, and the gathered probabilities of the true
             classes with the indices (the reference's add_quantum_inputs_statistics_logging, log_logits_as_probabilities
             and --tb-batches; none of them can run inside a launch of several iterations at all).  The window statistic
             is left out of the hook: it stays cheaper than what it stands for

Each variant is timed over `--repeats` blocks of `--steps` replays with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Then the launch alone, as the
median over the blocks of one graph of `--chain` `record()` calls divided by `--chain`: over each workload's own batch
buffers, recorded and skipped.  Prints one JSON line.

    python tools/time_batch_monitor.py [--steps 2000] [--repeats 5] [--bonds 2,4] [--samples 4096] [--variants ...]
                                       [--chain 50] [--workloads classifier,cfg2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dctn_amd  # noqa: E402
from dctn_amd import _lib as L  # noqa: E402
from dctn_amd import batches as B  # noqa: E402
from dctn_amd import training as T  # noqa: E402
from dctn_amd.batch_monitor import BatchMonitor  # noqa: E402

SIZE = 28
ALL = ("none", "none2", "period1", "period20", "host_hook")


def build(workload, bond, images, labels, dev, monitor_period):
    """(graphed step, monitor or None) of one workload."""
    torch.manual_seed(0)
    if workload == "classifier":
        from dctn_amd import conv_sbs as C
        from dctn_amd import mnist_model as M

        batch = 128
        src = B.DeviceBatches(images, labels, batch, dtype=torch.float32, seed=2024, phi=M.quantum_phi(False), device=dev)
        x, _, _ = src.gather(torch.arange(batch, device=dev))
        model = M.DCTNMnistModel(3, bond, False, C.DumbNormalInitialization((2 * bond) ** -0.5 * 1.3), False, 1.0).to(dev)
        model.scale_layers_using_batch(x)
        opt = T.FlatRMSprop(list(model.parameters()), lr=1e-5, alpha=0.9, momentum=0.9, weight_decay=1e-4)
    else:
        from dctn_amd import eps_plus_linear as E

        batch = 1024
        src = B.DeviceBatches(images, labels, batch, dtype=torch.bfloat16, seed=2024)
        model = E.EPSesPlusLinear(((3, 4),), E.UnitTheoreticalOutputStd(), 1.0, dev, torch.bfloat16, image_size=SIZE)
        opt = T.FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4, master_weights=True)
    mon = BatchMonitor(dev, batch, 10, (1, SIZE, SIZE, 2), kernel_size=3, period=monitor_period, capacity=8) if monitor_period else None
    kw = {} if mon is None else {"monitor": mon}
    return T.GraphedTrainStep(model, None, None, T.fused_cross_entropy, opt, warmup=2, batch_source=src, **kw), mon


class Variant:
    def __init__(self, name, workload, bond, images, labels, dev):
        self.step, self.mon = build(workload, bond, images, labels, dev, {"period1": 1, "period20": 20}.get(name, 0))
        self.hook = name == "host_hook"
        self.seen = None

    def __call__(self):
        out = self.step()
        if self.hook:
            with torch.no_grad():
                x, z, y = self.step.x, out["output"].float(), self.step.y
                p = torch.softmax(z, dim=1)
                self.seen = (x.mean().item(), x.std().item(), z.min().item(), z.max().item(), z.mean().item(), z.std().item(),
                             p.cpu(), p.gather(1, y.unsqueeze(1)).squeeze(1).cpu(), out["indices"].cpu())


def time_launch(step, period, chain, repeats, dev):
    """us per `record()` over the static batch buffers of `step`, replayed from one graph of `chain` of them."""
    x, z, y, idx = step.x, step.out.detach(), step.y, step.indices
    mon = BatchMonitor(dev, x.shape[1], z.shape[1], (x.shape[0],) + tuple(x.shape[2:]), kernel_size=3, period=period, capacity=8)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        mon.record(x, z, y, idx)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            mon.record(x, z, y, idx)
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
    return {"median_us": statistics.median(blocks), "min_us": min(blocks), "max_us": max(blocks), "batch": int(x.shape[1]),
            "x_dtype": str(x.dtype), "logits_dtype": str(z.dtype), "block_bytes": mon.block_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bonds", default="2,4")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--workloads", default="classifier,cfg2")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = [v for v in args.variants.split(",") if v]
    assert all(v in ALL for v in names)
    result = {"steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "version": L.lib().dctn_version(),
              "package": os.path.dirname(dctn_amd.__file__), "workload": {}, "launch_alone": {}}
    cases = []
    for w in [w for w in args.workloads.split(",") if w]:
        cases += [("classifier", int(b)) for b in args.bonds.split(",")] if w == "classifier" else [("cfg2", 0)]
    for workload, bond in cases:
        label = f"classifier float32 B=128 bond {bond} FlatRMSprop" if workload == "classifier" else \
            "cfg2 bf16 B=1024 FlatAdam(master)"
        runs = {v: Variant(v, workload, bond, images, labels, dev) for v in names}
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
                print(f"{label} repeat {r} {v}: {times[v][-1]:.2f} us", file=sys.stderr, flush=True)
        entry = {"variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                                  "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t]}
                              for v, t in times.items()}}
        med = {v: entry["variants"][v]["median_us"] for v in names}
        for v in names:
            if v != "none" and "none" in med:
                entry[f"{v}_minus_none_us"] = med[v] - med["none"]
        for v in ("period1", "period20"):   # what the device says it did
            if v in runs:
                raw = runs[v].mon.raw()
                entry[f"{v}_calls_recorded"] = [int(raw["calls"]), int(raw["recorded"])]
        if runs:
            step = next(iter(runs.values())).step
            result["launch_alone"][label + ", recorded"] = time_launch(step, 1, args.chain, args.repeats, dev)
            result["launch_alone"][label + ", skipped"] = time_launch(step, 1 << 30, args.chain, args.repeats, dev)
        result["workload"][label] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
