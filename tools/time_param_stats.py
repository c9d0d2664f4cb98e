"""What the parameter monitor costs a graphed training step, and what the launch costs alone, in one process.

Two workloads, every variant the whole `GraphedTrainStep` with the batch drawn inside the graph:

  classifier  three layers, B = 128, 28 x 28, float32, at each bond of `--bonds`: `DeviceBatches(phi=quantum_phi(False))`,
              forward, fused cross-entropy, backward, `FlatRMSprop(alpha=0.9, momentum=0.9, weight_decay=1e-4)`; 45 parameters
  cfg2        `EPSesPlusLinear(((3, 4),))`, bf16, B = 1024, `FlatAdam(master_weights=True)`; 3 parameters

  parent     with `--parent-lib PATH` (a libdctn_amd.so built from the parent commit, in the dctn_amd directory of a
             checkout of that commit): that tree's Python over that library's kernels, imported beside this build under
             another name.  `none` against it must sit inside the run's block spread: the same machine code
  none       no monitor
  none2      a second instance of `none`: what two instances of one graph differ by in this process
  period1    `param_stats=ParamStats.for_parameters(model, params, period=1)`: one `dctn_param_stats` launch more per
             step, every launch recorded
  period20   the same with `period=20`: nineteen launches of twenty read no element
  host_hook  what the monitor replaces: the step of `none`, replayed from a host loop that after every iteration calls
             `torch.norm(p).item()` and `torch.norm(p.grad).item()` per parameter (the reference's
             add_weights_and_grads_logging; it cannot run inside a launch of several iterations at all)

Each variant is timed over `--repeats` blocks of `--steps` replays with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Then the launch alone, as the
median over the blocks of one graph of `--chain` `record()` calls divided by `--chain`: over each workload's own flat
buffers, recorded and skipped.  Prints one JSON line.

    python tools/time_param_stats.py [--steps 2000] [--repeats 5] [--bonds 2,4] [--samples 4096] [--variants ...]
                                     [--chain 50] [--workloads classifier,cfg2] [--parent-lib PATH]
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

import dctn_amd  # noqa: E402
from dctn_amd import _lib as L  # noqa: E402
from dctn_amd.param_stats import ParamStats  # noqa: E402

SIZE = 28
ALL = ("parent", "none", "none2", "period1", "period20", "host_hook")


def parent_package(lib_path):
    """The `dctn_amd` package that holds the parent's library, imported as `dctn_parent`: its own Python over its own
    library."""
    path = os.path.dirname(os.path.abspath(lib_path))
    spec = importlib.util.spec_from_file_location("dctn_parent", os.path.join(path, "__init__.py"),
                                                  submodule_search_locations=[path])
    module = importlib.util.module_from_spec(spec)
    sys.modules["dctn_parent"] = module
    spec.loader.exec_module(module)
    assert os.path.samefile(module._lib.LIB_PATH, lib_path)
    return module


def build(workload, bond, package, images, labels, dev, monitor_period):
    """(model, optimizer, graphed step) of one workload from the modules of `package` ("dctn_amd" or "dctn_parent")."""
    T, B = importlib.import_module(package + ".training"), importlib.import_module(package + ".batches")
    torch.manual_seed(0)
    if workload == "classifier":
        M, C = importlib.import_module(package + ".mnist_model"), importlib.import_module(package + ".conv_sbs")
        src = B.DeviceBatches(images, labels, 128, dtype=torch.float32, seed=2024, phi=M.quantum_phi(False), device=dev)
        x, _, _ = src.gather(torch.arange(128, device=dev))
        model = M.DCTNMnistModel(3, bond, False, C.DumbNormalInitialization((2 * bond) ** -0.5 * 1.3), False, 1.0).to(dev)
        model.scale_layers_using_batch(x)
        regularised, others = list(model.parameters()), []
        make = lambda **kw: T.FlatRMSprop(regularised, lr=1e-5, alpha=0.9, momentum=0.9, weight_decay=1e-4, **kw)  # noqa: E731
    else:
        E = importlib.import_module(package + ".eps_plus_linear")
        src = B.DeviceBatches(images, labels, 1024, dtype=torch.bfloat16, seed=2024)
        model = E.EPSesPlusLinear(((3, 4),), E.UnitTheoreticalOutputStd(), 1.0, dev, torch.bfloat16, image_size=SIZE)
        regularised, others = list(model.epses) + [model.linear.weight], [model.linear.bias]
        make = lambda **kw: T.FlatAdam(regularised, others, lr=1e-4, l2=1e-4, master_weights=True, **kw)  # noqa: E731
    kw = {}
    if monitor_period:
        kw["param_stats"] = ParamStats.for_parameters(model, regularised + others, period=monitor_period, capacity=8)
    opt = make(**kw)
    return model, opt, T.GraphedTrainStep(model, None, None, T.fused_cross_entropy, opt, warmup=2, batch_source=src)


class Variant:
    def __init__(self, name, workload, bond, images, labels, dev):
        period = {"period1": 1, "period20": 20}.get(name, 0)
        self.model, self.opt, self.step = build(workload, bond, "dctn_parent" if name == "parent" else "dctn_amd", images,
                                                labels, dev, period)
        self.hook = name == "host_hook"
        self.seen = []

    def __call__(self):
        self.step()
        if self.hook:
            with torch.no_grad():
                self.seen = [(torch.norm(p).item(), 0.0 if p.grad is None else torch.norm(p.grad).item())
                             for p in self.opt.params]


def time_launch(opt, period, chain, repeats, dev):
    """us per `record()` over the flat buffers of `opt`, replayed from one graph of `chain` of them."""
    ps = ParamStats(dev, [str(i) for i in range(len(opt.params))], period=period, capacity=8)
    ps.bind([p.numel() for p in opt.params])
    grads = torch.zeros_like(opt.flat)
    args = (opt.flat, opt.master, grads)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ps.record(*args)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            ps.record(*args)
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
    return {"median_us": statistics.median(blocks), "min_us": min(blocks), "max_us": max(blocks),
            "segments": len(opt.params), "elements": int(opt.n), "workspace_bytes": ps.workspace_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bonds", default="2,4")
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--variants", default=",".join(ALL))
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--workloads", default="classifier,cfg2")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    parent = parent_package(args.parent_lib) if args.parent_lib else None
    names = [v for v in args.variants.split(",") if v and (v != "parent" or parent is not None)]
    assert all(v in ALL for v in names)
    result = {"steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "version": L.lib().dctn_version(),
              "parent_lib": args.parent_lib, "parent_version": None if parent is None else parent._lib.lib().dctn_version(),
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
            if v != "parent" and v != "none" and "none" in med:
                entry[f"{v}_minus_none_us"] = med[v] - med["none"]
        if "parent" in med and "none" in med:
            entry["none_minus_parent_us"] = med["none"] - med["parent"]
            entry["parent_spread_us"] = entry["variants"]["parent"]["spread_us"]
        for v in ("period1", "period20"):   # what the device says it did
            if v in runs:
                raw = runs[v].opt.param_stats.raw()
                entry[f"{v}_calls_recorded"] = [int(raw["calls"]), int(raw["recorded"])]
        if runs:
            opt = next(iter(runs.values())).opt
            result["launch_alone"][label + ", recorded"] = time_launch(opt, 1, args.chain, args.repeats, dev)
            result["launch_alone"][label + ", skipped"] = time_launch(opt, 1 << 30, args.chain, args.repeats, dev)
        result["workload"][label] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
