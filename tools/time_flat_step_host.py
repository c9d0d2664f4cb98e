"""What one eager `opt.step()` costs the HOST - Python marshalling plus the C dispatch - in this build and in another tree.

cfg2's parameters (bf16) in a FlatAdam and a FlatSGD, each in two configurations: plain, and guard + schedule + groups.
The gradients sit back to back in one buffer, so `step()` reads them in place and launches one kernel (two with a guard).
A block is `--steps` calls timed on the host clock with the device synchronised before the block and after the clock
stops: the launches queue up behind one another and the host never waits for one.  With `--other-tree PATH` (a checkout of
another commit with its library built) that tree's `dctn_amd` package is imported beside this one, under another name,
and the two alternate block by block, so that clock drift falls on both alike.  Prints one JSON line: per optimizer,
configuration and build the median, min, max and spread of the per-call time over the blocks (us), and this build's
median minus the other's.

    python tools/time_flat_step_host.py [--steps 3000] [--repeats 7] [--other-tree PATH]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC, SIZE, DTYPE = ((3, 4),), 28, torch.bfloat16
KNOTS = [(0, 1e-5), (1000, 1e-4), (1 << 30, 1e-5)]


def package(tree, name):
    """`dctn_amd` of the tree, imported as `name` (its relative imports and its library stay inside the tree)."""
    path = os.path.join(tree, "dctn_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def optimizer(pkg_name, kind, full, dev):
    import importlib

    T = importlib.import_module(pkg_name + ".training")
    model_mod = importlib.import_module(pkg_name + ".eps_plus_linear")
    torch.manual_seed(0)
    model = model_mod.EPSesPlusLinear(SPEC, model_mod.UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    reg, others = list(model.epses) + [model.linear.weight], [model.linear.bias]
    kw = {}
    if full:
        kw = dict(guard=T.GradGuard(dev, max_norm=1.0), schedule=T.LRSchedule(dev, KNOTS),
                  groups=T.ParamGroups(reg + others, [T.ParamGroup(model.linear.weight, lr_scale=0.1)]))
    if kind == "adam":
        opt = T.FlatAdam(reg, others, lr=1e-4, l2=1e-4, **kw)
    else:
        opt = T.FlatSGD(reg, others, lr=1e-4, momentum=0.9, l2=1e-4, **kw)
    store = torch.zeros(opt.n, dtype=DTYPE, device=dev)
    off = 0
    for p in opt.params:
        p.grad = store[off: off + p.numel()].view_as(p)
        off += p.numel()
    return opt


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
    result = {"workload": "eager opt.step(), cfg2 parameters bf16, gradients read in place", "steps": args.steps,
              "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev),
              "versions": {b: m._lib.lib().dctn_version() for b, m in builds.items()}, "cases": {}}
    for kind in ("adam", "sgd"):
        for full in (False, True):
            opts = {b: optimizer(m.__name__, kind, full, dev) for b, m in builds.items()}
            result["n"] = next(iter(opts.values())).n
            times = {b: [] for b in opts}
            for opt in opts.values():   # an untimed block each
                for _ in range(200):
                    opt.step()
            for _ in range(args.repeats):
                for b, opt in opts.items():   # alternating
                    step = opt.step
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize(dev)
                    times[b].append((t1 - t0) * 1e6 / args.steps)
            case = {b: {"median_us": round(statistics.median(t), 3), "min_us": round(min(t), 3), "max_us": round(max(t), 3),
                        "spread_us": round(max(t) - min(t), 3)} for b, t in times.items()}
            if "other" in case:
                case["this_minus_other_us"] = round(case["this"]["median_us"] - case["other"]["median_us"], 3)
            result["cases"][f"{kind} {'guard+schedule+groups' if full else 'plain'}"] = case
    print(json.dumps(result))


if __name__ == "__main__":
    main()
