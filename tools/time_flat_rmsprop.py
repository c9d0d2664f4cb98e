"""What a graphed training iteration costs under each flat optimizer, in one process.

cfg2 (bf16, B = 1024, master weights) as a GraphedTrainStep whose graph draws its own batches from a `DeviceBatches`
source over `--samples` synthetic 28 x 28 uint8 images, with K = 1 and K = 20 iterations per launch:

  rms0     `FlatRMSprop(momentum=0)`: no momentum buffer
  rms9     `FlatRMSprop(momentum=0.9)`
  adam     `FlatAdam`
  sgd      `FlatSGD(momentum=0.9)`, no weight decay: the kernels the parent has
  sgd_wd   `FlatSGD(momentum=0.9, weight_decay=1e-4)`: the DECAY kernels
  torch    `torch.optim.RMSprop(momentum=0.9, capturable=True)` on the bf16 parameters, if this torch captures it (left out
           with a note otherwise)
  p_<name> for each of the five, with `--parent-lib PATH` (a libdctn_amd.so built from the parent commit, in the dctn_amd
           directory of a checkout of that commit): that tree's Python over that library's optimizer, imported beside this
           build under another name.  <name> - p_<name> is judged against the two variants' own block spreads in the run.

Each variant is timed over `--repeats` blocks of `--steps` iterations with device synchronisation around each block; the
variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON line: per K and
variant the median, min and max of the per-iteration time over the blocks (us), their spread, and the differences named
above.

    python tools/time_flat_rmsprop.py [--steps 4000] [--repeats 5] [--samples 50000] [--variants ...] [--iters 1,20]
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
from dctn_amd import batches, eps_plus_linear, training  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024
LR, L2, WD = 1e-4, 1e-4, 1e-4
OURS = ("rms0", "rms9", "adam", "sgd", "sgd_wd")
ALL = OURS + ("torch",) + tuple(f"p_{v}" for v in OURS)


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


def make_variant(name, K, images, labels, dev):
    """Returns a callable that runs one launch (K iterations)."""
    parents = name.startswith("p_")
    name = name[2:] if parents else name
    if parents:   # the parent's classes: construction, warm-up and capture go through its library
        T, M = importlib.import_module("dctn_parent.training"), importlib.import_module("dctn_parent.eps_plus_linear")
        B = importlib.import_module("dctn_parent.batches")
    else:
        T, M, B = training, eps_plus_linear, batches
    torch.manual_seed(0)
    model = M.EPSesPlusLinear(SPEC, M.UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    reg, others = list(model.epses) + [model.linear.weight], [model.linear.bias]
    common = dict(lr=LR, l2=L2, master_weights=True)
    reg_fn, reg_coeff = None, 0.0
    if name in ("rms0", "rms9"):
        opt = T.FlatRMSprop(reg, others, momentum=0.0 if name == "rms0" else 0.9, weight_decay=WD, **common)
    elif name == "adam":
        opt = T.FlatAdam(reg, others, weight_decay=WD, **common)
    elif name == "sgd":
        opt = T.FlatSGD(reg, others, momentum=0.9, **common)
    elif name == "sgd_wd":
        opt = T.FlatSGD(reg, others, momentum=0.9, weight_decay=WD, **common)
    else:   # torch's own: no flat buffer, no master copy, the regulariser through autograd
        opt = torch.optim.RMSprop(model.parameters(), lr=LR, momentum=0.9, weight_decay=WD, capturable=True)
        reg_fn, reg_coeff = (lambda m: m.epswise_l2_regularizer()), L2
    src = B.DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
    return T.GraphedTrainStep(model, None, None, T.fused_cross_entropy, opt, reg_fn=reg_fn, reg_coeff=reg_coeff, warmup=2,
                              batch_source=src, iters_per_launch=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--variants", default=None)
    ap.add_argument("--iters", default="1,20")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    parent = parent_package(args.parent_lib) if args.parent_lib else None
    names = args.variants.split(",") if args.variants else [v for v in ALL if parent is not None or not v.startswith("p_")]
    assert all(v in ALL for v in names) and (parent is not None or not any(v.startswith("p_") for v in names))
    result = {"workload": "cfg2 bf16 B=1024 master weights, graphed, batch source", "samples": args.samples,
              "steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "parent_lib": args.parent_lib,
              "parent_version": None if parent is None else parent._lib.lib().dctn_version(),
              "version": L.lib().dctn_version(), "left_out": {}, "K": {}}
    for K in [int(k) for k in args.iters.split(",")]:
        launches = max(args.steps // K, 1)
        runs = {}
        for v in [n for n in names if n != "torch"] + [n for n in names if n == "torch"]:   # torch's capture is tried last
            if v in result["left_out"]:
                continue
            try:
                runs[v] = make_variant(v, K, images, labels, dev)
            except Exception as e:   # only torch's own optimizer may fail to capture; ours must not
                if v != "torch":
                    raise
                result["left_out"][v] = f"{type(e).__name__}: {str(e).splitlines()[0][:200]}"
                print(f"torch.optim.RMSprop(capturable=True) was not captured: {result['left_out'][v]}", file=sys.stderr)
        order = [v for v in names if v in runs]
        times = {v: [] for v in order}
        for v in order:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
            for _ in range(min(launches, max(200 // K, 1))):
                runs[v]()
        for r in range(args.repeats):
            for v in order:   # alternating
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
        med = {v: entry["variants"][v]["median_us"] for v in order}
        for hi, lo in tuple((v, f"p_{v}") for v in OURS) + (("sgd_wd", "sgd"), ("rms0", "adam"), ("rms9", "adam"),
                       ("rms9", "rms0"), ("torch", "rms9")):
            if hi in med and lo in med:
                entry[f"{hi}_minus_{lo}_us"] = med[hi] - med[lo]
        result["K"][str(K)] = entry
        del runs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
