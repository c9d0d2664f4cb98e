"""What an eager ``opt.step()`` call costs the host under each flat optimizer.

A captured step is replayed by the runtime, so the Python of ``step()`` shows only on the eager path.  cfg2's parameters
(bf16, master weights, n = 29 098, the gradients back to back so that they are read in place) under the five variants of
tools/time_flat_rmsprop.py - rms0, rms9, adam, sgd, sgd_wd - alternated block by block: the host wall time of ``--calls``
calls of ``step()``, the device idle and synchronised outside the loop, over ``--blocks`` blocks.  Prints one JSON line: per
variant the median of the per-call time over the blocks (us), their spread and the blocks.

``--parent-training PATH``: measure the classes of another commit's ``dctn_amd/training.py`` instead (the file alone, over
this tree's library - for a change that touches no kernel), loaded beside this package under another name.  One process
measures one side; compare separate fresh processes of one visit, their order alternated (parent this this parent ...):
the time of a process drifts by more than the sides differ.

    python tools/time_eager_step.py [--blocks 7] [--calls 3000] [--parent-training PATH] [--out FILE]
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
sys.path.insert(0, ROOT)

from dctn_amd import eps_plus_linear as M  # noqa: E402

SPEC, SIZE, DTYPE = ((3, 4),), 28, torch.bfloat16
LR, L2, WD = 1e-4, 1e-4, 1e-4
VARIANTS = ("rms0", "rms9", "adam", "sgd", "sgd_wd")


def training_module(path):
    if path is None:
        from dctn_amd import training
        return training
    spec = importlib.util.spec_from_file_location("dctn_amd.training_parent", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["dctn_amd.training_parent"] = mod
    spec.loader.exec_module(mod)
    assert mod.FlatAdam.__module__ == "dctn_amd.training_parent"   # its own classes, not a re-export of this tree's
    return mod


def make(T, name, dev):
    torch.manual_seed(0)
    model = M.EPSesPlusLinear(SPEC, M.UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    reg, others = list(model.epses) + [model.linear.weight], [model.linear.bias]
    common = dict(lr=LR, l2=L2, master_weights=True)
    if name in ("rms0", "rms9"):
        opt = T.FlatRMSprop(reg, others, momentum=0.0 if name == "rms0" else 0.9, weight_decay=WD, **common)
    elif name == "adam":
        opt = T.FlatAdam(reg, others, weight_decay=WD, **common)
    elif name == "sgd":
        opt = T.FlatSGD(reg, others, momentum=0.9, **common)
    else:
        opt = T.FlatSGD(reg, others, momentum=0.9, weight_decay=WD, **common)
    store = (torch.randn(opt.n, device=dev) * 1e-3).to(DTYPE)   # the gradients back to back: read in place
    off = 0
    for p in opt.params:
        p.grad = store[off: off + p.numel()].view_as(p)
        off += p.numel()
    return opt, model, store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-training", default=None)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    T = training_module(a.parent_training)
    opts = {v: make(T, v, dev) for v in VARIANTS}
    for v in VARIANTS:   # untimed: kernel attributes, allocator, clocks
        for _ in range(300):
            opts[v][0].step()
    torch.cuda.synchronize(dev)
    times = {v: [] for v in VARIANTS}
    for _ in range(a.blocks):
        for v in VARIANTS:   # alternating
            step = opts[v][0].step
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.calls):
                step()
            t1 = time.perf_counter()
            torch.cuda.synchronize(dev)
            times[v].append((t1 - t0) * 1e6 / a.calls)
    out = {"side": a.parent_training or "this tree", "calls": a.calls, "n": opts["adam"][0].n,
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
           "variants": {v: {"median_us": statistics.median(t), "spread_us": max(t) - min(t),
                            "blocks_us": [round(x, 3) for x in t]} for v, t in times.items()}}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
