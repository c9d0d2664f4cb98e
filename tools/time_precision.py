"""Training step of the float32 large-core models under the "exact", "high" (bf16x3) and "bf16" policies, in one process.

Each (model, policy) is one GraphedTrainStep (the step replayed from captured HIP graphs, as bench.py does), timed over
`--repeats` blocks of `--steps` replays with device synchronisation around each block; the policies alternate block by
block so that clock and thermal drift fall on all three alike.  Prints one JSON line: per model and policy the median
and min of the per-step time over the blocks (ms), and the speed-up of "high" over "exact".

    python tools/time_precision.py [--steps 20] [--repeats 7] [--batch 128] [--models cfg3a] [--policies high]
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
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatSGD, GraphedTrainStep, fused_cross_entropy  # noqa: E402

MODELS = {   # the reference's float32 large-core models (BASELINE cfg3a, cfg3b, cfg4's EPS layer)
    "cfg3a": (((4, 4), (3, 6)), 28, 2),
    "cfg3b": (((4, 8), (2, 8)), 28, 2),
    "cfg4_eps36": (((3, 6),), 32, 4),
}
POLICIES = ("exact", "high", "bf16")


def make_step(name, policy, batch, dev):
    spec, size, q0 = MODELS[name]
    dctn_amd.set_float32_matmul_precision(policy)
    torch.manual_seed(0)
    model = EPSesPlusLinear(spec, UnitTheoreticalOutputStd(), 1.0, dev, torch.float32, image_size=size, Q_0=q0)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, batch, size, size, q0, generator=g)
    x = (x / x.sum(-1, keepdim=True)).to(dev)
    y = torch.randint(0, 10, (batch,), generator=g).to(dev)
    opt = FlatSGD(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-3, momentum=0.9, l2=1e-4)
    step = GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=2)
    dctn_amd.set_float32_matmul_precision("exact")
    return step, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--policies", default=",".join(POLICIES), help="a subset, e.g. for a profile of one policy")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"steps": args.steps, "repeats": args.repeats, "batch": args.batch, "models": {}}
    for name in args.models.split(","):
        policies = args.policies.split(",")
        steps = {pol: make_step(name, pol, args.batch, dev) for pol in policies}
        times = {pol: [] for pol in policies}
        for _ in range(args.repeats):
            for pol in policies:   # alternating: the graphs carry their policy's kernels
                step, x, y = steps[pol]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(x, y)
                torch.cuda.synchronize(dev)
                times[pol].append((time.perf_counter() - t0) * 1e3 / args.steps)
        entry = {pol: {"median_ms": statistics.median(t), "min_ms": min(t)} for pol, t in times.items()}
        if "exact" in entry and "high" in entry:
            entry["high_speedup_vs_exact"] = entry["exact"]["median_ms"] / entry["high"]["median_ms"]
        entry["loss"] = {pol: float(steps[pol][0].loss.detach()) for pol in policies}
        result["models"][name] = entry
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
