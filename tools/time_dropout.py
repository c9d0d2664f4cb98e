"""Training iteration with component dropout: p = 1, p = 0.9 on torch's element-wise ops (the default path), p = 0.9 on
the fused kernels (`EPSesPlusLinear.use_fused_dropout`), in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) runs as a GraphedTrainStep, the step replayed from a captured HIP
graph; cfg3a (float32, B = 128, FlatAdam) runs eagerly through `train_step`.  Each variant is timed over `--repeats`
blocks of `--steps` iterations with device synchronisation around each block; the variants alternate block by block so
that clock and thermal drift fall on all three alike.  Prints one JSON line: per workload and variant the median, min
and max of the per-iteration time over the blocks (us), the spread (max - min) of the p = 1 blocks, and whether the fused
median is below the torch-op median by more than that spread.

    python tools/time_dropout.py [--steps 50] [--repeats 9] [--workloads cfg2_graph,cfg3a_eager]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, fused_cross_entropy, train_step  # noqa: E402

WORKLOADS = {   # name -> (specs, image size, dtype, batch, graphed)
    "cfg2_graph": (((3, 4),), 28, torch.bfloat16, 1024, True),
    "cfg3a_eager": (((4, 4), (3, 6)), 28, torch.float32, 128, False),
}
VARIANTS = {"p1": (1.0, False), "p09_torch_ops": (0.9, False), "p09_fused": (0.9, True)}


def make_step(name, variant, dev):
    spec, size, dtype, batch, graphed = WORKLOADS[name]
    p, fused = VARIANTS[variant]
    torch.manual_seed(0)
    model = EPSesPlusLinear(spec, UnitTheoreticalOutputStd(), p, dev, dtype, image_size=size)
    if fused:
        model.use_fused_dropout(2024)
    g = torch.Generator().manual_seed(1)
    u = torch.rand(1, batch, size, size, generator=g)
    x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype).to(dev)
    y = torch.randint(0, 10, (batch,), generator=g).to(dev)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4,
                   master_weights=dtype == torch.bfloat16)
    if graphed:
        step = GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=2)
        return (lambda: step(x, y)), model, opt
    for _ in range(2):
        train_step(model, x, y, fused_cross_entropy, opt)
    return (lambda: train_step(model, x, y, fused_cross_entropy, opt)), model, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"steps": args.steps, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"), "workloads": {}}
    for name in args.workloads.split(","):
        steps = {v: make_step(name, v, dev) for v in VARIANTS}
        times = {v: [] for v in VARIANTS}
        for v in VARIANTS:   # one untimed block each: clocks, allocator and caches settle before the first timed one
            for _ in range(args.steps):
                steps[v][0]()
        for _ in range(args.repeats):
            for v in VARIANTS:   # alternating
                run = steps[v][0]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run()
                torch.cuda.synchronize(dev)
                times[v].append((time.perf_counter() - t0) * 1e6 / args.steps)
        entry = {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "blocks_us": [round(b, 2) for b in t]}
                 for v, t in times.items()}
        spread = entry["p1"]["max_us"] - entry["p1"]["min_us"]
        gap = entry["p09_torch_ops"]["median_us"] - entry["p09_fused"]["median_us"]
        entry["p1_spread_us"] = spread
        entry["torch_ops_minus_fused_us"] = gap
        entry["fused_faster_beyond_spread"] = gap > spread
        # the in-place gradient path holds under fused dropout for the single-layer model (no gather launch)
        entry["grads_in_place"] = {v: steps[v][2]._grads().data_ptr() != steps[v][2].flat_grad.data_ptr() for v in VARIANTS}
        entry["draws_done_fused"] = steps["p09_fused"][1].dropout_state_dict()["draws_done"]
        result["workloads"][name] = entry
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
