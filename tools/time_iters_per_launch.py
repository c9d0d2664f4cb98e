"""Training iterations per graph launch: what one launch per iteration costs, and what the step trace costs, in one process.

cfg2 (bf16, B = 1024, FlatAdam with master weights) as a `GraphedTrainStep(batch_source=DeviceBatches(...))` over
`--samples` synthetic 28 x 28 uint8 images, five ways:

  K1        one iteration per launch, no trace: the graph as it was before `iters_per_launch` / `trace` existed
  K1_trace  one iteration per launch, every iteration ends with the step-trace launch
  K5_trace  five iterations per launch, with the trace
  K20_trace twenty iterations per launch, with the trace
  K20       twenty iterations per launch, no trace: what the launches alone cost, apart from the trace

Each variant is timed over `--repeats` blocks of `--iters` ITERATIONS (iters / K launches) with device synchronisation
around each block; the variants alternate block by block so that clock and thermal drift fall on all alike.  Prints one JSON
line: per variant the median, min, max and spread (max - min) of the time per iteration over the blocks (us), the ratio of
each variant's median to K1's, the cost of the trace at K = 1 (K1_trace - K1), and the size of each graph's private memory
pool (bytes reserved and bytes in use, from the allocator's snapshot) - which shows whether K iterations cost K times the
activations.  Every trace is read once at the end: `records_done` must equal the iterations that ran.

    python tools/time_iters_per_launch.py [--iters 10000] [--repeats 5] [--samples 50000] [--variants K1,K1_trace,...]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.batches import DeviceBatches  # noqa: E402
from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.training import FlatAdam, GraphedTrainStep, StepTrace, fused_cross_entropy  # noqa: E402

SPEC, SIZE, DTYPE, BATCH, WARMUP = ((3, 4),), 28, torch.bfloat16, 1024, 2
VARIANTS = {"K1": (1, False), "K1_trace": (1, True), "K5_trace": (5, True), "K20_trace": (20, True), "K20": (20, False)}


def pool_bytes(graph):
    """(reserved, in use) bytes of the graph's private pool, or None when the allocator's snapshot does not say."""
    try:
        pool = tuple(graph.pool())
        segments = [s for s in torch.cuda.memory_snapshot() if tuple(s.get("segment_pool_id", (0, 0))) == pool]
        return sum(s["total_size"] for s in segments), sum(s["active_size"] for s in segments)
    except Exception:   # noqa: BLE001
        return None


def make_variant(name, images, labels, dev):
    K, traced = VARIANTS[name]
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE)
    opt = FlatAdam(list(model.epses) + [model.linear.weight], [model.linear.bias], lr=1e-4, l2=1e-4, master_weights=True)
    src = DeviceBatches(images, labels, BATCH, dtype=DTYPE, seed=2024)
    trace = StepTrace(dev, capacity=64) if traced else None
    step = GraphedTrainStep(model, None, None, fused_cross_entropy, opt, warmup=WARMUP, batch_source=src,
                            iters_per_launch=K, trace=trace)
    return step, trace, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (args.samples,), generator=g)
    names = args.variants.split(",")
    runs = {v: make_variant(v, images, labels, dev) for v in names}
    pools = {v: pool_bytes(runs[v][0].g_main) for v in names}
    launches = {v: max(1, args.iters // VARIANTS[v][0]) for v in names}
    ran = {v: WARMUP for v in names}
    times = {v: [] for v in names}
    for v in names:   # one short untimed block each: clocks, allocator and caches settle before the first timed one
        for _ in range(max(1, min(args.iters, 200) // VARIANTS[v][0])):
            runs[v][0]()
            ran[v] += VARIANTS[v][0]
    for r in range(args.repeats):
        for v in names:   # alternating
            step, K = runs[v][0], VARIANTS[v][0]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(launches[v]):
                step()
            torch.cuda.synchronize(dev)
            times[v].append((time.perf_counter() - t0) * 1e6 / (launches[v] * K))
            ran[v] += launches[v] * K
            print(f"repeat {r} {v}: {times[v][-1]:.2f} us/iteration", file=sys.stderr, flush=True)
    result = {"workload": "cfg2 bf16 B=1024 FlatAdam(master) graphed, batch source", "samples": args.samples,
              "iters": args.iters, "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"),
              "device": torch.cuda.get_device_name(dev), "variants": {}}
    for v, t in times.items():
        entry = {"iters_per_launch": VARIANTS[v][0], "trace": VARIANTS[v][1], "median_us": statistics.median(t),
                 "min_us": min(t), "max_us": max(t), "spread_us": max(t) - min(t), "blocks_us": [round(b, 2) for b in t],
                 "pool_reserved_bytes": None if pools[v] is None else pools[v][0],
                 "pool_in_use_bytes": None if pools[v] is None else pools[v][1],
                 "batches_done": runs[v][2].state_dict()["batches_done"], "iterations_run": ran[v]}
        if runs[v][1] is not None:
            runs[v][1].read()
            entry["records_done"] = runs[v][1].state_dict()["records_done"]
        result["variants"][v] = entry
    med = {v: result["variants"][v]["median_us"] for v in names}
    if "K1" in med:
        result["ratio_to_K1"] = {v: med[v] / med["K1"] for v in names}
        if "K1_trace" in med:
            result["trace_cost_at_K1_us"] = med["K1_trace"] - med["K1"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
