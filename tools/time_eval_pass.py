"""One scheduled evaluation of the reference's runner, three ways, in one process.

The runner scores the whole training set and the validation set at every scheduled evaluation (new_runner.py:456-462).
Here: cfg2 in bf16, global batch 1024, synthetic 28 x 28 uint8 sets of `--train` and `--val` samples (50 000 + 10 000 are
49 + 10 = 59 batches), each set scored once per evaluation:

  a   `evaluation.score` (torch ops per batch) over the eager sequential source (`shuffle=False, drop_last=False`)
  b   `evaluation.score_fused` over the same source: gather, forward and one score launch per batch, all eager
  c   `evaluation.GraphedScore`: one captured graph of one padded batch per set, replayed `padded_steps` times

An evaluation is timed from the first launch to the host holding both results (every variant ends in a device-to-host
read).  `--repeats` blocks of `--evals` evaluations per variant; the variants alternate block by block so that clock and
thermal drift fall on all alike.  Prints one JSON line: per variant the median, min and max of the per-evaluation time over
the blocks (us) and the spread (max - min), the per-batch time of each, and whether c is below b by more than the larger
of their two spreads, and whether b and c report the same accuracies.

    python tools/time_eval_pass.py [--evals 20] [--repeats 5] [--train 50000] [--val 10000] [--variants a,b,c]
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
from dctn_amd.evaluation import GraphedScore, score, score_fused  # noqa: E402

SPEC, SIZE, DTYPE, BATCH = ((3, 4),), 28, torch.bfloat16, 1024


def make_set(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, SIZE, SIZE), dtype=torch.uint8, generator=g), torch.randint(0, 10, (n,), generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train", type=int, default=50000)
    ap.add_argument("--val", type=int, default=10000)
    ap.add_argument("--variants", default="a,b,c")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), 1.0, dev, DTYPE, image_size=SIZE).eval()
    sets = [make_set(args.train, 1), make_set(args.val, 2)]
    eager = [DeviceBatches(im, lab, BATCH, dtype=DTYPE, seed=0, shuffle=False, drop_last=False) for im, lab in sets]
    names = args.variants.split(",")
    runs = {}
    if "a" in names:
        runs["a"] = lambda: [score(model, src, dev) for src in eager]
    if "b" in names:
        runs["b"] = lambda: [score_fused(model, src, dev) for src in eager]
    if "c" in names:
        scorers = [GraphedScore(model, DeviceBatches(im, lab, BATCH, dtype=DTYPE, seed=0, shuffle=False)) for im, lab in sets]

        def graphed():
            for s in scorers:   # both passes are enqueued before either is read (make_evaluation_hook)
                s.launch()
            return [s.read() for s in scorers]

        runs["c"] = graphed
    results = {v: runs[v]() for v in names}   # one untimed evaluation each
    times = {v: [] for v in names}
    for r in range(args.repeats):
        for v in names:   # alternating
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.evals):
                runs[v]()
            torch.cuda.synchronize(dev)
            times[v].append((time.perf_counter() - t0) * 1e6 / args.evals)
            print(f"repeat {r} {v}: {times[v][-1]:.1f} us/evaluation", file=sys.stderr, flush=True)
    batches = sum(len(src) for src in eager)
    out = {"workload": "cfg2 bf16 B=1024, score the train and the validation set once", "train": args.train,
           "val": args.val, "batches": batches, "evals": args.evals, "repeats": args.repeats,
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev),
           "variants": {v: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                            "spread_us": max(t) - min(t), "per_batch_us": statistics.median(t) / batches,
                            "blocks_us": [round(b, 1) for b in t]} for v, t in times.items()},
           "results": results}
    if "b" in times and "c" in times:
        med, spread = {v: out["variants"][v]["median_us"] for v in "bc"}, {v: out["variants"][v]["spread_us"] for v in "bc"}
        out["c_below_b_beyond_spread"] = med["b"] - med["c"] > max(spread["b"], spread["c"])
        out["b_over_c"] = med["b"] / med["c"]
        out["b_and_c_report_equal_accuracies"] = [a for _, a in results["b"]] == [a for _, a in results["c"]]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
