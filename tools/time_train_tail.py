#!/usr/bin/env python3
"""The complete graphed cfg2 bf16 training iteration (B = 1024) under four optimizers (the two flat ones also with
float32 master weights), and scoring with and without
the fused accumulate kernel - one process, the variants alternated round by round, so that the differences are
read against the spread of one variant repeated.

    python tools/time_train_tail.py [--rounds 7] [--iters 2000] [--out FILE.json]

Prints one JSON object: per variant the median over the rounds of the mean time of one iteration (microseconds,
device events around `iters` replays), its min and max, the same for ten scoring batches of 1024, and for the
optimizer launch alone over 1.9 M parameters (cfg3a's count)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd  # noqa: E402
from dctn_amd.evaluation import score, score_fused  # noqa: E402
from dctn_amd.training import FlatAdam, FlatSGD, GraphedTrainStep, fused_cross_entropy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=2000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.manual_seed(0)
u = torch.rand(1, 1024, 28, 28)
x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(torch.bfloat16).to(dev)
y = torch.randint(0, 10, (1024,), device=dev)
L2 = 1e-2


def make(kind):
    torch.manual_seed(0)
    model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, dev, torch.bfloat16)
    flat = (list(model.epses) + [model.linear.weight], [model.linear.bias])
    reg = dict(reg_fn=lambda m: m.epswise_l2_regularizer(), reg_coeff=L2)   # what the folded l2 term replaces
    master = kind.endswith("_master")
    if kind in ("flat_sgd", "flat_sgd_master"):
        opt = FlatSGD(*flat, lr=1e-3, momentum=0.9, l2=L2, master_weights=master)
        return GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=2)
    if kind in ("flat_adam", "flat_adam_master"):
        opt = FlatAdam(*flat, lr=1e-3, weight_decay=1e-4, l2=L2, master_weights=master)
        return GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=2)
    fused = kind == "torch_adam_fused"
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True, fused=fused or None)
    return GraphedTrainStep(model, x, y, fused_cross_entropy, opt, warmup=2, **reg)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


steps, skipped = {}, {}
for kind in ("flat_sgd", "flat_sgd_master", "torch_adam", "torch_adam_fused", "flat_adam", "flat_adam_master"):
    try:
        steps[kind] = make(kind)
    except Exception as e:   # this torch build may refuse fused=True, capturable=True on ROCm: recorded, not hidden
        if kind != "torch_adam_fused":
            raise
        skipped[kind] = f"{type(e).__name__}: {e}"[:300]
for s in steps.values():
    timed(lambda: s(x, y), 200)
times = {k: [] for k in steps}
repeat = []   # one variant twice in the same round: the spread a difference has to exceed
for _ in range(args.rounds):
    for k, s in steps.items():
        times[k].append(timed(lambda: s(x, y), args.iters))
    repeat.append(timed(lambda: steps["flat_sgd"](x, y), args.iters))

torch.manual_seed(0)
model = EPSesPlusLinear(((3, 4),), UnitTheoreticalOutputStd(), 1.0, dev, torch.bfloat16)
dl = [(x, y, torch.arange(1024)) for _ in range(10)]
scorers = {"score": score, "score_fused": score_fused}
for f in scorers.values():
    for _ in range(5):
        f(model, dl, dev)
score_times = {k: [] for k in scorers}
for _ in range(args.rounds):
    for k, f in scorers.items():
        score_times[k].append(timed(lambda: f(model, dl, dev), 20))

# the optimizer launch alone as a stream: cfg3a's parameter count (1.9 M), 20 steps per captured graph
N_STREAM, STEPS_PER_GRAPH = 1_900_000, 20
stream_graphs = {}
for dtype, master in ((torch.bfloat16, False), (torch.bfloat16, True), (torch.float32, False)):
    for name, cls, kw in (("flat_sgd", FlatSGD, dict(momentum=0.9)), ("flat_adam", FlatAdam, dict(weight_decay=1e-4))):
        p = torch.nn.Parameter(torch.randn(N_STREAM, device=dev).to(dtype) * 0.1)
        p.grad = (torch.randn(N_STREAM, device=dev) * 0.01).to(dtype)
        opt = cls([p], lr=1e-4, l2=1e-3, master_weights=master, **kw)
        opt.step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(STEPS_PER_GRAPH):
                opt.step()
        g.replay()
        stream_graphs[f"{name}_{str(dtype).split('.')[-1]}{'_master' if master else ''}"] = (g, opt)
stream_times = {k: [] for k in stream_graphs}
for _ in range(args.rounds):
    for k, (g, _) in stream_graphs.items():
        stream_times[k].append(timed(g.replay, 20) / STEPS_PER_GRAPH)


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "iters": args.iters,
          "iteration": {k: summary(v) for k, v in times.items()}, "flat_sgd_repeated": summary(repeat),
          "skipped": skipped, "score_10_batches_of_1024": {k: summary(v) for k, v in score_times.items()},
          "optimizer_step_alone_1p9M_parameters": {k: summary(v) for k, v in stream_times.items()},
          "score_values": {k: f(model, dl, dev) for k, f in scorers.items()}}
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
