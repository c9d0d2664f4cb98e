"""Record what `checkpoint.RunState` lays out and writes, from the PARENT commit, on an MI355X.

    git worktree add ../parent <parent commit> && make -C ../parent/dctn_amd/csrc
    cp tests/golden/make_run_state_parent.py ../parent/tests/golden/
    (cd ../parent && python tests/golden/make_run_state_parent.py --commit <parent commit> --out <this tests/golden>)

writes tests/golden/run_state_parent.json - per case of `CASES` the run's ``entries``, the ``model`` and ``host`` parts of
``run.snapshot().manifest`` and ``arena_bytes``; the extras and the refusal messages of the two files - and the two
snapshot files of `FILES` beside it, each written after three eager steps.  tests/test_gpu_run_state_format.py rebuilds
every case with the code under test and loads the two files into objects built from other seeds and other
hyper-parameters (``variant=1``; nothing of variant 1 is in the record but the refusal messages, which name no value
of it).

Only the public surface of `RunState` and of the components is used, so the same script runs at both commits.  The record
is never regenerated from the code under review: a format change that is meant shows up as a diff of these files made
from the commit that precedes it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "run_state_parent.json")

DEV = torch.device("cuda", 0)
SPEC, IMAGE, N_SAMPLES, BATCH, CAPACITY = ((3, 4),), 8, 16, 4, 8
OPTIONS = ("master", "guard", "schedule", "groups", "source", "trace", "dropout")
# name: (optimizer, then one flag per entry of OPTIONS; "master" is bfloat16 parameters with float32 master weights,
# off is float32).  Every option is on and off for both optimizers; the last case has no optimizer.
CASES = {
    "adam_all":                     ("adam", 1, 1, 1, 1, 1, 1, 1),
    "adam_f32_plain":               ("adam", 0, 0, 0, 0, 0, 0, 0),
    "adam_bf16_plain":              ("adam", 1, 0, 0, 0, 0, 0, 0),
    "adam_f32_guard_source":        ("adam", 0, 1, 0, 0, 1, 0, 0),
    "adam_f32_schedule_trace":      ("adam", 0, 0, 1, 0, 0, 1, 0),
    "adam_bf16_groups_dropout":     ("adam", 1, 0, 0, 1, 0, 0, 1),
    "adam_f32_sched_groups_src_do": ("adam", 0, 0, 1, 1, 1, 0, 1),
    "adam_bf16_guard_trace":        ("adam", 1, 1, 0, 0, 0, 1, 0),
    "sgd_f32_guard_groups_source":  ("sgd", 0, 1, 0, 1, 1, 0, 0),
    "sgd_f32_plain":                ("sgd", 0, 0, 0, 0, 0, 0, 0),
    "sgd_bf16_plain":               ("sgd", 1, 0, 0, 0, 0, 0, 0),
    "sgd_all":                      ("sgd", 1, 1, 1, 1, 1, 1, 1),
    "sgd_f32_schedule":             ("sgd", 0, 0, 1, 0, 0, 0, 0),
    "sgd_bf16_guard_trace_dropout": ("sgd", 1, 1, 0, 0, 0, 1, 1),
    "sgd_f32_sched_groups_source":  ("sgd", 0, 0, 1, 1, 1, 0, 0),
    "sgd_bf16_groups":              ("sgd", 1, 0, 0, 1, 0, 0, 0),
    "no_optimizer":                 (None, 0, 1, 0, 0, 1, 1, 1),
}
# the two files: "Adam with everything on" and "grouped SGD without a schedule"
FILES = {"adam_all": "run_state_parent_adam.dctn", "sgd_f32_guard_groups_source": "run_state_parent_sgd.dctn"}
EXTRAS = {"num_iters_done": 2, "best": 0.25}
STEPS = 3

# what differs between the recorded objects (variant 0) and the fresh ones a file is loaded into (variant 1)
SEEDS = (dict(model=1, dropout=77, batch=5), dict(model=2, dropout=1234567, batch=99))
ADAM = (dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, l2=1e-4),
        dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, l2=3e-4))
SGD = (dict(lr=1e-3, momentum=0.9, l2=1e-4), dict(lr=5e-2, momentum=0.5, l2=0.0))
MAX_NORM = (2.5, 40.0)
KEEP = (0.9, 0.75)   # the dropout's p
KNOTS = (([(0, 0.0), (2, 1e-3), (5, 5e-4)], [0, 1, 0]), ([(0, 1e-2), (7, 1e-3)], None))
SCALE = (0.5, 1.0)
GROUP_LR_SCALES = ((0.5, 2.0), (1.0, 0.25))   # of the core and of the head's weight; the bias is frozen in variant 0


def data():
    g = torch.Generator().manual_seed(2026)
    return (torch.randint(0, 256, (N_SAMPLES, IMAGE, IMAGE), dtype=torch.uint8, generator=g),
            torch.randint(0, 10, (N_SAMPLES,), generator=g))


def build_case(name: str, variant: int = 0) -> SimpleNamespace:
    """The objects of a case and their `RunState`: model, opt, schedule, groups, guard, src, trace, run (None where the
    case has none)."""
    from dctn_amd import checkpoint as C
    from dctn_amd.batches import DeviceBatches
    from dctn_amd.eps_plus_linear import EPSesPlusLinear, UnitTheoreticalOutputStd
    from dctn_amd.training import FlatAdam, FlatSGD, GradGuard, LRSchedule, ParamGroup, ParamGroups, StepTrace

    kind, *flags = CASES[name]
    on = SimpleNamespace(**dict(zip(OPTIONS, map(bool, flags))))
    seeds = SEEDS[variant]
    dtype = torch.bfloat16 if on.master else torch.float32
    torch.manual_seed(seeds["model"])
    model = EPSesPlusLinear(SPEC, UnitTheoreticalOutputStd(), KEEP[variant] if on.dropout else 1.0, DEV, dtype,
                            image_size=IMAGE)
    if on.dropout:
        model.use_fused_dropout(seeds["dropout"])
    guard = GradGuard(DEV, MAX_NORM[variant]) if on.guard else None
    src = trace = schedule = groups = opt = None
    if on.source:
        images, labels = data()
        src = DeviceBatches(images, labels, BATCH, dtype=dtype, seed=seeds["batch"], rank=0, world=1, device=DEV)
    if on.trace:
        trace = StepTrace(DEV, CAPACITY)
    params = list(model.epses) + [model.linear.weight, model.linear.bias]
    if kind is not None:
        if on.schedule:
            schedule = LRSchedule(DEV, *KNOTS[variant])
            schedule.scale = SCALE[variant]
        if on.groups:
            core, head = GROUP_LR_SCALES[variant]
            groups = ParamGroups(params, [
                ParamGroup([params[0]], lr_scale=core, weight_decay=1e-3 if kind == "adam" and variant == 0 else None),
                ParamGroup([params[1]], lr_scale=head), ParamGroup([params[2]], frozen=variant == 0)])
        kw = dict(master_weights=on.master, guard=guard, schedule=schedule, groups=groups)
        opt = (FlatAdam(params[:-1], params[-1:], **ADAM[variant], **kw) if kind == "adam" else
               FlatSGD(params[:-1], params[-1:], **SGD[variant], **kw))
    run = C.RunState(model, opt, batch_source=src, guard=None if kind is not None else guard, trace=trace)
    return SimpleNamespace(name=name, kind=kind, on=on, model=model, opt=opt, schedule=schedule, groups=groups,
                           guard=guard, src=src, trace=trace, run=run)


def take_steps(case: SimpleNamespace, steps: int = STEPS) -> None:
    """Eager iterations of a case that has an optimizer and a source, each followed by the trace's record."""
    from dctn_amd.training import fused_cross_entropy, train_step

    for _ in range(steps):
        x, y, _ = case.src.draw()
        out = train_step(case.model, x, y, fused_cross_entropy, case.opt)
        if case.trace is not None:
            case.trace.record(out["output"], y, out["loss"], guard=case.guard, optimizer=case.opt, batch_source=case.src)


def layout(run) -> dict:
    """What the record holds of a run: entries, the manifest's model and host parts, the arena's size."""
    snap = run.snapshot()
    snap.wait()
    return json.loads(json.dumps(dict(entries=[[n, d, list(s)] for n, d, s in run.entries], model=snap.manifest["model"],
                                      host=snap.manifest["host"], arena_bytes=run.arena_bytes)))


def damaged_copy(path: str, how: str, out: str) -> str:
    """A copy of a snapshot file that a run of the same shape must refuse: ``kind`` - the other optimizer's name in the
    host scalars; ``batch_size`` - twice the source's; ``region`` - the last region gone, manifest and arena."""
    from dctn_amd import checkpoint as C

    manifest, arena = C.read_file(path)
    if how == "kind":
        saved = manifest["host"]["optimizer"]
        saved["kind"] = "FlatSGD" if saved["kind"] == "FlatAdam" else "FlatAdam"
    elif how == "batch_size":
        manifest["host"]["batch_source"]["batch_size"] *= 2
    elif how == "region":
        last = manifest["regions"].pop()
        arena = arena[: last["offset"]]
        manifest["arena_bytes"] = int(arena.size)
    else:
        raise KeyError(how)
    C.write_file(out, manifest, arena)
    return out


REFUSALS = ("kind", "batch_size", "region")


def refusal(run, path: str) -> str:
    """The message with which ``run.load(path)`` refuses, the path itself replaced by ``{path}``."""
    try:
        run.load(path)
    except ValueError as e:
        return str(e).replace(path, "{path}")
    raise AssertionError(f"{path} was loaded")


def main() -> None:
    import tempfile

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the parent commit (40 characters)")
    ap.add_argument("--out", default=HERE, help="directory for the record and the two files")
    a = ap.parse_args()
    assert len(a.commit) == 40
    record = {"parent_commit": a.commit, "device": torch.cuda.get_device_name(DEV), "cases": {}, "files": {}}
    for name in CASES:
        case = build_case(name)
        record["cases"][name] = layout(case.run)
        if name not in FILES:
            continue
        take_steps(case)
        path = case.run.snapshot(EXTRAS).save(os.path.join(a.out, FILES[name]))
        fresh = build_case(name, variant=1)
        with tempfile.TemporaryDirectory() as tmp:
            refusals = {how: refusal(fresh.run, damaged_copy(path, how, os.path.join(tmp, f"{how}.dctn")))
                        for how in REFUSALS}
        assert fresh.run.load(path) == EXTRAS
        record["files"][name] = dict(file=FILES[name], bytes=os.path.getsize(path), extras=EXTRAS, refusals=refusals)
        print(f"{FILES[name]}: {os.path.getsize(path)} bytes; {refusals}")
    with open(os.path.join(a.out, os.path.basename(RECORD)), "w") as f:
        json.dump(record, f, indent=1)   # (the host scalars keep their key order)
        f.write("\n")
    print(f"{len(record['cases'])} cases recorded from {a.commit}")


if __name__ == "__main__":
    main()
