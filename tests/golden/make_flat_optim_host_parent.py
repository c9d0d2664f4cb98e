"""Record what FlatAdam, FlatSGD and FlatRMSprop show on the HOST, from the PARENT commit.  No GPU: the optimizers build on
CPU tensors and nothing is launched.

    git worktree add ../parent <parent commit> && make -C ../parent/dctn_amd/csrc
    cp tests/golden/make_flat_optim_host_parent.py ../parent/tests/golden/
    (cd ../parent && python tests/golden/make_flat_optim_host_parent.py --commit <parent commit> --out <this tests/golden>)

writes tests/golden/flat_optim_host_parent.json.  tests/test_host_flat_optim_parent.py rebuilds every case with the code
under test and compares for equality.  tests/golden/flat_step_parent.json holds the bits the step kernels leave; this
record holds the other half of the classes: every key, key order, value and value type of ``state_dict()`` and
``run_host()``, the names of ``run_regions()``, ``lr``, ``t``, the step block's bytes, the descriptor's pointers and the
texts of the refusals.

A case is ``<optimizer>/<options>`` over parameters of `SIZES` elements, the first `N_REG_PARAMS` regularised:
  optimizer `OPTIMIZERS`
  options   `OPTION_SETS` for all three; `EXTRA` adds FlatSGD's weight decay (alone as 0.0, and as 0.25 under a table
            that names another) and FlatRMSprop's momentum buffer.
Observed, each time with `observe`: the optimizer as built; after ``lr`` was assigned (where it may be); after
``load_state_dict`` of a fixed state (count 5, another rate, halved hyper-parameters, buffers from a seeded generator);
after ``load_state_dict`` of that state written without ``master`` / ``ema`` / FlatSGD's ``weight_decay``; after
``run_restored(run_host(), own bytes)``; and after ``run_restored`` with other host scalars.

In the file a case holds its first observation whole and of each later one the fields that changed (`packed`).

Only the public classes are used, so the same script runs at both commits.  (On a machine without a GPU the recording,
and only the recording, answers the parent's FlatAdam that no capture is running: see `main`.)  The record is never
regenerated from the code under review.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "flat_optim_host_parent.json")

SIZES = [7, 1, 30, 5]
N_REG_PARAMS = 3
KNOTS, HOLD, SCALE = [(0, 0.0), (2, 1e-3), (5, 5e-4)], [0, 1, 0], 0.7
# name: (class, its arguments, the key the count travels under, whether a ParamGroup may name a weight decay)
OPTIMIZERS = {
    "adam": ("FlatAdam", dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, l2=1e-4), "t", True),
    "sgd": ("FlatSGD", dict(lr=1e-2, momentum=0.9, l2=1e-4), "steps", False),
    "rmsprop": ("FlatRMSprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=1e-2, l2=1e-4), "t", True),
}
OPTION_SETS = ("plain", "schedule", "groups", "ema", "schedule+groups+ema", "bfloat16+master")
EXTRA = {"sgd": {"decay0": ("plain", dict(weight_decay=0.0)), "decay+groups": ("groups", dict(weight_decay=0.25))},
         "rmsprop": {"momentum": ("plain", dict(momentum=0.9))}}
DESC_TENSORS = ("params", "master", "sq_sum", "state", "guard", "schedule", "groups")


def all_cases():
    return [f"{o}/{s}" for o in OPTIMIZERS for s in OPTION_SETS + tuple(EXTRA.get(o, ()))]


def digest(t: torch.Tensor) -> str:
    """64 bits of the SHA-256 of a tensor's bytes."""
    raw = t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def render(v):
    """A value with its Python type, ready for JSON: key order, tuple against list and int against float all show.  A
    dictionary becomes the list of its ``[key, value]`` pairs in its own order, so a record of one holds the ordered keys,
    the sorted keys and every value at once."""
    if isinstance(v, torch.Tensor):
        return f"Tensor:{v.dtype}:{list(v.shape)}:{digest(v)}"
    if isinstance(v, dict):
        return [[k, render(x)] for k, x in v.items()]
    if isinstance(v, (tuple, list)):
        return {type(v).__name__: [render(x) for x in v]}
    return f"{type(v).__name__}:{v!r}"


def build(name: str, **more):
    """(optimizer, its parameters) of a case; ``more`` overrides constructor arguments."""
    from dctn_amd import training as T

    optimizer, options = name.split("/")
    cls, args, _, takes_decay = OPTIMIZERS[optimizer]
    kw = dict(args)
    if options in EXTRA.get(optimizer, {}):
        options, extra = EXTRA[optimizer][options]
        kw.update(extra)
        takes_decay = takes_decay or "weight_decay" in extra
    options = options.split("+")
    dtype = torch.bfloat16 if "bfloat16" in options else torch.float32
    g = torch.Generator().manual_seed(517)
    params = [torch.nn.Parameter((torch.randn(k, generator=g) * 0.05).to(dtype)) for k in SIZES]
    kw["master_weights"] = "master" in options
    if "schedule" in options:
        kw["schedule"] = T.LRSchedule("cpu", KNOTS, HOLD)
        kw["schedule"].scale = SCALE
    if "groups" in options:
        kw["groups"] = T.ParamGroups(params, [
            T.ParamGroup([params[0]], lr_scale=0.5, weight_decay=1e-3 if takes_decay else None),
            T.ParamGroup([params[3]], frozen=True)])
    if "ema" in options:
        kw["ema"] = T.WeightEMA("cpu", 0.9, warmup=True)
    kw.update(more)
    return getattr(T, cls)(params[:N_REG_PARAMS], params[N_REG_PARAMS:], **kw), params


def observe(opt) -> dict:
    state, host = opt.state_dict(), opt.run_host()
    d = opt._desc
    tensors = dict(params=opt.flat, master=opt.master, sq_sum=opt.sq_sum, state=opt._state,
                   guard=None if opt.guard is None else opt.guard._block,
                   schedule=None if opt.schedule is None else opt.schedule._block,
                   groups=None if opt.groups is None else opt.groups._block)
    desc = [f + "=" + ("null" if not getattr(d, f) else "set") + "/" +
            ("none" if tensors[f] is None else "same" if tensors[f].data_ptr() == getattr(d, f) else "OTHER")
            for f in DESC_TENSORS]
    desc = " ".join(desc + [f"n={d.n} n_reg={d.n_reg} l2={float(d.l2)!r} dtype={d.dtype} ema_ref={opt._ema_ref is not None}"])
    seen = {
        "state": render(state), "host": render(host),
        "regions": [n for n, _ in opt.run_regions()],
        "regions_are_the_attributes": all(t is getattr(opt, n) for n, t in opt.run_regions()
                                          if n in ("flat", "m", "v", "buf", "square_avg", "master", "sq_sum")),
        "lr": render(opt.lr), "_lr": render(opt._lr), "t": render(opt.t), "_steps": render(getattr(opt, "_steps", None)),
        "step_block": None if opt._state is None else bytes(opt._state.view(torch.uint8).tolist()).hex(),
        "what": opt._what, "moments": list(opt._MOMENTS), "desc": desc,
    }
    if type(opt).__name__ != "FlatSGD":
        seen["lr_cell_is_cell_1"] = opt._lr_cell.data_ptr() == opt._state.data_ptr() + 4 and opt._lr_cell.numel() == 1
    if opt.groups is not None:
        seen["table_decays"] = render(opt.groups.weight_decays)
    return seen


def fixed_state(opt, count_key: str) -> dict:
    """A state of ``opt``'s own shape: count 5, another rate, every other scalar halved, tensors from a seeded generator."""
    g = torch.Generator().manual_seed(5)

    def other(key, v):
        if isinstance(v, torch.Tensor):
            return torch.randn(v.shape, generator=g).to(v.dtype)
        if isinstance(v, dict):
            return {k: other(k, x) for k, x in v.items()}
        if isinstance(v, tuple):
            return tuple(x * 0.5 for x in v)
        if key == count_key:
            return 5
        if key == "lr":
            return 0.0375
        if key == "updates":
            return 3
        if key in ("warmup", "decay"):
            return v
        return v * 0.5
    return {k: other(k, v) for k, v in opt.state_dict().items()}


def other_host(opt) -> dict:
    """``run_host()`` with other scalars: what a file written by another run of the same kind holds."""
    host = {}
    for k, v in opt.run_host().items():
        host[k] = v if k == "kind" else 9 if k == "steps" else [x * 0.25 for x in v] if isinstance(v, list) else v * 0.25
    return host


def own_blocks(opt) -> dict:
    return {n: t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().copy() for n, t in opt.run_regions()}


def refusal(f) -> list:
    try:
        f()
    except Exception as e:   # the record is of whatever is raised
        return [type(e).__name__, str(e)]
    return ["nothing raised", ""]


def run(name: str) -> dict:
    """The record's entry of a case."""
    optimizer = name.split("/")[0]
    count_key = OPTIMIZERS[optimizer][2]
    opt, _ = build(name)
    entry = {"built": observe(opt)}
    if opt.schedule is None:
        opt.lr = 0.0625
        entry["lr_assigned"] = observe(opt)
    state = fixed_state(opt, count_key)
    opt.load_state_dict(state)
    entry["loaded"] = observe(opt)
    bare = {k: v for k, v in fixed_state(opt, count_key).items() if k not in ("master", "ema") and
            not (optimizer == "sgd" and k == "weight_decay")}
    opt.load_state_dict(bare)
    entry["loaded_bare"] = observe(opt)
    opt.run_restored(opt.run_host(), own_blocks(opt))
    entry["restored"] = observe(opt)
    opt.run_restored(other_host(opt), own_blocks(opt))
    entry["restored_other"] = observe(opt)
    return json.loads(json.dumps(entry))


def packed(entry: dict) -> dict:
    """The record's form of a case: the first observation whole, of each later one the fields that differ from the one
    before it (most - regions, descriptor, `_what` - never change)."""
    out, before = {}, {}
    for moment, seen in entry.items():
        out[moment] = {k: v for k, v in seen.items() if k not in before or before[k] != v}
        assert list(seen) == list(before) or not before
        before = seen
    return out


def unpacked(record: dict) -> dict:
    out, before = {}, {}
    for moment, delta in record.items():
        before = out[moment] = {**before, **delta}
    return out


def refusals() -> dict:
    """The type and the full message of every refusal that can be reached without a device."""
    from dctn_amd import training as T

    out = {}
    for optimizer, (cls, _, count_key, _) in OPTIMIZERS.items():
        scheduled, _ = build(f"{optimizer}/schedule")
        out[f"{optimizer}/lr under a schedule"] = refusal(lambda: setattr(scheduled, "lr", 0.5))
        plain, _ = build(f"{optimizer}/plain")
        wrong = {k: (torch.zeros(v.numel() + 1) if isinstance(v, torch.Tensor) else v)
                 for k, v in fixed_state(plain, count_key).items()}
        out[f"{optimizer}/a state of the wrong size"] = refusal(lambda: plain.load_state_dict(wrong))
        mastered, _ = build(f"{optimizer}/bfloat16+master")
        wrong = dict(fixed_state(mastered, count_key), master=torch.zeros(3))
        out[f"{optimizer}/a master copy of the wrong size"] = refusal(lambda: mastered.load_state_dict(wrong))
        other = "FlatSGD" if cls != "FlatSGD" else "FlatAdam"
        out[f"{optimizer}/run_check with another kind"] = refusal(lambda: plain.run_check(dict(plain.run_host(), kind=other)))
        out[f"{optimizer}/run_check with its own kind"] = refusal(lambda: plain.run_check(plain.run_host()))
    light, _ = build("rmsprop/plain")
    heavy, _ = build("rmsprop/momentum")
    for label, opt, giver in (("a state with momentum", light, heavy), ("a state without momentum", heavy, light)):
        state = fixed_state(giver, "t")
        out[f"rmsprop/load_state_dict of {label}"] = refusal(lambda: opt.load_state_dict(state))
        out[f"rmsprop/run_restored of {label}"] = refusal(lambda: opt.run_restored(giver.run_host(), own_blocks(opt)))
    _, params = build("sgd/plain")
    table = T.ParamGroups(params, [T.ParamGroup([params[1]], weight_decay=0.5)])
    out["sgd/a table with a weight decay"] = refusal(lambda: T.FlatSGD(params[:N_REG_PARAMS], params[N_REG_PARAMS:],
                                                                        groups=table))
    out["sgd/a negative weight decay"] = refusal(lambda: build("sgd/plain", weight_decay=-1.0))
    out["adam/invalid hyper-parameters"] = refusal(lambda: build("adam/plain", eps=-1.0))
    out["rmsprop/invalid hyper-parameters"] = refusal(lambda: build("rmsprop/plain", alpha=1.0))
    out["adam/a schedule that is none"] = refusal(lambda: build("adam/plain", schedule=object()))
    out["adam/an average that is none"] = refusal(lambda: build("adam/plain", ema=object()))
    return out


def main() -> None:
    from dctn_amd import _lib as L

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the parent commit (40 characters)")
    ap.add_argument("--out", default=HERE, help="directory for the record")
    a = ap.parse_args()
    assert len(a.commit) == 40
    if not torch.cuda.is_available():
        # The parent's FlatAdam.lr asks the runtime whether a capture is running whatever the device of its tensors, and
        # on a machine without a GPU that question raises.  Recording only: answer what a machine with one answers outside
        # a capture.  `run` and `refusals` themselves patch nothing, so the test needs no such answer from the code under
        # test.
        torch.cuda.is_current_stream_capturing = lambda: False
    record = {"parent_commit": a.commit, "library_version": int(L.lib().dctn_version()), "torch": torch.__version__,
              "refusals": refusals(), "cases": {name: packed(run(name)) for name in all_cases()}}
    cases = record.pop("cases")
    with open(os.path.join(a.out, os.path.basename(RECORD)), "w") as f:   # the header, then one line per observation
        f.write(json.dumps(record, indent=1)[:-2] + ',\n "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(name)}: {{\n" + ",\n".join(
            f"   {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in case.items()) + "\n  }"
            for name, case in cases.items()))
        f.write("\n }\n}\n")
    record["cases"] = cases
    print(f"{len(record['cases'])} cases and {len(record['refusals'])} refusals recorded from {a.commit}")


if __name__ == "__main__":
    main()
