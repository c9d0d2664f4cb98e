"""Record the bits FlatAdam, FlatSGD and FlatRMSprop leave in every buffer, from the PARENT commit, on an MI355X.

    git worktree add ../parent <parent commit> && make -C ../parent/dctn_amd/csrc
    cp tests/golden/make_flat_step_parent.py ../parent/tests/golden/
    (cd ../parent && python tests/golden/make_flat_step_parent.py --commit <parent commit> --out <this tests/golden>)

writes tests/golden/flat_step_parent.json: per case one digest of the inputs and, per step and buffer, a 64-bit prefix of
the SHA-256 of the buffer's bytes.  tests/test_gpu_flat_step_parent.py rebuilds every case with the code under test and
compares.  The existing tests compare the forms of a step kernel with each other; this record is what notices all forms
changing together.

A case is ``<size>/<optimizer>/<variant>/<options>``:
  size      ``small``: n = 8199 in three parameters of 1001 / 3999 / 3199 elements, n_reg = 5000 - three workgroups of
            Adam's and RMSprop's geometry with a scalar tail of 3, 33 of SGD's, one table end inside a vector of four;
            ``odd``: the same with every buffer one element past an aligned address (float32 only), so that the launcher
            takes the scalar kernels; ``big``: n = 256 * 4096 + 4 * 1024 + 3 - lanes of the 1024-thread kernels take a second
            trip, SGD's four or more.
  optimizer `OPTIMIZERS`; variant `VARIANTS`
  options   a subset of guard, schedule, table, average (``small`` and ``odd``: all 16; ``big``: none and all four).  In
            the table the first segment runs at half the rate, the second is frozen, the third has its own decay where the
            optimizer takes one.
Steps (``big``: the first two): step 0 plain; step 1's gradient four times as large, so that a guard clips it; step 2
plain; guarded cases take one more with a single inf in the gradient: the launch is halted and must change nothing.

Only the public optimizer classes are used (an ``odd`` case moves the buffers of a built optimizer and the pointers of its
step descriptor), so the same script runs at both commits.  The record is never regenerated from the code under review.
"""
from __future__ import annotations

import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "flat_step_parent.json")

DEV = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
SMALL = (1001, 3999, 3199)
_BIG = 256 * 4096 + 4 * 1024 + 3
BIG = (400001, 500003, _BIG - 900004)   # ends inside vectors of four, too
SIZES = {"small": SMALL, "odd": SMALL, "big": BIG}
N_REG_PARAMS = 2
OPTIONS = ("guard", "schedule", "table", "average")
VARIANTS = {"float32": (F32, False), "bfloat16": (BF16, False), "bfloat16+master": (BF16, True)}
# name: (class, its arguments, whether a ParamGroup may name a weight decay)
OPTIMIZERS = {
    "adam": ("FlatAdam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, l2=1e-4), True),
    "sgd": ("FlatSGD", dict(lr=1e-2, momentum=0.9, l2=1e-4), False),
    "sgd_wd": ("FlatSGD", dict(lr=1e-2, momentum=0.9, l2=1e-4, weight_decay=1e-2), True),
    "rms0": ("FlatRMSprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=1e-2, momentum=0.0, l2=1e-4), True),
    "rms9": ("FlatRMSprop", dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=1e-2, momentum=0.9, l2=1e-4), True),
}
KNOTS = [(0, 2e-4), (2, 1e-3), (5, 5e-4)]   # every step of a case at another rate
OWN_DECAY = 5e-2
MOMENTS = ("m", "v", "square_avg", "buf")


def option_sets(size: str):
    every = [tuple(o for o, on in zip(OPTIONS, bits) if on) for bits in itertools.product((0, 1), repeat=4)]
    return [(), OPTIONS] if size == "big" else every


def case_names(optimizer: str, variant: str):
    """Every case of one optimizer and variant, in the record's order."""
    sizes = ("small", "odd", "big") if variant == "float32" else ("small", "big")
    return [f"{size}/{optimizer}/{variant}/{'+'.join(opts) or 'plain'}" for size in sizes for opts in option_sets(size)]


def digest(t: torch.Tensor) -> str:
    """64 bits of the SHA-256 of a tensor's bytes."""
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def inputs(size: str, dtype):
    """(w0, the gradients of steps 0 .. 3, the guard's threshold) from a seeded CPU generator."""
    n = sum(SIZES[size])
    g = torch.Generator().manual_seed(516 + n % 1000)
    w0 = (torch.randn(n, generator=g) * 0.05).to(dtype)
    grads = [(torch.randn(n, generator=g) * 0.01).to(dtype) for _ in range(4)]
    grads[1] = (grads[1].float() * 4.0).to(dtype)
    grads[3][4321] = float("inf")
    max_norm = 2.0 * float(grads[0].double().norm())   # steps 0 and 2 pass, step 1 is clipped
    return w0, grads, max_norm


def _moved(t: torch.Tensor) -> torch.Tensor:
    """The same values one element past an aligned address."""
    store = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    store[1:] = t
    assert store[1:].data_ptr() % 16 != 0
    return store[1:]


def _make_odd(opt) -> None:
    """Moves every per-element buffer of a built optimizer, and the pointers of its descriptors with them."""
    assert opt.master is None
    opt.flat = _moved(opt.flat)
    opt._desc.params = opt.flat.data_ptr()
    for name in MOMENTS:
        if getattr(opt, name, None) is not None:
            setattr(opt, name, _moved(getattr(opt, name)))
    if opt.ema is not None:
        opt.ema.values = _moved(opt.ema.values)
        opt.ema._desc.ema = opt.ema.values.data_ptr()


def build(name: str):
    """(optimizer, gradient store, gradients, steps to take, digest of the inputs) of a case."""
    from dctn_amd import training as T

    size, optimizer, variant, opts = name.split("/")
    opts = () if opts == "plain" else tuple(opts.split("+"))
    dtype, master = VARIANTS[variant]
    cls, args, takes_decay = OPTIMIZERS[optimizer]
    sizes = list(SIZES[size])
    w0, grads, max_norm = inputs(size, dtype)
    params = [torch.nn.Parameter(c.clone().to(DEV)) for c in w0.split(sizes)]
    kw = dict(args, master_weights=master)
    if "guard" in opts:
        kw["guard"] = T.GradGuard(DEV, max_norm)
    if "schedule" in opts:
        kw["schedule"] = T.LRSchedule(DEV, KNOTS)
    if "table" in opts:
        kw["groups"] = T.ParamGroups(params, [
            T.ParamGroup([params[0]], lr_scale=0.5), T.ParamGroup([params[1]], frozen=True),
            T.ParamGroup([params[2]], weight_decay=OWN_DECAY if takes_decay else None)])
    if "average" in opts:
        kw["ema"] = T.WeightEMA(DEV, 0.9, warmup=True)
    opt = getattr(T, cls)(params[:N_REG_PARAMS], params[N_REG_PARAMS:], **kw)
    store = torch.zeros(w0.numel() + 1, dtype=dtype, device=DEV)
    store = store[1:] if size == "odd" else store[:-1]
    for p, view in zip(params, store.split(sizes)):
        p.grad = view
    if size == "odd":
        _make_odd(opt)
    steps = 2 if size == "big" else 4 if "guard" in opts else 3
    h = hashlib.sha256()
    for t in [w0] + grads[:steps]:
        h.update(t.view(torch.uint8).numpy().tobytes())
    h.update(repr((max_norm, sorted(args.items()), KNOTS, OWN_DECAY)).encode())
    return opt, store, grads, steps, h.hexdigest()[:16]


def buffers(opt) -> dict:
    """Everything a step may write, by name.  sq_sum: the slots the launch used (the tensor has no others)."""
    torch.cuda.synchronize()
    out = {"params": opt.flat, "master": opt.master, "sq_sum": opt.sq_sum, "step_block": opt._state}
    for name in MOMENTS:
        out[name] = getattr(opt, name, None)
    if opt.guard is not None:
        out["guard_block"] = opt.guard._block
    if opt.groups is not None:
        out["table_steps"] = torch.tensor(opt.groups.steps, dtype=torch.int32)
        out["table_block"] = opt.groups._block
    if opt.ema is not None:
        out["average"], out["average_block"] = opt.ema.values, opt.ema._block
    return {k: v for k, v in out.items() if v is not None}


def run(name: str) -> dict:
    """The record's entry of a case: {"inputs": digest, "buffers": names, "steps": [[digest per buffer] per step]}."""
    opt, store, grads, steps, inputs_digest = build(name)
    names, rows = None, []
    for g in grads[:steps]:
        store.copy_(g)
        opt.step()
        now = buffers(opt)
        names = names or list(now)
        assert list(now) == names
        rows.append([digest(now[k]) for k in names])
    if name.startswith("odd/"):
        assert opt.flat.data_ptr() % 16 != 0 and opt._desc.params == opt.flat.data_ptr()
    return {"inputs": inputs_digest, "buffers": names, "steps": rows}


def all_cases():
    return [c for o in OPTIMIZERS for v in VARIANTS for c in case_names(o, v)]


def main() -> None:
    from dctn_amd import _lib as L

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the parent commit (40 characters)")
    ap.add_argument("--out", default=HERE, help="directory for the record")
    a = ap.parse_args()
    assert len(a.commit) == 40
    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        hipcc = f"unknown (torch.version.hip {torch.version.hip})"
    record = {"parent_commit": a.commit, "library_version": int(L.lib().dctn_version()), "hipcc": hipcc,
              "torch": torch.__version__, "device": torch.cuda.get_device_name(DEV), "cases": {}}
    for name in all_cases():
        record["cases"][name] = run(name)
    cases = record.pop("cases")
    with open(os.path.join(a.out, os.path.basename(RECORD)), "w") as f:   # the header, then one line per case
        f.write(json.dumps(record, indent=1)[:-2] + ',\n "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()))
        f.write("\n }\n}\n")
    print(f"{len(cases)} cases recorded from {a.commit}")


if __name__ == "__main__":
    main()
