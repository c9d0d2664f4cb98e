"""Preparing a colour source - per-channel moments and the autoscale factor - from the bytes against what it took before,
in one process.

`--samples` random (n, 32, 32, 3) uint8 images on the device, a constant channel, K = 3, the first 10 880 samples for the
factor (the reference's count):

  new   `colour_moments` (the histogram kernel, 4 x 256 integers to the host) and `calc_scaling_factor_from_bytes` (one
        workgroup per image through a 256-row table per channel, fixed-order sum)
  old   `channel_moments` on the device tensor (``bincount`` over a 4-byte copy of each channel) and `calc_scaling_factor` on
        the first 10 880 samples expanded to (1, 10880, 32, 32, 4) float64 on the device

Each variant runs `--repeats` times, the two alternating, every run between device synchronisations with the caching
allocator emptied and the peak counter reset in front of it, so that `peak_bytes` is what the run itself needed on top of
the resident bytes.  Prints one JSON line: per variant and stage the median, min and max time (ms), the peak device memory
over the resident data set (bytes), the numbers both give and whether the new ones repeat bit for bit.  A one-off set-up
cost: there is no threshold.

    python tools/time_colour_prepare.py [--samples 45000] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dctn_amd.batches import channel_moments, colour_moments, colour_table  # noqa: E402
from dctn_amd.window_stats import calc_scaling_factor, calc_scaling_factor_from_bytes  # noqa: E402

SIZE, CONSTANT, K, FIRST = 32, 1.0, 3, 10880


def expand_on_device(images, table):
    """(1, n, 32, 32, 4) float64 on the device from the float32 table: what a user of the expanded form holds."""
    t = table.to(images.device)
    cols = [t[c][images[..., c].long()] for c in range(3)] + [t[3][torch.zeros_like(images[..., 0]).long()]]
    return torch.stack(cols, dim=-1).unsqueeze(0).double()


def new_moments(images):
    return colour_moments(images)


def old_moments(images):
    mean, std = channel_moments(images)
    return mean.cpu(), std.cpu()


def new_factor(images, table):
    return calc_scaling_factor_from_bytes(images, table, K, samples=FIRST)


def old_factor(images, table):
    return calc_scaling_factor(expand_on_device(images[:FIRST], table), K)


def timed(fn, *args):
    dev = args[0].device
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=45000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (args.samples, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    stages = {"moments": (new_moments, old_moments), "factor": (new_factor, old_factor)}
    mean, std = colour_moments(images)
    table = colour_table(3, nu=1.0, mean=mean, std=std, constant_channel=CONSTANT, dtype=torch.float32)
    inputs = {"moments": (images,), "factor": (images, table)}
    for stage, fns in stages.items():   # one untimed run each: code objects, allocator
        for fn in fns:
            fn(*inputs[stage])
    ms = {s: {"new": [], "old": []} for s in stages}
    peak = {s: {"new": 0, "old": 0} for s in stages}
    outs = {s: {"new": [], "old": []} for s in stages}
    for r in range(args.repeats):
        for stage, fns in stages.items():
            for name, fn in zip(("new", "old"), fns):   # alternating
                out, t, p = timed(fn, *inputs[stage])
                ms[stage][name].append(t)
                peak[stage][name] = max(peak[stage][name], p)
                outs[stage][name].append(out)
                print(f"repeat {r} {stage} {name}: {t:.3f} ms, peak {p} bytes", file=sys.stderr, flush=True)
    result = {"workload": f"{args.samples} x 32 x 32 x 3 uint8, constant channel, K = {K}, first {FIRST} samples",
              "repeats": args.repeats, "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(dev),
              "resident_bytes": images.numel()}
    for stage in stages:
        result[stage] = {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                                "peak_bytes": peak[stage][name]} for name, t in ms[stage].items()}
    m_new, m_old = outs["moments"]["new"], outs["moments"]["old"]
    result["moments"]["new_repeat_bit_for_bit"] = all(torch.equal(a, m_new[0][i]) for o in m_new for i, a in enumerate(o))
    result["moments"]["largest_relative_difference"] = max(
        float(((a - b) / b).abs().max()) for a, b in zip(m_new[0], m_old[0]))
    f_new, f_old = outs["factor"]["new"], outs["factor"]["old"]
    result["factor"].update(new_value=f_new[0], old_values=sorted(set(f_old)), new_repeat_bit_for_bit=len(set(f_new)) == 1,
                            largest_relative_difference=max(abs(f / f_new[0] - 1.0) for f in f_old))
    result["total_new_ms"] = result["moments"]["new"]["median_ms"] + result["factor"]["new"]["median_ms"]
    result["total_old_ms"] = result["moments"]["old"]["median_ms"] + result["factor"]["old"]["median_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
