"""Durations of a step's kernels and the gaps at the boundaries between them, from a kernel trace.

    rocprofv3 --kernel-trace -d OUT -o k --output-format csv -- python3 bench.py --configs none --no-cpu-baseline
    python tools/kernel_gaps.py OUT/**/k_kernel_trace.csv [--kernels fwd_substring,dcore_substring,finish_substring]

Take the trace alone (no counters, no other tracing).  The step is the cyclic sequence of the kernels named by
`--kernels` (substrings of the kernel names, in launch order; default: the cfg2 bf16 step, `--f32` the float32 one).  For
every pair of dispatches that follow each other in the trace and in the cycle, the gap is start(next) - end(previous); a
pair with any other dispatch in between is not counted.  Prints, per kernel, the number of dispatches and the median /
10th / 90th percentile of its duration, per boundary the same for the gap, and the median period of a whole step
(start of the first kernel to its next start).  Inside a replayed graph the tracer may stamp a kernel's start at the
end of the one before it; the gap then reads 0 and the boundary shows in the duration: compare duration + gap of two
libraries, not either alone."""
import argparse
import csv
import sys

BF16 = "eps_fwd_head_q2reg_t_k,eps_bwd_dcore_q2reg_k,eps_head_reduce_k"
F32 = "eps_fwd_q2f32_k,eps_bwd_q2f32_k,eps_q2f32_finish_k"


def pct(values, q):
    s = sorted(values)
    return s[min(len(s) - 1, int(q * len(s)))]


def row(label, values):
    if not values:
        return f"{label:<44} {0:>7}"
    return f"{label:<44} {len(values):>7} {pct(values, 0.5) / 1e3:>9.2f} {pct(values, 0.1) / 1e3:>9.2f} {pct(values, 0.9) / 1e3:>9.2f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="*_kernel_trace.csv of rocprofv3")
    ap.add_argument("--kernels", default=None, help="substrings of the step's kernel names, in launch order")
    ap.add_argument("--f32", action="store_true", help="the float32 step (eps_q2f32.hip) instead of the bf16 one")
    a = ap.parse_args()
    names = (a.kernels or (F32 if a.f32 else BF16)).split(",")
    events = []   # (start, end, index into names or -1)
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            kind = next((i for i, n in enumerate(names) if n in r["Kernel_Name"]), -1)
            events.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    events.sort()
    n = len(names)
    dur = [[] for _ in names]
    gap = [[] for _ in names]   # gap[i]: behind kernel i, in front of kernel (i + 1) % n
    period, last_first = [], None
    for j, (s, e, k) in enumerate(events):
        if k < 0:
            last_first = None   # a foreign dispatch: the step around it is not a period
            continue
        dur[k].append(e - s)
        if k == 0:
            if last_first is not None:
                period.append(s - last_first)
            last_first = s
        if j + 1 < len(events) and events[j + 1][2] == (k + 1) % n:
            gap[k].append(events[j + 1][0] - e)
    print(f"{'':<44} {'count':>7} {'median':>9} {'p10':>9} {'p90':>9}   (us)")
    for i, name in enumerate(names):
        print(row("kernel " + name, dur[i]))
    for i, name in enumerate(names):
        print(row(f"gap {name[:18]} -> {names[(i + 1) % n][:18]}", gap[i]))
    print(row("step period (first kernel, start to start)", period))
    return 0


if __name__ == "__main__":
    sys.exit(main())
