#!/usr/bin/env python3
"""Per-way kernel statistics of `rocprofv3 --kernel-trace --stats -- python tools/run_affinity_map.py --sets small --trace --out ""`:
python tools/affinity_trace_summary.py <dir with *_kernel_trace.csv> [reps per way]  ->  the table of profiles/affinity_map_kernels.txt.

The traced process runs, after its warm-up, the batched call `reps` times and then the loop `reps` times.  The batched calls
are found by their own kernels: the last `reps` dispatches of `k_b_bounds` that are followed by no single-build `k_bounds` start
them, the first `k_bounds` after the last `k_b_split_entries` starts the loops.  Per way: dispatches per repetition, their summed
duration, the span from the first start to the last end, and the kernels by summed duration."""
import collections
import csv
import glob
import statistics
import sys


def short(name):
    n = name.replace("(anonymous namespace)::", "").replace("void ", "")
    if "rocprim" in n:
        for key in ("onesweep", "histogram", "block_sort", "merge", "radix_sort", "scan"):
            if key in n:
                return "rocprim " + key
        return "rocprim other"
    return n.split("(")[0][:44]


def main():
    f = glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(open(f))))
    names = [r[2] for r in rows]
    last_split = max(i for i, n in enumerate(names) if n.startswith("k_b_split_entries"))
    loop0 = next(i for i in range(last_split, len(names)) if names[i] == "k_bounds")
    starts = [i for i, n in enumerate(names) if n.startswith("k_b_bounds") and i < loop0]
    batch0 = starts[-reps]
    assert not any(n == "k_bounds" for n in names[batch0:last_split]), "the traced batched calls are not contiguous"
    for way, part in (("one build_affinity_batch call", rows[batch0:last_split + 1]), ("the loop of build_affinity calls", rows[loop0:])):
        tot = collections.defaultdict(list)
        for s, e, n in part:
            tot[n].append((e - s) / 1e3)
        busy = sum(sum(v) for v in tot.values())
        print(f"{way}: {len(part) / reps:.1f} kernel dispatches per repetition, {busy / reps:.1f} us of kernels per repetition, "
              f"{(part[-1][1] - part[0][0]) / 1e3 / reps:.1f} us from first start to last end per repetition ({reps} repetitions)")
        print(f"  {'kernel':<46}{'calls/rep':>10}{'sum us/rep':>12}{'median us':>11}")
        for n, v in sorted(tot.items(), key=lambda kv: -sum(kv[1])):
            print(f"  {n:<46}{len(v) / reps:>10.1f}{sum(v) / reps:>12.1f}{statistics.median(v):>11.2f}")


if __name__ == "__main__":
    main()
