#!/usr/bin/env python3
"""One step boundary of bench.py from a rocprofv3 kernel trace (--kernel-trace --output-format csv): every kernel that runs from
1.5 ms before a step's first k_pyramid_batch<u8> to 0.9 ms behind its end, times in microseconds relative to that launch's start,
with the hardware queue and the grid; then the step periods (between the ends of successive k_write_out launches; a batch that
runs as two parts has two per step) and the per-kernel totals over the steps behind the warm-up.

    rocprofv3 --kernel-trace -d <dir> --output-format csv -- python bench.py --steps 10 --warmup 3
    python tools/step_boundary.py <dir> [<dir> ...]
"""
import collections
import csv
import glob
import os
import sys


def load(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    out = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0][:58], int(r["Queue_Id"]), int(r["Grid_Size_X"]))
           for r in csv.DictReader(open(f))]
    out.sort()
    return out


def main(dirs):
    for d in dirs:
        k = load(d)
        pyr = [i for i, r in enumerate(k) if "k_pyramid_batch<unsigned char" in r[2]]
        print("%s: %d kernels, %d steps" % (d, len(k), len(pyr)))
        if len(pyr) < 6:
            continue
        b = k[pyr[-3]]
        for r in k:
            if r[1] >= b[0] - 1500000 and r[0] <= b[1] + 900000:
                print("  %9.1f %9.1f  %8.1f us  q%-2d grid %-8d %s" % ((r[0] - b[0]) / 1e3, (r[1] - b[0]) / 1e3, (r[1] - r[0]) / 1e3, r[3], r[4], r[2]))
        ends = [r[1] for r in k if "k_write_out" in r[2]]
        print("  periods between k_write_out ends (ms):", " ".join("%.3f" % ((ends[i + 1] - ends[i]) / 1e6) for i in range(len(ends) - 1)))
        tot, cnt = collections.defaultdict(float), collections.Counter()
        for r in k:
            if r[0] >= k[pyr[3]][0]:
                tot[r[2]] += (r[1] - r[0]) / 1e6
                cnt[r[2]] += 1
        for n, v in sorted(tot.items(), key=lambda x: -x[1])[:10]:
            print("  %-58s %9.3f ms %5d launches" % (n, v, cnt[n]))


if __name__ == "__main__":
    main(sys.argv[1:])
