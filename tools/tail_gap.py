#!/usr/bin/env python3
"""The chain's tail in a rocprofv3 kernel trace: python tools/tail_gap.py <dir with *_kernel_trace.csv> [skip_fraction=0.3]
For the steady-state part of the run, per K5 launch (fir_block_kernel) the gap between the end of the peak search
(row_first_peak_chunked_kernel) queued just before it on the same stream and K5's start, and the two kernels' durations
(median / mean / p90, microseconds)."""
import csv
import glob
import os
import statistics
import sys
from collections import defaultdict


def stats(xs):
    xs = sorted(xs)
    if not xs:
        return "n/a"
    return (f"n {len(xs):5d}  median {statistics.median(xs):7.1f}  mean {statistics.fmean(xs):7.1f}  "
            f"p90 {xs[int(0.9 * (len(xs) - 1))]:7.1f}")


def main(root, skip=0.3):
    ev = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Stream_Id"],
                       int(r["Workgroup_Size_X"])))
    ev.sort()
    t_lo = ev[0][0] + skip * (ev[-1][1] - ev[0][0])
    by_stream = defaultdict(list)
    for e in ev:
        by_stream[e[3]].append(e)
    gap, k5, peak = [], defaultdict(list), []
    for evs in by_stream.values():
        last_peak = None
        for s, e, name, _, wg in evs:
            if "row_first_peak_chunked_kernel" in name:
                last_peak = (s, e)
            elif "fir_block_kernel" in name and s >= t_lo:
                k5[wg].append((e - s) / 1e3)
                if last_peak is not None:
                    gap.append((s - last_peak[1]) / 1e3)
                    peak.append((last_peak[1] - last_peak[0]) / 1e3)
                last_peak = None
    print(f"peak search end -> K5 start: {stats(gap)}")
    print(f"peak search duration:        {stats(peak)}")
    for wg, d in sorted(k5.items()):
        print(f"K5 ({wg:4d} threads) duration: {stats(d)}")


if __name__ == "__main__":
    main(sys.argv[1], float(sys.argv[2]) if len(sys.argv) > 2 else 0.3)
