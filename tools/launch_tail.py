#!/usr/bin/env python3
"""The slow tail of one kernel's launches in a rocprofv3 --kernel-trace directory: the
median, the launches longer than twice a reference median (default: the trace's own), their
durations grouped by size, the sum of their excess over the median per step, and the
launches between 1.2 and 2 times the reference.

usage: tools/launch_tail.py <trace dir> <kernel name prefix> <steps in the trace> [reference median us]
"""
import collections
import csv
import glob
import statistics
import sys

trace, prefix, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
files = sorted(glob.glob(f"{trace}/**/*kernel_trace.csv", recursive=True))
if len(files) != 1:
    sys.exit(f"expected one kernel trace under {trace}, found {len(files)}")
dur = []
with open(files[0]) as fh:
    for r in csv.DictReader(fh):
        n = r["Kernel_Name"].replace("void ", "").replace("admmq::", "")
        if n.startswith(prefix):
            dur.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
med = statistics.median(dur)
ref = float(sys.argv[4]) if len(sys.argv) > 4 else med
mean = sum(dur) / len(dur)
sd = statistics.pstdev(dur)
slow = sorted(d for d in dur if d > 2 * ref)
excess = sum(d - med for d in slow)
print(f"kernel {prefix}: {len(dur)} launches in {steps} steps")
print(f"median {med:.1f} us, mean {mean:.2f} us, sigma {sd:.2f} us, min {min(dur):.1f} us, max {max(dur):.1f} us")
print(f"launches longer than 2 x {ref:.1f} us: {len(slow)} ({len(slow) / steps:.1f} per step)")
print(f"sum of their excess over the median: {excess / 1e3:.3f} ms = {excess / 1e3 / steps:.3f} ms per step")
# grouped by duration: bins of a quarter octave
bins = collections.Counter()
for d in slow:
    b = 0
    while ref * 2 ** ((b + 1) / 4) <= d:
        b += 1
    bins[b] += 1
for b in sorted(bins):
    lo, hi = ref * 2 ** (b / 4), ref * 2 ** ((b + 1) / 4)
    print(f"  {lo:7.1f} .. {hi:7.1f} us: {bins[b]:4d}")
print("durations (us): " + " ".join(f"{d:.0f}" for d in slow))
mid = sorted(d for d in dur if 1.2 * ref < d <= 2 * ref)
print(f"launches between 1.2 x and 2 x {ref:.1f} us: {len(mid)} ({len(mid) / steps:.1f} per step), "
      f"excess over the median {sum(d - med for d in mid) / 1e3 / steps:.3f} ms per step")
print("durations (us): " + " ".join(f"{d:.1f}" for d in mid))
