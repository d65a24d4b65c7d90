#!/usr/bin/env python3
"""What lies between the end of one sparse_align_kernel and the start of the next, from a rocprofv3 trace of bench.py:

  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o NAME -- python bench.py
  scripts/align_gap_timeline.py DIR/**/NAME_kernel_trace.csv DIR/**/NAME_memory_copy_trace.csv [n_gaps_listed]
  scripts/align_gap_timeline.py DIR/**/NAME_kernel_trace.csv - [n_gaps_listed]        (a pass with --kernel-trace alone)

For every pair of consecutive alignment kernels less than 2 ms apart (the steps of one queue): the idle time between them, and every
other kernel and every copy that runs in it or ends in it, with its duration and where it starts relative to the first kernel's end.
Then the medians over the steady-state gaps, and where the copies of a step ran relative to the kernels (inside a gap or beside a
kernel).  Last, every alignment kernel's begin and end, counted from the first one's begin, and how far its begin lies from the end
of the kernel before it: negative where the launch lanes (csrc/svoh_internal.h) start a kernel in the tail of the one before.
Times in microseconds."""
import csv
import statistics
import sys


def rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def col(r, *names):
    for n in names:
        if n in r and r[n] != "":
            return r[n]
    return ""


def kernel_timeline(align, n_list):
    """begin and end of the alignment kernels of the last queue (consecutive kernels less than 2 ms apart), and of the n_list before"""
    queue = [align[-1]]
    for k in reversed(align[:-1]):
        if queue[0][0] - k[1] > 2e6:
            break
        queue.insert(0, k)
    t0 = queue[0][0]
    print("alignment kernels of the last queue (%d): begin, end (us from the first one's begin), duration, begin - end of the kernel before" % len(queue))
    starts_inside = 0
    for i, k in enumerate(queue):
        d = (k[0] - queue[i - 1][1]) / 1e3 if i else 0.0
        starts_inside += 1 if i and d < 0 else 0
        if i < n_list or i >= len(queue) - n_list:
            print("    #%-3d begin %10.1f  end %10.1f  duration %8.1f  %s" % (i, (k[0] - t0) / 1e3, (k[1] - t0) / 1e3, (k[1] - k[0]) / 1e3,
                                                                              ("begin - previous end %+8.1f" % d) if i else ""))
    if len(queue) > 1:
        d_all = [(b[0] - a[1]) / 1e3 for a, b in zip(queue, queue[1:])]
        print("    kernels that begin before the kernel before them has ended: %d of %d;  begin - previous end: median %+.1f us, min %+.1f, max %+.1f"
              % (starts_inside, len(queue) - 1, statistics.median(d_all), min(d_all), max(d_all)))
        print("    the queue: %.1f us from the first begin to the last end, %.1f us per kernel" % ((queue[-1][1] - t0) / 1e3, (queue[-1][1] - t0) / 1e3 / len(queue)))


def main(kernel_csv, copy_csv, n_list=6):
    ks = [(int(col(r, "Start_Timestamp")), int(col(r, "End_Timestamp")), col(r, "Kernel_Name")) for r in rows(kernel_csv)]
    cs = [(int(col(r, "Start_Timestamp")), int(col(r, "End_Timestamp")),
           "copy %s%s" % (col(r, "Direction").replace("MEMORY_COPY_", ""), (" %s B" % col(r, "Bytes", "Size")) if col(r, "Bytes", "Size") else ""))
          for r in (rows(copy_csv) if copy_csv != "-" else [])]
    align = sorted(k for k in ks if "sparse_align_kernel" in k[2])
    others = sorted([k for k in ks if "sparse_align_kernel" not in k[2]] + cs)
    print("%d alignment kernels, %d other kernels, %d copies" % (len(align), len(ks) - len(align), len(cs)))
    gaps = []
    for a, b in zip(align, align[1:]):
        idle = (b[0] - a[1]) / 1e3
        if idle > 2000.0:
            continue
        inside = [(o[0], o[1], o[2]) for o in others if o[1] > a[1] and o[0] < b[0]]
        gaps.append((idle, a, b, inside))
    if not gaps:
        print("no consecutive alignment kernels found")
        return
    kernel_timeline(align, n_list)
    for idle, a, b, inside in gaps[-n_list:]:
        print("gap %8.1f us   (kernel before %.1f us, after %.1f us)" % (idle, (a[1] - a[0]) / 1e3, (b[1] - b[0]) / 1e3))
        t = a[1]
        for s, e, name in inside:
            print("    +%7.1f us  %7.1f us  %s%s" % ((s - a[1]) / 1e3, (e - s) / 1e3, name[:70], "   (started beside the kernel before)" if s < a[1] else ""))
            t = max(t, e)
        if inside:
            print("    idle behind the last of them: %.1f us" % ((b[0] - t) / 1e3))
    idles = [g[0] for g in gaps]
    busy = [sum((min(e, g[2][0]) - max(s, g[1][1])) for s, e, _ in g[3]) / 1e3 for g in gaps]
    print("gaps: %d   median %.1f us   mean %.1f   min %.1f   max %.1f;   of the median gap, copies and other kernels fill %.1f us"
          % (len(idles), statistics.median(idles), statistics.mean(idles), min(idles), max(idles), statistics.median(busy)))
    # where the copies ran: wholly beside an alignment kernel, or not
    first, last = align[0][0], align[-1][1]
    beside = sum(1 for s, e, _ in cs if any(k[0] <= s and e <= k[1] for k in align))
    in_window = sum(1 for s, e, _ in cs if s >= first and e <= last)
    print("copies between the first and the last alignment kernel: %d, of them wholly beside a running alignment kernel: %d" % (in_window, beside))
    print("alignment kernel: median %.1f us" % statistics.median((k[1] - k[0]) / 1e3 for k in align))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 6)
