#!/usr/bin/env python3
"""The alignment kernel's patch loops by instruction class, block by block, and the kernel's registers, scratch and
static LDS -- for several kernels of one assembly file (cross-compiled as scripts/isa_loop_census.sh does; no GPU needed).

  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S svo_pro_universal_amd/csrc/sparse_align.hip -o k.s
  scripts/isa_align_blocks.py k.s sparse_align_kernelILi4ELi128ELb0E sparse_align_kernelILi4ELi256ELb0ELb0ELb0ELi1ELb0ELb0E ...

Every block inside a loop with at least MIN_F64 (20) fp64 instructions is listed: the pixel blocks are the ones with
conversions (cvt) and byte reads, the others are the projection and the Jacobian rows with the map to the normal equations.
"fp64 outside the pixel blocks" is the sum over the listed blocks without a conversion from an integer."""
import collections
import re
import sys

MIN_F64 = 20
lines = open(sys.argv[1]).read().splitlines()


def kind(t):
    op = t.split()[0]
    if op.startswith("v_cvt"): return "cvt"
    if "f64" in op: return "fp64"
    if op.startswith("ds_"): return "ds"
    if op.startswith(("global_", "buffer_", "flat_")): return "vmem"
    if op.startswith("scratch_"): return "scratch"
    if op.startswith("s_"): return "salu"
    if op.startswith("v_"): return "valu_other"
    return "other"


cols = ["fp64", "cvt", "ds", "vmem", "scratch", "salu", "valu_other"]
for pat in sys.argv[2:]:
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(pat) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    name = lines[start].rstrip(":")
    blocks, cur = [], None
    for l in lines[start:end]:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
        if m:
            d = re.search(r"Depth=(\d+)", l)
            cur = dict(name=m.group(1), depth=int(d.group(1)) if d else 0, c=collections.Counter())
            blocks.append(cur)
            continue
        t = l.strip()
        if cur is None or not t or t.startswith(";") or t.startswith("."):
            continue
        cur["c"][kind(t)] += 1
    res = {}
    for l in lines[end:]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)", l)
        if m:
            res[m.group(1)] = int(m.group(2))
        if ".end_amdhsa_kernel" in l:
            break
    print("%s" % name)
    print("  registers (arch + acc) %d, scratch %d B, static LDS %d B" %
          (res.get("next_free_vgpr", -1), res.get("private_segment_fixed_size", -1), res.get("group_segment_fixed_size", -1)))
    print("  %-12s %5s %6s | " % ("block", "depth", "total") + " ".join("%10s" % c for c in cols))
    outside = pixel = 0
    for b in blocks:
        if b["depth"] < 1 or b["c"]["fp64"] < MIN_F64:
            continue
        is_pixel = b["c"]["cvt"] >= 8
        if is_pixel: pixel += b["c"]["fp64"]
        else: outside += b["c"]["fp64"]
        print("  %-12s %5d %6d | " % (b["name"], b["depth"], sum(b["c"].values())) + " ".join("%10d" % b["c"][c] for c in cols) +
              ("   pixel block" if is_pixel else ""))
    tot = collections.Counter()
    for b in blocks:
        tot.update(b["c"])
    print("  %-12s %5s %6d | " % ("whole kernel", "", sum(tot.values())) + " ".join("%10d" % tot[c] for c in cols))
    print("  fp64 in the listed blocks: %d in pixel blocks, %d outside them" % (pixel, outside))
    print()
