"""Output formats of debig_png_decode_batch_fmt (include/decode_png.h) per source format, on the GPU.

    python tools/bench_png_out_formats.py [--n 64] [--size 1024] [--reps 5] [--out FILE] [--manifest FILE]
    rocprofv3 --kernel-trace -d DIR -o run -- python tools/bench_png_out_formats.py --reps 3 --manifest M.json
    python tools/bench_png_out_formats.py --summarize M.json --trace DIR [--out FILE]

The source formats of tools/bench_png_spec.py, each decoded to RGBA8, RGB8, GRAY8, NATIVE (8-bit) and NATIVE-depth,
every image through the general path (DEBIG_PNG_FORCE_GENERAL): ms per whole batch call (files in host memory ->
pixels in host memory), the median of --reps after one warm-up call, and GB/s of pixels produced.  The de-filter
kernel alone comes from a kernel trace: with --manifest the run records how many calls each (source, output) pair made
in order; every call launches exactly one general de-filter kernel (debig_png_spec_defilter_kernel for RGBA8,
debig_png_spec_defilter_fmt_kernel otherwise), so --summarize maps the trace's dispatches back to the pairs and prints
the median kernel time of each, and its ratio to the RGBA8 kernel time of the same source files.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUTPUTS = [("rgba8", "rgba", 8), ("rgb8", "rgb", 8), ("gray8", "gray", 8), ("native", "native", 8),
           ("native-depth", "native", "native")]
KERNELS = ("debig_png_spec_defilter_kernel", "debig_png_spec_defilter_fmt_kernel")


def sources(size):
    """[(name, distinct files)]: the formats of tools/bench_png_spec.py except its routing variants of RGBA8"""
    import bench_png_spec as B

    rng = np.random.default_rng(1)
    out = []
    for name, ct, depth, il, trns, general in B.FORMATS:
        if name in ("rgba8 tuned", "rgba8 general"):
            name = "rgba8"
            if general:
                continue
        files = []
        for k in range(4):
            s = B._image(rng, size, ct, depth, k)
            pal = t = None
            if ct == 3:
                pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(1 << depth)]
                t = bytes(rng.integers(0, 256, size=(1 << depth) // 2, dtype=np.uint8))
            files.append(B.encode_fast(s, ct, depth, il, t, pal))
        out.append((name, files))
    return out


def run(a):
    import torch
    from debigulator_amd import api

    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.cuda.get_device_name(0)
    lines = ["# tools/bench_png_out_formats.py --n %d --size %d --reps %d (%s), every image through the general path"
             % (a.n, a.size, a.reps, dev),
             "# whole batch call: median ms over reps after one warm-up call; GB/s of output pixels",
             "# %-14s %-13s %10s %10s %12s" % ("source", "output", "ms/batch", "GB/s", "MB out/batch")]
    manifest = {"device": dev, "n": a.n, "size": a.size, "calls": []}
    for sname, distinct in sources(a.size):
        files = [distinct[k % 4] for k in range(a.n)]
        for oname, mode, depth in OUTPUTS:
            out = api.png_decode_batch(files, force_general=True, mode=mode, depth=depth)  # warm-up
            assert all(st == 0 for st, _, _ in out), (sname, oname)
            nbytes = sum(px.nbytes for _, px, _ in out)
            del out
            times = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                api.png_decode_batch(files, force_general=True, mode=mode, depth=depth)
                times.append(time.perf_counter() - t0)
            ms = 1e3 * float(np.median(times))
            lines.append("  %-14s %-13s %10.2f %10.2f %12.1f" % (sname, oname, ms, nbytes / (ms * 1e-3) / 1e9, nbytes / 1e6))
            print(lines[-1], flush=True)
            manifest["calls"].append([sname, oname, 1 + a.reps])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.manifest:
        with open(a.manifest, "w") as f:
            json.dump(manifest, f)


def _dispatches(trace_dir):
    """[(kernel name, start ns, end ns, vgprs, scratch bytes)] of the two de-filter kernels, in start order, from the
    rocprofv3 output under trace_dir (its database, or the CSV of --output-format csv)"""
    dbs = glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True)
    rows = []
    if dbs:
        import sqlite3

        assert len(dbs) == 1, dbs
        c = sqlite3.connect(dbs[0])
        for name, st, en, vg, sc in c.execute("select name, start, end, vgpr_count, scratch_size from kernels"):
            rows.append((name.split("(")[0].strip(), int(st), int(en), int(vg), int(sc)))
    else:
        paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
        assert len(paths) == 1, paths
        for r in csv.DictReader(open(paths[0])):
            rows.append((r["Kernel_Name"].split("(")[0].strip(), int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         int(r.get("VGPR_Count", -1)), int(r.get("Scratch_Size", -1))))
    return sorted((r for r in rows if r[0] in KERNELS), key=lambda r: r[1])


def summarize(a):
    man = json.load(open(a.manifest))
    rows = _dispatches(a.trace)
    want = sum(c for _, _, c in man["calls"])
    assert len(rows) == want, (len(rows), want)
    lines = ["# de-filter kernel alone (rocprofv3 --kernel-trace), %d x %d^2 images per call (%s)"
             % (man["n"], man["size"], man["device"]),
             "# median over the calls after the warm-up; ratio: to the RGBA8 kernel on the same source files",
             "# %-14s %-13s %-36s %10s %8s" % ("source", "output", "kernel", "us", "ratio")]
    i = 0
    base = {}
    res = {}
    for sname, oname, calls in man["calls"]:
        rs = rows[i: i + calls]
        i += calls
        us = float(np.median([(r[2] - r[1]) / 1e3 for r in rs[1:]]))
        if oname == "rgba8":
            base[sname] = us
        res[rs[-1][0]] = rs[-1][3:]
        lines.append("  %-14s %-13s %-36s %10.1f %8.2f" % (sname, oname, rs[-1][0], us, us / base[sname]))
        print(lines[-1])
    for k, (vg, sc) in sorted(res.items()):
        lines.append("# %s: %d VGPRs, %d bytes of scratch per lane (from the trace)" % (k, vg, sc))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--manifest", default=None)
    ap.add_argument("--summarize", action="store_true")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)


if __name__ == "__main__":
    main()
