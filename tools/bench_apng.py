"""APNG batch decode (include/decode_png.h: debig_apng_decode_batch) on the GPU, against the still-image path.

Workload: 64 APNGs of 512 x 512 RGBA8, 8 full-canvas frames each, SOURCE / OVER alternating, photo-like content from a
fixed seed (8 distinct animations, repeated); the same 512 frame streams packaged as 512 standalone PNGs (IHDR + one
IDAT + IEND, the packaging of tests/apng_ref.py).  Both calls inflate, check and de-filter the same 512 streams and
download the same 512 MiB; the APNG call adds one composite pass in HBM.

    python tools/bench_apng.py --role apng  --out-json A.json [--reps 10 --warmup 2]   # apng_decode_batch, 64 files
    python tools/bench_apng.py --role still --out-json S.json                           # png_decode_batch, 512 files
        (DEBIG_LIB=<other libdebigulator_hip.so> runs the still path of another build, e.g. the parent commit's)
    python tools/bench_apng.py --role kernel     # one APNG call + device-to-device copies of the output's byte count,
                                                 # under rocprofv3 --kernel-trace --stats -d DIR -o apng
    python tools/bench_apng.py --report --json S1.json A1.json ... --db DIR/.../apng_results.db --out profiles/apng.txt
"""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_FILES, SIZE, FRAMES, DISTINCT = 64, 512, 8, 8
HBM_PEAK = 8.0e12  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured float4 copy)


def _frame_rgba(rng, seed, k):
    y, x = np.mgrid[0:SIZE, 0:SIZE].astype(np.float32)
    phase = seed * 0.7 + k * 0.35
    img = np.empty((SIZE, SIZE, 4), np.float32)
    img[..., 0] = 128 + 100 * np.sin(x / (37 + seed) + phase) * np.cos(y / 53)
    img[..., 1] = 128 + 90 * np.sin((x + y) / (61 + k) + phase)
    img[..., 2] = 128 + 80 * np.cos(y / (29 + seed) - phase)
    img[..., 3] = np.clip(255 * (0.3 + (x + k * 31) % SIZE / SIZE), 0, 255)  # fractional alpha under OVER
    img[..., :3] += rng.normal(0, 6, size=(SIZE, SIZE, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _stream(rgba):
    from bench_png_spec import _filter_rows

    return zlib.compress(_filter_rows(rgba.reshape(SIZE, -1), 4).tobytes(), 6)


def workload():
    """-> (64 APNG files, 512 standalone PNG files)"""
    import apng_ref as A
    import png_spec_ref as R

    rng = np.random.default_rng(20261016)
    anims, stills = [], []
    for s in range(DISTINCT):
        zs = [_stream(_frame_rgba(rng, s, k)) for k in range(FRAMES)]
        frames = [A.frame(np.zeros((SIZE, SIZE, 4), np.uint8), blend=k % 2) for k in range(FRAMES)]
        anims.append(A.encode(frames, 6, 8, zdata=dict(enumerate(zs))))
        ihdr = R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIZE, SIZE, 8, 6, 0, 0, 0))
        stills.append([R.SIG + ihdr + R.chunk(b"IDAT", z) + R.chunk(b"IEND", b"") for z in zs])
    files = [anims[i % DISTINCT] for i in range(N_FILES)]
    pngs = [p for i in range(N_FILES) for p in stills[i % DISTINCT]]
    return files, pngs


def timed(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["apng", "still", "kernel"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-json")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--json", nargs="*", default=[])
    ap.add_argument("--db", help="the rocprofv3 results database of a --role kernel run")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.report:
        return report(a)
    import torch  # noqa: F401  (torch first: it brings its own HIP runtime)
    from debigulator_amd import api

    files, pngs = workload()
    if a.role == "apng":
        out = api.apng_decode_batch(files)
        assert all(st == 0 for st, _, _ in out)
        ts = timed(lambda: api.apng_decode_batch(files), a.reps, a.warmup)
    elif a.role == "still":
        out = api.png_decode_batch(pngs)
        assert all(st == 0 for st, _, _ in out)
        ts = timed(lambda: api.png_decode_batch(pngs), a.reps, a.warmup)
    else:
        import torch

        out = api.apng_decode_batch(files[:DISTINCT])
        st = api.png_decode_batch(pngs[: FRAMES * DISTINCT])
        for i in range(DISTINCT):  # full-canvas SOURCE frame 0: the still decode of the same stream
            assert np.array_equal(out[i][1][0], st[i * FRAMES][1])
        api.apng_decode_batch(files)
        nbytes = N_FILES * FRAMES * SIZE * SIZE * 4
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        torch.cuda.synchronize()
        print("kernel run done")
        return
    res = {"role": a.role, "lib": os.environ.get("DEBIG_LIB", "tree"), "ms": [1e3 * t for t in ts]}
    print(json.dumps(res))
    if a.out_json:
        with open(a.out_json, "w") as f:
            json.dump(res, f)


def report(a):
    runs = [json.load(open(p)) for p in a.json]
    med = {}
    for r in runs:
        med.setdefault(r["role"], []).append(float(np.median(r["ms"])))
    lines = ["# tools/bench_apng.py: %d APNGs of %d x %d RGBA8, %d full-canvas frames each (SOURCE / OVER alternating), "
             "against the same %d streams as standalone PNGs" % (N_FILES, SIZE, SIZE, FRAMES, N_FILES * FRAMES),
             "# 1. whole call, median of %d calls per run, runs alternating (apng: this tree; still: DEBIG_LIB)"
             % len(runs[0]["ms"])]
    for role in ("apng", "still"):
        v = med.get(role, [])
        lines.append("%-6s runs (ms): %s" % (role, " ".join("%.2f" % x for x in v)))
    if med.get("apng") and med.get("still"):
        ratios = [x / y for x, y in zip(med["apng"], med["still"])]
        spread = lambda v: (max(v) - min(v)) / float(np.median(v))  # noqa: E731
        lines.append("ratio apng / still: median %.3f (per run pair: %s); spread of runs: apng %.1f %%, still %.1f %%"
                     % (float(np.median(ratios)), " ".join("%.3f" % r for r in ratios), 100 * spread(med["apng"]),
                        100 * spread(med["still"])))
    if a.db:
        import sqlite3

        c = sqlite3.connect(a.db)
        rows = list(c.execute("select name, start, duration, grid_x from kernels where name like '%apng_composite%' "
                              "or name like '%copyBuffer%' order by start"))
        comp = [r for r in rows if "apng_composite" in r[0]]
        big = max(comp, key=lambda r: r[3])  # the 64-file call (the first one checks 8 files)
        copies = [r for r in rows if "copyBuffer" in r[0] and r[1] > big[1]]  # the device-to-device copies after it
        nbytes = N_FILES * FRAMES * SIZE * SIZE * 4
        moved = 2 * nbytes  # full-canvas frames: every frame pixel read once, every output byte written once
        kc, kd = float(big[2]), float(np.median([r[2] for r in copies]))
        lines.append("# 2. composite kernel alone (rocprofv3 --kernel-trace, a run of its own), ns")
        lines.append("debig_apng_composite_kernel (64 files, %d workgroups): %d" % (big[3] // 256, big[2]))
        lines.append("device-to-device copy of %d MiB (torch copy_ -> __amd_rocclr_copyBuffer): %s (median %d)"
                     % (nbytes >> 20, " ".join(str(r[2]) for r in copies), kd))
        lines.append("composite / copy: %.3f; composite %.2f TB/s (%d MiB read + written) = %.0f %% of the %.1f TB/s HBM "
                     "peak; the copy %.2f TB/s" % (kc / kd, moved / kc / 1e3, moved >> 20,
                                                   100 * moved / kc / 1e3 / (HBM_PEAK / 1e12), HBM_PEAK / 1e12,
                                                   moved / kd / 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
