"""PNG bytes -> one resized, normalised tensor (api.png_decode_batch_tensor) against the route without it.

Workload: 256 PNG files of mixed sizes around 1024 x 1024 (8 distinct images from a fixed seed -- six RGB8, two RGBA16 --
repeated), photo-like content, -> (256, 3, 224, 224) float32, ImageNet mean / std, antialias on.

    python tools/bench_png_tensor.py --role call [--reps 8 --warmup 2] --out-json T.json
        the two routes alternating in one process, a device synchronise inside every timed call:
          tensor: api.png_decode_batch_tensor
          torch:  api.png_decode_batch_device(layout="chw") -> per image torch.nn.functional.interpolate(antialias=True)
                  on the GPU -> normalise -> torch.stack   (what a caller does without the new call)
    python tools/bench_png_tensor.py --role kernel
        one tensor call + device-to-device copies of the bytes the resize kernel must move (crop bytes read + tensor bytes
        written); run it under  rocprofv3 --kernel-trace --stats -d DIR -o tensor -- python tools/bench_png_tensor.py ...
    python tools/bench_png_tensor.py --report --json T.json [--db DIR/.../tensor_results.db] --out profiles/png_tensor.txt
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

N_FILES, OUT = 256, (224, 224)
SHAPES = [(1024, 1024, 2, 8), (960, 1152, 2, 8), (1152, 896, 2, 8), (1000, 1000, 2, 8), (1100, 940, 2, 8), (900, 1200, 2, 8),
          (1024, 1024, 6, 16), (896, 1088, 6, 16)]  # (h, w, colour type, depth)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _png(rng, k, h, w, ct, depth):
    import png_spec_ref as R

    ch = 3 if ct == 2 else 4
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, ch), np.float32)
    for c in range(ch):
        img[..., c] = 0.5 + 0.4 * np.sin(x / (31 + 7 * c + k) + 0.6 * k) * np.cos(y / (47 + 5 * c) - 0.3 * c)
    img += rng.normal(0, 0.02, size=img.shape)
    full = (1 << depth) - 1
    s = np.clip(img * full, 0, full).astype(np.uint8 if depth == 8 else ">u2")
    rows = np.zeros((h, 1 + w * ch * depth // 8), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = s.reshape(h, -1).view(np.uint8)
    ihdr = R.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, 0))
    return R.SIG + ihdr + R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b"")


def workload():
    rng = np.random.default_rng(20261016)
    distinct = [_png(rng, k, *s) for k, s in enumerate(SHAPES)]
    return [distinct[i % len(distinct)] for i in range(N_FILES)], [SHAPES[i % len(SHAPES)] for i in range(N_FILES)]


def route_tensor(api, files):
    st, t, _ = api.png_decode_batch_tensor(files, OUT, mode="rgb", depth=8, dtype="float32", layout="chw", mean=MEAN, std=STD)
    return st, t


def route_torch(api, files):
    import torch
    import torch.nn.functional as F

    out = api.png_decode_batch_device(files, mode="rgb", depth=8, layout="chw")
    mean = torch.tensor(MEAN, device="cuda").view(3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(3, 1, 1)
    imgs = [F.interpolate(t[None].float(), size=OUT, mode="bilinear", align_corners=False, antialias=True)[0] for _, t, _ in out]
    return [s for s, _, _ in out], (torch.stack(imgs) / 255.0 - mean) / std


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", choices=["call", "kernel"])
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-json")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--db", help="the rocprofv3 results database of a --role kernel run")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.report:
        return report(a)
    import torch
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    files, shapes = workload()
    if a.role == "kernel":
        st, t = route_tensor(api, files)
        assert st == [0] * N_FILES
        nbytes = sum(h * w * 3 for h, w, _, _ in shapes) + t.numel() * 4  # RGB8 crops read + float32 tensor written
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)  # a copy of nbytes / 2 moves nbytes
        torch.cuda.synchronize()
        print("kernel run done: %d bytes" % nbytes)
        return
    sa, ta = route_tensor(api, files)
    sb, tb = route_torch(api, files)
    assert sa == sb == [0] * N_FILES and ta.shape == tb.shape == (N_FILES, 3) + OUT
    diff = float((ta - tb).abs().max())  # Q14 weights against torch's float32 weights, on the normalised scale (1 / std ~ 4.4)
    ts = {"tensor": [], "torch": []}
    for r in range(a.warmup + a.reps):
        for name, fn in (("tensor", route_tensor), ("torch", route_torch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(api, files)
            torch.cuda.synchronize()
            if r >= a.warmup:
                ts[name].append(1e3 * (time.perf_counter() - t0))
    res = {"ms": ts, "max_abs_diff": diff, "file_mib": sum(len(f) for f in files) / 2 ** 20,
           "decoded_mib": sum(h * w * 3 for h, w, _, _ in shapes) / 2 ** 20}
    print(json.dumps(res))
    if a.out_json:
        with open(a.out_json, "w") as f:
            json.dump(res, f)


def report(a):
    r = json.load(open(a.json))
    files, shapes = N_FILES, SHAPES
    med = {k: float(np.median(v)) for k, v in r["ms"].items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in r["ms"].items()}
    lines = ["# tools/bench_png_tensor.py: %d PNG files (%d distinct, sizes %s; %.0f MiB of files, %.0f MiB as RGB8) -> "
             "(%d, 3, %d, %d) float32, mean / std, antialias on" % (files, len(shapes), " ".join("%dx%d/%s%d" % (w, h, "RGB" if ct == 2 else "RGBA", d)
                                                                                                for h, w, ct, d in shapes),
                                                                    r["file_mib"], r["decoded_mib"], files, OUT[0], OUT[1]),
             "# 1. whole call, the two routes alternating in one process, %d timed calls each after warm-up, a device synchronise"
             % len(r["ms"]["tensor"]),
             "#    inside every timed call.  tensor: api.png_decode_batch_tensor.  torch: api.png_decode_batch_device(layout=\"chw\")",
             "#    -> per image torch.nn.functional.interpolate(antialias=True) -> normalise -> torch.stack (the route without the call)."]
    for k in ("tensor", "torch"):
        lines.append("%-6s calls (ms): %s | median %.2f, spread (max - min) / median %.1f %%"
                     % (k, " ".join("%.2f" % x for x in r["ms"][k]), med[k], 100 * spread[k]))
    lines.append("ratio tensor / torch: %.3f (medians); largest |difference| of the two results on the normalised scale: %.2e"
                 % (med["tensor"] / med["torch"], r["max_abs_diff"]))
    if a.db:
        import sqlite3

        c = sqlite3.connect(a.db)
        rows = list(c.execute("select name, start, duration, grid_x from kernels where name like '%png_resize%' "
                              "or name like '%copyBuffer%' order by start"))
        k = [x for x in rows if "png_resize" in x[0]][-1]
        copies = [x for x in rows if "copyBuffer" in x[0] and x[1] > k[1]]
        nbytes = sum(h * w * 3 for h, w, _, _ in [SHAPES[i % len(SHAPES)] for i in range(N_FILES)]) + N_FILES * 3 * OUT[0] * OUT[1] * 4
        kd = float(np.median([x[2] for x in copies]))
        lines.append("# 2. resize kernel alone (rocprofv3 --kernel-trace, a run of its own), ns; scale ~4.6: 10 - 11 taps per axis")
        lines.append("debig_png_resize_kernel (%d workgroups): %d" % (k[3] // 256, k[2]))
        lines.append("device-to-device copy moving the same %d MiB (crops read + tensor written): %s (median %d)"
                     % (nbytes >> 20, " ".join(str(x[2]) for x in copies), kd))
        lines.append("resize / copy: %.2f; the resize moves its bytes at %.2f TB/s, the copy at %.2f TB/s.  The share of pass-1 "
                     "arithmetic against memory is not named: no counter run was made." % (k[2] / kd, nbytes / k[2] / 1e3, nbytes / kd / 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
