"""PNG bytes -> one affinely warped tensor (api.png_decode_batch_tensor(..., warp=), api.png_decode_batch_labels(..., warp=))
against the route there was without it, and the warp launch on its own.

Workload: 64 RGB8 files of 512 x 512 (smooth content with noise, 4 distinct images from a fixed seed, repeated) and 64 grey-8
label files of the same size (blocks of 21 classes); every image gets its own matrix: a rotation in +-30 degrees, a scale that
shrinks the 512 x 512 crop by 1.6 .. 2.3 into 224 x 224, a translation of a few pixels, a flip for every second one.

    python tools/bench_png_warp.py [--reps 8 --warmup 2] --out profiles/png_warp.txt

One line per case, the three routes alternating in one process:
    launch: debig_png_warp_kernel / debig_png_label_warp_kernel alone (device events around one launch on resident sources);
    call:   the whole api call (host clock around a call that ends in a device synchronise);
    torch:  the route without the warp call -- png_decode_batch_tensor to a uint8 tensor at crop size (no resize), then torch
            affine_grid + grid_sample (bilinear or nearest, zeros padding, align_corners=False) + normalise (images), or the
            same on png_decode_batch_labels' output as float32 and back to int64 (labels).
The torch route computes in float32, so its elements differ from the integer rule's in the last bits; the line states the
largest difference seen (in units of the output) so that the two routes are known to do the same work."""
import argparse
import ctypes as C
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_FILES, SIDE, N_DISTINCT, CLASSES, OUT = 64, 512, 4, 21, (224, 224)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _png(rows_px, ct):
    import png_spec_ref as R

    rows = np.zeros((SIDE, 1 + rows_px.shape[1]), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = rows_px
    return (R.SIG + R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIDE, SIDE, 8, ct, 0, 0, 0)) +
            R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b""))


def workload():
    rng = np.random.default_rng(20261018)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    imgs, labs = [], []
    for k in range(N_DISTINCT):
        s = ((x[:, :, None] * (3 + k) + y[:, :, None] * 2 + np.arange(3) * 40) // 3 % 256 + rng.integers(0, 9, size=(SIDE, SIDE, 3))) % 256
        imgs.append(_png(s.astype(np.uint8).reshape(SIDE, SIDE * 3), 2))
        blocks = rng.integers(0, CLASSES, size=(SIDE // 32, SIDE // 32), dtype=np.uint8)
        labs.append(_png(np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1), 0))
    return [imgs[i % N_DISTINCT] for i in range(N_FILES)], [labs[i % N_DISTINCT] for i in range(N_FILES)]


def matrices(api):
    rng = np.random.default_rng(7)
    return [api.png_warp_matrix((SIDE, SIDE), OUT, angle=float(rng.uniform(-30, 30)), scale=OUT[0] / SIDE * float(rng.uniform(1.0, 1.4)),
                                translate=(float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8))), hflip=bool(i & 1)) for i in range(N_FILES)]


def theta(ms):
    """the inverse matrices in pixel units -> affine_grid's theta (normalised coordinates, align_corners=False)"""
    H, W = OUT
    t = np.empty((len(ms), 2, 3), np.float32)
    for i, m in enumerate(ms):
        for r, cl in ((0, SIDE), (1, SIDE)):
            a, b, c = m[r]
            t[i, r] = [a * W / cl, b * H / cl, (a * W + b * H + 2 * c) / cl - 1.0]
    return t


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stat(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def _cell(ts):
    med, sp = _stat(ts)
    return "%.3f ms (spread %.1f %%)" % (med, 100 * sp)


def launch_alone(ms, labels, filt, dtype_code, layout, reps, warmup):
    """the warp launch on resident sources: N_FILES images of SIDE x SIDE (RGB8, or one-byte labels) -> OUT; [ms], tasks"""
    import torch
    import png_warp_ref as WR
    from test_emu_png_warp import LabelWarpTask, WarpTask
    from debigulator_amd import _native as N

    L = N.lib()
    L.debig_hip_png_warp_batch.restype = C.c_int
    L.debig_hip_png_warp_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
    L.debig_hip_png_label_warp_batch.restype = C.c_int
    L.debig_hip_png_label_warp_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    e0, e1 = L.debig_hip_event_create(), L.debig_hip_event_create()
    H, W = OUT
    ch = 1 if labels else 3
    es = 8 if labels else (1, 4, 2, 2)[dtype_code]
    run = max(1, 4096 // W)
    tasks = []
    for i, m in enumerate(ms):
        q = WR.quantise([v for r in m for v in r])
        for y0 in range(0, H, run):
            if labels:
                t = LabelWarpTask(src_off=i * SIDE * SIDE, out_off=i * H * W * es, src_pitch=SIDE, crop_w=SIDE, crop_h=SIDE, out_w=W,
                                  out_h=H, row0=y0, rows=min(run, H - y0), border_label=255, src_bytes=1, dtype=3, border_mode=0)
            else:
                chw = layout == "chw"
                t = WarpTask(src_off=i * SIDE * SIDE * 3, out_off=i * H * W * 3 * es, src_pitch=SIDE * 3, crop_w=SIDE, crop_h=SIDE,
                             out_w=W, out_h=H, row0=y0, rows=min(run, H - y0), out_sx=1 if chw else 3, out_sy=W if chw else 3 * W,
                             out_sc=H * W if chw else 1, channels=3, bits=8, dtype=dtype_code, filter=filt, border_mode=0)
                t.a[:] = [1.0 / (255.0 * (1 << 22))] * 4
            t.m[:] = q
            tasks.append(t)
    T = type(tasks[0])
    d_tasks = torch.from_numpy(np.frombuffer(bytes((T * len(tasks))(*tasks)), np.uint8).copy()).cuda()
    src = torch.randint(0, CLASSES if labels else 256, (N_FILES * SIDE * SIDE * ch,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N_FILES * H * W * ch * es, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ts = []
    for r in range(warmup + reps):
        L.debig_hip_event_record(e0, None)
        if labels:
            rc = L.debig_hip_png_label_warp_batch(src.data_ptr(), out.data_ptr(), d_tasks.data_ptr(), None, len(tasks), None)
        else:
            rc = L.debig_hip_png_warp_batch(src.data_ptr(), out.data_ptr(), d_tasks.data_ptr(), len(tasks), None)
        L.debig_hip_event_record(e1, None)
        assert rc == 0, rc
        k = float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)
        if r >= warmup:
            ts.append(k)
    L.debig_hip_event_destroy(e0)
    L.debig_hip_event_destroy(e1)
    return ts, len(tasks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    imgs, labs = workload()
    ms = matrices(api)
    th = torch.from_numpy(theta(ms)).cuda()
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)

    def torch_image(mode):
        st, t, _ = api.png_decode_batch_tensor(imgs, (SIDE, SIDE), mode="rgb", dtype="uint", layout="chw", antialias=False)
        grid = TF.affine_grid(th, (N_FILES, 3) + OUT, align_corners=False)
        x = TF.grid_sample(t.to(torch.float32), grid, mode=mode, padding_mode="zeros", align_corners=False)
        return st, (x / 255.0 - mean) / std

    def torch_labels():
        st, t, _ = api.png_decode_batch_labels(labs, (SIDE, SIDE), dtype="uint8")
        grid = TF.affine_grid(th, (N_FILES, 1) + OUT, align_corners=False)
        x = TF.grid_sample(t.view(N_FILES, 1, SIDE, SIDE).to(torch.float32), grid, mode="nearest", padding_mode="zeros", align_corners=False)
        return st, x[:, 0].to(torch.int64)

    cases = [
        ("rgb8 -> float32 chw, bilinear", False, 0, 1, "chw",
         lambda: api.png_decode_batch_tensor(imgs, OUT, mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD, warp=ms)[:2],
         lambda: torch_image("bilinear")),
        ("rgb8 -> float32 chw, nearest", False, 2, 1, "chw",
         lambda: api.png_decode_batch_tensor(imgs, OUT, mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD, warp=ms, filter="nearest")[:2],
         lambda: torch_image("nearest")),
        ("rgb8 -> bfloat16 hwc, bilinear", False, 0, 3, "hwc",
         lambda: api.png_decode_batch_tensor(imgs, OUT, mode="rgb", dtype="bfloat16", layout="hwc", mean=MEAN, std=STD, warp=ms)[:2], None),
        ("grey-8 labels -> int64", True, 2, 3, "hw",
         lambda: api.png_decode_batch_labels(labs, OUT, dtype="int64", warp=ms)[:2], torch_labels),
    ]
    lines = ["# tools/bench_png_warp.py: %d RGB8 files and %d grey-8 label files of %d x %d (%d distinct each; %.1f + %.1f MiB of files)"
             % (N_FILES, N_FILES, SIDE, SIDE, N_DISTINCT, sum(map(len, imgs)) / 2 ** 20, sum(map(len, labs)) / 2 ** 20),
             "# -> (%d, %d, %d) per image, one matrix per image (rotation +-30 degrees, shrinking 1.6 .. 2.3 x, translation, flips);"
             % ((3,) + OUT),
             "# %d timed runs after %d warm-up runs, routes alternating in one process; spread = (max - min) / median" % (a.reps, a.warmup),
             "# launch = the warp kernel alone on resident sources (device events); call = the whole api call; torch = decode at crop",
             "# size + affine_grid + grid_sample (+ normalise); all three end in a device synchronise.  No LDS-staged variant was built.",
             "# max diff = the largest |call - torch| element (float32 arithmetic against the integer rule; nearest: the share that differs)"]
    for name, labels, filt, dcode, layout, call, other in cases:
        st, t = call()
        assert st == [0] * N_FILES
        diff = "-"
        if other is not None:
            st2, t2 = other()
            assert st2 == [0] * N_FILES and t2.shape == t.shape
            if labels:
                diff = "%.4f %% of picks" % (100.0 * float((t != t2).float().mean()))
            elif filt == 2:  # (another pick moves a normalised sample by at least 1 / (255 * 0.229) = 0.017, or not at all)
                diff = "%.4f %% of elements by more than 0.01" % (100.0 * float(((t.float() - t2.float()).abs() > 0.01).float().mean()))
            else:
                diff = "%.4f" % float((t.float() - t2.float()).abs().max())
        tc, tt = [], []
        for r in range(a.warmup + a.reps):
            x = _timed(call)
            y = _timed(other) if other is not None else None
            if r >= a.warmup:
                tc.append(x)
                if y is not None:
                    tt.append(y)
        tk, n_tasks = launch_alone(ms, labels, filt, dcode, layout, a.reps, a.warmup)
        line = "%-32s launch %s, %d tasks | call %s" % (name, _cell(tk), n_tasks, _cell(tc))
        if tt:
            line += " | torch %s | call / torch %.3f | max diff %s" % (_cell(tt), _stat(tc)[0] / _stat(tt)[0], diff)
        lines.append(line)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
