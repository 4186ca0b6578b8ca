"""Transparent PNG bytes -> one tensor composited over a background (api.png_decode_batch_tensor(alpha="over")) against the
route without it, and the alpha resize kernel against the plain one.

Workload: 64 PNG files of 1024 x 1024 RGBA8, and 64 of RGBA16 (4 distinct images each from a fixed seed, repeated; smooth
colour, alpha with fully transparent, fully opaque and graded regions) -> (64, 3, 224, 224) float32 and (64, 3, 512, 512)
bfloat16, white background, antialias on, no mean / std.

    python tools/bench_png_tensor_alpha.py [--reps 8 --warmup 2] --out profiles/png_tensor_alpha.txt
        1. whole call, the two routes alternating in one process, a device synchronise inside every timed call:
             over:     api.png_decode_batch_tensor(mode="rgb", alpha="over")
             two-step: api.png_decode_batch_tensor(mode="rgba") -> rgb * a + background * (1 - a) in torch on the device
                       (what a caller does without the new call; it filters STRAIGHT alpha, so its pixels differ)
        2. the resize kernels alone on the SAME tile lists (device events around one launch each, after a warm-up launch):
             debig_png_resize_kernel (RGBA in, 4 channels out), debig_png_resize_alpha_kernel OVER (3 out) and
             PREMULTIPLIED (4 out), from random pixels in device memory
"""
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

N_FILES, SIDE, N_DISTINCT = 64, 1024, 4
TARGETS = [((224, 224), "float32"), ((512, 512), "bfloat16")]
BG = (1.0, 1.0, 1.0)


def _png(rng, k, depth):
    import png_spec_ref as R

    h = w = SIDE
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, 4), np.float32)
    for c in range(3):
        img[..., c] = 0.5 + 0.4 * np.sin(x / (31 + 7 * c + k) + 0.6 * k) * np.cos(y / (47 + 5 * c) - 0.3 * c)
    img[..., :3] += rng.normal(0, 0.02, size=(h, w, 3))
    img[..., 3] = np.clip(0.5 + 1.5 * np.sin(x / (90 + 11 * k)) * np.cos(y / (70 + 13 * k)), 0, 1)  # 0, 1 and grades between
    full = (1 << depth) - 1
    s = np.clip(img * full, 0, full).astype(np.uint8 if depth == 8 else ">u2")
    rows = np.zeros((h, 1 + w * 4 * depth // 8), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = s.reshape(h, -1).view(np.uint8)
    ihdr = R.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 6, 0, 0, 0))
    return R.SIG + ihdr + R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b"")


def workload(depth):
    rng = np.random.default_rng(20261017 + depth)
    distinct = [_png(rng, k, depth) for k in range(N_DISTINCT)]
    return [distinct[i % N_DISTINCT] for i in range(N_FILES)]


def route_over(api, files, size, depth, dtype):
    return api.png_decode_batch_tensor(files, size, mode="rgb", depth=depth, dtype=dtype, alpha="over", background=BG)[:2]


def route_two_step(api, files, size, depth, dtype):
    import torch

    st, t, _ = api.png_decode_batch_tensor(files, size, mode="rgba", depth=depth, dtype=dtype)
    bg = torch.tensor(BG, device=t.device, dtype=t.dtype).view(1, 3, 1, 1)
    a = t[:, 3:]
    return st, t[:, :3] * a + bg * (1 - a)


def _timed(fn, reps, warmup):
    import torch

    ts = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def _stat(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def tile_lists(depth, size, dtype_name):
    """the task lists of the three launches on the same tiles (the host's tile rule at 4 source channels) ->
    {name: (struct, out channels, tasks)}, the axis table's bytes, element size"""
    import png_resize_ref as Z
    from test_emu_png_resize import HQ_CAP, TILE_W, WX_CAP, Task, axis_table
    from test_emu_png_resize_alpha import AlphaTask

    H, W = size
    Sc, sb = 4, depth // 8
    dtype = Z.DTYPES[dtype_name]
    es = {Z.T_F32: 4, Z.T_BF16: 2}[dtype]
    tb, ent, mt = axis_table(SIDE, W, True)
    assert (H, W) == (W, W)  # one table serves both axes
    tw = min(W, TILE_W, WX_CAP // mt, HQ_CAP // (mt * Sc))
    img_bytes = SIDE * SIDE * Sc * sb
    a, b = Z.affine(depth, (1, 1, 1, 1), (0, 0, 0, 0))
    lists = {}
    for name, cls, oc, mode in (("plain", Task, 4, 0), ("over", AlphaTask, 3, 2), ("premultiplied", AlphaTask, 4, 1)):
        tasks = []
        for i in range(N_FILES):
            y0 = 0
            while y0 < H:
                lo, hi, th = ent[y0][0], sum(ent[y0]), 1
                while y0 + th < H and th < 64:
                    f, e = ent[y0 + th][0], sum(ent[y0 + th])
                    if (max(hi, e) - min(lo, f)) * tw * Sc > HQ_CAP:
                        break
                    lo, hi, th = min(lo, f), max(hi, e), th + 1
                for x0 in range(0, W, tw):
                    t = cls(src_off=i * img_bytes, out_off=i * H * W * oc * es, wx_off=0, wy_off=0, src_pitch=SIDE * Sc, tile_x=x0,
                            tile_y=y0, tile_w=min(tw, W - x0), tile_h=th, src_y0=lo, src_rows=hi - lo, out_sx=1, out_sy=W,
                            out_sc=H * W, channels=Sc, bits=depth, dtype=dtype)
                    t.a, t.b = (C.c_float * 4)(*a), (C.c_float * 4)(*b)
                    if cls is AlphaTask:
                        t.mode, t.src_channels, t.out_channels = mode, Sc, oc
                        t.bg = (C.c_uint16 * 4)(*([(1 << depth) - 1] * 3 + [0]))
                    tasks.append(t)
                y0 += th
        lists[name] = (cls, oc, tasks)
    return lists, tb, es


def kernels_alone(depth, size, dtype_name, reps, warmup):
    """one launch per list, alternating, between device events -> {name: [ms]}, n_tasks"""
    import torch
    from debigulator_amd import _native as N
    from test_emu_png_resize import Task

    L = N.lib()
    for f in (L.debig_hip_png_resize_batch, L.debig_hip_png_resize_alpha_batch):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    H, W = size
    lists, tb, es = tile_lists(depth, size, dtype_name)
    img_bytes = SIDE * SIDE * 4 * (depth // 8)
    torch.manual_seed(depth)
    src = torch.randint(0, 256, (N_FILES * img_bytes,), dtype=torch.uint8, device="cuda")
    wts = torch.from_numpy(np.frombuffer(tb, np.uint8).copy()).cuda()
    out = torch.empty(N_FILES * H * W * 4 * es, dtype=torch.uint8, device="cuda")
    e0, e1 = L.debig_hip_event_create(), L.debig_hip_event_create()
    res, dev = {}, {}
    for name, (cls, oc, tasks) in lists.items():
        dev[name] = torch.from_numpy(np.frombuffer(bytes((cls * len(tasks))(*tasks)), np.uint8).copy()).cuda()
        res[name] = []
    torch.cuda.synchronize()
    for r in range(warmup + reps):
        for name, (cls, oc, tasks) in lists.items():  # alternating
            fn = L.debig_hip_png_resize_batch if cls is Task else L.debig_hip_png_resize_alpha_batch
            L.debig_hip_event_record(e0, None)
            rc = fn(src.data_ptr(), out.data_ptr(), dev[name].data_ptr(), wts.data_ptr(), len(tasks), None)
            L.debig_hip_event_record(e1, None)
            assert rc == 0, rc
            ms = L.debig_hip_event_elapsed_ms(e0, e1)  # (synchronises on e1)
            if r >= warmup:
                res[name].append(float(ms))
    L.debig_hip_event_destroy(e0)
    L.debig_hip_event_destroy(e1)
    return res, len(lists["plain"][2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["# tools/bench_png_tensor_alpha.py: %d PNG files of %d x %d RGBA (%d distinct), white background, antialias on, no mean / std;"
             % (N_FILES, SIDE, SIDE, N_DISTINCT),
             "# %d timed runs after %d warm-up runs, routes / kernels alternating in one process; spread = (max - min) / median"
             % (a.reps, a.warmup),
             "# 1. whole call (ms, host clock around a call that ends in a device synchronise).  over: png_decode_batch_tensor(mode=\"rgb\",",
             "#    alpha=\"over\").  two-step: png_decode_batch_tensor(mode=\"rgba\") then rgb * a + bg * (1 - a) in torch on the device.",
             "#    max |diff|: the largest difference of the two results on the [0, 1] scale (straight against premultiplied filtering)."]
    klines = ["# 2. the resize kernels alone on the same tile lists (ms, device events around one launch; random pixels in device memory).",
              "#    plain: debig_png_resize_kernel, RGBA in, 4 channels out.  over / premultiplied: debig_png_resize_alpha_kernel, RGBA in,",
              "#    3 / 4 channels out."]
    for depth in (8, 16):
        files = workload(depth)
        mib = sum(len(f) for f in files) / 2 ** 20
        for size, dtype in TARGETS:
            sa, ta = route_over(api, files, size, depth, dtype)
            sb_, tb_ = route_two_step(api, files, size, depth, dtype)
            assert sa == sb_ == [0] * N_FILES and tuple(ta.shape) == tuple(tb_.shape) == (N_FILES, 3) + size
            diff = float((ta.float() - tb_.float()).abs().max())
            ts = {"over": [], "two-step": []}
            for r in range(a.warmup + a.reps):
                for name, fn in (("over", route_over), ("two-step", route_two_step)):
                    t = _timed(lambda: fn(api, files, size, depth, dtype), 1, 0)
                    if r >= a.warmup:
                        ts[name] += t
            tag = "RGBA%d (%.0f MiB of files) -> (%d, 3, %d, %d) %s" % (depth, mib, N_FILES, size[0], size[1], dtype)
            lines.append(tag)
            for name in ("over", "two-step"):
                med, sp = _stat(ts[name])
                lines.append("  %-8s (ms): %s | median %.2f, spread %.1f %%" % (name, " ".join("%.2f" % x for x in ts[name]), med, 100 * sp))
            lines.append("  ratio over / two-step: %.3f (medians); max |diff| %.3e"
                         % (_stat(ts["over"])[0] / _stat(ts["two-step"])[0], diff))
            res, n_tasks = kernels_alone(depth, size, dtype, a.reps, a.warmup)
            klines.append("RGBA%d -> (%d, C, %d, %d) %s, %d tiles" % (depth, N_FILES, size[0], size[1], dtype, n_tasks))
            for name in ("plain", "over", "premultiplied"):
                med, sp = _stat(res[name])
                klines.append("  %-13s (ms): %s | median %.4f, spread %.1f %%" % (name, " ".join("%.4f" % x for x in res[name]), med, 100 * sp))
            klines.append("  ratio over / plain: %.3f; premultiplied / plain: %.3f (medians)"
                          % (_stat(res["over"])[0] / _stat(res["plain"])[0], _stat(res["premultiplied"])[0] / _stat(res["plain"])[0]))
    text = "\n".join(lines + klines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
