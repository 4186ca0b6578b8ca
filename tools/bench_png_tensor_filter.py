"""PNG bytes -> one bicubic-resized, normalised tensor (api.png_decode_batch_tensor(filter="bicubic")) against the route
without it, and the signed resize kernel against the bilinear kernels.

Workload: 64 PNG files of 1024 x 1024 RGB8, and 64 of RGBA8 (4 distinct images each from a fixed seed, repeated; smooth
colour with noise) -> (64, C, 224, 224) float32 and (64, C, 512, 512) bfloat16, antialias on, ImageNet mean / std.

    python tools/bench_png_tensor_filter.py [--reps 8 --warmup 2] --out profiles/png_tensor_filter.txt
        1. whole call, the two routes alternating in one process, a device synchronise inside every timed call:
             bicubic: api.png_decode_batch_tensor(filter="bicubic")
             torch:   api.png_decode_batch_device(layout="chw") -> per image interpolate(mode="bicubic", antialias=True) ->
                      normalise -> torch.stack (what a caller does without the new filter)
        2. the resize kernels alone (device events around one launch each, after warm-up launches), every kernel on the tile
           list the host's rule makes from ITS axis table (bicubic has twice the taps per axis, so its tiles span more source
           rows): debig_png_resize_kernel (bilinear), debig_png_resize_alpha_kernel (bilinear, RGBA over white) and
           debig_png_resize_cubic_kernel (straight; RGBA also over white), from random pixels in device memory
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
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]


def _png(rng, k, ch):
    import png_spec_ref as R

    h = w = SIDE
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, ch), np.float32)
    for c in range(ch):
        img[..., c] = 0.5 + 0.4 * np.sin(x / (31 + 7 * c + k) + 0.6 * k) * np.cos(y / (47 + 5 * c) - 0.3 * c)
    img += rng.normal(0, 0.02, size=(h, w, ch))
    s = np.clip(img * 255, 0, 255).astype(np.uint8)
    rows = np.zeros((h, 1 + w * ch), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = s.reshape(h, -1)
    ihdr = R.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if ch == 3 else 6, 0, 0, 0))
    return R.SIG + ihdr + R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b"")


def workload(ch):
    rng = np.random.default_rng(20261017 + ch)
    distinct = [_png(rng, k, ch) for k in range(N_DISTINCT)]
    return [distinct[i % N_DISTINCT] for i in range(N_FILES)]


def route_bicubic(api, files, size, mode, dtype):
    ch = len(mode)
    return api.png_decode_batch_tensor(files, size, mode=mode, dtype=dtype, mean=MEAN[:ch], std=STD[:ch], filter="bicubic")[:2]


def route_torch(api, files, size, mode, dtype):
    import torch

    ch = len(mode)
    res = api.png_decode_batch_device(files, mode=mode, layout="chw")
    mean = torch.tensor(MEAN[:ch], device="cuda").view(ch, 1, 1)
    std = torch.tensor(STD[:ch], device="cuda").view(ch, 1, 1)
    outs = []
    for _, t, _ in res:
        f = torch.nn.functional.interpolate(t[None].float(), size=size, mode="bicubic", align_corners=False, antialias=True)[0]
        outs.append(((f.clamp(0, 255) / 255 - mean) / std).to(getattr(torch, dtype)))
    return [s for s, _, _ in res], torch.stack(outs)


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


def tile_lists(Sc, size, dtype_name):
    """{name: (launcher name, struct, tasks, table bytes)}: each kernel on the host's tiles for its own axis table"""
    import png_resize_ref as Z
    import test_emu_png_resize as E
    import test_emu_png_resize_filter as EF
    from test_emu_png_resize_alpha import AlphaTask

    H, W = size
    assert H == W  # one table serves both axes
    dtype = Z.DTYPES[dtype_name]
    es = {Z.T_F32: 4, Z.T_BF16: 2}[dtype]
    img_bytes = SIDE * SIDE * Sc
    a, b = Z.affine(8, (1, 1, 1, 1), (0, 0, 0, 0))
    kinds = [("bilinear", "debig_hip_png_resize_batch", E.Task, E.axis_table, Sc, None),
             ("bicubic", "debig_hip_png_resize_cubic_batch", AlphaTask, EF.axis_table, Sc, 0)]
    if Sc == 4:
        kinds += [("bilinear over", "debig_hip_png_resize_alpha_batch", AlphaTask, E.axis_table, 3, 2),
                  ("bicubic over", "debig_hip_png_resize_cubic_batch", AlphaTask, EF.axis_table, 3, 2)]
    lists = {}
    for name, launcher, cls, table, oc, mode in kinds:
        tb, ent, mt = table(SIDE, W, True)
        tw = min(W, E.TILE_W, E.WX_CAP // mt, E.HQ_CAP // (mt * Sc))
        tasks = []
        for i in range(N_FILES):
            y0 = 0
            while y0 < H:
                lo, hi, th = ent[y0][0], sum(ent[y0]), 1
                while y0 + th < H and th < 64:
                    f, e = ent[y0 + th][0], sum(ent[y0 + th])
                    if (max(hi, e) - min(lo, f)) * tw * Sc > E.HQ_CAP:
                        break
                    lo, hi, th = min(lo, f), max(hi, e), th + 1
                for x0 in range(0, W, tw):
                    t = cls(src_off=i * img_bytes, out_off=i * H * W * oc * es, wx_off=0, wy_off=0, src_pitch=SIDE * Sc, tile_x=x0,
                            tile_y=y0, tile_w=min(tw, W - x0), tile_h=th, src_y0=lo, src_rows=hi - lo, out_sx=1, out_sy=W,
                            out_sc=H * W, channels=Sc, bits=8, dtype=dtype)
                    t.a, t.b = (C.c_float * 4)(*a), (C.c_float * 4)(*b)
                    if mode is not None:
                        t.mode, t.src_channels, t.out_channels = mode, Sc, oc
                        t.bg = (C.c_uint16 * 4)(*([255] * 3 + [0] if mode == 2 else [0] * 4))
                    tasks.append(t)
                y0 += th
        lists[name] = (launcher, cls, tasks, tb, mt)
    return lists, es


def kernels_alone(Sc, size, dtype_name, reps, warmup):
    """one launch per list, alternating, between device events -> {name: ([ms], tiles, max taps)}"""
    import torch
    from debigulator_amd import _native as N

    L = N.lib()
    for f in (L.debig_hip_png_resize_batch, L.debig_hip_png_resize_alpha_batch, L.debig_hip_png_resize_cubic_batch):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    H, W = size
    lists, es = tile_lists(Sc, size, dtype_name)
    torch.manual_seed(Sc)
    src = torch.randint(0, 256, (N_FILES * SIDE * SIDE * Sc,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N_FILES * H * W * 4 * es, dtype=torch.uint8, device="cuda")
    e0, e1 = L.debig_hip_event_create(), L.debig_hip_event_create()
    res, dev = {}, {}
    for name, (launcher, cls, tasks, tb, mt) in lists.items():
        dev[name] = (torch.from_numpy(np.frombuffer(bytes((cls * len(tasks))(*tasks)), np.uint8).copy()).cuda(),
                     torch.from_numpy(np.frombuffer(tb, np.uint8).copy()).cuda())
        res[name] = ([], len(tasks), mt)
    torch.cuda.synchronize()
    for r in range(warmup + reps):
        for name, (launcher, cls, tasks, tb, mt) in lists.items():  # alternating
            L.debig_hip_event_record(e0, None)
            rc = getattr(L, launcher)(src.data_ptr(), out.data_ptr(), dev[name][0].data_ptr(), dev[name][1].data_ptr(), len(tasks), None)
            L.debig_hip_event_record(e1, None)
            assert rc == 0, rc
            ms = L.debig_hip_event_elapsed_ms(e0, e1)  # (synchronises on e1)
            if r >= warmup:
                res[name][0].append(float(ms))
    L.debig_hip_event_destroy(e0)
    L.debig_hip_event_destroy(e1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["# tools/bench_png_tensor_filter.py: %d PNG files of %d x %d, 8 bit (%d distinct), antialias on, ImageNet mean / std;"
             % (N_FILES, SIDE, SIDE, N_DISTINCT),
             "# %d timed runs after %d warm-up runs, routes / kernels alternating in one process; spread = (max - min) / median"
             % (a.reps, a.warmup),
             "# 1. whole call (ms, host clock around a call that ends in a device synchronise).  bicubic: png_decode_batch_tensor(",
             "#    filter=\"bicubic\").  torch: png_decode_batch_device(layout=\"chw\") -> per image interpolate(mode=\"bicubic\",",
             "#    antialias=True) -> normalise -> torch.stack.  max |diff|: the largest difference of the two results in units of one",
             "#    8-bit level (diff * std * 255; integer Q14 arithmetic against float32, output dtype rounding included)."]
    klines = ["# 2. the resize kernels alone (ms, device events around one launch; random pixels in device memory), each on the tiles the",
              "#    host's rule makes from its own axis table.  bilinear: debig_png_resize_kernel; bilinear over: debig_png_resize_alpha_kernel;",
              "#    bicubic / bicubic over: debig_png_resize_cubic_kernel (STRAIGHT / OVER)."]
    for mode in ("rgb", "rgba"):
        ch = len(mode)
        files = workload(ch)
        mib = sum(len(f) for f in files) / 2 ** 20
        for size, dtype in TARGETS:
            sa, ta = route_bicubic(api, files, size, mode, dtype)
            sb_, tb_ = route_torch(api, files, size, mode, dtype)
            assert sa == sb_ == [0] * N_FILES and tuple(ta.shape) == tuple(tb_.shape) == (N_FILES, ch) + size
            std = torch.tensor(STD[:ch], device="cuda").view(1, ch, 1, 1)
            diff = float(((ta.float() - tb_.float()).abs() * std * 255).max())
            ts = {"bicubic": [], "torch": []}
            for r in range(a.warmup + a.reps):
                for name, fn in (("bicubic", route_bicubic), ("torch", route_torch)):
                    t = _timed(lambda: fn(api, files, size, mode, dtype))
                    if r >= a.warmup:
                        ts[name].append(t)
            lines.append("%s8 (%.0f MiB of files) -> (%d, %d, %d, %d) %s" % (mode.upper(), mib, N_FILES, ch, size[0], size[1], dtype))
            for name in ("bicubic", "torch"):
                med, sp = _stat(ts[name])
                lines.append("  %-8s (ms): %s | median %.2f, spread %.1f %%" % (name, " ".join("%.2f" % x for x in ts[name]), med, 100 * sp))
            lines.append("  ratio bicubic / torch: %.3f (medians); max |diff| %.3f levels"
                         % (_stat(ts["bicubic"])[0] / _stat(ts["torch"])[0], diff))
            res = kernels_alone(ch, size, dtype, a.reps, a.warmup)
            klines.append("%s8 -> (%d, C, %d, %d) %s" % (mode.upper(), N_FILES, size[0], size[1], dtype))
            for name, (ms, n_tasks, mt) in res.items():
                med, sp = _stat(ms)
                klines.append("  %-13s (ms): %s | median %.4f, spread %.1f %%; %d tiles, %d taps per axis"
                              % (name, " ".join("%.4f" % x for x in ms), med, 100 * sp, n_tasks, mt))
            klines.append("  ratio bicubic / bilinear: %.3f (medians)" % (_stat(res["bicubic"][0])[0] / _stat(res["bilinear"][0])[0]))
            if "bicubic over" in res:
                klines.append("  ratio bicubic over / bilinear over: %.3f (medians)"
                              % (_stat(res["bicubic over"][0])[0] / _stat(res["bilinear over"][0])[0]))
    text = "\n".join(lines + klines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
