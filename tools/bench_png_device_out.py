"""PNG pixels that stay on the device (include/decode_png.h: debig_png_decode_batch_dev), on the GPU.

    python tools/bench_png_device_out.py [--n 64] [--size 1024] [--reps 7] [--out profiles/png_device_out.txt]

The workload of tools/bench_png_out_formats.py: n images of size x size (four distinct files, repeated).  Every figure is
the median of --reps runs after one warm-up, with the run-to-run spread (max - min over the median); the two sides of a
comparison alternate run by run.
  1. Whole call to (C, H, W) tensors on the device.  Today's route: png_decode_batch(datas, mode, depth), then per image
     torch.from_numpy(...).to(device) and permute(2, 0, 1).contiguous() -- calls that exist without this feature, so it
     is the yardstick.  The new route: png_decode_batch_device(..., layout="chw").  RGB8 files to RGB8, RGBA16 files to
     RGBA16.  The results are compared before any time is.
  2. Kernel alone: debig_hip_png_spec_defilter_planar_batch against debig_hip_png_spec_defilter_fmt_batch on the same
     task lists (scanline streams made here and put on the device, no inflate), device events around each launch.
  3. HWC on the device against debig_png_decode_batch_fmt to host buffers, the same files: the difference is the
     download.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WHOLE = [("rgb8", 2, 8, "rgb", 8), ("rgba16", 6, 16, "rgba", 16)]
# kernel alone: source (colour type, depth) -> resolved out_fmt (layout | 0x10 for 16 bits)
KERNEL = [("rgb8 -> RGB8", 2, 8, 0x01), ("rgba8 -> RGBA8", 6, 8, 0x00), ("rgba8 -> RGB8", 6, 8, 0x01),
          ("grey+alpha8 -> GRAY_ALPHA8", 4, 8, 0x03), ("rgb16 -> RGB16", 2, 16, 0x11), ("rgba16 -> RGBA16", 6, 16, 0x10),
          ("rgba16 -> RGBA8", 6, 16, 0x00)]
CHANNELS = {0: 4, 1: 3, 2: 1, 3: 2}


class SpecTask(C.Structure):  # include/debig_hip.h: debig_png_spec_task
    _fields_ = [("stream_off", C.c_uint64), ("rgba_off", C.c_uint64), ("pal_off", C.c_uint64), ("scratch_off", C.c_uint64),
                ("width", C.c_uint32), ("height", C.c_uint32), ("img_width", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32),
                ("bpp_f", C.c_uint8), ("depth", C.c_uint8), ("color_type", C.c_uint8), ("channels", C.c_uint8),
                ("key", C.c_uint16 * 3), ("has_key", C.c_uint16), ("n_pal", C.c_uint16), ("out_fmt", C.c_uint16),
                ("img_height", C.c_uint32)]


def _a16(x):
    return (x + 15) // 16 * 16


def stat(v):
    med = float(np.median(v))
    return med, 100.0 * (max(v) - min(v)) / med


def alternate(routes, reps):
    """routes: {name: callable}; one warm-up each, then reps rounds with the routes in turn -> {name: [ms]}"""
    import torch

    for fn in routes.values():
        fn()
    ts = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return ts


def files_of(ct, depth, size, n):
    import bench_png_spec as B

    rng = np.random.default_rng(1)
    distinct = [B.encode_fast(B._image(rng, size, ct, depth, k), ct, depth) for k in range(4)]
    return [distinct[k % 4] for k in range(n)]


def kernel_alone(ct, depth, out_fmt, size, n, reps, dev):
    """-> (format twin [ms], planar [ms]): n tasks of size x size, the same task list to both launchers"""
    import torch
    import bench_png_spec as B
    import png_spec_ref as R
    from debigulator_amd import _native as N

    L = N.lib()
    for name in ("debig_hip_png_spec_defilter_fmt_batch", "debig_hip_png_spec_defilter_planar_batch"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    rng = np.random.default_rng(2)
    bpp = R.bpp_f(ct, depth)
    rb = R.row_bytes(size, ct, depth)
    streams = [B._filter_rows(B._pack(B._image(rng, size, ct, depth, k), ct, depth), bpp).tobytes() for k in range(4)]
    slot = _a16(len(streams[0])) + 32
    scratch = 4 * (_a16(rb) + 16)
    out_bytes = size * size * CHANNELS[out_fmt & 3] * (2 if out_fmt & 0x10 else 1)
    arena = np.zeros(64 + n * (slot + scratch) + 64, np.uint8)
    tasks = (SpecTask * n)()
    for i in range(n):
        off = 64 + i * slot
        arena[off: off + len(streams[i % 4])] = np.frombuffer(streams[i % 4], np.uint8)
        t = tasks[i]
        t.stream_off, t.rgba_off, t.scratch_off = off, i * (_a16(out_bytes) + 16), 64 + n * slot + i * scratch
        t.width = t.height = t.img_width = t.img_height = size
        t.dx = t.dy = 1
        t.bpp_f, t.depth, t.color_type, t.channels, t.out_fmt = bpp, depth, ct, R.CHANNELS[ct], out_fmt
    d_arena = torch.from_numpy(arena).to(dev)
    d_out = torch.empty(n * (_a16(out_bytes) + 16) + 64, dtype=torch.uint8, device=dev)
    d_tasks = torch.from_numpy(np.frombuffer(bytes(tasks), np.uint8).copy()).to(dev)
    d_res = torch.zeros(8 * n, dtype=torch.uint8, device=dev)
    outs = {}

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        N.check(fn(d_arena.data_ptr(), d_out.data_ptr(), d_tasks.data_ptr(), d_res.data_ptr(), n, None), "de-filter launch")
        e1.record()
        torch.cuda.synchronize()
        assert not d_res.cpu().numpy().view(np.uint32)[0::2].any(), "a task failed"
        return e0.elapsed_time(e1)

    fns = {"fmt": L.debig_hip_png_spec_defilter_fmt_batch, "planar": L.debig_hip_png_spec_defilter_planar_batch}
    for k, fn in fns.items():  # warm-up, and the two outputs must be the same pixels
        run(fn)
        outs[k] = d_out[: out_bytes].cpu().numpy().copy()
    ch, bs = CHANNELS[out_fmt & 3], 2 if out_fmt & 0x10 else 1
    hwc = outs["fmt"].view(np.uint16 if bs == 2 else np.uint8).reshape(size, size, ch)
    chw = outs["planar"].view(np.uint16 if bs == 2 else np.uint8).reshape(ch, size, size)
    assert np.array_equal(np.transpose(hwc, (2, 0, 1)), chw), "planar and interleaved pixels differ"
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(run(fn))
    return ts["fmt"], ts["planar"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5
    import torch
    from debigulator_amd import api

    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    lines = ["# tools/bench_png_device_out.py --n %d --size %d --reps %d (%s)" % (a.n, a.size, a.reps, torch.cuda.get_device_name(0)),
             "# medians over reps after one warm-up, the two sides alternating; spread = (max - min) / median of the runs"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    emit("# 1. whole call -> (C, H, W) tensors on the device, ms: today = png_decode_batch + from_numpy().to() + permute().contiguous()")
    emit("# 3. whole call, HWC, ms: debig_png_decode_batch_fmt to host buffers against debig_png_decode_batch_dev")
    for name, ct, depth, mode, d in WHOLE:
        fs = files_of(ct, depth, a.size, a.n)

        def today():
            out = api.png_decode_batch(fs, mode=mode, depth=d)
            return [torch.from_numpy(px).to(dev).permute(2, 0, 1).contiguous() for _, px, _ in out]

        def new():
            return api.png_decode_batch_device(fs, mode=mode, depth=d, layout="chw", device=dev)

        want, got = today(), new()
        for w, (st, t, _) in zip(want, got):
            assert st == 0 and torch.equal(w.view(torch.uint8), t.view(torch.uint8))
        del want, got
        ts = alternate({"today": today, "new": new}, a.reps)
        (mt, st_), (mn, sn) = stat(ts["today"]), stat(ts["new"])
        emit("1. %-7s today %8.2f (spread %4.1f %%)   png_decode_batch_device chw %8.2f (spread %4.1f %%)   new / today = %.3f"
             % (name, mt, st_, mn, sn, mn / mt))
        ts = alternate({"fmt": lambda: api.png_decode_batch(fs, mode=mode, depth=d),
                        "dev": lambda: api.png_decode_batch_device(fs, mode=mode, depth=d, layout="hwc", device=dev)}, a.reps)
        (mf, sf), (md, sd) = stat(ts["fmt"]), stat(ts["dev"])
        emit("3. %-7s _fmt  %8.2f (spread %4.1f %%)   _dev hwc %8.2f (spread %4.1f %%)   dev / fmt = %.3f   the download: %.2f ms"
             % (name, mf, sf, md, sd, md / mf, mf - md))
    emit("# 2. kernel alone, the same %d tasks of %d^2 to both launchers, device events around the launch, us" % (a.n, a.size))
    for name, ct, depth, out_fmt in KERNEL:
        f, p = kernel_alone(ct, depth, out_fmt, a.size, a.n, a.reps, dev)
        (mf, sf), (mp, sp) = stat(f), stat(p)
        emit("2. %-27s format twin %8.1f (spread %4.1f %%)   planar %8.1f (spread %4.1f %%)   planar / twin = %.3f"
             % (name, 1e3 * mf, sf, 1e3 * mp, sp, mp / mf))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
