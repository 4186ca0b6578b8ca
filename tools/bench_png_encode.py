"""PNG encode on the device (api.png_encode_batch) against the route there was without it, each kernel against a device-to-device
copy of its input bytes, and the compressed size against zlib level 1 and level 0.

Workload: 64 images of 512 x 512 and of 1024 x 1024 in device memory:
    photo     RGB8: the sample PNGs of tests/golden/resources, tiled and cropped to the side (8 distinct images, repeated)
    noise     RGB8: uniformly random bytes
    labels    uint8, a blocky 21-class map, written with a palette
    ids       int32 at depth 16: api.png_label_components of that map
  at levels 0 and 1, filter adaptive, and filter none for the two label workloads.

    python tools/bench_png_encode.py [--reps 6 --warmup 2 --host-reps 3] --out profiles/png_encode.txt
        (a) the whole call (host clock, the call synchronises) against tensor.cpu() + Pillow save(format="PNG", compress_level=1) per
            image, on one thread and on 16 threads (Pillow releases the interpreter lock while it compresses);
        (b) each kernel alone (device events around one launch over the host's cut) against torch's device-to-device copy of the
            kernel's input bytes;
        (c) the DEFLATE bytes of the call's files against zlib.compress(stream, 1) and against level 0 on the same filtered streams
            (the stream is what the file's own IDAT inflates to).
    Every cell: median ms (spread = (max - min) / median).  No hardware counters are collected."""
import argparse
import ctypes as C
import io
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_IMAGES, N_DISTINCT = 64, 8
SIDES = (512, 1024)


def workload(kind, side, rng, api, dev):
    """-> (the device tensor (N, side, side[, 3]), the keywords of the call)"""
    import torch
    from PIL import Image

    if kind == "photo":
        res = os.path.join(ROOT, "tests", "golden", "resources")
        names = sorted(f for f in os.listdir(res) if f.endswith(".png"))[:N_DISTINCT]
        imgs = []
        for f in names:
            a = np.asarray(Image.open(os.path.join(res, f)).convert("RGB"))
            reps = (-(-side // a.shape[0]), -(-side // a.shape[1]), 1)
            imgs.append(np.tile(a, reps)[:side, :side])
        a = np.stack([imgs[k % len(imgs)] for k in range(N_IMAGES)])
    elif kind == "noise":
        a = np.stack([rng.integers(0, 256, (side, side, 3), dtype=np.uint8) for _ in range(N_DISTINCT)] * (N_IMAGES // N_DISTINCT))
    else:
        maps = [np.repeat(np.repeat(rng.integers(0, 21, (side // 32, side // 32)), 32, axis=0), 32, axis=1).astype(np.uint8) for _ in range(N_DISTINCT)]
        a = np.stack(maps * (N_IMAGES // N_DISTINCT))
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = {}
    if kind == "labels":
        kw["palette"] = rng.integers(0, 256, (21, 3), dtype=np.uint8)
    if kind == "ids":
        t, _ = api.png_label_components(t, 4)
    return t, kw


def pillow_route(t, kw, threads):
    """today's route: the tensor to the host, Pillow image by image"""
    from PIL import Image

    a = t.cpu().numpy()

    def one(x):
        if x.dtype == np.int32:
            im = Image.fromarray(x.astype(np.uint16))
        else:
            im = Image.fromarray(x)
            if "palette" in kw:
                im.putpalette(kw["palette"].tobytes())  # (an "L" image becomes a "P" image)
        buf = io.BytesIO()
        im.save(buf, format="PNG", compress_level=1)
        return buf.getvalue()

    if threads == 1:
        return [one(x) for x in a]
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, a))


def med(xs):
    xs = sorted(xs)
    m = xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])
    return m, (xs[-1] - xs[0]) / m if m else 0.0


def cell(xs):
    m, s = med(xs)
    return "%.3g (%4.1f %%)" % (m, 100 * s)


def kernels_alone(t, kw, filt, level, reps, warmup):
    """device events around one launch of each kernel over the host's cut, and around a copy of its input bytes"""
    import torch

    import png_encode_ref as R
    import test_emu_png_encode as E
    from debigulator_amd import _native as N

    L = N.lib()
    n, H, W = t.shape[:3]
    Cn = t.shape[3] if t.dim() == 4 else 1
    dtype = {torch.uint8: 0, torch.int32: 2}[t.dtype]
    depth = 8 if dtype == 0 else 16
    rb = W * Cn * depth // 8
    slen = H * (1 + rb)
    streams = torch.empty(n * slen, dtype=torch.uint8, device=t.device)
    flags = torch.zeros(n, dtype=torch.int32, device=t.device)
    ft, dt, at = [], [], 0
    img_bytes = H * W * Cn * t.element_size()
    for i in range(n):
        for y0, r in R.row_runs(H, rb):
            ft.append(E.FTask(image_off=i * img_bytes, stream_off=i * slen, w=W, h=H, row0=y0, rows=r, channels=Cn, dtype=dtype, depth=depth,
                              layout=0, filter=filt, palette_entries=21 if "palette" in kw else 0, flag_idx=i))
        cuts = R.chunks(slen)
        for k, (off, ln) in enumerate(cuts):
            dt.append(E.DTask(stream_off=i * slen, stream_len=slen, chunk_off=off, slot_off=at, chunk_len=ln, slot_cap=R.slot_bytes(ln),
                              level=level, bpp=Cn * depth // 8, last=int(k == len(cuts) - 1), count_idx=len(dt)))
            at += R.slot_bytes(ln)
    slots = torch.empty(at, dtype=torch.uint8, device=t.device)
    counts = torch.zeros(len(dt), dtype=torch.int32, device=t.device)

    def up(tasks, cls):
        return torch.frombuffer(bytearray(bytes((cls * len(tasks))(*tasks))), dtype=torch.uint8).to(t.device)

    d_ft, d_dt = up(ft, E.FTask), up(dt, E.DTask)
    for fn in (L.debig_hip_png_encode_filter_batch, L.debig_hip_png_encode_deflate_batch):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    copy_in, copy_st = torch.empty_like(t), torch.empty_like(streams)
    runs = {"filter": lambda: L.debig_hip_png_encode_filter_batch(t.data_ptr(), streams.data_ptr(), d_ft.data_ptr(), flags.data_ptr(), len(ft), stream),
            "copy_t": lambda: copy_in.copy_(t),
            "deflate": lambda: L.debig_hip_png_encode_deflate_batch(streams.data_ptr(), slots.data_ptr(), d_dt.data_ptr(), counts.data_ptr(), len(dt), stream),
            "copy_s": lambda: copy_st.copy_(streams)}
    out = {}
    for name, fn in runs.items():
        ms = []
        for k in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn()
            b.record()
            torch.cuda.synchronize()
            assert name.startswith("copy") or rc == 0
            if k >= warmup:
                ms.append(a.elapsed_time(b))
        out[name] = ms
    return out, n * img_bytes, n * slen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="*", default=list(SIDES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode.txt"))
    a = ap.parse_args()
    import torch

    from debigulator_amd import api

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    lines = ["# tools/bench_png_encode.py on %s: %d images per tensor, %d timed runs after %d warm-up runs (the host route: %d after 1);"
             % (torch.cuda.get_device_name(0), N_IMAGES, a.reps, a.warmup, a.host_reps),
             "# every cell: median ms (spread = (max - min) / median).  call: api.png_encode_batch whole, host clock, the call synchronises;",
             "# host1 / host16: tensor.cpu() + Pillow save(compress_level=1) per image on 1 / 16 threads.  filter, deflate: the kernels alone, device",
             "# events; copy_t, copy_s: torch's device-to-device copy of the tensor / of the filtered streams; GB/s: input bytes of the kernel per second.",
             "# size: DEFLATE bytes of the call's files / zlib.compress(stream, 1) on the same filtered streams; /L0: over the level-0 payload.",
             "# No hardware counters were collected.",
             "side  kind    filter    L | call ms          host1 ms         host16 ms        host16/call | filter ms        copy_t ms        filter GB/s  x copy | "
             "deflate ms       copy_s ms        deflate GB/s  x copy | size/zlib1  size/L0"]
    for side in a.sides:
        for kind in ("photo", "noise", "labels", "ids"):
            t, kw = workload(kind, side, rng, api, dev)
            for filt in (("adaptive", "none") if kind in ("labels", "ids") else ("adaptive",)):
                host = {}
                for threads in (1, 16):
                    ms = []
                    for k in range(1 + a.host_reps):
                        t0 = time.perf_counter()
                        pillow_route(t, kw, threads)
                        if k:
                            ms.append(1e3 * (time.perf_counter() - t0))
                    host[threads] = ms
                for level in (0, 1):
                    ms = []
                    for k in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        res = api.png_encode_batch(t, filter=filt, level=level, **kw)
                        if k >= a.warmup:
                            ms.append(1e3 * (time.perf_counter() - t0))
                    assert all(s == 0 for s, _ in res)
                    ours = zl = l0 = 0
                    for _, d in res[:N_DISTINCT]:
                        at = d.index(b"IDAT") + 4
                        ln = int.from_bytes(d[at - 8: at - 4], "big")
                        z = d[at: at + ln]
                        stream = zlib.decompress(z)
                        ours += ln - 6
                        zl += len(zlib.compress(stream, 1)) - 6
                        l0 += len(stream) + 5 * (-(-len(stream) // 32768)) + 5 * (-(-len(stream) // 32768) - 1)
                    kt, tb, sb = kernels_alone(t, kw, api.PNG_ENCODE_FILTERS[filt], level, a.reps, a.warmup)
                    mf, mc, md, ms_ = (med(kt[k])[0] for k in ("filter", "copy_t", "deflate", "copy_s"))
                    lines.append("%-5d %-7s %-9s %d | %-16s %-16s %-16s %-11.2f | %-16s %-16s %-12.1f %-6.1f | %-16s %-16s %-13.1f %-6.1f | %-11.3f %.3f"
                                 % (side, kind, filt, level, cell(ms), cell(host[1]), cell(host[16]), med(host[16])[0] / med(ms)[0], cell(kt["filter"]),
                                    cell(kt["copy_t"]), tb / mf / 1e6, mf / mc, cell(kt["deflate"]), cell(kt["copy_s"]), sb / md / 1e6, md / ms_,
                                    ours / zl, ours / l0))
                    print(lines[-1], flush=True)
            del t
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
