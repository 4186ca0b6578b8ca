"""Level 3 of the PNG encode (api.png_encode_batch_lz: row-above candidates and one-step lazy matching in front of level 2's back end)
against level 2 and against zlib, on the cells of tools/bench_png_encode_dyn.py / profiles/png_encode_dyn.txt -- 64 images of
512 x 512 and of 1024 x 1024 in device memory: photographs, noise, a blocky palette map, 16-bit instance ids -- and a palette map
with curved borders; filter adaptive, and filter none for the label workloads.

    python tools/bench_png_encode_lz.py [--reps 6 --warmup 2 --host-reps 3] --out profiles/png_encode_lz.txt
        (a) size: the DEFLATE bytes of the level-3 files over the level-2 files' and over zlib.compress(stream, 1) and
            zlib.compress(stream, 6) on the same filtered streams;
        (b) kernels alone (device events around one launch over the host's cut): the lz kernel and the level-2 dynamic kernel on the
            same tasks (level 2 is the parent commit's code: the yardstick);
        (c) the whole call at level 3 against level 2 (host clock, the call synchronises) and against tensor.cpu() + Pillow
            save(compress_level=1) per image on 16 threads; a cell where the host route wins is marked MISS, one inside the two
            spreads TIE.
    Every time: median ms (spread = (max - min) / median).  No hardware counters are collected."""
import argparse
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_png_encode as B  # noqa: E402
from bench_png_encode_dyn import payload  # noqa: E402


def curved(side, k):
    """a class map of 19 classes with curved borders, image k of the batch"""
    y, x = np.mgrid[0:side, 0:side]
    return (((np.sin((x + 11 * k) / 23) + np.cos((y + 7 * k) / 17) + np.sin((x + y) / 31)) * 3).astype(np.int64) % 19).astype(np.uint8)


def workload(kind, side, rng, api, dev):
    import torch

    if kind != "curved":
        return B.workload(kind, side, rng, api, dev)
    a = np.stack([curved(side, k) for k in range(B.N_DISTINCT)] * (B.N_IMAGES // B.N_DISTINCT))
    return torch.from_numpy(a).to(dev), {"palette": rng.integers(0, 256, (21, 3), dtype=np.uint8)}


def kernels_alone(t, reps, warmup, filt, kw):
    """-> {name: [ms]}: the level-2 and the level-3 kernel over the host's cut of the batch's filtered streams"""
    import torch

    import png_encode_lz_ref as Z
    import png_encode_ref as R
    import test_emu_png_encode as E
    import test_emu_png_encode_dyn as Y
    import test_emu_png_encode_lz as Q
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
    ft, d2, d3, at, tk = [], [], [], 0, 0
    img_bytes = H * W * Cn * t.element_size()
    for i in range(n):
        for y0, r in R.row_runs(H, rb):
            ft.append(E.FTask(image_off=i * img_bytes, stream_off=i * slen, w=W, h=H, row0=y0, rows=r, channels=Cn, dtype=dtype, depth=depth,
                              layout=0, filter=filt, palette_entries=21 if "palette" in kw else 0, flag_idx=i))
        cuts = R.chunks(slen)
        for k, (off, ln) in enumerate(cuts):
            common = dict(stream_off=i * slen, stream_len=slen, chunk_off=off, slot_off=at, chunk_len=ln, slot_cap=R.slot_bytes(ln),
                          bpp=Cn * depth // 8, last=int(k == len(cuts) - 1), count_idx=len(d2), token_off=tk, token_cap=4 * R.CHUNK)
            d2.append(Y.YTask(level=2, **common))
            d3.append(Q.ZTask(level=3, row_stride=Z.host_stride(W, Cn, depth), **common))
            at += R.slot_bytes(ln)
            tk += 4 * R.CHUNK
    slots = torch.empty(at, dtype=torch.uint8, device=t.device)
    tokens = torch.empty(tk, dtype=torch.uint8, device=t.device)
    counts = torch.zeros(len(d2), dtype=torch.int32, device=t.device)

    def up(tasks, cls):
        return torch.frombuffer(bytearray(bytes((cls * len(tasks))(*tasks))), dtype=torch.uint8).to(t.device)

    d_ft, d_2, d_3 = up(ft, E.FTask), up(d2, Y.YTask), up(d3, Q.ZTask)
    L.debig_hip_png_encode_filter_batch.restype = C.c_int
    L.debig_hip_png_encode_filter_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    for fn in (L.debig_hip_png_encode_dynamic_batch, L.debig_hip_png_encode_lz_batch):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    assert L.debig_hip_png_encode_filter_batch(t.data_ptr(), streams.data_ptr(), d_ft.data_ptr(), flags.data_ptr(), len(ft), stream) == 0
    torch.cuda.synchronize()
    runs = {"level2": lambda: L.debig_hip_png_encode_dynamic_batch(streams.data_ptr(), slots.data_ptr(), tokens.data_ptr(), d_2.data_ptr(),
                                                                   counts.data_ptr(), len(d2), stream),
            "level3": lambda: L.debig_hip_png_encode_lz_batch(streams.data_ptr(), slots.data_ptr(), tokens.data_ptr(), d_3.data_ptr(), counts.data_ptr(),
                                                              len(d3), stream)}
    out = {}
    for name, fn in runs.items():
        ms = []
        for k in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn()
            b.record()
            torch.cuda.synchronize()
            assert rc == 0
            if k >= warmup:
                ms.append(a.elapsed_time(b))
        out[name] = ms
    return out


def verdict(host, call):
    """MISS: every run of the host route is faster than every run of the call; TIE: the two ranges of runs overlap"""
    if max(host) < min(call):
        return "  MISS"
    return "" if min(host) > max(call) else "  TIE"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="*", default=list(B.SIDES))
    ap.add_argument("--kinds", nargs="*", default=["photo", "noise", "labels", "ids", "curved"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_lz.txt"))
    a = ap.parse_args()
    import torch

    from debigulator_amd import api

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    lines = ["# tools/bench_png_encode_lz.py on %s: %d images per tensor, %d timed runs after %d warm-up runs (the host route: %d after 1);"
             % (torch.cuda.get_device_name(0), B.N_IMAGES, a.reps, a.warmup, a.host_reps),
             "# every time: median ms (spread = (max - min) / median).  L3 KiB: the DEFLATE bytes of the level-3 files of the tensor's distinct images;",
             "# L3/L2, L3/zlib1, L3/zlib6: over the level-2 files' and over zlib.compress(stream, 1 / 6) on the same filtered streams.  level2, level3: the",
             "# kernels alone on the same tasks, device events (level 2 is the parent commit's code).  call L2 / L3: api.png_encode_batch_dyn /",
             "# api.png_encode_batch_lz whole, host clock; host16: tensor.cpu() + Pillow save(compress_level=1) per image on 16 threads; MISS: the host",
             "# route's slowest run beats the call's fastest; TIE: the two ranges of runs overlap.  No hardware counters were collected.",
             "side  kind    filter   | L3 KiB   L3/L2  L3/zlib1 L3/zlib6 | level2 ms        level3 ms        L3/L2  | call L2 ms       call L3 ms       L3/L2  "
             "host16 ms        host16/L3"]
    for side in a.sides:
        for kind in a.kinds:
            t, kw = workload(kind, side, rng, api, dev)
            for filt in (("adaptive", "none") if kind in ("labels", "ids", "curved") else ("adaptive",)):
                host = []
                for k in range(1 + a.host_reps):
                    t0 = time.perf_counter()
                    B.pillow_route(t, kw, 16)
                    if k:
                        host.append(1e3 * (time.perf_counter() - t0))
                call, files = {}, {}
                for level, fn in ((2, api.png_encode_batch_dyn), (3, api.png_encode_batch_lz)):
                    ms = []
                    for k in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        res = fn(t, filter=filt, level=level, **kw)
                        if k >= a.warmup:
                            ms.append(1e3 * (time.perf_counter() - t0))
                    assert all(s == 0 for s, _ in res)
                    call[level], files[level] = ms, [d for _, d in res[:B.N_DISTINCT]]
                l2 = l3 = z1 = z6 = 0
                for f2, f3 in zip(files[2], files[3]):
                    p2, p3 = payload(f2), payload(f3)
                    stream = zlib.decompress(p3)
                    assert stream == zlib.decompress(p2)
                    l2 += len(p2) - 6
                    l3 += len(p3) - 6
                    z1 += len(zlib.compress(stream, 1)) - 6
                    z6 += len(zlib.compress(stream, 6)) - 6
                kt = kernels_alone(t, a.reps, a.warmup, api.PNG_ENCODE_FILTERS[filt], kw)
                m2, m3 = B.med(kt["level2"])[0], B.med(kt["level3"])[0]
                h16, c3 = B.med(host)[0], B.med(call[3])[0]
                lines.append("%-5d %-7s %-8s | %-8.1f %-6.3f %-8.3f %-8.3f | %-16s %-16s %-6.2f | %-16s %-16s %-6.2f %-16s %.2f%s"
                             % (side, kind, filt, l3 / 1024, l3 / l2, l3 / z1, l3 / z6, B.cell(kt["level2"]), B.cell(kt["level3"]), m3 / m2,
                                B.cell(call[2]), B.cell(call[3]), c3 / B.med(call[2])[0], B.cell(host), h16 / c3, verdict(host, call[3])))
                print(lines[-1], flush=True)
            del t
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
