"""Level 2 of the PNG encode (api.png_encode_batch_dyn: one dynamic Huffman block per chunk) against level 1 and against zlib, on
the cells of tools/bench_png_encode.py / profiles/png_encode.txt: 64 images of 512 x 512 and of 1024 x 1024 in device memory --
photographs, noise, a blocky palette map, 16-bit instance ids --, filter adaptive, and filter none for the two label workloads.

    python tools/bench_png_encode_dyn.py [--reps 6 --warmup 2 --host-reps 3] --out profiles/png_encode_dyn.txt
        (a) size: the DEFLATE bytes of the level-2 files over zlib.compress(stream, 1) on the same filtered streams and over the
            level-1 files', and the share of chunks whose task wrote a dynamic block (BTYPE of the first block of every slot);
        (b) kernels alone (device events around one launch over the host's cut): the dynamic kernel, the same under
            DEBIG_PNG_ENCODE_ONLY_DYNAMIC, the level-1 kernel of THIS tree on the same tasks (the parent commit's level-1 times are in
            profiles/png_encode.txt), and torch's device-to-device copy of the filtered streams; build + emit: the ONLY_DYNAMIC run
            minus the level-1 run (both run the same matcher; level 1 emits while it matches);
        (c) the whole call at level 2 against level 1 (host clock, the call synchronises) and against tensor.cpu() + Pillow
            save(compress_level=1) per image on 16 threads; a cell where the host route wins is marked MISS.
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


def kernels_alone(t, reps, warmup, filt, kw):
    """-> ({name: [ms]}, stream bytes, the share of tasks whose first block is dynamic)"""
    import torch

    import png_encode_dyn_ref as D
    import png_encode_ref as R
    import test_emu_png_encode as E
    import test_emu_png_encode_dyn as Y
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
    ft, d1, d2, d3, at, tk = [], [], [], [], 0, 0
    img_bytes = H * W * Cn * t.element_size()
    for i in range(n):
        for y0, r in R.row_runs(H, rb):
            ft.append(E.FTask(image_off=i * img_bytes, stream_off=i * slen, w=W, h=H, row0=y0, rows=r, channels=Cn, dtype=dtype, depth=depth,
                              layout=0, filter=filt, palette_entries=21 if "palette" in kw else 0, flag_idx=i))
        cuts = R.chunks(slen)
        for k, (off, ln) in enumerate(cuts):
            common = dict(stream_off=i * slen, stream_len=slen, chunk_off=off, slot_off=at, chunk_len=ln, slot_cap=R.slot_bytes(ln),
                          bpp=Cn * depth // 8, last=int(k == len(cuts) - 1), count_idx=len(d1))
            d1.append(E.DTask(level=1, **common))
            d2.append(Y.YTask(level=2, token_off=tk, token_cap=4 * R.CHUNK, **common))
            d3.append(Y.YTask(level=2, token_off=tk, token_cap=4 * R.CHUNK, flags=D.ONLY_DYNAMIC, **common))
            at += R.slot_bytes(ln)
            tk += 4 * R.CHUNK
    slots = torch.empty(at, dtype=torch.uint8, device=t.device)
    tokens = torch.empty(tk, dtype=torch.uint8, device=t.device)
    counts = torch.zeros(len(d1), dtype=torch.int32, device=t.device)

    def up(tasks, cls):
        return torch.frombuffer(bytearray(bytes((cls * len(tasks))(*tasks))), dtype=torch.uint8).to(t.device)

    d_ft, d_1, d_2, d_3 = up(ft, E.FTask), up(d1, E.DTask), up(d2, Y.YTask), up(d3, Y.YTask)
    for fn in (L.debig_hip_png_encode_filter_batch, L.debig_hip_png_encode_deflate_batch):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    L.debig_hip_png_encode_dynamic_batch.restype = C.c_int
    L.debig_hip_png_encode_dynamic_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    assert L.debig_hip_png_encode_filter_batch(t.data_ptr(), streams.data_ptr(), d_ft.data_ptr(), flags.data_ptr(), len(ft), stream) == 0
    torch.cuda.synchronize()
    copy_st = torch.empty_like(streams)

    def dyn(tasks):
        return lambda: L.debig_hip_png_encode_dynamic_batch(streams.data_ptr(), slots.data_ptr(), tokens.data_ptr(), tasks.data_ptr(), counts.data_ptr(),
                                                            len(d1), stream)

    runs = {"level1": lambda: L.debig_hip_png_encode_deflate_batch(streams.data_ptr(), slots.data_ptr(), d_1.data_ptr(), counts.data_ptr(), len(d1), stream),
            "only_dynamic": dyn(d_3), "dynamic": dyn(d_2), "copy_s": lambda: copy_st.copy_(streams)}
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
        if name == "dynamic":  # BTYPE of the first block of every slot
            first = slots[torch.tensor([d.slot_off for d in d1], device=t.device)].cpu().numpy()
            share = float((((first >> 1) & 3) == 2).mean())
    return out, n * slen, share


def payload(d):
    at = d.index(b"IDAT") + 4
    ln = int.from_bytes(d[at - 8: at - 4], "big")
    return d[at: at + ln]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="*", default=list(B.SIDES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_dyn.txt"))
    a = ap.parse_args()
    import torch

    from debigulator_amd import api

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    lines = ["# tools/bench_png_encode_dyn.py on %s: %d images per tensor, %d timed runs after %d warm-up runs (the host route: %d after 1);"
             % (torch.cuda.get_device_name(0), B.N_IMAGES, a.reps, a.warmup, a.host_reps),
             "# every time: median ms (spread = (max - min) / median).  L2/zlib1, L2/L1: DEFLATE bytes of the level-2 files over zlib.compress(stream, 1)",
             "# on the same filtered streams / over the level-1 files'; dyn: the share of chunks written as a dynamic block.  level1, dynamic, only_dyn:",
             "# the kernels alone on the same tasks, device events (level1: this tree's; the parent commit's are in profiles/png_encode.txt); copy_s: torch's",
             "# device-to-device copy of the filtered streams; b+e: only_dyn - level1, the build and emit phases.  call L1 / L2: api.png_encode_batch(level=1) /",
             "# api.png_encode_batch_dyn whole, host clock; host16: tensor.cpu() + Pillow save(compress_level=1) per image on 16 threads; MISS: the host route wins.",
             "# No hardware counters were collected.",
             "side  kind    filter   | L2/zlib1 L2/L1  dyn   | level1 ms        dynamic ms       only_dyn ms      copy_s ms        dyn/L1 x copy  b+e ms | "
             "call L1 ms       call L2 ms       L2/L1  host16 ms        host16/L2"]
    for side in a.sides:
        for kind in ("photo", "noise", "labels", "ids"):
            t, kw = B.workload(kind, side, rng, api, dev)
            for filt in (("adaptive", "none") if kind in ("labels", "ids") else ("adaptive",)):
                host = []
                for k in range(1 + a.host_reps):
                    t0 = time.perf_counter()
                    B.pillow_route(t, kw, 16)
                    if k:
                        host.append(1e3 * (time.perf_counter() - t0))
                call, files = {}, {}
                for level, fn in ((1, api.png_encode_batch), (2, api.png_encode_batch_dyn)):
                    ms = []
                    for k in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        res = fn(t, filter=filt, level=level, **kw)
                        if k >= a.warmup:
                            ms.append(1e3 * (time.perf_counter() - t0))
                    assert all(s == 0 for s, _ in res)
                    call[level], files[level] = ms, [d for _, d in res[:B.N_DISTINCT]]
                l1 = l2 = zl = 0
                for d1, d2 in zip(files[1], files[2]):
                    z1, z2 = payload(d1), payload(d2)
                    stream = zlib.decompress(z2)
                    assert stream == zlib.decompress(z1)
                    l1 += len(z1) - 6
                    l2 += len(z2) - 6
                    zl += len(zlib.compress(stream, 1)) - 6
                kt, sb, share = kernels_alone(t, a.reps, a.warmup, api.PNG_ENCODE_FILTERS[filt], kw)
                m1, m2, m3, mc = (B.med(kt[k])[0] for k in ("level1", "dynamic", "only_dynamic", "copy_s"))
                h16, c2 = B.med(host)[0], B.med(call[2])[0]
                lines.append("%-5d %-7s %-8s | %-8.3f %-6.3f %-5.2f | %-16s %-16s %-16s %-16s %-6.2f %-7.0f %-6.2f | %-16s %-16s %-6.2f %-16s %.2f%s"
                             % (side, kind, filt, l2 / zl, l2 / l1, share, B.cell(kt["level1"]), B.cell(kt["dynamic"]), B.cell(kt["only_dynamic"]),
                                B.cell(kt["copy_s"]), m2 / m1, m2 / mc, m3 - m1, B.cell(call[1]), B.cell(call[2]), c2 / B.med(call[1])[0], B.cell(host),
                                h16 / c2, "  MISS" if h16 < c2 else ""))
                print(lines[-1], flush=True)
            del t
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
