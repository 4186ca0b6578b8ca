"""Colour-coded label PNG bytes -> one integer class-map tensor (api.png_decode_batch_color_labels) against the route it replaces,
and the kernel behind it against a device-to-device copy.

Workload: 64 RGB mask files of 1024 x 1024, blocks of 32 x 32 in 21 colours (4 distinct images from a fixed seed, repeated), one
shared map of those 21 colours -> (64, 512, 512) int64.

    python tools/bench_png_color_labels.py [--reps 8 --warmup 2] --out profiles/png_color_labels.txt
        (a) whole call, the two routes alternating in one process, a device synchronise inside every timed call:
              color_labels: api.png_decode_batch_color_labels(colors=map, dtype="int64")
              torch route:  api.png_decode_batch_device(mode="rgb"), then per image a nearest index (two index tensors), a pack
                            to int64, torch.searchsorted on the sorted keys + a compare for `missing`, then torch.stack
            (the same elements: checked);
        (b) debig_png_color_label_kernel alone (device events around one launch), MAP for every dtype and PACK for int32 / int64,
            on blocky and on random-colour sources, against a device-to-device copy of the bytes it writes.
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

N_FILES, SIDE, N_DISTINCT, CLASSES, OUT = 64, 1024, 4, 21, (512, 512)


def _colours():
    rng = np.random.default_rng(7)
    return rng.integers(0, 256, size=(CLASSES, 3), dtype=np.uint8)


def _mask(rng, colours):
    blocks = rng.integers(0, CLASSES, size=(SIDE // 32, SIDE // 32))
    return colours[np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1)]


def _png(px):
    import png_spec_ref as R

    rows = np.zeros((SIDE, 1 + 3 * SIDE), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = px.reshape(SIDE, 3 * SIDE)
    return (R.SIG + R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIDE, SIDE, 8, 2, 0, 0, 0)) +
            R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b""))


def workload():
    rng = np.random.default_rng(20261017)
    colours = _colours()
    masks = [_mask(rng, colours) for _ in range(N_DISTINCT)]
    pngs = [_png(m) for m in masks]
    return [pngs[i % N_DISTINCT] for i in range(N_FILES)], masks, colours


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


def _line(name, ts, fmt="%.2f"):
    med, sp = _stat(ts)
    return ("  %-22s (ms): %s | median " + fmt + ", spread %.1f %%") % (name, " ".join(fmt % x for x in ts), med, 100 * sp)


def _events(L):
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    return L.debig_hip_event_create(), L.debig_hip_event_create()


def kernel_alone(masks, keys, reps, warmup):
    """(b): [(name, [kernel ms], [copy ms], bytes written, tasks)] -- 64 images of 1024 x 1024 RGB8 to OUT"""
    import torch
    import png_color_label_ref as CR
    import png_label_ref as LR
    from test_emu_png_color_labels import ColorLabelTask
    from debigulator_amd import _native as N

    L = N.lib()
    L.debig_hip_png_color_label_batch.restype = C.c_int
    L.debig_hip_png_color_label_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    e0, e1 = _events(L)
    H, W = OUT
    img = SIDE * SIDE * 3
    blocky = torch.from_numpy(np.concatenate([masks[i % N_DISTINCT].reshape(-1) for i in range(N_FILES)])).cuda()
    noisy = torch.randint(0, 256, (N_FILES * img,), dtype=torch.uint8, device="cuda")
    table = CR.table(keys, range(len(keys)))
    tab = np.concatenate([table.reshape(-1), LR.index(SIDE, W).astype(np.uint32), LR.index(SIDE, H).astype(np.uint32)]).astype(np.uint32)
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    sx_off = table.nbytes
    run = max(1, 16384 // W)
    res = []
    for mode, code, dtype in [(1, c, d) for c, d in enumerate(LR.DTYPES)] + [(0, 2, "int32"), (0, 3, "int64")]:
        es = 1 << code
        tasks = [ColorLabelTask(src_off=i * img, out_off=i * H * W * es, sx_off=sx_off, sy_off=sx_off + 4 * W, map_off=0, src_pitch=SIDE,
                                out_w=W, out_h=H, row0=y0, rows=min(run, H - y0), map_slots=len(table), missing=0, image=i, dtype=code,
                                mode=mode) for i in range(N_FILES) for y0 in range(0, H, run)]
        d_tasks = torch.from_numpy(np.frombuffer(bytes((ColorLabelTask * len(tasks))(*tasks)), np.uint8).copy()).cuda()
        out = torch.empty(N_FILES * H * W * es, dtype=torch.uint8, device="cuda")
        other = torch.empty_like(out)
        cnt = torch.zeros(N_FILES, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for sname, src in (("blocky", blocky), ("random", noisy)):
            kt, ct = [], []
            for r in range(warmup + reps):
                L.debig_hip_event_record(e0, None)
                rc = L.debig_hip_png_color_label_batch(src.data_ptr(), out.data_ptr(), d_tasks.data_ptr(), d_tab.data_ptr(), cnt.data_ptr(),
                                                       len(tasks), None)
                L.debig_hip_event_record(e1, None)
                assert rc == 0, rc
                k = float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                other.copy_(out)
                b.record()
                torch.cuda.synchronize()
                if r >= warmup:
                    kt.append(k)
                    ct.append(float(a.elapsed_time(b)))
            res.append(("%s %s, %s source" % ("MAP" if mode else "PACK", dtype, sname), kt, ct, out.numel(), len(tasks)))
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
    import png_label_ref as LR
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    files, masks, colours = workload()
    keys = api.png_pack_rgb(colours).astype(np.int64)
    keys, first = np.unique(keys, return_index=True)  # (sorted, and distinct should the seed ever repeat a colour)
    values = first.astype(np.int64)
    colors = (keys.astype(np.uint32), values)
    H, W = OUT
    d_keys, d_vals = torch.from_numpy(keys).cuda(), torch.from_numpy(values).cuda()

    def route_call():
        st, t, _, um = api.png_decode_batch_color_labels(files, OUT, colors, -1, "int64")
        return st, t

    def route_torch():
        outs, sts = [], []
        for st, t, inf in api.png_decode_batch_device(files, mode="rgb"):
            sy = torch.from_numpy(LR.index(inf["height"], H)).cuda()
            sx = torch.from_numpy(LR.index(inf["width"], W)).cuda()
            p = t[sy][:, sx].to(torch.int64)
            key = p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)
            k = torch.searchsorted(d_keys, key).clamp_(max=len(keys) - 1)
            outs.append(torch.where(d_keys[k] == key, d_vals[k], torch.full_like(key, -1)))
            sts.append(st)
        return sts, torch.stack(outs)

    sa, ta = route_call()
    sb, tb = route_torch()
    assert sa == sb == [0] * N_FILES and torch.equal(ta, tb)
    ts = {"color_labels": [], "torch route": []}
    for r in range(a.warmup + a.reps):
        for name, fn in (("color_labels", route_call), ("torch route", route_torch)):
            t = _timed(fn)
            if r >= a.warmup:
                ts[name].append(t)
    lines = ["# tools/bench_png_color_labels.py: %d RGB mask files of %d x %d (%d distinct, blocks of 32 x 32 in %d colours; %.1f MiB of"
             % (N_FILES, SIDE, SIDE, N_DISTINCT, CLASSES, sum(len(f) for f in files) / 2 ** 20),
             "# files), one shared map of the %d colours -> (%d, %d, %d) int64; %d timed runs after %d warm-up runs, routes / kernels"
             % (len(keys), N_FILES, H, W, a.reps, a.warmup),
             "# alternating in one process; spread = (max - min) / median",
             "# (a) whole call (ms, host clock around a call that ends in a device synchronise): color_labels =",
             "#     png_decode_batch_color_labels(colors=map, dtype=\"int64\"); torch route = png_decode_batch_device(mode=\"rgb\"), per image",
             "#     a nearest index, a pack, torch.searchsorted on the sorted keys, then torch.stack (the same elements: checked)"]
    lines += [_line(k, v) for k, v in ts.items()]
    lines.append("  ratio color_labels / torch route: %.3f (medians)" % (_stat(ts["color_labels"])[0] / _stat(ts["torch route"])[0]))
    lines += ["# (b) debig_png_color_label_kernel alone (ms, device events around one launch): %d x %d x %d RGB8 -> (%d, %d, %d),"
              % ((N_FILES, SIDE, SIDE, N_FILES) + OUT),
              "#     a %d-slot table; blocky = the masks above, random = every pixel another colour (every pick probes and misses);"
              % (2 * len(keys) if len(keys) & (len(keys) - 1) == 0 else 1 << (2 * len(keys) - 1).bit_length()),
              "#     against a device-to-device copy (torch copy_) of the bytes it writes"]
    for name, kt, ct, nbytes, n_tasks in kernel_alone(masks, [int(k) for k in keys], a.reps, a.warmup):
        lines.append("%s: %.0f MiB written, %d tasks" % (name, nbytes / 2 ** 20, n_tasks))
        lines += [_line("kernel", kt, "%.4f"), _line("copy", ct, "%.4f")]
        lines.append("  ratio kernel / copy: %.2f (medians); %.0f GB/s written" % (_stat(kt)[0] / _stat(ct)[0], nbytes / _stat(kt)[0] / 1e6))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
