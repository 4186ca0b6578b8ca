"""Label PNG bytes -> one integer class-map tensor (api.png_decode_batch_labels) against the only route there was without it,
and the two kernels behind it against their nearest relatives.

Workload: 64 label files of 1024 x 1024 -- 32 of 8-bit palette (21 entries) and 32 of 8-bit grey, blocky content of 21 classes
(4 distinct images each from a fixed seed, repeated) -> (64, 512, 512) int64.

    python tools/bench_png_labels.py [--reps 8 --warmup 2] --out profiles/png_labels.txt
        (a) whole call, the two routes alternating in one process, a device synchronise inside every timed call, on the grey-8
            half (the other route cannot read a palette index):
              labels: api.png_decode_batch_labels(dtype="int64")
              tensor: api.png_decode_batch_tensor(mode="gray", dtype="uint", filter="nearest") followed by .to(torch.int64)
            and the labels route on all 64 files;
        (b) debig_png_label_gather_kernel alone (device events around one launch) for every dtype, against a device-to-device
            copy of the bytes it writes;
        (c) debig_png_spec_defilter_index_kernel against its output-format twin writing GRAY8, on the same grey-8 task list.
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


def _labels(rng):
    blocks = rng.integers(0, CLASSES, size=(SIDE // 32, SIDE // 32), dtype=np.uint8)
    return np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1)


def _png(lab, ct):
    import png_spec_ref as R

    rows = np.zeros((SIDE, 1 + SIDE), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = lab
    out = R.SIG + R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIDE, SIDE, 8, ct, 0, 0, 0))
    if ct == 3:
        out += R.chunk(b"PLTE", bytes((37 * k + 11 * c) % 256 for k in range(CLASSES) for c in range(3)))
    return out + R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b"")


def workload():
    rng = np.random.default_rng(20261017)
    labs = [_labels(rng) for _ in range(N_DISTINCT)]
    grey = [_png(labs[i % N_DISTINCT], 0) for i in range(N_FILES // 2)]
    pal = [_png(labs[i % N_DISTINCT], 3) for i in range(N_FILES // 2)]
    return grey, pal, labs


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


def gather_alone(reps, warmup):
    """(b): {dtype: ([kernel ms], [copy ms], bytes written)} -- 64 images of 1024 x 1024 one-byte labels to OUT"""
    import torch
    import png_label_ref as LR
    from test_emu_png_labels import LabelTask
    from debigulator_amd import _native as N

    L = N.lib()
    L.debig_hip_png_label_gather_batch.restype = C.c_int
    L.debig_hip_png_label_gather_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    e0, e1 = _events(L)
    H, W = OUT
    src = torch.randint(0, CLASSES, (N_FILES * SIDE * SIDE,), dtype=torch.uint8, device="cuda")
    tab = np.concatenate([LR.index(SIDE, W), LR.index(SIDE, H)]).astype(np.uint32)
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    run = max(1, 16384 // W)
    res = {}
    for code, dtype in enumerate(LR.DTYPES):
        es = 1 << code
        tasks = [LabelTask(src_off=i * SIDE * SIDE, out_off=i * H * W * es, sx_off=0, sy_off=4 * W, src_pitch=SIDE, out_w=W, out_h=H,
                           row0=y0, rows=min(run, H - y0), src_bytes=1, dtype=code) for i in range(N_FILES) for y0 in range(0, H, run)]
        d_tasks = torch.from_numpy(np.frombuffer(bytes((LabelTask * len(tasks))(*tasks)), np.uint8).copy()).cuda()
        out = torch.empty(N_FILES * H * W * es, dtype=torch.uint8, device="cuda")
        other = torch.empty_like(out)
        torch.cuda.synchronize()
        kt, ct = [], []
        for r in range(warmup + reps):
            L.debig_hip_event_record(e0, None)
            rc = L.debig_hip_png_label_gather_batch(src.data_ptr(), out.data_ptr(), d_tasks.data_ptr(), d_tab.data_ptr(), None, len(tasks), None)
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
        res[dtype] = (kt, ct, out.numel(), len(tasks))
    L.debig_hip_event_destroy(e0)
    L.debig_hip_event_destroy(e1)
    return res


def defilter_alone(labs, reps, warmup):
    """(c): {kernel: [ms]} -- the grey-8 half as scanline streams in device memory, one task list for both kernels"""
    import torch
    from test_emu_png_out_format import SpecTask
    from test_emu_png_spec import SpecResult
    from debigulator_amd import _native as N

    L = N.lib()
    for f in (L.debig_hip_png_spec_defilter_index_batch, L.debig_hip_png_spec_defilter_fmt_batch):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    e0, e1 = _events(L)
    n = N_FILES // 2
    stream = SIDE * (SIDE + 1)
    pitch = (stream + 15) // 16 * 16 + 32
    ring = 4 * ((SIDE + 15) // 16 * 16 + 16)
    arena = np.zeros(64 + n * (pitch + ring) + 64, np.uint8)
    tasks = []
    for i in range(n):
        rows = np.zeros((SIDE, 1 + SIDE), np.uint8)
        rows[:, 0] = np.arange(SIDE) % 5  # every filter type (the bytes are then not the labels: only the time is read)
        rows[:, 1:] = labs[i % N_DISTINCT]
        arena[64 + i * pitch: 64 + i * pitch + stream] = rows.reshape(-1)
        tasks.append(SpecTask(stream_off=64 + i * pitch, rgba_off=i * SIDE * SIDE, pal_off=0, scratch_off=64 + n * pitch + i * ring,
                              width=SIDE, height=SIDE, img_width=SIDE, x0=0, y0=0, dx=1, dy=1, bpp_f=1, depth=8, color_type=0,
                              channels=1, out_fmt=2))
    d_arena = torch.from_numpy(arena).cuda()
    d_tasks = torch.from_numpy(np.frombuffer(bytes((SpecTask * n)(*tasks)), np.uint8).copy()).cuda()
    d_res = torch.zeros(n * C.sizeof(SpecResult), dtype=torch.uint8, device="cuda")
    out = torch.empty(n * SIDE * SIDE + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"index": [], "fmt GRAY8": []}
    outs = {}
    for r in range(warmup + reps):
        for name, fn in (("index", L.debig_hip_png_spec_defilter_index_batch), ("fmt GRAY8", L.debig_hip_png_spec_defilter_fmt_batch)):
            L.debig_hip_event_record(e0, None)
            rc = fn(d_arena.data_ptr(), out.data_ptr(), d_tasks.data_ptr(), d_res.data_ptr(), n, None)
            L.debig_hip_event_record(e1, None)
            assert rc == 0, rc
            ms = float(L.debig_hip_event_elapsed_ms(e0, e1))
            if r >= warmup:
                res[name].append(ms)
            if r == 0:
                outs[name] = out.clone()
                assert not d_res.cpu().numpy().view(np.uint32)[0::2].any()
    assert torch.equal(outs["index"], outs["fmt GRAY8"])  # grey 8 without a key: the same bytes
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
    grey, pal, labs = workload()
    both = [f for pair in zip(grey, pal) for f in pair]

    def route_labels(files):
        return api.png_decode_batch_labels(files, OUT, dtype="int64")[:2]

    def route_tensor(files):
        st, t, _ = api.png_decode_batch_tensor(files, OUT, mode="gray", dtype="uint", layout="hwc", filter="nearest")
        return st, t[..., 0].to(torch.int64)

    sa, ta = route_labels(grey)
    sb, tb = route_tensor(grey)
    assert sa == sb == [0] * len(grey) and torch.equal(ta, tb)
    assert route_labels(both)[0] == [0] * N_FILES
    ts = {"labels": [], "tensor + .to(int64)": [], "labels, all 64 files": []}
    for r in range(a.warmup + a.reps):
        for name, fn in (("labels", lambda: route_labels(grey)), ("tensor + .to(int64)", lambda: route_tensor(grey)),
                         ("labels, all 64 files", lambda: route_labels(both))):
            t = _timed(fn)
            if r >= a.warmup:
                ts[name].append(t)
    lines = ["# tools/bench_png_labels.py: %d label files of %d x %d (half 8-bit palette of %d entries, half 8-bit grey; %d distinct,"
             % (N_FILES, SIDE, SIDE, CLASSES, N_DISTINCT),
             "# blocks of 32 x 32 of %d classes; %.1f MiB of files) -> (%d, %d, %d) int64; %d timed runs after %d warm-up runs, routes /"
             % (CLASSES, sum(len(f) for f in both) / 2 ** 20, N_FILES, OUT[0], OUT[1], a.reps, a.warmup),
             "# kernels alternating in one process; spread = (max - min) / median",
             "# (a) whole call (ms, host clock around a call that ends in a device synchronise), the %d grey-8 files: labels ="
             % len(grey),
             "#     png_decode_batch_labels(dtype=\"int64\"); tensor = png_decode_batch_tensor(mode=\"gray\", dtype=\"uint\",",
             "#     filter=\"nearest\") then .to(torch.int64) (the same elements: checked); and the labels route on all %d files" % N_FILES]
    lines += [_line(k, v) for k, v in ts.items()]
    lines.append("  ratio labels / tensor route: %.3f (medians)" % (_stat(ts["labels"])[0] / _stat(ts["tensor + .to(int64)"])[0]))
    lines += ["# (b) debig_png_label_gather_kernel alone (ms, device events around one launch): %d x %d x %d one-byte labels ->"
              % (N_FILES, SIDE, SIDE),
              "#     (%d, %d, %d) of each dtype, against a device-to-device copy (torch copy_) of the bytes it writes" % ((N_FILES,) + OUT)]
    for dtype, (kt, ct, nbytes, n_tasks) in gather_alone(a.reps, a.warmup).items():
        lines.append("%s: %.0f MiB written, %d tasks" % (dtype, nbytes / 2 ** 20, n_tasks))
        lines += [_line("gather", kt, "%.4f"), _line("copy", ct, "%.4f")]
        lines.append("  ratio gather / copy: %.2f (medians); %.0f GB/s written" % (_stat(kt)[0] / _stat(ct)[0], nbytes / _stat(kt)[0] / 1e6))
    lines += ["# (c) debig_png_spec_defilter_index_kernel against debig_png_spec_defilter_fmt_kernel writing GRAY8 (ms, device events",
              "#     around one launch): the %d grey-8 images as scanline streams in device memory, filter types y %% 5, one task list"
              % (N_FILES // 2)]
    res = defilter_alone(labs, a.reps, a.warmup)
    lines += [_line(k, v, "%.4f") for k, v in res.items()]
    lines.append("  ratio index / fmt: %.3f (medians)" % (_stat(res["index"])[0] / _stat(res["fmt GRAY8"])[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
