"""Boundary bands of a label tensor (api.png_label_boundary) against a device-to-device copy of the tensor and against the route
there was without it, torch behind the decode call.

Workload: 64 class maps of 512 x 512 and of 1024 x 1024 in device memory, uint8 and int64, mode "ring", three kinds of map:
    blocky   32 x 32 blocks of uniformly drawn ids, the generator of tools/bench_png_labels.py (11 % / 31 % / 70 % boundary at r = 1 / 3 / 8)
    random   uniformly random ids per element: nearly every element is a boundary element
    flat     one id: no boundary, every window is walked to its end
radii 1, 3 and 8 under the square, and the disk at radius 8.

    python tools/bench_png_label_boundary.py [--reps 8 --warmup 2] --out profiles/png_label_boundary.txt
        (a) debig_png_label_boundary_kernel alone (device events around one launch over the host's tile cut) against torch's
            device-to-device copy of the same tensor, alternating; both read the tensor once and write it once;
        (b) the whole call api.png_label_boundary (tiles cut and uploaded, output allocated, launch; a device synchronise inside)
            against the torch route on the same tensor, alternating, ids below 2^24 and the square only: x = labels.float(),
            boundary = max_pool2d(x) != -max_pool2d(-x) with a window of 2 r + 1 and -inf padding, torch.where(boundary, value,
            labels).  The two results are compared for equality before anything is timed.
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

N_MAPS, N_DISTINCT, BLOCK, NUM_IDS, VALUE = 64, 4, 32, 21, 255
SIDES, DTYPES, KINDS = (512, 1024), ("uint8", "int64"), ("blocky", "random", "flat")
WINDOWS = ((1, "square"), (3, "square"), (8, "square"), (8, "disk"))


def maps(kind, side, rng):
    """(N_MAPS, side, side) int64 on the host: N_DISTINCT images from the seed, repeated"""
    out = []
    for _ in range(N_DISTINCT):
        if kind == "blocky":
            blocks = rng.integers(0, NUM_IDS, size=(side // BLOCK, side // BLOCK))
            out.append(np.repeat(np.repeat(blocks, BLOCK, axis=0), BLOCK, axis=1))
        elif kind == "random":
            out.append(rng.integers(0, NUM_IDS, size=(side, side)))
        else:
            out.append(np.full((side, side), int(rng.integers(0, NUM_IDS))))
    return np.stack([out[i % N_DISTINCT] for i in range(N_MAPS)]).astype(np.int64)


def torch_route(t, radius):
    """the ring as a loader makes it behind the decode call today (square windows, ids below 2^24)"""
    import torch
    import torch.nn.functional as F

    x = t.float().unsqueeze(1)
    k = 2 * radius + 1
    b = F.max_pool2d(x, k, 1, radius) != -F.max_pool2d(-x, k, 1, radius)
    return torch.where(b.squeeze(1), torch.full_like(t, VALUE), t)


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


def _cell(ts, fmt="%.3f"):
    med, sp = _stat(ts)
    return (fmt + " (%4.1f %%)") % (med, 100 * sp)


def _events(L):
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    return L.debig_hip_event_create(), L.debig_hip_event_create()


def kernel_alone(L, ev, t, radius, shape, reps, warmup):
    """(a) -> ([kernel ms], [copy ms], tasks, the tile, the kernel's output)"""
    import torch
    import png_label_boundary_ref as R
    from test_emu_png_label_boundary import BoundaryTask, host_tile

    n, H, W = t.shape
    es = t.element_size()
    code = {1: 0, 2: 1, 4: 2, 8: 3}[es]
    tw, th = host_tile(es, radius)
    table = R.reach(radius, shape)
    tasks = []
    for i in range(n):
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                k = BoundaryTask(label_off=i * H * W * es, out_off=i * H * W * es, value=VALUE, w=W, h=H, x0=x0, y0=y0, tile_w=min(tw, W - x0),
                                 tile_h=min(th, H - y0), dtype=code, mode=0, radius=radius)
                for d, v in enumerate(table):
                    k.reach[d] = v
                tasks.append(k)
    d_tasks = torch.from_numpy(np.frombuffer(bytes((BoundaryTask * len(tasks))(*tasks)), np.uint8).copy()).cuda()
    out = torch.empty_like(t)
    other = torch.empty_like(t)
    e0, e1 = ev
    kt, ct = [], []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        L.debig_hip_event_record(e0, None)
        rc = L.debig_hip_png_label_boundary_batch(t.data_ptr(), out.data_ptr(), d_tasks.data_ptr(), len(tasks), None)
        L.debig_hip_event_record(e1, None)
        assert rc == 0, rc
        k = float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        other.copy_(t)
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            kt.append(k)
            ct.append(float(a.elapsed_time(b)))
    return kt, ct, len(tasks), (tw, th), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_label_boundary.txt"))
    ap.add_argument("--quick", action="store_true", help="one size, one kind: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()

    import torch
    from debigulator_amd import _native as N
    from debigulator_amd import api

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L = N.lib()
    L.debig_hip_png_label_boundary_batch.restype = C.c_int
    L.debig_hip_png_label_boundary_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
    ev = _events(L)
    tdt = {"int64": torch.int64, "uint8": torch.uint8}
    lines = ["# tools/bench_png_label_boundary.py on %s: %d maps per tensor, mode ring, %d timed runs after %d warm-up runs, the two sides"
             % (torch.cuda.get_device_name(0), N_MAPS, args.reps, args.warmup),
             "# of a comparison alternating in one process; every cell: median ms (spread = (max - min) / median)",
             "# kernel: debig_png_label_boundary_kernel alone, device events; copy: torch's device-to-device copy of the same tensor (both",
             "#   read it once and write it once); GB/s: twice the bytes of the tensor over the kernel's median; bnd: boundary elements",
             "# call: api.png_label_boundary whole, host clock with a device synchronise; torch: float() -> max_pool2d != -max_pool2d(-x) ->",
             "#   where, on the same tensor, square windows only ('-': not a square, no torch route)",
             "%-5s %-6s %-7s %-9s %-7s %-5s | %-17s %-17s %-8s %-6s | %-17s %-17s %-8s"
             % ("side", "dtype", "kind", "window", "tile", "bnd %", "kernel ms", "copy ms", "krn/copy", "GB/s", "call ms", "torch ms", "torch/call")]
    sides, kinds = ((512,), ("blocky",)) if args.quick else (SIDES, KINDS)
    for side in sides:
        for dtype in DTYPES:
            for kind in kinds:
                rng = np.random.default_rng(20261020 + side)
                host = maps(kind, side, rng)
                t = torch.from_numpy(host).to("cuda").to(tdt[dtype])  # (ids below 21 fit a uint8)
                for radius, shape in WINDOWS:
                    torch.cuda.synchronize()
                    kt, ct, n_tasks, tile, raw = kernel_alone(L, ev, t, radius, shape, args.reps, args.warmup)
                    mine = api.png_label_boundary(t, radius, shape, "ring", VALUE)
                    assert torch.equal(mine, raw), (side, dtype, kind, radius, shape)
                    bnd = 100.0 * float((mine != t).float().mean())  # (no id is 255)
                    at, tt = [], []
                    if shape == "square":
                        assert torch.equal(mine, torch_route(t, radius)), (side, dtype, kind, radius)
                    for r in range(args.warmup + args.reps):
                        a = _timed(lambda: api.png_label_boundary(t, radius, shape, "ring", VALUE))
                        b = _timed(lambda: torch_route(t, radius)) if shape == "square" else 0.0
                        if r >= args.warmup:
                            at.append(a)
                            tt.append(b)
                    km, cm, am = _stat(kt)[0], _stat(ct)[0], _stat(at)[0]
                    lines.append("%-5d %-6s %-7s %-9s %-7s %-5.1f | %-17s %-17s %-8.2f %-6.0f | %-17s %-17s %-8s"
                                 % (side, dtype, kind, "%s %d" % (shape, radius), "%dx%d" % tile, bnd, _cell(kt), _cell(ct), km / cm,
                                    2 * t.numel() * t.element_size() / km / 1e6, _cell(at, "%.2f"),
                                    _cell(tt, "%.2f") if shape == "square" else "-",
                                    "%.1f" % (_stat(tt)[0] / am) if shape == "square" else "-"))
                    print(lines[-1], flush=True)
                    del mine, raw
    for e in ev:
        L.debig_hip_event_destroy(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
