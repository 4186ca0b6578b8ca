"""Connected components of a label tensor (api.png_label_components) against a device-to-device copy of the output and against the
route there was without it: tensor -> host -> scipy.ndimage.label image by image, and value by value for a multi-class map -> device.

Workload: 64 maps of 512 x 512 and of 1024 x 1024 in device memory, uint8 (blocky and random also int64), both connectivities,
ids="consecutive", no background:
    blocky        32 x 32 blocks of uniformly drawn ids (4 ids)
    random        uniformly random ids per element: components of a few elements, about as many roots as elements
    flat          one id: one component, every run of rows one tree before the merge
  and the maps that are hard on a union-find:
    bars          one-pixel vertical bars: every column a chain that is linked element by element
    serpentine    corridors in every other row joined at alternating ends: one component whose tree is a chain of corridors
    spiral        a square spiral, one element wide: one component, the longest path an image of this size has
    checkerboard  every element its own component under 4; two components made of diagonal links only under 8

    python tools/bench_png_label_components.py [--reps 8 --warmup 2 --host-reps 2 --host-warmup 1] --out profiles/png_label_components.txt
        (a) each kernel alone (device events around one launch over the host's cut, the five in the call's order so that every merge
            starts from a fresh plane) against torch's device-to-device copy of the int32 output;
        (b) the whole call (tasks cut and uploaded, output allocated, five launches, the counts read back; a device synchronise
            inside) against the host route on the same tensor, alternating: labels.cpu() -> per image, per value of the image,
            scipy.ndimage.label(img == value, structure) with the numbers stacked -> .to(device).  The host route numbers value by
            value, the call in raster order, so before anything is timed the host result is renumbered by first element and then
            compared for equality, as are the counts.  --host-reps / --host-warmup: the runs of the host side alone, which takes
            seconds per run (the file says how many were taken).  Where scipy cannot be imported: (a) only, and the file says so.
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

N_MAPS, N_DISTINCT, BLOCK, NUM_IDS = 64, 4, 32, 4
SIDES = (512, 1024)
KINDS = ("blocky", "random", "flat", "bars", "serpentine", "spiral", "checkerboard")
BOTH_DTYPES = ("blocky", "random")
STAGES = ("rows", "merge", "count", "number", "finish")


def maps(kind, side, rng):
    """(N_MAPS, side, side) int64 on the host: N_DISTINCT images from the seed (the drawn kinds), repeated"""
    from test_emu_png_label_components import _serpentine, _spiral

    yy, xx = np.mgrid[0:side, 0:side]
    spiral = _spiral(side) if kind == "spiral" else None  # (walked element by element in python: once)
    out = []
    for k in range(N_DISTINCT):
        if kind == "blocky":
            blocks = rng.integers(0, NUM_IDS, size=(side // BLOCK, side // BLOCK))
            out.append(np.repeat(np.repeat(blocks, BLOCK, axis=0), BLOCK, axis=1))
        elif kind == "random":
            out.append(rng.integers(0, NUM_IDS, size=(side, side)))
        elif kind == "flat":
            out.append(np.full((side, side), int(rng.integers(0, NUM_IDS))))
        elif kind == "bars":
            out.append((xx + k) % 2)
        elif kind == "serpentine":
            out.append(_serpentine(side, side).astype(np.int64) if k % 2 == 0 else _serpentine(side, side)[:, ::-1].astype(np.int64))
        elif kind == "spiral":
            out.append(np.rot90(spiral, k).astype(np.int64))
        else:
            out.append((yy + xx + k) % 2)
    return np.stack([out[i % N_DISTINCT] for i in range(N_MAPS)]).astype(np.int64)


def host_image(ndi, img, structure):
    """one image as a loader does it on the host today -> (int32 ids 1 .. K, numbered value by value; K)"""
    out = np.zeros(img.shape, np.int32)
    total = 0
    for v in np.unique(img):
        lab, k = ndi.label(img == v, structure=structure)
        out[lab > 0] = lab[lab > 0] + total
        total += k
    return out, total


def host_route(ndi, t, connectivity):
    import torch

    structure = np.ones((3, 3), int) if connectivity == 8 else None
    lab = t.cpu().numpy()
    res = [host_image(ndi, im, structure) for im in lab]
    return torch.from_numpy(np.stack([r[0] for r in res])).to(t.device), [r[1] for r in res]


def in_raster_order(ids):
    """ids 1 .. K in any order -> the same sets numbered by their first element in raster order"""
    flat = ids.reshape(-1)
    _, first, inverse = np.unique(flat, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int32)
    rank[np.argsort(first)] = np.arange(1, first.size + 1, dtype=np.int32)
    return rank[inverse].reshape(ids.shape)


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


def kernels_alone(L, ev, t, connectivity, reps, warmup):
    """(a) -> ({stage: [ms]}, [copy ms], the kernels' output, the tasks' counts)"""
    import torch
    from test_emu_png_label_components import Task, host_run

    n, H, W = t.shape
    es = t.element_size()
    code = {1: 0, 2: 1, 4: 2, 8: 3}[es]
    per = host_run(W)
    n_per = -(-H // per)
    tasks = [Task(label_off=i * H * W * es, parent_off=i * H * W * 4, out_off=i * H * W * 4, background=0, w=W, h=H, row0=y0,
                  rows=min(per, H - y0), dtype=code, connectivity=connectivity, use_background=0, ids=1, count_idx=i * n_per + k,
                  count_first=i * n_per) for i in range(n) for k, y0 in enumerate(range(0, H, per))]
    d_t = torch.from_numpy(np.frombuffer(bytes((Task * len(tasks))(*tasks)), np.uint8).copy()).cuda()
    parent = torch.empty((n, H, W), dtype=torch.int32, device=t.device)
    counts = torch.zeros(len(tasks), dtype=torch.int32, device=t.device)
    out = torch.empty((n, H, W), dtype=torch.int32, device=t.device)
    other = torch.empty_like(out)
    bufs = {"rows": (t, parent), "merge": (t, parent), "count": (parent, counts), "number": (parent, counts, out), "finish": (parent, out)}
    e0, e1 = ev
    times, cps = {s: [] for s in STAGES}, []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        for s in STAGES:
            fn = getattr(L, "debig_hip_png_label_components_%s_batch" % s)
            L.debig_hip_event_record(e0, None)
            rc = fn(*[b.data_ptr() for b in bufs[s]], d_t.data_ptr(), len(tasks), None)
            L.debig_hip_event_record(e1, None)
            assert rc == 0, (s, rc)
            ms = float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)
            if r >= warmup:
                times[s].append(ms)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        other.copy_(out)
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            cps.append(float(a.elapsed_time(b)))
    return times, cps, out, counts.reshape(n, n_per).sum(dim=1).cpu().numpy()


def _write(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--host-warmup", type=int, default=1)
    ap.add_argument("--sides", type=int, nargs="*", default=list(SIDES))
    ap.add_argument("--kinds", nargs="*", default=list(KINDS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_label_components.txt"))
    ap.add_argument("--quick", action="store_true", help="one size, two kinds: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()

    import torch
    from debigulator_amd import _native as N
    from debigulator_amd import api

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    L = N.lib()
    for s in STAGES:
        fn = getattr(L, "debig_hip_png_label_components_%s_batch" % s)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * (4 if s == "number" else 3) + [C.c_uint32, C.c_void_p]
    ev = _events(L)
    tdt = {"int64": torch.int64, "uint8": torch.uint8}
    lines = ["# tools/bench_png_label_components.py on %s: %d maps per tensor, ids consecutive, no background, %d timed runs after %d warm-up runs"
             % (torch.cuda.get_device_name(0), N_MAPS, args.reps, args.warmup),
             "# (the host route: %d after %d), the two sides of a comparison alternating in one process; every cell: median ms (spread = (max - min)"
             % (args.host_reps, args.host_warmup),
             "# / median).  rows .. finish: the five kernels alone, device events; copy: torch's device-to-device copy of the int32 output;",
             "# sum/copy: the five medians over the copy's.  call: api.png_label_components whole, host clock with a device synchronise; host:",
             "# tensor -> host -> scipy.ndimage.label per image and per value of the image -> device" + (
                 "" if ndi else "  -- scipy could NOT be imported: (a) only"),
             "%-5s %-6s %-12s %-2s | %-16s %-17s %-16s %-16s %-17s %-16s %-8s | %-16s %-17s %-9s"
             % ("side", "dtype", "kind", "c", "rows ms", "merge ms", "count ms", "number ms", "finish ms", "copy ms", "sum/copy", "call ms", "host ms",
                "host/call")]
    sides, kinds = ((512,), ("blocky", "bars")) if args.quick else (args.sides, args.kinds)
    for side in sides:
        for kind in kinds:
            for dtype in (("uint8", "int64") if kind in BOTH_DTYPES and not args.quick else ("uint8",)):
                rng = np.random.default_rng(20261021 + side)
                host = maps(kind, side, rng)
                t = torch.from_numpy(host).to("cuda").to(tdt[dtype])  # (ids below 4 fit a uint8)
                for connectivity in (4, 8):
                    torch.cuda.synchronize()
                    times, cps, raw, raw_counts = kernels_alone(L, ev, t, connectivity, args.reps, args.warmup)
                    mine, counts = api.png_label_components(t, connectivity)
                    assert torch.equal(mine, raw) and counts.tolist() == raw_counts.tolist(), (side, dtype, kind, connectivity)
                    at, ht = [], []
                    if ndi:  # the distinct maps through the host route: every image of the batch is compared
                        want, wk = host_route(ndi, t[:N_DISTINCT], connectivity)
                        want = [torch.from_numpy(in_raster_order(w)).to(t.device) for w in want.cpu().numpy()]
                        assert all(torch.equal(mine[i], want[i % N_DISTINCT]) and counts[i] == wk[i % N_DISTINCT] for i in range(N_MAPS)), (
                            side, dtype, kind, connectivity)
                        del want
                    for r in range(args.warmup + args.reps):
                        a = _timed(lambda: api.png_label_components(t, connectivity))
                        if r >= args.warmup:
                            at.append(a)
                        hr = r - (args.warmup + args.reps - args.host_warmup - args.host_reps)  # the host side's runs are the last ones
                        if ndi and hr >= 0:
                            b = _timed(lambda: host_route(ndi, t, connectivity))
                            if hr >= args.host_warmup:
                                ht.append(b)
                    total = sum(_stat(times[s])[0] for s in STAGES)
                    lines.append("%-5d %-6s %-12s %-2d | %-16s %-17s %-16s %-16s %-17s %-16s %-8.1f | %-16s %-17s %-9s"
                                 % (side, dtype, kind, connectivity, _cell(times["rows"]), _cell(times["merge"]), _cell(times["count"]),
                                    _cell(times["number"]), _cell(times["finish"]), _cell(cps), total / _stat(cps)[0], _cell(at, "%.2f"),
                                    _cell(ht, "%.0f") if ht else "-", "%.0f" % (_stat(ht)[0] / _stat(at)[0]) if ht else "-"))
                    print(lines[-1], flush=True)
                    _write(args.out, lines)  # (after every line: a run that is cut short leaves what it measured)
                    del mine, raw
    for e in ev:
        L.debig_hip_event_destroy(e)
    _write(args.out, lines)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
