"""Distance maps of a label tensor (api.png_label_distance) against a device-to-device copy of the output and against the route
there was without it: tensor -> host -> scipy.ndimage.distance_transform_edt image by image -> device.

Workload: 64 class maps of 512 x 512 and of 1024 x 1024 in device memory, uint8 and int64, three kinds of map:
    blocky   32 x 32 blocks of uniformly drawn ids (4 ids)
    random   uniformly random ids per element: every site is a neighbour
    flat     one id: the large background that a data-dependent scan would lose on (NONE under "differs"; distance 0 under to=<id>)
both modes (to=None and to=<the id of element (0, 0) of the first map>), cap none and 16, out="squared".

    python tools/bench_png_label_distance.py [--reps 8 --warmup 2 --host-reps 8 --host-warmup 2] --out profiles/png_label_distance.txt
        (a) each kernel alone (device events around one launch over the host's cut) against torch's device-to-device copy of the int32
            output, alternating;
        (b) the whole call (tasks cut and uploaded, output allocated, two launches; a device synchronise inside) against the host
            route on the same tensor, alternating: labels.cpu() -> per image distance_transform_edt(img != to) (to=None: one transform
            per id of the image, (img == id), combined) -> rint of the square, the cap -> .to(device).  The two results are compared
            for equality before anything is timed.  --host-reps / --host-warmup: the runs of the host side alone, which takes
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
SIDES, DTYPES, KINDS = (512, 1024), ("uint8", "int64"), ("blocky", "random", "flat")
CAPS = (None, 16)


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


def host_image(ndi, img, to, cap):
    """one image as a loader does it on the host today -> int32 D2 (NONE: INT32_MAX, or cap^2)"""
    none = 2 ** 31 - 1 if cap is None else cap * cap
    if to is not None:
        if not (img == to).any():
            return np.full(img.shape, none, np.int32)
        e = ndi.distance_transform_edt(img != to)
        d = np.rint(e * e).astype(np.int64)
    else:
        ids = np.unique(img)
        if ids.size == 1:
            return np.full(img.shape, none, np.int32)
        d = np.zeros(img.shape, np.int64)
        for v in ids:  # the inside distance of every class
            e = ndi.distance_transform_edt(img == v)
            d += np.rint(e * e).astype(np.int64)
    return (d if cap is None else np.minimum(d, cap * cap)).astype(np.int32)


def host_route(ndi, t, to, cap):
    import torch

    lab = t.cpu().numpy()
    return torch.from_numpy(np.stack([host_image(ndi, im, to, cap) for im in lab])).to(t.device)


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


def kernels_alone(L, ev, t, to, cap, reps, warmup):
    """(a) -> ([rows kernel ms], [cols kernel ms], [copy ms], the kernels' output)"""
    import torch
    from test_emu_png_label_distance import COLS, ColsTask, RowsTask, host_run

    n, H, W = t.shape
    es = t.element_size()
    code = {1: 0, 2: 1, 4: 2, 8: 3}[es]
    per = host_run(W)
    rt = [RowsTask(label_off=i * H * W * es, g_off=i * H * W * 2, value=0 if to is None else to, w=W, h=H, row0=y0, rows=min(per, H - y0),
                   dtype=code, sites=0 if to is None else 1) for i in range(n) for y0 in range(0, H, per)]
    ct = [ColsTask(g_off=i * H * W * 2, out_off=i * H * W * 4, w=W, h=H, x0=x0, cols=min(COLS, W - x0), cap=cap or 0, format=0)
          for i in range(n) for x0 in range(0, W, COLS)]
    d_rt = torch.from_numpy(np.frombuffer(bytes((RowsTask * len(rt))(*rt)), np.uint8).copy()).cuda()
    d_ct = torch.from_numpy(np.frombuffer(bytes((ColsTask * len(ct))(*ct)), np.uint8).copy()).cuda()
    g = torch.empty((n, H, W), dtype=torch.int16, device=t.device)
    out = torch.empty((n, H, W), dtype=torch.int32, device=t.device)
    other = torch.empty_like(out)
    e0, e1 = ev
    rts, cts, cps = [], [], []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        L.debig_hip_event_record(e0, None)
        rc = L.debig_hip_png_label_distance_rows_batch(t.data_ptr(), g.data_ptr(), d_rt.data_ptr(), len(rt), None)
        L.debig_hip_event_record(e1, None)
        assert rc == 0, rc
        kr = float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)
        L.debig_hip_event_record(e0, None)
        rc = L.debig_hip_png_label_distance_cols_batch(g.data_ptr(), out.data_ptr(), d_ct.data_ptr(), len(ct), None)
        L.debig_hip_event_record(e1, None)
        assert rc == 0, rc
        kc = float(L.debig_hip_event_elapsed_ms(e0, e1))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        other.copy_(out)
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            rts.append(kr)
            cts.append(kc)
            cps.append(float(a.elapsed_time(b)))
    return rts, cts, cps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=8)
    ap.add_argument("--host-warmup", type=int, default=2)
    ap.add_argument("--sides", type=int, nargs="*", default=list(SIDES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_label_distance.txt"))
    ap.add_argument("--quick", action="store_true", help="one size, one kind: a rehearsal of the tool, not a measurement")
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
    for name in ("debig_hip_png_label_distance_rows_batch", "debig_hip_png_label_distance_cols_batch"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
    ev = _events(L)
    tdt = {"int64": torch.int64, "uint8": torch.uint8}
    lines = ["# tools/bench_png_label_distance.py on %s: %d maps per tensor, out squared, %d timed runs after %d warm-up runs (the host route:"
             % (torch.cuda.get_device_name(0), N_MAPS, args.reps, args.warmup),
             "# %d after %d), the two sides of a comparison alternating in one process; every cell: median ms (spread = (max - min) / median)"
             % (args.host_reps, args.host_warmup),
             "# rows / cols: the two kernels alone, device events; copy: torch's device-to-device copy of the int32 output",
             "# call: api.png_label_distance whole, host clock with a device synchronise; host: tensor -> host -> scipy distance_transform_edt per",
             "#   image (to=None: per id of the image) -> device" + ("" if ndi else "  -- scipy could NOT be imported: (a) only"),
             "%-5s %-6s %-7s %-7s %-4s | %-17s %-17s %-17s %-9s | %-17s %-19s %-9s"
             % ("side", "dtype", "kind", "to", "cap", "rows ms", "cols ms", "copy ms", "both/copy", "call ms", "host ms", "host/call")]
    sides, kinds = ((512,), ("blocky",)) if args.quick else (args.sides, KINDS)
    for side in sides:
        for dtype in DTYPES:
            for kind in kinds:
                rng = np.random.default_rng(20261020 + side)
                host = maps(kind, side, rng)
                t = torch.from_numpy(host).to("cuda").to(tdt[dtype])  # (ids below 4 fit a uint8)
                for to in (None, int(host[0, 0, 0])):
                    for cap in CAPS:
                        torch.cuda.synchronize()
                        rts, cts, cps, raw = kernels_alone(L, ev, t, to, cap, args.reps, args.warmup)
                        mine = api.png_label_distance(t, to, cap)
                        assert torch.equal(mine, raw), (side, dtype, kind, to, cap)
                        at, ht = [], []
                        if ndi:  # the distinct maps through the host route: every image of the batch is compared
                            want = host_route(ndi, t[:N_DISTINCT], to, cap)
                            assert all(torch.equal(mine[i], want[i % N_DISTINCT]) for i in range(N_MAPS)), (side, dtype, kind, to, cap)
                            del want
                        for r in range(args.warmup + args.reps):
                            a = _timed(lambda: api.png_label_distance(t, to, cap))
                            if r >= args.warmup:
                                at.append(a)
                            hr = r - (args.warmup + args.reps - args.host_warmup - args.host_reps)  # the host side's runs are the last ones
                            if ndi and hr >= 0:
                                b = _timed(lambda: host_route(ndi, t, to, cap))
                                if hr >= args.host_warmup:
                                    ht.append(b)
                        rm, cm, pm, am = _stat(rts)[0], _stat(cts)[0], _stat(cps)[0], _stat(at)[0]
                        lines.append("%-5d %-6s %-7s %-7s %-4s | %-17s %-17s %-17s %-9.1f | %-17s %-19s %-9s"
                                     % (side, dtype, kind, "differs" if to is None else "to=%d" % to, cap or "-", _cell(rts), _cell(cts), _cell(cps),
                                        (rm + cm) / pm, _cell(at, "%.2f"), _cell(ht, "%.0f") if ht else "-",
                                        "%.0f" % (_stat(ht)[0] / am) if ht else "-"))
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
