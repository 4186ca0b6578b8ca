"""Per-id pixel counts and bounding boxes of a label tensor (api.png_label_stats) against a device-to-device copy of the tensor
and against the route there was without it, torch behind the decode call.

Workload: 64 class maps of 512 x 512 and of 1024 x 1024 in device memory, int64 and uint8, num_ids 21 and 256, three kinds of map:
    blocky   32 x 32 blocks of uniformly drawn ids, the generator of tools/bench_png_labels.py (a lane's open record covers whole items)
    random   uniformly random ids per element: no run to aggregate, every element closes a record into LDS
    flat     one id: every lane piles onto the same five LDS counters

    python tools/bench_png_label_stats.py [--reps 8 --warmup 2] --out profiles/png_label_stats.txt
        (a) debig_png_label_stats_kernel alone (device events around one launch over the host's task list, the records cleared in
            front of the events) against torch's device-to-device copy of the same tensor, alternating; the copy moves twice the
            bytes the kernel reads;
        (b) the whole call api.png_label_stats (tasks cut and uploaded, records cleared, launch, records copied back and converted;
            a device synchronise inside) against the torch route on the same tensor, alternating: per image torch.bincount of the
            clamped ids, then per id that occurs a mask and the min / max of the rows and columns it touches (the masks_to_boxes
            pattern), the records gathered on the host.  The two results are compared before anything is timed.
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

N_MAPS, N_DISTINCT, BLOCK = 64, 4, 32
SIDES, DTYPES, IDS, KINDS = (512, 1024), ("int64", "uint8"), (21, 256), ("blocky", "random", "flat")


def maps(kind, side, num_ids, rng):
    """(N_MAPS, side, side) int64 on the host: N_DISTINCT images from the seed, repeated"""
    out = []
    for _ in range(N_DISTINCT):
        if kind == "blocky":
            blocks = rng.integers(0, num_ids, size=(side // BLOCK, side // BLOCK))
            out.append(np.repeat(np.repeat(blocks, BLOCK, axis=0), BLOCK, axis=1))
        elif kind == "random":
            out.append(rng.integers(0, num_ids, size=(side, side)))
        else:
            out.append(np.full((side, side), int(rng.integers(0, num_ids))))
    return np.stack([out[i % N_DISTINCT] for i in range(N_MAPS)]).astype(np.int64)


def torch_route(t, num_ids):
    """the statistics as a loader computes them behind the decode call today -> int64 (N, num_ids + 1, 5)"""
    import torch

    n, H, W = t.shape
    out = np.zeros((n, num_ids + 1, 5), np.int64)
    for i in range(n):
        img = t[i].to(torch.int64)
        key = torch.where((img >= 0) & (img < num_ids), img, torch.full_like(img, num_ids))
        counts = torch.bincount(key.reshape(-1), minlength=num_ids + 1)
        present = torch.nonzero(counts).reshape(-1).tolist()
        boxes = []
        for k in present:
            m = key == k
            ys = torch.nonzero(m.any(dim=1)).reshape(-1)
            xs = torch.nonzero(m.any(dim=0)).reshape(-1)
            boxes.append(torch.stack([counts[k], xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]))
        if present:
            out[i, present] = torch.stack(boxes).cpu().numpy()
    return out


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


def kernel_alone(L, ev, t, num_ids, reps, warmup):
    """(a) -> ([kernel ms], [copy ms], tasks)"""
    import torch
    from test_emu_png_label_stats import StatsTask

    n, H, W = t.shape
    es = t.element_size()
    code = {1: 0, 2: 1, 4: 2, 8: 3}[es]
    run = max(1, 16384 // W)
    tasks = [StatsTask(label_off=(i * H + y0) * W * es, stat_off=i * (num_ids + 1) * 20, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0),
                       n_ids=num_ids, dtype=code) for i in range(n) for y0 in range(0, H, run)]
    d_tasks = torch.from_numpy(np.frombuffer(bytes((StatsTask * len(tasks))(*tasks)), np.uint8).copy()).cuda()
    stats = torch.zeros(n * (num_ids + 1) * 5, dtype=torch.int32, device="cuda")
    other = torch.empty_like(t)
    e0, e1 = ev
    kt, ct = [], []
    for r in range(warmup + reps):
        stats.zero_()
        torch.cuda.synchronize()
        L.debig_hip_event_record(e0, None)
        rc = L.debig_hip_png_label_stats_batch(t.data_ptr(), stats.data_ptr(), d_tasks.data_ptr(), len(tasks), None)
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
    return kt, ct, len(tasks), stats.cpu().numpy().view(np.uint32).reshape(n, num_ids + 1, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_label_stats.txt"))
    ap.add_argument("--quick", action="store_true", help="one size, one kind: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()

    import torch
    import png_label_stats_ref as R
    from debigulator_amd import _native as N
    from debigulator_amd import api

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L = N.lib()
    L.debig_hip_png_label_stats_batch.restype = C.c_int
    L.debig_hip_png_label_stats_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
    ev = _events(L)
    tdt = {"int64": torch.int64, "uint8": torch.uint8}
    lines = ["# tools/bench_png_label_stats.py on %s: %d maps per tensor, %d timed runs after %d warm-up runs, the two sides of a"
             % (torch.cuda.get_device_name(0), N_MAPS, args.reps, args.warmup),
             "# comparison alternating in one process; every cell: median ms (spread = (max - min) / median)",
             "# kernel: debig_png_label_stats_kernel alone, device events; copy: torch's device-to-device copy of the same tensor (it moves",
             "#   twice the bytes the kernel reads); GB/s: bytes of the tensor over the kernel's median",
             "# call: api.png_label_stats whole, host clock with a device synchronise; torch: per image bincount, per present id a mask",
             "#   and min / max of its rows and columns, on the same tensor",
             "%-6s %-6s %-4s %-7s | %-17s %-17s %-8s %-7s | %-17s %-19s %-8s"
             % ("side", "dtype", "ids", "kind", "kernel ms", "copy ms", "krn/copy", "GB/s", "call ms", "torch ms", "torch/call")]
    sides, kinds = ((512,), ("blocky",)) if args.quick else (SIDES, KINDS)
    for side in sides:
        for dtype in DTYPES:
            for num_ids in IDS:
                for kind in kinds:
                    rng = np.random.default_rng(20261020 + side + num_ids)
                    host = maps(kind, side, num_ids, rng)
                    t = torch.from_numpy(host).to("cuda").to(tdt[dtype])  # (ids up to 255 fit a uint8)
                    torch.cuda.synchronize()
                    kt, ct, n_tasks, raw = kernel_alone(L, ev, t, num_ids, args.reps, args.warmup)
                    mine = api.png_label_stats(t, num_ids)
                    theirs = torch_route(t, num_ids)
                    assert np.array_equal(mine, theirs) and np.array_equal(R.to_public(raw, side, side), mine), (side, dtype, num_ids, kind)
                    at, tt = [], []
                    for r in range(args.warmup + args.reps):
                        a = _timed(lambda: api.png_label_stats(t, num_ids))
                        b = _timed(lambda: torch_route(t, num_ids))
                        if r >= args.warmup:
                            at.append(a)
                            tt.append(b)
                    km, cm, am, tm = _stat(kt)[0], _stat(ct)[0], _stat(at)[0], _stat(tt)[0]
                    lines.append("%-6d %-6s %-4d %-7s | %-17s %-17s %-8.2f %-7.0f | %-17s %-19s %-8.1f"
                                 % (side, dtype, num_ids, kind, _cell(kt), _cell(ct), km / cm, t.numel() * t.element_size() / km / 1e6,
                                    _cell(at, "%.2f"), _cell(tt, "%.1f"), tm / am))
                    print(lines[-1], flush=True)
    for e in ev:
        L.debig_hip_event_destroy(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
