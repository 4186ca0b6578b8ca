"""PNG bytes of colour-coded masks -> one affinely warped class-map tensor (api.png_decode_batch_color_labels(..., warp=))
against the route there was without it, and the warp launch on its own against its two yardsticks.

Workload: 64 RGB8 mask files of 512 x 512 (blocks of 32 x 32 pixels in 21 colours, 4 distinct images from a fixed seed,
repeated), one shared map of the 21 colours; every image gets its own matrix, the matrices of tools/bench_png_warp.py: a
rotation in +-30 degrees, a scale that shrinks the 512 x 512 crop by 1.6 .. 2.3 into 224 x 224, a translation of a few pixels,
a flip for every second one.  Output: (64, 224, 224) int64, border_label 255.

    python tools/bench_png_color_labels_warp.py [--reps 8 --warmup 2] --out profiles/png_color_label_warp.txt

Four measurements, the routes of each alternating in one process:
    call:   the whole api call (host clock around a call that ends in a device synchronise);
    torch:  the route it replaces -- png_decode_batch_color_labels at the crop's size, then torch affine_grid +
            grid_sample(mode="nearest", zeros padding, align_corners=False) on a float32 copy and a cast back to int64.  That
            route computes positions in float32, so some picks differ; the line states their share.  It also loses `unmatched`;
    launch: debig_png_color_label_warp_kernel alone on resident sources (device events around one launch), MAP and PACK;
    label:  debig_png_label_warp_kernel alone on the same geometry (one-byte labels, no LUT, the same matrices and tasks);
    copy:   a device-to-device copy of the bytes the launch writes."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_png_warp as BW  # noqa: E402  (the matrices, the timing helpers and the file writer of the warp's measurement)

N_FILES, SIDE, N_DISTINCT, CLASSES, OUT = BW.N_FILES, BW.SIDE, BW.N_DISTINCT, BW.CLASSES, BW.OUT


def workload():
    """-> (files, colours (CLASSES, 3) uint8)"""
    rng = np.random.default_rng(20261019)
    colours = rng.integers(0, 256, size=(CLASSES, 3), dtype=np.uint8)
    assert len({tuple(c) for c in colours.tolist()}) == CLASSES
    masks = []
    for _ in range(N_DISTINCT):
        blocks = rng.integers(0, CLASSES, size=(SIDE // 32, SIDE // 32))
        px = colours[np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1)]
        masks.append(BW._png(px.reshape(SIDE, SIDE * 3), 2))
    return [masks[i % N_DISTINCT] for i in range(N_FILES)], colours


def _events(L):
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    return L.debig_hip_event_create(), L.debig_hip_event_create()


def launches_alone(ms, colours, reps, warmup):
    """the colour-label warp launch (MAP, PACK), the label warp launch and a device-to-device copy on resident sources of
    N_FILES images of SIDE x SIDE -> OUT int64, alternating -> ({name: [ms]}, tasks)"""
    import torch
    import png_color_label_ref as CR
    import png_warp_ref as WR
    from test_emu_png_color_labels_warp import ColorLabelWarpTask
    from test_emu_png_warp import LabelWarpTask
    from debigulator_amd import _native as N

    L = N.lib()
    L.debig_hip_png_color_label_warp_batch.restype = C.c_int
    L.debig_hip_png_color_label_warp_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    L.debig_hip_png_label_warp_batch.restype = C.c_int
    L.debig_hip_png_label_warp_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    e0, e1 = _events(L)
    H, W = OUT
    es = 8
    run = max(1, 4096 // W)
    keys = [int(k) for k in CR.pack(colours)]
    table = CR.table(keys, range(CLASSES))
    ct, lt = {0: [], 1: []}, []
    for i, m in enumerate(ms):
        q = WR.quantise([v for r in m for v in r])
        for y0 in range(0, H, run):
            geo = dict(out_off=i * H * W * es, src_pitch=SIDE, crop_w=SIDE, crop_h=SIDE, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0),
                       border_label=255, dtype=3, border_mode=0)
            for mode in (0, 1):
                t = ColorLabelWarpTask(src_off=i * SIDE * SIDE * 3, map_off=0, map_slots=len(table), missing=-1, image=i, mode=mode, **geo)
                t.m[:] = q
                ct[mode].append(t)
            t = LabelWarpTask(src_off=i * SIDE * SIDE, src_bytes=1, **geo)
            t.m[:] = q
            lt.append(t)
    n_tasks = len(lt)

    def dev(ts):
        return torch.from_numpy(np.frombuffer(bytes((type(ts[0]) * len(ts))(*ts)), np.uint8).copy()).cuda()

    d_ct, d_lt = {k: dev(v) for k, v in ct.items()}, dev(lt)
    d_tab = torch.from_numpy(np.frombuffer(table.tobytes(), np.uint8).copy()).cuda()
    d_cnt = torch.zeros(N_FILES, dtype=torch.int32, device="cuda")
    # resident sources: blocks of the 21 colours (the lookups hit), and one-byte labels of the same blocks
    rng = np.random.default_rng(3)
    blocks = np.repeat(np.repeat(rng.integers(0, CLASSES, size=(N_FILES, SIDE // 32, SIDE // 32)), 32, axis=1), 32, axis=2)
    src3 = torch.from_numpy(np.ascontiguousarray(colours[blocks]).reshape(-1)).cuda()
    src1 = torch.from_numpy(blocks.astype(np.uint8).reshape(-1)).cuda()
    out = torch.empty(N_FILES * H * W * es, dtype=torch.uint8, device="cuda")
    twin = torch.empty_like(out)
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream().cuda_stream

    def timed(fn, stream):
        L.debig_hip_event_record(e0, stream)
        rc = fn()
        L.debig_hip_event_record(e1, stream)
        assert not rc, rc
        return float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)

    routes = {
        "map": (lambda: L.debig_hip_png_color_label_warp_batch(src3.data_ptr(), out.data_ptr(), d_ct[1].data_ptr(), d_tab.data_ptr(),
                                                               d_cnt.data_ptr(), n_tasks, None), None),
        "pack": (lambda: L.debig_hip_png_color_label_warp_batch(src3.data_ptr(), out.data_ptr(), d_ct[0].data_ptr(), d_tab.data_ptr(),
                                                                None, n_tasks, None), None),
        "label": (lambda: L.debig_hip_png_label_warp_batch(src1.data_ptr(), out.data_ptr(), d_lt.data_ptr(), None, n_tasks, None), None),
        "copy": (lambda: twin.copy_(out) is None, cur),
    }
    ts = {k: [] for k in routes}
    for r in range(warmup + reps):
        for k, (fn, stream) in routes.items():
            x = timed(fn, stream)
            if r >= warmup:
                ts[k].append(x)
    L.debig_hip_event_destroy(e0)
    L.debig_hip_event_destroy(e1)
    return ts, n_tasks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    files, colours = workload()
    cmap = (colours.astype(np.int64), np.arange(CLASSES))
    ms = BW.matrices(api)
    th = torch.from_numpy(BW.theta(ms)).cuda()

    def call():
        st, t, _, um = api.png_decode_batch_color_labels(files, OUT, cmap, -1, "int64", warp=ms, border_label=255)
        return st, t, um

    def other():
        st, t, _, um = api.png_decode_batch_color_labels(files, (SIDE, SIDE), cmap, -1, "int64")
        grid = TF.affine_grid(th, (N_FILES, 1) + OUT, align_corners=False)
        x = TF.grid_sample(t.view(N_FILES, 1, SIDE, SIDE).to(torch.float32), grid, mode="nearest", padding_mode="zeros", align_corners=False)
        return st, x[:, 0].to(torch.int64), um

    st, t, um = call()
    st2, t2, _ = other()
    assert st == st2 == [0] * N_FILES and um == [0] * N_FILES and t.shape == t2.shape
    # (the torch route pads with 0, the call with 255: compare where the call did not take the border)
    differ = 100.0 * float(((t != t2) & (t != 255)).float().mean())
    tc, tt = [], []
    for r in range(a.warmup + a.reps):
        x, y = BW._timed(call), BW._timed(other)
        if r >= a.warmup:
            tc.append(x)
            tt.append(y)
    tk, n_tasks = launches_alone(ms, colours, a.reps, a.warmup)
    med = {k: BW._stat(v)[0] for k, v in tk.items()}
    lines = ["# tools/bench_png_color_labels_warp.py: %d RGB8 mask files of %d x %d (%d distinct, blocks of %d colours; %.1f MiB of files),"
             % (N_FILES, SIDE, SIDE, N_DISTINCT, CLASSES, sum(map(len, files)) / 2 ** 20),
             "# one shared map -> (%d, %d, %d) int64, one matrix per image (rotation +-30 degrees, shrinking 1.6 .. 2.3 x, translation, flips);"
             % ((N_FILES,) + OUT),
             "# %d timed runs after %d warm-up runs, routes alternating in one process; spread = (max - min) / median" % (a.reps, a.warmup),
             "# call = the whole api call; torch = png_decode_batch_color_labels at the crop's size + affine_grid + grid_sample(nearest) on a",
             "# float32 copy + cast back; both end in a device synchronise.  launch = the kernel alone on resident sources (device events),",
             "# label = debig_png_label_warp_kernel on the same geometry, copy = a device-to-device copy of the %.1f MiB the launch writes."
             % (N_FILES * OUT[0] * OUT[1] * 8 / 2 ** 20),
             "whole call        call %s | torch %s | call / torch %.3f | picks that differ %.4f %%"
             % (BW._cell(tc), BW._cell(tt), BW._stat(tc)[0] / BW._stat(tt)[0], differ),
             "launch, MAP       %s, %d tasks | label %s | launch / label %.2f | copy %s | launch / copy %.2f"
             % (BW._cell(tk["map"]), n_tasks, BW._cell(tk["label"]), med["map"] / med["label"], BW._cell(tk["copy"]), med["map"] / med["copy"]),
             "launch, PACK      %s, %d tasks | launch / label %.2f | launch / copy %.2f"
             % (BW._cell(tk["pack"]), n_tasks, med["pack"] / med["label"], med["pack"] / med["copy"])]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
