"""PNG bytes -> one perspectively warped tensor (api.png_decode_batch_tensor(..., perspective=), api.png_decode_batch_labels(...,
perspective=)) against the route there was without it, and the four perspective kernels on their own against their affine twins.

Workload: 64 RGB8 files of 1024 x 1024 (smooth content with noise, 4 distinct images from a fixed seed, repeated) and 64 grey-8
label files of the same size (blocks of 21 classes), into 224 x 224 and 512 x 512.  Every image gets its own map.

    python tools/bench_png_perspective.py [--reps 8 --warmup 2] --out profiles/png_perspective.txt

KERNEL ALONE (device events around one launch on resident sources, the launches of a pair and the copy alternating; the same
task lists for both kernels of a pair, under an affine matrix -- a rotation in +-30 degrees, the shrink onto the output, a
translation -- with row 2 = (0, 0, 1), so both do identical memory work and the ratio is the price of the four 64-bit divisions
per pixel), and a device-to-device copy of the output:
    png_persp / png_warp (RGB8 -> float32 CHW, bilinear), png_persp_color / png_warp_color (the same with a colour record),
    png_label_persp / png_label_warp (bytes -> int64), png_color_label_persp / png_color_label_warp (RGB8, PACK -> int32).
WHOLE CALL (host clock around a call that ends in a device synchronise, routes alternating in one process), under a random
keystone per image:
    call:  png_decode_batch_tensor(..., perspective=) to float32 CHW with mean / std, bilinear; png_decode_batch_labels(...,
           perspective=) to int64;
    torch: the route without it -- decode to a uint8 tensor at source size, a homography grid built in torch from the same
           matrices, grid_sample(mode="bilinear" | "nearest", padding_mode="zeros", align_corners=False), normalise (images) or
           back to int64 (labels).
The torch route computes in float32, so its elements differ from the integer rule's in the last bits; each line states the largest
difference seen so that the two routes are known to do the same work."""
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

N_FILES, SIDE, N_DISTINCT, CLASSES = 64, 1024, 4, 21
OUTS = [(224, 224), (512, 512)]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _png(rows_px, ct):
    import png_spec_ref as R

    rows = np.zeros((SIDE, 1 + rows_px.shape[1]), np.uint8)  # filter type 0 on every row
    rows[:, 1:] = rows_px
    return (R.SIG + R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIDE, SIDE, 8, ct, 0, 0, 0)) +
            R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b""))


def workload():
    rng = np.random.default_rng(20261019)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    imgs, labs = [], []
    for k in range(N_DISTINCT):
        s = ((x[:, :, None] * (3 + k) + y[:, :, None] * 2 + np.arange(3) * 40) // 3 % 256 + rng.integers(0, 9, size=(SIDE, SIDE, 3))) % 256
        imgs.append(_png(s.astype(np.uint8).reshape(SIDE, SIDE * 3), 2))
        blocks = rng.integers(0, CLASSES, size=(SIDE // 32, SIDE // 32), dtype=np.uint8)
        labs.append(_png(np.repeat(np.repeat(blocks, 32, axis=0), 32, axis=1), 0))
    return [imgs[i % N_DISTINCT] for i in range(N_FILES)], [labs[i % N_DISTINCT] for i in range(N_FILES)]


def affine_maps(api, out):
    rng = np.random.default_rng(7)
    return [api.png_warp_matrix((SIDE, SIDE), out, angle=float(rng.uniform(-30, 30)), scale=out[0] / SIDE * float(rng.uniform(1.0, 1.4)),
                                translate=(float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8))), hflip=bool(i & 1)) for i in range(N_FILES)]


def keystones(api, out):
    """the source's corners, each moved by up to a fifth of the side, onto the output's corners"""
    rng = np.random.default_rng(8)
    corners = np.array([(0, 0), (SIDE, 0), (SIDE, SIDE), (0, SIDE)], np.float64)
    return [api.png_perspective_matrix(corners + rng.uniform(-0.2, 0.2, (4, 2)) * SIDE, out) for _ in range(N_FILES)]


def _stat(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def _cell(ts):
    med, sp = _stat(ts)
    return "%.3f ms (spread %.1f %%)" % (med, 100 * sp)


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _events(fns, reps, warmup):
    """device events around one call of each of fns, the calls alternating -> one list of [ms] per fn"""
    import torch

    ts = [[] for _ in fns]
    for r in range(warmup + reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ts[k].append(float(e0.elapsed_time(e1)))
    return ts


def kernels_alone(api, out, reps, warmup):
    """-> [(pair name, tasks, persp [ms], warp [ms], copy [ms])]"""
    import torch
    import map_launch as PL
    import png_warp_ref as WR
    from test_emu_png_color import ColorRec, WarpColorTask
    from test_emu_png_color_labels_warp import ColorLabelWarpTask
    from test_emu_png_warp import LabelWarpTask, WarpTask
    from debigulator_amd import _native as N

    L = N.lib()
    H, W = out
    run = max(1, 4096 // W)
    qs = [WR.quantise([v for r in m for v in r]) for m in affine_maps(api, out)]
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, T, ch, es in (("png_warp", WarpTask, 3, 4), ("png_warp_color", WarpColorTask, 3, 4), ("png_label_warp", LabelWarpTask, 1, 8),
                            ("png_color_label_warp", ColorLabelWarpTask, 3, 4)):
        tasks = []
        for i, q in enumerate(qs):
            for y0 in range(0, H, run):
                common = dict(src_off=i * SIDE * SIDE * ch, crop_w=SIDE, crop_h=SIDE, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0))
                if T in (WarpTask, WarpColorTask):
                    t = T(out_off=i * H * W * 3 * es, src_pitch=SIDE * 3, out_sx=1, out_sy=W, out_sc=H * W, channels=3, bits=8, dtype=1, filter=0,
                          border_mode=0, **common)
                    t.a[:] = [1.0 / (255.0 * (1 << 22))] * 4
                    if T is WarpColorTask:
                        t.color_off = 64 * i
                elif T is LabelWarpTask:
                    t = T(out_off=i * H * W * es, src_pitch=SIDE, border_label=255, src_bytes=1, dtype=3, border_mode=0, **common)
                else:
                    t = T(out_off=i * H * W * es, src_pitch=SIDE, border_label=-1, dtype=2, mode=0, border_mode=0, image=i, **common)
                t.m[:] = q
                tasks.append(t)
        n = len(tasks)
        warp_tasks = (T * n)(*tasks)
        persp_tasks, _ = PL.extend(warp_tasks, n, PL.PerspTail, PL.persp_fill([(0, 0, 1 << 30)] * N_FILES))
        d_warp = torch.from_numpy(np.frombuffer(bytes(warp_tasks), np.uint8).copy()).cuda()
        d_persp = torch.from_numpy(np.frombuffer(bytes(persp_tasks), np.uint8).copy()).cuda()
        src = torch.randint(0, CLASSES if ch == 1 else 256, (N_FILES * SIDE * SIDE * ch,), dtype=torch.uint8, device="cuda")
        n_out = N_FILES * H * W * (3 if T in (WarpTask, WarpColorTask) else 1) * es
        o1 = torch.empty(n_out, dtype=torch.uint8, device="cuda")
        o2 = torch.empty(n_out, dtype=torch.uint8, device="cuda")
        recs = (ColorRec * N_FILES)()
        for r in recs:
            r.k[0] = r.k[4] = r.k[8] = 65536
        extra = {"png_warp": (), "png_warp_color": (torch.from_numpy(np.frombuffer(bytes(recs), np.uint8).copy()).cuda().data_ptr(),),
                 "png_label_warp": (None,), "png_color_label_warp": (None, None)}[name]

        def launcher(kernel, d_tasks, dst):
            fn = getattr(L, "debig_hip_%s_batch" % kernel)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p] * (3 + len(extra)) + [C.c_uint32, C.c_void_p]

            def go():
                assert fn(src.data_ptr(), dst.data_ptr(), d_tasks.data_ptr(), *extra, n, stream) == 0
            return go

        o3 = torch.empty_like(o1)
        tp, tw, tc = _events([launcher(PL.TWIN["persp"][name], d_persp, o1), launcher(name, d_warp, o2), lambda: o3.copy_(o1)], 4 * reps, warmup)
        assert torch.equal(o1, o2), (name, "row 2 = (0, 0, 1) must give the warp kernel's bytes")
        rows.append((PL.TWIN["persp"][name] + " / " + name, n, tp, tw, tc))
    return rows


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
    imgs, labs = workload()
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    lines = ["# tools/bench_png_perspective.py: %d RGB8 files and %d grey-8 label files of %d x %d (%d distinct each; %.1f + %.1f MiB of files)"
             % (N_FILES, N_FILES, SIDE, SIDE, N_DISTINCT, sum(map(len, imgs)) / 2 ** 20, sum(map(len, labs)) / 2 ** 20),
             "# %d timed runs after %d warm-up runs; spread = (max - min) / median.  The divisions are the plain 64-bit operators; no" % (a.reps, a.warmup),
             "# reciprocal variant has been built or measured.",
             "# KERNEL ALONE: persp and warp on the same task lists under an affine matrix with row 2 = (0, 0, 1) (identical memory work, the",
             "# outputs compared byte for byte), copy = a device-to-device copy of the output; device events around one launch, the three",
             "# alternating, %d timed launches each." % (4 * a.reps),
             "# WHOLE CALL: call = the api call with perspective= (a random keystone per image); torch = decode at source size + homography",
             "# grid in torch + grid_sample (+ normalise); host clock, both end in a device synchronise, alternating in one process."]
    for out in OUTS:
        H, W = out
        lines.append("## -> %d x %d" % (W, H))
        for name, n, tp, tw, tc in kernels_alone(api, out, a.reps, a.warmup):
            lines.append("kernel %-44s %5d tasks | persp %s | warp %s | copy %s | persp / warp %.2f | persp / copy %.2f"
                         % (name, n, _cell(tp), _cell(tw), _cell(tc), _stat(tp)[0] / _stat(tw)[0], _stat(tp)[0] / _stat(tc)[0]))
        ms = keystones(api, out)
        Mt = torch.tensor(np.array(ms), dtype=torch.float32, device="cuda")

        def grid():
            ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32) + 0.5,
                                    torch.arange(W, device="cuda", dtype=torch.float32) + 0.5, indexing="ij")
            p = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, device="cuda")])
            q = Mt @ p
            return torch.stack([q[:, 0] / q[:, 2] * (2.0 / SIDE) - 1.0, q[:, 1] / q[:, 2] * (2.0 / SIDE) - 1.0], dim=-1).view(N_FILES, H, W, 2)

        def torch_image():
            st, t, _ = api.png_decode_batch_tensor(imgs, (SIDE, SIDE), mode="rgb", dtype="uint", layout="chw", antialias=False)
            x = TF.grid_sample(t.to(torch.float32), grid(), mode="bilinear", padding_mode="zeros", align_corners=False)
            return st, (x / 255.0 - mean) / std

        def torch_labels():
            st, t, _ = api.png_decode_batch_labels(labs, (SIDE, SIDE), dtype="uint8")
            x = TF.grid_sample(t.view(N_FILES, 1, SIDE, SIDE).to(torch.float32), grid(), mode="nearest", padding_mode="zeros", align_corners=False)
            return st, x[:, 0].to(torch.int64)

        for name, labels, call, other in (
                ("rgb8 -> float32 chw, bilinear", False,
                 lambda: api.png_decode_batch_tensor(imgs, out, mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD, perspective=ms)[:2],
                 torch_image),
                ("grey-8 labels -> int64", True, lambda: api.png_decode_batch_labels(labs, out, dtype="int64", perspective=ms)[:2], torch_labels)):
            st, t = call()
            st2, t2 = other()
            assert st == st2 == [0] * N_FILES and t2.shape == t.shape
            if labels:
                diff = "%.4f %% of picks differ" % (100.0 * float((t != t2).float().mean()))
            else:
                diff = "max |call - torch| %.4f" % float((t.float() - t2.float()).abs().max())
            del t, t2
            tc, tt = [], []
            for r in range(a.warmup + a.reps):
                x, y = _timed(call), _timed(other)
                if r >= a.warmup:
                    tc.append(x)
                    tt.append(y)
            lines.append("call   %-44s | call %s | torch %s | call / torch %.3f | %s" % (name, _cell(tc), _cell(tt), _stat(tc)[0] / _stat(tt)[0], diff))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
