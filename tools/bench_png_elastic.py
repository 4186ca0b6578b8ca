"""PNG bytes -> one elastically deformed tensor (api.png_decode_batch_tensor(..., elastic=), api.png_decode_batch_labels(...,
elastic=)) against the route there was without it, and the four elastic kernels on their own against their affine twins.

Workload (tools/bench_png_perspective.py's): 64 RGB8 files of 1024 x 1024 and 64 grey-8 label files of the same size, into 224 x 224
and 512 x 512.  Every image gets its own affine map (a rotation in +-30 degrees, the shrink onto the output, a translation) and its
own field of 17 x 17 nodes (png_elastic_field: alpha 12 output pixels, sigma two node spacings).

    python tools/bench_png_elastic.py [--reps 8 --warmup 2] --out profiles/png_elastic.txt

KERNEL ALONE (device events around one launch on resident sources, the launches of a pair and the copy alternating; the same
task lists for both kernels of a pair -- the elastic one reads its field on top, so the ratio is the price of staging the grid and
of the per-pixel interpolation; with a field of zeros the two outputs are first compared byte for byte), and a device-to-device copy
of the output:
    png_elastic / png_warp (RGB8 -> float32 CHW, bilinear), png_elastic_color / png_warp_color (the same with a colour record),
    png_label_elastic / png_label_warp (bytes -> int64), png_color_label_elastic / png_color_label_warp (RGB8, PACK -> int32).
WHOLE CALL (host clock around a call that ends in a device synchronise, routes alternating in one process):
    call:  png_decode_batch_tensor(..., warp=, elastic=) to float32 CHW with mean / std, bilinear; png_decode_batch_labels(...,
           warp=, elastic=) to int64;
    torch: the route without it -- decode to a uint8 tensor at source size, the fields upsampled to the output with
           F.interpolate(mode="bicubic", align_corners=True), the displaced pixel centres through the same matrices into a grid,
           grid_sample(mode="bilinear" | "nearest", padding_mode="zeros", align_corners=False), normalise (images) or back to int64
           (labels).
The torch route computes in float32 and places its nodes slightly differently (align_corners=True puts the end nodes on the end
pixels' centres, the rule puts them on the output's edges), so its elements differ from the integer rule's; each line states the
difference seen so that the two routes are known to do the same work."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_png_perspective as B  # noqa: E402  (the workload, the affine maps, the timers)

N_FILES, SIDE, CLASSES = B.N_FILES, B.SIDE, B.CLASSES
OUTS, MEAN, STD = B.OUTS, B.MEAN, B.STD
GRID = (17, 17)


def fields(api, out, zeros=False):
    if zeros:
        return [np.zeros(GRID + (2,)) for _ in range(N_FILES)]
    return [api.png_elastic_field(out, alpha=12.0, sigma=2.0 * out[0] / (GRID[0] - 1), grid=GRID, rng=100 + i) for i in range(N_FILES)]


def kernels_alone(api, out, reps, warmup):
    """-> [(pair name, tasks, elastic [ms], warp [ms], copy [ms])]"""
    import torch
    import map_launch as EL
    import png_elastic_ref as ER
    import png_warp_ref as WR
    from test_emu_png_color import ColorRec, WarpColorTask
    from test_emu_png_color_labels_warp import ColorLabelWarpTask
    from test_emu_png_warp import LabelWarpTask, WarpTask
    from debigulator_amd import _native as N

    L = N.lib()
    H, W = out
    run = max(1, 4096 // W)
    qs = [WR.quantise([v for r in m for v in r]) for m in B.affine_maps(api, out)]
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
        d_warp = torch.from_numpy(np.frombuffer(bytes(warp_tasks), np.uint8).copy()).cuda()
        src = torch.randint(0, CLASSES if ch == 1 else 256, (N_FILES * SIDE * SIDE * ch,), dtype=torch.uint8, device="cuda")
        n_out = N_FILES * H * W * (3 if T in (WarpTask, WarpColorTask) else 1) * es
        o1 = torch.empty(n_out, dtype=torch.uint8, device="cuda")
        o2 = torch.empty(n_out, dtype=torch.uint8, device="cuda")
        recs = (ColorRec * N_FILES)()
        for r in recs:
            r.k[0] = r.k[4] = r.k[8] = 65536
        d_recs = torch.from_numpy(np.frombuffer(bytes(recs), np.uint8).copy()).cuda()  # (held: the launches below read it)
        extra = {"png_warp": (), "png_warp_color": (d_recs.data_ptr(),),
                 "png_label_warp": (None,), "png_color_label_warp": (None, None)}[name]

        def launcher(kernel, d_tasks, dst, more=()):
            fn = getattr(L, "debig_hip_%s_batch" % kernel)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p] * (3 + len(extra) + len(more)) + [C.c_uint32, C.c_void_p]

            def go():
                assert fn(src.data_ptr(), dst.data_ptr(), d_tasks.data_ptr(), *extra, *more, n, stream) == 0
            return go

        def elastic(zeros):
            buf, offs = EL.fields_buffer([ER.quantise_field(f) for f in fields(api, out, zeros)], lead=0)
            d_fields = torch.from_numpy(buf.copy()).cuda()
            d_tasks = torch.from_numpy(np.frombuffer(bytes(EL.extend(warp_tasks, n, EL.ElasticTail, EL.elastic_fill(offs, GRID))[0]), np.uint8).copy()).cuda()
            return launcher(EL.TWIN["elastic"][name], d_tasks, o1, (d_fields.data_ptr(),)), (d_fields, d_tasks)

        warp = launcher(name, d_warp, o2)
        go, keep = elastic(True)
        go()
        warp()
        torch.cuda.synchronize()
        assert torch.equal(o1, o2), (name, "a field of zeros must give the warp kernel's bytes")
        go, keep = elastic(False)
        o3 = torch.empty_like(o1)
        te, tw, tc = B._events([go, warp, lambda: o3.copy_(o1)], 4 * reps, warmup)
        rows.append((EL.TWIN["elastic"][name] + " / " + name, n, te, tw, tc))
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
    imgs, labs = B.workload()
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    lines = ["# tools/bench_png_elastic.py: %d RGB8 files and %d grey-8 label files of %d x %d (%d distinct each; %.1f + %.1f MiB of files)"
             % (N_FILES, N_FILES, SIDE, SIDE, B.N_DISTINCT, sum(map(len, imgs)) / 2 ** 20, sum(map(len, labs)) / 2 ** 20),
             "# %d timed runs after %d warm-up runs; spread = (max - min) / median.  Fields of %d x %d nodes, one per image." % (a.reps, a.warmup, GRID[1], GRID[0]),
             "# KERNEL ALONE: elastic and warp on the same task lists and matrices (with a field of zeros the outputs are first compared byte",
             "# for byte), copy = a device-to-device copy of the output; device events around one launch, the three alternating, %d timed" % (4 * a.reps),
             "# launches each.",
             "# WHOLE CALL: call = the api call with warp= and elastic=; torch = decode at source size + F.interpolate(field, bicubic) + the grid",
             "# in torch + grid_sample (+ normalise); host clock, both end in a device synchronise, alternating in one process."]
    for out in OUTS:
        H, W = out
        lines.append("## -> %d x %d" % (W, H))
        print("measuring -> %d x %d ..." % (W, H), file=sys.stderr, flush=True)
        for name, n, te, tw, tc in kernels_alone(api, out, a.reps, a.warmup):
            lines.append("kernel %-50s %5d tasks | elastic %s | warp %s | copy %s | elastic / warp %.2f | elastic / copy %.2f"
                         % (name, n, B._cell(te), B._cell(tw), B._cell(tc), B._stat(te)[0] / B._stat(tw)[0], B._stat(te)[0] / B._stat(tc)[0]))
        ms = B.affine_maps(api, out)
        fs = fields(api, out)
        Mt = torch.tensor(np.array(ms), dtype=torch.float32, device="cuda")  # (N, 2, 3)
        Ft = torch.tensor(np.array(fs), dtype=torch.float32, device="cuda").permute(0, 3, 1, 2).contiguous()  # (N, 2, gh, gw)

        def grid():
            d = TF.interpolate(Ft, size=(H, W), mode="bicubic", align_corners=True)
            ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32) + 0.5,
                                    torch.arange(W, device="cuda", dtype=torch.float32) + 0.5, indexing="ij")
            p = torch.stack([(xs[None] + d[:, 0]).reshape(N_FILES, -1), (ys[None] + d[:, 1]).reshape(N_FILES, -1),
                             torch.ones(N_FILES, H * W, device="cuda")], dim=1)  # (N, 3, H W)
            q = torch.bmm(Mt, p)
            return (q * (2.0 / SIDE) - 1.0).permute(0, 2, 1).reshape(N_FILES, H, W, 2)

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
                 lambda: api.png_decode_batch_tensor(imgs, out, mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD, warp=ms, elastic=fs)[:2],
                 torch_image),
                ("grey-8 labels -> int64", True, lambda: api.png_decode_batch_labels(labs, out, dtype="int64", warp=ms, elastic=fs)[:2], torch_labels)):
            st, t = call()
            st2, t2 = other()
            assert st == st2 == [0] * N_FILES and t2.shape == t.shape
            if labels:
                diff = "%.3f %% of picks differ" % (100.0 * float((t != t2).float().mean()))
            else:
                diff = "mean |call - torch| %.4f" % float((t.float() - t2.float()).abs().mean())
            del t, t2
            tc, tt = [], []
            for r in range(a.warmup + a.reps):
                x, y = B._timed(call), B._timed(other)
                if r >= a.warmup:
                    tc.append(x)
                    tt.append(y)
            lines.append("call   %-50s | call %s | torch %s | call / torch %.3f | %s" % (name, B._cell(tc), B._cell(tt), B._stat(tc)[0] / B._stat(tt)[0], diff))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
