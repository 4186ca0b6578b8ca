"""PNG bytes -> one colour-jittered, resized, normalised tensor (api.png_decode_batch_tensor(..., color=)) against the route there
was without it, and the two colour kernels on their own against the kernels they extend.

Workload: 64 RGB8 files of 1024 x 1024 (smooth content with noise, 4 distinct images from a fixed seed, repeated) ->
(64, 3, 224, 224) float32 with mean / std; every image gets its own png_color_matrix (brightness, contrast and saturation in
0.6 .. 1.4, hue in +-36 degrees).

    python tools/bench_png_tensor_color.py [--reps 8 --warmup 2] --out profiles/png_tensor_color.txt

(a) call:  the whole api call with color= (host clock around a call that ends in a device synchronise), against
    torch: the route it replaces -- png_decode_batch_tensor to float32 WITHOUT normalisation, then torch.einsum with the matrices,
           add the offsets, clamp to [0, 1], normalise; the two alternate in one process;
(b) debig_png_resize_color_kernel alone against debig_png_resize_kernel on the same tile tasks with the identity matrix (device
    events around one launch on resident sources; pass 1 is identical, so the difference is what pass 2 and the mix cost), and
    against a device-to-device copy of the bytes it writes;
(c) the same pair for debig_png_warp_color_kernel against debig_png_warp_kernel (a rotation in +-30 degrees per image, bilinear).
The torch route computes in float32, so its elements differ from the integer rule's in the last bits; (a) states the largest
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

N_FILES, SIDE, N_DISTINCT, OUT = 64, 1024, 4, (224, 224)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
TILE_W, HQ_CAP, WX_CAP = 64, 12288, 4096  # include/debig_hip.h


def workload():
    import png_spec_ref as R

    rng = np.random.default_rng(20261018)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    imgs = []
    for k in range(N_DISTINCT):
        s = ((x[:, :, None] * (3 + k) + y[:, :, None] * 2 + np.arange(3) * 40) // 3 % 256 + rng.integers(0, 9, size=(SIDE, SIDE, 3))) % 256
        rows = np.zeros((SIDE, 1 + 3 * SIDE), np.uint8)  # filter type 0 on every row
        rows[:, 1:] = s.astype(np.uint8).reshape(SIDE, 3 * SIDE)
        imgs.append(R.SIG + R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIDE, SIDE, 8, 2, 0, 0, 0)) +
                    R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b""))
    return [imgs[i % N_DISTINCT] for i in range(N_FILES)]


def matrices(api):
    rng = np.random.default_rng(11)
    return np.stack([api.png_color_matrix(*(float(v) for v in rng.uniform(0.6, 1.4, 3)), hue=float(rng.uniform(-36, 36))) for _ in range(N_FILES)])


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


def _cell(ts):
    med, sp = _stat(ts)
    return "%.3f ms (spread %.1f %%)" % (med, 100 * sp)


def _events(L):
    L.debig_hip_event_create.restype = C.c_void_p
    L.debig_hip_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_elapsed_ms.restype = C.c_float
    L.debig_hip_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.debig_hip_event_destroy.argtypes = [C.c_void_p]
    return L.debig_hip_event_create(), L.debig_hip_event_create()


def _dev(buf):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda()


def _alternate(L, launches, reps, warmup):
    """launches: [callable -> rc]; each timed by device events, alternating -> [[ms]]"""
    e0, e1 = _events(L)
    ts = [[] for _ in launches]
    for r in range(warmup + reps):
        for k, fn in enumerate(launches):
            L.debig_hip_event_record(e0, None)
            rc = fn()
            L.debig_hip_event_record(e1, None)
            assert rc == 0, rc
            ms = float(L.debig_hip_event_elapsed_ms(e0, e1))  # (synchronises on e1)
            if r >= warmup:
                ts[k].append(ms)
    L.debig_hip_event_destroy(e0)
    L.debig_hip_event_destroy(e1)
    return ts


def kernels_alone(reps, warmup):
    """(b) and (c): the colour kernels with the identity matrix against the kernels they extend, on the same tasks, and a
    device-to-device copy of the bytes they write -> the report lines"""
    import torch
    import png_color_ref as CR
    import png_filter_ref as FR
    import png_warp_ref as WR
    from test_emu_png_color import ColorRec, ResizeColorTask, WarpColorTask, _axis_table
    from test_emu_png_resize import Task as ResizeTask
    from test_emu_png_warp import WarpTask
    from debigulator_amd import _native as N
    from debigulator_amd.api import png_warp_matrix

    L = N.lib()
    for name in ("debig_hip_png_resize_batch", "debig_hip_png_resize_color_batch", "debig_hip_png_warp_color_batch"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    L.debig_hip_png_warp_batch.restype = C.c_int
    L.debig_hip_png_warp_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
    H, W = OUT
    ch, es = 3, 4
    slot = H * W * ch * es
    a = 1.0 / (255.0 * (1 << 22))
    # ---- the tile tasks of the host's rule, once as the plain task and once with the record's place
    tb, ent, mt = _axis_table(FR.BILINEAR, SIDE, W, True)
    weights = bytearray(tb)
    rec_off = len(weights)
    rec = ColorRec()
    rec.k[:], rec.o[:] = CR.quantise(CR.IDENTITY, 8)
    weights.extend(bytes(rec))
    tw = min(W, TILE_W, WX_CAP // mt, HQ_CAP // (mt * ch))
    plain, color = [], []
    for i in range(N_FILES):
        y0 = 0
        while y0 < H:
            lo, hi, th = ent[y0][0], sum(ent[y0]), 1
            while y0 + th < H and th < 64:
                f, e = ent[y0 + th][0], sum(ent[y0 + th])
                if (max(hi, e) - min(lo, f)) * tw * ch > HQ_CAP:
                    break
                lo, hi, th = min(lo, f), max(hi, e), th + 1
            for x0 in range(0, W, tw):
                kw = dict(src_off=i * SIDE * SIDE * ch, out_off=i * slot, wx_off=0, wy_off=0, src_pitch=SIDE * ch, tile_x=x0, tile_y=y0,
                          tile_w=min(tw, W - x0), tile_h=th, src_y0=lo, src_rows=hi - lo, out_sx=1, out_sy=W, out_sc=H * W, channels=ch,
                          bits=8, dtype=1)
                for T, lst, more in ((ResizeTask, plain, {}), (ResizeColorTask, color, dict(color_off=rec_off))):
                    t = T(**kw, **more)
                    t.a[:] = [a] * 4
                    lst.append(t)
            y0 += th
    n_r = len(plain)
    src = torch.randint(0, 256, (N_FILES * SIDE * SIDE * ch,), dtype=torch.uint8, device="cuda")
    out = torch.empty(N_FILES * slot, dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    d_w = _dev(weights)
    d_plain, d_color = _dev((ResizeTask * n_r)(*plain)), _dev((ResizeColorTask * n_r)(*color))
    # ---- the warp tasks: a rotation per image
    rng = np.random.default_rng(7)
    run = max(1, 4096 // W)
    wplain, wcolor = [], []
    for i in range(N_FILES):
        m = png_warp_matrix((SIDE, SIDE), OUT, angle=float(rng.uniform(-30, 30)), scale=OUT[0] / SIDE * float(rng.uniform(1.0, 1.4)))
        q = WR.quantise([v for r in m for v in r])
        for y0 in range(0, H, run):
            kw = dict(src_off=i * SIDE * SIDE * ch, out_off=i * slot, src_pitch=SIDE * ch, crop_w=SIDE, crop_h=SIDE, out_w=W, out_h=H, row0=y0,
                      rows=min(run, H - y0), out_sx=1, out_sy=W, out_sc=H * W, channels=ch, bits=8, dtype=1, filter=0, border_mode=0)
            for T, lst, more in ((WarpTask, wplain, {}), (WarpColorTask, wcolor, dict(color_off=0))):
                t = T(**kw, **more)
                t.m[:] = q
                t.a[:] = [a] * 4
                lst.append(t)
    n_w = len(wplain)
    d_wplain, d_wcolor, d_rec = _dev((WarpTask * n_w)(*wplain)), _dev((WarpColorTask * n_w)(*wcolor)), _dev(bytes(rec))
    torch.cuda.synchronize()
    s, o, o2 = src.data_ptr(), out.data_ptr(), out2.data_ptr()
    tr = _alternate(L, [lambda: L.debig_hip_png_resize_batch(s, o, d_plain.data_ptr(), d_w.data_ptr(), n_r, None),
                        lambda: L.debig_hip_png_resize_color_batch(s, o2, d_color.data_ptr(), d_w.data_ptr(), n_r, None)], reps, warmup)
    same_r = bool(torch.equal(out, out2))
    tw_ = _alternate(L, [lambda: L.debig_hip_png_warp_batch(s, o, d_wplain.data_ptr(), n_w, None),
                         lambda: L.debig_hip_png_warp_color_batch(s, o2, d_wcolor.data_ptr(), d_rec.data_ptr(), n_w, None)], reps, warmup)
    same_w = bool(torch.equal(out, out2))
    tcopy = []
    for r in range(warmup + reps):
        ms = _timed(lambda: out2.copy_(out))
        if r >= warmup:
            tcopy.append(ms)
    lines = []
    for name, (tp, tc), n, same in (("(b) resize", tr, n_r, same_r), ("(c) warp  ", tw_, n_w, same_w)):
        lines.append("%s %d tasks | plain kernel %s | colour kernel, identity %s | colour / plain %.3f | same bytes: %s | d2d copy of the %.1f MiB "
                     "written %s | colour / copy %.2f" % (name, n, _cell(tp), _cell(tc), _stat(tc)[0] / _stat(tp)[0], same, N_FILES * slot / 2 ** 20,
                                                          _cell(tcopy), _stat(tc)[0] / _stat(tcopy)[0]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from debigulator_amd import api

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    imgs = workload()
    Ms = matrices(api)
    lin = torch.from_numpy(Ms[:, :, :3].astype(np.float32)).cuda()
    off = torch.from_numpy(Ms[:, :, 3].astype(np.float32)).cuda().view(N_FILES, 3, 1, 1)
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)

    def call():
        return api.png_decode_batch_tensor(imgs, OUT, mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD, color=Ms)[:2]

    def torch_route():
        st, t, _ = api.png_decode_batch_tensor(imgs, OUT, mode="rgb", dtype="float32", layout="chw")
        x = torch.einsum("ncd,ndhw->nchw", lin, t) + off
        return st, (x.clamp_(0.0, 1.0) - mean) / std

    st, t = call()
    st2, t2 = torch_route()
    assert st == st2 == [0] * N_FILES and t.shape == t2.shape == (N_FILES, 3) + OUT
    diff = float((t - t2).abs().max())
    tc, tt = [], []
    for r in range(a.warmup + a.reps):
        x, y = _timed(call), _timed(torch_route)
        if r >= a.warmup:
            tc.append(x)
            tt.append(y)
    lines = ["# tools/bench_png_tensor_color.py: %d RGB8 files of %d x %d (%d distinct; %.1f MiB of files) -> (%d, 3, %d, %d) float32 with"
             % (N_FILES, SIDE, SIDE, N_DISTINCT, sum(map(len, imgs)) / 2 ** 20, N_FILES, OUT[0], OUT[1]),
             "# mean / std, one png_color_matrix per image (brightness, contrast, saturation 0.6 .. 1.4, hue +-36 degrees);",
             "# %d timed runs after %d warm-up runs, routes alternating in one process; spread = (max - min) / median" % (a.reps, a.warmup),
             "# (a) call = the whole api call with color=; torch = decode to float32 without normalisation + einsum + add + clamp +",
             "#     normalise; both end in a device synchronise.  (b), (c): one launch on resident sources, device events.",
             "(a) call %s | torch %s | call / torch %.3f | max |call - torch| %.2e" % (_cell(tc), _cell(tt), _stat(tc)[0] / _stat(tt)[0], diff)]
    lines += kernels_alone(a.reps, a.warmup)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
