"""PNG bytes -> one Gaussian-blurred, resized, normalised tensor (api.png_decode_batch_tensor(..., blur=)) against the same call
without an operation and against the route there was without the feature, and the blur kernel on its own against a device copy
and against the tone apply kernel.

Workload: 64 RGB8 files of 1024 x 1024 (smooth content with noise, 4 distinct images from a fixed seed, repeated) ->
(64, 3, S, S) float32 with mean / std, S = 224 and 512; file i is blurred with ("gaussian", 23, sigma_i), sigma_i spread evenly
over 0.1 .. 2.0 (the SimCLR / BYOL range).  The method is that of tools/bench_png_tensor_tone.py.

    python tools/bench_png_tensor_blur.py [--reps 8 --warmup 2] --out profiles/png_tensor_blur.txt

(a) blur:  the whole api call with blur=[("gaussian", 23, sigma_i)] (host clock around a call that ends in a device synchronise),
    none:  the same call with blur=[None] * 64 (what the intermediate and the second pass cost on top), and
    torch: the route without the feature -- png_decode_batch_tensor(dtype="uint", layout="hwc"), then per image (every file has its
           own sigma) a reflect pad, a depthwise torch.nn.functional.conv2d with that file's 23 x 23 kernel (what torchvision's
           GaussianBlur runs), a round to the 8-bit step and the normalisation; the three alternate in one process.  The routes
           differ by the rounding to 8 bits that the torch route has and this call has not, and by the Q14 taps: at most
           (0.5 + 0.05) / 255 / min(std); (a) states the largest difference seen.
(b) debig_png_blur_kernel alone (device events around one launch on resident 8-bit noise images, float32 CHW out), with the host's
    32 x 32 tile and, for the record, with a 64 x 32 tile (a smaller share of halo, which the kernel also takes at this radius),
    against a device-to-device copy of the bytes it writes and against debig_png_tone_apply_kernel (a caller's table: no
    histogram) on the same images."""
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

N_FILES, SIDE, N_DISTINCT, OUTS = 64, 1024, 4, (224, 512)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
KSIZE = 23
SIGMAS = [0.1 + 1.9 * i / (N_FILES - 1) for i in range(N_FILES)]
RUN = 4096  # include/debig_hip.h: DEBIG_PNG_TONE_RUN


def workload():
    import png_spec_ref as R

    rng = np.random.default_rng(20261019)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    imgs = []
    for k in range(N_DISTINCT):
        s = ((x[:, :, None] * (3 + k) + y[:, :, None] * 2 + np.arange(3) * 40) // 3 % 256 + rng.integers(0, 9, size=(SIDE, SIDE, 3))) % 256
        rows = np.zeros((SIDE, 1 + 3 * SIDE), np.uint8)  # filter type 0 on every row
        rows[:, 1:] = s.astype(np.uint8).reshape(SIDE, 3 * SIDE)
        imgs.append(R.SIG + R.chunk(b"IHDR", struct.pack(">IIBBBBB", SIDE, SIDE, 8, 2, 0, 0, 0)) +
                    R.chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + R.chunk(b"IEND", b""))
    return [imgs[i % N_DISTINCT] for i in range(N_FILES)]


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


def kernel_alone(S, reps, warmup):
    """(b) at output size S -> the report line"""
    import torch
    import png_blur_ref as B
    from test_emu_png_blur import BlurTask
    from test_emu_png_tone import ToneTask
    from debigulator_amd import _native as N

    L = N.lib()
    L.debig_hip_png_blur_batch.restype = C.c_int
    L.debig_hip_png_blur_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p]
    L.debig_hip_png_tone_apply_batch.restype = C.c_int
    L.debig_hip_png_tone_apply_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    ch, es, px, r = 3, 4, S * S, KSIZE // 2
    img = (px * ch + 15) // 16 * 16
    slot = px * ch * es
    a = 1.0 / (255.0 * (1 << 22))
    tables = b"".join(np.array(B.weights(KSIZE, s) + [0] * (64 - KSIZE), np.int16).tobytes() for s in SIGMAS)
    d_tasks = []
    for tw, th in ((32, 32), (64, 32)):
        tasks = []
        for i in range(N_FILES):
            for y0 in range(0, S, th):
                for x0 in range(0, S, tw):
                    t = BlurTask(src_off=i * img, out_off=i * slot, table_off=i * 128, k=0, radius=r, w=S, h=S, x0=x0, y0=y0,
                                 tile_w=min(tw, S - x0), tile_h=min(th, S - y0), out_sx=1, out_sy=S, out_sc=px, channels=ch,
                                 colour_channels=ch, dtype=1, op=B.GAUSSIAN)
                    t.a[:] = [a] * 4
                    tasks.append(t)
        d_tasks.append((len(tasks), torch.from_numpy(np.frombuffer(bytes((BlurTask * len(tasks))(*tasks)), np.uint8).copy()).cuda()))
    tone = []
    for i in range(N_FILES):
        for p0 in range(0, px, RUN):
            t = ToneTask(src_off=i * img, out_off=i * slot, hist_off=0, lut_off=0, pix0=p0, pix_n=min(RUN, px - p0), out_w=S, out_h=S,
                         out_sx=1, out_sy=S, out_sc=px, channels=ch, colour_channels=ch, dtype=1, op=5)
            t.a[:] = [a] * 4
            tone.append(t)
    d_tone = torch.from_numpy(np.frombuffer(bytes((ToneTask * len(tone))(*tone)), np.uint8).copy()).cuda()
    noise = torch.randint(0, 256, (N_FILES * img,), dtype=torch.uint8, device="cuda")
    d_tab = torch.from_numpy(np.frombuffer(tables, np.uint8).copy()).cuda()
    lut = torch.arange(256, dtype=torch.uint8, device="cuda")
    out = torch.empty(N_FILES * slot, dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    sp, op = noise.data_ptr(), out.data_ptr()
    same = []
    for n, dt in d_tasks:  # either tiling gives the restatement's elements (the last file: the widest kernel)
        out.zero_()
        assert L.debig_hip_png_blur_batch(sp, op, dt.data_ptr(), d_tab.data_ptr(), n, None) == 0
        torch.cuda.synchronize()
        i = N_FILES - 1
        src = noise[i * img: i * img + px * ch].view(S, S, ch).cpu().numpy()
        want = B.blur(src, B.GAUSSIAN, KSIZE, SIGMAS[i], "float32", (1, 1, 1, 1), (0, 0, 0, 0), "chw")
        same.append(bool(np.array_equal(out[i * slot: (i + 1) * slot].view(torch.float32).view(ch, S, S).cpu().numpy(), want)))
    ts = _alternate(L, [lambda: L.debig_hip_png_blur_batch(sp, op, d_tasks[0][1].data_ptr(), d_tab.data_ptr(), d_tasks[0][0], None),
                        lambda: L.debig_hip_png_blur_batch(sp, op, d_tasks[1][1].data_ptr(), d_tab.data_ptr(), d_tasks[1][0], None),
                        lambda: L.debig_hip_png_tone_apply_batch(sp, op, d_tone.data_ptr(), None, lut.data_ptr(), len(tone), None)],
                    reps, warmup)
    tco = []
    for k in range(warmup + reps):
        ms = _timed(lambda: out2.copy_(out))
        if k >= warmup:
            tco.append(ms)
    return ("(b) %d^2 blur kernel (gaussian 23, float32 chw) | tile 32 x 32, %d tasks: %s | tile 64 x 32, %d tasks: %s | the restatement's "
            "elements: %s | tone apply kernel %s | d2d copy of the %.1f MiB written %s | blur / copy %.2f | blur / tone apply %.2f"
            % (S, d_tasks[0][0], _cell(ts[0]), d_tasks[1][0], _cell(ts[1]), same, _cell(ts[2]), N_FILES * slot / 2 ** 20, _cell(tco),
               _stat(ts[0])[0] / _stat(tco)[0], _stat(ts[0])[0] / _stat(ts[2])[0])), _stat(ts[0])[0]


def whole_call(api, imgs, S, reps, warmup, kernel_ms):
    import torch
    import torch.nn.functional as F
    import png_blur_ref as B

    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    kw = dict(mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD)
    blurs = [("gaussian", KSIZE, s) for s in SIGMAS]
    r = KSIZE // 2
    k1 = [torch.tensor(B.weights_real(KSIZE, s), dtype=torch.float32, device="cuda") for s in SIGMAS]
    k2 = [(k[:, None] * k[None, :]).expand(3, 1, KSIZE, KSIZE).contiguous() for k in k1]

    def blur():
        return api.png_decode_batch_tensor(imgs, (S, S), blur=blurs, **kw)[:2]

    def none():
        return api.png_decode_batch_tensor(imgs, (S, S), blur=[None] * N_FILES, **kw)[:2]

    def torch_route():
        st, t, _ = api.png_decode_batch_tensor(imgs, (S, S), mode="rgb", dtype="uint", layout="hwc")
        out = torch.empty((N_FILES, 3, S, S), dtype=torch.float32, device="cuda")
        for i in range(N_FILES):
            x = F.pad(t[i].permute(2, 0, 1).to(torch.float32)[None], (r, r, r, r), mode="reflect")
            out[i] = F.conv2d(x, k2[i], groups=3)[0].round_()
        return st, (out / 255.0 - mean) / std

    st, t = blur()
    st2, t2 = torch_route()
    assert st == st2 == [0] * N_FILES and t.shape == t2.shape == (N_FILES, 3, S, S)
    diff = float((t - t2).abs().max())
    assert diff <= 0.56 / 255.0 / min(STD), diff
    tb, tn, tr = [], [], []
    for k in range(warmup + reps):
        x, y, z = _timed(blur), _timed(none), _timed(torch_route)
        if k >= warmup:
            tb.append(x)
            tn.append(y)
            tr.append(z)
    gap, spread = _stat(tr)[0] - _stat(tb)[0], (max(tb) - min(tb)) + (max(tr) - min(tr))
    return "(a) %d^2 blur %s | none %s | torch %s | blur / none %.3f | blur / torch %.3f | torch - blur %.3f ms against a spread of %.3f ms " \
           "(both routes' max - min) | the blur kernel's share of the call %.1f %% | max |blur - torch| %.2e" \
           % (S, _cell(tb), _cell(tn), _cell(tr), _stat(tb)[0] / _stat(tn)[0], _stat(tb)[0] / _stat(tr)[0], gap, spread,
              100 * kernel_ms / _stat(tb)[0], diff)


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
    lines = ["# tools/bench_png_tensor_blur.py: %d RGB8 files of %d x %d (%d distinct; %.1f MiB of files) -> (%d, 3, S, S) float32 with mean / std,"
             % (N_FILES, SIDE, SIDE, N_DISTINCT, sum(map(len, imgs)) / 2 ** 20, N_FILES),
             "# file i blurred with (gaussian, %d, sigma_i), sigma_i evenly over %.1f .. %.1f; %d timed runs after %d warm-up runs, routes"
             % (KSIZE, SIGMAS[0], SIGMAS[-1], a.reps, a.warmup),
             "# alternating in one process; spread = (max - min) / median",
             "# (a) blur = the whole api call with blur=; none = the same call, no operation; torch = decode to uint8 hwc + per image a reflect",
             "#     pad + a depthwise conv2d with the file's 23 x 23 kernel + round + normalise in torch; all end in a device synchronise.",
             "# (b) one launch on resident 8-bit noise images, device events."]
    alone = [kernel_alone(S, a.reps, a.warmup) for S in OUTS]
    for S, (_, ms) in zip(OUTS, alone):
        lines.append(whole_call(api, imgs, S, a.reps, a.warmup, ms))
    lines += [line for line, _ in alone]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
