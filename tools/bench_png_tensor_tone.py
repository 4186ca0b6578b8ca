"""PNG bytes -> one equalised, resized, normalised tensor (api.png_decode_batch_tensor(..., tone=)) against the same call without an
operation and against the route there was without the feature, and the two tone kernels on their own against device copies.

Workload: 64 RGB8 files of 1024 x 1024 (smooth content with noise, 4 distinct images from a fixed seed, repeated) ->
(64, 3, S, S) float32 with mean / std, S = 224 and 512; every image is equalised.

    python tools/bench_png_tensor_tone.py [--reps 8 --warmup 2] --out profiles/png_tensor_tone.txt

(a) tone:  the whole api call with tone=["equalize"] * 64 (host clock around a call that ends in a device synchronise), against
    none:  the same call with tone=[None] * 64 (what the histogram, the tables and the second pass cost on top), and against
    torch: the route without the feature -- png_decode_batch_tensor(dtype="uint", layout="hwc"), then on the device one
           torch.bincount per image, the equalize rule on the (64, 3, 256) histograms, a gather through the tables and the
           normalisation; the three alternate in one process.  The two routes give the same elements up to float32 rounding of
           the normalisation; (a) states the largest difference seen.
(b) debig_png_tone_hist_kernel alone (device events around one launch on resident 8-bit images) on noise and on flat images
    -- flat / noise says whether one histogram set per wavefront is enough under contention -- against a device-to-device copy
    of the bytes it reads;
(c) debig_png_tone_apply_kernel alone (equalize: it builds the tables from the histograms) against a device-to-device copy of
    the bytes it writes."""
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
RUN = 4096  # include/debig_hip.h: DEBIG_PNG_TONE_RUN


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


def torch_equalize_tables(h):
    """h (N, 3, 256) int64 on the device -> the equalize tables (N, 3, 256) int64, by the rule of include/decode_png.h"""
    import torch

    nz = h > 0
    last = 255 - torch.argmax(nz.flip(-1).to(torch.int8), dim=-1, keepdim=True)
    step = (h.sum(-1, keepdim=True) - h.gather(-1, last)) // 255
    n = step // 2 + torch.cumsum(h, -1) - h
    lut = torch.clamp(n // torch.clamp(step, min=1), max=255)
    ident = torch.arange(256, device=h.device).expand_as(lut)
    return torch.where((nz.sum(-1, keepdim=True) < 2) | (step == 0), ident, lut)


def kernels_alone(S, reps, warmup):
    """(b) and (c) at output size S -> the report lines"""
    import torch
    from test_emu_png_tone import ToneTask
    from debigulator_amd import _native as N

    L = N.lib()
    L.debig_hip_png_tone_hist_batch.restype = C.c_int
    L.debig_hip_png_tone_hist_batch.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p]
    L.debig_hip_png_tone_apply_batch.restype = C.c_int
    L.debig_hip_png_tone_apply_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    ch, es, px = 3, 4, S * S
    img = (px * ch + 15) // 16 * 16
    slot = px * ch * es
    a = 1.0 / (255.0 * (1 << 22))
    tasks = []
    for i in range(N_FILES):
        for p0 in range(0, px, RUN):
            t = ToneTask(src_off=i * img, out_off=i * slot, hist_off=i * ch * 1024, lut_off=0, pix0=p0, pix_n=min(RUN, px - p0), out_w=S,
                         out_h=S, out_sx=1, out_sy=S, out_sc=px, channels=ch, colour_channels=ch, dtype=1, op=2)
            t.a[:] = [a] * 4
            tasks.append(t)
    n = len(tasks)
    d_tasks = torch.from_numpy(np.frombuffer(bytes((ToneTask * n)(*tasks)), np.uint8).copy()).cuda()
    noise = torch.randint(0, 256, (N_FILES * img,), dtype=torch.uint8, device="cuda")
    flat = torch.full((N_FILES * img,), 93, dtype=torch.uint8, device="cuda")
    src2 = torch.empty_like(noise)
    hist = torch.zeros(N_FILES * ch * 256, dtype=torch.int32, device="cuda")
    lut = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.empty(N_FILES * slot, dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    tp, hp, op = d_tasks.data_ptr(), hist.data_ptr(), out.data_ptr()
    th = _alternate(L, [lambda: L.debig_hip_png_tone_hist_batch(noise.data_ptr(), hp, tp, n, None),
                        lambda: L.debig_hip_png_tone_hist_batch(flat.data_ptr(), hp, tp, n, None)], reps, warmup)
    # the histograms now hold the sums of all runs: exact whatever they are; take fresh ones of the noise for the apply kernel
    hist.zero_()
    assert L.debig_hip_png_tone_hist_batch(noise.data_ptr(), hp, tp, n, None) == 0
    torch.cuda.synchronize()
    want = torch.stack([torch.bincount(noise[i * img: i * img + px * ch].view(px, ch).long().add_(torch.arange(ch, device="cuda") * 256).view(-1),
                                       minlength=ch * 256) for i in range(N_FILES)])
    same_h = bool(torch.equal(hist.view(N_FILES, ch * 256).long(), want))
    ta = _alternate(L, [lambda: L.debig_hip_png_tone_apply_batch(noise.data_ptr(), op, tp, hp, lut.data_ptr(), n, None)], reps, warmup)[0]
    tabs = torch_equalize_tables(want.view(N_FILES, ch, 256))
    x = noise.view(N_FILES, img)[:, : px * ch].view(N_FILES, px, ch).permute(0, 2, 1).long()
    ref = (tabs.gather(-1, x) << 22).to(torch.float32) * np.float32(a)
    same_a = bool(torch.equal(out.view(torch.float32).view(N_FILES, ch, px), ref))
    tcs, tco = [], []
    for r in range(warmup + reps):
        ms1, ms2 = _timed(lambda: src2.copy_(noise)), _timed(lambda: out2.copy_(out))
        if r >= warmup:
            tcs.append(ms1)
            tco.append(ms2)
    mib_in, mib_out = N_FILES * img / 2 ** 20, N_FILES * slot / 2 ** 20
    return ["(b) %d^2 histogram kernel, %d tasks | noise %s | flat %s | flat / noise %.2f | exact: %s | d2d copy of the %.1f MiB read %s | "
            "noise / copy %.2f" % (S, n, _cell(th[0]), _cell(th[1]), _stat(th[1])[0] / _stat(th[0])[0], same_h, mib_in, _cell(tcs),
                                   _stat(th[0])[0] / _stat(tcs)[0]),
            "(c) %d^2 apply kernel (equalize, float32 chw), %d tasks | %s | same elements as torch: %s | d2d copy of the %.1f MiB written %s "
            "| apply / copy %.2f" % (S, n, _cell(ta), same_a, mib_out, _cell(tco), _stat(ta)[0] / _stat(tco)[0])]


def whole_call(api, imgs, S, reps, warmup):
    import torch

    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    chan = (torch.arange(3, device="cuda") * 256).view(1, 3)
    kw = dict(mode="rgb", dtype="float32", layout="chw", mean=MEAN, std=STD)

    def tone():
        return api.png_decode_batch_tensor(imgs, (S, S), tone=["equalize"] * N_FILES, **kw)[:2]

    def none():
        return api.png_decode_batch_tensor(imgs, (S, S), tone=[None] * N_FILES, **kw)[:2]

    def torch_route():
        st, t, _ = api.png_decode_batch_tensor(imgs, (S, S), mode="rgb", dtype="uint", layout="hwc")
        h = torch.stack([torch.bincount((t[i].view(-1, 3).long() + chan).view(-1), minlength=768) for i in range(N_FILES)])
        tabs = torch_equalize_tables(h.view(N_FILES, 3, 256))
        x = tabs.gather(-1, t.view(N_FILES, S * S, 3).permute(0, 2, 1).long()).view(N_FILES, 3, S, S)
        return st, (x.to(torch.float32) / 255.0 - mean) / std

    st, t = tone()
    st2, t2 = torch_route()
    assert st == st2 == [0] * N_FILES and t.shape == t2.shape == (N_FILES, 3, S, S)
    diff = float((t - t2).abs().max())
    tt, tn, tr = [], [], []
    for r in range(warmup + reps):
        x, y, z = _timed(tone), _timed(none), _timed(torch_route)
        if r >= warmup:
            tt.append(x)
            tn.append(y)
            tr.append(z)
    gap, spread = _stat(tr)[0] - _stat(tt)[0], (max(tt) - min(tt)) + (max(tr) - min(tr))
    return "(a) %d^2 tone %s | none %s | torch %s | tone / none %.3f | tone / torch %.3f | torch - tone %.3f ms against a spread of %.3f ms " \
           "(both routes' max - min) | max |tone - torch| %.2e" % (S, _cell(tt), _cell(tn), _cell(tr), _stat(tt)[0] / _stat(tn)[0],
                                                                  _stat(tt)[0] / _stat(tr)[0], gap, spread, diff)


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
    lines = ["# tools/bench_png_tensor_tone.py: %d RGB8 files of %d x %d (%d distinct; %.1f MiB of files) -> (%d, 3, S, S) float32 with mean / std,"
             % (N_FILES, SIDE, SIDE, N_DISTINCT, sum(map(len, imgs)) / 2 ** 20, N_FILES),
             "# every image equalised; %d timed runs after %d warm-up runs, routes alternating in one process; spread = (max - min) / median"
             % (a.reps, a.warmup),
             "# (a) tone = the whole api call with tone=equalize; none = the same call, no operation; torch = decode to uint8 hwc + a bincount",
             "#     per image + the table rule + gather + normalise in torch; all end in a device synchronise.",
             "# (b), (c): one launch on resident 8-bit images, device events."]
    for S in OUTS:
        lines.append(whole_call(api, imgs, S, a.reps, a.warmup))
    for S in OUTS:
        lines += kernels_alone(S, a.reps, a.warmup)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
