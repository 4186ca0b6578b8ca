"""Spec-complete PNG batch decode (include/decode_png.h: debig_png_decode_batch) per format, on the GPU.

    python tools/bench_png_spec.py [--n 64] [--size 1024] [--reps 5] [--out profiles/png_spec_formats.txt]

For a batch of n images of size x size per format: ms per batch call (files in host memory -> RGBA in host memory: upload,
CRC, gather, inflate, Adler-32, de-filter, download) and GB/s of RGBA produced.  RGBA8 runs twice: through the tuned
de-filter (default routing) and forced through the general kernel.  The files are made here with a vectorised encoder
(filter type y % 5, zlib level 6); four distinct images per format, repeated.
"""
import argparse
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_spec_ref as R  # noqa: E402


def _filter_rows(raw, bpp):
    """raw: (h, rb) uint8 -> filtered scanlines with filter type y % 5 (vectorised per row)"""
    h, rb = raw.shape
    r = raw.astype(np.int32)
    up = np.zeros_like(r)
    up[1:] = r[:-1]
    left = np.zeros_like(r)
    left[:, bpp:] = r[:, :-bpp]
    ul = np.zeros_like(r)
    ul[1:, bpp:] = r[:-1, :-bpp]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    preds = [np.zeros_like(r), left, up, (left + up) >> 1, paeth]
    ft = np.arange(h) % 5
    out = np.empty((h, rb + 1), dtype=np.uint8)
    out[:, 0] = ft
    for t in range(5):
        m = ft == t
        out[m, 1:] = ((r[m] - preds[t][m]) & 0xFF).astype(np.uint8)
    return out


def _pack(sub, ct, depth):
    h, w, ch = sub.shape
    if depth == 16:
        return sub.astype(">u2").reshape(h, -1).view(np.uint8)
    if depth == 8:
        return sub.reshape(h, -1).astype(np.uint8)
    bits = np.unpackbits(sub.reshape(h, w, 1).astype(np.uint8), axis=2)[:, :, 8 - depth:]
    return np.packbits(bits.reshape(h, -1), axis=1)


def encode_fast(s, ct, depth, il=0, trns=None, palette=None):
    h, w = s.shape[:2]
    parts = []
    for x0, y0, dx, dy, wp, hp in R.passes(w, h, il):
        parts.append(_filter_rows(_pack(s[y0::dy, x0::dx], ct, depth), R.bpp_f(ct, depth)).tobytes())
    z = zlib.compress(b"".join(parts), 6)
    return R.encode(s, ct, depth, il, trns=trns, palette=palette, zdata=z)


def _image(rng, size, ct, depth, seed):
    y, x = np.mgrid[0:size, 0:size]
    ch = R.CHANNELS[ct]
    base = (x[:, :, None] * (seed + 1) + y[:, :, None] * (seed + 2) + 37 * np.arange(ch)) % 4096
    noise = rng.integers(0, 8, size=(size, size, ch))
    if depth == 16:
        return ((base * 16 + noise * 5) % 65536).astype(np.uint16)
    top = 1 << depth
    return ((base // (4096 // top) + (noise % 2 if depth >= 8 else 0)) % top).astype(np.uint8)


FORMATS = [  # name, ct, depth, interlace, tRNS, force_general
    ("grey8", 0, 8, 0, False, False), ("grey16", 0, 16, 0, False, False), ("grey+alpha8", 4, 8, 0, False, False),
    ("rgb16", 2, 16, 0, False, False), ("rgba16", 6, 16, 0, False, False), ("palette4+tRNS", 3, 4, 0, True, False),
    ("grey1", 0, 1, 0, False, False), ("rgba8 adam7", 6, 8, 1, False, False), ("rgba8 tuned", 6, 8, 0, False, False),
    ("rgba8 general", 6, 8, 0, False, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from debigulator_amd import api

    import torch

    lines = ["# tools/bench_png_spec.py --n %d --size %d --reps %d (%s)" % (a.n, a.size, a.reps, torch.cuda.get_device_name(0)),
             "# format            ms/batch (median)   GB/s of RGBA   compressed MB/batch"]
    rng = np.random.default_rng(1)
    for name, ct, depth, il, trns, general in FORMATS:
        distinct = []
        for k in range(4):
            s = _image(rng, a.size, ct, depth, k)
            pal = t = None
            if ct == 3:
                pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(1 << depth)]
                t = bytes(rng.integers(0, 256, size=(1 << depth) // 2, dtype=np.uint8))
            distinct.append(encode_fast(s, ct, depth, il, t, pal))
        files = [distinct[k % 4] for k in range(a.n)]
        out = api.png_decode_batch(files, force_general=general)  # warm-up, and a check
        assert all(st == 0 for st, _, _ in out), (name, [st for st, _, _ in out][:4])
        ref = R.decode(distinct[0]) if a.size <= 256 else None
        if ref is not None:
            assert np.array_equal(out[0][1], ref[1]), name
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.png_decode_batch(files, force_general=general)
            times.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(times))
        gbs = a.n * 4 * a.size * a.size / (ms * 1e-3) / 1e9
        mb = sum(len(f) for f in files) / 1e6
        lines.append("%-18s %10.2f %18.2f %16.1f" % (name, ms, gbs, mb))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
