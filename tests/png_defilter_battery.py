"""TEST TOOLING: the battery of the tuned 8-bit de-filter (csrc/png_kernel.inc: debig_png_defilter_kernel<NWD, BLK, MWG, PX>), for two
back ends: the CPU lock-step emulator (tests/test_emu_png_defilter_battery.py) and debig_hip_png_defilter_batch on the MI355X
(tests/test_gpu_png_defilter_battery.py).  Three parts:

  * images(S): the image list for a launch mode with S band slots (wavefronts that take the bands of one image round robin: NWD x G).
    Images are raw scanline streams, not PNG files: uniform random bytes and a random filter byte 0 .. 4 per row unless the
    group says otherwise.
  * run(images, launch): lays out the stream arena (streams and palettes at chosen residues, every gap and 64 bytes at either end
    filled with 0xA5), the output arena (filled with 0x5A), the tasks and the results (filled with 0xEE), calls
    launch(stream_arena, out_arena, images, results, n) -> return code, and checks.
  * the check: every image BIT FOR BIT against png_spec_ref._unfilter (pure Python, written independently of the kernel) of the same
    bytes under the three expansions (RGBA as is, RGB + 255, palette planes R[256] G[256] B[256] + 255); the stream arena unchanged;
    the output arena unchanged outside the images and a wide palette image's scratch; every debig_png_result as expected.
    Nothing is compared with the emulator's output or with the oracle.

The references are cached across modes: the images whose height derives from S are the first rows of ONE stream per image (the
de-filter is causal from the top), so the reference of a lower image is the top of the reference of the highest one so far."""
import ctypes as C
import zlib

import numpy as np

import png_spec_ref as R
from debigulator_amd._native import DebigPngImage, DebigPngResult

REDO = 0xFFFFFFFD  # PNG_ROW_REDO: bad_row of an image the several-workgroups launch gave up
NO_ROW = 0xFFFFFFFF  # bad_row of an image without a bad row
BPP = {6: 4, 2: 3, 3: 1}
S_FILL, O_FILL, R_FILL = 0xA5, 0x5A, 0xEE
PREVROW = 16384  # PNG_PREVROW_BYTES: a palette row wider than this goes through scratch at tmp_off
# (w, h) of tests/test_emulator_kernels.py::test_defilter_kernel_group_and_band_edges
EDGES = [(1, 1), (2, 3), (3, 65), (4, 64), (5, 2), (7, 130), (8, 63), (63, 5), (65, 66), (130, 9)]
# the mid-row wait: 4 k + 1 pixels, k on both sides of 16 and 32 = 16 + 16 (the pixel-skew step's block and follower lag),
# of 79 = 63 + 16 (the group step's), and multiples of the 6-step blocks of <16, 6> in between; two long rows
MIDROW_W = [4 * k + 1 for k in (5, 6, 7, 15, 16, 17, 31, 32, 33, 79, 80, 81)] + [1030, 1300]
ENDS = np.array([0, 1, 2, 127, 128, 129, 253, 254, 255], dtype=np.uint8)
WIDE = "status-wide-palette"  # the one image that runs in one mode only (a 2 MB stream, 8.5 MB of pixels)
S_MAX = 64  # the widest mode: 16 workgroups of 4 wavefronts


class Image:
    """one task.  ref: (key, stream) for the reference cache where they are not (name, the image's own stream) -- a stream of more
    rows that the image is the top of, or the stream the kernel is to treat the image's as; exp: the expected pixels where they need no reference;
    sres / rres: stream_off & 3 and rgba_off & 15 (None: by the image's place in the call); tmp: "scratch" gives a wide palette
    image its w + 16 bytes at tmp_off; expect: (good, bad_row), pixels are checked when good"""

    def __init__(self, name, ct, w, h, stream, pal=None, asserts_off=0, tmp=None, sres=None, rres=None, expect=(1, NO_ROW),
                 ref=None, exp=None):
        self.name, self.ct, self.w, self.h, self.stream, self.pal = name, ct, w, h, stream, pal
        self.asserts_off, self.tmp, self.sres, self.rres, self.expect, self.ref, self.exp = asserts_off, tmp, sres, rres, expect, ref, exp
        assert stream.dtype == np.uint8 and len(stream) == h * (w * BPP[ct] + 1)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_stream(name, ct, w, h, filters="mixed", values=None):
    """h rows of (filter byte, w * bpp bytes).  filters: "mixed" (random 0 .. 4 per row), an int (every row), or a function of y"""
    rng = _rng(name)
    rb = w * BPP[ct]
    st = rng.integers(0, 256, (h, rb + 1), dtype=np.uint8)
    if values is not None:
        st = values[rng.integers(0, len(values), (h, rb + 1))]
    if filters == "mixed":
        st[:, 0] = rng.integers(0, 5, h)
    elif callable(filters):
        st[:, 0] = [filters(y) for y in range(h)]
    else:
        st[:, 0] = filters
    return st.reshape(-1)


def palette(name):
    return _rng(name + "/palette").integers(0, 256, 768, dtype=np.uint8)


_REF = {}  # key -> de-filtered rows (h, w * bpp) of the highest image with that key so far


def ref_rows(key, stream, w, h, bpp):
    """the specification's de-filter of the stream's h rows; `stream` may hold more rows than h (then they are what a later, higher
    image under the same key will ask for)"""
    rb = w * bpp
    have = _REF.get(key)
    if have is None or have.shape[0] < h:
        rows, bad, _ = R._unfilter(stream.tobytes(), 0, w, h, rb, bpp)
        assert bad is None, (key, bad)
        have = _REF[key] = rows
    return have[:h]


def expand(rows, ct, w, h, pal):
    """de-filtered rows (h, w * bpp) -> the RGBA pixels (h, w, 4) debig_png_image promises"""
    px = rows.reshape(h, w, BPP[ct])
    if ct == 6:
        return px
    if ct == 2:
        return np.concatenate([px, np.full((h, w, 1), 255, np.uint8)], axis=2)
    idx = px[:, :, 0].astype(np.int64)
    return np.stack([pal[idx], pal[256 + idx], pal[512 + idx], np.full((h, w), 255, np.uint8)], axis=2)


def expected(im):
    if im.exp is not None:
        return im.exp
    key, stream = im.ref if im.ref is not None else (im.name, im.stream)
    return expand(ref_rows(key, stream, im.w, im.h, BPP[im.ct]), im.ct, im.w, im.h, im.pal)


def _top(name, ct, w, h, h_max, filters):
    """the first h rows of the image `name` of h_max rows (the same stream in every mode)"""
    st = make_stream(name, ct, w, h_max, filters)
    return Image(name, ct, w, h, st[: h * (w * BPP[ct] + 1)], ref=(name, st))


def zero_bad_rows(stream, w, bpp):
    """asserts_off = 1 in numpy: a row whose filter byte is above 4 decodes as zeros (pk_defilter<5>, m_keep = 0: what the reference's
    undo_PNG_filter returns without its assert) -- which is a row of filter type 0 whose bytes are all zero"""
    st = stream.reshape(-1, w * bpp + 1).copy()
    st[st[:, 0] > 4] = 0
    return st.reshape(-1)


def filter_forward(px, fts):
    """the scanline stream of the pixel rows px (h, w * bpp) under the filter types fts, by png_spec_ref._filter_row"""
    h, rb = px.shape
    out, prev = bytearray(), bytes(rb)
    for y in range(h):
        raw = px[y].tobytes()
        out.append(fts[y])
        out += R._filter_row(fts[y], raw, prev, 4)
        prev = raw
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def packed_filters(y):
    """the rows of the packed-arithmetic image: None on rows 0, 8, ..., Average on rows 4, 12, ..., Paeth on all others"""
    return 0 if y % 8 == 0 else 3 if y % 8 == 4 else 4


GROUPS = ("edges", "wrap-mixed", "wrap-paeth", "wrap-rest", "midrow", "align", "packed", "status")


def images(S, groups=GROUPS, wide=False):
    """{group: [Image]} for a mode with S band slots.  wide: with the 16400-pixel palette image and its tmp_off = 0 twin"""
    assert 1 <= S <= S_MAX
    out = {}
    if "edges" in groups:
        out["edges"] = []
        for ct in (6, 2, 3):
            for w, h in EDGES:
                name = "edge-ct%d-%dx%d" % (ct, w, h)
                out["edges"].append(Image(name, ct, w, h, make_stream(name, ct, w, h), pal=palette(name) if ct == 3 else None))
    # a slot takes a second band (64 S + 70 rows: S + 2 bands), slot 0 a third (128 S + 5 rows)
    for kind, filters in (("mixed", "mixed"), ("paeth", 4)):
        if "wrap-" + kind in groups:
            g = out["wrap-" + kind] = []
            for w in (1, 5, 67):
                g.append(_top("wrap-rgba-w%d-%s" % (w, kind), 6, w, 64 * S + 70, 64 * S_MAX + 70, filters))
            g.append(_top("wrap3-rgba-w5-%s" % kind, 6, 5, 128 * S + 5, 128 * S_MAX + 5, filters))
    if "wrap-rest" in groups:
        g = out["wrap-rest"] = [_top("wrap-rgb-w90", 2, 90, 64 * S + 3, 64 * S_MAX + 3, "mixed")]
        g.append(Image("wrap-palette-50x200", 3, 50, 200, make_stream("wrap-palette-50x200", 3, 50, 200),
                       pal=palette("wrap-palette-50x200")))  # stays on one slot: still right beside the others
    if "midrow" in groups:  # three bands, Paeth throughout: the band below waits for the row above it in mid-row
        g = out["midrow"] = []
        for w in MIDROW_W:
            name = "midrow-rgba-w%d" % w
            g.append(Image(name, 6, w, 130, make_stream(name, 6, w, 130, 4)))
        g.append(Image("midrow-rgb-w321", 2, 321, 130, make_stream("midrow-rgb-w321", 2, 321, 130, 4)))
    if "align" in groups:  # two bands at every stream_off & 3 and every rgba_off & 15 the output allows
        g = out["align"] = []
        for ct in (6, 2):
            st = make_stream("align-ct%d" % ct, ct, 9, 70)
            for sres in range(4):
                for rres in (0, 4, 8, 12):
                    g.append(Image("align-ct%d-s%d-r%d" % (ct, sres, rres), ct, 9, 70, st, sres=sres, rres=rres, ref=("align-ct%d" % ct, st)))
    if "packed" in groups:  # the GPU's packed 16-bit vector code against the emulator's scalar code, at the ends of a byte
        g = out["packed"] = []
        g.append(Image("packed-ends-67x130", 6, 67, 130, make_stream("packed-ends-67x130", 6, 67, 130, packed_filters, ENDS)))
        fts = [3 + (y & 1) for y in range(130)]  # a + b = 510 in the average, a = b = c = 255 in the predictor
        g.append(Image("packed-all255-67x130", 6, 67, 130, filter_forward(np.full((130, 67 * 4), 255, np.uint8), fts),
                       exp=np.full((130, 67, 4), 255, np.uint8)))
    if "status" in groups:  # what the kernel is built to report; no task breaks a bound
        g = out["status"] = []
        w, h = 40, 64 * S + 100
        name = "status-bad-rows"
        st = make_stream("%s-S%d" % (name, S), 6, w, h)
        for bad in (64 * S + 17, 70):  # a row past the wrap and an early row: the earlier one is reported
            st[bad * (4 * w + 1)] = 9
        g.append(Image(name, 6, w, h, st, expect=(0, 70)))
        g.append(Image(name + "-asserts-off", 6, w, h, st, asserts_off=1, ref=((name, S), zero_bad_rows(st, w, 4))))
        if wide:
            st = make_stream(WIDE, 3, PREVROW + 16, 130)
            g.append(Image(WIDE, 3, PREVROW + 16, 130, st, pal=palette(WIDE), tmp="scratch"))
            g.append(Image(WIDE + "-no-scratch", 3, PREVROW + 16, 130, st, pal=palette(WIDE), expect=(0, NO_ROW)))
    return out


def names(wide=True):
    """{group: the names of its images}: the same in every mode"""
    return {g: [im.name for im in v] for g, v in images(1, wide=wide).items()}


def filler(i):
    """a 1 x 1 RGBA image (fills a call up to the number of images that selects the mode): no neighbours, so every filter type
    leaves the four bytes as they are"""
    st = _rng("filler-%d" % i).integers(0, 256, 5, dtype=np.uint8)
    st[0] = i % 5
    return Image("filler-%d" % i, 6, 1, 1, st, exp=st[1:].reshape(1, 1, 4).copy())


def _aligned(nbytes, fill):
    """nbytes at a multiple of 64, as a view into a larger array (the launch seam uploads the whole array at the same residue)"""
    root = np.full(nbytes + 64, fill, dtype=np.uint8)
    at = -root.ctypes.data % 64
    return root[at: at + nbytes]


def run(imgs, launch):
    """one call with the images `imgs`: lay out, launch, check.  -> (the output arena with the images that failed blanked,
    [(good, bad_row)]), for comparing two runs of the same call byte by byte"""
    n = len(imgs)
    so, ro, lay = 64, 64, []
    for i, im in enumerate(imgs):
        so = (so + 3) // 4 * 4 + (i & 3 if im.sres is None else im.sres)
        ro = (ro + 15) // 16 * 16 + (4 * i & 15 if im.rres is None else im.rres)
        e = {"so": so, "ro": ro, "po": 0, "to": 0}
        so += len(im.stream) + 16 + (i % 3)  # the arena stays readable 16 bytes past every stream
        ro += 4 * im.w * im.h + 16
        if im.pal is not None:
            e["po"] = so + 1
            so += 1 + 768
        if im.tmp == "scratch":
            e["to"] = ro = (ro + 3) // 4 * 4
            ro += im.w + 16
        lay.append(e)
    sa, ra = _aligned(so + 64, S_FILL), _aligned(ro + 64, O_FILL)
    img, res = (DebigPngImage * n)(), (DebigPngResult * n)()
    C.memset(res, R_FILL, C.sizeof(res))
    for i, (im, e) in enumerate(zip(imgs, lay)):
        sa[e["so"]: e["so"] + len(im.stream)] = im.stream
        if im.pal is not None:
            sa[e["po"]: e["po"] + 768] = im.pal
        img[i].stream_off, img[i].rgba_off, img[i].pal_off, img[i].tmp_off = e["so"], e["ro"], e["po"], e["to"]
        img[i].width, img[i].height, img[i].color_type, img[i].asserts_off = im.w, im.h, im.ct, im.asserts_off
        assert (sa.ctypes.data + e["so"]) & 3 == (i & 3 if im.sres is None else im.sres)
        assert (ra.ctypes.data + e["ro"]) & 15 == (4 * i & 15 if im.rres is None else im.rres)
    sa0, img0 = sa.copy(), bytes(img)
    assert launch(sa, ra, img, res, n) == 0
    assert np.array_equal(sa, sa0), "the stream arena was written"
    assert bytes(img) == img0, "the tasks were written"
    got = [(res[i].good, res[i].bad_row) for i in range(n)]
    redo = [im.name for im, r in zip(imgs, got) if r == (0, REDO) and im.expect != r]
    assert not redo, ("given up as REDO", redo)
    blank = ra.copy()
    for im, e, r in zip(imgs, lay, got):
        assert r == im.expect, (im.name, r, im.expect)
        size = 4 * im.w * im.h
        if r[0]:
            px = ra[e["ro"]: e["ro"] + size].reshape(im.h, im.w, 4)
            want = expected(im)
            if not np.array_equal(px, want):
                ys, xs = np.nonzero((px != want).any(axis=2))
                raise AssertionError((im.name, "%d wrong pixels, the first at row %d, x %d" % (len(ys), ys[0], xs[0])))
        else:  # what a failed image's rows hold depends on how far the other wavefronts came
            ra[e["ro"]: e["ro"] + size] = O_FILL
        blank[e["ro"]: e["ro"] + size] = O_FILL
        if e["to"]:
            blank[e["to"]: e["to"] + im.w + 16] = O_FILL
            ra[e["to"]: e["to"] + im.w + 16] = O_FILL
    assert (blank == O_FILL).all(), "the output arena was written outside the images"
    return ra, got


def calls(imgs, n):
    """the battery images in calls of exactly n images: battery images first, then 1 x 1 fillers up to n"""
    out = []
    for at in range(0, len(imgs), n):
        part = list(imgs[at: at + n])
        out.append(part + [filler(i) for i in range(n - len(part))])
    return out


def paeth_classes(stream, rows, w, h, bpp=4):
    """From the reference's intermediates alone, per channel, over the Paeth rows of an image: the (pick, tie) classes of the predictor
    that occur -- pick 0 / 1 / 2 for a / b / c by the rule on pa, pb, pc, tie = (pa == pb, pa == pc, pb == pc) -- and the extremes of
    b - c, a - c and a + b - 2 c.  -> [(classes, min and max of the three)] per channel"""
    ft = stream.reshape(h, w * bpp + 1)[:, 0]
    px = np.zeros((h + 1, w + 1, bpp), dtype=np.int64)  # a row of zeros above, a pixel of zeros to the left
    px[1:, 1:] = rows.reshape(h, w, bpp)
    a, b, c = px[1:, :-1], px[:-1, 1:], px[:-1, :-1]
    sel = ft == 4
    out = []
    for ch in range(bpp):
        A, B, Cc = a[sel, :, ch].ravel(), b[sel, :, ch].ravel(), c[sel, :, ch].ravel()
        pa, pb, pc = abs(B - Cc), abs(A - Cc), abs(A + B - 2 * Cc)
        pick = np.where((pa <= pb) & (pa <= pc), 0, np.where(pb <= pc, 1, 2))
        cls = set(zip(pick.tolist(), (pa == pb).tolist(), (pa == pc).tolist(), (pb == pc).tolist()))
        ext = [(int(v.min()), int(v.max())) for v in (B - Cc, A - Cc, A + B - 2 * Cc)]
        out.append((cls, ext))
    return out


def reachable_paeth_classes():
    """every (pick, tie) class some a, b, c in 0 .. 255 reach: with x = a - c and y = b - c, pa = |y|, pb = |x|, pc = |x + y|"""
    x, y = np.meshgrid(np.arange(-255, 256), np.arange(-255, 256))
    pa, pb, pc = abs(y).ravel(), abs(x).ravel(), abs(x + y).ravel()
    pick = np.where((pa <= pb) & (pa <= pc), 0, np.where(pb <= pc, 1, 2))
    return set(zip(pick.tolist(), (pa == pb).tolist(), (pa == pc).tolist(), (pb == pc).tolist()))
