"""CPU: the battery of the tuned 8-bit de-filter (tests/png_defilter_battery.py) on the lock-step emulator (tools/simt_emu), bit for
bit against the pure-Python de-filter tests/png_spec_ref.py: debig_png_defilter_kernel<1>, <2>, <4>, <8> and <16, 6> through
emu_png_defilter_batch_w, and the pixel-skew kernels <4, 16, true, true> and <8, 16, true, true> in ONE workgroup per image
(emu_png_defilter_mwg_w with G = 1: no wait across workgroups, which the emulator, running one workgroup at a time, could never
satisfy).  tests/test_gpu_png_defilter_battery.py runs the same battery through the product launcher on the MI355X, where the
packed arithmetic, the lane shift, the byte alignment, the wavefront meeting point and the system-scope accesses are other code
 and the hand-over between workgroups exists.

Also here: the contract of DEBIG_DEFILTER_NO_REDO (include/debig_hip.h) on emu_png_defilter_mwg_w, and what the packed-arithmetic
image reaches, asserted from the reference alone."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_binding as eb
import png_defilter_battery as B

# mode -> (S: the band slots of an image, wavefronts per workgroup, pixel-skew kernel); the highest S first, so that the references of
# the images whose height derives from S are computed once
MODES = {"w16": (16, 16, False), "w8": (8, 8, False), "px8": (8, 8, True), "w4": (4, 4, False), "px4": (4, 4, True),
         "w2": (2, 2, False), "w1": (1, 1, False)}
WIDE_MODE = "px4"  # the 16400-pixel palette image: one mode only, the kernel the GPU battery runs it on (it stays on one wavefront)


@pytest.fixture(scope="module")
def emu():
    L = eb.load_emu()
    L.emu_png_defilter_batch_w.restype = C.c_int
    L.emu_png_defilter_batch_w.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.emu_png_defilter_mwg_w.restype = C.c_int
    L.emu_png_defilter_mwg_w.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_uint32)]
    return L


def _launcher(emu, mode):
    S, nwd, px = MODES[mode]

    def launch(sa, ra, img, res, n):
        if not px:
            return emu.emu_png_defilter_batch_w(sa.ctypes.data, ra.ctypes.data, img, res, n, nwd)
        n_redo = C.c_uint32(7)
        rc = emu.emu_png_defilter_mwg_w(sa.ctypes.data, ra.ctypes.data, img, res, n, 1, nwd, C.byref(n_redo))
        assert n_redo.value == 0  # one workgroup per image waits for no other
        return rc

    return launch


CASES = [(m, g) for m in MODES for g in B.GROUPS]


def test_every_battery_image_runs_in_every_mode():
    names = B.names(wide=True)
    assert set(names) == set(B.GROUPS) and all(names.values())
    for mode, (S, nwd, px) in MODES.items():
        ran = [im.name for g in B.GROUPS if (mode, g) in CASES for im in B.images(S, (g,), wide=mode == WIDE_MODE)[g]]
        assert len(ran) == len(set(ran))
        left = {n for v in names.values() for n in v} - set(ran)
        assert left == (set() if mode == WIDE_MODE else {B.WIDE, B.WIDE + "-no-scratch"}), (mode, left)
    assert sorted({(nwd, px) for S, nwd, px in MODES.values()}) == [(1, False), (2, False), (4, False), (4, True), (8, False), (8, True),
                                                                     (16, False)]


@pytest.mark.parametrize("mode,group", CASES, ids=["%s-%s" % c for c in CASES])
def test_battery(emu, mode, group):
    imgs = B.images(MODES[mode][0], (group,), wide=mode == WIDE_MODE)[group]
    B.run(imgs, _launcher(emu, mode))


def _python_launch(flaw=None):
    """a back end that writes what the check expects, from the reference itself -- and, with a flaw, one byte that it must not"""

    def launch(sa, ra, img, res, n):
        for i in range(n):
            im = launch.imgs[i]
            res[i].good, res[i].bad_row = im.expect
            if im.expect[0]:
                ra[img[i].rgba_off: img[i].rgba_off + 4 * im.w * im.h] = B.expected(im).reshape(-1)
        k = n // 2
        if flaw == "pixel":
            ra[img[k].rgba_off + 4 * launch.imgs[k].w * launch.imgs[k].h - 1] ^= 1
        elif flaw == "before":
            ra[img[k].rgba_off - 1] ^= 1
        elif flaw == "behind":
            ra[img[k].rgba_off + 4 * launch.imgs[k].w * launch.imgs[k].h] ^= 1
        elif flaw == "stream":
            sa[img[k].stream_off] ^= 1
        elif flaw == "result":
            res[k].bad_row = 0
        elif flaw == "redo":
            res[k].good, res[k].bad_row = 0, B.REDO
        elif flaw == "task":
            img[k].height += 1
        elif flaw == "nothing":
            C.memset(res, B.R_FILL, C.sizeof(res))
        return 0

    return launch


@pytest.mark.parametrize("flaw", [None, "pixel", "before", "behind", "stream", "result", "redo", "task", "nothing"])
def test_the_check_sees_one_wrong_byte(flaw):
    """the runner's check on a back end that is right by construction, and on the same with one flaw each: the last byte of an
    image, the byte on either side of it, a stream byte, a result word, an image given up, a task field, and no work at all"""
    imgs = B.images(1, ("edges", "status"))
    imgs = imgs["edges"][:7] + imgs["status"]
    launch = _python_launch(flaw)
    launch.imgs = imgs
    if flaw is None:
        B.run(imgs, launch)
        return
    with pytest.raises(AssertionError):
        B.run(imgs, launch)


def test_packed_image_reaches_every_class_and_extreme():
    """What the packed-arithmetic image is there for, from the reference's intermediates alone: in every channel all ten reachable
    (pick, tie) classes of the Paeth predictor occur, b - c and a - c reach -255 and 255, a + b - 2 c reaches -510 and 510 (the ends of
    what a 16-bit lane of pk_sub / pk_add / pk_abs holds); the all-255 image has a = b = c = 255 and a + b = 510 on every inner pixel."""
    reachable = B.reachable_paeth_classes()
    assert len(reachable) == 10
    ends, full = B.images(1, ("packed",))["packed"]
    assert set(np.unique(ends.stream.reshape(130, -1)[:, 1:])) == set(B.ENDS.tolist())
    assert [int(f) for f in ends.stream.reshape(130, -1)[:10, 0]] == [0, 4, 4, 4, 3, 4, 4, 4, 0, 4]
    rows = B.ref_rows(ends.name, ends.stream, 67, 130, 4)
    for ch, (cls, ext) in enumerate(B.paeth_classes(ends.stream, rows, 67, 130)):
        assert cls == reachable, (ch, reachable - cls)
        assert ext == [(-255, 255), (-255, 255), (-510, 510)], (ch, ext)
    assert sorted(set(full.stream.reshape(130, -1)[:, 0].tolist())) == [3, 4]
    rows, bad, _ = B.R._unfilter(full.stream.tobytes(), 0, 67, 130, 268, 4)
    assert bad is None and (rows == 255).all()


def _contract_images(slots):
    """G = 2 workgroups: `slots` band slots.  Two images with more bands than that -- slot 0, whose workgroup the emulator runs
    first, waits for the last band of the round from a workgroup that has not started -- and two that fit the first workgroup's
    wavefronts"""
    out = []
    for name, ct, w, h in (("redo-rgba", 6, 9, 64 * (slots + 1) + 5), ("redo-rgb", 2, 6, 64 * slots + 1), ("fits-rgba", 6, 13, 64 * 4),
                           ("fits-rgb", 2, 21, 130)):
        out.append(B.Image(name, ct, w, h, B.make_stream("contract-" + name, ct, w, h)))
    return out


@pytest.mark.parametrize("wpw", [4, 8])
def test_no_redo_switch_leaves_the_given_up_images_redo(emu, wpw):
    """DEBIG_DEFILTER_NO_REDO set and not "0": the one-workgroup launch behind the several-workgroups launch is left out, an image
    that launch gave up stays good = 0, bad_row = 0xfffffffd, and an image that fits one workgroup is that launch's own work: good,
    the specification's pixels.  Unset, empty or "0": every image comes back good and right (the launch as before)."""
    g = 2
    imgs = _contract_images(g * wpw)
    seen = {}

    def launch(sa, ra, img, res, n):
        n_redo = C.c_uint32(0)
        rc = emu.emu_png_defilter_mwg_w(sa.ctypes.data, ra.ctypes.data, img, res, n, g, wpw, C.byref(n_redo))
        seen["n_redo"] = n_redo.value
        seen["res"] = [(res[i].good, res[i].bad_row) for i in range(n)]
        return rc

    old = os.environ.get("DEBIG_DEFILTER_NO_REDO")
    try:
        for value in (None, "", "0"):
            os.environ.pop("DEBIG_DEFILTER_NO_REDO", None)
            if value is not None:
                os.environ["DEBIG_DEFILTER_NO_REDO"] = value
            B.run(imgs, launch)
            assert seen["n_redo"] == 2  # given up by the first launch, decoded by the second
        os.environ["DEBIG_DEFILTER_NO_REDO"] = "1"
        for im in imgs[:2]:
            im.expect = (0, B.REDO)
        B.run(imgs, launch)
        assert seen["n_redo"] == 2 and seen["res"] == [(0, B.REDO), (0, B.REDO), (1, B.NO_ROW), (1, B.NO_ROW)]
    finally:
        os.environ.pop("DEBIG_DEFILTER_NO_REDO", None)
        if old is not None:
            os.environ["DEBIG_DEFILTER_NO_REDO"] = old
