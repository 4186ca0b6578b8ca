"""debig_hip_png_defilter_batch (include/debig_hip.h; csrc/png_kernel.inc: debig_png_defilter_kernel<NWD, BLK, MWG, PX>) called DIRECTLY on
the MI355X with the battery tests/png_defilter_battery.py, in every launch mode the launcher has, each chosen the way the product
chooses it: by the number of images in the call (battery images first, then 1 x 1 RGBA images up to n; all of them are checked).

    mode    n per call  environment                  kernel              band slots S per image
    g16x4        8      DEBIG_DEFILTER_NO_REDO=1     <4, 16, true, true>   64   16 workgroups of 4 wavefronts
    g8x4        17      DEBIG_DEFILTER_NO_REDO=1     <4, 16, true, true>   32
    g4x8        33      DEBIG_DEFILTER_NO_REDO=1     <8, 16, true, true>   32
    g2x8        65      DEBIG_DEFILTER_NO_REDO=1     <8, 16, true, true>   16
    w16          8      DEBIG_DEFILTER_RESIDENT=1    <16, 6>               16   one workgroup per image from here on
    w8 .. w1   129 / 257 / 513 / 1025                <8> <4> <2> <1>        8 / 4 / 2 / 1

Every n is the lowest of its bracket, so a several-workgroups grid is about half of the 256 CUs.  What this reaches that nothing else
does: on the emulator (tests/test_emu_png_defilter_battery.py, the same battery) pk_add / pk_sub / pk_abs / pk_neg_mask are scalar C,
png_lane_above a shuffle, png_funnel a shift, png_wave_sync a barrier, the sys_* accesses plain, and an image has ONE workgroup; here
they are packed 16-bit vector code, DPP, v_alignbyte, a fence with a barrier and a wait, system-scope atomics and a write-through
16-byte store -- and a band is handed from CU to CU.  The whole-call GPU tests cross into this code with smooth images under one
filter rule whose slots never take a second band.

Under DEBIG_DEFILTER_NO_REDO the one-workgroup launch that decodes again what the several-workgroups launch gave up is left out, so
an image that comes back good IS that launch's own work; none may come back REDO (the device is this job's alone and the grid is
half of it: a REDO here is a finding).  Each call also runs with the switch unset and must give the same bytes.

Bit for bit against tests/png_spec_ref.py; nothing is compared with the emulator, which is neither built nor loaded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_defilter_battery as B  # noqa: E402
import stage_launch as SL  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL = "png_defilter"
# mode -> (n per call, DEBIG_DEFILTER_RESIDENT or None, wavefronts per workgroup, workgroups per image); the highest S first, so
# that the references of the images whose height derives from S are computed once
MODES = {"g16x4": (8, None, 4, 16), "g8x4": (17, None, 4, 8), "g4x8": (33, None, 8, 4), "g2x8": (65, None, 8, 2),
         "w16": (8, "1", 16, 1), "w8": (129, None, 8, 1), "w4": (257, None, 4, 1), "w2": (513, None, 2, 1), "w1": (1025, None, 1, 1)}
WIDE_MODE = "g16x4"  # the 16400-pixel palette image: one mode only -- the one a call of a few such images takes
CASES = [(m, g) for m in MODES for g in B.GROUPS]


def launcher_rule(n, cus, resident=None):
    """debig_hip_png_defilter_batch's choice, restated: (wavefronts per workgroup, workgroups per image).  G from n, halved until
    n * G workgroups are resident together (one per CU; DEBIG_DEFILTER_RESIDENT overrides the CU count); G = 1: defilter_waves(n)"""
    g = 16 if n <= 16 else 8 if n <= 32 else 4 if n <= 64 else 2 if n <= 128 else 1
    wpw = 4 if n <= 32 else 8
    resident = cus if resident is None else int(resident)
    while g > 1 and n * g > resident:
        g >>= 1
    if g > 1:
        return wpw, g
    return (16 if n <= 64 else 8 if n <= 256 else 4 if n <= 512 else 2 if n <= 1024 else 1), 1


def test_the_device_gives_every_mode_of_the_table(gpu_device):
    import torch

    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    for mode, (n, resident, wpw, g) in MODES.items():
        assert launcher_rule(n, cus, resident) == (wpw, g), (mode, cus)
        assert launcher_rule(n - 1, cus, resident) != (wpw, g) or mode in ("g16x4", "w16"), (mode, "n is not the lowest of its bracket")
        if g > 1:
            assert n * g <= cus * 9 // 16, (mode, "more than about half of the CUs")
    # the shape overrides are read once per process: set, they would make every mode the same
    assert "DEBIG_DEFILTER_WAVES" not in os.environ and "DEBIG_DEFILTER_WGS" not in os.environ


def test_every_battery_image_runs_in_every_mode():
    names = B.names(wide=True)
    every = {n for v in names.values() for n in v}
    for mode, (n, resident, wpw, g) in MODES.items():
        ran = [im.name for gr in B.GROUPS if (mode, gr) in CASES for im in B.images(wpw * g, (gr,), wide=mode == WIDE_MODE)[gr]]
        assert len(ran) == len(set(ran))
        assert every - set(ran) == (set() if mode == WIDE_MODE else {B.WIDE, B.WIDE + "-no-scratch"}), mode
        for gr in B.GROUPS:  # battery images first, fillers up to n, every call of exactly n images
            imgs = B.images(1, (gr,), wide=mode == WIDE_MODE)[gr]
            cs = B.calls(imgs, n)
            assert all(len(c) == n for c in cs) and [im.name for c in cs for im in c if not im.name.startswith("filler")] == [im.name for im in imgs]
    assert sorted((wpw, g) for _, _, wpw, g in MODES.values()) == [(1, 1), (2, 1), (4, 1), (4, 8), (4, 16), (8, 1), (8, 2), (8, 4), (16, 1)]


@pytest.fixture
def launch(gpu_device, monkeypatch):
    monkeypatch.setattr(SL, "backend", "gpu")
    monkeypatch.setitem(SL.KERNELS, KERNEL, (SL.IN, SL.OUT, SL.TASKS, SL.OUT))
    assert "DEBIG_DEFILTER_WAVES" not in os.environ and "DEBIG_DEFILTER_WGS" not in os.environ
    return lambda sa, ra, img, res, n: SL.launch(KERNEL, sa, ra, img, res, n, 0)


@pytest.mark.parametrize("mode,group", CASES, ids=["%s-%s" % c for c in CASES])
def test_battery(launch, monkeypatch, mode, group):
    n, resident, wpw, g = MODES[mode]
    monkeypatch.delenv("DEBIG_DEFILTER_RESIDENT", raising=False)
    if resident is not None:
        monkeypatch.setenv("DEBIG_DEFILTER_RESIDENT", resident)
    imgs = B.images(wpw * g, (group,), wide=mode == WIDE_MODE)[group]
    for call in B.calls(imgs, n):
        monkeypatch.delenv("DEBIG_DEFILTER_NO_REDO", raising=False)
        plain = B.run(call, launch)  # the call as the product makes it: right pixels, whoever decoded them
        monkeypatch.setenv("DEBIG_DEFILTER_NO_REDO", "1")
        own = B.run(call, launch)  # no REDO launch: right pixels and no image given up (B.run asserts both)
        assert own[1] == plain[1] and np.array_equal(own[0], plain[0]), (mode, "the switch changes the bytes")
