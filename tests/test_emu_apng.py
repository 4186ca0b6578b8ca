"""The APNG composite kernel (csrc/apng_kernel.inc: debig_apng_composite_kernel) on the CPU lock-step emulator, plain and
under ASan/UBSan, against the numpy compositor of tests/apng_ref.py on random frame buffers: every (dispose, blend) pair,
regions touching each canvas edge, 1 x 1 frames and canvases, canvas widths 1..70, output slots at every offset mod 16,
1 and 40+ frames, tasks of every size and fewer workgroups than tasks.  Every byte outside the canvases must stay
untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apng_ref as A  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402


class FrameDesc(C.Structure):  # include/debig_hip.h: debig_apng_frame_desc
    _fields_ = [("rgba_off", C.c_uint64), ("x_off", C.c_uint32), ("y_off", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("dispose_op", C.c_uint8), ("blend_op", C.c_uint8), ("reserved", C.c_uint16),
                ("reserved2", C.c_uint32)]


class Task(C.Structure):  # include/debig_hip.h: debig_apng_task
    _fields_ = [("out_off", C.c_uint64), ("ftab_off", C.c_uint64), ("px0", C.c_uint64), ("n_px", C.c_uint32),
                ("n_frames", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


assert C.sizeof(FrameDesc) == 32 and C.sizeof(Task) == 40
TASK_PX = 1024  # DEBIG_APNG_TASK_PX
FILL = 0xEE
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_APNG_EMU_ASAN") == "1")
        L.emu_apng_composite_batch.restype = C.c_int
        L.emu_apng_composite_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def random_file(rng, W, H, n_frames, ops=None, full_first=False):
    """(W, H, frames [(pixels, fcTL dict)]): random regions (some touching the edges), ops and pixels; alpha 0, 255 and
    fractional"""
    frames = []
    for k in range(n_frames):
        if (full_first and k == 0) or rng.random() < 0.15:
            x, y, w, h = 0, 0, W, H
        else:
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            x = int(rng.choice([0, W - w, rng.integers(0, W - w + 1)]))
            y = int(rng.choice([0, H - h, rng.integers(0, H - h + 1)]))
        dop, bop = ops[k % len(ops)] if ops else (int(rng.integers(0, 3)), int(rng.integers(0, 2)))
        px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        a = rng.random((h, w))
        px[..., 3] = np.where(a < 0.3, 0, np.where(a < 0.6, 255, px[..., 3]))
        frames.append((px, dict(x=x, y=y, width=w, height=h, dispose=dop, blend=bop)))
    return W, H, frames


def run(files, out_misalign=None, task_px=TASK_PX, grid=0, frame_misalign=4):
    """composite files (random_file tuples) in one launch -> [(F, H, W, 4) arrays]; every other byte must stay FILL"""
    nf = sum(len(f[2]) for f in files)
    arena = bytearray(32 * nf)
    descs, tasks, outs = [], [], []
    out_total = 64
    q = 0
    for i, (W, H, frames) in enumerate(files):
        ftab_off = 32 * q
        for px, fr in frames:
            arena += bytes((-len(arena)) % 16 + frame_misalign % 16)  # frames at 4 mod 16 by default
            d = FrameDesc()
            d.rgba_off = len(arena)
            d.x_off, d.y_off, d.width, d.height = fr["x"], fr["y"], fr["width"], fr["height"]
            d.dispose_op, d.blend_op = fr["dispose"], fr["blend"]
            descs.append(d)
            arena += px.tobytes()
            q += 1
        m = out_misalign[i] if out_misalign is not None else i % 16
        out_off = out_total + m
        outs.append((out_off, len(frames) * W * H * 4))
        out_total = out_off + len(frames) * W * H * 4 + 16 + (-(out_off + len(frames) * W * H * 4)) % 16
        for p0 in range(0, W * H, task_px):
            t = Task()
            t.out_off, t.ftab_off, t.px0 = out_off, ftab_off, p0
            t.n_px, t.n_frames, t.width, t.height = min(task_px, W * H - p0), len(frames), W, H
            tasks.append(t)
    arena += bytes(64)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    ft = (FrameDesc * nf)(*descs)
    C.memmove(a.ctypes.data, ft, C.sizeof(ft))
    out = np.full(out_total + 64, FILL, dtype=np.uint8)
    TT = (Task * len(tasks))(*tasks)
    assert launch("apng_composite", a, out, TT, len(tasks), grid, emu=_emu) == 0
    untouched = np.ones(len(out), dtype=bool)
    res = []
    for (W, H, frames), (off, size) in zip(files, outs):
        untouched[off: off + size] = False
        res.append(out[off: off + size].reshape(len(frames), H, W, 4))
    assert (out[untouched] == FILL).all(), "bytes outside the canvases were written"
    return res


def _check(files, **kw):
    for (W, H, frames), got in zip(files, run(files, **kw)):
        exp = A.composite([px for px, _ in frames], [fr for _, fr in frames], W, H)
        assert np.array_equal(got, exp), ((W, H, [fr for _, fr in frames]), np.argwhere(got != exp)[:4])


OPS = [(d, b) for d in range(3) for b in range(2)]


@pytest.mark.parametrize("dop,bop", OPS)
def test_every_op_pair(dop, bop):
    rng = np.random.default_rng(dop * 2 + bop)
    files = [random_file(rng, 37, 29, 6, ops=[(dop, bop)]) for _ in range(3)]
    files.append(random_file(rng, 23, 11, 6, ops=[(dop, bop), (2, 1), (1, 0)]))
    _check(files)


def test_regions_at_every_edge_and_every_op_sequence():
    rng = np.random.default_rng(11)
    W, H = 17, 13
    files = []
    for k, (x, y, w, h) in enumerate([(0, 0, 5, 4), (W - 5, 0, 5, 4), (0, H - 4, 5, 4), (W - 5, H - 4, 5, 4),
                                      (0, 3, W, 2), (6, 0, 2, H), (0, 0, W, H), (W - 1, H - 1, 1, 1)]):
        frames = []
        for j in range(8):
            px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
            fr = dict(x=x, y=y, width=w, height=h, dispose=OPS[(j + k) % 6][0], blend=OPS[(j + k) % 6][1])
            if j % 2:  # shift a neighbour region in between
                fr = dict(fr, x=0, y=0, width=W, height=H)
                px = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
            frames.append((px, fr))
        files.append((W, H, frames))
    _check(files)


def test_one_by_one():
    rng = np.random.default_rng(12)
    files = [random_file(rng, 1, 1, n) for n in (1, 2, 5, 41)]
    files.append((9, 7, [(rng.integers(0, 256, size=(1, 1, 4), dtype=np.uint8),
                          dict(x=x, y=y, width=1, height=1, dispose=d, blend=b))
                         for x, y, d, b in [(0, 0, 2, 1), (8, 6, 1, 1), (4, 3, 0, 0), (8, 0, 2, 0), (0, 6, 1, 1)]]))
    _check(files)


def test_widths_1_to_70():
    rng = np.random.default_rng(13)
    files = [random_file(rng, w, 1 + w % 5, 3 + w % 4) for w in range(1, 71)]
    _check(files)


@pytest.mark.parametrize("frame_misalign", [0, 4, 8, 12])
def test_output_slots_at_every_offset(frame_misalign):
    rng = np.random.default_rng(14 + frame_misalign)
    files = [random_file(rng, 5 + k % 7, 3 + k % 4, 3) for k in range(16)]
    _check(files, out_misalign=list(range(16)), frame_misalign=frame_misalign)


def test_many_frames_and_task_shapes():
    rng = np.random.default_rng(15)
    files = [random_file(rng, 45, 31, 43), random_file(rng, 70, 20, 1), random_file(rng, 33, 35, 40, full_first=True)]
    _check(files)
    _check(files, task_px=37)
    _check(files, task_px=1000, grid=3)


def test_kernel_under_address_sanitizer():
    """the same kernel source under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so), in a child process"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import numpy as np
import test_emu_apng as E
rng = np.random.default_rng(21)
files = [E.random_file(rng, w, 1 + w %% 4, 1 + w %% 6) for w in range(1, 40, 3)]
files += [E.random_file(rng, 1, 1, 3), E.random_file(rng, 37, 29, 41)]
E._check(files, out_misalign=[k %% 16 for k in range(len(files))])
E._check(files, task_px=7, grid=2, frame_misalign=12)
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_APNG_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
