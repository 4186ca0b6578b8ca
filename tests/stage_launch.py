"""TEST TOOLING: the one launch seam of the tensor-stage kernel batteries (tests/test_emu_png_*.py, tests/test_emu_apng.py).

    launch(kernel_name, buffer, ..., n_tasks, grid, emu=<the module's lazy emulator loader>)

runs one launch of a kernel whose workgroups loop over their tasks (`for (ti = blockIdx.x; ti < n_tasks; ti += gridDim.x)`) with
`grid` workgroups (0: one per task) and returns the launcher's return code.  A buffer is a numpy array (a view into a larger
array stands for the address it starts at), a ctypes array or None.

`backend` selects where:
  "emu"  (default) emu_<kernel_name>_batch of the CPU lock-step emulator (tools/simt_emu), on the host buffers themselves.  The
         library is loaded by the `emu` callable at the first launch, never on import.
  "gpu"  debig_hip_<kernel_name>_batch of the product library on the current torch stream, with DEBIG_STAGE_GRID
         (include/debig_hip.h) set to `grid`.  Every buffer is uploaded whole (for a view: the array it is a view of, so the
         sentinels in front of an output travel too) to an address with the host address's residue mod 64, and every buffer
         comes back: the outputs (KERNELS) are copied over the host arrays, the inputs and the bytes around every buffer must be
         unchanged.  tests/test_gpu_png_stage_kernels.py runs the batteries this way.

The four launchers of the general PNG de-filter (NO_GRID: png_spec_defilter, _fmt, _planar, _index) start one workgroup per task and
take no grid: for them `grid` must be 0, the emulator twin gets none and DEBIG_STAGE_GRID is left as it is.  Their first buffer is
the arena (INOUT): the kernel reads the streams and palettes in it and writes the tasks' scratch rings, which lie in it too, so it
is uploaded and copied back like an output, and its runner (tests/test_emu_png_spec.py: launch_defilter) asserts which bytes of it
may have changed.  tests/test_gpu_png_defilter_kernels.py runs their batteries on the GPU."""
import ctypes as C
import os

import numpy as np

IN, OUT, TASKS, INOUT = "in", "out", "tasks", "inout"
# kernel name -> its buffer arguments in the launchers' order (include/debig_hip.h); OUT: the kernel writes or accumulates into it;
# INOUT: it reads the buffer and writes a part of it that the caller knows (copied back like OUT, the caller checks the rest)
KERNELS = {
    "apng_composite": (IN, OUT, TASKS),
    "png_resize": (IN, OUT, TASKS, IN),
    "png_resize_alpha": (IN, OUT, TASKS, IN),
    "png_resize_cubic": (IN, OUT, TASKS, IN),
    "png_resize_color": (IN, OUT, TASKS, IN),
    "png_label_gather": (IN, OUT, TASKS, IN, IN),
    "png_color_label": (IN, OUT, TASKS, IN, OUT),
    "png_warp": (IN, OUT, TASKS),
    "png_warp_color": (IN, OUT, TASKS, IN),
    "png_label_warp": (IN, OUT, TASKS, IN),
    "png_color_label_warp": (IN, OUT, TASKS, IN, OUT),
    "png_tone_hist": (IN, OUT, TASKS),
    "png_tone_apply": (IN, OUT, TASKS, IN, IN),
    "png_blur": (IN, OUT, TASKS, IN),
    "png_spec_defilter": (INOUT, OUT, TASKS, OUT),
    "png_spec_defilter_fmt": (INOUT, OUT, TASKS, OUT),
    "png_spec_defilter_planar": (INOUT, OUT, TASKS, OUT),
    "png_spec_defilter_index": (INOUT, OUT, TASKS, OUT),
}
# the launchers without a task loop: one workgroup per task, no grid argument in the emulator twin, DEBIG_STAGE_GRID not read
NO_GRID = {"png_spec_defilter", "png_spec_defilter_fmt", "png_spec_defilter_planar", "png_spec_defilter_index"}
# the warp kernels under the other two maps: a persp kernel has the buffers of its warp twin, an elastic kernel its twin's and the fields
for _w in ("png_warp", "png_warp_color", "png_label_warp", "png_color_label_warp"):
    KERNELS[_w.replace("warp", "persp")] = KERNELS[_w]
    KERNELS[_w.replace("warp", "elastic")] = KERNELS[_w] + (IN,)
backend = "emu"
record = None  # a list: every launch appends (kernel name, the task array, n_tasks, grid), for tests that assert what ran
SLACK, GUARD = 64, 0xA5


def launch(name, *args, emu=None):
    bufs, n, grid = args[:-2], args[-2], args[-1]
    assert len(bufs) == len(KERNELS[name]), name
    if record is not None:
        record.append((name, bufs[KERNELS[name].index(TASKS)], n, grid))
    if name in NO_GRID:
        assert grid == 0, (name, "starts one workgroup per task")
    if backend == "emu":
        ptrs = [b.ctypes.data if isinstance(b, np.ndarray) else b for b in bufs]
        return getattr(emu(), "emu_%s_batch" % name)(*ptrs, n, *(() if name in NO_GRID else (grid,)))
    assert backend == "gpu", backend
    return _gpu_launch(name, bufs, n, grid)


def _root(b):
    """(the bytes of the whole array that b is a view of, b's offset in them)"""
    if not isinstance(b, np.ndarray):  # a ctypes array
        return np.frombuffer(b, np.uint8), 0
    root = b
    while isinstance(root.base, np.ndarray):
        root = root.base
    assert root.flags.c_contiguous
    return root.reshape(-1).view(np.uint8), b.ctypes.data - root.ctypes.data


def _gpu_launch(name, bufs, n, grid):
    import torch

    from debigulator_amd import _native as N

    fn = getattr(N.lib(), "debig_hip_%s_batch" % name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * len(bufs) + [C.c_uint32, C.c_void_p]
    dev = torch.device("cuda", torch.cuda.current_device())
    ptrs, held = [], []
    for role, b in zip(KERNELS[name], bufs):
        if b is None:
            ptrs.append(None)
            continue
        host, off = _root(b)
        shift = SLACK + host.ctypes.data % 64  # (torch's blocks start at a multiple of 512)
        stage = bytearray([GUARD]) * (shift + len(host) + SLACK)
        stage[shift: shift + len(host)] = host.tobytes()
        t = torch.frombuffer(stage, dtype=torch.uint8).to(dev)
        assert t.data_ptr() % 64 == 0
        ptrs.append(t.data_ptr() + shift + off)
        held.append((role, host, shift, stage, t))
    old = os.environ.get("DEBIG_STAGE_GRID")
    if grid:
        os.environ["DEBIG_STAGE_GRID"] = str(grid)
    elif name not in NO_GRID:
        os.environ.pop("DEBIG_STAGE_GRID", None)
    try:
        rc = fn(*ptrs, n, torch.cuda.current_stream().cuda_stream)
    finally:
        if old is None:
            os.environ.pop("DEBIG_STAGE_GRID", None)
        else:
            os.environ["DEBIG_STAGE_GRID"] = old
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    for role, host, shift, stage, t in held:
        back = t.cpu().numpy()
        end = shift + len(host)
        assert (back[:shift] == GUARD).all() and (back[end:] == GUARD).all(), (name, role, "bytes around the buffer were written")
        if role in (OUT, INOUT):
            host[:] = back[shift:end]
        else:
            assert back[shift:end].tobytes() == bytes(stage[shift:end]), (name, role, "an input buffer was written")
    return rc
