"""TEST TOOLING: the launch seam of the four perspective kernels (csrc/png_persp_kernel.inc), on top of tests/stage_launch.py.

stage_launch.KERNELS lists the kernels of the batteries that exist; this module adds the four new ones' buffer roles -- those of
their warp twins -- for the duration of a call only and goes through stage_launch.launch, so stage_launch.backend ("emu" / "gpu")
and stage_launch.record are honoured.

    launch(kernel_name, buffer, ..., n_tasks, grid)       one launch of png_persp / png_persp_color / png_label_persp /
                                                          png_color_label_persp (the emulator library is loaded here)
    with as_persp(module, ps): module.run_...(...)        the runners of the warp batteries (test_emu_png_warp, test_emu_png_color,
                                                          test_emu_png_color_labels_warp) build warp tasks and call their module's
                                                          `launch`; inside the block that call extends every task by p[] and
                                                          launches the persp twin instead.  ps: one (p0, p1, p2) per JOB in the
                                                          runner's job order (a job's tasks follow each other, the first has
                                                          row0 == 0) -- so buffers, sentinels, arenas, row runs and grids are the
                                                          warp batteries' own."""
import contextlib
import ctypes as C
from unittest import mock

import stage_launch as SL
from emu_binding import load_emu

TWIN = {"png_warp": "png_persp", "png_warp_color": "png_persp_color", "png_label_warp": "png_label_persp",
        "png_color_label_warp": "png_color_label_persp"}
ROLES = {p: SL.KERNELS[w] for w, p in TWIN.items()}
TASK_BYTES = {"png_persp": 176, "png_persp_color": 184, "png_label_persp": 128, "png_color_label_persp": 144}  # include/debig_hip.h
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        for name, roles in ROLES.items():
            fn = getattr(L, "emu_%s_batch" % name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p] * len(roles) + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def launch(name, *args):
    assert name in ROLES, name
    with mock.patch.dict(SL.KERNELS, ROLES):
        return SL.launch(name, *args, emu=_emu)


_TYPES = {}


def persp_task_type(warp_task_type):
    """the persp task of a warp task type: the warp task, field for field, followed by int64 p[3]"""
    if warp_task_type not in _TYPES:
        _TYPES[warp_task_type] = type("Persp" + warp_task_type.__name__, (C.Structure,),
                                      {"_fields_": [("w", warp_task_type), ("p", C.c_int64 * 3)]})
    return _TYPES[warp_task_type]


def extend(tasks, n, ps):
    """a ctypes array of n warp tasks -> the array of their persp tasks, p[] from ps by job (see the module docstring)"""
    T = persp_task_type(type(tasks[0]))
    out = (T * n)()
    job = -1
    for k in range(n):
        job += tasks[k].row0 == 0
        C.memmove(C.addressof(out[k].w), C.addressof(tasks[k]), C.sizeof(tasks[k]))
        out[k].p[:] = [int(v) for v in ps[job]]
    assert job == len(ps) - 1, (job, len(ps))
    return out


@contextlib.contextmanager
def as_persp(module, ps):
    def _launch(name, *args, emu=None):
        roles = SL.KERNELS[name]
        bufs, n, grid = list(args[:-2]), args[-2], args[-1]
        at = roles.index(SL.TASKS)
        bufs[at] = extend(bufs[at], n, ps)
        assert C.sizeof(bufs[at]) == n * TASK_BYTES[TWIN[name]]
        return launch(TWIN[name], *bufs, n, grid)

    with mock.patch.object(module, "launch", _launch):
        yield
