"""TEST TOOLING: the launch seam of the four elastic kernels (csrc/png_elastic_kernel.inc), on top of tests/stage_launch.py.

stage_launch.KERNELS lists the kernels of the batteries that exist; this module adds the four new ones' buffer roles -- those of
their warp twins, followed by the fields' nodes -- for the duration of a call only and goes through stage_launch.launch, so
stage_launch.backend ("emu" / "gpu") and stage_launch.record are honoured.

    launch(kernel_name, buffer, ..., n_tasks, grid)       one launch of png_elastic / png_elastic_color / png_label_elastic /
                                                          png_color_label_elastic (the emulator library is loaded here)
    with as_elastic(module, qs, grid): module.run_...()   the runners of the warp batteries (test_emu_png_warp, test_emu_png_color,
                                                          test_emu_png_color_labels_warp) build warp tasks and call their module's
                                                          `launch`; inside the block that call extends every task by the field
                                                          words and launches the elastic twin instead.  qs: one quantised field
                                                          ((grid_h, grid_w, 2) integers) or None (no field: UINT64_MAX) per JOB in
                                                          the runner's job order (a job's tasks follow each other, the first has
                                                          row0 == 0); grid = (grid_h, grid_w) -- so buffers, sentinels, arenas, row
                                                          runs and grids are the warp batteries' own."""
import contextlib
import ctypes as C
from unittest import mock

import numpy as np

import stage_launch as SL
from emu_binding import load_emu

TWIN = {"png_warp": "png_elastic", "png_warp_color": "png_elastic_color", "png_label_warp": "png_label_elastic",
        "png_color_label_warp": "png_color_label_elastic"}
ROLES = {e: SL.KERNELS[w] + (SL.IN,) for w, e in TWIN.items()}
TASK_BYTES = {"png_elastic": 168, "png_elastic_color": 176, "png_label_elastic": 120, "png_color_label_elastic": 136}  # debig_hip.h
NO_FIELD = (1 << 64) - 1
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


def elastic_task_type(warp_task_type):
    """the elastic task of a warp task type: the warp task, field for field, followed by field_off, grid_w, grid_h and padding"""
    if warp_task_type not in _TYPES:
        _TYPES[warp_task_type] = type("Elastic" + warp_task_type.__name__, (C.Structure,),
                                      {"_fields_": [("w", warp_task_type), ("field_off", C.c_uint64), ("grid_w", C.c_uint16),
                                                    ("grid_h", C.c_uint16), ("reserved3", C.c_uint32)]})
    return _TYPES[warp_task_type]


def fields_buffer(qs, lead=16):
    """the quantised fields one behind the other behind `lead` bytes -> (the buffer as uint8, the offset of each; NO_FIELD for None)"""
    parts, offs, at = [np.full(lead, 0xEE, np.uint8)], [], lead
    for q in qs:
        if q is None:
            offs.append(NO_FIELD)
            continue
        b = np.ascontiguousarray(q, dtype=np.int32).reshape(-1).view(np.uint8)
        offs.append(at)
        parts.append(b)
        at += len(b)
    return np.concatenate(parts), offs


def extend(tasks, n, offs, grid):
    """a ctypes array of n warp tasks -> the array of their elastic tasks, field_off from offs by job (see the module docstring)"""
    T = elastic_task_type(type(tasks[0]))
    out = (T * n)()
    job = -1
    for k in range(n):
        job += tasks[k].row0 == 0
        C.memmove(C.addressof(out[k].w), C.addressof(tasks[k]), C.sizeof(tasks[k]))
        out[k].field_off = offs[job]
        out[k].grid_h, out[k].grid_w = grid
    assert job == len(offs) - 1, (job, len(offs))
    return out


@contextlib.contextmanager
def as_elastic(module, qs, grid):
    buf, offs = fields_buffer(qs)

    def _launch(name, *args, emu=None):
        roles = SL.KERNELS[name]
        bufs, n, g = list(args[:-2]), args[-2], args[-1]
        at = roles.index(SL.TASKS)
        bufs[at] = extend(bufs[at], n, offs, grid)
        assert C.sizeof(bufs[at]) == n * TASK_BYTES[TWIN[name]]
        return launch(TWIN[name], *bufs, buf, n, g)

    with mock.patch.object(module, "launch", _launch):
        yield
