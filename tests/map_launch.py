"""TEST TOOLING: the eight warp kernels under a projective or an elastic map (csrc/png_persp_kernel.inc, csrc/png_elastic_kernel.inc)
through the runners of the affine batteries, on top of tests/stage_launch.py, whose KERNELS lists them beside their warp twins.

    launch(kernel_name, buffer, ..., n_tasks, grid)       one launch of a persp or elastic kernel through stage_launch.launch
                                                          (backend and record are honoured; the emulator library is loaded here)
    with as_persp(module, ps): module.run_...(...)        the runners of the warp batteries (test_emu_png_warp, test_emu_png_color,
    with as_elastic(module, qs, grid): module.run_...()   test_emu_png_color_labels_warp) build warp tasks and call their module's
                                                          `launch`; inside the block that call extends every task by the map's tail
                                                          and launches the twin of that map instead -- so buffers, sentinels,
                                                          arenas, row runs and grids are the warp batteries' own.
                                                          ps: one (p0, p1, p2) per JOB in the runner's job order (a job's tasks
                                                          follow each other, the first has row0 == 0); qs: one quantised field
                                                          ((grid_h, grid_w, 2) integers) or None (no field: UINT64_MAX) per job,
                                                          grid = (grid_h, grid_w); the fields travel as one trailing buffer."""
import contextlib
import ctypes as C
from unittest import mock

import numpy as np

import stage_launch as SL
from emu_binding import load_emu

WARPS = ("png_warp", "png_warp_color", "png_label_warp", "png_color_label_warp")
TWIN = {m: {w: w.replace("warp", m) for w in WARPS} for m in ("persp", "elastic")}  # one table per map: warp kernel -> its twin
TASK_BYTES = {"png_persp": 176, "png_persp_color": 184, "png_label_persp": 128, "png_color_label_persp": 144,  # include/debig_hip.h
              "png_elastic": 168, "png_elastic_color": 176, "png_label_elastic": 120, "png_color_label_elastic": 136}
NO_FIELD = (1 << 64) - 1
_LIB = {}


class PerspTail(C.Structure):  # include/debig_hip.h: what a persp task adds to its warp task
    _fields_ = [("p", C.c_int64 * 3)]


class ElasticTail(C.Structure):  # ... and an elastic task
    _fields_ = [("field_off", C.c_uint64), ("grid_w", C.c_uint16), ("grid_h", C.c_uint16), ("reserved3", C.c_uint32)]


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        for twins in TWIN.values():
            for name in twins.values():
                fn = getattr(L, "emu_%s_batch" % name)
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p] * len(SL.KERNELS[name]) + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def launch(name, *args):
    assert any(name in twins.values() for twins in TWIN.values()), name
    return SL.launch(name, *args, emu=_emu)


_TYPES = {}


def task_type(warp_task_type, tail_type):
    """the task of a map: the warp task, field for field, followed by the fields of the map's tail"""
    if (warp_task_type, tail_type) not in _TYPES:
        _TYPES[warp_task_type, tail_type] = type(tail_type.__name__[:-4] + warp_task_type.__name__, (C.Structure,),
                                                 {"_fields_": [("w", warp_task_type)] + tail_type._fields_})
    return _TYPES[warp_task_type, tail_type]


def persp_task_type(warp_task_type):
    return task_type(warp_task_type, PerspTail)


def elastic_task_type(warp_task_type):
    return task_type(warp_task_type, ElasticTail)


def extend(tasks, n, tail_type, fill):
    """a ctypes array of n warp tasks -> the array of their tasks under a map; fill(task, job) sets the tail of each, job counted
    as the module docstring says -> (the array, the number of jobs)"""
    out = (task_type(type(tasks[0]), tail_type) * n)()
    job = -1
    for k in range(n):
        job += tasks[k].row0 == 0
        C.memmove(C.addressof(out[k].w), C.addressof(tasks[k]), C.sizeof(tasks[k]))
        fill(out[k], job)
    return out, job + 1


def persp_fill(ps):
    def fill(t, job):
        t.p[:] = [int(v) for v in ps[job]]
    return fill


def elastic_fill(offs, grid):
    def fill(t, job):
        t.field_off = offs[job]
        t.grid_h, t.grid_w = grid
    return fill


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


@contextlib.contextmanager
def as_map(module, twin, tail_type, fill, n_jobs, *trailing):
    """inside the block module.launch(warp kernel, ...) launches twin[warp kernel] on the extended tasks, `trailing` buffers behind
    the warp kernel's own"""
    def _launch(name, *args, emu=None):
        bufs, n, grid = list(args[:-2]), args[-2], args[-1]
        at = SL.KERNELS[name].index(SL.TASKS)
        bufs[at], jobs = extend(bufs[at], n, tail_type, fill)
        assert jobs == n_jobs, (jobs, n_jobs)
        assert C.sizeof(bufs[at]) == n * TASK_BYTES[twin[name]]
        return launch(twin[name], *bufs, *trailing, n, grid)

    with mock.patch.object(module, "launch", _launch):
        yield


def as_persp(module, ps):
    return as_map(module, TWIN["persp"], PerspTail, persp_fill(ps), len(ps))


def as_elastic(module, qs, grid):
    buf, offs = fields_buffer(qs)
    return as_map(module, TWIN["elastic"], ElasticTail, elastic_fill(offs, grid), len(offs), buf)
