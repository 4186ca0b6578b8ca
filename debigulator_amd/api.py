"""Host-side mirror of the reference's interface, over the C drop-in layer.

Same names, argument meaning and error behaviour as the reference headers
(src/inflate.h:51-60, src/decode_png.h:69-103, src/decode_gz.h:23-38); every call goes
through the C-ABI of libdebigulator_hip.so (include/inflate.h, decode_png.h, decode_gz.h)
and runs on the GPU.  No CPU fallback exists: without the library or a GPU these raise.
"""
import ctypes as C

import numpy as np

from . import _native as N

_configured = False
NOT_SET = 0xFFFFFFFFFFFFFFFF


class DecodedData(C.Structure):
    _fields_ = [("data", C.c_void_p), ("data_size", C.c_uint32), ("good", C.c_uint32)]


def _lib():
    global _configured
    L = N.lib()
    if not _configured:
        vp, u8p, u32, u64 = C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint64
        L.debig_inflate.restype = None
        L.debig_inflate.argtypes = [vp, u64, C.POINTER(u64), vp, u64, vp, u64, C.POINTER(u32), u32]
        L.debig_inflate_batch.restype = C.c_int
        L.debig_inflate_batch.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32]
        L.decode_png_init.restype = None
        L.decode_png_init.argtypes = [vp, vp, vp, vp, u32, u32]
        L.decode_png_deinit.argtypes = [u32]
        L.decode_png_get_width_height.argtypes = [vp, u64, C.POINTER(u32), C.POINTER(u32), u8p]
        L.decode_png.restype = None
        L.decode_png.argtypes = [vp, u64, vp, u64, u32, u8p]
        L.debig_decode_png_batch.restype = C.c_int
        L.debig_decode_png_batch.argtypes = [vp, vp, vp, vp, vp, u32, u32]
        L.init_decode_gz.argtypes = [vp, vp, vp]
        L.decode_gz.restype = C.POINTER(DecodedData)
        L.decode_gz.argtypes = [vp, u32]
        L.init_PNG_decoder.argtypes = [vp]
        L.get_PNG_width_height.argtypes = [vp, u64, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.decode_PNG.argtypes = [vp, u64, vp, u64, C.POINTER(u32)]
        _configured = True
    return L


_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]
_libc.free.argtypes = [C.c_void_p]


def _fn(name):
    return C.cast(getattr(_libc, name), C.c_void_p)


def _u8(b):
    return np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b)


def inflate(data, recipient_size, thread_id=0):
    """reference inflate(): -> (good, final_recipient_size or None if untouched, bytes)"""
    L = _lib()
    d = _u8(data)
    out = np.zeros(max(recipient_size, 1), dtype=np.uint8)
    fin = C.c_uint64(NOT_SET)
    good = C.c_uint32(7)
    L.debig_inflate(out.ctypes.data, recipient_size, C.byref(fin), None, 0, d.ctypes.data, len(d), C.byref(good), thread_id)
    final = None if fin.value == NOT_SET else fin.value
    return good.value, final, out[: min(final or 0, recipient_size)].tobytes()


def inflate_batch(datas, recipient_sizes, thread_id=0):
    L = _lib()
    n = len(datas)
    ins = [_u8(d) for d in datas]
    outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in recipient_sizes]
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    out_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs])
    in_sizes = (C.c_uint64 * n)(*[len(a) for a in ins])
    caps = (C.c_uint64 * n)(*recipient_sizes)
    finals = (C.c_uint64 * n)(*([NOT_SET] * n))
    goods = (C.c_uint32 * n)()
    rc = L.debig_inflate_batch(out_ptrs, caps, finals, in_ptrs, in_sizes, goods, n, thread_id)
    N.check(rc, "debig_inflate_batch")
    res = []
    for i in range(n):
        final = None if finals[i] == NOT_SET else finals[i]
        res.append((goods[i], final, outs[i][: min(final or 0, recipient_sizes[i])].tobytes()))
    return res


_png_inited = set()


def decode_png_init(working_memory_size=120_000_000, thread_id=0):
    _lib().decode_png_init(_fn("malloc"), _fn("free"), _fn("memset"), _fn("memcpy"), working_memory_size, thread_id)
    _png_inited.add(thread_id)


def decode_png_get_width_height(data):
    d = _u8(data)
    w, h, g = C.c_uint32(), C.c_uint32(), C.c_uint8()
    _lib().decode_png_get_width_height(d.ctypes.data, len(d), C.byref(w), C.byref(h), C.byref(g))
    return w.value, h.value, g.value


def decode_png(data, thread_id=0, rgba_size=None):
    """reference decode_png(): -> (good, RGBA uint8 array of 4*w*h)"""
    if thread_id not in _png_inited:
        decode_png_init(thread_id=thread_id)
    d = _u8(data)
    w, h, _ = decode_png_get_width_height(d)
    n = w * h * 4 if rgba_size is None else rgba_size
    out = np.zeros(max(n, 1), dtype=np.uint8)
    good = C.c_uint8(7)
    _lib().decode_png(d.ctypes.data, len(d), out.ctypes.data, n, thread_id, C.byref(good))
    return good.value, out[:n]


def decode_png_batch(datas, thread_id=0):
    if thread_id not in _png_inited:
        decode_png_init(thread_id=thread_id)
    L = _lib()
    n = len(datas)
    ins = [_u8(d) for d in datas]
    sizes = []
    for a in ins:
        w, h, _ = decode_png_get_width_height(a)
        sizes.append(w * h * 4)
    outs = [np.zeros(max(s, 1), dtype=np.uint8) for s in sizes]
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_sizes = (C.c_uint64 * n)(*[len(a) for a in ins])
    out_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs])
    out_sizes = (C.c_uint64 * n)(*sizes)
    goods = (C.c_uint8 * n)()
    rc = L.debig_decode_png_batch(in_ptrs, in_sizes, out_ptrs, out_sizes, goods, n, thread_id)
    N.check(rc, "debig_decode_png_batch")
    return [(goods[i], outs[i][: sizes[i]]) for i in range(n)]


_gz_inited = False


def decode_gz(data):
    """reference decode_gz(): -> (good, bytes) ; None if the library returned NULL"""
    global _gz_inited
    L = _lib()
    if not _gz_inited:
        L.init_decode_gz(_fn("malloc"), _fn("memset"), _fn("memcpy"))
        _gz_inited = True
    d = _u8(data).copy()
    p = L.decode_gz(d.ctypes.data, len(d))
    if not p:
        return None
    dd = p.contents
    good, size = dd.good, dd.data_size
    out = C.string_at(dd.data, size) if (good and dd.data) else b""
    if dd.data:
        _libc.free(dd.data)
    _libc.free(C.cast(p, C.c_void_p))
    return good, out


def decode_gz_batch(datas, out_caps, verify_trailer=True):
    """n gzip members in one launch -> [(good, bytes, trailer_ok)]; trailer_ok = CRC-32 and ISIZE
    of the member match the decompressed bytes (checked on the GPU; the reference never checks)."""
    L = _lib()
    L.debig_decode_gz_batch_ex.restype = C.c_int
    L.debig_decode_gz_batch_ex.argtypes = [C.c_void_p] * 7 + [C.c_uint32]
    n = len(datas)
    ins = [_u8(d) for d in datas]
    outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in out_caps]
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_sizes = (C.c_uint32 * n)(*[len(a) for a in ins])
    out_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs])
    caps = (C.c_uint64 * n)(*out_caps)
    sizes = (C.c_uint64 * n)()
    goods = (C.c_uint32 * n)()
    tok = (C.c_uint32 * n)()
    rc = L.debig_decode_gz_batch_ex(in_ptrs, in_sizes, out_ptrs, caps, sizes, goods, tok if verify_trailer else None, n)
    N.check(rc, "debig_decode_gz_batch_ex")
    return [(goods[i], outs[i][: sizes[i]].tobytes(), tok[i]) for i in range(n)]


GZ_STATUS = {0: "ok", 1: "header", 2: "truncated", 3: "inflate", 4: "output_full", 5: "crc", 6: "isize", 7: "trailing"}


def gunzip_batch(datas, out_caps):
    """RFC 1952-complete gunzip of n files (include/decode_gz.h: debig_gunzip_batch): every
    member, every optional header field, CRC-32/ISIZE verified on the GPU.
    -> [(status, bytes, n_members)], status as in GZ_STATUS."""
    L = _lib()
    L.debig_gunzip_batch.restype = C.c_int
    L.debig_gunzip_batch.argtypes = [C.c_void_p] * 7 + [C.c_uint32]
    n = len(datas)
    ins = [_u8(d) for d in datas]
    outs = [np.zeros(max(c, 1), dtype=np.uint8) for c in out_caps]
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_sizes = (C.c_uint64 * n)(*[len(d) for d in datas])
    out_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs])
    caps = (C.c_uint64 * n)(*out_caps)
    sizes = (C.c_uint64 * n)()
    status = (C.c_uint32 * n)()
    members = (C.c_uint32 * n)()
    rc = L.debig_gunzip_batch(in_ptrs, in_sizes, out_ptrs, caps, sizes, status, members, n)
    N.check(rc, "debig_gunzip_batch")
    return [(status[i], outs[i][: sizes[i]].tobytes(), members[i]) for i in range(n)]


PNG_STATUS = {0: "ok", 1: "signature", 2: "chunk", 3: "ihdr", 4: "crc", 5: "zlib", 6: "inflate", 7: "adler",
              8: "data_short", 9: "data_long", 10: "filter", 11: "palette", 12: "output", 13: "animation", 14: "box", 15: "label",
              16: "warp", 17: "color", 18: "tone", 19: "blur", 20: "encode", 21: "range"}
PNG_FORCE_GENERAL = 1  # include/decode_png.h: DEBIG_PNG_FORCE_GENERAL


class PngInfo(C.Structure):  # include/decode_png.h: debig_png_info
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint8), ("color_type", C.c_uint8),
                ("interlace", C.c_uint8), ("has_trns", C.c_uint8), ("reserved", C.c_uint32)]


def _info_dict(inf):
    return {k: int(getattr(inf, k)) for k in ("width", "height", "bit_depth", "color_type", "interlace", "has_trns")}


def _png_spec_lib():
    L = N.lib()
    L.debig_png_info_get.restype = C.c_uint32
    L.debig_png_info_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PngInfo)]
    L.debig_png_decode_batch.restype = C.c_int
    L.debig_png_decode_batch.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32]
    L.debig_png_decode_batch_fmt.restype = C.c_int
    L.debig_png_decode_batch_fmt.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_uint32]
    L.debig_png_decode_batch_layout.restype = C.c_int
    L.debig_png_decode_batch_layout.argtypes = [C.c_void_p] * 6 + [C.c_uint32] * 4
    L.debig_png_decode_batch_dev.restype = C.c_int
    L.debig_png_decode_batch_dev.argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 4
    L.debig_png_out_layout.restype = C.c_uint64
    L.debig_png_out_layout.argtypes = [C.POINTER(PngInfo), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return L


# include/decode_png.h: out_format = layout | depth
PNG_MODES = {"rgba": 0, "rgb": 1, "gray": 2, "gray_alpha": 3, "native": 4}
PNG_DEPTHS = {8: 0x00, 16: 0x10, "native": 0x20}


def png_out_format(mode="rgba", depth=8):
    """(mode, depth) -> the out_format of debig_png_decode_batch_fmt"""
    if mode not in PNG_MODES:
        raise ValueError(f"mode must be one of {sorted(PNG_MODES)}, not {mode!r}")
    if isinstance(depth, bool) or depth not in PNG_DEPTHS:
        raise ValueError(f"depth must be 8, 16 or 'native', not {depth!r}")
    return PNG_MODES[mode] | PNG_DEPTHS[depth]


PNG_LAYOUTS = {"hwc": 0, "chw": 1}  # include/decode_png.h: DEBIG_PNG_LAYOUT_*
PNG_BAD_FORMAT, PNG_BAD_ARG = -1, -2  # DEBIG_PNG_BAD_FORMAT, DEBIG_PNG_BAD_ARG


def png_layout_code(layout="hwc"):
    """layout -> the out_layout of debig_png_decode_batch_layout / _dev"""
    if layout not in PNG_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(PNG_LAYOUTS)}, not {layout!r}")
    return PNG_LAYOUTS[layout]


def png_out_layout(info, mode="rgba", depth=8):
    """the output of one image (info: a png_info dict) in (mode, depth) -> (channels, bytes_per_sample, nbytes)
    (include/decode_png.h: debig_png_out_layout)"""
    inf = PngInfo(**{k: info[k] for k in ("width", "height", "bit_depth", "color_type", "interlace", "has_trns")})
    ch, bs = C.c_uint32(), C.c_uint32()
    nbytes = _png_spec_lib().debig_png_out_layout(C.byref(inf), png_out_format(mode, depth), C.byref(ch), C.byref(bs))
    if nbytes == 0:
        raise ValueError(f"no output layout for {info}")
    return ch.value, bs.value, int(nbytes)


def png_info(data):
    """signature, IHDR and the chunks up to the first IDAT (host only, include/decode_png.h: debig_png_info_get)
    -> (status, info dict), status as in PNG_STATUS"""
    d = _u8(data)
    inf = PngInfo()
    st = _png_spec_lib().debig_png_info_get(d.ctypes.data, len(d), C.byref(inf))
    return st, _info_dict(inf)


def png_decode_batch(datas, force_general=False, mode="rgba", depth=8, layout="hwc"):
    """every PNG the specification allows -> pixels (include/decode_png.h: debig_png_decode_batch_fmt / _layout).
    mode: "rgba" | "rgb" | "gray" | "gray_alpha" | "native" (as in the file); depth: 8 | 16 | "native" (16 for 16-bit
    files, else 8); layout: "hwc" (interleaved) | "chw" (channel planes).  -> [(status, ndarray (h, w, channels) -- or
    (channels, h, w) for "chw" -- of uint8 / uint16 or None, info dict)], status as in PNG_STATUS.  The defaults give
    RGBA8, (h, w, 4) uint8."""
    fmt = png_out_format(mode, depth)
    lay = png_layout_code(layout)
    L = _png_spec_lib()
    n = len(datas)
    ins = [_u8(d) for d in datas]
    outs, caps = [], []
    for a in ins:
        st, inf = png_info(a)
        if st == 0:
            ch, bs, nbytes = png_out_layout(inf, mode, depth)
            shape = (ch, inf["height"], inf["width"]) if lay else (inf["height"], inf["width"], ch)
            outs.append(np.empty(shape, dtype=np.uint16 if bs == 2 else np.uint8))
            caps.append(nbytes)
        else:
            outs.append(np.empty(4, dtype=np.uint8))
            caps.append(0)
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_sizes = (C.c_uint64 * n)(*[len(a) for a in ins])
    out_ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    caps = (C.c_uint64 * n)(*caps)
    status = (C.c_uint32 * n)()
    infos = (PngInfo * n)()
    if lay:
        rc = L.debig_png_decode_batch_layout(in_ptrs, in_sizes, out_ptrs, caps, status, infos, n,
                                             PNG_FORCE_GENERAL if force_general else 0, fmt, lay)
    else:
        rc = L.debig_png_decode_batch_fmt(in_ptrs, in_sizes, out_ptrs, caps, status, infos, n,
                                          PNG_FORCE_GENERAL if force_general else 0, fmt)
    N.check(rc, "debig_png_decode_batch_layout" if lay else "debig_png_decode_batch_fmt")
    return [(int(status[i]), outs[i] if status[i] == 0 else None, _info_dict(infos[i])) for i in range(n)]


def png_decode_batch_device(datas, mode="rgba", depth=8, layout="hwc", device="cuda:0", force_general=False):
    """png_decode_batch with the pixels left on the GPU (include/decode_png.h: debig_png_decode_batch_dev): no pixel byte
    goes to the host.  -> [(status, torch tensor or None, info dict)]; every tensor is a view of ONE torch.uint8 arena on
    `device` (offsets multiples of 16), shaped (h, w, channels) or, with layout="chw", (channels, h, w).  16-bit results
    have dtype torch.uint16 where the installed torch has it, else they are torch.int16 views of the same bits.  The call
    returns after the work has finished.  The library works on the calling thread's current device: any other `device`
    raises ValueError (select it with torch.cuda.set_device first)."""
    import torch

    fmt = png_out_format(mode, depth)
    lay = png_layout_code(layout)
    L = _png_spec_lib()
    dev = _png_device(L, device)
    n = len(datas)
    ins = [_u8(d) for d in datas]
    offs, caps, shapes, total = [], [], [], 0
    for a in ins:
        st, inf = png_info(a)
        offs.append(total)
        if st == 0:
            ch, bs, nbytes = png_out_layout(inf, mode, depth)
            shapes.append(((ch, inf["height"], inf["width"]) if lay else (inf["height"], inf["width"], ch), bs))
            caps.append(nbytes)
            total += (nbytes + 15) // 16 * 16
        else:
            shapes.append(None)
            caps.append(0)
    arena = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_sizes = (C.c_uint64 * n)(*[len(a) for a in ins])
    status = (C.c_uint32 * n)()
    infos = (PngInfo * n)()
    rc = L.debig_png_decode_batch_dev(in_ptrs, in_sizes, arena.data_ptr(), (C.c_uint64 * n)(*offs),
                                      (C.c_uint64 * n)(*caps), status, infos, n,
                                      PNG_FORCE_GENERAL if force_general else 0, fmt, lay)
    if rc in (PNG_BAD_FORMAT, PNG_BAD_ARG):
        raise ValueError(f"debig_png_decode_batch_dev rejected its arguments ({rc})")
    N.check(rc, "debig_png_decode_batch_dev")
    u16 = getattr(torch, "uint16", torch.int16)
    out = []
    for i in range(n):
        t = None
        if status[i] == 0:
            shape, bs = shapes[i]
            t = arena[offs[i]: offs[i] + caps[i]]
            t = (t.view(u16) if bs == 2 else t).view(shape)
        out.append((int(status[i]), t, _info_dict(infos[i])))
    return out


class PngBox(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


def _png_device(L, device):
    """the device rule of png_decode_batch_device and the dense-tensor calls -> the current device as a torch.device"""
    import torch

    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a GPU, not {device!r}")
    L.debig_hip_get_device.restype = C.c_int
    cur = L.debig_hip_get_device()
    if dev.index is not None and dev.index != cur:
        raise ValueError(f"device {device!r} is not the current device (cuda:{cur}), on which the library works")
    return torch.device("cuda", cur)


def _png_dense_out(shape, tdt, fill, dev):
    """the one tensor of a dense-tensor call: as allocated, or holding `fill`, once that fill has finished"""
    import torch

    if fill is None:
        out = torch.empty(shape, dtype=tdt, device=dev)
    elif tdt == getattr(torch, "uint16", None):  # (torch.full has no uint16 kernel: fill the same bits as int16)
        out = torch.full(shape, int(np.array(fill, np.uint16).view(np.int16)), dtype=torch.int16, device=dev).view(tdt)
    else:
        out = torch.full(shape, fill, dtype=tdt, device=dev)
    torch.cuda.synchronize(dev)  # the fill runs on torch's stream, the library on its own
    return out


def _png_batch_args(datas, boxes):
    """the per-file arguments of a dense-tensor call -> in_ptrs, in_sizes, boxes (or None), status, infos; in_ptrs keeps
    the bytes it points to alive"""
    n = len(datas)
    if boxes is not None and len(boxes) != n:
        raise ValueError("boxes needs one entry (or None) per file")
    ins = [_u8(x) for x in datas]
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_ptrs._ins = ins
    bx = None
    if boxes is not None:
        bx = (PngBox * n)(*[PngBox(*[int(v) for v in b]) if b is not None else PngBox(0, 0, 0, 0) for b in boxes])
    return in_ptrs, (C.c_uint64 * n)(*[len(a) for a in ins]), bx, (C.c_uint32 * n)(), (PngInfo * n)()


class PngTensorDesc(C.Structure):  # include/decode_png.h: debig_png_tensor_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("out_format", C.c_uint32), ("out_layout", C.c_uint32),
                ("dtype", C.c_uint32), ("resize_flags", C.c_uint32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


PNG_TENSOR_DTYPES = {"uint": 0, "float32": 1, "float16": 2, "bfloat16": 3}  # include/decode_png.h: DEBIG_PNG_T_*
PNG_RESIZE_ANTIALIAS = 1  # DEBIG_PNG_RESIZE_ANTIALIAS


def png_tensor_desc(size, mode="rgb", depth=8, dtype="float32", layout="chw", mean=None, std=None, antialias=True):
    """the debig_png_tensor_desc of png_decode_batch_tensor's arguments (no GPU needed) -> (desc, channels, element bytes).
    dtype: "float32" | "float16" | "bfloat16", or an integer result: "uint" ("uint8" with depth 8, "uint16" with depth 16)"""
    if mode == "native" or depth == "native":
        raise ValueError("png_decode_batch_tensor needs a concrete mode and depth: every image of the tensor has the same channels")
    fmt = png_out_format(mode, depth)
    lay = png_layout_code(layout)
    if dtype in ("uint8", "uint16"):
        if dtype != f"uint{depth}":
            raise ValueError(f"dtype {dtype!r} needs depth={dtype[4:]}")
        dtype = "uint"
    if dtype not in PNG_TENSOR_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(PNG_TENSOR_DTYPES)}, 'uint8' or 'uint16', not {dtype!r}")
    H, W = (int(v) for v in size)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"size must be (H, W) with 1 <= H, W <= 16384, not {size!r}")
    ch = {0: 4, 1: 3, 2: 1, 3: 2}[fmt & 15]
    d = PngTensorDesc(out_w=W, out_h=H, out_format=fmt, out_layout=lay, dtype=PNG_TENSOR_DTYPES[dtype],
                      resize_flags=PNG_RESIZE_ANTIALIAS if antialias else 0)

    def per_channel(v, name, default):
        if v is None:
            return [default] * ch
        v = [float(x) for x in (v if hasattr(v, "__len__") else [v] * ch)]
        if len(v) != ch:
            raise ValueError(f"{name} needs {ch} values for mode {mode!r}, not {len(v)}")
        return v

    m, sd = per_channel(mean, "mean", 0.0), per_channel(std, "std", 1.0)
    if (mean is not None or std is not None) and dtype == "uint":
        raise ValueError("mean / std need a float dtype")
    if any(x == 0.0 for x in sd):
        raise ValueError("std must not be 0")
    for k in range(4):
        d.scale[k] = np.float32(1.0 / sd[k]) if k < ch else 1.0  # in float64, then float32
        d.bias[k] = np.float32(-m[k] / sd[k]) if k < ch else 0.0
    if not all(np.isfinite(d.scale[k]) and np.isfinite(d.bias[k]) for k in range(4)):
        raise ValueError("mean / std give a non-finite scale or bias")
    return d, ch, (depth // 8 if dtype == "uint" else 4 if dtype == "float32" else 2)


class PngAlphaDesc(C.Structure):  # include/decode_png.h: debig_png_alpha_desc
    _fields_ = [("mode", C.c_uint32), ("background", C.c_uint16 * 4), ("reserved", C.c_uint32)]


PNG_ALPHA_MODES = {"straight": 0, "premultiplied": 1, "over": 2}  # include/decode_png.h: DEBIG_PNG_ALPHA_*


def png_alpha_desc(alpha="straight", background=None, mode="rgb", depth=8):
    """the debig_png_alpha_desc of png_decode_batch_tensor's alpha / background arguments (no GPU needed), or None for
    alpha="straight".  "over" needs mode "rgb" or "gray" (the tensor's channels) and composites over `background`: one value
    per output channel on the [0, 1] scale (a number: every channel; None: 1.0, white), stored as round(x * (2^depth - 1));
    "premultiplied" needs mode "rgba" or "gray_alpha"."""
    if alpha not in PNG_ALPHA_MODES:
        raise ValueError(f"alpha must be one of {sorted(PNG_ALPHA_MODES)}, not {alpha!r}")
    if alpha == "straight":
        if background is not None:
            raise ValueError("background needs alpha='over'")
        return None
    if depth not in (8, 16):
        raise ValueError("alpha needs a concrete depth (8 or 16)")
    d = PngAlphaDesc(mode=PNG_ALPHA_MODES[alpha])
    if alpha == "premultiplied":
        if mode not in ("rgba", "gray_alpha"):
            raise ValueError(f"alpha='premultiplied' needs mode 'rgba' or 'gray_alpha', not {mode!r}")
        if background is not None:
            raise ValueError("background needs alpha='over'")
        return d
    if mode not in ("rgb", "gray"):
        raise ValueError(f"alpha='over' needs mode 'rgb' or 'gray' (the channels of the tensor), not {mode!r}")
    ch = 3 if mode == "rgb" else 1
    if background is None:
        background = 1.0
    bg = [float(x) for x in (background if hasattr(background, "__len__") else [background] * ch)]
    if len(bg) != ch:
        raise ValueError(f"background needs {ch} values for mode {mode!r}, not {len(bg)}")
    if not all(0.0 <= x <= 1.0 for x in bg):  # (a NaN fails every comparison)
        raise ValueError(f"background values must lie in [0, 1], not {bg!r}")
    for k, x in enumerate(bg):
        d.background[k] = int(round(x * ((1 << depth) - 1)))
    return d


class PngFilterDesc(C.Structure):  # include/decode_png.h: debig_png_filter_desc
    _fields_ = [("filter", C.c_uint32), ("reserved", C.c_uint32)]


PNG_FILTERS = {"bilinear": 0, "bicubic": 1, "nearest": 2}  # include/decode_png.h: DEBIG_PNG_FILTER_*


def png_filter_desc(filter="bilinear"):
    """the debig_png_filter_desc of png_decode_batch_tensor's filter argument (no GPU needed), or None for "bilinear" (the
    calls without a filter).  "bicubic": the Keys kernel with a = -1/2, antialiased when it shrinks (at most 32 x per axis);
    "nearest": the source sample at the output pixel's centre, antialias ignored."""
    if filter not in PNG_FILTERS:
        raise ValueError(f"filter must be one of {sorted(PNG_FILTERS)}, not {filter!r}")
    if filter == "bilinear":
        return None
    return PngFilterDesc(filter=PNG_FILTERS[filter])


class PngWarp(C.Structure):  # include/decode_png.h: debig_png_warp
    _fields_ = [("m", C.c_double * 6)]


class PngWarpDesc(C.Structure):  # include/decode_png.h: debig_png_warp_desc
    _fields_ = [("filter", C.c_uint32), ("border_mode", C.c_uint32), ("border", C.c_uint16 * 4), ("alpha_mode", C.c_uint32),
                ("reserved", C.c_uint32)]


class PngLabelWarpDesc(C.Structure):  # include/decode_png.h: debig_png_label_warp_desc
    _fields_ = [("border_mode", C.c_uint32), ("border_label", C.c_int32)]


PNG_BORDERS = {"constant": 0, "clamp": 1}  # include/decode_png.h: DEBIG_PNG_BORDER_*
PNG_WARP_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def png_warp_matrix(src_wh, out_size, angle=0.0, scale=1.0, shear=(0, 0), translate=(0, 0), hflip=False, vflip=False):
    """the INVERSE 2 x 3 matrix (a tuple of two rows of three floats) that png_decode_batch_tensor(..., warp=) and
    png_decode_batch_labels(..., warp=) take, for a source (crop) of src_wh = (w, h) pixels and an output of out_size = (H, W),
    built about the two centres (no GPU needed).  Seen from the source to the output, the operations compose in this order:
      1. the flips (hflip: left <-> right, vflip: top <-> bottom);
      2. scale: a number or (sx, sy), > 1 enlarges;
      3. shear = (x, y) in degrees: x' = x + tan(x) y, y' = tan(y) x + y;
      4. the rotation by `angle` degrees, counter-clockwise as the image is seen (what PIL's and torchvision's rotate mean);
         multiples of 90 are exact;
      5. translate = (tx, ty) in OUTPUT pixels, to the right and down;
    and the source centre (w / 2, h / 2) lands on the output centre (W / 2, H / 2) before the translation.  With no other argument
    png_warp_matrix((w, h), (h, w)) is the identity; hflip, vflip and angle = 90 / 180 / 270 with the matching out_size give
    numpy.fliplr / flipud / rot90(k = 1, 2, 3) of the decode exactly."""
    import math

    w, h = (float(v) for v in src_wh)
    H, W = (float(v) for v in out_size)
    sx, sy = (float(v) for v in (scale if hasattr(scale, "__len__") else (scale, scale)))
    if sx == 0.0 or sy == 0.0:
        raise ValueError("scale must not be 0")
    a = float(angle) % 360.0
    if a % 90.0 == 0.0:
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(a // 90.0)]
    else:
        c, s = math.cos(math.radians(a)), math.sin(math.radians(a))
    tx_, ty_ = (math.tan(math.radians(float(v))) if float(v) != 0.0 else 0.0 for v in shear)
    det = 1.0 - tx_ * ty_
    if abs(det) < 1e-12:  # (tan(45 degrees) is not exactly 1 in float64)
        raise ValueError("the shear is singular")
    # the inverse chain, output -> source: rotation^-1, shear^-1, scale^-1, flips
    m = ((c, -s), (s, c))
    sh = ((1.0 / det, -tx_ / det), (-ty_ / det, 1.0 / det))
    m = tuple(tuple(sh[r][0] * m[0][k] + sh[r][1] * m[1][k] for k in range(2)) for r in range(2))
    fx, fy = (-1.0 if hflip else 1.0), (-1.0 if vflip else 1.0)
    m = (tuple(fx * v / sx for v in m[0]), tuple(fy * v / sy for v in m[1]))
    ox, oy = W / 2.0 + float(translate[0]), H / 2.0 + float(translate[1])
    rows = ((m[0][0], m[0][1], w / 2.0 - (m[0][0] * ox + m[0][1] * oy)),
            (m[1][0], m[1][1], h / 2.0 - (m[1][0] * ox + m[1][1] * oy)))
    return tuple(tuple(v + 0.0 for v in r) for r in rows)  # (+ 0.0: no negative zeros)


def _png_warps(warp, n):
    """warp: a sequence of n entries, each None (the identity) or a 2 x 3 matrix -> (PngWarp * n)"""
    if len(warp) != n:
        raise ValueError("warp needs one entry (a 2 x 3 matrix, or None) per file")
    ws = (PngWarp * n)()
    for i, m in enumerate(warp):
        v = PNG_WARP_IDENTITY if m is None else [float(x) for x in np.asarray(m, dtype=np.float64).reshape(-1)]
        if len(v) != 6:
            raise ValueError(f"warp[{i}] must be a 2 x 3 matrix")
        ws[i].m[:] = v
    return ws


class PngPersp(C.Structure):  # include/decode_png.h: debig_png_persp
    _fields_ = [("m", C.c_double * 9)]


PNG_PERSP_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def png_perspective_from_warp(m2x3):
    """the 3 x 3 matrix of `perspective=` that means what the 2 x 3 matrix of `warp=` means: (0, 0, 1) appended as row 2.  The
    calls then give the bytes of their warp= form."""
    v = [float(x) for x in np.asarray(m2x3, dtype=np.float64).reshape(-1)]
    if len(v) != 6:
        raise ValueError("png_perspective_from_warp takes a 2 x 3 matrix")
    return (tuple(v[0:3]), tuple(v[3:6]), (0.0, 0.0, 1.0))


def png_perspective_matrix(src_quad, out_size, dst_quad=None):
    """the INVERSE 3 x 3 matrix (a tuple of three rows of three floats, M22 = 1) that `perspective=` takes, from four point pairs
    (no GPU needed): the output point dst_quad[k] = (X, Y) maps to the crop point src_quad[k] = (x, y).  Both are continuous
    coordinates in which pixel j covers [j, j + 1); dst_quad defaults to the corners of the out_size = (H, W) output in the order
    (0, 0), (W, 0), (W, H), (0, H).  Solved in float64 (the eight-equation system of the homography); a degenerate
    quadrilateral raises ValueError.  Whether the horizon stays clear of the output is decided by the decode call (status 16)."""
    H, W = (float(v) for v in out_size)
    src = np.asarray(src_quad, dtype=np.float64).reshape(-1)
    dst = np.asarray(dst_quad if dst_quad is not None else ((0, 0), (W, 0), (W, H), (0, H)), dtype=np.float64).reshape(-1)
    if src.size != 8 or dst.size != 8:
        raise ValueError("png_perspective_matrix takes four (x, y) points per quadrilateral")
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k in range(4):
        X, Y, x, y = dst[2 * k], dst[2 * k + 1], src[2 * k], src[2 * k + 1]
        A[2 * k] = (X, Y, 1, 0, 0, 0, -x * X, -x * Y)
        A[2 * k + 1] = (0, 0, 0, X, Y, 1, -y * X, -y * Y)
        b[2 * k], b[2 * k + 1] = x, y
    try:
        h = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        raise ValueError("the quadrilaterals are degenerate") from None
    if not np.isfinite(h).all():
        raise ValueError("the quadrilaterals are degenerate")
    h = [float(v) + 0.0 for v in h] + [1.0]
    return (tuple(h[0:3]), tuple(h[3:6]), tuple(h[6:9]))


def _png_persps(perspective, n):
    """perspective: a sequence of n entries, each None (the identity) or a 3 x 3 matrix -> (PngPersp * n)"""
    if len(perspective) != n:
        raise ValueError("perspective needs one entry (a 3 x 3 matrix, or None) per file")
    ps = (PngPersp * n)()
    for i, m in enumerate(perspective):
        v = PNG_PERSP_IDENTITY if m is None else [float(x) for x in np.asarray(m, dtype=np.float64).reshape(-1)]
        if len(v) != 9:
            raise ValueError(f"perspective[{i}] must be a 3 x 3 matrix")
        ps[i].m[:] = v
    return ps


class PngElastic(C.Structure):  # include/decode_png.h: debig_png_elastic
    _fields_ = [("nodes", C.c_void_p)]


class PngElasticDesc(C.Structure):  # include/decode_png.h: debig_png_elastic_desc
    _fields_ = [("grid_w", C.c_uint32), ("grid_h", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def png_elastic_field(size, alpha, sigma, grid=None, rng=None):
    """a random displacement field for `elastic=` (numpy only, no GPU needed): an array of shape (grid_h, grid_w, 2) holding
    (dx, dy) per node IN OUTPUT PIXELS for an output of size = (H, W).  Uniform noise in [-1, 1] is drawn on the node grid,
    smoothed by a Gaussian of `sigma` output pixels (expressed in node spacings, edges replicated), scaled by `alpha` (a number, or
    (alpha_x, alpha_y)) and clipped to +-4096.  grid = (grid_h, grid_w), each 2 .. 33; by default the node spacing is about
    sigma.  rng: a numpy Generator, a seed, or None.  This is a GENERATOR in the spirit of torchvision's ElasticTransform, not a
    parity target: it does not reproduce that transform's random numbers or its full-resolution blur."""
    H, W = (int(v) for v in size)
    sigma = float(sigma)
    if H < 1 or W < 1 or not sigma > 0.0:
        raise ValueError("png_elastic_field needs a size of at least 1 x 1 and sigma > 0")
    if grid is None:
        grid = tuple(int(min(33, max(2, round(v / sigma) + 1))) for v in (H, W))
    gh, gw = (int(v) for v in grid)
    if not (2 <= gh <= 33 and 2 <= gw <= 33):
        raise ValueError("grid dimensions must lie in 2 .. 33")
    ax, ay = (float(v) for v in (alpha if hasattr(alpha, "__len__") else (alpha, alpha)))
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    f = rng.uniform(-1.0, 1.0, size=(gh, gw, 2))
    for axis, (g, extent) in enumerate(((gh, H), (gw, W))):
        s = sigma * (g - 1) / extent  # sigma in node spacings
        r = int(min(g - 1, np.ceil(3.0 * s)))
        if r < 1:
            continue
        k = np.exp(-0.5 * (np.arange(-r, r + 1) / s) ** 2)
        k /= k.sum()
        idx = np.clip(np.arange(g)[:, None] + np.arange(-r, r + 1)[None, :], 0, g - 1)  # (g, 2r + 1), edges replicated
        f = np.moveaxis(np.tensordot(k, np.moveaxis(f, axis, 0)[idx], axes=([0], [1])), 0, axis)
    f = f * np.array((ax, ay))
    return np.clip(f, -4096.0, 4096.0)


def _png_elastics(elastic, n):
    """elastic: a sequence of n entries, each None (no field) or an array of shape (grid_h, grid_w, 2), all of one shape ->
    (PngElastic * n) (which keeps the arrays alive), PngElasticDesc"""
    if len(elastic) != n:
        raise ValueError("elastic needs one entry (a (grid_h, grid_w, 2) array, or None) per file")
    es = (PngElastic * n)()
    keep, shape = [], None
    for i, e in enumerate(elastic):
        if e is None:
            continue
        a = np.ascontiguousarray(e, dtype=np.float64)
        if a.ndim != 3 or a.shape[2] != 2 or not (2 <= a.shape[0] <= 33 and 2 <= a.shape[1] <= 33):
            raise ValueError(f"elastic[{i}] must have the shape (grid_h, grid_w, 2) with grid_h and grid_w in 2 .. 33")
        if shape is not None and a.shape != shape:
            raise ValueError(f"elastic[{i}] has the shape {a.shape}, an earlier entry {shape}: one grid size per call")
        shape = a.shape
        keep.append(a)
        es[i].nodes = a.ctypes.data
    es._keep = keep
    gh, gw = shape[:2] if shape is not None else (2, 2)
    return es, PngElasticDesc(gw, gh, (C.c_uint32 * 2)(0, 0))


def _png_fit_warps(datas, boxes, size):
    """what `elastic=` without `warp=` takes as its matrices: per file png_warp_matrix((crop_w, crop_h), size), which puts the
    crop's centre on the output's centre at the crop's own scale; a file whose header cannot be read gets the identity (and its
    decode status)"""
    ws = []
    for i, x in enumerate(datas):
        st, inf = png_info(x)
        b = boxes[i] if boxes is not None else None
        cw, ch = (int(b[2]), int(b[3])) if b is not None and (int(b[2]) or int(b[3])) else (inf["width"], inf["height"])
        ws.append(png_warp_matrix((cw, ch), size) if st == 0 and cw > 0 and ch > 0 else None)
    return ws


def png_warp_desc(filter="bilinear", border="constant", border_value=None, mode="rgb", depth=8, alpha="straight"):
    """the debig_png_warp_desc of png_decode_batch_tensor's warp arguments (no GPU needed).  filter: "bilinear" | "nearest";
    border: "constant" (a tap outside the crop is border_value: per channel on the [0, 1] scale, a number for every channel,
    None: 0, stored as round(x * (2^depth - 1))) or "clamp" (the edge pixels repeat)."""
    if filter not in ("bilinear", "nearest"):
        raise ValueError(f"a warp goes with filter 'bilinear' or 'nearest', not {filter!r}")
    if alpha != "straight":
        raise ValueError(f"a warp goes with alpha='straight' only, not {alpha!r}")
    if border not in PNG_BORDERS:
        raise ValueError(f"border must be one of {sorted(PNG_BORDERS)}, not {border!r}")
    if depth not in (8, 16):
        raise ValueError("a warp needs a concrete depth (8 or 16)")
    ch = {"rgba": 4, "rgb": 3, "gray": 1, "gray_alpha": 2}[mode]
    d = PngWarpDesc(filter=PNG_FILTERS[filter], border_mode=PNG_BORDERS[border])
    if border_value is not None:
        if border != "constant":
            raise ValueError("border_value needs border='constant'")
        bv = [float(x) for x in (border_value if hasattr(border_value, "__len__") else [border_value] * ch)]
        if len(bv) != ch:
            raise ValueError(f"border_value needs {ch} values for mode {mode!r}, not {len(bv)}")
        if not all(0.0 <= x <= 1.0 for x in bv):  # (a NaN fails every comparison)
            raise ValueError(f"border_value values must lie in [0, 1], not {bv!r}")
        for k, x in enumerate(bv):
            d.border[k] = int(round(x * ((1 << depth) - 1)))
    return d


class PngColor(C.Structure):  # include/decode_png.h: debig_png_color
    _fields_ = [("m", C.c_double * 12)]


PNG_LUMA = (6968 / 32768, 23434 / 32768, 2366 / 32768)  # include/decode_png.h: the grey weights of the RGB -> GRAY conversion


def png_color_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, center=0.5, luma=PNG_LUMA):
    """the 3 x 4 colour matrix (numpy float64: row c is (m_c0 m_c1 m_c2 | m_c3), out_c = m_c0 R + m_c1 G + m_c2 B + m_c3 on the
    [0, 1] scale) that png_decode_batch_tensor(..., color=) takes (no GPU needed).  The operations compose in this fixed order:
      1. brightness b: x -> b x;
      2. contrast c about `center`: x -> c x + (1 - c) center (the same fixed centre for every image, not the image's mean);
      3. saturation s: x -> s x + (1 - s) (luma . x) (1, 1, 1); luma: the grey weights (the default: the header's);
      4. hue, in degrees: the rotation about the grey axis (1, 1, 1),
         cos h I + (1 - cos h) / 3 J + sin h / sqrt(3) [[0, -1, 1], [1, 0, -1], [-1, 1, 0]]  (J: all ones).
    The defaults give the identity exactly; saturation=0 gives three rows equal to luma; hue=120 and hue=240 are the cyclic
    channel permutations (exact once quantised).  There is no clamp between the operations: the call clamps once, at the end."""
    import math

    b, c, s_, ce = float(brightness), float(contrast), float(saturation), float(center)
    lw = [float(v) for v in luma]
    if len(lw) != 3:
        raise ValueError("luma needs three weights")
    h = float(hue) % 360.0
    if h % 90.0 == 0.0:  # (cos and sin of a quarter turn are not exact in float64)
        ch_, sh_ = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(h // 90.0)]
    else:
        ch_, sh_ = math.cos(math.radians(h)), math.sin(math.radians(h))
    eye = np.eye(3)
    S = s_ * eye + (1.0 - s_) * np.outer(np.ones(3), np.asarray(lw, np.float64))
    Hm = ch_ * eye + ((1.0 - ch_) / 3.0) * np.ones((3, 3)) + (sh_ / math.sqrt(3.0)) * np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    HS = Hm @ S
    M = np.empty((3, 4), np.float64)
    M[:, :3] = HS * (c * b)
    M[:, 3] = HS @ np.full(3, (1.0 - c) * ce)
    return M + 0.0  # (+ 0.0: no negative zeros)


def _png_colors(color, n):
    """color: one 3 x 4 matrix for the batch, or an (n, 3, 4) array / a sequence of n matrices -> (PngColor * n)"""
    a = np.asarray(color, dtype=np.float64)
    if a.shape == (3, 4):
        a = np.broadcast_to(a, (n, 3, 4))
    if a.shape != (n, 3, 4):
        raise ValueError(f"color must be one 3 x 4 matrix or an ({n}, 3, 4) array, not shape {a.shape}")
    cs = (PngColor * n)()
    for i in range(n):
        cs[i].m[:] = [float(x) for x in a[i].reshape(-1)]
    return cs


class PngTone(C.Structure):  # include/decode_png.h: debig_png_tone
    _fields_ = [("op", C.c_uint32), ("param", C.c_uint32)]


PNG_TONE_OPS = {"none": 0, "autocontrast": 1, "equalize": 2, "posterize": 3, "solarize": 4, "table": 5}  # DEBIG_PNG_TONE_*


def png_tone_table(op, param=0, hist=None):
    """the 256-entry table (numpy uint8) of one colour channel for the tone operation `op` ("autocontrast", "equalize",
    "posterize", "solarize", or its number) with `param` (bits to keep; threshold), from the channel's histogram `hist` (256
    counts below 2^32; ignored by "posterize" and "solarize") -- include/decode_png.h: debig_png_tone_table, the host's own
    statement of what the device builds (no GPU needed).  None on the conditions of status 18 ("tone")."""
    code = PNG_TONE_OPS.get(op, op) if isinstance(op, str) else int(op)
    if isinstance(op, str) and op not in PNG_TONE_OPS:
        raise ValueError(f"op must be one of {sorted(PNG_TONE_OPS)}, not {op!r}")
    if not 0 <= int(param) < 1 << 32 or not 0 <= code < 1 << 32:
        return None
    h = None
    if hist is not None:
        h = np.ascontiguousarray(hist, dtype=np.uint32)
        if h.shape != (256,):
            raise ValueError("hist must hold 256 counts")
    L = _png_spec_lib()
    L.debig_png_tone_table.restype = C.c_int
    L.debig_png_tone_table.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lut = np.zeros(256, np.uint8)
    ok = L.debig_png_tone_table(code, int(param), h.ctypes.data if h is not None else None, lut.ctypes.data)
    return lut if ok else None


def _png_tones(tone, n):
    """tone: a sequence of n entries, each None, "autocontrast", "equalize", ("posterize", bits), ("solarize", threshold) or
    ("table", 256 uint8) -> ((PngTone * n), the distinct tables one behind the other (numpy uint8) or None, their number)"""
    if len(tone) != n:
        raise ValueError(f"tone must have one entry per file ({n}), not {len(tone)}")
    ts = (PngTone * n)()
    tabs, index = [], {}
    for i, e in enumerate(tone):
        if e is None:
            continue
        name, arg = (e, 0) if isinstance(e, str) else (e[0], e[1]) if len(e) == 2 else (None, None)
        if name not in PNG_TONE_OPS or name == "none" or (isinstance(e, str) and name in ("posterize", "solarize", "table")):
            raise ValueError(f"tone[{i}]: None, 'autocontrast', 'equalize', ('posterize', bits), ('solarize', threshold) or "
                             f"('table', 256 uint8), not {e!r}")
        ts[i].op = PNG_TONE_OPS[name]
        if name == "table":
            t = np.asarray(arg)
            if t.shape != (256,) or t.dtype.kind not in "iu" or t.min() < 0 or t.max() > 255:
                raise ValueError(f"tone[{i}]: a table is 256 integers in 0 .. 255")
            key = t.astype(np.uint8).tobytes()
            if key not in index:
                index[key] = len(tabs)
                tabs.append(key)
            ts[i].param = index[key]
        else:
            a = int(arg)
            ts[i].param = a if 0 <= a < 1 << 32 else 0xFFFFFFFF  # (out of range either way: status 18)
    return ts, (np.frombuffer(b"".join(tabs), np.uint8).copy() if tabs else None), len(tabs)


class PngBlur(C.Structure):  # include/decode_png.h: debig_png_blur
    _fields_ = [("op", C.c_uint32), ("ksize", C.c_uint32), ("value", C.c_double)]


PNG_BLUR_OPS = {"none": 0, "gaussian": 1, "sharpness": 2}  # DEBIG_PNG_BLUR_*


def png_blur_weights(ksize, sigma):
    """the ksize Q14 taps (numpy int16; symmetric, not negative, their sum 16384) of the Gaussian blur with `sigma` --
    include/decode_png.h: debig_png_blur_weights, the host's own statement of what the device convolves with (no GPU needed).
    None on the conditions of status 19 ("blur"): ksize even or outside 3 .. 63, sigma not finite, not above 0 or above 1000."""
    k = int(ksize)
    if not 0 <= k < 1 << 32:
        return None
    L = _png_spec_lib()
    L.debig_png_blur_weights.restype = C.c_int
    L.debig_png_blur_weights.argtypes = [C.c_uint32, C.c_double, C.c_void_p]
    q = np.zeros(63, np.int16)
    return q[:k].copy() if L.debig_png_blur_weights(k, float(sigma), q.ctypes.data) else None


def _png_blurs(blur, n):
    """blur: a sequence of n entries, each None, ("gaussian", ksize, sigma) or ("sharpness", factor) -> (PngBlur * n)"""
    if len(blur) != n:
        raise ValueError(f"blur must have one entry per file ({n}), not {len(blur)}")
    bs = (PngBlur * n)()
    for i, e in enumerate(blur):
        if e is None:
            continue
        ok = isinstance(e, (tuple, list)) and len(e) >= 1 and ((e[0] == "gaussian" and len(e) == 3) or (e[0] == "sharpness" and len(e) == 2))
        if not ok:
            raise ValueError(f"blur[{i}]: None, ('gaussian', ksize, sigma) or ('sharpness', factor), not {e!r}")
        bs[i].op = PNG_BLUR_OPS[e[0]]
        if e[0] == "gaussian":
            k = int(e[1])
            bs[i].ksize = k if 0 <= k < 1 << 32 and k == e[1] else 0  # (out of range either way: status 19)
        bs[i].value = float(e[-1])
    return bs


def png_decode_batch_tensor(datas, size, mode="rgb", depth=8, dtype="float32", layout="chw", mean=None, std=None, boxes=None,
                            antialias=True, device="cuda:0", fill=None, force_general=False, alpha="straight",
                            background=None, warp=None, border="constant", border_value=None, color=None, tone=None, perspective=None,
                            elastic=None, blur=None, filter="bilinear"):
    """bytes of N PNG files -> ONE dense tensor on the GPU, cropped, resized to size = (H, W), converted and normalised
    (include/decode_png.h: debig_png_decode_batch_tensor) -> (statuses, tensor, infos).  tensor: (N, C, H, W), or
    (N, H, W, C) with layout="hwc", one allocation; dtype "float32" | "float16" | "bfloat16" (value = sample01 / std -
    mean / std per channel, mean and std on the [0, 1] scale, absent: 1 and 0) or "uint" (uint8 for depth 8, uint16 for 16,
    the latter as torch.int16 bits where torch has no uint16).  boxes: per image None or (x, y, w, h), the crop inside the
    image.  The resize is bilinear with half-pixel centres, antialiased when it shrinks (what
    torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True) means, in Q14 integer weights).
    The slot of a file whose status is not 0 is left as allocated, or holds `fill` when that is given.  Same device rule
    as png_decode_batch_device.
    alpha: "straight" (the default: alpha is dropped or resized like a colour channel, no premultiplication), "over"
    (mode "rgb" / "gray": the file's alpha composites the pixels over `background`, per output channel on the [0, 1]
    scale, default white, inside the resize launch) or "premultiplied" (mode "rgba" / "gray_alpha": premultiplied colour
    and plain alpha, filtered in premultiplied space) -- debig_png_decode_batch_tensor_alpha, see png_alpha_desc.
    filter: "bilinear" (the default: the calls above, unchanged), "bicubic" (the Keys kernel with a = -1/2, clipped to the
    crop and renormalised, antialiased when it shrinks: what Pillow's BICUBIC and interpolate(mode="bicubic",
    antialias=True) mean, in Q14 integer weights with signed sums and clamps to [0, 1] of full scale; a crop more than 32
    times the output on an axis is E_BOX) or "nearest" (the source sample at the output pixel's centre, torch's
    "nearest-exact"; antialias is ignored) -- debig_png_decode_batch_tensor_filter, see png_filter_desc.  Every alpha mode
    goes with every filter.
    warp: None (everything above, unchanged), or one entry per file: None (the identity) or the INVERSE 2 x 3 matrix that
    takes the centre of output pixel (X, Y) to a position inside the crop (png_warp_matrix makes one from flips, an angle, a
    scale, a shear and a translation) -- debig_png_decode_batch_tensor_warp: the resize is replaced by the affine map, in
    integer arithmetic, filter "bilinear" or "nearest", alpha "straight"; `antialias` is not applied under a warp.  border:
    what a tap outside the crop is: "constant" (border_value, per channel on the [0, 1] scale, default 0) or "clamp" (the edge
    pixels).  A matrix with a non-finite or too large entry: status 16 ("warp").  (Pass warp, border and border_value by
    name: `filter` stays the last parameter, as its callers and tests know it; `color` below likewise goes by name.)
    color: None (everything above, unchanged), or one 3 x 4 colour matrix for the batch or an (N, 3, 4) array, one per file
    (png_color_matrix makes one from brightness, contrast, saturation and hue): out_c = m_c0 R + m_c1 G + m_c2 B + m_c3 on the
    [0, 1] scale, applied in integers between the filter and the conversion, clamped once, before mean / std --
    debig_png_decode_batch_tensor_color, or debig_png_decode_batch_tensor_warp_color together with warp.  It goes with mode "rgb"
    or "rgba" (alpha is not mixed), filter "bilinear" or "nearest" and alpha "straight".  A matrix with a non-finite entry or
    one above 16 in magnitude: status 17 ("color").
    tone: None (everything above, unchanged), or one entry per file: None, "autocontrast", "equalize", ("posterize", bits 1 .. 8),
    ("solarize", threshold 0 .. 256) or ("table", 256 uint8) -- debig_png_decode_batch_tensor_tone: the file's image goes
    through everything above to 8-bit samples, then every colour channel (not alpha) through a 256-entry table -- Pillow's
    ImageOps.equalize exactly, autocontrast with cutoff 0 in exact integers, posterize, solarize, or the caller's --, then
    through the conversion with mean / std.  The histograms of "autocontrast" and "equalize" are taken on the device.  A file
    whose entry is None gets, bit for bit, what the call without `tone` gives it.  It goes with depth 8 and alpha "straight" or
    "over"; bits or a threshold out of range: status 18 ("tone").  (By name, like `color`.)
    blur: None (everything above, unchanged), or one entry per file: None, ("gaussian", ksize, sigma) -- ksize odd, 3 .. 63,
    0 < sigma <= 1000: torchvision's GaussianBlur with reflected borders, on every channel, alpha included -- or
    ("sharpness", factor) -- |factor| <= 16: Pillow's ImageEnhance.Sharpness, the blend of the colour channels with their 3 x 3
    SMOOTH; 1 is the identity, 0 is SMOOTH -- debig_png_decode_batch_tensor_blur: the file's image goes through everything above,
    `tone` included, to 8-bit samples, then through the filter in integers (Q14 taps, see png_blur_weights), then ONCE through the
    conversion with mean / std, so float outputs keep the precision below an 8-bit step.  A file whose entry is None gets, bit
    for bit, what the call without `blur` gives it.  It goes with depth 8 and alpha "straight" or "over"; a bad ksize, sigma or
    factor: status 19 ("blur").  (By name, like `tone`.)
    perspective: None (everything above, unchanged), or one entry per file: None (the identity) or the INVERSE 3 x 3 matrix M of a
    projective map: the centre p = (X + 1/2, Y + 1/2, 1) of an output pixel lies at (M0 . p / M2 . p, M1 . p / M2 . p) in the crop
    (png_perspective_matrix makes one from two quadrilaterals, png_perspective_from_warp from a 2 x 3 matrix) --
    debig_png_decode_batch_tensor_persp.  It takes the place of `warp` (both together: ValueError) with its filter, border,
    border_value and alpha rules, goes with color, tone and blur exactly as warp does, and with row (0, 0, 1) gives the bytes of
    warp=.  A matrix whose horizon crosses or nearly touches the output, or with a non-finite or too large entry: status 16
    ("warp").  (By name, like `tone`.  It stands in front of `blur`, which with `filter` stays at the end of the list: `blur`, like
    every argument behind `background`, is to be passed by name -- a positional `blur` would now land here and be refused.)
    elastic (by name, like `perspective`, behind which it stands): None (everything above, unchanged), or one entry per file: None (no field) or an array
    of shape (grid_h, grid_w, 2), the displacement (dx, dy) IN OUTPUT PIXELS at each node of a grid that spans the output from edge
    to edge (png_elastic_field draws one); all entries of a call share one shape, grid_h and grid_w in 2 .. 33 --
    debig_png_decode_batch_tensor_elastic.  The field is interpolated with Catmull-Rom weights in integers and displaces the output
    sampling point BEFORE the matrix of `warp` maps it into the crop: one resampling.  Without `warp` each file takes
    png_warp_matrix((crop_w, crop_h), size), the crop centred on the output at its own scale (to resize, pass warp= with a scale).  filter, border, border_value, alpha, color, tone
    and blur follow the rules of `warp`; an entry of None or of zeros gives the bytes of the call without `elastic`, and the same
    field given to png_decode_batch_labels / _color_labels picks the same source pixels as filter="nearest" here.  With
    `perspective`: ValueError.  A non-finite node or one above 4096 pixels in magnitude: status 16 ("warp")."""
    import torch

    if perspective is not None and warp is not None:
        raise ValueError("perspective and warp exclude each other")
    if elastic is not None:
        if perspective is not None:
            raise ValueError("elastic and perspective exclude each other")
        els, eld = _png_elastics(elastic, len(datas))
        if boxes is not None and len(boxes) != len(datas):
            raise ValueError("boxes needs one entry (or None) per file")
        if warp is None:
            warp = _png_fit_warps(datas, boxes, size)

    if tone is not None:
        if depth != 8:
            raise ValueError("tone needs depth 8")
        if alpha == "premultiplied":
            raise ValueError("tone goes with alpha 'straight' or 'over', not 'premultiplied'")
    if blur is not None:
        if depth != 8:
            raise ValueError("blur needs depth 8")
        if alpha == "premultiplied":
            raise ValueError("blur goes with alpha 'straight' or 'over', not 'premultiplied'")

    if color is not None:
        if filter == "bicubic":
            raise ValueError("color goes with filter 'bilinear' or 'nearest', not 'bicubic'")
        if alpha != "straight":
            raise ValueError(f"color goes with alpha='straight' only, not {alpha!r}")
        if mode not in ("rgb", "rgba"):
            raise ValueError(f"color needs mode 'rgb' or 'rgba', not {mode!r}")
    wd = None
    if warp is not None or perspective is not None:
        wd = png_warp_desc(filter, border, border_value, mode, depth, alpha)
        if background is not None:
            raise ValueError("background needs alpha='over'")
        antialias = False
    elif border != "constant" or border_value is not None:
        raise ValueError("border / border_value need warp")  # (or perspective)
    d, ch, es = png_tensor_desc(size, mode, depth, dtype, layout, mean, std, antialias)
    ad = png_alpha_desc(alpha, background, mode, depth)
    fd = png_filter_desc(filter)
    ws = _png_warps(warp, len(datas)) if warp is not None else None
    cs = _png_colors(color, len(datas)) if color is not None else None
    L = _png_spec_lib()
    L.debig_png_decode_batch_tensor.restype = C.c_int
    L.debig_png_decode_batch_tensor.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    L.debig_png_decode_batch_tensor_alpha.restype = C.c_int
    L.debig_png_decode_batch_tensor_alpha.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    dev = _png_device(L, device)
    n = len(datas)
    args = _png_batch_args(datas, boxes)
    H, W = d.out_h, d.out_w
    tdt = {1: torch.float32, 2: torch.float16, 3: torch.bfloat16}.get(d.dtype)
    if tdt is None:
        tdt = torch.uint8 if es == 1 else getattr(torch, "uint16", torch.int16)
    shape = (n, ch, H, W) if d.out_layout else (n, H, W, ch)
    out = _png_dense_out(shape, tdt, fill, dev)
    in_ptrs, in_sizes, bx, status, infos = args
    if elastic is not None:
        bs = _png_blurs(blur, n) if blur is not None else None
        ts, tabs, n_tabs = _png_tones(tone, n) if tone is not None else (None, None, 0)
        L.debig_png_decode_batch_tensor_elastic.restype = C.c_int
        L.debig_png_decode_batch_tensor_elastic.argtypes = [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + \
            [C.c_void_p] * 4
        rc = L.debig_png_decode_batch_tensor_elastic(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, cs, ts,
                                                     tabs.ctypes.data if tabs is not None else None, n_tabs, bs, status, infos, n,
                                                     PNG_FORCE_GENERAL if force_general else 0, C.byref(d), C.byref(wd), els,
                                                     C.byref(eld))
    elif perspective is not None:
        ps = _png_persps(perspective, n)
        bs = _png_blurs(blur, n) if blur is not None else None
        ts, tabs, n_tabs = _png_tones(tone, n) if tone is not None else (None, None, 0)
        L.debig_png_decode_batch_tensor_persp.restype = C.c_int
        L.debig_png_decode_batch_tensor_persp.argtypes = [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + \
            [C.c_void_p] * 2
        rc = L.debig_png_decode_batch_tensor_persp(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ps, cs, ts,
                                                   tabs.ctypes.data if tabs is not None else None, n_tabs, bs, status, infos, n,
                                                   PNG_FORCE_GENERAL if force_general else 0, C.byref(d), C.byref(wd))
    elif blur is not None:
        bs = _png_blurs(blur, n)
        ts, tabs, n_tabs = _png_tones(tone, n) if tone is not None else (None, None, 0)
        L.debig_png_decode_batch_tensor_blur.restype = C.c_int
        L.debig_png_decode_batch_tensor_blur.argtypes = [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + \
            [C.c_void_p] * 4
        plain = wd is None and cs is None
        rc = L.debig_png_decode_batch_tensor_blur(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, cs, ts,
                                                  tabs.ctypes.data if tabs is not None else None, n_tabs, bs, status, infos, n,
                                                  PNG_FORCE_GENERAL if force_general else 0, C.byref(d),
                                                  C.byref(ad) if plain and ad is not None else None,
                                                  C.byref(fd) if wd is None and fd is not None else None,
                                                  C.byref(wd) if wd is not None else None)
    elif tone is not None:
        ts, tabs, n_tabs = _png_tones(tone, n)
        L.debig_png_decode_batch_tensor_tone.restype = C.c_int
        L.debig_png_decode_batch_tensor_tone.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + \
            [C.c_void_p] * 4
        plain = wd is None and cs is None
        rc = L.debig_png_decode_batch_tensor_tone(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, cs, ts,
                                                  tabs.ctypes.data if tabs is not None else None, n_tabs, status, infos, n,
                                                  PNG_FORCE_GENERAL if force_general else 0, C.byref(d),
                                                  C.byref(ad) if plain and ad is not None else None,
                                                  C.byref(fd) if wd is None and fd is not None else None,
                                                  C.byref(wd) if wd is not None else None)
    elif cs is not None and wd is not None:
        L.debig_png_decode_batch_tensor_warp_color.restype = C.c_int
        L.debig_png_decode_batch_tensor_warp_color.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_tensor_warp_color(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, cs, status, infos, n,
                                                        PNG_FORCE_GENERAL if force_general else 0, C.byref(d), C.byref(wd))
    elif cs is not None:
        L.debig_png_decode_batch_tensor_color.restype = C.c_int
        L.debig_png_decode_batch_tensor_color.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_tensor_color(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, cs, status, infos, n,
                                                   PNG_FORCE_GENERAL if force_general else 0, C.byref(d),
                                                   C.byref(fd) if fd is not None else None)
    elif wd is not None:
        L.debig_png_decode_batch_tensor_warp.restype = C.c_int
        L.debig_png_decode_batch_tensor_warp.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_tensor_warp(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, status, infos, n,
                                                  PNG_FORCE_GENERAL if force_general else 0, C.byref(d), C.byref(wd))
    elif fd is not None:
        L.debig_png_decode_batch_tensor_filter.restype = C.c_int
        L.debig_png_decode_batch_tensor_filter.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_tensor_filter(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, status, infos, n,
                                                    PNG_FORCE_GENERAL if force_general else 0, C.byref(d),
                                                    C.byref(ad) if ad is not None else None, C.byref(fd))
    elif ad is None:
        rc = L.debig_png_decode_batch_tensor(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, status, infos, n,
                                             PNG_FORCE_GENERAL if force_general else 0, C.byref(d))
    else:
        rc = L.debig_png_decode_batch_tensor_alpha(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, status, infos, n,
                                                   PNG_FORCE_GENERAL if force_general else 0, C.byref(d), C.byref(ad))
    if rc in (PNG_BAD_FORMAT, PNG_BAD_ARG):
        raise ValueError(f"debig_png_decode_batch_tensor rejected its arguments ({rc})")
    N.check(rc, "debig_png_decode_batch_tensor")
    return [int(s) for s in status], out, [_info_dict(i) for i in infos]


PNG_LABEL_STATS_MAX_IDS = 1024  # include/decode_png.h: DEBIG_PNG_LABEL_STATS_MAX_IDS


def _png_stats_ids(num_ids):
    """the num_ids of png_label_stats and of the decode calls' stats= (None: no statistics) -> the int, or ValueError"""
    if num_ids is None:
        return None
    if isinstance(num_ids, bool) or not isinstance(num_ids, (int, np.integer)) or not 1 <= int(num_ids) <= PNG_LABEL_STATS_MAX_IDS:
        raise ValueError(f"num_ids must be an integer in 1 .. {PNG_LABEL_STATS_MAX_IDS}, not {num_ids!r}")
    return int(num_ids)


def _png_label_code(labels):
    """the labels of the calls that post-process a dense label tensor -> the DEBIG_PNG_L_* code of their dtype, or ValueError"""
    import torch

    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise ValueError("labels must be a (N, H, W) tensor")
    codes = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3}
    if hasattr(torch, "uint16"):
        codes[torch.uint16] = 1
    if labels.dtype not in codes:
        raise ValueError(f"labels must be uint8, uint16 (or int16), int32 or int64, not {labels.dtype}")
    return codes[labels.dtype]


def _png_label_input(labels, status):
    """what follows _png_label_code (a check of the call's own that needs the code stands between the two) -> (n, H, W, the
    status as a ctypes array or None), or ValueError"""
    if not labels.is_contiguous():
        raise ValueError("labels must be contiguous")
    if labels.device.type != "cuda":
        raise ValueError("labels must be on the GPU")
    n, H, W = (int(v) for v in labels.shape)
    if n and not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"labels must be (N, H, W) with 1 <= H, W <= 16384, not {tuple(labels.shape)}")
    if status is not None and len(status) != n:
        raise ValueError("status needs one entry per image")
    return n, H, W, None if status is None else (C.c_uint32 * n)(*[int(v) for v in status])


def _png_label_skipped(out, st, src=None):
    """the images the library leaves alone (a status entry that is not 0), and only they: zeros, or the image of src"""
    for i in ([] if st is None else [i for i in range(len(st)) if st[i] != 0]):
        if src is None:
            out[i].zero_()
        else:
            out[i].copy_(src[i])


def _png_label_call(name, argtypes, labels, *args):
    """one C call on a label tensor, which is its first argument -> None; ValueError where the library rejects its arguments"""
    import torch

    L = _png_spec_lib()
    _png_device(L, labels.device)
    fn = getattr(L, name)
    fn.restype = C.c_int
    fn.argtypes = argtypes
    torch.cuda.synchronize(labels.device)  # whoever wrote the tensor runs on torch's stream, the library on its own
    rc = fn(labels.data_ptr(), *args)
    if rc == PNG_BAD_ARG:
        raise ValueError(f"{name} rejected its arguments ({rc})")
    N.check(rc, name)


def png_label_stats(labels, num_ids, status=None):
    """per-id pixel counts and bounding boxes of a dense (N, H, W) label tensor on the GPU (include/decode_png.h:
    debig_png_label_stats, which has the rule) -> a numpy int64 array (N, num_ids + 1, 5) of (count, x0, y0, x1, y1): record
    k < num_ids for the elements equal to k, record num_ids ("other") for every element that is negative or >= num_ids (a border
    label of -1, an ignore value of 255, a packed colour); the box is [x0, x1) x [y0, y1) in output pixels, an id that does not
    occur has five zeros.  labels: a contiguous tensor of torch.uint8, uint16 (or int16, read as the uint16 bits, which is how
    the label calls hand out uint16), int32 or int64 on the current device -- the tensor of png_decode_batch_labels /
    png_decode_batch_color_labels under any of their maps, or one made otherwise.  num_ids: 1 .. 1024.  status: None, or one
    entry per image: the records of an image whose entry is not 0 stay zero.  One kernel launch reads the tensor once; the call
    waits for the work queued on the device before it, and for its own."""
    num_ids = _png_stats_ids(num_ids)
    if num_ids is None:
        raise ValueError("num_ids must be an integer")
    code = _png_label_code(labels)
    n, H, W, st = _png_label_input(labels, status)
    out = np.zeros((n, num_ids + 1, 5), np.uint32)
    if n == 0:
        return out.astype(np.int64)
    _png_label_call("debig_png_label_stats", [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p],
                    labels, n, W, H, code, num_ids, st, out.ctypes.data)
    return out.astype(np.int64)


PNG_LABEL_BOUNDARY_MAX_RADIUS = 16  # include/decode_png.h: DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS
_PNG_BOUNDARY_SHAPES = {"square": 0, "diamond": 1, "disk": 2}  # DEBIG_PNG_BOUNDARY_*
_PNG_BOUNDARY_MODES = {"ring": 0, "edge": 1}


def _png_boundary_shape(radius, shape):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= PNG_LABEL_BOUNDARY_MAX_RADIUS:
        raise ValueError(f"radius must be an integer in 1 .. {PNG_LABEL_BOUNDARY_MAX_RADIUS}, not {radius!r}")
    if not isinstance(shape, str) or shape not in _PNG_BOUNDARY_SHAPES:
        raise ValueError(f"shape must be one of {sorted(_PNG_BOUNDARY_SHAPES)}, not {shape!r}")
    return int(radius), _PNG_BOUNDARY_SHAPES[shape]


def png_label_boundary_reach(radius, shape="square"):
    """the reach table of a boundary shape (include/decode_png.h: debig_png_label_boundary_reach) -> [reach[0], ..., reach[radius]]:
    the half-width of the window at a row distance of d.  "square": radius (Chebyshev ball), "diamond": radius - d (L1 ball),
    "disk": isqrt(radius^2 - d^2) (Euclidean ball)."""
    radius, code = _png_boundary_shape(radius, shape)
    L = _png_spec_lib()
    L.debig_png_label_boundary_reach.restype = None
    L.debig_png_label_boundary_reach.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    table = (C.c_uint8 * 17)()
    L.debig_png_label_boundary_reach(radius, code, table)
    return [int(v) for v in table[: radius + 1]]


def png_label_boundary(labels, radius=1, shape="square", mode="ring", value=255, status=None):
    """boundary bands of a dense (N, H, W) label tensor on the GPU (include/decode_png.h: debig_png_label_boundary, which has the
    rule) -> a NEW device tensor: Pascal-VOC-style void rings, trimaps, edge targets.  An element is a boundary element iff an
    element of the image at (x + dx, y + dy) with |dy| <= radius and |dx| <= reach[|dy|] (png_label_boundary_reach) differs from
    it: both sides of an edge are marked, the window is clipped at the image, elements are compared whole (exact for packed
    colours and int64 ids).  mode="ring": boundary ? value : the element, in the dtype of the input (value must fit it; it may equal
    an id); mode="edge": a uint8 tensor of 1 / 0.  labels: a contiguous tensor of torch.uint8, uint16 (or int16, read as the uint16
    bits, value in 0 .. 65535, returned as int16), int32 or int64 on the current device -- the tensor of png_decode_batch_labels /
    png_decode_batch_color_labels under any of their maps, or one made otherwise.  A ring cannot be carried through a warp, so the
    documented use is labels -> png_label_boundary -> png_label_stats: decode (and warp) first, make the ring from the tensor that
    came back, then take the statistics, where a ring value of 255 counts as "other".  radius: 1 .. 16; shape: "square", "diamond"
    or "disk".  status: None, or one entry per image: an image whose entry is not 0 is not looked at and comes back as its input
    under "ring", as zeros under "edge".  One kernel launch reads the tensor once and writes the result once; the call waits for
    the work queued on the device before it, and for its own."""
    import torch

    radius, shape_code = _png_boundary_shape(radius, shape)
    if not isinstance(mode, str) or mode not in _PNG_BOUNDARY_MODES:
        raise ValueError(f"mode must be one of {sorted(_PNG_BOUNDARY_MODES)}, not {mode!r}")
    code = _png_label_code(labels)
    if mode == "ring":
        lo, hi = [(0, 255), (0, 65535), (-2 ** 31, 2 ** 31 - 1), (-2 ** 63, 2 ** 63 - 1)][code]
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
            raise ValueError(f"value must be an integer in {lo} .. {hi} for {labels.dtype}, not {value!r}")
    n, H, W, st = _png_label_input(labels, status)
    out = torch.empty((n, H, W), dtype=torch.uint8 if mode == "edge" else labels.dtype, device=labels.device)
    if n == 0:
        return out
    _png_label_skipped(out, st, None if mode == "edge" else labels)
    _png_label_call("debig_png_label_boundary", [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_int64, C.c_void_p],
                    labels, out.data_ptr(), n, W, H, code, radius, shape_code, _PNG_BOUNDARY_MODES[mode],
                    int(value) if mode == "ring" else 0, st)
    return out


PNG_LABEL_DISTANCE_MAX_CAP = 32767  # include/decode_png.h: DEBIG_PNG_LABEL_DISTANCE_MAX_CAP
_PNG_DISTANCE_FORMATS = {"squared": 0, "root": 1}  # DEBIG_PNG_DISTANCE_SQUARED / _ROOT


def png_label_distance(labels, to=None, cap=None, out="squared", status=None):
    """exact Euclidean distance maps of a dense (N, H, W) label tensor on the GPU (include/decode_png.h: debig_png_label_distance,
    which has the rule) -> a NEW device tensor: what scipy.ndimage.distance_transform_edt gives image by image on the host -- U-Net
    border weights, signed distance maps for boundary losses, truncated distance targets, centre-ness, trimaps wider than 16.
    D2(x, y) is the smallest (x - x')^2 + (y - y')^2 over the SITES of the element, an exact integer.  to=None: the sites are the
    elements of the image that differ from it (on a binary mask both halves of a signed distance map at once, on a multi-class map
    the inside distance of every class); to=<int>: the elements equal to it (distance_transform_edt(labels != to); those elements
    get 0; a value the dtype cannot hold matches nothing).  Elements are compared whole (exact for packed colours and int64 ids);
    positions outside the image are never sites.  cap: None, or 1 .. 32767: the result is min(D2, cap^2).  out="squared": torch.int32,
    D2 itself; an element without any site (a flat image, an absent value) gets cap^2, or 2^31 - 1 without a cap.  out="root":
    torch.float32, the float32 nearest to the square root (exactly np.sqrt(d2.astype(float64)).astype(float32)); without a site cap,
    or +inf without a cap.  labels: a contiguous tensor of torch.uint8, uint16 (or int16, read as the uint16 bits: to is then
    0 .. 65535), int32 or int64 on the current device -- the tensor of png_decode_batch_labels / png_decode_batch_color_labels under
    any of their maps, or one made otherwise.  A distance map cannot be carried through a warp, so the documented use is labels ->
    png_label_distance: decode (and warp) first, then measure the tensor that came back.  png_label_distance(t) <= r * r is
    png_label_boundary(t, r, "disk", "edge") for r = 1 .. 16.  status: None, or one entry per image: an image whose entry is not 0
    is not looked at and comes back as zeros.  Two kernel launches, each linear in the image whatever it holds; the call waits for
    the work queued on the device before it, and for its own."""
    import torch

    if to is not None and (isinstance(to, bool) or not isinstance(to, (int, np.integer)) or not -2 ** 63 <= int(to) < 2 ** 63):
        raise ValueError(f"to must be None or an integer that fits 64 bits, not {to!r}")
    if cap is not None and (isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= int(cap) <= PNG_LABEL_DISTANCE_MAX_CAP):
        raise ValueError(f"cap must be None or an integer in 1 .. {PNG_LABEL_DISTANCE_MAX_CAP}, not {cap!r}")
    if not isinstance(out, str) or out not in _PNG_DISTANCE_FORMATS:
        raise ValueError(f"out must be one of {sorted(_PNG_DISTANCE_FORMATS)}, not {out!r}")
    code = _png_label_code(labels)
    n, H, W, st = _png_label_input(labels, status)
    res = torch.empty((n, H, W), dtype=torch.int32 if out == "squared" else torch.float32, device=labels.device)
    if n == 0:
        return res
    _png_label_skipped(res, st)
    _png_label_call("debig_png_label_distance",
                    [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p],
                    labels, res.data_ptr(), n, W, H, code, 0 if to is None else 1, 0 if to is None else int(to),
                    0 if cap is None else int(cap), _PNG_DISTANCE_FORMATS[out], st)
    return res


_PNG_COMPONENTS_IDS = {"first": 0, "consecutive": 1}  # DEBIG_PNG_COMPONENTS_FIRST / _CONSECUTIVE


def png_label_components(labels, connectivity=4, background=None, ids="consecutive", status=None):
    """connected components of a dense (N, H, W) label tensor on the GPU (include/decode_png.h: debig_png_label_components, which
    has the rule) -> (a NEW torch.int32 device tensor (N, H, W), a numpy int64 array (N,) of K, the components of every image):
    what skimage.measure.label(x, background=..., connectivity=1|2) gives image by image on the host, and scipy.ndimage.label on a
    binary mask -- instance ids from a class map, split "stuff" regions, specks to drop, a border weight per cell, per-instance boxes.
    Two elements are neighbours iff they are adjacent (connectivity=4: by an edge; 8: by an edge or a corner) AND hold the same
    value; a component is a class of the transitive closure.  Elements are compared whole (exact for packed colours and int64
    ids).  background=None: every element belongs to a component; background=<int>: the elements equal to it belong to none (a
    value the dtype cannot hold matches nothing).  ids="consecutive": the components are numbered 1 .. K in the raster order of
    their first elements, scipy.ndimage.label's numbering, background 0; ids="first": every element gets y * W + x of its
    component's first element in raster order, background -1 -- canonical, and one launch less.  labels: a contiguous tensor of
    torch.uint8, uint16 (or int16, read as the uint16 bits: background is then 0 .. 65535), int32 or int64 on the current device --
    the tensor of png_decode_batch_labels / png_decode_batch_color_labels under any of their maps, or one made otherwise.  A warp
    tears objects apart and a crop cuts them, so the documented use is labels -> png_label_components -> png_label_stats(ids, K + 1):
    decode (and warp) first, label the tensor that came back, and png_label_stats(ids, int(K.max()) + 1) then has every instance's
    pixel count and tight box in record k = 1 .. K, with nothing in "other".  status: None, or one entry per image: an image whose
    entry is not 0 is not looked at and comes back as zeros with K = 0.  Union-find in three (first) or five launches; its work
    depends on the data (include/decode_png.h).  The call waits for the work queued on the device before it, and for its own."""
    import torch

    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be 4 or 8, not {connectivity!r}")
    if background is not None and (isinstance(background, bool) or not isinstance(background, (int, np.integer)) or
                                   not -2 ** 63 <= int(background) < 2 ** 63):
        raise ValueError(f"background must be None or an integer that fits 64 bits, not {background!r}")
    if not isinstance(ids, str) or ids not in _PNG_COMPONENTS_IDS:
        raise ValueError(f"ids must be one of {sorted(_PNG_COMPONENTS_IDS)}, not {ids!r}")
    code = _png_label_code(labels)
    n, H, W, st = _png_label_input(labels, status)
    res = torch.empty((n, H, W), dtype=torch.int32, device=labels.device)
    if n == 0:
        return res, np.zeros(0, np.int64)
    _png_label_skipped(res, st)
    counts = (C.c_uint32 * n)()
    _png_label_call("debig_png_label_components",
                    [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p],
                    labels, res.data_ptr(), n, W, H, code, int(connectivity), 0 if background is None else 1,
                    0 if background is None else int(background), _PNG_COMPONENTS_IDS[ids], st, counts)
    return res, np.array(list(counts), np.int64)


class PngEncodeDesc(C.Structure):  # include/decode_png.h: debig_png_encode_desc
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("dtype", C.c_uint32), ("depth", C.c_uint32),
                ("layout", C.c_uint32), ("palette_entries", C.c_uint32), ("trns_entries", C.c_uint32), ("palette_off", C.c_uint64),
                ("trns_off", C.c_uint64)]


PNG_ENCODE_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}  # DEBIG_PNG_FILTER_NONE .. _ADAPTIVE
PNG_ENCODE_STATUS = {0: "ok", 12: "output", 20: "encode", 21: "range"}  # what png_encode_batch hands out (names: PNG_STATUS)


def _png_encode_side(what, given, n, width):
    """palette= / trns= of png_encode_batch -> one uint8 array or None per image.  A list or tuple has one entry per image; anything
    else is one array for the batch: (entries, 3) for a palette (width 3), (entries,) for tRNS (width 0)"""
    def one(v):
        if v is None:
            return None
        a = np.asarray(v.cpu() if hasattr(v, "cpu") else (np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else v))
        ok = a.dtype == np.uint8 and ((a.ndim == 2 and a.shape[1] == 3) if width else a.ndim == 1) and 1 <= a.shape[0] <= 256
        if not ok:
            raise ValueError(f"{what} must be uint8 of shape " + ("(entries, 3)" if width else "(entries,)") + " with 1 .. 256 entries")
        return np.ascontiguousarray(a)
    if isinstance(given, (list, tuple)):
        if len(given) != n:
            raise ValueError(f"a list of {what}s needs one entry per image")
        return [one(v) for v in given]
    return [one(given)] * n


def png_encode_batch(images, layout="hwc", depth=None, palette=None, trns=None, filter="adaptive", level=1):
    """tensors on the GPU -> PNG files (include/decode_png.h: debig_png_encode_batch, which has the file's rules)
    -> [(status, bytes or None)], one per image; status 0, or 12 "output", 20 "encode" (the descriptor breaks a rule: more than 4
    channels, a depth that does not fit the dtype, more than one channel with int32 / int64, a palette with channels != 1 or
    depth != 8, more tRNS than palette entries), 21 "range" (an int32 / int64 element outside 0 .. 2^depth - 1, or an element
    that is not below the palette's entries).  images: ONE tensor (N, H, W), (N, H, W, C) under layout="hwc" or (N, C, H, W) under
    "chw", or a LIST of tensors of different shapes (H, W), (H, W, C) or (C, H, W); torch.uint8, uint16 (or int16, read as the
    uint16 bits, which is how the label calls hand out uint16), int32 or int64, on the current device; a tensor that is not
    contiguous is made so.  1 / 2 / 3 / 4 channels give grey, grey + alpha, RGB, RGBA; depth: None -- 8 for uint8, 16 for uint16,
    for int32 / int64 8 with a palette and 16 without --, 8 or 16.  palette: (entries, 3) uint8, one for the batch or a list with
    one (or None) per image: colour type 3, one channel at depth 8; trns: the palette's alpha bytes, likewise.  filter: "none",
    "sub", "up", "average", "paeth" for every row, or "adaptive" (per row the minimum sum of absolute differences); level 0
    (stored) or 1 (LZ77 + fixed Huffman, never longer than level 0).  The bytes are a pure function of the arguments.  Filtering,
    DEFLATE, Adler-32 and CRC-32 run on the device; each file comes down once.  The call waits for the work queued on the device
    before it, and for its own.  Not provided: 1 / 2 / 4-bit depths, Adam7, other ancillary chunks, APNG, host tensors.  Level 2
    (dynamic Huffman blocks) is png_encode_batch_dyn."""
    return _png_encode(images, layout, depth, palette, trns, filter, level, (0, 1), "debig_png_encode_batch")


def png_encode_batch_dyn(images, layout="hwc", depth=None, palette=None, trns=None, filter="adaptive", level=2):
    """png_encode_batch with level 0, 1 or 2 (include/decode_png.h: debig_png_encode_batch_dyn): the same arguments, rules, statuses
    and errors.  Levels 0 and 1 give png_encode_batch's bytes.  Level 2 keeps level 1's chunks and matches and writes every chunk
    as one dynamic Huffman block where that is smaller than the fixed-code block and than the chunk stored, so a level-2 file is
    never longer than the level-1 file; its zlib header is 78 5E.  The bytes are a pure function of the arguments."""
    return _png_encode(images, layout, depth, palette, trns, filter, level, (0, 1, 2), "debig_png_encode_batch_dyn")


def png_encode_batch_lz(images, layout="hwc", depth=None, palette=None, trns=None, filter="adaptive", level=3):
    """png_encode_batch with level 0, 1, 2 or 3 (include/decode_png.h: debig_png_encode_batch_lz): the same arguments, rules, statuses
    and errors.  Levels 0 .. 2 give png_encode_batch_dyn's bytes.  Level 3 keeps level 2's chunks and blocks and matches otherwise:
    it also tries the byte above and its two neighbours, and a short match gives way to a longer one that starts one byte later.
    That is made for label maps, instance ids and other flat tensors, above all under filter="none"; on photographs it changes
    next to nothing, and a level-3 file is NOT guaranteed to be at most the level-2 file.  Its zlib header is 78 9C.  The bytes are
    a pure function of the arguments."""
    return _png_encode(images, layout, depth, palette, trns, filter, level, (0, 1, 2, 3), "debig_png_encode_batch_lz")


def _png_encode(images, layout, depth, palette, trns, filter, level, levels, call):
    """the body of png_encode_batch, png_encode_batch_dyn and png_encode_batch_lz: `levels` are the call's, `call` is its C entry point"""
    import torch

    if not isinstance(filter, str) or filter not in PNG_ENCODE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(PNG_ENCODE_FILTERS)}, not {filter!r}")
    if isinstance(level, bool) or level not in levels:
        raise ValueError(f"level must be {', '.join(str(v) for v in levels[:-1])} or {levels[-1]}, not {level!r}")
    lay = png_layout_code(layout)
    if depth is not None and (isinstance(depth, bool) or depth not in (8, 16)):
        raise ValueError(f"depth must be None, 8 or 16, not {depth!r}")
    one = isinstance(images, torch.Tensor)
    if one:
        if images.dim() not in (3, 4):
            raise ValueError("one tensor must be (N, H, W), (N, H, W, C) or (N, C, H, W)")
        items = [images[i] for i in range(images.shape[0])]
    elif isinstance(images, (list, tuple)):
        items = list(images)
    else:
        raise ValueError("images must be a tensor or a list of tensors")
    n = len(items)
    pals, trn = _png_encode_side("palette", palette, n, 3), _png_encode_side("trns", trns, n, 0)
    codes = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3}
    if hasattr(torch, "uint16"):
        codes[torch.uint16] = 1
    for t in items:
        if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3):
            raise ValueError("an image must be a tensor (H, W), (H, W, C) or (C, H, W)")
        if t.dtype not in codes:
            raise ValueError(f"images must be uint8, uint16 (or int16), int32 or int64, not {t.dtype}")
        if t.device.type != "cuda":
            raise ValueError("images must be on the GPU")
    if n == 0:
        return []
    L = _png_spec_lib()
    _png_device(L, items[0].device)
    items = [t if t.is_contiguous() else t.contiguous() for t in items]
    descs = (PngEncodeDesc * n)()
    side = bytearray()
    for i, t in enumerate(items):
        d = descs[i]
        if t.dim() == 2:
            (H, W), Cn = t.shape, 1
        elif lay == 0:
            H, W, Cn = t.shape
        else:
            Cn, H, W = t.shape
        d.width, d.height, d.channels, d.dtype, d.layout = int(W), int(H), int(Cn), codes[t.dtype], lay
        d.depth = depth if depth is not None else 8 if d.dtype == 0 else 16 if d.dtype == 1 or pals[i] is None else 8
        if pals[i] is not None:
            d.palette_entries, d.palette_off = pals[i].shape[0], len(side)
            side += pals[i].tobytes()
        if trn[i] is not None:
            d.trns_entries, d.trns_off = trn[i].shape[0], len(side)
            side += trn[i].tobytes()
    L.debig_png_encode_bound.restype = C.c_uint64
    L.debig_png_encode_bound.argtypes = [C.POINTER(PngEncodeDesc)]
    fn = getattr(L, call)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 3
    caps = [int(L.debig_png_encode_bound(C.byref(descs[i]))) for i in range(n)]
    outs = [np.empty(max(c, 1), np.uint8) for c in caps]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in items])
    out_ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    out_caps = (C.c_uint64 * n)(*caps)
    sizes, status = (C.c_uint64 * n)(), (C.c_uint32 * n)()
    side_buf = (C.c_uint8 * max(len(side), 1)).from_buffer_copy(bytes(side) or b"\0")
    torch.cuda.synchronize(items[0].device)  # whoever wrote the tensors runs on torch's stream, the library on its own
    rc = fn(ptrs, descs, side_buf, out_ptrs, out_caps, sizes, status, n, PNG_ENCODE_FILTERS[filter], int(level))
    if rc == PNG_BAD_ARG:
        raise ValueError(f"{call} rejected its arguments ({rc})")
    N.check(rc, call)
    return [(int(status[i]), outs[i][: sizes[i]].tobytes() if status[i] == 0 else None) for i in range(n)]


class PngLabelDesc(C.Structure):  # include/decode_png.h: debig_png_label_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("dtype", C.c_uint32), ("reserved", C.c_uint32),
                ("lut", C.POINTER(C.c_int32))]


PNG_LABEL_DTYPES = {"uint8": 0, "uint16": 1, "int32": 2, "int64": 3}  # include/decode_png.h: DEBIG_PNG_L_*


def png_label_desc(size, dtype="int64", lut=None):
    """the debig_png_label_desc of png_decode_batch_labels' arguments (no GPU needed) -> (desc, element bytes).  The desc
    keeps the 256 int32 of `lut` alive (desc._lut)."""
    if dtype not in PNG_LABEL_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(PNG_LABEL_DTYPES)}, not {dtype!r}")
    H, W = (int(v) for v in size)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"size must be (H, W) with 1 <= H, W <= 16384, not {size!r}")
    d = PngLabelDesc(out_w=W, out_h=H, dtype=PNG_LABEL_DTYPES[dtype])
    if lut is not None:
        table = np.asarray(lut)
        if table.shape != (256,) or table.dtype.kind not in "iu":
            raise ValueError("lut needs 256 integers")
        top = {"uint8": 255, "uint16": 65535}.get(dtype, 2 ** 31 - 1)
        low = 0 if dtype in ("uint8", "uint16") else -2 ** 31
        if int(table.min()) < low or int(table.max()) > top:
            raise ValueError(f"lut entries must lie in [{low}, {top}] for dtype {dtype!r}")
        d._lut = np.ascontiguousarray(table, dtype=np.int32)
        d.lut = d._lut.ctypes.data_as(C.POINTER(C.c_int32))
    return d, 1 << PNG_LABEL_DTYPES[dtype]


def png_label_warp_desc(border="constant", border_label=None, dtype="int64"):
    """the debig_png_label_warp_desc of png_decode_batch_labels' warp arguments (no GPU needed).  border_label: the element of
    a pick outside the crop under border="constant" (the ignore index; None: 0); it must fit dtype."""
    if border not in PNG_BORDERS:
        raise ValueError(f"border must be one of {sorted(PNG_BORDERS)}, not {border!r}")
    if dtype not in PNG_LABEL_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(PNG_LABEL_DTYPES)}, not {dtype!r}")
    if border_label is not None and border != "constant":
        raise ValueError("border_label needs border='constant'")
    v = 0 if border_label is None else int(border_label)
    top = {"uint8": 255, "uint16": 65535}.get(dtype, 2 ** 31 - 1)
    low = 0 if dtype in ("uint8", "uint16") else -2 ** 31
    if not low <= v <= top:
        raise ValueError(f"border_label must lie in [{low}, {top}] for dtype {dtype!r}, not {v}")
    return PngLabelWarpDesc(border_mode=PNG_BORDERS[border], border_label=v)


def png_decode_batch_labels(datas, size, dtype="int64", boxes=None, lut=None, fill=None, device="cuda:0", warp=None,
                            border="constant", border_label=None, perspective=None, elastic=None, stats=None):
    """bytes of N label PNGs -> ONE dense (N, H, W) integer tensor on the GPU (include/decode_png.h:
    debig_png_decode_batch_labels) -> (statuses, tensor, infos).  The label of a pixel is its palette index (colour type 3)
    or its raw grey sample (colour type 0, 1 to 16 bits): nothing is scaled, PLTE colours and tRNS are ignored.  size =
    (H, W); boxes: per image None or (x, y, w, h), the crop inside the image; the pick is the source pixel under the output
    pixel's centre -- the grid of png_decode_batch_tensor(filter="nearest") with the same box.  lut: 256 integers, the
    element is lut[label] (an id -> train-id remap; 16-bit files take none).  dtype: "uint8" | "uint16" | "int32" | "int64";
    uint16 comes as torch.int16 bits where torch has no uint16.  Colour types 2, 4 and 6, a 16-bit file with dtype "uint8" or
    with a lut: status 15 ("label").  The slot of a file whose status is not 0 is left as allocated, or holds `fill` when that
    is given.  Same device rule as png_decode_batch_device.
    warp: None (everything above, unchanged), or one entry per file: None (the identity) or the INVERSE 2 x 3 matrix of
    png_decode_batch_tensor(warp=) -- debig_png_decode_batch_labels_warp: the pick is the one of that call's filter="nearest"
    under the same matrix, so an image and its mask stay aligned.  border: "constant" (a pick outside the crop stores
    border_label as it is, not through the lut: the ignore index; default 0) or "clamp".  A matrix with a non-finite or too
    large entry: status 16 ("warp").
    perspective (by name; the last parameter, so every older positional call means what it meant): in place of warp (both
    together: ValueError), one entry per file: None (the identity) or the INVERSE 3 x 3 matrix of
    png_decode_batch_tensor(perspective=) -- debig_png_decode_batch_labels_persp: the pick is again that call's
    filter="nearest" under the same matrix; border and border_label as for warp.  A horizon across the output: status 16.
    elastic (by name; the last parameter): None, or one entry per file: None or a (grid_h, grid_w, 2) displacement field, as
    png_decode_batch_tensor(elastic=) takes it -- debig_png_decode_batch_labels_elastic: the pick is that call's filter="nearest"
    under the same matrix and field.  It goes with warp; without warp each file takes png_warp_matrix((crop_w, crop_h), size).  With
    perspective: ValueError.  A bad node: status 16.
    stats (by name; the last parameter): None (everything above, the return value included), or num_ids: the call runs
    png_label_stats(tensor, num_ids, statuses) on the tensor it has just written and returns (statuses, tensor, infos, records);
    the tensor is the one of the same call without stats."""
    import torch

    _png_stats_ids(stats)
    if perspective is not None and warp is not None:
        raise ValueError("perspective and warp exclude each other")
    if elastic is not None:
        if perspective is not None:
            raise ValueError("elastic and perspective exclude each other")
        els, eld = _png_elastics(elastic, len(datas))
        if boxes is not None and len(boxes) != len(datas):
            raise ValueError("boxes needs one entry (or None) per file")
        if warp is None:
            warp = _png_fit_warps(datas, boxes, size)
    wd = None
    if warp is not None or perspective is not None:
        wd = png_label_warp_desc(border, border_label, dtype)
    elif border != "constant" or border_label is not None:
        raise ValueError("border / border_label need warp")
    d, es = png_label_desc(size, dtype, lut)
    ws = _png_warps(warp, len(datas)) if warp is not None else None
    L = _png_spec_lib()
    L.debig_png_decode_batch_labels.restype = C.c_int
    L.debig_png_decode_batch_labels.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    dev = _png_device(L, device)
    n = len(datas)
    args = _png_batch_args(datas, boxes)
    tdt = {"uint8": torch.uint8, "uint16": getattr(torch, "uint16", torch.int16), "int32": torch.int32, "int64": torch.int64}[dtype]
    out = _png_dense_out((n, d.out_h, d.out_w), tdt, fill, dev)
    in_ptrs, in_sizes, bx, status, infos = args
    if elastic is not None:
        L.debig_png_decode_batch_labels_elastic.restype = C.c_int
        L.debig_png_decode_batch_labels_elastic.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        rc = L.debig_png_decode_batch_labels_elastic(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, status, infos, n, 0,
                                                     C.byref(d), C.byref(wd), els, C.byref(eld))
    elif perspective is not None:
        L.debig_png_decode_batch_labels_persp.restype = C.c_int
        L.debig_png_decode_batch_labels_persp.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_labels_persp(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, _png_persps(perspective, n),
                                                   status, infos, n, 0, C.byref(d), C.byref(wd))
    elif wd is not None:
        L.debig_png_decode_batch_labels_warp.restype = C.c_int
        L.debig_png_decode_batch_labels_warp.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_labels_warp(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, status, infos, n, 0,
                                                  C.byref(d), C.byref(wd))
    else:
        rc = L.debig_png_decode_batch_labels(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, status, infos, n, 0, C.byref(d))
    if rc == PNG_BAD_ARG:
        raise ValueError(f"debig_png_decode_batch_labels rejected its arguments ({rc})")
    N.check(rc, "debig_png_decode_batch_labels")
    res = [int(s) for s in status], out, [_info_dict(i) for i in infos]
    return res if stats is None else res + (png_label_stats(out, stats, res[0]),)


class PngColorMap(C.Structure):  # include/decode_png.h: debig_png_color_map
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("keys", C.POINTER(C.c_uint32)), ("values", C.POINTER(C.c_int32))]


class PngColorLabelDesc(C.Structure):  # include/decode_png.h: debig_png_color_label_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("dtype", C.c_uint32), ("mode", C.c_uint32), ("missing", C.c_int32),
                ("n_maps", C.c_uint32), ("maps", C.POINTER(PngColorMap)), ("reserved", C.c_uint32), ("reserved2", C.c_uint32)]


PNG_CL_PACK, PNG_CL_MAP = 0, 1  # include/decode_png.h: DEBIG_PNG_CL_*
PNG_CMAP_MAX = 2048  # DEBIG_PNG_CMAP_MAX


def png_pack_rgb(rgb):
    """(..., 3) integers R, G, B in 0 .. 255 -> the packed colours R | G << 8 | B << 16 the colour-label call looks up"""
    a = np.asarray(rgb)
    if a.ndim < 1 or a.shape[-1] != 3 or a.dtype.kind not in "iu":
        raise ValueError("colours need a last axis of 3 integers")
    if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
        raise ValueError("colour components must lie in 0 .. 255")
    a = a.astype(np.uint32)
    return a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16)


def _png_color_map_arrays(colors):
    """one map -- a dict {(r, g, b): value} or a pair (keys, values), keys packed or (m, 3) RGB -> (uint32 keys, int32 values);
    what the arrays hold (range, distinct keys, the size limit) is the C call's to judge"""
    if isinstance(colors, dict):
        keys = png_pack_rgb(np.array(list(colors.keys()), dtype=np.int64).reshape(len(colors), 3))
        values = np.array(list(colors.values()))
    elif isinstance(colors, tuple) and len(colors) == 2:
        keys, values = np.asarray(colors[0]), np.asarray(colors[1])
        if keys.ndim == 2:
            keys = png_pack_rgb(keys)
    else:
        raise ValueError("a colour map is a dict {(r, g, b): value} or a pair (keys, values)")
    if keys.ndim != 1 or values.shape != keys.shape or (keys.size and (keys.dtype.kind not in "iu" or values.dtype.kind not in "iu")):
        raise ValueError("a colour map needs as many integer values as keys")
    if keys.size and (int(keys.min()) < 0 or int(keys.max()) > 0xFFFFFFFF or int(values.min()) < -2 ** 31 or int(values.max()) > 2 ** 31 - 1):
        raise ValueError("colour keys are uint32 and values int32")
    return np.ascontiguousarray(keys, dtype=np.uint32), np.ascontiguousarray(values, dtype=np.int32)


def png_color_label_desc(size, colors=None, missing=-1, dtype="int64", n=None):
    """the debig_png_color_label_desc of png_decode_batch_color_labels' arguments (no GPU needed) -> (desc, element bytes).
    colors: None (PACK), one map, or a list of n maps (n: the number of files).  The desc keeps the arrays alive (desc._keep)."""
    if dtype not in PNG_LABEL_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(PNG_LABEL_DTYPES)}, not {dtype!r}")
    H, W = (int(v) for v in size)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"size must be (H, W) with 1 <= H, W <= 16384, not {size!r}")
    d = PngColorLabelDesc(out_w=W, out_h=H, dtype=PNG_LABEL_DTYPES[dtype], mode=PNG_CL_PACK)
    if colors is None:
        if dtype not in ("int32", "int64"):
            raise ValueError("packed colours (colors=None) need dtype 'int32' or 'int64'")
        return d, 1 << PNG_LABEL_DTYPES[dtype]
    if isinstance(colors, list):
        if n is None or len(colors) != n:
            raise ValueError("a list of colour maps needs one map per file")
        maps = [_png_color_map_arrays(m) for m in colors]
    else:
        maps = [_png_color_map_arrays(colors)]
    if not -2 ** 31 <= int(missing) <= 2 ** 31 - 1:
        raise ValueError("missing must be an int32")
    arr = (PngColorMap * max(len(maps), 1))()
    for m, (k, v) in zip(arr, maps):
        m.n = len(k)
        m.keys = k.ctypes.data_as(C.POINTER(C.c_uint32))
        m.values = v.ctypes.data_as(C.POINTER(C.c_int32))
    d._keep = (arr, maps)
    d.mode, d.missing, d.n_maps, d.maps = PNG_CL_MAP, int(missing), len(maps), arr
    return d, 1 << PNG_LABEL_DTYPES[dtype]


def png_decode_batch_color_labels(datas, size, colors=None, missing=-1, dtype="int64", boxes=None, fill=None, device="cuda:0",
                                  perspective=None, elastic=None, stats=None, warp=None, border="constant", border_label=None):
    """bytes of N colour-coded label PNGs -> ONE dense (N, H, W) integer tensor on the GPU (include/decode_png.h:
    debig_png_decode_batch_color_labels) -> (statuses, tensor, infos, unmatched).  The colour of a pixel is what
    png_decode_batch(mode="rgb") gives for it (palette files through PLTE, grey replicated, alpha and tRNS dropped), packed as
    R | G << 8 | B << 16.  colors=None: the element is the packed colour itself (COCO panoptic's rgb2id; dtype "int32" or
    "int64").  colors = a dict {(r, g, b): value} or a pair (keys, values) -- keys packed, or (m, 3) RGB; at most 2048 distinct
    colours --: the element is the colour's value, or `missing`; a list of N of those gives every file its own map (COCO
    panoptic's per-image segment id -> category tables, with keys packed as the segment ids are).  unmatched[i]: how many
    elements of image i took `missing`.  size, boxes, fill, dtype, the device rule and the grid are those of
    png_decode_batch_labels; 16-bit files have status 15 ("label").
    warp: None (everything above, unchanged), or one entry per file: None (the identity) or the INVERSE 2 x 3 matrix of
    png_decode_batch_tensor(warp=) -- debig_png_decode_batch_color_labels_warp: the pick is the one of that call's
    filter="nearest" and of png_decode_batch_labels(warp=) under the same matrix, so an image and its colour mask stay aligned.
    border: "constant" (a pick outside the crop stores border_label as it is, not through the map, and is never counted in
    unmatched: the ignore index; default 0) or "clamp".  A matrix with a non-finite or too large entry: status 16 ("warp").
    perspective (by name): in place of warp (both together: ValueError), one entry per file: None (the identity) or the INVERSE
    3 x 3 matrix of png_decode_batch_tensor(perspective=) -- debig_png_decode_batch_color_labels_persp: the same pick as that
    call's filter="nearest" and png_decode_batch_labels(perspective=); border, border_label and unmatched as for warp.  A horizon
    across the output: status 16.  NOTE: `perspective` stands in front of `warp` in the parameter list (`warp`, `border` and
    `border_label` stay the last three), so `warp`, `border` and `border_label` are to be passed BY NAME from now on: a call that
    passed `warp` as the ninth positional argument now hands it to `perspective` and is refused (a 2 x 3 entry is no 3 x 3 matrix).
    elastic (by name; it stands behind `perspective`, so `warp`, `border` and `border_label` stay the last three): None, or one
    entry per file: None or a (grid_h, grid_w, 2) displacement field, as png_decode_batch_tensor(elastic=) takes it --
    debig_png_decode_batch_color_labels_elastic: the same pick as that call's filter="nearest" and
    png_decode_batch_labels(elastic=); border, border_label and unmatched as for warp.  It goes with warp; without warp each
    file takes png_warp_matrix((crop_w, crop_h), size).  With perspective: ValueError.  A bad node: status 16.
    stats (by name; it stands behind `elastic`, so `warp`, `border` and `border_label` stay the last three): None (everything
    above, the return value included), or num_ids: the call runs png_label_stats(tensor, num_ids, statuses) on the tensor it has
    just written and returns (statuses, tensor, infos, unmatched, records).  Under a map, record "other" of an image counts its `missing` elements (when missing is no id below num_ids) and
    the border picks alike; packed colours (colors=None) are ids like any other, so most of them are "other"."""
    import torch

    _png_stats_ids(stats)
    if perspective is not None and warp is not None:
        raise ValueError("perspective and warp exclude each other")
    if elastic is not None:
        if perspective is not None:
            raise ValueError("elastic and perspective exclude each other")
        els, eld = _png_elastics(elastic, len(datas))
        if boxes is not None and len(boxes) != len(datas):
            raise ValueError("boxes needs one entry (or None) per file")
        if warp is None:
            warp = _png_fit_warps(datas, boxes, size)
    wd = None
    if warp is not None or perspective is not None:
        wd = png_label_warp_desc(border, border_label, dtype)
    elif border != "constant" or border_label is not None:
        raise ValueError("border / border_label need warp")
    n = len(datas)
    d, es = png_color_label_desc(size, colors, missing, dtype, n)
    ws = _png_warps(warp, n) if warp is not None else None
    L = _png_spec_lib()
    L.debig_png_decode_batch_color_labels.restype = C.c_int
    L.debig_png_decode_batch_color_labels.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p]
    dev = _png_device(L, device)
    args = _png_batch_args(datas, boxes)
    tdt = {"uint8": torch.uint8, "uint16": getattr(torch, "uint16", torch.int16), "int32": torch.int32, "int64": torch.int64}[dtype]
    out = _png_dense_out((n, d.out_h, d.out_w), tdt, fill, dev)
    in_ptrs, in_sizes, bx, status, infos = args
    unmatched = (C.c_uint32 * n)()
    if elastic is not None:
        L.debig_png_decode_batch_color_labels_elastic.restype = C.c_int
        L.debig_png_decode_batch_color_labels_elastic.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        rc = L.debig_png_decode_batch_color_labels_elastic(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, status, infos,
                                                           unmatched, n, 0, C.byref(d), C.byref(wd), els, C.byref(eld))
    elif perspective is not None:
        L.debig_png_decode_batch_color_labels_persp.restype = C.c_int
        L.debig_png_decode_batch_color_labels_persp.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_color_labels_persp(in_ptrs, in_sizes, out.data_ptr() if n else None, bx,
                                                         _png_persps(perspective, n), status, infos, unmatched, n, 0, C.byref(d),
                                                         C.byref(wd))
    elif wd is not None:
        L.debig_png_decode_batch_color_labels_warp.restype = C.c_int
        L.debig_png_decode_batch_color_labels_warp.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        rc = L.debig_png_decode_batch_color_labels_warp(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, ws, status, infos,
                                                        unmatched, n, 0, C.byref(d), C.byref(wd))
    else:
        rc = L.debig_png_decode_batch_color_labels(in_ptrs, in_sizes, out.data_ptr() if n else None, bx, status, infos, unmatched,
                                                   n, 0, C.byref(d))
    if rc == PNG_BAD_ARG:
        raise ValueError(f"debig_png_decode_batch_color_labels rejected its arguments ({rc})")
    N.check(rc, "debig_png_decode_batch_color_labels")
    res = [int(s) for s in status], out, [_info_dict(i) for i in infos], [int(u) for u in unmatched]
    return res if stats is None else res + (png_label_stats(out, stats, res[0]),)


class ApngFrame(C.Structure):  # include/decode_png.h: debig_apng_frame
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("x_off", C.c_uint32), ("y_off", C.c_uint32),
                ("delay_num", C.c_uint16), ("delay_den", C.c_uint16), ("dispose_op", C.c_uint8), ("blend_op", C.c_uint8),
                ("reserved", C.c_uint16)]


class ApngInfo(C.Structure):  # include/decode_png.h: debig_apng_info
    _fields_ = [("png", PngInfo), ("num_frames", C.c_uint32), ("num_plays", C.c_uint32),
                ("default_is_frame", C.c_uint32), ("reserved", C.c_uint32)]


_APNG_LIST_CAP = 1 << 16  # frames listed for a file that fails the walk (its num_frames is only what acTL claims)


def _apng_lib():
    L = _png_spec_lib()
    L.debig_apng_info_get.restype = C.c_uint32
    L.debig_apng_info_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ApngInfo), C.c_void_p, C.c_uint32]
    L.debig_apng_decode_batch.restype = C.c_int
    L.debig_apng_decode_batch.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32]
    return L


def apng_info(data):
    """the whole chunk walk of a PNG or APNG, no CRCs (host only, include/decode_png.h: debig_apng_info_get) ->
    (status, info): the png_info dict plus num_frames, num_plays, default_is_frame and frames, a list of dicts with x, y,
    width, height, delay_num, delay_den, dispose and blend (a still PNG: one frame, the whole canvas)"""
    d = _u8(data)
    L = _apng_lib()
    inf = ApngInfo()
    st = L.debig_apng_info_get(d.ctypes.data, len(d), C.byref(inf), None, 0)
    cap = inf.num_frames if st == 0 else min(inf.num_frames, _APNG_LIST_CAP)
    frames = (ApngFrame * max(cap, 1))()
    if cap:
        L.debig_apng_info_get(d.ctypes.data, len(d), C.byref(inf), frames, cap)
    out = _info_dict(inf.png)
    out.update(num_frames=int(inf.num_frames), num_plays=int(inf.num_plays), default_is_frame=int(inf.default_is_frame))
    out["frames"] = [{"x": int(f.x_off), "y": int(f.y_off), "width": int(f.width), "height": int(f.height),
                      "delay_num": int(f.delay_num), "delay_den": int(f.delay_den), "dispose": int(f.dispose_op),
                      "blend": int(f.blend_op)} for f in frames[:cap] if f.width]
    return st, out


def apng_decode_batch(datas, force_general=False):
    """animated (and still) PNGs -> composited RGBA8 frames (include/decode_png.h: debig_apng_decode_batch) ->
    [(status, ndarray (F, H, W, 4) uint8 or None, info dict as apng_info gives it)], status as in PNG_STATUS; frame k is
    the canvas after frame k is rendered, before its dispose_op"""
    L = _apng_lib()
    n = len(datas)
    ins = [_u8(d) for d in datas]
    outs, caps, pre = [], [], []
    for a in ins:
        st, inf = apng_info(a)
        pre.append(inf)
        if st == 0:
            outs.append(np.empty((inf["num_frames"], inf["height"], inf["width"], 4), dtype=np.uint8))
            caps.append(outs[-1].nbytes)
        else:
            outs.append(np.empty(4, dtype=np.uint8))
            caps.append(0)
    in_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    in_sizes = (C.c_uint64 * n)(*[len(a) for a in ins])
    out_ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    caps = (C.c_uint64 * n)(*caps)
    status = (C.c_uint32 * n)()
    rc = L.debig_apng_decode_batch(in_ptrs, in_sizes, out_ptrs, caps, status, None, n,
                                   PNG_FORCE_GENERAL if force_general else 0)
    N.check(rc, "debig_apng_decode_batch")
    return [(int(status[i]), outs[i] if status[i] == 0 else None, pre[i]) for i in range(n)]
