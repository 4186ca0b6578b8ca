"""CPU: the battery of tests/checksum_battery.py through debig_checksum_kernel on the lock-step emulator (emu_checksum_batch), every
result against zlib.  The arena of a launch is a numpy view whose first byte sits at the address residue the launch asks for.
tests/test_gpu_checksum.py runs the same launches on the MI355X."""
import ctypes as C

import numpy as np
import pytest

import checksum_battery as B
import emu_binding as eb


class Span(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64)]


@pytest.fixture(scope="module")
def emu():
    L = eb.load_emu()
    L.emu_checksum_batch.restype = C.c_int
    L.emu_checksum_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    return L


def at_residue(data, residue):
    """a copy of data whose first byte has address = residue (mod 16), inside a block of 0xC3 bytes"""
    block = np.full(len(data) + 32, 0xC3, dtype=np.uint8)
    start = (residue - block.ctypes.data) % 16
    view = block[start:start + len(data)]
    view[:] = data
    assert view.ctypes.data % 16 == residue
    return view


def run(emu, la, kind):
    arena = at_residue(la.data, la.residue)
    n = len(la.spans)
    spans = (Span * max(n, 1))()
    for i, (off, ln) in enumerate(la.spans):
        spans[i].off, spans[i].len = off, ln
    out = np.full(n + 32, 0xA5A5A5A5, dtype=np.uint32)
    assert emu.emu_checksum_batch(arena.ctypes.data, spans, out[16:].ctypes.data, n, kind) == 0
    assert (arena == la.data).all()  # the kernel only reads the arena
    assert (out[:16] == 0xA5A5A5A5).all() and (out[16 + n:] == 0xA5A5A5A5).all()  # and writes n results, nothing else
    return out[16:16 + n]


def both_kinds(emu, la):
    for kind, _ in B.KINDS:
        B.check(la, kind, run(emu, la, kind))


def test_battery_covers_what_it_claims():
    B.assert_coverage(B.launches(B.MANY_EMU), big_grid=False)
    B.assert_coverage(B.launches(B.MANY_GPU), big_grid=True)  # the list the GPU runs


@pytest.mark.parametrize("fill", B.FILLS)
def test_alignment_and_length_grid(emu, fill):
    """every front residue x the lengths around a lane load, a piece and 1, 2, 3 tiles (393 spans), trail == 0 included"""
    both_kinds(emu, B.grid(fill))


def test_arena_pointer_at_every_residue(emu):
    for f in range(16):
        both_kinds(emu, B.arena_residue(f))


@pytest.mark.parametrize("inner,outer", [(0x00, 0xFF), (0xFF, 0x00)])
def test_bytes_around_a_span_stay_out_of_its_sums(emu, inner, outer):
    both_kinds(emu, B.surround(inner, outer))


def test_adler_sums_at_their_largest(emu):
    """0xFF up to 4 MiB + 3: lengths around 65521, sums past 2^32 before the modulus"""
    both_kinds(emu, B.adler_modulus())


def test_one_byte_at_each_class_of_position(emu):
    both_kinds(emu, B.moving_byte())


def test_many_spans_in_one_launch(emu):
    both_kinds(emu, B.many(B.MANY_EMU))


def test_first_and_last_byte_of_the_allocation(emu):
    for r in range(16):
        both_kinds(emu, B.ends(r))


def test_no_spans_no_writes(emu):
    la = B.Launch("none", np.zeros(64, dtype=np.uint8), [])
    for kind, _ in B.KINDS:
        assert len(run(emu, la, kind)) == 0
