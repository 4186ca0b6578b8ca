"""GPU: the battery of tests/checksum_battery.py through debig_hip_checksum_batch on the MI355X, every result against zlib.  The
launches are the ones tests/test_emu_checksum.py runs on the emulator (the many-spans launch has 70 000 spans here: one workgroup
each, a grid past 65 535); nothing is compared with the emulator, which is not loaded.  One kernel launch per battery launch and
kind.  The arena must come back unchanged, and so must the 64 sentinel bytes on either side of the result array."""
import ctypes as C

import numpy as np
import pytest

import checksum_battery as B

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5A5A5A5 - (1 << 32)  # as int32


@pytest.fixture(scope="module")
def run(gpu_device):
    import torch

    from debigulator_amd import _native as N
    from debigulator_amd.checksum import SPAN_DTYPE, _lib

    L = _lib()

    def _run(la, kind):
        block = torch.full((len(la.data) + 32,), 0xC3, dtype=torch.uint8, device=gpu_device)
        start = (la.residue - block.data_ptr()) % 16
        arena = block[start:start + len(la.data)]
        arena.copy_(torch.from_numpy(la.data))
        assert arena.data_ptr() % 16 == la.residue
        n = len(la.spans)
        sp = np.zeros(max(n, 1), dtype=SPAN_DTYPE)
        sp["off"][:n] = [s[0] for s in la.spans]
        sp["len"][:n] = [s[1] for s in la.spans]
        d_spans = torch.from_numpy(sp.view(np.uint8).reshape(-1)).to(gpu_device)
        d_out = torch.full((n + 32,), SENTINEL, dtype=torch.int32, device=gpu_device)
        stream = torch.cuda.current_stream(gpu_device)
        rc = L.debig_hip_checksum_batch(arena.data_ptr(), d_spans.data_ptr(), d_out[16:].data_ptr(), n, kind,
                                        C.c_void_p(stream.cuda_stream))
        N.check(rc, "debig_hip_checksum_batch")
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.uint32)
        whole = block.cpu().numpy()
        assert (whole[start:start + len(la.data)] == la.data).all()  # the kernel only reads the arena
        assert (whole[:start] == 0xC3).all() and (whole[start + len(la.data):] == 0xC3).all()
        assert (out[:16] == 0xA5A5A5A5).all() and (out[16 + n:] == 0xA5A5A5A5).all()  # n results, nothing else
        return out[16:16 + n]

    return _run


def both_kinds(run, la):
    for kind, _ in B.KINDS:
        B.check(la, kind, run(la, kind))


def test_battery_covers_what_it_claims():
    B.assert_coverage(B.launches(B.MANY_GPU), big_grid=True)


@pytest.mark.parametrize("fill", B.FILLS)
def test_alignment_and_length_grid(run, fill):
    """every front residue x the lengths around a lane load, a piece and 1, 2, 3 tiles (393 spans), trail == 0 included"""
    both_kinds(run, B.grid(fill))


def test_arena_pointer_at_every_residue(run):
    for f in range(16):
        both_kinds(run, B.arena_residue(f))


@pytest.mark.parametrize("inner,outer", [(0x00, 0xFF), (0xFF, 0x00)])
def test_bytes_around_a_span_stay_out_of_its_sums(run, inner, outer):
    both_kinds(run, B.surround(inner, outer))


def test_adler_sums_at_their_largest(run):
    """0xFF up to 4 MiB + 3: lengths around 65521, sums past 2^32 before the modulus"""
    both_kinds(run, B.adler_modulus())


def test_one_byte_at_each_class_of_position(run):
    both_kinds(run, B.moving_byte())


def test_many_spans_in_one_launch_past_a_16_bit_grid(run):
    la = B.many(B.MANY_GPU)
    assert len(la.spans) > B.GRID_LIMIT
    both_kinds(run, la)


def test_first_and_last_byte_of_the_allocation(run):
    for r in range(16):
        both_kinds(run, B.ends(r))


def test_no_spans_no_writes(run):
    la = B.Launch("none", np.zeros(64, dtype=np.uint8), [])
    for kind, _ in B.KINDS:
        assert len(run(la, kind)) == 0
