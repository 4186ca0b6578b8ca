"""TEST TOOLING: the battery of the checksum kernel (csrc/checksum_kernel.inc: debig_checksum_kernel), for two back ends: the CPU
lock-step emulator (tests/test_emu_checksum.py) and debig_hip_checksum_batch on the MI355X (tests/test_gpu_checksum.py).  Plain
data: a Launch is the bytes of one arena, the residue mod 16 its first byte is to have as an ADDRESS, and the spans (off, len) of
one kernel launch.  A back end hands check() a function (launch, kind) -> the uint32 results; check() compares every result with
zlib.crc32 / zlib.adler32 of the same bytes.  Nothing here loads a library or the emulator.

What the cases are for, in the kernel's terms (front = address of the span's first byte mod 16, plen = front + len, the tile grid
starts `front` bytes below the span, trail = zero bytes staged behind the span in its last tile):
  * grid(fill): every front x the lengths around a 16-byte lane load, a 64-byte piece and 1, 2 and 3 tiles, measured both from the
    span's start and from the grid's (plen a whole number of tiles: trail == 0), on random bytes, on 0xFF and on zeros;
  * arena_residue(f): the same lengths with span.off = 0 and the ARENA pointer at residue f;
  * surround(inner, outer): a span of one value inside the other -- a byte read from outside the span changes the answer;
  * adler_modulus(): long runs of 0xFF, where every partial sum of Adler-32 is as large as it gets;
  * moving_byte(): one 0x01 in a span of zeros, at each class of position (lane, piece, tile, first and last byte), so one
    position weight (Adler) or one power of x (CRC) decides the answer alone;
  * many(n): n short spans, duplicated, overlapping, and a second time in reverse order -- one workgroup each;
  * ends(r): spans that start at the first byte and end at the last byte of the allocation, the last byte at residue r."""
import random
import zlib

import numpy as np

T, PIECE, LANE = 16384, 64, 16  # CK_TILE, CK_PIECE, bytes per lane load
CRC32, ADLER32 = 0, 1
KINDS = ((CRC32, zlib.crc32), (ADLER32, zlib.adler32))
FILLS = ("random", "ff", "zero")
ADLER_LENS = [65520, 65521, 65522, 2 * 65521, 3 * 5552, 1 << 20, (4 << 20) + 3]
MOVING_LEN, MOVING_F = 2 * T + 5, 5
MOVING_POS = [0, 1, 15, 16, 63, 64, T - 6, T - 5, T - 4, 2 * T - 1, 2 * T + 4]
MANY_GPU, MANY_EMU = 70000, 2000
GRID_LIMIT = 65535  # a launch with more workgroups than this needs the 32-bit grid


class Launch:
    def __init__(self, name, data, spans, residue=0):
        self.name, self.data, self.spans, self.residue = name, data, list(spans), residue
        assert data.dtype == np.uint8 and 0 <= residue < 16
        for off, n in self.spans:
            assert 0 <= off and off + n <= len(data), (name, off, n)

    def front(self, i):
        return (self.residue + self.spans[i][0]) % 16


def lengths(f):
    """the lengths of the alignment x length grid for front residue f"""
    raw = [0, 1, 2, 3, 4, 15, 16, 17, 16 - f, 17 - f, 63, 64, 65, 64 - f, 65 - f, T - 1, T, T + 1, T - f - 1, T - f, T - f + 1,
           2 * T - f - 1, 2 * T - f, 2 * T - f + 1, 3 * T - f, 3 * T - f + 1]
    return sorted({n for n in raw if n >= 0})


GRID = [(f, n) for f in range(16) for n in lengths(f)]
assert len(GRID) == 393
# a padded length of exactly 1, 2 and 3 tiles (trail == 0) for every front residue
assert {(f, (f + n) // T) for f, n in GRID if n and (f + n) % T == 0} >= {(f, k) for f in range(16) for k in (1, 2, 3)}


def _filled(n, fill, seed=0):
    if fill == "random":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return np.full(n, {"ff": 0xFF, "zero": 0x00}[fill], dtype=np.uint8)


def _pack(specs, gap=32, lead=64):
    """offsets for spans (front residue, length) in an arena whose pointer is 16-byte aligned, `gap` bytes or more between two
    spans and `lead` in front of the first and behind the last -> (offsets, arena size)"""
    offs, cur = [], lead
    for f, n in specs:
        off = cur + (f - cur) % 16
        offs.append(off)
        cur = off + n + gap
    return offs, cur + lead


def grid(fill):
    """all 393 spans of the alignment x length grid in one launch"""
    offs, size = _pack(GRID)
    la = Launch("grid-" + fill, _filled(size, fill, 11), [(o, n) for o, (f, n) in zip(offs, GRID)])
    assert [la.front(i) for i in range(len(GRID))] == [f for f, n in GRID]
    return la


def arena_residue(f):
    """the lengths of front residue f with span.off = 0: the arena pointer itself sits at residue f"""
    ns = lengths(f)
    la = Launch("arena-residue-%d" % f, _filled(max(ns) + 48, "random", 100 + f), [(0, n) for n in ns], residue=f)
    assert all(la.front(i) == f for i in range(len(ns)))
    return la


def surround(inner, outer):
    """spans of `inner` bytes in an arena of `outer` bytes, 32 bytes or more of it on both sides of every span"""
    specs = [(f, n) for f in range(16) for n in (1, 5, 16, 17, 100, T - f, T + 3)]
    offs, size = _pack(specs, gap=40)
    data = np.full(size, outer, dtype=np.uint8)
    for o, (f, n) in zip(offs, specs):
        assert (data[o - 32:o] == outer).all() and (data[o:o + n + 32] == outer).all()  # no overlap, surround intact so far
        data[o:o + n] = inner
    return Launch("surround-%02x-in-%02x" % (inner, outer), data, [(o, n) for o, (f, n) in zip(offs, specs)])


def adler_modulus():
    """0xFF from residue 3 on: a, s1, bs and sum_a of the Adler branch at their largest, lengths around the modulus 65521, a
    multiple of zlib's own block NMAX = 5552, and 256 tiles and more"""
    return Launch("adler-modulus", _filled(3 + max(ADLER_LENS) + 29, "ff"), [(3, n) for n in ADLER_LENS])


def moving_byte():
    specs = [(MOVING_F, MOVING_LEN)] * len(MOVING_POS)
    offs, size = _pack(specs)
    data = np.zeros(size, dtype=np.uint8)
    for o, p in zip(offs, MOVING_POS):
        assert 0 <= p < MOVING_LEN
        data[o + p] = 1
    return Launch("moving-byte", data, [(o, MOVING_LEN) for o in offs])


def many(n):
    """n spans of 0 .. 40 bytes at random offsets of a 100 000-byte arena: overlaps and duplicates by construction (every eighth
    span repeats an earlier one), and the second half of the list is the first half in reverse order"""
    rng = random.Random(70)
    half = []
    for i in range(n // 2):
        if i % 8 == 7:
            half.append(half[rng.randrange(len(half))])
        else:
            ln = rng.randint(0, 40)
            half.append((rng.randrange(0, 100000 - ln + 1), ln))
    spans = half + half[::-1]
    assert len(spans) == n and len(set(spans)) < n // 2
    return Launch("many-%d" % n, _filled(100000, "random", 71), spans)


def ends(r):
    """an arena that is the whole allocation, its last byte at address residue r: one span covers it all (starts at byte 0, ends
    at the last byte), the others end at the last byte after a start at every residue"""
    size = T + 48 + (r + 1) % 16  # the address of the last byte = size - 1 = r (mod 16): the arena pointer is 16-byte aligned
    spans = [(0, size), (0, 1), (0, 17)] + [(size - n, n) for n in (1, 2, 15, 16, 17, 33, 64, 100)]
    la = Launch("ends-%d" % r, _filled(size, "random", 200 + r), spans)
    assert (size - 1) % 16 == r
    return la


def launches(n_many):
    """every launch of the battery, in the order the tests run them"""
    out = [grid(fill) for fill in FILLS] + [arena_residue(f) for f in range(16)]
    out += [surround(0x00, 0xFF), surround(0xFF, 0x00), adler_modulus(), moving_byte(), many(n_many)]
    out += [ends(r) for r in range(16)]
    return out


def assert_coverage(las, big_grid):
    """what the issue asks the battery to assert about itself"""
    fronts = {}
    for la in las:
        for i, (off, n) in enumerate(la.spans):
            if n and (la.front(i) + n) % T == 0:
                fronts.setdefault(la.front(i), set()).add((la.front(i) + n) // T)
    assert all(fronts.get(f, set()) >= {1, 2, 3} for f in range(16)), fronts  # trail == 0 at 1, 2 and 3 tiles, every front
    assert {la.residue for la in las if all(off == 0 for off, n in la.spans)} >= set(range(16))  # the arena pointer at every residue
    assert {(len(la.data) - 1) % 16 for la in las if la.name.startswith("ends-")} == set(range(16))
    if big_grid:
        assert max(len(la.spans) for la in las) > GRID_LIMIT  # one workgroup per span: the grid is past 16 bits


def want(la, kind):
    fn = dict(KINDS)[kind]
    raw = la.data.tobytes()
    return [fn(raw[off:off + n]) & 0xFFFFFFFF for off, n in la.spans]


def check(la, kind, got):
    """got: the kernel's uint32 results of launch `la` for `kind`"""
    exp = want(la, kind)
    assert len(got) == len(exp)
    bad = [(i, la.spans[i], la.front(i), "%08x" % int(g), "%08x" % e) for i, (g, e) in enumerate(zip(got, exp)) if int(g) != e]
    assert not bad, (la.name, kind, len(bad), bad[:5])
