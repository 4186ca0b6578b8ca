"""CPU: the oracle against the COMPILED, UNMODIFIED reference (oracle/_ref, built by oracle/Makefile), on
fuzzed, flush-heavy, damaged and sample inputs.  The reference's answers to exactly these inputs are stored as
digests in tests/golden/vs_reference.json: tests/golden/make_golden.py --only-vs-reference records them by
running this module against the live reference, so the module needs nothing outside the repository."""
import glob
import hashlib
import json
import os
import random
import zlib

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ANSWERS = os.path.join(GOLD, "vs_reference.json")


def _digest(b):
    return hashlib.sha256(bytes(b)).hexdigest()[:32]


class StoredReference:
    """The reference's answers as digests: inflate -> (good, final, sha), decode_png / decode_gz -> (good, sha),
    inflate_b (build B, asserts off, in a child process) -> (good, final, sha) or None where it died.
    live = (binding.Reference("A"), ref_worker.RefWorker()): record the answers instead of looking them up."""

    def __init__(self, answers, live=None):
        self.answers, self.live = answers, live

    def _answer(self, op, size, data, compute):
        k = hashlib.sha256(f"{op} {size} ".encode() + bytes(data)).hexdigest()[:32]
        if self.live is not None:
            self.answers[k] = compute()
        assert k in self.answers, f"{op}: input not in {ANSWERS} (tests/golden/make_golden.py --only-vs-reference)"
        a = self.answers[k]
        return None if a is None else tuple(a)

    def inflate(self, raw, cap):
        def live():
            g, f, o = self.live[0].inflate(raw, cap)
            return [g, f, _digest(o)]
        return self._answer("inflate", cap, raw, live)

    def inflate_b(self, raw, cap):
        def live():
            r = self.live[1].inflate("B", raw, cap)
            return None if r is None else [r[0], r[1], r[2][:32]]
        return self._answer("inflate_b", cap, raw, live)

    def decode_png(self, data, rgba_size=None):
        def live():
            g, o = self.live[0].decode_png(data, tid=2, rgba_size=rgba_size)
            return [g, _digest(o)]
        return self._answer("decode_png", rgba_size, data, live)

    def decode_gz(self, data, expect_size):
        def live():
            g, o = self.live[0].decode_gz(data, expect_size)
            return [g, _digest(o)]
        return self._answer("decode_gz", expect_size, data, live)


@pytest.fixture(scope="module")
def ref():
    return StoredReference(json.load(open(ANSWERS)))


def test_raw_inflate_fuzz(oracle, ref):
    rng = random.Random(77)
    truncated = 0
    for it in range(1500):
        n = rng.randint(1, 6000)
        kind = rng.randint(0, 3)
        if kind == 0:
            data = bytes(rng.getrandbits(8) for _ in range(n))
        elif kind == 1:
            words = [bytes(rng.getrandbits(8) for _ in range(rng.randint(3, 9))) for _ in range(100)]
            data = (b" ".join(rng.choice(words) for _ in range(n // 5 + 1)))[:n]
        elif kind == 2:
            data = bytes([rng.choice(b"ab")]) * n
        else:
            data = bytes(rng.choice(b"abcdefgh") for _ in range(n))
        c = zlib.compressobj(rng.choice([0, 1, 6, 9]), zlib.DEFLATED, -15, 9,
                             rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]))
        raw = c.compress(data) + c.flush()
        cap = max(len(data) + 1, len(raw))
        a = oracle.inflate(raw, cap)
        assert (a[0], a[1], _digest(a[2])) == ref.inflate(raw, cap), it
        truncated += a[2] != data
    assert truncated > 10  # the tail rule Q2 really fires and both sides agree on it


def test_flush_heavy_streams(oracle, ref):
    """Encoders that flush every few bytes (PNG writers flushing per row): hundreds of blocks,
    empty stored blocks in between, fixed and dynamic codes.  The GPU kernels treat this pattern
    specially (short-block probe), so the oracle is pinned to the reference on it as well."""
    rng = random.Random(78)
    for it in range(250):
        data = bytes(rng.choice(b"abcdefgh \n") for _ in range(rng.randint(20, 5000)))
        c = zlib.compressobj(rng.choice([0, 1, 6, 9]), zlib.DEFLATED, -15, 9,
                             rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE]))
        raw, i, maxchunk = b"", 0, rng.choice([3, 20, 60, 200])
        while i < len(data):
            n = rng.randint(1, maxchunk)
            raw += c.compress(data[i:i + n])
            i += n
            raw += c.flush(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_BLOCK]))
        raw += c.flush()
        cap = max(len(data) + 1, len(raw))
        g, f, o = oracle.inflate(raw, cap)
        assert (g, f, _digest(o)) == ref.inflate(raw, cap), it


def test_gates(oracle, ref):
    raw = zlib.compress(b"hello world " * 40)[2:-4]
    # (recipient_size between C and D is excluded: the asserts-on reference aborts there, Q12)
    for cap in (len(raw) - 1, 4096):
        assert oracle.inflate(raw, cap)[:2] == ref.inflate(raw, cap)[:2]
    for short in (b"\x03\x00", b"\x4b\x04\x00", b"\x4b\x04\x00\x00"):
        assert oracle.inflate(short, 64)[:2] == ref.inflate(short, 64)[:2] == (0, None)


def test_resources(oracle, ref):
    for f in sorted(glob.glob(os.path.join(GOLD, "resources", "*.png"))):
        d = open(f, "rb").read()
        g1, o1 = oracle.decode_png(d)
        assert (g1, _digest(o1)) == ref.decode_png(d), os.path.basename(f)
    d = open(os.path.join(GOLD, "resources", "gzipsample.gz"), "rb").read()
    g1, o1, n = oracle.decode_gz(d, 600000)
    assert (g1, _digest(o1)) == ref.decode_gz(d, n) and g1 == 1


def _safe_offsets(png):
    """byte offsets whose corruption keeps the reference inside defined behaviour: chunk
    types, CRCs, IHDR flags, the zlib header -- never a chunk length or IDAT payload (the
    reference computes the CRC over `length` bytes before it bounds-checks the length)."""
    offs = list(range(0, 8))
    at = 8
    first_idat = True
    while at + 8 <= len(png):
        ln = int.from_bytes(png[at:at + 4], "big")
        typ = bytes(png[at + 4:at + 8])
        offs += list(range(at + 4, at + 8))
        if typ == b"IHDR":
            offs += list(range(at + 8 + 8, at + 8 + 13))
        if typ == b"IDAT" and first_idat:
            offs += [at + 8, at + 9]
            first_idat = False
        offs += list(range(at + 8 + ln, at + 12 + ln))
        at += 12 + ln
    return offs


def test_png_rejects_agree(oracle, ref):
    base = bytearray(open(os.path.join(GOLD, "resources", "structuredart1.png"), "rb").read())
    offs = _safe_offsets(base)
    rng = random.Random(5)
    rejected = 0
    for it in range(200):
        d = bytearray(base)
        for _ in range(rng.randint(1, 2)):
            d[rng.choice(offs)] ^= 1 << rng.randrange(8)
        g1, o1 = oracle.decode_png(bytes(d), rgba_size=400)
        g2, o2 = ref.decode_png(bytes(d), rgba_size=400)
        assert g1 == g2, it
        rejected += g1 == 0
        if g1:
            assert _digest(o1) == o2, it
    assert rejected > 50


from ref_worker import corrupt_cases  # noqa: E402


def test_corrupted_raw_streams_fail_like_the_reference(oracle, ref):
    """VERDICT r1 missing-5: HOW the reference fails on damaged raw streams -- bad code-length code
    (src/inflate.c:1427-1434), distance symbol > 29 (:1809), distance beyond the output with the
    partial final size (:1843-1852), undecodable bit patterns (:465-473), stored LEN/NLEN (:949) --
    pinned on the same mutators the GPU suite leans on.  Reference build B (asserts off: build A
    aborts where B reports), in a child process; cases on which the oracle notes undefined
    behaviour of the reference (ub_flags) or the reference dies are excluded."""
    compared = failed = partial = crashes = 0
    for it, (raw, cap) in enumerate(corrupt_cases(4242, 1500)):
        g, f, o, st = oracle.inflate(raw, cap, want_stats=True)
        if st.ub_flags:
            continue
        r = ref.inflate_b(raw, cap)
        if r is None:
            crashes += 1
            continue
        assert (g, f, _digest(o)) == r, it
        compared += 1
        failed += g == 0
        partial += g == 0 and bool(f)
    assert compared > 800 and failed > 150 and partial > 100, (compared, failed, partial, crashes)
    assert crashes < 20, crashes
