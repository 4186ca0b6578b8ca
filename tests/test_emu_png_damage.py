"""CPU: the inflate kernels on the lock-step emulator (tools/simt_emu) with exactly what debig_png_decode_batch hands them
for a damaged file -- DEBIG_STREAM_NO_REF_GATES, out_cap == the scanline size, the Adler-32 trailer (and whatever follows it)
inside in_len -- at every kernel width.  The result is mapped to a PNG status as csrc/host/debig_png_spec.c maps it (the
loop after debig_launch_inflate_planned) and held against the two-armed expectation of tests/png_damage.py; every width must
agree with every other one on every file, the files of the weak arm included.  That includes the 64 Z cases
whose bit flip makes a code-length set over-subscribed: without the Kraft check in build_code (csrc/inflate_kernel.inc) 7 of
them ended in E_INFLATE at one width and in E_DATA_SHORT / E_DATA_LONG at another, and one decoded to DEBIG_PNG_OK; all 64
run here, at every width, and must be E_INFLATE."""
import struct
import zlib

import pytest

import emu_binding as eb
import png_damage as D
import png_spec_ref as R

E_OUTPUT_FULL = 8  # include/debig_hip.h: DEBIG_E_OUTPUT_FULL
NO_REF_GATES = 1   # include/debig_hip.h: DEBIG_STREAM_NO_REF_GATES
WIDTHS = [1, 4, eb.SPLIT, eb.STRAND, eb.STRAND_PIPE, eb.CHUNKED]
PER_FAMILY = {"C": 0, "H": 10, "K": 0, "P": 30, "T": 30, "Z": 0}  # + every spliced C / T file, and of Z:
PER_ARM = {"exact": 30, "oracle": 50, "weak": 24, "oversubscribed": 64}  # (all 64 over-subscribed files)


@pytest.fixture(scope="module")
def emu():
    return eb.load_emu()


@pytest.fixture(scope="module")
def work(oracle):
    """the files that reach the inflate: [(case, expectation, IDAT concatenation, scan, info, palette, key)]"""
    cases = D.corpus()
    exps = D.expectations(cases, oracle)
    reach = [(c, e) for c, e in zip(cases, exps) if not e.host and e.ref_status != R.E_CRC]
    spliced = [(c, e) for c, e in reach if c.family != "Z" and e.arm != "exact"]  # every file of the other families zlib rejects
    keep = {c.name for c in D.thin([c for c, _ in reach], PER_FAMILY)} | {c.name for c, _ in spliced}
    for arm, n in PER_ARM.items():
        keep |= {c.name for c in D.thin([c for c, e in reach if c.family == "Z" and e.arm == arm], n)}
    out = []
    for c, e in reach:
        if c.name in keep:
            out.append((c, e) + D.stream_of(c.data))
    assert {c.family for c, *_ in out} >= set("CHPTZ") and len(out) <= 340
    assert all(sum(e.arm == arm for _, e, *_ in out) >= n for arm, n in PER_ARM.items())
    return out


def png_status(z, scan, good, status, final_size, in_end_bits, out, inf, pal, key):
    """csrc/host/debig_png_spec.c, after the inflate launch: good / status / final_size / in_end_bits -> DEBIG_PNG_*"""
    if not good:
        return R.E_DATA_LONG if status == E_OUTPUT_FULL else R.E_INFLATE
    if final_size < scan:
        return R.E_DATA_SHORT
    t = 2 + (in_end_bits + 7) // 8
    if t + 4 > len(z):
        return R.E_ADLER
    if struct.unpack(">I", z[t: t + 4])[0] != zlib.adler32(out) & 0xFFFFFFFF:
        return R.E_ADLER
    return R.pixels(out, inf, pal, key)[0]


_RUNS = {}


def _run(emu, work, nw):
    if nw not in _RUNS:
        raws = [z[2:] for _, _, z, *_ in work]
        caps = [scan for _, _, _, scan, *_ in work]
        outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, flags=NO_REF_GATES, chunk_bytes=256, out_misalign=3)
        res = []
        for (c, e, z, scan, inf, pal, key), (good, final, _, r), (_, oo), cap in zip(work, outs, offs, caps):
            assert (arena[oo + cap: oo + cap + 64] == 0xA5).all(), (c.name, "the guard behind out_cap was written")
            out = arena[oo: oo + scan].tobytes()
            res.append(png_status(z, scan, r.good, r.status, r.final_size, r.in_end_bits, out, inf, pal, key))
        _RUNS[nw] = res
    return _RUNS[nw]


@pytest.mark.parametrize("nw", WIDTHS)
def test_mapped_status_follows_the_expectation(emu, work, nw):
    got = _run(emu, work, nw)
    wrong = [(c.name, g, sorted(e.allowed), e.arm) for (c, e, *_), g in zip(work, got) if g not in e.allowed]
    assert not wrong, (len(wrong), wrong[:12])


def test_every_width_agrees_with_every_other(emu, work):
    first = _run(emu, work, WIDTHS[0])
    for nw in WIDTHS[1:]:
        got = _run(emu, work, nw)
        diff = [(c.name, a, b, e.arm) for (c, e, *_), a, b in zip(work, first, got) if a != b]
        assert not diff, (hex(nw), len(diff), diff[:12])
