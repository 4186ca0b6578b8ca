"""The damaged-file corpus of tests/png_damage.py without a GPU: the corpus itself (sizes, block types, the share of the
weak arm), every status debig_png_decode_batch decides on the host against tests/png_spec_ref.py, debig_png_info_get on
every file of every family, IHDR sizes up to 2^31 through the raw call, and the APNG container sweep through the host-only
walk against tests/apng_ref.py."""
import collections
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_damage as D  # noqa: E402
import png_spec_ref as R  # noqa: E402
from test_png_spec_cpu import PngInfo, _host_status, lib  # noqa: E402,F401  (lib: the fixture)

INFO_KEYS = ("width", "height", "bit_depth", "color_type", "interlace", "has_trns")
WEAK_CAP = 0.15  # of all Z cases


@pytest.fixture(scope="module")
def corpus():
    return D.corpus()


@pytest.fixture(scope="module")
def expects(corpus, oracle):
    return D.expectations(corpus, oracle)


def test_base_files(oracle):
    bases = D.base_files()
    kinds = collections.Counter()
    loose = []
    for b in bases:
        st, px, inf = R.decode(b.data)
        assert st == R.OK and px.shape == (b.h, b.w, 4), b.name
        assert 7 <= b.w <= 70 and 7 <= b.h <= 70
        sizes = [ln for _, ln, t in D.spans(b.data) if t == b"IDAT"]
        assert len(sizes) >= 2 and 0 in sizes, b.name  # several IDAT chunks, one of them empty
        good, final, out, stats = oracle.inflate(b.z[2:], max(b.scan, len(b.z)), want_stats=True)
        assert good and out == b.raw and stats.ub_flags == 0
        kinds.update(stored=stats.n_stored, fixed=stats.n_fixed, dynamic=stats.n_dynamic)
        if not b.scan >= len(b.z) - 2 >= 5:
            loose.append(b.name)
    assert loose == ["rgb8key"]  # the one stored-block file with scan < z_total, kept on purpose
    assert kinds["stored"] and kinds["fixed"] and kinds["dynamic"]
    assert {(b.ct, b.depth, b.il) for b in bases} >= {(6, 8, 0), (2, 8, 0), (3, 4, 1), (0, 16, 1), (0, 1, 0), (4, 8, 0), (6, 16, 0)}


def test_corpus_counts_and_weak_arm_share(corpus, expects):
    """prints the per-family, per-status counts (pytest -s shows them; DESIGN.md records them) and holds the weak arm to
    at most 15 % of all Z cases"""
    assert len({c.name for c in corpus}) == len(corpus)
    assert D.corpus() == corpus  # deterministic
    table, arms = collections.Counter(), collections.Counter()
    for c, e in zip(corpus, expects):
        key = "/".join(str(s) for s in sorted(e.allowed)) if e.arm != "weak" else "late"
        table[(c.family, key)] += 1
        arms[(c.family, e.arm)] += 1
    for fam in D.FAMILIES:
        n = sum(v for (f, _), v in table.items() if f == fam)
        print("family %s: %5d cases; status -> count: %s; arms: %s" % (
            fam, n, ", ".join("%s: %d" % (k, v) for (f, k), v in sorted(table.items()) if f == fam),
            ", ".join("%s %d" % (a, v) for (f, a), v in sorted(arms.items()) if f == fam)))
        assert n >= 100
    nz = sum(v for (f, _), v in arms.items() if f == "Z")
    weak = arms[("Z", "weak")] + arms[("Z", "oversubscribed")]  # (the second: outside the oracle's domain too, but decided by the kernels' Kraft check)
    assert arms[("Z", "oversubscribed")] <= nz // 40
    print("weak arm: %d of %d Z cases = %.1f %%" % (weak, nz, 100.0 * weak / nz))
    assert weak <= WEAK_CAP * nz
    assert arms[("Z", "oracle")] >= 100 and arms[("Z", "exact")] >= 1000
    # outside Z the reference decoder decides, except for the few files whose IDAT concatenation is cut short or spliced
    other = [c.name for c, e in zip(corpus, expects) if c.family != "Z" and e.arm != "exact"]
    assert len(other) <= 40 and all(("IDAT@" in n and n.split()[-1] in ("dropped", "doubled", "swapped")) or
                                    n.endswith("zlib header only") for n in other), other
    # every status of the header occurs as an exact expectation
    seen = {next(iter(e.allowed)) for e in expects if e.arm == "exact"}
    assert seen >= set(range(0, 12)) - {R.E_INFLATE}
    assert any(e.allowed == {R.E_INFLATE, R.E_DATA_LONG} for e in expects)


def test_every_file_is_small_enough_for_the_wrappers(corpus):
    """the Python wrappers size their buffers from IHDR: w, h <= 4096 and 4wh <= 1 MiB wherever IHDR is valid"""
    for c in corpus:
        inf = R.info(c.data)[1]
        assert inf["width"] <= 4096 and inf["height"] <= 4096 and 4 * inf["width"] * inf["height"] <= 1 << 20, c.name


def test_host_decided_statuses(lib, corpus, expects):
    host = [(c, e) for c, e in zip(corpus, expects) if e.host]
    assert len(host) >= 1200 and {c.family for c, _ in host} >= set("CHKT")
    got = _host_status(lib, [c.data for c, _ in host])
    wrong = [(c.name, g, e.ref_status) for (c, e), g in zip(host, got) if g != e.ref_status]
    assert not wrong, (len(wrong), wrong[:10])
    # one file per call, a thinned subset
    for c, e in host[::23]:
        assert _host_status(lib, [c.data]) == [e.ref_status], c.name


def test_info_get_on_every_file(lib, corpus):
    wrong = []
    for c in corpus:
        est, einf = R.info(c.data)
        inf = PngInfo()
        st = lib.debig_png_info_get(c.data, len(c.data), C.byref(inf))
        got = {k: int(getattr(inf, k)) for k in INFO_KEYS}
        if st != est or got != {k: einf[k] for k in INFO_KEYS}:
            wrong.append((c.name, st, est, got, einf))
    assert not wrong, (len(wrong), wrong[:5])


def test_huge_ihdr_sizes_through_the_raw_call(lib):
    cases = D.huge_ihdr_cases()
    want = [R.decode(d, out_cap=cap)[0] for _, d, cap in cases]
    assert set(want) == {R.E_OUTPUT, R.E_IHDR}
    got = _host_status(lib, [d for _, d, _ in cases], caps=[cap for _, _, cap in cases])
    assert got == want, [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w]
    for (name, d, _), w in zip(cases, want):
        inf = PngInfo()
        est, einf = R.info(d)
        assert lib.debig_png_info_get(d, len(d), C.byref(inf)) == est == (R.E_IHDR if w == R.E_IHDR else R.OK), name
        assert (inf.width, inf.height) == (einf["width"], einf["height"]), name


def test_ihdr_rewrites_with_a_stale_crc_follow_the_order(lib, corpus, expects):
    """E_IHDR comes from the chunk walk, so it outranks everything later; a legal rewrite with the old CRC is E_CRC, but
    E_OUTPUT comes before the CRC: with out_caps of 0 the library must answer E_OUTPUT there, on the host, and the walk's own
    status everywhere else"""
    kept = [(c, e) for c, e in zip(corpus, expects) if c.family == "H" and c.name.endswith("CRC kept")]
    assert len(kept) >= 300
    assert {e.ref_status for _, e in kept} <= {R.E_IHDR, R.E_CRC, R.E_CHUNK}
    assert sum(e.ref_status == R.E_CRC for _, e in kept) >= 50
    want = [R.decode(c.data, out_cap=0)[0] for c, _ in kept]
    assert want == [e.ref_status if e.host else R.E_OUTPUT for _, e in kept]
    got = _host_status(lib, [c.data for c, _ in kept], caps=[0] * len(kept))
    assert got == want, [(c.name, g, w) for (c, _), g, w in zip(kept, got, want) if g != w][:10]
    # the same with the CRC mended, and every other H file: E_OUTPUT wherever the reference gets that far
    rest = [c for c in corpus if c.family == "H" and not c.name.endswith("CRC kept")]
    want = [R.decode(c.data, out_cap=0)[0] for c in rest]
    assert R.E_OUTPUT in want and R.E_IHDR in want
    got = _host_status(lib, [c.data for c in rest], caps=[0] * len(rest))
    assert got == want, [(c.name, g, w) for c, g, w in zip(rest, got, want) if g != w][:10]


def test_apng_container_sweep(lib):
    from debigulator_amd import api as A

    files = D.apng_corpus()
    assert len(files) >= 1000
    seen = collections.Counter()
    wrong = []
    for name, data in files:
        est, einf = D.apng_walk_ref(data)
        st, inf = A.apng_info(data)
        seen[est] += 1
        if st != est:
            wrong.append((name, st, est))
        elif st == R.OK and inf != einf:
            wrong.append((name, inf, einf))
    assert not wrong, (len(wrong), wrong[:8])
    print("APNG sweep: status -> count: %s" % dict(sorted(seen.items())))
    assert seen[R.OK] >= 5 and seen[13] >= 40 and seen[R.E_CHUNK] >= 600
