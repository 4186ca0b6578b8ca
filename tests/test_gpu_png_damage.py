"""Damaged PNG files on the MI355X: the corpus of tests/png_damage.py (container, IHDR, per-chunk bit flips, damage under a
valid compression, zlib header and trailer, damage in the DEFLATE data) through every PNG call, both de-filter routes and
every inflate kernel width, against the two-armed expectation of that module -- tests/png_spec_ref.py wherever zlib accepts
the DEFLATE data, the CPU oracle of the shared inflate where it does not, the set of late statuses where neither applies."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_damage as D  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_device_out as DO  # noqa: E402

pytestmark = pytest.mark.gpu
E_LABEL = 15
PER_FAMILY = {"C": 520, "H": 300, "K": 187, "P": 130, "T": 250, "Z": 600}


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A

    return A


class World:
    """the thinned corpus and its expectations, computed once"""

    def __init__(self, oracle):
        full = D.corpus()
        exps = D.expectations(full, oracle)
        spliced = [c for c, e in zip(full, exps) if (c.family != "Z" and e.arm != "exact") or e.arm == "oversubscribed"]
        names = {c.name for c in D.thin(full, PER_FAMILY)} | {c.name for c in spliced}
        self.cases = [c for c in full if c.name in names]
        assert len(self.cases) <= 2100 and sum(e.arm == "oversubscribed" for e in exps) >= 50
        self.exps = D.expectations(self.cases, oracle)
        self.bases = D.base_files()
        self.base_px = [R.decode(b.data)[1] for b in self.bases]
        # the files that reach the inflate (no host status, no CRC error)
        self.reach = [(c, e) for c, e in zip(self.cases, self.exps) if not e.host and e.ref_status != R.E_CRC]

    def with_neighbours(self, cases, exps):
        """every seventh file an undamaged one -> (files, [(name, allowed, pixels)])"""
        files, want = [], []
        k = 0
        for c, e in zip(cases, exps):
            if len(files) % 7 == 6:
                b = k % len(self.bases)
                files.append(self.bases[b].data)
                want.append(("undamaged " + self.bases[b].name, frozenset((R.OK,)), self.base_px[b]))
                k += 1
            files.append(c.data)
            want.append((c.name, e.allowed, e.pixels))
        return files, want


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def _check(out, want, what):
    wrong = [(name, st, sorted(allowed)) for (st, _, _), (name, allowed, _) in zip(out, want) if st not in allowed]
    assert not wrong, (what, len(wrong), wrong[:10])
    for (st, px, _), (name, allowed, epx) in zip(out, want):
        if st == R.OK:
            assert epx is not None, (what, name)
            assert np.array_equal(px, epx), (what, name)


@pytest.mark.parametrize("general", [False, True], ids=["routed", "general"])
def test_every_family_both_routes(api, world, general):
    files, want = world.with_neighbours(world.cases, world.exps)
    assert {c.family for c in world.cases} == set(D.FAMILIES)
    _check(api.png_decode_batch(files, force_general=general), want, "one batch")


def test_every_family_one_file_per_call(api, world):
    files, want = world.with_neighbours(world.cases, world.exps)
    for k in range(0, len(files), 29):
        _check(api.png_decode_batch([files[k]]), [want[k]], "alone")
        _check(api.png_decode_batch([files[k]], force_general=True), [want[k]], "alone, general")


def _pool(world, n=200):
    """n files that all reach the inflate: the spliced C files first, then P, T and Z cases, an undamaged file at every seventh place"""
    cases = [c for c, e in world.reach if c.family == "C" and e.arm != "exact"][:6]
    cases += D.thin([c for c, _ in world.reach if c.family in "PTZ"], {"C": 0, "H": 0, "K": 0, "P": 50, "T": 50, "Z": 120}, seed=3)
    # two in three files of the largest base file left out: with them the largest quarter of the streams holds half of the input
    # bytes, and debig_plan_batch then launches 513..1024 streams 4 wide instead of 2 wide (test_every_inflate_width asserts it)
    big = [c for c in cases if " rgba8: " in c.name]
    cases = [c for c in cases if c not in big[1::3] and c not in big[2::3]]
    exps = [world.exps[world.cases.index(c)] for c in cases]
    files, want = world.with_neighbours(cases, exps)
    assert len(files) >= n and {name[0] for name, _, _ in want[:n]} >= set("CPTZu")
    return files[:n], want[:n]


# include/debig_hip.h, csrc/host/debig_ctx.h
WAVES_SPLIT, WAVES_STRAND, WAVES_STRAND_PIPE, WAVES_CHUNKED, WAVES_LARGE4_SMALL1 = 0x10, 0x12, 0x13, 0x20, 0x41
LARGE_IN_BYTES, LARGE_OUT_BYTES, CHUNKED_ROWS_MIN_IN_BYTES = 256 << 10, 1 << 20, 256 << 10


def _planned_width(files):
    """debig_plan_batch (csrc/host/debig_ctx.h) restated for a batch of PNG files that all reach the inflate: in_len is the
    IDAT concatenation without the zlib header, out_cap the scanline size, every stream carries DEBIG_STREAM_IMAGE_ROWS"""
    streams = [D.stream_of(f)[:2] for f in files]
    ins, caps, n = [len(z) - 2 for z, _ in streams], [scan for _, scan in streams], len(files)
    if n <= 1024:
        if sum(ins) >= n << 20 or (n <= 512 and min(ins) >= CHUNKED_ROWS_MIN_IN_BYTES):
            return WAVES_CHUNKED
    if n <= 256:
        return 8
    if n <= 768:
        if sum(ins) >= n * (128 << 10):
            return WAVES_STRAND_PIPE
        waves = 4 if n <= 512 else 2
    elif n <= 1024:
        waves = WAVES_STRAND_PIPE
    else:
        large = sum(i >= LARGE_IN_BYTES or c >= LARGE_OUT_BYTES for i, c in zip(ins, caps))
        if max(ins) >= 4 << 20 and n <= 16384:
            return WAVES_CHUNKED
        if 0 < large <= 256:
            return WAVES_LARGE4_SMALL1
        return WAVES_STRAND_PIPE if n <= 2048 else WAVES_STRAND if n <= 3072 else WAVES_SPLIT
    if 512 < n <= 1024 and 2 * sum(sorted(ins, reverse=True)[: n // 4]) >= sum(ins) > 0:
        return 4  # skewed sizes: launched 4-wide, longest first
    return waves


def _same(a, b, what):
    assert a[0] == b[0], what
    if a[0] == R.OK:
        assert np.array_equal(a[1], b[1]), what


def test_every_inflate_width(api, world):
    """The batch sizes are chosen against debig_pick_waves (csrc/host/debig_ctx.h) and the constants of include/debig_hip.h
    it reads; every file of the batch reaches the inflate, so the batch size is the stream count:
      200  <= 256: 8 wavefronts per stream;      400 <= 512: 4;      700 <= DEBIG_STRAND_MIN_STREAMS (768): 2;
      1500 <= DEBIG_STRAND_PIPE_MAX_STREAMS (2048): DEBIG_WAVES_STRAND_PIPE;
      2600 <= DEBIG_STRAND_MAX_STREAMS (3072): DEBIG_WAVES_STRAND;      3500: DEBIG_WAVES_SPLIT.
    Every batch repeats the 200 files of the first one and must give their statuses and pixels again."""
    files, want = _pool(world)
    assert len(files) == 200
    first = api.png_decode_batch(files)
    _check(first, want, "200 streams")
    assert len({st for st, _, _ in first}) >= 6
    assert _planned_width(files) == 8
    for n, width in ((400, 4), (700, 2), (1500, WAVES_STRAND_PIPE), (2600, WAVES_STRAND), (3500, WAVES_SPLIT)):
        batch = [files[i % 200] for i in range(n)]
        assert _planned_width(batch) == width, (n, hex(_planned_width(batch)))
        out = api.png_decode_batch(batch)
        for i, o in enumerate(out):
            _same(o, first[i % 200], ("%d streams" % n, want[i % 200][0]))


def _big_rgba(rng, w, h, noise):
    y, x = np.mgrid[0:h, 0:w]
    s = ((x[:, :, None] * 2 + y[:, :, None] * 3 + np.arange(4) * 9) // 4 % 256).astype(np.uint8)
    if noise:
        s = rng.integers(0, noise, size=s.shape, dtype=np.uint8)
    return s


def test_large_images_beside_many_small_files(api, world, oracle):
    """DEBIG_WAVES_LARGE4_SMALL1: more than 1024 streams of which 1..256 are large; the three images are large by
    DEBIG_LARGE_OUT_BYTES (include/debig_hip.h: out_cap = their scanline size >= 1 MiB), two of them damaged near the end"""
    rng = np.random.default_rng(11)
    s = _big_rgba(rng, 520, 520, 0)
    raw = R.scanlines(s, 6, 8, filters=0)
    assert len(raw) >= 1 << 20
    z = D.zwrap(raw, "dynamic")[0]
    good = R.encode(s, 6, 8, zdata=z)
    bad_data = D.Case("Z", "large, bit flipped near the end", R.encode(s, 6, 8, zdata=z[:-12] + bytes([z[-12] ^ 0x10]) + z[-11:]))
    bad_adler = D.Case("T", "large, Adler-32 byte", R.encode(s, 6, 8, zdata=z[:-1] + bytes([z[-1] ^ 1])))
    big = [(good, frozenset((R.OK,)), R.decode(good)[1])]
    for c in (bad_data, bad_adler):
        e = D.expectation(c, oracle)
        big.append((c.data, e.allowed, e.pixels))
    files, want = _pool(world)
    first = api.png_decode_batch(files)
    batch = [files[i % 200] for i in range(1500)]
    for k, (data, _, _) in enumerate(big):
        batch.insert(100 + 500 * k, data)
    assert _planned_width(batch) == WAVES_LARGE4_SMALL1
    out = api.png_decode_batch(batch)
    at = {100 + 500 * k for k in range(len(big))}
    small = [o for j, o in enumerate(out) if j not in at]
    assert len(small) == 1500 and len(out) == 1503
    for i, o in enumerate(small):
        _same(o, first[i % 200], ("beside large images", want[i % 200][0]))
    for k, (data, allowed, epx) in enumerate(big):
        st, px, _ = out[100 + 500 * k]
        assert st in allowed, (k, st)
        if st == R.OK:
            assert np.array_equal(px, epx), k


_LONG = []


def _long_files(oracle):
    """six files of one 512 x 512 RGBA8 image of noise (4wh = 1 MiB, about 790 KB of IDAT), five of them damaged ->
    (files, allowed statuses, the undamaged file, its index); made once"""
    if not _LONG:
        rng = np.random.default_rng(12)
        s = _big_rgba(rng, 512, 512, 64)
        z = D.zwrap(R.scanlines(s, 6, 8, filters=0), "dynamic")[0]
        flip = lambda k, m: z[:k] + bytes([z[k] ^ m]) + z[k + 1:]  # noqa: E731
        cases = [D.Case("Z", "long: first byte", R.encode(s, 6, 8, zdata=flip(2, 0x04))),
                 D.Case("Z", "long: middle", R.encode(s, 6, 8, zdata=flip(len(z) // 2, 0x20))),
                 D.Case("Z", "long: last block", R.encode(s, 6, 8, zdata=flip(len(z) - 40, 0x01))),
                 D.Case("Z", "long: truncated in the middle", R.encode(s, 6, 8, zdata=z[: len(z) // 2])),
                 D.Case("T", "long: Adler-32", R.encode(s, 6, 8, zdata=flip(len(z) - 2, 0x80)))]
        good = R.encode(s, 6, 8, zdata=z)
        files = [c.data for c in cases[:2]] + [good] + [c.data for c in cases[2:]]
        allowed = [D.expectation(c, oracle).allowed for c in cases]
        _LONG.append((files, allowed[:2] + [frozenset((R.OK,))] + allowed[2:], good, 2, R.decode(good)[1]))
    return _LONG[0]


@pytest.mark.parametrize("chunk_bytes", [None, "3072"])
def test_long_streams_as_chunk_tasks(api, oracle, monkeypatch, chunk_bytes):
    """DEBIG_WAVES_CHUNKED: at most 512 image-row streams, EVERY one at least DEBIG_CHUNKED_ROWS_MIN_IN_BYTES (256 KiB,
    csrc/host/debig_ctx.h) long -- the truncated one included; DEBIG_CHUNK_BYTES = 3072 cuts each into a few hundred tasks.
    Only the statuses of the damaged files need the reference; the undamaged file is compared with the general route and
    the reference."""
    files, allowed, good, at, good_px = _long_files(oracle)
    assert min(len(D.stream_of(f)[0]) - 2 for f in files) >= 256 << 10 and len(files) <= 8
    assert _planned_width(files) == WAVES_CHUNKED
    assert all(R.info(f)[1]["width"] * R.info(f)[1]["height"] * 4 <= 1 << 20 for f in files)
    if chunk_bytes is None:
        monkeypatch.delenv("DEBIG_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("DEBIG_CHUNK_BYTES", chunk_bytes)
    a = api.png_decode_batch(files)
    b = api.png_decode_batch(files, force_general=True)
    for k, ((sa, pa, _), (sb, pb, _), al) in enumerate(zip(a, b, allowed)):
        assert sa in al and sb == sa, (k, sa, sb, sorted(al))
    assert a[at][0] == R.OK and np.array_equal(a[at][1], b[at][1]) and np.array_equal(a[at][1], good_px)


# ------------------------------------------------------------------------------------------------ every call
def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _calls(api, n):
    """name -> (call(files) -> (statuses, per-file outputs or a dense array), dense fill or None, E_LABEL rule or None)"""
    size = (16, 16)
    warp = [[[0.9, 0.2, 0.5], [-0.2, 1.1, 1.0]]]
    color = api.png_color_matrix(brightness=1.2, contrast=0.8, saturation=1.3)
    labels_rule = lambda inf: inf["color_type"] in (2, 4, 6)  # noqa: E731
    color_rule = lambda inf: inf["bit_depth"] == 16  # noqa: E731

    def host(**kw):
        return lambda f: (lambda o: ([s for s, _, _ in o], [p for _, p, _ in o]))(api.png_decode_batch(f, **kw))

    def device(**kw):
        return lambda f: (lambda o: ([s for s, _, _ in o], [None if t is None else _np(t) for _, t, _ in o]))(
            api.png_decode_batch_device(f, **kw))

    def dense(fn, fill, **kw):
        def call(f):
            k = dict(kw)
            if "warp" in k:
                k["warp"] = warp * len(f)
            r = fn(f, size, fill=fill, **k)
            return r[0], _np(r[1])
        return call

    return {
        "png_decode_batch rgba8": (host(), None, None),
        "png_decode_batch rgb16": (host(mode="rgb", depth=16), None, None),
        "png_decode_batch native": (host(mode="native", depth="native"), None, None),
        "png_decode_batch_device hwc": (device(layout="hwc"), None, None),
        "png_decode_batch_device chw": (device(layout="chw", mode="rgb"), None, None),
        # (antialias off: with it a crop more than 64 times the output is E_BOX, one more rule decided at IHDR)
        "png_decode_batch_tensor": (dense(api.png_decode_batch_tensor, -7.0, antialias=False), -7.0, None),
        "png_decode_batch_tensor warp": (dense(api.png_decode_batch_tensor, -7.0, warp=True), -7.0, None),
        "png_decode_batch_tensor color": (dense(api.png_decode_batch_tensor, -7.0, color=color, antialias=False), -7.0, None),
        "png_decode_batch_tensor warp + color": (dense(api.png_decode_batch_tensor, -7.0, warp=True, color=color), -7.0, None),
        "png_decode_batch_labels": (dense(api.png_decode_batch_labels, -9), -9, labels_rule),
        "png_decode_batch_labels warp": (dense(api.png_decode_batch_labels, -9, warp=True), -9, labels_rule),
        "png_decode_batch_color_labels": (dense(api.png_decode_batch_color_labels, -9), -9, color_rule),
        "png_decode_batch_color_labels warp": (dense(api.png_decode_batch_color_labels, -9, warp=True), -9, color_rule),
        "apng_decode_batch": (lambda f: (lambda o: ([s for s, _, _ in o], [None if p is None else p[0] for _, p, _ in o]))(
            api.apng_decode_batch(f)), None, None),
    }


@pytest.fixture(scope="module")
def thin_batch(world):
    """at most 300 files of every family, the eight undamaged files among them at every 31st place"""
    cases = D.thin(world.cases, {"C": 70, "H": 60, "K": 30, "P": 40, "T": 40, "Z": 50}, seed=5)
    assert {c.family for c in cases} == set(D.FAMILIES)
    exps = [world.exps[world.cases.index(c)] for c in cases]
    files = [c.data for c in cases]
    allowed = [e.allowed for e in exps]
    at = []
    for b, base in enumerate(world.bases):
        at.append(31 * b + 5)
        files.insert(at[-1], base.data)
        allowed.insert(at[-1], frozenset((R.OK,)))
    assert len(files) <= 300
    return files, allowed, at


@pytest.mark.parametrize("name", ["png_decode_batch rgba8", "png_decode_batch rgb16", "png_decode_batch native",
                                  "png_decode_batch_device hwc", "png_decode_batch_device chw", "png_decode_batch_tensor",
                                  "png_decode_batch_tensor warp", "png_decode_batch_tensor color",
                                  "png_decode_batch_tensor warp + color", "png_decode_batch_labels",
                                  "png_decode_batch_labels warp", "png_decode_batch_color_labels",
                                  "png_decode_batch_color_labels warp", "apng_decode_batch"])
def test_every_call_gives_the_same_status(api, world, thin_batch, name):
    """one status per file whatever the call; a label call answers E_LABEL as soon as IHDR has been read (it outranks what
    comes later in the file), exactly there; a failed file's slot keeps `fill`; the undamaged files come out bit for bit as
    from the same call on a batch of undamaged files only"""
    files, allowed, at = thin_batch
    call, fill, rule = _calls(api, len(files))[name]
    ref_st = [s for s, _, _ in api.png_decode_batch(files)]
    assert all(s in al for s, al in zip(ref_st, allowed))
    st, out = call(files)
    clean_st, clean = call([b.data for b in world.bases])
    want = list(ref_st)
    if rule is not None:
        for i, f in enumerate(files):
            inf = R.info(f)[1]
            if inf["width"] and rule(inf):
                want[i] = E_LABEL
        assert 20 <= want.count(E_LABEL) <= len(want) - 20
    assert st == want, [(i, a, b) for i, (a, b) in enumerate(zip(st, want)) if a != b][:10]
    for i in range(len(files)):
        if st[i] != R.OK:
            if fill is not None:
                assert (out[i] == fill).all(), (name, i)
            else:
                assert out[i] is None
    for b, i in enumerate(at):
        assert st[i] == clean_st[b]
        if st[i] == R.OK:
            assert out[i].dtype == clean[b].dtype and np.array_equal(out[i], clean[b]), (name, world.bases[b].name)
    assert sum(s == R.OK for s in clean_st) >= 2


# ------------------------------------------------------------------------------------------------ own regions
@pytest.mark.parametrize("layout,mode,depth", [("hwc", "rgba", 8), ("chw", "rgb", 8), ("hwc", "rgba", 16)])
def test_nothing_outside_a_files_own_region(api, world, layout, mode, depth):
    """P, T and Z files in the raw device arena with 0xA5 gaps: a file that fails before the de-filter leaves its region
    untouched, E_FILTER / E_PALETTE files write inside their own region only, no gap is written"""
    fmt = api.png_out_format(mode, depth)
    picked = [(c, e) for c, e in world.reach if c.family in "PTZ"]
    cases = D.thin([c for c, _ in picked], {"C": 0, "H": 0, "K": 0, "P": 130, "T": 60, "Z": 150}, seed=9)
    allowed = [world.exps[world.cases.index(c)].allowed for c in cases]
    datas = [c.data for c in cases]
    st, a, offs, exact = DO._raw_dev(api, datas, fmt, layout, gaps=[0, 16, 48, 4096])
    assert all(s in al for s, al in zip(st, allowed)), [(c.name, s) for c, s, al in zip(cases, st, allowed) if s not in al][:10]
    assert {R.E_FILTER, R.E_PALETTE, R.E_ADLER, R.E_DATA_SHORT, R.E_DATA_LONG, R.OK} <= set(st)
    written = [s in (R.OK, R.E_FILTER, R.E_PALETTE) for s in st]
    DO._assert_outside_untouched(a, offs, exact, written)
    ok = [i for i, s in enumerate(st) if s == R.OK]
    host = api.png_decode_batch([datas[i] for i in ok], mode=mode, depth=depth, layout=layout)
    for i, (hs, hpx, _) in zip(ok, host):
        assert hs == R.OK and a[offs[i]: offs[i] + exact[i]].tobytes() == hpx.tobytes(), cases[i].name
