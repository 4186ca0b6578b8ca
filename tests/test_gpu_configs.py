"""GPU: the other BASELINE.json configs as parity cases (config 2 is tests/test_gpu_inflate.py
and bench.py): config 3 = 1024 PNGs cycled from the reference's 15 sample files, config 4
shape = large all-Paeth RGBA PNGs (scaled down so the oracle finishes in seconds, plus a
size-independent property at a larger size), config 5 shape = gzip members of 1 MiB."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from debigulator_amd import workload

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def test_cfg3_1024_pngs_resident(gpu_device):
    from debigulator_amd.png_device import DevicePngBatch

    gold = json.load(open(os.path.join(GOLD, "resources.json")))["png"]
    files = [f for f in sorted(glob.glob(os.path.join(GOLD, "resources", "*.png")))
             if not f.endswith("backgrounddetailed1.png")]  # ct 2: reference output is the P3 artefact
    datas = [open(f, "rb").read() for f in files]
    pngs = [datas[i % len(datas)] for i in range(1024)]
    b = DevicePngBatch(pngs, device=gpu_device)
    b.launch()
    res, ires = b.results()
    assert (res["good"] == 1).all() and (ires["good"] == 1).all()
    for i in list(range(0, 28)) + list(range(1000, 1024)):
        name = os.path.basename(files[i % len(files)])
        assert sha(b.rgba(i).tobytes()) == gold[name]["rgba_sha256"], (i, name)


@pytest.mark.parametrize("noise", [workload.CFG4_NOISE, 24], ids=["ratio3", "ratio1.4"])
def test_cfg4_shape_paeth_rgba(gpu_device, oracle, noise):
    """all rows Paeth, RGBA, dynamic Huffman, 64 KiB IDAT chunks; 4 distinct seeds of 512x512 vs
    the oracle byte for byte.  noise = CFG4_NOISE is BASELINE config 4's data (scanline stream /
    compressed about 3:1, asserted); 24 is the noisier round-1 data (1.4:1), kept as a second case."""
    from debigulator_amd.png_device import DevicePngBatch

    pngs, pix = [], []
    for s in range(4):
        p, x = workload.make_png(7000 + s, 512, 512, ct=6, ftype=4, noise=noise, enc="dynamic", idat_chunk=65536)
        pngs.append(p)
        pix.append(x)
        if noise == workload.CFG4_NOISE:
            assert 2.8 < 512 * (512 * 4 + 1) / len(p) < 3.2
    b = DevicePngBatch(pngs, device=gpu_device)
    b.launch()
    res, ires = b.results()
    assert (res["good"] == 1).all() and (ires["good"] == 1).all()
    for i in range(4):
        good, want = oracle.decode_png(pngs[i])
        assert good == 1
        got = b.rgba(i)
        assert np.array_equal(got, want)
        # the generator's own pixels (round trip: filter -> deflate -> inflate -> de-filter)
        assert np.array_equal(got.reshape(512, 2048), pix[i])


def test_cfg4_roundtrip_property_large(gpu_device):
    """size-independent property at 2048x2048 (16 MiB of RGBA per image): de-filter(inflate(
    deflate(filter(pixels)))) == pixels"""
    from debigulator_amd.png_device import DevicePngBatch

    p, x = workload.make_png(7100, 2048, 2048, ct=6, ftype=4, noise=workload.CFG4_NOISE, enc="dynamic", idat_chunk=65536)
    assert 2.8 < 2048 * (2048 * 4 + 1) / len(p) < 3.2  # BASELINE config 4: ratio about 3:1
    b = DevicePngBatch([p, p], device=gpu_device)
    b.launch()
    res, ires = b.results()
    assert (res["good"] == 1).all() and (ires["good"] == 1).all()
    assert int(res[0]["final_size"]) == 2048 * (2048 * 4 + 1)
    assert np.array_equal(b.rgba(1).reshape(2048, 8192), x)


def test_cfg4_one_full_size_image(gpu_device):
    """BASELINE config 4 at its real size: ONE 8192 x 8192 RGBA image, every row Paeth, ratio about 3:1
    (a 268 MB scanline stream: several hundred chunk tasks, offsets beyond 2^28 inside one recipient,
    8192-pixel rows in the de-filter).  Property (the oracle needs minutes here): the decoded pixels
    are the generator's, through the path the library picks for the batch (chunk tasks)."""
    from debigulator_amd.png_device import DevicePngBatch

    side = 8192
    png, pix = workload.make_png(9001, side, side, ct=6, ftype=4, noise=workload.CFG4_NOISE, enc="dynamic",
                                 idat_chunk=65536)
    assert 2.8 < side * (side * 4 + 1) / len(png) < 3.2
    b = DevicePngBatch([png], device=gpu_device)
    b.launch()
    res, ires = b.results()
    assert (res["good"] == 1).all() and (ires["good"] == 1).all()
    assert int(res[0]["final_size"]) == side * (side * 4 + 1)
    assert np.array_equal(b.rgba(0).reshape(side, side * 4), np.asarray(pix).reshape(side, side * 4))


@pytest.mark.parametrize("n", [5, 40, 100])
def test_defilter_several_workgroups_per_image(gpu_device, oracle, n):
    """Few images: the de-filter spreads one image over several workgroups (csrc/png_kernel.inc, MWG:
    8 x 4 wavefronts per image up to 32 images, 4 x 4 up to 64, 2 x 8 up to 128), bands handed from CU to
    CU through memory.  Odd widths (cache lines of the handed-over row straddle the groups), every
    filter type, RGB and palette images, up to 333 rows: at most 6 bands over 64, 32 or 16 slots, so NO slot
    takes a second band here (the wrap of the band ring is tests/test_gpu_png_defilter_battery.py's) -- against
    the oracle; one image with a filter byte > 4 fails alone (the failure flag is global)."""
    from debigulator_amd.png_device import DevicePngBatch

    rng = np.random.default_rng(n)
    shapes = [(97, 333, 6), (501, 260, 6), (64, 200, 2), (333, 140, 3), (1030, 70, 6)]
    pngs, want = [], []
    for i in range(n):
        w, h, ct = shapes[i % len(shapes)]
        pal = rng.integers(0, 256, 768, dtype=np.uint8) if ct == 3 else None
        png, pix = workload.make_png(500 + i, w, h, ct=ct, ftype=(5, 4, 3, 1, 2)[i % 5], noise=6, enc="dynamic", palette=pal)
        pngs.append(png)
        if ct == 2:  # the device batch class gives the spec-conforming RGBA image (the reference's RGB bug replay is
            rgba = np.full((h, w, 4), 255, dtype=np.uint8)  # another kernel): the generator's pixels + alpha 255
            rgba[:, :, :3] = np.asarray(pix).reshape(h, w, 3)
            want.append((1, rgba.reshape(-1)))
        else:
            want.append(oracle.decode_png(png))
    b = DevicePngBatch(pngs, device=gpu_device)
    b.launch()
    res, ires = b.results()
    assert (res["good"] == 1).all() and (ires["good"] == 1).all()
    for i in range(n):
        g, px = want[i]
        assert g == 1
        assert np.array_equal(b.rgba(i).reshape(-1), np.asarray(px).reshape(-1)), i
    # a filter byte > 4 in the middle of image 1 (second band's wavefront finds it): that image fails, the others do not
    st = b.inflate
    off = int(st.streams_host[1]["out_off"])
    w1, h1, _ = shapes[1]
    row = 100
    b.launch_inflate_only()
    st.d_out[off + row * (4 * w1 + 1)] = 9
    b.launch_defilter_only()
    _, ires = b.results()
    assert ires[1]["good"] == 0 and int(ires[1]["bad_row"]) == row
    assert all(ires[i]["good"] == 1 for i in range(n) if i != 1)


def test_defilter_workgroups_not_resident_together_fall_back(gpu_device, oracle):
    """The several-workgroups-per-image de-filter when its residency assumption does NOT hold: 64 images x 8
    workgroups of 4 wavefronts (87 KB of LDS each: one per CU) are twice what the device holds at once
    (DEBIG_DEFILTER_WGS / DEBIG_DEFILTER_RESIDENT force the shape past the shim's own limit).  Workgroups that
    wait in vain give their image up as REDO within tens of milliseconds and the one-workgroup pass of the same
    call decodes those images: every image comes back good and with the oracle's pixels -- a valid PNG never
    turns into good = 0 (src/decode_png.c:1430-1507).  In a child process: the shape overrides are read once."""
    import subprocess
    import sys

    code = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
from debigulator_amd import workload
from debigulator_amd.png_device import DevicePngBatch
from oracle.binding import Oracle
oracle = Oracle()
n = 64
pngs, want = [], []
for i in range(n):
    w, h = ((97, 900), (260, 700), (64, 1300), (130, 520))[i %% 4]
    png, pix = workload.make_png(900 + i, w, h, ct=6, ftype=(5, 4, 3, 1, 2)[i %% 5], noise=6, enc="dynamic")
    pngs.append(png)
    if i < 8: want.append(oracle.decode_png(png))
b = DevicePngBatch(pngs, device=%(dev)r)
b.launch()
res, ires = b.results()
assert (res["good"] == 1).all(), "inflate"
assert (ires["good"] == 1).all(), [(i, int(ires[i]["bad_row"])) for i in range(n) if ires[i]["good"] != 1][:5]
for i in range(8):
    g, px = want[i]
    assert g == 1 and np.array_equal(b.rgba(i).reshape(-1), np.asarray(px).reshape(-1)), i
print("fallback ok")
""" % {"root": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dev": gpu_device}
    env = dict(os.environ, DEBIG_DEFILTER_WGS="8", DEBIG_DEFILTER_RESIDENT="1000000")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fallback ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_cfg5_shape_gzip_members(gpu_device, oracle):
    """gzip members of 1 MiB (text-like, dynamic Huffman, EOB >= 8 bits so the tail rule never
    truncates): header located on the host, payloads inflated in one launch."""
    from debigulator_amd.batch import DeviceBatch

    members, plains, raws, caps = [], [], [], []
    for i in range(48):
        plain = workload.payload("text", workload.SEED0 + 100000 + i, 1 << 20)
        raw = workload.encode("dynamic", plain)
        gz = workload.gzip_member(raw, plain)
        ok, off, ln = oracle.gz_locate(gz)
        assert ok and gz[off:off + ln] == raw
        members.append(gz)
        plains.append(plain)
        raws.append(gz[off:off + ln])
        caps.append((1 << 20) + 1)
    b = DeviceBatch.from_streams(raws, caps, device=gpu_device)
    b.launch()
    res = b.results()
    assert (res["good"] == 1).all() and (res["final_size"] == (1 << 20)).all()
    host = b.outputs_host()
    import zlib

    for i in range(48):
        off = int(b.streams_host[i]["out_off"])
        got = host[off:off + (1 << 20)]
        assert np.array_equal(got, plains[i])
        # trailer: CRC32 + ISIZE of the member (the reference never checks them; we can)
        crc, isz = np.frombuffer(members[i][-8:], dtype="<u4")
        assert zlib.crc32(got.tobytes()) == crc and isz == (1 << 20)
    # and three of them through the oracle, byte for byte
    for i in (0, 17, 47):
        good, out, n = oracle.decode_gz(members[i], (1 << 20) + 16)
        assert good == 1 and out == plains[i].tobytes()


def test_drop_in_decode_gz_batch(gpu_device):
    from debigulator_amd import api

    plain = workload.payload("text", 99, 300000)
    gz = workload.gzip_member(workload.encode("dynamic", plain), plain)
    good, out = api.decode_gz(gz)
    assert good == 1 and out == plain.tobytes()


def test_decode_png_pipelined_groups_and_lanes(gpu_device, oracle, monkeypatch):
    """DevicePngBatch.launch_pipelined (opt-in: DEBIG_PNG_PIPELINE=1): the inflate in groups of images through chunk tasks
    on one and on two lanes (a workspace each), every group's de-filter on a side stream behind it -- against the oracle's
    decode_png, image for image, results in the caller's order."""
    import random

    from debigulator_amd.png_device import DevicePngBatch

    rng = random.Random(7)
    pngs = []
    for it in range(21):
        w, h = rng.randint(60, 420), rng.randint(40, 300)
        pngs.append(workload.make_png(8300 + it, w, h, ct=rng.choice([6, 6, 3]), ftype=rng.choice([1, 2, 3, 4, 5]),
                                      noise=rng.choice([3, 24, workload.CFG4_NOISE]), enc="dynamic", idat_chunk=65536)[0])
    monkeypatch.setenv("DEBIG_CHUNK_BYTES", "2048")
    b = DevicePngBatch(pngs, device=gpu_device)
    want = [oracle.decode_png(p) for p in pngs]
    for group, lanes in ((21, 1), (5, 1), (4, 2), (2, 3)):
        b.d_rgba.zero_()
        b.launch_pipelined(group_images=group, lanes=lanes)
        assert len(b.inflate.chunk_groups) == -(-21 // group)
        res, ires = b.results()
        for i, (good, px) in enumerate(want):
            assert int(ires[i]["good"] and res[i]["good"]) == good == 1, (group, lanes, i)
            assert np.array_equal(b.rgba(i), px), (group, lanes, i)
    monkeypatch.delenv("DEBIG_CHUNK_BYTES", raising=False)


def test_decode_png_in_chunk_tasks_with_the_aliasing_replay(gpu_device, oracle, monkeypatch):
    """decode_png's inflate forced through chunk tasks of 1 and 2 KiB (DEBIG_WAVES_PER_STREAM = 0x20,
    DEBIG_CHUNK_BYTES): RGBA and palette images of odd sizes, every filter type, several noise
    levels -- the reference's buffer-aliasing replay (P2: the last 772 bytes of the scanline stream)
    then falls into the last task's planes, on a task boundary, or hands the stream back.  Every
    image must equal the oracle's decode_png, and the reference's sample files their digests."""
    import random

    from debigulator_amd.png_device import DevicePngBatch

    rng = random.Random(99)
    pngs = []
    for it in range(48):
        ct = rng.choice([6, 6, 6, 3])
        w, h = rng.randint(20, 420), rng.randint(20, 300)
        p, _ = workload.make_png(8100 + it, w, h, ct=ct, ftype=rng.choice([0, 1, 2, 3, 4, 5]),
                                 noise=rng.choice([1, 3, 8, 24, workload.CFG4_NOISE]), enc="dynamic",
                                 idat_chunk=rng.choice([8192, 65536]))
        pngs.append(p)
    gold = json.load(open(os.path.join(GOLD, "resources.json")))["png"]
    files = [f for f in sorted(glob.glob(os.path.join(GOLD, "resources", "*.png")))
             if not f.endswith("backgrounddetailed1.png")]
    monkeypatch.setenv("DEBIG_WAVES_PER_STREAM", "0x20")
    for chunk in ("1024", "2048"):
        monkeypatch.setenv("DEBIG_CHUNK_BYTES", chunk)
        b = DevicePngBatch(pngs + [open(f, "rb").read() for f in files], device=gpu_device)
        b.launch()
        res, ires = b.results()
        for i, p in enumerate(pngs):
            good, want = oracle.decode_png(p)
            assert int(ires[i]["good"] and res[i]["good"]) == good, (chunk, i)
            if good:
                assert np.array_equal(b.rgba(i), want), (chunk, i)
        for k, f in enumerate(files):
            assert sha(b.rgba(len(pngs) + k).tobytes()) == gold[os.path.basename(f)]["rgba_sha256"], (chunk, f)
    monkeypatch.delenv("DEBIG_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("DEBIG_WAVES_PER_STREAM", raising=False)
