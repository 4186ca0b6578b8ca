"""GPU parity on streams whose Huffman tables have a chosen shape (tests/table_shapes.py), every kernel width, against
the oracle and the reference-made tests/golden/corpus_tables.json: ladders of every code length with the 48-bit token at
every phase of a byte, second-level runs of every size, the 256-entry second-level area filled exactly and overflowed
(the canonical probe), sequences of blocks whose tables differ in every way, incomplete codes and codes outside the
reference's probe range (Q7), and four probe groups at every bit offset of two scan segments and across a window edge.
tests/test_table_shapes_cpu.py proves, with a model of the tables, that the streams reach those routes."""
import json
import os

import numpy as np
import pytest

import handback_corpus as hc
import png_spec_ref as R
import table_shapes as ts
from debigulator_amd.batch import DeviceBatch
from test_gpu_inflate import WIDTHS, _check
from test_gpu_inflate_tokens import _check_wide_guard

pytestmark = pytest.mark.gpu

ORC_UB_LONGCODE_500 = 0x40
_EXP = {}


def _family(oracle, name):
    """the cases of one family; the generator's condition (the reference has a defined answer to every one of them -- the
    named Q8 case through its build without asserts --, none is skipped, the plain-Python decode of the token list says
    the same) is asserted here, once per family"""
    if name not in _EXP:
        cs = ts.families()[name]
        for c in cs:
            g, f, out, st = oracle.inflate(c.raw, c.cap, want_stats=True)
            assert st.ub_flags == (ORC_UB_LONGCODE_500 if c.name == ts.Q8_CASE else 0), c
            assert (g, f, out) == (int(c.legal), len(c.plain), c.plain), c
        _EXP[name] = cs
    return _EXP[name]


def _run(oracle, gpu_device, cs, **kw):
    _check(oracle, gpu_device, [c.raw for c in cs], [c.cap for c in cs], **kw)


def test_all_eleven_widths_are_mapped_to_a_geometry():
    assert len(WIDTHS) == 11 and set(WIDTHS) == set(ts.WIDTH_GEOMETRY)


@pytest.mark.parametrize("fam,in_skew,out_skew", [("T1", 5, 3), ("T2", 1, 15), ("T3", 7, 13), ("T4", 3, 9), ("T5", 11, 1)])
def test_table_families_every_width(oracle, gpu_device, fam, in_skew, out_skew):
    _run(oracle, gpu_device, _family(oracle, fam), in_skew=in_skew, out_skew=out_skew)


@pytest.mark.parametrize("part", [0, 1, 2])
def test_positions_every_width(oracle, gpu_device, part):
    """T6: every bit offset of two scan segments, the window edge and the long arm, a third of the streams per case"""
    _run(oracle, gpu_device, _family(oracle, "T6")[part::3], in_skew=2 + part, out_skew=11 - part)


def test_tables_corpus_reference_made(gpu_device):
    """every width against the compiled reference's own answers (tests/golden/corpus_tables.json), no oracle in between"""
    items = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "corpus_tables.json")))
    assert len(items) >= 60
    _check_wide_guard(gpu_device, [bytes.fromhex(k["raw_hex"]) for k in items], [k["recipient_size"] for k in items],
                      [(k["good"], k["final"], k["out_sha256"]) for k in items], in_skew=9, out_skew=3)


def test_long_arms_as_small_chunk_tasks(oracle, gpu_device, monkeypatch):
    """T3's and T6's long arms at 1024 compressed bytes per task: the overflowing tables are built again in every task"""
    monkeypatch.setenv("DEBIG_CHUNK_BYTES", "1024")
    cs = ts.long_arms()
    assert all(len(c.raw) >= 5 * 1024 for c in cs)
    _run(oracle, gpu_device, cs, widths=(0x20,), in_skew=2, out_skew=3)
    monkeypatch.delenv("DEBIG_CHUNK_BYTES", raising=False)


# ------------------------------------------------------------------ the PNG arm
@pytest.fixture(scope="module")
def png_arm():
    arm = ts.png_arm()
    assert len(arm) == 16 + 8 + 1
    return arm


def test_png_arm_spec_decode(gpu_device, png_arm):
    """T2, T3 and the six-block stream of T4 as one-row 8-bit grey images through api.png_decode_batch, routed and with the
    general kernels forced -- the strict (DEBIG_STREAM_NO_REF_GATES) table build -- against png_spec_ref.decode"""
    from debigulator_amd import api

    files = [ts.png_file(raw, pixels, 0) for _, raw, pixels in png_arm]
    want = [R.decode(f) for f in files]
    for (name, _, pixels), (st, px, _) in zip(png_arm, want):
        assert st == 0 and bytes(px[0, :, 0]) == pixels, name
    for force in (False, True):
        for (name, _, _), (st, px, _), (est, epx, _) in zip(png_arm, api.png_decode_batch(files, force_general=force), want):
            assert st == est == 0, (name, force)
            assert np.array_equal(px, epx), (name, force)


def test_png_arm_fused_and_hybrid_launch(gpu_device, png_arm):
    """the same rows as palette images (the reference-compatible decode knows colour types 2, 3 and 6) through the fused
    inflate -> de-filter kernel and through what DevicePngBatch.launch() picks"""
    from debigulator_amd.png_device import DevicePngBatch

    files = [ts.png_file(raw, pixels, 3) for _, raw, pixels in png_arm]
    want = [R.decode(f)[1] for f in files]
    for how in ("fused", "launch"):
        b = DevicePngBatch(files * 2, device=gpu_device)
        b.launch_fused() if how == "fused" else b.launch()
        res, ires = b.results()
        assert (res["good"] == 1).all() and (ires["good"] == 1).all(), how
        for i in range(2 * len(files)):
            assert np.array_equal(np.asarray(b.rgba(i)).reshape(-1), want[i % len(files)].reshape(-1)), (how, png_arm[i % len(files)][0])


# What a route may still hand back under DEBIG_NO_HANDBACK, by family, and why (the reason read from its code):
#   the pair routes 0x10..0x13 hand a stream back only when its share of the token workspace runs out (scan_body /
#   strand_body: row_cur against slot.rows, rec_cur against rec_lim, si.ovf).  A window costs one token row per symbol of
#   its busiest lane, a window ends with its block, and the share is planned from the input length
#   (inflate_split_kernel.inc: PlanStreamWeight): the long runs of ONE-bit literals of T6 and the six short blocks of a T2
#   stream need several times that.  The test therefore gives the pair routes HANDBACK_WS_SCALE times the library's own
#   estimate (DeviceBatch: DEBIG_WS_SCALE) -- at the estimate's 92 + out_cap / 364 rows for a short stream that is above the
#   90 + 1088 rows of the longest T6 run -- and then NOTHING may come back;
#   the chunked route 0x20 hands back every stream that does not end DEBIG_OK (scan_body: `CHUNKED && status != DEBIG_OK`;
#   inflate_chunk_kernel.inc: "a failing stream ... is handed to debig_inflate_kernel, which owns the exact error
#   semantics"): the ten `hit` streams of T5.  Its token rows are planned as 9 bytes per compressed byte plus 24 576 bytes
#   per task (debig_ck_plan_kernel: tok_need) and shared out by compressed length (CkTaskWeight), with no term for the
#   recipient and no scale to turn: the per-task term alone, less the sixteenth that goes to records, is 90 rows of 256
#   bytes.  A short stream that needs more than that (table_shapes.token_rows: T2's four six-block streams, ten T4
#   streams, the long arms, T6 from about 34 one-bit literals on) may come back; one that needs no more may not.
#   The numbers, of the streams this test runs per family: CHUNKED_MAY below -- none of T1's 14, the four six-block streams
#   of T2's 16, the long arm of T3's 9, ten of T4's 38 (both six-block streams and eight pairs), the ten failing ones of
#   T5's 20, and of T6's 200 (offsets 0..39, every 7th beyond, every 5th window-edge stream, the long arm) the 166 whose
#   run of one-bit literals is longer than 33.  The pair routes: 0 of every family.
HANDBACK_WS_SCALE = "16"
CHUNKED_MAY = {"T1": 0, "T2": 4, "T3": 1, "T4": 10, "T5": 10, "T6": 166}
HANDBACK_ROUTES = (0x10, 0x11, 0x12, 0x13, 0x20)
CHUNK_TASK_ROWS = 24576 * 15 // 16 // 256


def _may_hand_back(width, cs):
    if width != 0x20:
        return set()
    return {c.name for c in cs if not c.legal or ts.token_rows(c) > CHUNK_TASK_ROWS}


@pytest.mark.parametrize("fam", ["T1", "T2", "T3", "T4", "T5", "T6"])
def test_routes_decode_the_table_shapes_themselves(oracle, gpu_device, monkeypatch, fam):
    monkeypatch.setenv("DEBIG_NO_HANDBACK", "1")
    monkeypatch.setenv("DEBIG_WS_SCALE", HANDBACK_WS_SCALE)
    cs = _family(oracle, fam)
    if fam == "T6":
        cs = cs[:40] + cs[40:ts.T6_SPAN:7] + cs[ts.T6_SPAN:-1:5] + cs[-1:]
    items = [hc.Item(c.name, c.raw, c.cap) for c in cs]
    exp = hc.expectations(oracle.inflate, items)
    for width in HANDBACK_ROUTES:
        b = DeviceBatch.from_streams([i.raw for i in items], [i.cap for i in items], device=gpu_device, in_skew=3, out_skew=5)
        b.d_out.zero_()
        b.d_results.zero_()
        b.launch(waves_per_stream=width)
        names = hc.handed_back(items, exp, hc.device_rows(items, b.streams_host, b.results(), b.outputs_host()),
                               f"{fam} {width:#x}", partial_ok=width == 0x13)
        print(f"handed back: {fam} {width:#x}: {len(names)} of {len(items)} {sorted(names)[:8]}")
        may = _may_hand_back(width, cs)
        assert names <= may, (fam, hex(width), sorted(names - may))
        assert len(may) == (CHUNKED_MAY[fam] if width == 0x20 else 0) and len(names) <= len(may)
        assert len(may) <= len(items) - 8  # never a whole family: at least eight streams of each must be the route's own
    monkeypatch.delenv("DEBIG_NO_HANDBACK", raising=False)
    monkeypatch.delenv("DEBIG_WS_SCALE", raising=False)
