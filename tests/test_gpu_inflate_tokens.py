"""GPU parity on token-made DEFLATE streams (tests/token_fuzz.py), every kernel width, against the
oracle and the reference-made tests/golden/corpus_tokens.json: the LZ77 edges that zlib, the stream
generator and the header fuzzer never reach -- distance 32 768 / 32 767, distance = bytes produced on
both sides of the first 32 KiB, overlap around the store widths, dependent chains, far matches into
stored blocks across chunk tasks, 1032:1 expansion, matches that end on and cross recipient_size,
random token lists with far distances as common as near ones."""
import hashlib
import json
import os

import pytest

import handback_corpus as hc
import token_fuzz as tf
from debigulator_amd.batch import DeviceBatch
from test_gpu_inflate import WIDTHS, _check

pytestmark = pytest.mark.gpu

_EXP = {}


def _family(oracle, name):
    """the cases of one family; the generator's condition (the reference has a defined answer to every
    one of them, none is skipped) is asserted here, once per family"""
    if name not in _EXP:
        cs = tf.f8_random(oracle.inflate) if name == "F8" else tf.fixed_families()[name]
        for c in cs:
            assert oracle.inflate(c.raw, c.cap, want_stats=True)[3].ub_flags == 0, c
        _EXP[name] = cs
    return _EXP[name]


def _run(oracle, gpu_device, cs, **kw):
    _check(oracle, gpu_device, [c.raw for c in cs], [c.cap for c in cs], **kw)


@pytest.mark.parametrize("fams,in_skew,out_skew", [(("F1", "F2", "F3"), 5, 3), (("F4", "F6"), 1, 15), (("F5",), 7, 13)],
                         ids=["F1-F2-F3", "F4-F6", "F5"])
def test_token_families_every_width(oracle, gpu_device, fams, in_skew, out_skew):
    cs = [c for f in fams for c in _family(oracle, f)]
    _run(oracle, gpu_device, cs, in_skew=in_skew, out_skew=out_skew)


def test_random_token_lists_every_width(oracle, gpu_device):
    _run(oracle, gpu_device, _family(oracle, "F8"), in_skew=3, out_skew=9)


@pytest.mark.parametrize("chunk", ["1024", "3072"])
def test_chunked_path_small_tasks_far_matches_across_tasks(oracle, gpu_device, monkeypatch, chunk):
    """F5 and F8 cut into dozens of chunk tasks each: a task opens with a match whose source starts
    exactly 32 768 bytes in front of it, in the window that earlier tasks hand over"""
    monkeypatch.setenv("DEBIG_CHUNK_BYTES", chunk)
    _run(oracle, gpu_device, _family(oracle, "F5") + _family(oracle, "F8"), widths=(0x20,),
         in_skew=int(chunk) % 7, out_skew=3)
    # ... and the chunk tasks themselves did it: under DEBIG_NO_HANDBACK (include/debig_hip.h) the kernel behind them is not
    # launched, a stream handed back stays DEBIG_E_RETRY and every other one is held to the oracle once more
    monkeypatch.setenv("DEBIG_NO_HANDBACK", "1")
    for fam, cap in (("F5", 1), ("F8", 30)):
        items = [hc.Item(c.name, c.raw, c.cap) for c in _family(oracle, fam)]
        b = DeviceBatch.from_streams([i.raw for i in items], [i.cap for i in items], device=gpu_device,
                                     in_skew=int(chunk) % 7, out_skew=3)
        b.launch(waves_per_stream=0x20)
        names = hc.handed_back(items, hc.expectations(oracle.inflate, items),
                               hc.device_rows(items, b.streams_host, b.results(), b.outputs_host()), fam)
        assert len(names) <= cap, (fam, sorted(names))
    monkeypatch.delenv("DEBIG_NO_HANDBACK", raising=False)
    monkeypatch.delenv("DEBIG_CHUNK_BYTES", raising=False)


def _check_wide_guard(gpu_device, raws, caps, want, **kw):
    """every width gives want[i] = (good, final, sha256 of the bytes) and leaves 1 KiB behind
    recipient_size untouched: a match can overrun by 258 bytes.  DeviceBatch leaves 64 bytes between
    recipients, so every stream is followed by one that fails the reference's size gate (2 input bytes,
    Q1) and whose 1 KiB recipient nobody writes."""
    n = len(raws)
    raws = [r for raw in raws for r in (raw, b"\x03\x00")]
    caps = [c for cap in caps for c in (cap, 1024)]
    b = DeviceBatch.from_streams(raws, caps, device=gpu_device, **kw)
    for width in WIDTHS:
        b.d_out.zero_()
        b.d_results.zero_()
        b.launch(waves_per_stream=width)
        res = b.results()
        host = b.outputs_host()
        for i, (good, final, digest) in enumerate(want):
            off = int(b.streams_host[2 * i]["out_off"])
            cap = int(b.streams_host[2 * i]["out_cap"])
            assert cap == caps[2 * i] and int(b.streams_host[2 * i + 1]["out_off"]) - (off + cap) < 128
            assert res[2 * i]["good"] == good and res[2 * i]["final_set"] == 1, (hex(width), i)
            assert int(res[2 * i]["final_size"]) == final, (hex(width), i)
            assert hashlib.sha256(host[off:off + final].tobytes()).hexdigest() == digest, (hex(width), i)
            assert res[2 * i + 1]["good"] == 0 and res[2 * i + 1]["final_set"] == 0
            assert not host[off + cap:off + cap + 1024].any(), f"width {width:#x} stream {i}: wrote past recipient_size"
    assert len(want) == n


def test_recipient_edge_every_width(oracle, gpu_device):
    """F7: the last match crosses recipient_size by 1, 2 and 257 bytes, ends on it, ends one short"""
    cs = _family(oracle, "F7")
    want = []
    for c in cs:
        g, f, out = oracle.inflate(c.raw, c.cap)
        want.append((g, f, hashlib.sha256(out).hexdigest()))
    assert sum(g == 0 for g, _, _ in want) == 48
    _check_wide_guard(gpu_device, [c.raw for c in cs], [c.cap for c in cs], want, in_skew=2, out_skew=11)


def test_token_corpus_reference_made(gpu_device):
    """every width against the compiled reference's own answers (tests/golden/corpus_tokens.json), no
    oracle in between"""
    items = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "corpus_tokens.json")))
    assert len(items) >= 36
    _check_wide_guard(gpu_device, [bytes.fromhex(k["raw_hex"]) for k in items], [k["recipient_size"] for k in items],
                      [(k["good"], k["final"], k["out_sha256"]) for k in items], out_skew=3)
