"""GPU: every throughput route of the inflate decodes its streams ITSELF.  DeviceBatch with its own workspaces (the
product's sizes) under DEBIG_NO_HANDBACK (include/debig_hip.h): the kernel behind the route is not launched, a stream
handed back stays DEBIG_E_RETRY, and every other stream is held to the oracle bit for bit (tests/handback_corpus.py).
The conditions are those of tests/test_emu_handback.py, which also writes tests/golden/handback.json: the names the
lock-step emulator hands back at the same workspace sizes."""
import ctypes as C
import json
import os

import pytest

import handback_corpus as hc
from debigulator_amd import _native as N
from debigulator_amd.batch import DeviceBatch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handback.json")
ROUTES = {"split": (N.WAVES_SPLIT, 0), "queued": (N.WAVES_SPLIT_QUEUED, 0), "strand": (N.WAVES_STRAND, 0),
          "pipe": (N.WAVES_STRAND_PIPE, 0), "chunked1024": (N.WAVES_CHUNKED, 1024), "chunked3072": (N.WAVES_CHUNKED, 3072)}
TOKEN_ROUTES = ("split", "queued", "strand", "pipe")
CHUNK_ROUTES = ("chunked1024", "chunked3072")
CLEAN = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "noise", "text", "runs", "mixed", "longtext")  # mixed: the three before it in one batch
F8_CAP, TEXT_CAP = 30, 2
# the emulator's layout (tests/test_emu_handback.py: ALIGN): which streams the long-segment scan hands back depends on where
# a stream lies in its 16-byte line
LAYOUT = dict(in_align=256, out_align=256, in_skew=3, out_skew=5)


class World:
    """the corpora with the oracle's answers, one DeviceBatch per corpus, and what every (route, corpus) handed back"""

    def __init__(self, oracle, device):
        self.inflate, self.device = oracle.inflate, device
        self.items, self.exp, self.done, self.ws = {}, {}, {}, {}
        self.small = hc.small_zlib_corpora()

    def corpus(self, name):
        if name not in self.items:
            it = (hc.token_family(name, self.inflate) if name in hc.TOKEN_FAMILIES else
                  hc.long_text_corpus() if name == "longtext" else
                  [i for three in zip(*self.small.values()) for i in three] if name == "mixed" else self.small[name])
            self.items[name], self.exp[name] = it, hc.expectations(self.inflate, it)
        return self.items[name], self.exp[name]

    def run(self, monkeypatch, route, name, switch=True, ws_scale=None):
        """a fresh DeviceBatch (its workspace is sized at the first launch) -> (names handed back, workspace bytes)"""
        items, exp = self.corpus(name)
        width, chunk = ROUTES[route]
        monkeypatch.setenv("DEBIG_NO_HANDBACK", "1" if switch else "0")
        if chunk:
            monkeypatch.setenv("DEBIG_CHUNK_BYTES", str(chunk))
        if ws_scale is not None:
            monkeypatch.setenv("DEBIG_WS_SCALE", str(ws_scale))
        try:
            b = DeviceBatch.from_streams([i.raw for i in items], [i.cap for i in items], device=self.device, **LAYOUT)
            b.launch(waves_per_stream=width)
            res, host = b.results(), b.outputs_host()
        finally:
            for v in ("DEBIG_NO_HANDBACK", "DEBIG_CHUNK_BYTES", "DEBIG_WS_SCALE"):
                monkeypatch.delenv(v, raising=False)
        if chunk:
            assert b.chunk_groups == [(0, len(items))]
        ws = b.d_ws_chunked if chunk else b.d_ws
        names = hc.handed_back(items, exp, hc.device_rows(items, b.streams_host, res, host), f"{route} {name}",
                               partial_ok=route == "pipe")
        return names, int(ws.numel())

    def handed(self, monkeypatch, route, name):
        if (route, name) not in self.done:
            self.done[route, name], self.ws[route, name] = self.run(monkeypatch, route, name)
        return self.done[route, name]

    def failing(self, name):
        items, exp = self.corpus(name)
        return {it.name for it, e in zip(items, exp) if e[0] != 1}


@pytest.fixture(scope="module")
def world(oracle, gpu_device):
    return World(oracle, gpu_device)


@pytest.mark.parametrize("route", TOKEN_ROUTES)
def test_token_routes_decode_these_themselves(world, monkeypatch, route):
    """nothing of F1..F7, of the noise, text and one-byte-run corpora or of the long text streams is handed back at the _io
    size, valid or failing: these routes report errors themselves"""
    for name in CLEAN:
        assert world.handed(monkeypatch, route, name) == set(), name
    assert (len(world.failing("F2")), len(world.failing("F7"))) == (14, 48)


@pytest.mark.parametrize("route", TOKEN_ROUTES)
def test_token_routes_random_token_lists(world, monkeypatch, route):
    names = world.handed(monkeypatch, route, "F8")
    print(f"{route}: {len(names)} of 300 handed back")
    assert len(names) <= F8_CAP, sorted(names)


@pytest.mark.parametrize("route", CHUNK_ROUTES)
def test_chunk_tasks_decode_all_but_a_few(world, monkeypatch, route):
    """every stream the oracle fails is handed back (the design); of the others F4 none, F5 at most 1 of 3, F6 at most 1 of
    4, at most 2 of the 8 long text streams; at most 30 of the 300 of F8; a text stream that is not handed back was at least
    four tasks"""
    chunk = ROUTES[route][1]
    for name, cap in (("F2", None), ("F7", None), ("F4", 0), ("F5", 1), ("F6", 1), ("longtext", TEXT_CAP), ("F8", F8_CAP)):
        names, failing = world.handed(monkeypatch, route, name), world.failing(name)
        print(f"{route} {name}: {len(names)} handed back, {len(failing)} fail")
        assert failing <= names, (name, sorted(failing - names))
        if cap is None:
            assert names == failing and len(names) == {"F2": 14, "F7": 48}[name]
        else:
            assert len(names) <= cap, (name, sorted(names))
    for it in world.corpus("longtext")[0]:
        if it.name not in world.handed(monkeypatch, route, "longtext"):
            assert len(it.raw) // chunk >= 4, it.name


@pytest.mark.parametrize("route,name", [("split", "runs"), ("strand", "text"), ("pipe", "text")])
def test_quarter_of_the_workspace_hands_streams_back(world, monkeypatch, route, name):
    """DEBIG_WS_SCALE = 0.25: the switch reports real hand-backs, and without it the same call is the oracle's throughout"""
    names, ws = world.run(monkeypatch, route, name, ws_scale=0.25)
    assert names - world.failing(name), (route, name)
    again, ws2 = world.run(monkeypatch, route, name, switch=False, ws_scale=0.25)
    assert again == set() and ws2 == ws


def test_quarter_of_the_chunk_workspace_hands_streams_back(world, monkeypatch, gpu_device):
    """the same for chunk tasks, through debig_hip_inflate_batch_ws with a caller-owned buffer of a quarter of the size"""
    import torch

    items, exp = world.corpus("longtext")
    monkeypatch.setenv("DEBIG_CHUNK_BYTES", "3072")
    b = DeviceBatch.from_streams([i.raw for i in items], [i.cap for i in items], device=gpu_device, **LAYOUT)
    ws = torch.empty(int(b.lib.debig_hip_inflate_chunked_workspace_bytes(*hc.totals(items))) // 4, dtype=torch.uint8, device=gpu_device)
    got = []
    for switch in ("1", "0"):
        monkeypatch.setenv("DEBIG_NO_HANDBACK", switch)
        b.d_out.zero_()
        b.d_results.zero_()
        N.check(b.lib.debig_hip_inflate_batch_ws(b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_streams.data_ptr(), b.d_results.data_ptr(),
                                                 b.n, N.WAVES_CHUNKED, ws.data_ptr(), ws.numel(),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "debig_hip_inflate_batch_ws")
        got.append(hc.handed_back(items, exp, hc.device_rows(items, b.streams_host, b.results(), b.outputs_host()), switch))
    monkeypatch.delenv("DEBIG_NO_HANDBACK", raising=False)
    monkeypatch.delenv("DEBIG_CHUNK_BYTES", raising=False)
    assert got[0] and got[1] == set()


def test_no_usable_workspace_is_an_error_under_the_switch(world, monkeypatch, gpu_device):
    """a workspace too small to try sends the whole batch to the one-kernel path; under the switch the call says so"""
    import torch

    items, exp = world.corpus("text")
    b = DeviceBatch.from_streams([i.raw for i in items], [i.cap for i in items], device=gpu_device)
    ws = torch.empty(4096, dtype=torch.uint8, device=gpu_device)
    args = (b.d_in.data_ptr(), b.d_out.data_ptr(), b.d_streams.data_ptr(), b.d_results.data_ptr(), b.n)
    tail = (ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for width in (N.WAVES_SPLIT, N.WAVES_SPLIT_QUEUED, N.WAVES_STRAND, N.WAVES_STRAND_PIPE, N.WAVES_CHUNKED):
        monkeypatch.setenv("DEBIG_NO_HANDBACK", "1")
        assert b.lib.debig_hip_inflate_batch_ws(*args, width, *tail) == 1, hex(width)  # hipErrorInvalidValue
        monkeypatch.setenv("DEBIG_NO_HANDBACK", "0")
        b.d_results.zero_()
        N.check(b.lib.debig_hip_inflate_batch_ws(*args, width, *tail), "debig_hip_inflate_batch_ws")
        hc.check_all_oracle(items, exp, hc.device_rows(items, b.streams_host, b.results(), b.outputs_host()), hex(width))
    monkeypatch.delenv("DEBIG_NO_HANDBACK", raising=False)


def _planned_width(ins, caps):
    """debig_plan_batch (csrc/host/debig_ctx.h) restated for more than 1024 plain streams, as tests/test_gpu_png_damage.py
    restates it for PNG files"""
    n = len(ins)
    assert n > 1024
    large = sum(i >= (256 << 10) or c >= (1 << 20) for i, c in zip(ins, caps))
    if max(ins) >= 4 << 20 and n <= 16384:
        return N.WAVES_CHUNKED
    if 0 < large <= 256:
        return 0x41
    return N.WAVES_STRAND_PIPE if n <= 2048 else N.WAVES_STRAND if n <= 3072 else N.WAVES_SPLIT


@pytest.mark.parametrize("n,width", [(1100, N.WAVES_STRAND_PIPE), (2600, N.WAVES_STRAND), (3500, N.WAVES_SPLIT)])
def test_benchmark_routes_through_the_host_call(native_lib, gpu_device, monkeypatch, n, width):
    """api.inflate_batch (the library's cached workspace) on the benchmark's streams, 20 000 bytes each, a third of every
    kind: the width is the planner's, and under the switch every stream is good -- decoded by that route"""
    from debigulator_amd import api

    per = -(-n // 3)
    items, plains = [], []
    for kind in ("fixed", "dynamic", "stored"):
        it, pl = hc.bench_streams(kind, per)
        items, plains = items + it, plains + pl
    items, plains = items[:n], plains[:n]
    assert _planned_width([len(i.raw) for i in items], [i.cap for i in items]) == width
    monkeypatch.setenv("DEBIG_NO_HANDBACK", "1")
    out = api.inflate_batch([i.raw for i in items], [i.cap for i in items])
    monkeypatch.delenv("DEBIG_NO_HANDBACK", raising=False)
    assert [i for i, o in enumerate(out) if o[0] != 1] == []
    for i in range(0, n, 97):
        assert out[i][1] == len(plains[i]) and out[i][2] == plains[i], items[i].name


def test_device_hands_back_what_the_emulator_does(world, monkeypatch):
    """tests/golden/handback.json: split, strand and 3072-byte chunk tasks on F5, F6, F8, the one-byte runs and the long text
    streams, same workspace bytes on both sides"""
    entries = json.load(open(GOLD))
    assert len(entries) == 15
    diff = []
    for e in entries:
        assert ROUTES[e["route"]][1] == e["chunk_bytes"]
        names = world.handed(monkeypatch, e["route"], e["corpus"])
        assert world.ws[e["route"], e["corpus"]] == e["ws_bytes"], e["route"]
        if sorted(names) != e["names"]:
            diff.append((e["route"], e["corpus"], sorted(names - set(e["names"])), sorted(set(e["names"]) - names)))
    assert diff == []
