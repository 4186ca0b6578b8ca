"""CPU: which streams the five throughput routes of the inflate hand back, on the lock-step emulator, with the
workspace sizes the PRODUCT computes (debig_hip_inflate_workspace_bytes_io, debig_hip_inflate_chunked_workspace_bytes,
called through the library) and under DEBIG_NO_HANDBACK, so that a stream which is not handed back was decoded by the
route itself -- tests/handback_corpus.py holds it to the oracle bit for bit.

The caps are conditions, not measurements (the figures of the emulator are in DESIGN.md section 10):
  split, queued, strand, pipe at the _io size: nothing of F1..F7, of the noise, text and one-byte-run corpora or of the long
      text streams is handed back, valid or failing (these routes report errors themselves); at most 30 of the 300 of F8;
  chunk tasks of 1024 and 3072 bytes: every stream the oracle fails is handed back (the design), F4 0, F5 at most 1 of 3,
      F6 at most 1 of 4, at most 2 of the 8 long text streams, at most 30 of F8;
  a quarter of the workspace: streams ARE handed back, and without the switch the same call is the oracle's throughout;
  tests/golden/handback.json: the names handed back on split, strand and 3072-byte chunk tasks, which
      tests/test_gpu_handback.py compares the device's with (python tests/test_emu_handback.py writes the file)."""
import ctypes as C
import json
import os

import pytest

import emu_binding as eb
import handback_corpus as hc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handback.json")
ROUTES = {"split": (eb.SPLIT, 0), "queued": (eb.SPLIT_QUEUED, 0), "strand": (eb.STRAND, 0), "pipe": (eb.STRAND_PIPE, 0),
          "chunked1024": (eb.CHUNKED, 1024), "chunked3072": (eb.CHUNKED, 3072)}
TOKEN_ROUTES = ("split", "queued", "strand", "pipe")
CHUNK_ROUTES = ("chunked1024", "chunked3072")
CLEAN = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "noise", "text", "runs", "mixed", "longtext")  # mixed: the three before it in one batch
GOLDEN_ROUTES = ("split", "strand", "chunked3072")
GOLDEN_CORPORA = ("F5", "F6", "F8", "runs", "longtext")
F8_CAP, TEXT_CAP = 30, 2
# every stream starts 3 bytes, every recipient 5 bytes behind a multiple of 256 -- on the device as well: which streams the
# long-segment scan hands back depends on where a stream lies in its 16-byte line
ALIGN = 256


def product_lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    for f in ("debig_hip_inflate_workspace_bytes_io", "debig_hip_inflate_chunked_workspace_bytes"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    return L


class World:
    """the corpora with the oracle's answers, and what every (route, corpus) handed back: each computed once"""

    def __init__(self, oracle):
        self.emu, self.lib, self.inflate = eb.load_emu(), product_lib(), oracle.inflate
        self.items, self.exp, self.done = {}, {}, {}
        self.small = hc.small_zlib_corpora()

    def corpus(self, name):
        if name not in self.items:
            it = (hc.token_family(name, self.inflate) if name in hc.TOKEN_FAMILIES else
                  hc.long_text_corpus() if name == "longtext" else
                  [i for three in zip(*self.small.values()) for i in three] if name == "mixed" else self.small[name])
            self.items[name], self.exp[name] = it, hc.expectations(self.inflate, it)
        return self.items[name], self.exp[name]

    def ws_bytes(self, route, items):
        """the product's own size for this batch on this route; DEBIG_CHUNK_BYTES is read at every call"""
        chunk = ROUTES[route][1]
        if not chunk:
            return int(self.lib.debig_hip_inflate_workspace_bytes_io(*hc.totals(items)))
        os.environ["DEBIG_CHUNK_BYTES"] = str(chunk)
        try:
            return int(self.lib.debig_hip_inflate_chunked_workspace_bytes(*hc.totals(items)))
        finally:
            os.environ.pop("DEBIG_CHUNK_BYTES", None)

    def run(self, route, name, ws_bytes, switch=True):
        items, exp = self.corpus(name)
        nw, chunk = ROUTES[route]
        kw = {"chunk_bytes": chunk} if chunk else {}
        outs, arena, offs = eb.emu_inflate(self.emu, [i.raw for i in items], [i.cap for i in items], nw=nw, ws_bytes=ws_bytes,
                                           no_handback=switch, align=ALIGN, in_misalign=3, out_misalign=5, **kw)
        names = hc.handed_back(items, exp, hc.emu_rows(items, outs, arena, offs), f"{route} {name}", partial_ok=route == "pipe")
        if not switch:
            assert not names and eb.last_split_retried > 0, (route, name, eb.last_split_retried)
        else:
            assert eb.last_split_retried == len(names)  # the emulator's own count
        return names

    def handed(self, route, name):
        if (route, name) not in self.done:
            self.done[route, name] = self.run(route, name, self.ws_bytes(route, self.corpus(name)[0]))
        return self.done[route, name]

    def failing(self, name):
        items, exp = self.corpus(name)
        return {it.name for it, e in zip(items, exp) if e[0] != 1}


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def test_switch_is_off_unless_set_to_something_but_zero(world):
    """DEBIG_NO_HANDBACK empty or 0: the call is the ordinary one (a quarter of the workspace, so that streams are handed
    back and the kernel behind the route has work)"""
    items, exp = world.corpus("runs")
    ws = world.ws_bytes("split", items) // 4
    for value, off in (("", True), ("0", True), ("1", False), ("00", False), ("no", False)):
        os.environ["DEBIG_NO_HANDBACK"] = value
        try:
            outs, arena, offs = eb.emu_inflate(world.emu, [i.raw for i in items], [i.cap for i in items], nw=eb.SPLIT, ws_bytes=ws)
        finally:
            os.environ.pop("DEBIG_NO_HANDBACK", None)
        names = hc.handed_back(items, exp, hc.emu_rows(items, outs, arena, offs), value)
        assert eb.last_split_retried > 0 and (names == set()) == off, (value, names)


@pytest.mark.parametrize("name", CLEAN)
@pytest.mark.parametrize("route", TOKEN_ROUTES)
def test_token_routes_decode_these_themselves(world, route, name):
    assert world.handed(route, name) == set()
    if name in ("F2", "F7"):
        assert len(world.failing(name)) == {"F2": 14, "F7": 48}[name]  # failing streams among them: reported, not handed back


@pytest.mark.parametrize("route", TOKEN_ROUTES)
def test_token_routes_random_token_lists(world, route):
    names = world.handed(route, "F8")
    print(f"{route}: {len(names)} of 300 handed back")
    assert len(names) <= F8_CAP, sorted(names)


@pytest.mark.parametrize("route", CHUNK_ROUTES)
def test_chunk_tasks_decode_all_but_a_few(world, route):
    chunk = ROUTES[route][1]
    for name, cap in (("F2", None), ("F7", None), ("F4", 0), ("F5", 1), ("F6", 1), ("longtext", TEXT_CAP), ("F8", F8_CAP)):
        names, failing = world.handed(route, name), world.failing(name)
        print(f"{route} {name}: {len(names)} handed back, {len(failing)} fail")
        assert failing <= names, (name, sorted(failing - names))  # a failing stream is the one-kernel path's
        if cap is None:
            assert names == failing and len(names) == {"F2": 14, "F7": 48}[name]
        else:
            assert len(names) <= cap, (name, sorted(names))
    for it in world.corpus("longtext")[0]:
        if it.name not in world.handed(route, "longtext"):
            assert len(it.raw) // chunk >= 4, it.name  # ... as several tasks each


@pytest.mark.parametrize("route,name", [("split", "runs"), ("strand", "text"), ("pipe", "text"), ("chunked3072", "longtext")])
def test_quarter_of_the_workspace_hands_streams_back(world, route, name):
    """the switch reports real hand-backs, and the kernel behind the route decodes them"""
    ws = world.ws_bytes(route, world.corpus(name)[0]) // 4
    names = world.run(route, name, ws)
    assert names and names - world.failing(name), (route, name)
    world.run(route, name, ws, switch=False)  # asserts: the oracle's answer for every stream, some from the second kernel


def _golden_entries(world):
    out = []
    for route in GOLDEN_ROUTES:
        for name in GOLDEN_CORPORA:
            out.append({"route": route, "corpus": name, "ws_bytes": world.ws_bytes(route, world.corpus(name)[0]),
                        "chunk_bytes": ROUTES[route][1], "names": sorted(world.handed(route, name))})
    return out


def test_golden_list_is_what_the_emulator_hands_back(world):
    """tests/golden/handback.json, which the device is compared with, is this emulator's answer at the product's sizes"""
    assert _golden_entries(world) == json.load(open(GOLD))


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.binding import Oracle, build

    build(ref=False)
    with open(GOLD, "w") as f:
        json.dump(_golden_entries(World(Oracle())), f, indent=1)
        f.write("\n")
