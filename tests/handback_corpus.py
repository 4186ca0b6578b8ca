"""TEST TOOLING: the corpora and the check of the hand-back tests (tests/test_emu_handback.py on the lock-step
emulator, tests/test_gpu_handback.py on the device).

The five throughput routes of the inflate -- DEBIG_WAVES_SPLIT, _SPLIT_QUEUED, _STRAND, _STRAND_PIPE and _CHUNKED --
hand a stream they give up to the workgroup-per-stream kernel launched behind them in the same call, and afterwards
nothing in the results says which kernel produced the bytes.  Under DEBIG_NO_HANDBACK (include/debig_hip.h) that launch
is left out: a stream handed back stays good = 0, status = DEBIG_E_RETRY (final_set = 0 too, except behind the
two-wavefront pipeline, whose LZ77 wavefront has replayed part of the stream by then), and every OTHER stream is the
route's own work.  handed_back() returns the names of the first kind and holds the second kind to the oracle bit for
bit, by the rules of tests/test_gpu_inflate.py: _check.

Everything here is seeded; nothing imports the project beyond tests/token_fuzz.py and the workload generator."""
import collections
import random
import zlib

import token_fuzz as tf

E_RETRY = 11  # include/debig_hip.h: DEBIG_E_RETRY
UB_EXCLUDED = 0x10 | 0x02  # oracle.ub_flags for which the reference has no defined answer (tests/test_gpu_inflate.py)
TOKEN_FAMILIES = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "F8")

Item = collections.namedtuple("Item", "name raw cap")
# one stream's answer, whoever gave it: `data` = the recipient's first final_size bytes, `tail_ok` = nothing behind
# recipient_size was touched
Row = collections.namedtuple("Row", "good final_set final_size status data tail_ok")


def _deflate(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def token_family(name, inflate=None):
    """one family of tests/token_fuzz.py (F8 needs the oracle's inflate: it decides which flipped streams stay)"""
    cs = tf.f8_random(inflate) if name == "F8" else tf.fixed_families()[name]
    return [Item(c.name, c.raw, c.cap) for c in cs]


def small_zlib_corpora():
    """-> {"noise": 20, "text": 20, "runs": 20}: zlib streams of 2..60 KB of output.  noise = random bytes (stored blocks),
    text = ten letters at random (literals under short codes), runs = ONE byte repeated: 20..70 compressed bytes of
    length-258 matches at distance 1 under codes of one or two bits, the highly compressible kind
    debig_hip_inflate_workspace_bytes_io exists for"""
    rng = random.Random(1)
    out = {"noise": [], "text": [], "runs": []}
    for k in range(60):
        kind = ("noise", "text", "runs")[k % 3]
        n = rng.randint(2000, 60000)
        if kind == "noise":
            data = bytes(rng.getrandbits(8) for _ in range(n))
        elif kind == "text":
            data = bytes(rng.choice(b"abcdefgh \n") for _ in range(n))
        else:
            data = bytes([65 + k % 3]) * n
        raw = _deflate(data)
        out[kind].append(Item(f"{kind}/{k // 3}/n{n}", raw, max(n + 1, len(raw))))
    return out


def long_text_corpus():
    """eight zlib streams of 400 random words, 150..213 KB of output, 46..65 KB compressed: dozens of chunk tasks each at
    DEBIG_CHUNK_BYTES = 1024 and 3072"""
    rng = random.Random(3)
    words = [bytes(rng.getrandbits(8) for _ in range(rng.randint(3, 9))) for _ in range(400)]
    out = []
    for k in range(8):
        b = bytearray()
        while len(b) < 150000 + 9000 * k:
            b += rng.choice(words) + b" "
        out.append(Item(f"longtext/{k}/n{len(b)}", _deflate(bytes(b)), len(b) + 1))
    return out


def bench_streams(kind, n, nbytes=20000):
    """n streams of the benchmark's generator -> (items, plains)"""
    from debigulator_amd import workload

    pairs = workload.make_streams(kind, n, nbytes)
    items = [Item(f"{kind}/{i}", bytes(raw), max(len(plain) + 1, len(raw))) for i, (raw, plain) in enumerate(pairs)]
    return items, [bytes(plain) for _, plain in pairs]


def totals(items):
    """-> (total_in_bytes, total_out_cap, n): the arguments of the product's workspace-size functions"""
    return sum(len(it.raw) for it in items), sum(it.cap for it in items), len(items)


def expectations(inflate, items):
    """the oracle's answer to every item: [(good, final or None, bytes, ub_flags)]"""
    out = []
    for it in items:
        g, f, o, st = inflate(it.raw, it.cap, want_stats=True)
        out.append((g, f, o, st.ub_flags))
    return out


def emu_rows(items, outs, arena, offs, fill=0xA5, guard=1024):
    """rows of an emu_binding.emu_inflate() call"""
    rows = []
    for it, (good, final, data, r), (_, oo) in zip(items, outs, offs):
        tail_ok = bool((arena[oo + it.cap:oo + it.cap + guard] == fill).all())
        rows.append(Row(int(good), int(r.final_set), int(r.final_size), int(r.status), data, tail_ok))
    return rows


def device_rows(items, streams_host, res, host, guard=32):
    """rows of a DeviceBatch launch: streams_host / res in the caller's order, host = the whole output arena, zeroed before
    the launch"""
    rows = []
    for i, it in enumerate(items):
        off, cap = int(streams_host[i]["out_off"]), int(streams_host[i]["out_cap"])
        assert cap == it.cap
        n = min(int(res[i]["final_size"]), cap) if res[i]["final_set"] else 0
        rows.append(Row(int(res[i]["good"]), int(res[i]["final_set"]), int(res[i]["final_size"]), int(res[i]["status"]),
                        host[off:off + n].tobytes(), not host[off + cap:off + cap + guard].any()))
    return rows


def handed_back(items, exp, rows, where="", partial_ok=False):
    """-> the set of names the route handed back.  Every other stream is held to the oracle: good, whether the final size is
    set, the size, every byte; no stream, handed back or not, may touch what lies behind recipient_size.
    partial_ok: DEBIG_WAVES_STRAND_PIPE, where a stream handed back may carry the size its LZ77 wavefront got to."""
    assert len(items) == len(exp) == len(rows)
    names = set()
    for it, (g, f, o, ub), r in zip(items, exp, rows):
        assert r.tail_ok, f"{where} {it.name}: wrote past recipient_size"
        if r.status == E_RETRY:
            assert r.good == 0 and (partial_ok or r.final_set == 0), (where, it.name, r[:4])
            names.add(it.name)
            continue
        if ub & UB_EXCLUDED:
            continue  # the reference itself is in undefined behaviour here
        assert r.good == g, (where, it.name, r[:4], f)
        if f is None:
            assert r.final_set == 0, (where, it.name, r[:4])
            continue
        assert r.final_set == 1 and r.final_size == f, (where, it.name, r[:4], f)
        assert r.data == o, f"{where} {it.name}: bytes differ"
    assert len(names) == sum(r.status == E_RETRY for r in rows), "two streams of one name"
    return names


def check_all_oracle(items, exp, rows, where=""):
    """a call WITHOUT the switch: nothing is handed back, every stream is the oracle's"""
    assert handed_back(items, exp, rows, where) == set(), where
