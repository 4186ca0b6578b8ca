"""GPU: debig_gunzip_batch (include/decode_gz.h) on the case families of tests/gunzip_cases.py -- headers with every field and cut at
every length, plain multi-member files, well-formed BGZF, BGZF whose BSIZE or ISIZE lies, trailing bytes, caps, damage -- against
the restatement tests/gunzip_ref.py (zlib inflates, the rule of the header is applied in plain Python; tests/test_gunzip_ref_cpu.py
holds it to python's gzip module).  Every file gets: a status the restatement allows (one, except in the two families named
there), out_sizes, n_members, and the output bytes -- all of them, or for an understated BGZF ISIZE those in front of the failing
member.  The same files in one call, in reverse order and alone must fare the same."""
import ctypes as C

import numpy as np
import pytest

import gunzip_cases as G
import gunzip_ref as R

pytestmark = pytest.mark.gpu
FILL = 0xEE


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def cases():
    cs = G.cases()
    return cs, [G.want(c) for c in cs]


def gunzip(api, cases):
    """debig_gunzip_batch over the cases -> [(status, out_size, members, the whole output buffer)]; a case without data is a NULL input
    entry, one without cap a NULL output entry.  Buffers are cap + 32 bytes of FILL: what lies behind cap must stay"""
    from debigulator_amd import _native as N

    L = api._lib()
    L.debig_gunzip_batch.restype = C.c_int
    L.debig_gunzip_batch.argtypes = [C.c_void_p] * 7 + [C.c_uint32]
    n = len(cases)
    ins = [None if c.data is None else np.frombuffer(c.data + b"\0", dtype=np.uint8) for c in cases]  # + 1: never an empty array
    outs = [None if c.cap is None else np.full(c.cap + 32, FILL, dtype=np.uint8) for c in cases]
    in_ptrs = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in ins])
    out_ptrs = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in outs])
    in_sizes = (C.c_uint64 * n)(*[0 if c.data is None else len(c.data) for c in cases])
    caps = (C.c_uint64 * n)(*[c.cap or 0 for c in cases])
    sizes = (C.c_uint64 * n)(*([77] * n))
    status = (C.c_uint32 * n)(*([77] * n))
    members = (C.c_uint32 * n)(*([77] * n))
    N.check(L.debig_gunzip_batch(in_ptrs, in_sizes, out_ptrs, caps, sizes, status, members, n), "debig_gunzip_batch")
    return [(status[i], sizes[i], members[i], outs[i]) for i in range(n)]


def check(case, want, got):
    st, size, members, buf = got
    assert st in want.statuses, (case.name, st, want.statuses)
    assert (size, members) == (want.out_size, want.members), (case.name, st, size, members, want.out_size, want.members)
    if buf is not None:
        assert buf[:len(want.out)].tobytes() == want.out, case.name
        assert (buf[case.cap:] == FILL).all(), case.name  # nothing behind the cap


@pytest.fixture(scope="module")
def forward(api, cases):
    """everything in one call"""
    return gunzip(api, cases[0])


def test_every_family_in_one_call(cases, forward):
    bad = []
    for c, w, g in zip(cases[0], cases[1], forward):
        try:
            check(c, w, g)
        except AssertionError as e:
            bad.append(str(e)[:300])
    assert not bad, (len(bad), bad[:12])


def test_lying_bgzf_never_passes_and_keeps_the_members_before(cases, forward):
    n = 0
    for c, w, (st, size, members, buf) in zip(cases[0], cases[1], forward):
        if c.name.startswith("lie-"):
            before = b"".join(G.LIE_PARTS[:int(c.name.split("-member-")[1][0])])  # the members in front of the lying one
            assert st != R.OK and size >= len(before) and buf[:len(before)].tobytes() == before, (c.name, st, size)
            n += 1
    assert n >= 25


def test_same_answers_in_reverse_order_and_alone(api, cases, forward):
    cs, ws = cases

    def same(c, w, a, b):
        check(c, w, b)
        if w.family is None:
            assert a[:3] == b[:3], c.name
        keep = len(w.out)
        assert a[3] is None and b[3] is None or (a[3][:keep] == b[3][:keep]).all(), c.name

    back = gunzip(api, cs[::-1])[::-1]
    for c, w, a, b in zip(cs, ws, forward, back):
        same(c, w, a, b)
    picks = list(range(7, len(cs), len(cs) // 20))[:20]
    names = {cs[i].name.split("-")[0] for i in picks}
    assert len(picks) == 20 and {"hdr", "bgzf", "lie", "trailing", "cap", "cut", "trailer"} <= names, names
    for i in picks:
        same(cs[i], ws[i], forward[i], gunzip(api, [cs[i]])[0])


def test_a_call_in_which_no_file_has_a_member_left(api, cases):
    """The verdict on a header must not depend on another file of the call still having a member to inflate: every file that ends
    at a header (its first, or the one behind its first member) in calls that hold nothing else -- the first ones have no launch
    at all, the second ones none in their second round."""
    cs, ws = cases
    firsts = [(c, w) for c, w in zip(cs, ws) if c.name.startswith("hdr-") and w.members == 0 and w.family is None
              and w.statuses <= {R.E_HEADER, R.E_TRUNCATED}]
    seconds = [(c, w) for c, w in zip(cs, ws) if c.name.startswith("hdr-") and c.name.endswith("-second") and w.family is None
               and w.statuses != {R.OK}]
    assert len(firsts) >= 30 and len(seconds) >= 25
    assert {min(w.statuses) for c, w in seconds} == {R.E_HEADER, R.E_TRUNCATED, R.E_TRAILING}
    for group in (firsts, seconds, firsts[:1], firsts[-1:], seconds[:1], seconds[-1:]):
        for (c, w), g in zip(group, gunzip(api, [c for c, w in group])):
            check(c, w, g)


def test_decode_gz_batch_ex_trailer_verdicts(api, oracle):
    """debig_decode_gz_batch_ex: one member per entry under the reference's header rule (FNAME skipped), trailer_ok = CRC-32 and ISIZE
    match.  An empty member is a 2-byte stream: the reference's inflate refuses inputs under 5 bytes (the oracle says so here), and
    trailer_ok of a member that did not decode is 0."""
    d = G.blob(9000, 900)
    good = G.member(d, name=b"with a name")
    bad_crc = G._patch(good, -8, "<B", good[-8] ^ 1)
    bad_isize = G._patch(good, -4, "<I", len(d) + 1)
    plain = G.member(d)
    empty = G.member(b"", name=b"e")
    assert oracle.inflate(empty[12:-8], 64)[0] == 0
    res = api.decode_gz_batch([good, bad_crc, bad_isize, plain, empty], [len(d) + 64] * 5)
    assert [(g, t) for g, _, t in res] == [(1, 1), (1, 0), (1, 0), (1, 1), (0, 0)]
    assert all(out == d for g, out, t in res[:4]) and res[4][1] == b""
