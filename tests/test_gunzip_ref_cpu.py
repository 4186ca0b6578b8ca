"""CPU: the restatement of debig_gunzip_batch (tests/gunzip_ref.py) and the case list of the GPU test (tests/gunzip_cases.py) checked
without a GPU: the restatement against the status written down per case, against python's gzip module on every file that is
well-formed, and its header walk against the library's own (debig_gz_parse_header, host code)."""
import ctypes as C
import gzip

import pytest

import gunzip_cases as G
import gunzip_ref as R


@pytest.fixture(scope="module")
def cases():
    return G.cases()


def test_case_list_has_one_status_outside_the_two_families(cases):
    for c in cases:
        w = G.want(c)
        assert w.statuses == G.allowed(c), (c.name, w)
        if c.expect in G.FAMILY_SETS:
            assert w.family == c.expect, (c.name, w)
        else:
            assert w.family is None and len(w.statuses) == 1, (c.name, w)
        assert w.out_size <= (c.cap or 0) and len(w.out) <= w.out_size
        assert (len(w.out) == w.out_size) == (w.family != G.RACE), c.name
    assert {c.expect for c in cases} == set(range(8)) | set(G.FAMILY_SETS)  # every status and both families occur


def test_lies_never_pass_and_keep_the_members_before_them(cases):
    lies = [c for c in cases if c.name.startswith("lie-")]
    assert len(lies) >= 25
    for c in lies:
        w, k = G.want(c), int(c.name.split("-member-")[1][0])
        assert R.OK not in w.statuses
        before = b"".join(G.LIE_PARTS[:k])
        assert w.out[:len(before)] == before and w.out_size >= len(before), c.name
        # the members in front of member k are the output, and member k's too where only its checksums fail
        counted = k + (1 if c.expect in (R.E_CRC, R.E_ISIZE, G.RACE) else 0)
        assert w.members == counted, (c.name, w.members)


def test_restatement_agrees_with_gzip_on_every_well_formed_file(cases):
    n = 0
    for c in cases:
        w = G.want(c)
        if w.statuses == {R.OK}:
            assert gzip.decompress(c.data) == w.out, c.name
            n += 1
    assert n >= 60


def test_header_walk_agrees_with_the_library(native_lib, cases):
    f = native_lib.debig_gz_parse_header
    f.restype = C.c_uint32
    f.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def lib(b):
        hl, ms = C.c_uint64(77), C.c_uint64(77)
        st = f(b, len(b), C.byref(hl), C.byref(ms))
        return st, hl.value, ms.value

    n = 0
    for c in cases:
        if c.data is None:
            continue
        assert lib(c.data) == R.parse_header(c.data), c.name
        n += 1
    # every header of the BGZF chains, the lying ones included: walk them by the restatement's sizes
    big = next(c for c in cases if c.name == "bgzf-300-eof").data
    pos = members = 0
    while pos < len(big):
        st, hl, bs = R.parse_header(big[pos:])
        assert (st, hl, bs) == lib(big[pos:]) and st == R.OK and bs >= hl + 8
        pos += bs
        members += 1
    assert members == 301 and pos == len(big) and n >= 300
