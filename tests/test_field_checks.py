"""Header-field validation without a GPU: the restatement of nghttp2_check_*
(tests/field_checks_ref.py) against results recorded from the reference's own
tables (tests/golden/field_checks.json), the host function
nghttp2_amd_hd_check_field against the restatement, and the checked inflate
(nghttp2_amd_hd_inflate_blocks_checked) on batches whose literals are all raw
(no Huffman literal, so no GPU call): the fields equal the unchecked call's
and every mask equals the restatement applied to the emitted field."""
import itertools
import json
import os

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd
from nghttp2_amd import workloads as W
from tests import field_checks_ref as R
from tests.test_inflate_host import _int, _lit

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "field_checks.json")))
EDGES = [b"", b":", b":a", b"a:", b"A", b" a", b"a\t", b" ", b"\x7f", b"\x80"]


def test_constants_match_header():
    text = open(os.path.join(HERE, "..", "include", "nghttp2_amd_hd.h")).read()
    for name in ("NAME", "VALUE", "VALUE_RFC9113", "METHOD", "PATH", "AUTHORITY", "NAME_LOWER", "INVALID"):
        line = [l for l in text.splitlines() if l.startswith("#define NGHTTP2_AMD_CHECK_%s " % name)]
        assert len(line) == 1, name
        v = int(line[0].split()[2].rstrip("u"), 16)
        assert v == getattr(hd, "CHECK_" + name) == getattr(nghttp2_amd, "CHECK_" + name) == \
            getattr(R, "CHECK_" + name)


def test_restatement_equals_golden():
    assert GOLDEN["order"] == ["header_name", "header_value", "header_value_rfc9113", "method", "path",
                               "authority", "nonempty_header_name_is_1"]
    assert R.table_sha256() == GOLDEN["table_sha256"]
    for c in range(256):
        assert R.results(bytes([c])) == GOLDEN["one_byte"][c], c
        assert R.results(b":" + bytes([c])) == GOLDEN["colon_byte"][c], c
    assert len(GOLDEN["vectors"]) == 25
    for fn, hx, want in GOLDEN["vectors"]:
        assert R.results(bytes.fromhex(hx))[GOLDEN["order"].index(fn)] == want, (fn, hx)


def test_check_field_on_golden_and_edges():
    strings = [bytes([c]) for c in range(256)] + [b":" + bytes([c]) for c in range(256)]
    strings += [bytes.fromhex(hx) for _, hx, _ in GOLDEN["vectors"]] + EDGES
    for s in strings:
        assert hd.check_field(s) == R.mask(s), s
    # the expected masks of the edges, bit by bit
    N, V, V9, M, P, A, NL = (R.CHECK_NAME, R.CHECK_VALUE, R.CHECK_VALUE_RFC9113, R.CHECK_METHOD,
                             R.CHECK_PATH, R.CHECK_AUTHORITY, R.CHECK_NAME_LOWER)
    assert hd.check_field(b"") == V | V9 | P | A | NL
    assert hd.check_field(b":") == V | V9 | P | A
    assert hd.check_field(b":a") == N | V | V9 | P | A
    assert hd.check_field(b"a:") == V | V9 | P | A
    assert hd.check_field(b"A") == V | V9 | M | P | A
    assert hd.check_field(b" a") == V
    assert hd.check_field(b"\x7f") == 0
    assert hd.check_field(b"\x80") == V | V9 | P


def test_check_field_all_two_byte_strings():
    bad = [bytes(p) for p in itertools.product(range(256), repeat=2) if hd.check_field(bytes(p)) != R.mask(bytes(p))]
    assert not bad, bad[:8]


def test_check_field_random_strings():
    for pool, off in (W.gen_all_bytes(4096, seed=11), W.gen_names(4096)):
        for i in range(len(off) - 1):
            s = pool[off[i]:off[i + 1]].tobytes()
            assert hd.check_field(s) == R.mask(s), s


# ---- the checked inflate on raw literals -----------------------------------
def _checked(infs, blocks, **kw):
    st, f, m = nghttp2_amd.inflate_blocks(infs, blocks, checks=True, **kw)
    flat = [x for fb in f for x in fb]
    assert m.shape == (len(flat), 2) and m.dtype == np.uint8
    for k, (n, v, _) in enumerate(flat):
        assert (int(m[k, 0]), int(m[k, 1])) == (R.mask(n), R.mask(v)), (k, n, v)
    return st, f, m


def _pair(blocks_of, nconn=1):
    """The same blocks through the unchecked and the checked call, each on its
    own fresh inflaters: equal status and fields, masks == restatement."""
    conns, blocks = blocks_of
    a = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    b = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    st0, f0 = nghttp2_amd.inflate_blocks([a[c] for c in conns], blocks)
    st1, f1, m = _checked([b[c] for c in conns], blocks)
    assert (st0, f0) == (st1, f1)
    for x, y in zip(a, b):
        assert x.dynamic_table() == y.dynamic_table()
    return st1, f1, m


NAMES = [b"x-ok", b"X-Upper", b":path", b":", b"", b"a:b", b"na me", b"n\x00", b"caf\xc3\xa9"]
VALUES = [b"", b"plain", b" lead", b"trail\t", b"nul\x00byte", b"del\x7f", b"GET", b"/p?q=1", b"h\xffst",
          b"user@host:80", b"a b", b"{json}"]


def test_raw_literals_and_static_references():
    blocks = []
    for n in NAMES:
        for v in VALUES:
            # new name without indexing; never indexed; static name + literal value
            blocks.append(b"\x00" + _lit(n) + _lit(v) + b"\x10" + _lit(n) + _lit(v) +
                          _int(1 + (len(v) * 7 + len(n)) % 61, 4, 0x00) + _lit(v))
    blocks.append(b"".join(_int(i, 7, 0x80) for i in range(1, 62)))  # every static entry
    for conns in ([0] * len(blocks), [k % 5 for k in range(len(blocks))]):  # direct and grouped replay
        st, f, m = _pair((conns, blocks), nconn=5)
        assert all(s >= 0 for s in st)
    # :method GET is a method, a path-legal value, and a name with the ':' skipped
    assert int(m[-61 + 1, 0]) & R.CHECK_NAME and int(m[-61 + 1, 1]) & R.CHECK_METHOD


def test_dynamic_references_across_eviction_and_resize():
    big = b"v" * 1500
    blocks = [
        b"\x40" + _lit(b"x-first") + _lit(b" blank-led") + b"\x40" + _lit(b"Bad-Name") + _lit(b"ok"),
        b"\xbe\xbf" + _int(62, 6, 0x40) + _lit(b"nul\x00"),       # both entries, then Bad-Name: nul
        b"\xbe\xbf\xc0",                                            # all three from the table
        b"\x40" + _lit(b"x-big") + _lit(big) + b"\x40" + _lit(b"x-big2") + _lit(big),  # evicts the first three
        b"\xbe\xbf",
        b"\x40" + _lit(b"x-big3") + _lit(big),                      # evicts x-big
        b"\xbe\xbf" + _int(63, 4, 0x00) + _lit(b"tab\t"),
        _int(100, 5, 0x20) + b"\x40" + _lit(b"small") + _lit(b"\x7f"),  # resize: everything out, one small in
        b"\xbe",
        _int(4096, 5, 0x20) + b"\xbe" + b"\x40" + _lit(b"x y") + _lit(b"z") + b"\xbe\xbf",
    ]
    st, f, m = _pair(([0] * len(blocks), blocks))
    assert all(s >= 0 for s in st), st
    assert f[2] == [(b"Bad-Name", b"nul\x00", 0), (b"Bad-Name", b"ok", 0), (b"x-first", b" blank-led", 0)]
    # two connections interleaved (the grouped replay), one block per call too
    conns = [k % 2 for k in range(2 * len(blocks))]
    both = [blocks[k // 2] for k in range(2 * len(blocks))]
    _pair((conns, both), nconn=2)
    infs = [nghttp2_amd.HpackInflater()]
    for b, want in zip(blocks, f):
        st1, f1, _ = _checked(infs, [b])
        assert f1 == [want]


def test_entries_inserted_by_an_unchecked_call_are_checked_at_first_reference():
    inf = nghttp2_amd.HpackInflater()
    nghttp2_amd.inflate_blocks([inf], [b"\x40" + _lit(b"Up") + _lit(b" v")])
    st, f, m = _checked([inf], [b"\xbe\xbe"])
    assert f == [[(b"Up", b" v", 0)] * 2]


def test_masks_of_fields_before_a_header_comp_error():
    blocks = [b"\x82" + b"\x00" + _lit(b"A") + _lit(b"b") + b"\xff\xff\xff\xff\xff\xff",  # index overflow
              b"\x84"]
    for conns in ([0, 1], [0, 0]):
        st, f, m = _pair((conns, blocks), nconn=2)
        assert st[0] == nghttp2_amd.NGHTTP2_ERR_HEADER_COMP and len(f[0]) == 2
        assert m.shape[0] == 2 + len(f[1])


@pytest.mark.parametrize("cap", [3, 7])
def test_cut_and_retry_keeps_masks_in_field_order(cap):
    blocks = [b"\x40" + _lit(b"n%d" % k) + _lit(b" v%d" % k) + b"\xbe\x82" for k in range(9)]
    for conns in ([0] * 9, [k % 3 for k in range(9)]):
        infs = [nghttp2_amd.HpackInflater() for _ in range(3)]
        st, f, m = _checked([infs[c] for c in conns], blocks, nva_cap=cap, arena_cap=cap * 30)
        assert st == [3] * 9
