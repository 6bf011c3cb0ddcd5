"""HTTP message validation without a GPU: the value facts
(nghttp2_amd_hd_http_facts), the per-field step and the block ends
(nghttp2_amd_hd_http_on_header, _on_request_headers, _on_response_headers) and
nghttp2_amd_hd_inflate_blocks_http on batches of raw literals (no Huffman
literal: no GPU call).  tests/http_fields_ref.py is the checker;
tests/golden/http_fields.json, recorded from the reference's own
nghttp2_http_on_header, pins it."""
import ctypes

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd as H
from tests import field_checks_ref as FC
from tests import http_fields_cases as C
from tests import http_fields_ref as R

SPECIAL = [b"", b"HEAD", b"HEAd", b"CONNECT", b"CONNECTS", b"CONNECt", b"OPTIONS", b"OPTIONs", b"http", b"HTTPS",
           b"httpx", b"TrAiLeRs", b"trailers", b"trailerz", b"*", b"/", b"0", b"007", b"9223372036854775807",
           b"9223372036854775808", b"99999999999999999999", b"0" * 1000 + b"7", b"0" * 70000, b"1" + b"0" * 19,
           b"a" * 70000, b"a" * 69999 + b"@", b" \t \t", b"h2+x-y.z", b"localhost:8080", b"user@host"]


# ---- the restatement against the reference's recorded results
def test_ref_facts_match_golden():
    g = C.golden()
    for c in range(256):
        assert list(R.facts(bytes([c]))) == g["one_byte"][c], c
    for hx, f, n in g["uints"]:
        assert R.facts(bytes.fromhex(hx)) == (f, n), hx
    assert R.authority_table_sha256() == g["authority_sha256"]


def test_ref_step_matches_golden():
    g = C.golden()
    mask = g["flags_compared"]
    assert len(g["blocks"]) > 300
    for i, b in enumerate(g["blocks"]):
        fields = [(bytes.fromhex(n), bytes.fromhex(v)) for n, v in b["fields"]]
        verdicts, state, result = R.run_block(fields, b["mode"], tuple(b["state"]))
        assert verdicts == b["verdicts"], i
        assert (state[0] & mask, state[1], state[2]) == (b["state_after"][0] & mask, *b["state_after"][1:]), i
        want = R.ERR if R.ERR in b["verdicts"] else R.MESSAGING if b["end"] == -1 else 0
        assert result == want, i


def test_corpus_covers_every_verdict_and_mode_bit():
    g = C.golden()
    seen = {v for b in g["blocks"] for v in b["verdicts"]}
    assert seen == {0, R.IGN, R.REMOVE, R.ERR, R.NOT_EXAMINED}
    assert {b["end"] for b in g["blocks"]} == {None, 0, -1}
    for bit in (1, 2, 4, 8, 0x10):
        assert any(b["mode"] & bit for b in g["blocks"]) and any(not b["mode"] & bit for b in g["blocks"])


# ---- the host facts function
def test_host_facts_all_two_byte_strings():
    L = nghttp2_amd.lib()
    num = ctypes.c_int64()
    buf = ctypes.create_string_buffer(2)
    for a in range(256):
        for b in range(256):
            buf[0], buf[1] = a, b
            got = L.nghttp2_amd_hd_http_facts(buf, 2, ctypes.byref(num))
            assert (got, num.value) == R.facts(bytes((a, b))), (a, b)


def test_host_facts_special_strings():
    for s in SPECIAL + [bytes([c]) for c in range(256)]:
        assert H.http_facts(s) == R.facts(s), s[:40]
    assert nghttp2_amd.lib().nghttp2_amd_hd_http_facts(None, 5, None) == R.facts(b"")[0]


def test_null_state_is_refused():
    L = nghttp2_amd.lib()
    assert L.nghttp2_amd_hd_http_on_header(None, 0, b"a", 1, 0, -1, 0, 0, 0, -1) == H.NGHTTP2_ERR_INVALID_ARGUMENT
    assert L.nghttp2_amd_hd_http_on_request_headers(None, 0) == H.NGHTTP2_ERR_INVALID_ARGUMENT
    assert L.nghttp2_amd_hd_http_on_response_headers(None) == H.NGHTTP2_ERR_INVALID_ARGUMENT


# ---- the host step and the block ends
def _lib_run_block(fields, mode, state):
    st = H.HttpState(*state)
    verdicts, result, stopped = [], 0, False
    for name, value in fields:
        if stopped:
            verdicts.append(R.NOT_EXAMINED)
            continue
        f, n = H.http_facts(value)
        rv = H.http_on_header(st, mode, name, len(value), H.lookup_token(name), H.check_field(name),
                              H.check_field(value), f, n)
        verdicts.append(rv)
        if rv == R.ERR:
            stopped, result = True, R.ERR
    if not stopped and not mode & R.MODE_TRAILER:
        rv = H.http_on_request_headers(st, mode) if mode & R.MODE_REQUEST else H.http_on_response_headers(st)
        assert rv in (0, -1)
        if rv:
            result = R.MESSAGING
    return verdicts, (st.http_flags, st.status_code, st.content_length), result


def test_host_step_on_corpus():
    for i, (mode, state, fields) in enumerate(C.blocks()):
        v, s, r = _lib_run_block(fields, mode, state)
        ev, es, er = R.run_block(fields, mode, state)
        assert (v, r) == (ev, er), i
        assert (s[0] & R.FLAGS_COMPARED, s[1], s[2]) == (es[0] & R.FLAGS_COMPARED, es[1], es[2]), i


# ---- the _http inflate on raw literals
def _inflate(nconn, **kw):
    conn, wire, modes, states = C.wire(C.raw_lit, nconn)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    res = nghttp2_amd.inflate_blocks([infs[c] for c in conn], wire, http=modes, http_state=states, **kw)
    return res


@pytest.mark.parametrize("nconn", [1, 7])
def test_inflate_http_raw_literals(nconn):
    res = _inflate(nconn, checks=True, tokens=True)
    status, fields, masks, toks = res[:4]
    want = [f for _, _, fs in C.blocks() for f in fs]
    assert [(n, v) for fs in fields for n, v, _ in fs] == want
    assert status == [len(fs) for _, _, fs in C.blocks()]
    assert masks.tolist() == [[FC.mask(n), FC.mask(v)] for n, v in want]
    assert toks.tolist() == [H.lookup_token(n) for n, _ in want]
    C.check_http(res)


@pytest.mark.parametrize("nconn", [1, 7])
def test_inflate_http_cut_batch_equals_uncut(nconn):
    """A batch cut by small buffers (and resubmitted) gives the verdicts and
    states of an uncut one; neither masks nor tokens are asked for."""
    res = _inflate(nconn, nva_cap=9, arena_cap=700)
    assert len(res) == 5
    C.check_http(res)


def test_inflate_http_entry_inserted_by_plain_call():
    """Entries that a call without http inserted get their facts at the first
    reference from an _http call."""
    lit = C.raw_lit
    inf = nghttp2_amd.HpackInflater()
    fields = [(b":method", b"HEAD"), (b":scheme", b"HTTPS"), (b":authority", b"user@host"), (b":path", b"/x"),
              (b"content-length", b"0042"), (b"te", b"TRAILERS")]
    first = b"".join(b"\x40" + lit(n) + lit(v) for n, v in fields)
    st, _ = nghttp2_amd.inflate_blocks([inf], [first])
    assert st == [len(fields)]
    second = b"".join(C.hpack_int(62 + len(fields) - 1 - k, 7, 0x80) for k in range(len(fields)))
    for _ in range(2):  # the second time from the entries' own descriptors
        res = nghttp2_amd.inflate_blocks([inf], [second], http=[R.MODE_REQUEST])
        ev, es, er = R.run_block(fields, R.MODE_REQUEST, (0, -1, -1))
        assert R.ERR in ev and ev[-1] == R.NOT_EXAMINED
        assert res[2].tolist() == ev and res[4] == [er]
        assert tuple(res[3][0].tolist()) == es
    ok = [fields[0], fields[1], (b":authority", b"host"), fields[3], fields[4], fields[5]]
    third = C.hpack_int(62 + 5, 7, 0x80) + C.hpack_int(62 + 4, 7, 0x80) + b"\x00" + lit(b":authority") + \
        lit(b"host") + b"".join(C.hpack_int(62 + 5 - k, 7, 0x80) for k in (3, 4, 5))
    res = nghttp2_amd.inflate_blocks([inf], [third], http=[R.MODE_REQUEST])
    ev, es, er = R.run_block(ok, R.MODE_REQUEST, (0, -1, -1))
    assert ev == [0] * 6 and es[2] == 42 and er == 0
    assert res[2].tolist() == ev and res[4] == [er] and tuple(res[3][0].tolist()) == es


def test_inflate_http_header_comp_block():
    """A block that ends in HEADER_COMP: verdicts for the fields before the
    error, the block result HEADER_COMP."""
    lit = C.raw_lit
    inf = nghttp2_amd.HpackInflater()
    bad = b"\x00" + lit(b":method") + lit(b"GET") + b"\x00" + lit(b"Upper") + lit(b"x") + b"\xff\xff"
    res = nghttp2_amd.inflate_blocks([inf], [bad], http=[R.MODE_REQUEST])
    assert res[0] == [H.NGHTTP2_ERR_HEADER_COMP]
    assert res[2].tolist() == [0, R.ERR] and res[4] == [R.HEADER_COMP]


def _raw_call(fn, infs, wire, extra):
    nb = len(wire)
    bufs = [ctypes.create_string_buffer(b, len(b)) for b in wire]
    ptrs = (ctypes.c_void_p * nb)(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_size_t * nb)(*[len(b) for b in wire])
    ips = (ctypes.c_void_p * nb)(*[i.p.value for i in infs])
    nva = np.zeros(4096, dtype=H._NV_DTYPE)
    arena = np.zeros(1 << 17, dtype=np.uint8)
    st = np.zeros(nb, dtype=np.int32)
    chk = np.zeros((4096, 2), dtype=np.uint8)
    tk = np.zeros(4096, dtype=np.int32)
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    vp = ctypes.c_void_p
    rv = fn(ips, nb, ptrs, lens, vp(nva.ctypes.data), 4096, ctypes.byref(nv_used), vp(arena.ctypes.data),
            arena.size, ctypes.byref(ar_used), vp(st.ctypes.data), vp(chk.ctypes.data), vp(tk.ctypes.data), *extra)
    return rv, nv_used.value, ar_used.value, nva.tobytes(), arena.tobytes(), st.tobytes(), chk.tobytes(), tk.tobytes()


def test_inflate_http_all_null_is_fields():
    L = H._inflate_lib()
    conn, wire, _, _ = C.wire(C.raw_lit, 3)
    a = _raw_call(L.nghttp2_amd_hd_inflate_blocks_fields, _conns(conn), wire, (None,))
    b = _raw_call(L.nghttp2_amd_hd_inflate_blocks_http, _conns(conn), wire, (None, None, None, None, None))
    assert a == b and a[0] == 0 and a[1] == sum(len(fs) for _, _, fs in C.blocks())
    # the modes without the states (or the reverse) is refused
    modes = (ctypes.c_uint8 * len(wire))()
    c = _raw_call(L.nghttp2_amd_hd_inflate_blocks_http, _conns(conn), wire, (modes, None, None, None, None))
    assert c[0] == H.NGHTTP2_ERR_INVALID_ARGUMENT


def _conns(conn):
    infs = [nghttp2_amd.HpackInflater() for _ in range(max(conn) + 1)]
    return [infs[c] for c in conn]
