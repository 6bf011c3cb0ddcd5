"""nghttp2_amd_hd_parse_block (the host twin of the GPU block parse,
csrc/hd_parse.h) on the CPU:

- against the Python restatement (tests/hd_parse_ref.py), record for record:
  random blocks with every representation, byte corruptions, every
  truncation of a few blocks, and the placed integer and literal edges;
- every block of tests/golden/ref_hd_wire.json: the twin's records replayed
  through the oracle's table logic reproduce the fields, error code and table
  the reference recorded, and a block the reference inflated parses ok;
- the ops_cap contract."""
import ctypes

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd
from oracle import hpack_oracle as HO
from tests import hd_parse_ref as P
from tests import ref_hd_wire_lib as R


def twin(block):
    rv, ops = hd.parse_block(block)
    assert rv in (0, hd.NGHTTP2_ERR_HEADER_COMP), rv
    return rv == 0, P.as_tuples(ops)


def test_record_layout():
    assert hd.OP_DTYPE.itemsize == 32
    assert [hd.OP_DTYPE.fields[f][1] for f in P.FIELDS] == [0, 1, 2, 4, 8, 12, 16, 20, 24, 28]
    assert (hd.OP_SIZE, hd.OP_INDEXED, hd.OP_LITERAL) == (P.SIZE, P.INDEXED, P.LITERAL)
    assert (hd.OP_INDEX_REQUIRED, hd.OP_NO_INDEX, hd.OP_NEW_NAME, hd.OP_NAME_HUFF, hd.OP_VALUE_HUFF) == \
        (P.INDEX_REQUIRED, P.NO_INDEX, P.NEW_NAME, P.NAME_HUFF, P.VALUE_HUFF)
    assert nghttp2_amd.parse_block is hd.parse_block


def test_a_block_by_hand():
    """RFC 7541 C.4.1's request: four representations, one Huffman value."""
    blk = bytes.fromhex("828684418cf1e3c2e5f23a6ba0ab90f4ff")
    ok, ops = twin(blk)
    assert ok
    assert ops == [(P.INDEXED, 0, 0, 2, 0, 0, 0, 0, -1, -1), (P.INDEXED, 0, 0, 6, 0, 0, 0, 0, -1, -1),
                   (P.INDEXED, 0, 0, 4, 0, 0, 0, 0, -1, -1),
                   (P.LITERAL, P.INDEX_REQUIRED | P.VALUE_HUFF, 0, 1, 0, 0, 5, 12, -1, 0)]


@pytest.mark.parametrize("name,blk", P.edge_blocks(), ids=[n for n, _ in P.edge_blocks()])
def test_edges_equal_reference(name, blk):
    assert twin(blk) == P.parse(blk)


def test_edge_verdicts():
    """What the placed blocks are placed for, stated once by hand."""
    got = {name: twin(blk) for name, blk in P.edge_blocks()}
    for w in (4, 5, 6, 7):
        k = (1 << w) - 1
        for name, value in (("max-1", k - 1), ("max+0", k), ("max+127", k + 127), ("max+128", k + 128),
                            ("u32max", P.U32)):
            ok, ops = got["int%d/%s" % (w, name)]
            assert ok and len(ops) == 1 and ops[0][3] == value, (w, name)
            ok, ops = got["int%d/%s/mid" % (w, name)]
            assert ok and [o[3] for o in ops] == [2, value, 4], (w, name)
        for name in ("u32max+1", "shift32", "shift28-carry", "cut-prefix", "cut-cont", "cut-cont4"):
            assert got["int%d/%s" % (w, name)] == (False, []), (w, name)
            ok, ops = got["int%d/%s/mid" % (w, name)]
            assert not ok and [o[3] for o in ops] == [2], (w, name)
    for n in (0, 1, 15, 16, 17, 65536):
        ok, ops = got["huff-value/%d" % n]
        assert ok and ops[0][7] == n and ops[0][9] == 0 and ops[0][1] & P.VALUE_HUFF
        ok, ops = got["huff-name/%d" % n]
        assert ok and ops[0][5] == n and ops[0][8] == 0 and ops[0][9] == -1
        ok, ops = got["raw-value/%d" % n]
        assert ok and ops[0][7] == n and (ops[0][8], ops[0][9]) == (0, -1)
    for kind in ("huff-value", "huff-name", "raw-value"):
        assert got[kind + "/65537"] == (False, [])
    assert got["len=left"][0] and len(got["len=left"][1]) == 2
    for name in ("len=left+1", "mid-opcode/newname"):
        ok, ops = got[name]
        assert not ok and [o[0] for o in ops] == [P.INDEXED]
    for name in ("len=left+1/raw", "mid-opcode/name-len", "mid-opcode/no-value", "mid-opcode/indname-no-value"):
        assert got[name] == (False, [])
    assert [o[0] for o in got["size/first"][1]] == [P.SIZE, P.INDEXED, P.LITERAL]
    assert [o[0] for o in got["size/middle"][1]] == [P.INDEXED, P.SIZE, P.LITERAL]
    assert [o[0] for o in got["size/last"][1]] == [P.LITERAL, P.INDEXED, P.SIZE]
    assert [o[3] for o in got["size/twice"][1]] == [0, 4096, 2]


def test_random_corrupted_and_truncated_equal_reference():
    order, blocks = P.random_blocks(0xB10C5, 8, 12, corrupt=0.3)
    assert any(not P.parse(b)[0] for b in blocks) and sum(P.parse(b)[0] for b in blocks) > len(blocks) // 2
    nhuff = 0
    for blk in blocks:
        ok, ops = P.parse(blk)
        assert twin(blk) == (ok, ops), blk.hex()
        nhuff += sum(bool(o[1] & (P.NAME_HUFF | P.VALUE_HUFF)) for o in ops)
    assert nhuff > 50
    # every truncation of a few blocks, and every byte of one flipped eight ways
    whole = [b for b in blocks if P.parse(b)[0] and len(b) > 20][:4]
    assert len(whole) == 4
    for blk in whole:
        for cut in range(len(blk) + 1):
            assert twin(blk[:cut]) == P.parse(blk[:cut]), (blk.hex(), cut)
    blk = whole[0]
    for at in range(len(blk)):
        for bit in range(8):
            x = blk[:at] + bytes([blk[at] ^ (1 << bit)]) + blk[at + 1:]
            assert twin(x) == P.parse(x), (x.hex(), at, bit)


def test_numbering_within_a_block():
    """Name before value, in order, and the literals of the representations
    before a failure keep their numbers."""
    blk = b"\x00" + P.huff_lit(2) + P.huff_lit(3) + b"\x82" + b"\x40" + P.raw_lit(2) + P.huff_lit(1) + \
        b"\x10" + P.huff_lit(1) + P.raw_lit(1) + b"\x00" + P.huff_lit(1) + b"\x85"  # cut: length 5, nothing left
    ok, ops = twin(blk)
    assert not ok
    assert [(o[8], o[9]) for o in ops] == [(0, 1), (-1, -1), (-1, 2), (3, -1)]
    assert P.parse(blk, base=7, lit0=5)[1][3][8] == 8


# prefix width -> (opcode bits, what completes the representation behind the
# integer): indexed, size update, and a literal with an indexed name (with and
# without indexing) followed by an empty raw value literal
INT_FORMS = {7: (0x80, b""), 5: (0x20, b""), 6: (0x40, b"\x00"), 4: (0x00, b"\x00")}


def _int_encodings(v, prefix, first):
    """v under `first`'s bits: the shortest form and, of a value with
    continuation groups, the forms padded with zero groups to runs of five and
    of six groups."""
    short = P.enc_int(v, prefix, first)
    out = [short]
    groups = len(short) - 1
    for run in (5, 6):
        if 0 < groups < run:
            out.append(short[:-1] + bytes([short[-1] | 0x80]) + b"\x80" * (run - groups - 1) + b"\x00")
    return out


def test_read_int_agrees_with_decode_length():
    """The two statements of the prefix integer, hdparse::read_int (every block
    parser's, the inflater's included) and the public resumable
    nghttp2_amd_hd_decode_length: a one-representation block is accepted
    exactly when decode_length over the integer's bytes ends (fin) without an
    error, and then with the same value and the same number of bytes consumed.
    Every encoding is also cut after every byte; a cut one is a block that ends
    inside its integer (what completes the representation follows a whole
    encoding only).
    A literal's name index of 0 is no integer: 0x40 / 0x00 open a literal with
    a new name, so that cell of the grid asserts that instead."""
    n = accepted_n = 0
    for prefix, (first, tail) in INT_FORMS.items():
        mask = (1 << prefix) - 1
        values = [0, mask - 1, mask, mask + 1, mask + 127, mask + 128, 1 << 14, 1 << 21, 1 << 28, P.U32 - mask,
                  P.U32, P.U32 + 1, mask + (1 << 35)]  # (the last: six groups, none of them padding)
        for v in values:
            if v == 0 and tail:
                rv, ops = hd.parse_block(bytes([first]) + b"\x00" + tail)
                assert rv == 0 and len(ops) == 1 and ops[0]["flags"] & hd.OP_NEW_NAME and ops[0]["value"] == 0
                assert hd.parse_block(bytes([first]) + tail)[0] == hd.NGHTTP2_ERR_HEADER_COMP
                continue
            encs = _int_encodings(v, prefix, first)
            assert sorted({len(e) - 1 for e in encs} - {len(encs[0]) - 1}) == \
                [r for r in (5, 6) if 0 < len(encs[0]) - 1 < r]
            for enc in encs:
                for k in range(1, len(enc) + 1):
                    cut = enc[:k]
                    rv, value, _, fin = hd.decode_length(cut, prefix)
                    block = cut + tail if k == len(enc) else cut
                    prv, ops = hd.parse_block(block)
                    assert prv in (0, hd.NGHTTP2_ERR_HEADER_COMP)
                    assert (prv == 0) == (rv >= 0 and bool(fin)), (prefix, v, enc.hex(), k)
                    n += 1
                    if prv:
                        assert len(ops) == 0
                        continue
                    accepted_n += 1
                    assert len(ops) == 1 and int(ops[0]["value"]) == value == v, (prefix, v, enc.hex())
                    # (a literal's value bytes start one length byte behind the integer)
                    consumed = int(ops[0]["value_off"]) - 1 if tail else len(block)
                    assert consumed == rv == len(enc), (prefix, v, enc.hex())
    # (accepted: at least the shortest form of the 11 values within uint32 at four widths, less the two 0 cells)
    assert n > 500 and accepted_n > 42


INFLATE_CONNS = R.connections(None, "i")


@pytest.mark.parametrize("c", INFLATE_CONNS, ids=lambda c: c["family"] + "/" + c["name"])
def test_golden_wire_parse_then_replay(c):
    inf = HO.Inflater()
    for k, s in enumerate(c["steps"]):
        w = R.where(c, k)
        if s["op"] == "ichange":
            assert inf.change_table_size(s["v"]) == s["rv"], w
        elif s["op"] == "inflate":
            wire = s["wire"]
            ok, ops = twin(wire)
            if s["status"] >= 0:
                assert ok, w
            status, fields = P.replay(inf, ok, ops, P.wire_literal(wire), wire[0] if wire else None)
            R.check_inflate_result(s, status, [(n, v, fl, HO.lookup_token(n)) for n, v, fl in fields], w)
        else:
            continue
        R.check_inflate_state(s, (list(inf.table), inf.size, inf.max), w)


def test_golden_has_the_cases():
    steps = [s for c in INFLATE_CONNS for s in c["steps"] if s["op"] == "inflate"]
    assert len(steps) > 800
    parsed = [twin(s["wire"]) for s in steps]
    assert sum(1 for ok, _ in parsed if not ok) > 50
    # blocks the parse accepts and the replay refuses (table state), both ways round
    assert any(ok and s["status"] < 0 for (ok, _), s in zip(parsed, steps))
    assert any(not ok and ops and s["fields"] for (ok, ops), s in zip(parsed, steps))


def test_ops_cap_contract():
    L = hd.lib()
    blk = b"\x82\x86\x84" + b"\x00" + P.huff_lit(2) + P.raw_lit(3) + b"\xbe"
    ok, want = twin(blk)
    assert ok and len(want) == 5
    buf = np.frombuffer(blk, dtype=np.uint8)
    for cap in range(0, 7):
        ops = np.full(8, 0xA5, dtype=np.uint8).repeat(32).view(hd.OP_DTYPE)
        canary = ops.copy()
        nops = ctypes.c_size_t(99)
        rv = L.nghttp2_amd_hd_parse_block(buf.ctypes.data, len(blk), ops.ctypes.data, cap, ctypes.byref(nops))
        assert nops.value == 5, cap
        assert rv == (hd.NGHTTP2_ERR_BUFFER_ERROR if cap < 5 else 0), cap
        assert P.as_tuples(ops[:min(cap, 5)]) == want[:cap], cap
        assert ops[min(cap, 5):].tobytes() == canary[min(cap, 5):].tobytes(), cap
    assert hd.parse_block(blk, ops_cap=4) == (hd.NGHTTP2_ERR_BUFFER_ERROR, 5)
    # a failing block: the cap comes first, then the failure with what completed
    bad = blk + b"\xff"
    assert hd.parse_block(bad, ops_cap=4) == (hd.NGHTTP2_ERR_BUFFER_ERROR, 5)
    rv, ops = hd.parse_block(bad, ops_cap=5)
    assert rv == hd.NGHTTP2_ERR_HEADER_COMP and P.as_tuples(ops) == want
    # the arguments
    nops = ctypes.c_size_t()
    bad_arg = hd.NGHTTP2_ERR_INVALID_ARGUMENT
    assert L.nghttp2_amd_hd_parse_block(None, 1, None, 0, ctypes.byref(nops)) == bad_arg
    assert L.nghttp2_amd_hd_parse_block(buf.ctypes.data, 1, None, 1, ctypes.byref(nops)) == bad_arg
    assert L.nghttp2_amd_hd_parse_block(buf.ctypes.data, 1, None, 0, None) == bad_arg
    assert L.nghttp2_amd_hd_parse_block(None, 0, None, 0, ctypes.byref(nops)) == 0 and nops.value == 0
    assert L.nghttp2_amd_hd_parse_block(buf.ctypes.data, 3, None, 0, ctypes.byref(nops)) == \
        hd.NGHTTP2_ERR_BUFFER_ERROR and nops.value == 3


def test_bound():
    assert hd.parse_blocks_bound(0, 0) == (1, 1, 16, 16)
    assert hd.parse_blocks_bound(1000, 3) == (1000, 1000, 1024, 16)
    assert hd.parse_blocks_bound(1009, 4)[2:] == (1040, 32)
    with pytest.raises(RuntimeError):
        hd.parse_blocks_bound(1 << 32, 1)
