"""nghttp2_amd_hd_replay_host (csrc/hd_replay.h walked on the host; no GPU):
the meaning of a block's records -- index resolution, insertion with
eviction, the size update rules, the bad state -- over the same header, ring
and stores the device contexts use.

Held against the Python restatement (tests/hd_parse_ref.py: replay on
oracle.hpack_oracle.Inflater) in status, fields, table, size, max and the
three flags after every block, and against every inflate step the reference
itself recorded (tests/golden/ref_hd_wire.json).  Huffman literals are
decoded through the C oracle."""
import numpy as np
import pytest

from nghttp2_amd import hd
from oracle import hpack_oracle as HO
from tests import hd_parse_ref as P
from tests import hd_replay_ref as R
from tests import ref_hd_wire_lib as W


def ref_block(ref, blk):
    rv, ops = hd.parse_block(blk)
    return P.replay(ref, rv == 0, P.as_tuples(ops), P.wire_literal(blk), blk[0] if blk else None)


def ref_state(ref):
    return [tuple(e) for e in ref.table], ref.size, ref.max, (ref.expect_size, ref.bad, ref.mid_block)


def run_steps(steps, table_bytes=4096):
    """One connection's steps on the twin, block by block, and on the oracle:
    equal after every step.  Returns the statuses of the blocks."""
    inf, ref = hd.HostReplayInflater(table_bytes), HO.Inflater()
    out = []
    for k, s in enumerate(steps):
        if isinstance(s, tuple):
            assert inf.change_table_size(s[1]) == ref.change_table_size(s[1]), (k, s)
        else:
            st, f, _ = R.host_blocks(inf, [s])
            rs, rf = ref_block(ref, s)
            assert (st[0], f[0]) == (rs, rf), (k, s.hex()[:80])
            out.append(rs)
        assert R.host_state(inf) == ref_state(ref), (k, s)
    return out


def run_connections(order, blocks, table_bytes):
    nconn = max(order) + 1
    per = [[b for c, b in zip(order, blocks) if c == i] for i in range(nconn)]
    fails = 0
    for mine in per:
        fails += sum(s < 0 for s in run_steps(mine, table_bytes))
        # the same blocks in one call: the walk carries the table across them
        inf, ref = hd.HostReplayInflater(table_bytes), HO.Inflater()
        st, f, _ = R.host_blocks(inf, mine)
        want = [ref_block(ref, b) for b in mine]
        assert list(zip(st, f)) == want
        assert R.host_state(inf) == ref_state(ref)
    return fails


@pytest.mark.parametrize("seed", [0xE2E, 1, 2, 3])
def test_random_blocks_against_restatement(seed):
    order, blocks = P.random_blocks(seed, 12, 6, corrupt=0.12 if seed == 0xE2E else 0.3)
    fails = run_connections(order, blocks, 4096)
    assert 0 < fails < len(blocks)


def test_edge_blocks_against_restatement():
    blocks = [b for _, b in P.edge_blocks()]
    run_connections(list(range(len(blocks))), blocks, 4096)
    # all of them on one connection (65536-byte entries: a larger store)
    run_connections([0] * len(blocks), blocks, 1 << 18)


@pytest.mark.parametrize("name", sorted(R.RULES))
def test_rule(name):
    st = run_steps(R.RULES[name])
    want = {
        "size/first": [1], "size/second": [1, 1], "size/after-field": [-523, -523],
        "size/above-settings": [-523, -523], "size/at-settings": [1],
        "size/above-min-after-shrink": [1, -523], "size/at-min-after-shrink": [1, 1],
        "expect/missing": [-523, -523], "expect/missing-empty": [-523, -523],
        "expect/leading-size-fails": [-523], "expect/met": [1, 1, 1],
        "index/0": [-523, -523], "index/name-0": [-523, -523], "index/last-and-past": [-523, -523],
        "index/past": [-523, -523], "index/name-past": [-523],
        "entry/larger-than-max": [3, -523, -523], "entry/exactly-max": [3, -523],
        "evict/own-name": [3, 3, -523], "evict/inside-one-block": [5, -523],
        "huff/bad-name-good-value": [-523, -523], "huff/good-name-bad-value": [-523, -523],
        "huff/indexed-name-bad-value": [-523, -523], "huff/insert-and-reference": [2, 2],
        "parse/cut-after-fields": [-523, -523], "no-index": [2], "empty": [0, 1, 0],
    }[name]
    assert st == want


def test_rule_flags():
    """Both values of mid_block after a failed block, and what a change of
    the table size then returns."""
    inf = hd.HostReplayInflater()
    assert inf.change_table_size(100) == 0 and inf.flags() == (True, False, False)
    assert R.host_blocks(inf, [b"\x82"])[0] == [hd.NGHTTP2_ERR_HEADER_COMP]
    assert inf.flags() == (True, True, False) and inf.change_table_size(200) == 0
    inf = hd.HostReplayInflater()
    inf.change_table_size(100)
    assert R.host_blocks(inf, [R.size(200) + b"\x82"])[0] == [hd.NGHTTP2_ERR_HEADER_COMP]
    assert inf.flags() == (True, True, True)
    assert inf.change_table_size(300) == hd.NGHTTP2_ERR_INVALID_STATE and inf.hdr[0]["settings_max"] == 100


def test_own_name_eviction_fields():
    st, f, _ = R.host_blocks(hd.HostReplayInflater(), R.RULES["evict/own-name"][:2])
    assert st == [3, 3]
    assert f[0] == [(b"abcdefgh", b"12345678", 0), (b"abcdefgh", b"w" * 20, 0), (b"abcdefgh", b"w" * 20, 0)]
    assert f[1] == [(b"abcdefgh", b"w" * 20, 0), (b"abcdefgh", b"x" * 21, 0), (b"abcdefgh", b"x" * 21, 0)]


def test_overflow_is_all_or_nothing():
    blocks = [R.ins(b"abc", b"def") + b"\xbe\x82", b"\xbe" + R.ins(b"x", b"y")]
    inf = hd.HostReplayInflater()
    st, f, totals = R.host_blocks(inf, blocks)
    nf, nb = int(totals[0]), int(totals[1])
    assert (nf, nb) == (5, sum(len(n) + len(v) + 2 for b in f for n, v, _ in b)) and totals[2] == 0
    for nva_cap, arena_cap, bit in ((nf - 1, nb, hd.DEV_OVERFLOW_NVA), (nf, nb - 1, hd.DEV_OVERFLOW_ARENA)):
        again = hd.HostReplayInflater()
        wire, off, op_off, ops, pst = R.batch(blocks)
        t, nva, arena, nv_off, out = again.replay(wire, off, op_off, ops, pst, nva_cap=nva_cap, arena_cap=arena_cap)
        assert t.tolist() == [nf, nb, bit, 0] and out.tolist() == st and nv_off.tolist() == [0, 3, 5]
        assert not arena.any() and not nva.view(np.uint8).any()
        assert R.host_state(again) == ([], 0, 4096, (False, False, False))
        t, nva, arena, nv_off, out = again.replay(wire, off, op_off, ops, pst, nva_cap=nf, arena_cap=nb)
        assert t[2] == 0 and hd.replay_fields(nva, arena, nv_off, out) == (st, f)
        assert R.host_state(again) == R.host_state(inf)


def test_capacity_rule():
    """Settings and a size update far above table_bytes: insertions up to
    exactly table_bytes accounted are taken, the next one is NOMEM with the
    earlier fields emitted, and every later block fails."""
    tb = 4096
    inf = hd.HostReplayInflater(tb)
    assert inf.change_table_size(0xFFFFFFFF) == 0
    one = R.ins(b"a", b"v" * 991)  # 1 + 991 + 32 = 1024
    st, f, _ = R.host_blocks(inf, [R.size(1 << 30) + one * 4])
    assert st == [4] and inf.table_size() == tb and inf.table_max() == 1 << 30 and len(inf.table()) == 4
    st, f, _ = R.host_blocks(inf, [b"\x82" + R.ins(b"b", b"") + b"\x84", b"\x82"])
    assert st == [hd.NGHTTP2_ERR_NOMEM, hd.NGHTTP2_ERR_HEADER_COMP]
    assert f == [[(b":method", b"GET", 0)], []]
    assert inf.flags() == (False, True, True)
    assert R.host_blocks(inf, [b"\x82"])[0] == [hd.NGHTTP2_ERR_HEADER_COMP]
    # the same bytes with room: the HPACK numbers alone decide
    big = hd.HostReplayInflater(2 * tb)
    big.change_table_size(0xFFFFFFFF)
    st, f, _ = R.host_blocks(big, [R.size(1 << 30) + one * 4, b"\x82" + R.ins(b"b", b"") + b"\x84"])
    assert st == [4, 3] and big.table_size() == tb + 33


def test_recorded_reference():
    """All 881 recorded inflate steps and 255 ichange steps of the 322 inflate
    connections, through parse, the oracle decode and the twin.  Every table
    of the fixture is within 4096 bytes at every step's end and, as this run
    shows (no NOMEM), within it inside every step too: table_bytes = 4096."""
    conns = W.connections(side="i")
    ninf = nchg = nomem = 0
    recorded = sum(len(W.inflate_steps(c)) for c in conns)  # every ichange and inflate step there is
    for c in conns:
        inf = hd.HostReplayInflater(4096)
        for k, s in enumerate(c["steps"]):
            if s["op"] == "ichange":
                assert inf.change_table_size(s["v"]) == s["rv"], W.where(c, k)
                nchg += 1
            elif s["op"] == "inflate":
                st, f, _ = R.host_blocks(inf, [s["wire"]])
                nomem += st[0] == hd.NGHTTP2_ERR_NOMEM
                W.check_inflate_result(s, st[0], [(n, v, fl, hd.lookup_token(n)) for n, v, fl in f[0]], W.where(c, k))
                ninf += 1
            else:
                continue
            W.check_inflate_state(s, (inf.table(), inf.table_size(), inf.table_max()), W.where(c, k))
    assert (len(conns), ninf, nchg) == (322, 881, 255)
    skipped = recorded - ninf - nchg
    assert nomem == 0 and skipped == 0


def test_arguments():
    L = hd._replay_lib()
    inf = hd.HostReplayInflater()
    bad = hd.NGHTTP2_ERR_INVALID_ARGUMENT
    a = np.zeros(64, np.uint32)
    p = a.ctypes.data
    full = [inf.hdr.ctypes.data, inf.ring.ctypes.data, inf.store.ctypes.data, 4096, p, 0, p, 1, p, p, p, None, None,
            None, 0, p, 1, p, 1, p, p, p]
    assert L.nghttp2_amd_hd_replay_host(*full) == 0
    for k in (0, 1, 2, 4, 6, 8, 9, 10, 15, 17, 19, 20, 21):
        b = list(full)
        b[k] = None
        assert L.nghttp2_amd_hd_replay_host(*b) == bad, k
    for tb in (0, 2048, 4097, 6144):
        b = list(full)
        b[3] = tb
        assert L.nghttp2_amd_hd_replay_host(*b) == bad, tb
    b = list(full)
    b[7] = 0
    b[0] = None
    assert L.nghttp2_amd_hd_replay_host(*b) == 0  # no block: nothing is touched
