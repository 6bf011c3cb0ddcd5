"""The inflate front-end's host logic (nghttp2_amd_hd_inflate_blocks: pass-1
parse, connection grouping, the output bound and the cut-and-replay when a
batch outgrows the caller's buffers, pass-2 replay against each connection's
dynamic table) on blocks whose literals are all raw: such a batch has no
Huffman literal, so no GPU call is made and it runs here.  Checked against
the oracle's inflater (lib/nghttp2_hd.c:1919-2288 restated), block by block,
connection by connection, and against the shared chain the device path is
built from (nghttp2_amd_hd_parse_block, then nghttp2_amd_hd_replay_host)."""
import random

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd
from oracle import hpack_oracle as HO
from tests import hd_parse_ref as P
from tests import hd_replay_ref as RR


def _int(v, prefix, first):
    k = (1 << prefix) - 1
    if v < k:
        return bytes([first | v])
    out = [first | k]
    v -= k
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _lit(s):
    return _int(len(s), 7, 0) + s


def _block(rng, ndyn):
    """Indexed static and dynamic references, literals with incremental
    indexing (new and indexed names), literals without indexing, size updates
    at the block start; raw strings only."""
    b = b""
    if rng.random() < 0.1:
        b += _int(rng.choice([0, 100, 4096]), 5, 0x20)
        ndyn[0] = 0 if b[-1] == 0x20 else ndyn[0]
    for _ in range(rng.randint(0, 12)):
        r = rng.random()
        if r < 0.25:
            b += _int(rng.randint(1, 61), 7, 0x80)
        elif r < 0.4 and ndyn[0]:
            b += _int(62 + rng.randint(0, ndyn[0] - 1), 7, 0x80)
        elif r < 0.7:
            b += b"\x40" + _lit(bytes(rng.choice(b"abcdef") for _ in range(rng.randint(1, 30)))) + \
                _lit(bytes(rng.randint(32, 126) for _ in range(rng.randint(0, 200))))
            ndyn[0] = min(ndyn[0] + 1, 8)
        elif r < 0.85:
            b += _int(rng.randint(1, 61), 6, 0x40) + _lit(bytes(rng.randint(32, 126) for _ in range(rng.randint(0, 90))))
            ndyn[0] = min(ndyn[0] + 1, 8)
        else:
            b += _int(rng.randint(1, 61), 4, 0x00) + _lit(b"x" * rng.randint(0, 50))
    return b


@pytest.mark.parametrize("cap", [None, 5, 20, 60])
def test_raw_literal_batches_match_oracle(cap):
    rng = random.Random(1234 + (cap or 0))
    for _ in range(12):
        nconn = rng.randint(1, 9)
        infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
        refs = [HO.Inflater() for _ in range(nconn)]
        ndyn = [[0] for _ in range(nconn)]
        conns = [rng.randrange(nconn) for _ in range(rng.randint(1, 40))]
        blocks = [_block(rng, ndyn[c]) for c in conns]
        kw = {} if cap is None else {"nva_cap": cap, "arena_cap": cap * 40}
        st, f = nghttp2_amd.inflate_blocks([infs[c] for c in conns], blocks, **kw)
        for k, (c, b) in enumerate(zip(conns, blocks)):
            assert (st[k], f[k]) == refs[c].inflate_block(b), (k, c)
        for c in range(nconn):
            assert infs[c].dynamic_table_size() == refs[c].size
            assert [tuple(map(bytes, e)) for e in infs[c].dynamic_table()] == \
                [tuple(map(bytes, e)) for e in refs[c].table]


def test_static_table_is_one_table_for_both_sides():
    """The inflater and the deflater read one static table: for indices
    1..61 both get_table_entry functions return the oracle's RFC 7541
    Appendix A entry, byte for byte; index 0 and, on fresh objects with empty
    dynamic tables, index 62 are INVALID_ARGUMENT from both."""
    import ctypes
    inf, de = nghttp2_amd.HpackInflater(), nghttp2_amd.HpackDeflater()
    getters = ((inf.L.nghttp2_amd_hd_inflate_get_table_entry, inf.p),
               (de.L.nghttp2_amd_hd_deflate_get_table_entry, de.p))

    def entry(get, p, idx):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        la, lb = ctypes.c_size_t(), ctypes.c_size_t()
        rv = get(p, idx, ctypes.byref(a), ctypes.byref(la), ctypes.byref(b), ctypes.byref(lb))
        if rv != 0:
            return rv
        return ctypes.string_at(a, la.value), la.value, ctypes.string_at(b, lb.value), lb.value

    assert len(HO.STATIC) == 61
    for idx in range(1, 62):
        name, value = HO.STATIC[idx - 1]
        for get, p in getters:
            assert entry(get, p, idx) == (name, len(name), value, len(value)), idx
    for get, p in getters:
        assert entry(get, p, 0) == nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT
        assert entry(get, p, 62) == nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT


def test_same_inflater_twice_in_separate_batches():
    """The grouping stamp: an inflater's connection number from one call must
    not leak into the next (different batch, different connection order)."""
    rng = random.Random(7)
    infs = [nghttp2_amd.HpackInflater() for _ in range(3)]
    refs = [HO.Inflater() for _ in range(3)]
    ndyn = [[0] for _ in range(3)]
    for order in ([0, 1, 2, 0], [2, 2, 1], [1, 0, 2, 1, 0]):
        blocks = [_block(rng, ndyn[c]) for c in order]
        st, f = nghttp2_amd.inflate_blocks([infs[c] for c in order], blocks)
        for k, (c, b) in enumerate(zip(order, blocks)):
            assert (st[k], f[k]) == refs[c].inflate_block(b)


def _raw_only(block):
    """No completed representation of block holds a Huffman literal (those are
    the literals a batch sends to the GPU)."""
    _, ops = hd.parse_block(block)
    return not np.any(ops["flags"] & (hd.OP_NAME_HUFF | hd.OP_VALUE_HUFF))


def _chain_cases():
    """name -> the steps of one connection, a block or ("change", value), all
    without Huffman literals: random connections; every prefix of the second
    block of some of them (a cut at every byte, behind the first block's table);
    single-byte corruptions of the second block of others; the placed edges of
    tests/hd_parse_ref.py and the rules of tests/hd_replay_ref.py."""
    rng = random.Random(0xC4A1)
    cases = {}
    for c in range(40):
        ndyn = [0]
        cases["random/%d" % c] = [_block(rng, ndyn) for _ in range(6)]

    def pair():
        ndyn = [0]
        a, b = _block(rng, ndyn), _block(rng, ndyn)
        return (a, b) if 20 < len(b) < 400 else pair()
    for c in range(10):
        a, b = pair()
        for cut in range(len(b) + 1):
            cases["prefix/%d/%d" % (c, cut)] = [a, b[:cut]]
    c = 0
    while c < 300:
        a, b = pair()
        at = rng.randrange(len(b))
        x = b[:at] + bytes([b[at] ^ rng.randint(1, 255)]) + b[at + 1:]
        if _raw_only(x):
            cases["corrupt/%d" % c] = [a, x]
            c += 1
    for name, blk in P.edge_blocks():
        if _raw_only(blk):
            cases["edge/" + name] = [blk]
    for name, steps in RR.RULES.items():
        if all(_raw_only(s) for s in steps if not isinstance(s, tuple)):
            cases["rule/" + name] = steps
    return cases


def test_inflater_equals_parse_then_host_replay():
    """Pass 1 of the inflater is hdparse::walk; this holds the whole call to
    the other users of that walk.  nghttp2_amd_hd_inflate_blocks on fresh
    inflaters against nghttp2_amd_hd_parse_block + nghttp2_amd_hd_replay_host
    (table_bytes 4096) on the same blocks: status, fields and flags of every
    block, the result of every change of the table size, and the table at the
    end.  The cases' step t go through one inflate_blocks call, a connection
    each.  No block may end in the replay's NOMEM (its store's capacity rule,
    which the inflater does not have), so that rule hides no mismatch."""
    cases = _chain_cases()
    assert sum(k.startswith("edge/") for k in cases) > 60 and sum(k.startswith("rule/") for k in cases) > 20
    assert sum(k.startswith("prefix/") for k in cases) > 1000
    names = sorted(cases)
    infs = {k: nghttp2_amd.HpackInflater() for k in names}
    twins = {k: hd.HostReplayInflater(4096) for k in names}
    nomem = failed = fields = 0
    for t in range(max(len(v) for v in cases.values())):
        live = [k for k in names if t < len(cases[k])]
        for k in live:
            step = cases[k][t]
            if isinstance(step, tuple):
                assert infs[k].change_table_size(step[1]) == twins[k].change_table_size(step[1]), (k, t)
        live = [k for k in live if not isinstance(cases[k][t], tuple)]
        st, f = nghttp2_amd.inflate_blocks([infs[k] for k in live], [cases[k][t] for k in live])
        for i, k in enumerate(live):
            cs, cf, _ = RR.host_blocks(twins[k], [cases[k][t]])
            nomem += cs[0] == hd.NGHTTP2_ERR_NOMEM
            failed += st[i] < 0
            fields += len(f[i])
            assert (st[i], f[i]) == (cs[0], cf[0]), (k, t, cases[k][t].hex())
    assert nomem == 0
    assert failed > 300 and fields > 5000
    for k in names:
        assert [tuple(map(bytes, e)) for e in infs[k].dynamic_table()] == twins[k].table(), k
        assert infs[k].dynamic_table_size() == twins[k].table_size(), k
