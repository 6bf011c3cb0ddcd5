"""The inflater's annotation levels against each other, without a GPU (raw
literals only): a plain call, checks, tokens, checks + tokens, and http.

An entry of the dynamic table carries what the call that inserted it computed
of its bytes; a later call that wants more fills the rest in at the first
reference.  So every ordered pair of levels (A, B) is run: block 1 at level A
inserts, block 2 at level B references the entries every way the wire can.
The checkers are the project's restatements, each pinned to the reference by
golden files: tests/field_checks_ref.py (masks), hd.lookup_token (tokens),
tests/http_fields_ref.py (verdicts, states, block results) and the oracle's
inflater (fields, statuses, dynamic tables)."""
import ctypes

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd as H
from oracle import hpack_oracle as HO
from tests import field_checks_ref as FC
from tests import http_fields_ref as R
from tests.http_fields_cases import hpack_int, raw_lit

BUFFER_ERROR = H.NGHTTP2_ERR_BUFFER_ERROR
LEVELS = {"plain": {}, "checks": {"checks": True}, "tokens": {"tokens": True},
          "checks+tokens": {"checks": True, "tokens": True},
          "http": {"checks": True, "tokens": True, "http": True}}
PAIRS = [(a, b) for a in LEVELS for b in LEVELS]
FRESH = (0, -1, -1)

# What block 1 inserts, per connection: names with a token and without,
# values with a number, "trailers", a bad byte; the fields that end a block's
# examination (an upper-case name, a connection-specific field) come last.
ENTRIES = [
    [(b":method", b"HEAD"), (b"content-length", b"0042"), (b"te", b"TrAiLeRs"), (b"x-custom", b"v\x01bad"),
     (b"priority", b"u=1"), (b"bad name", b"x"), (b"Upper-Name", b"ok"), (b"connection", b"close")],
    [(b":status", b"204"), (b"content-length", b"0"), (b"x-custom", b" lead"), (b"te", b"gzip"),
     (b"host", b"user@host"), (b"", b"empty-name"), (b"transfer-encoding", b"chunked")],
]
MODES = [R.MODE_REQUEST, 0]


def indexed(i):
    return hpack_int(i, 7, 0x80)


def block1(c):
    return b"".join(b"\x40" + raw_lit(n) + raw_lit(v) for n, v in ENTRIES[c])


def block2(c):
    """Every entry of block 1 fully indexed, then by name with a literal value
    (with indexing, without, never indexed), static entries both ways, new
    names; the insertions of this block shift the later indices."""
    n = len(ENTRIES[c])
    out = [indexed(62 + n - 1 - k) for k in range(n)]                 # dynamic, fully indexed
    out += [indexed(2), indexed(8), indexed(28), indexed(61)]          # static, fully indexed
    out.append(hpack_int(62 + n - 2, 6, 0x40) + raw_lit(b"7"))        # entry 1's name, inserted: one more entry
    out.append(hpack_int(62 + n + 1 - 1, 4, 0x00) + raw_lit(b"trailers"))  # entry 0's name, not indexed
    out.append(hpack_int(62, 4, 0x10) + raw_lit(b"99999999999999999999"))  # the newest entry's name, never indexed
    out.append(hpack_int(28, 6, 0x40) + raw_lit(b"12"))               # a static name, inserted
    out.append(hpack_int(58, 4, 0x00) + raw_lit(b"bad\x7fbyte"))      # a static name, not indexed
    out.append(b"\x40" + raw_lit(b"x-new") + raw_lit(b"trailers"))    # new names
    out.append(b"\x00" + raw_lit(b":protocol") + raw_lit(b"websocket"))
    out.append(b"\x10" + raw_lit(b"X-Upper") + raw_lit(b"\x00"))
    out += [indexed(62), indexed(63), indexed(64)]                     # what this block inserted
    return b"".join(out)


def call(level, infs, blocks, modes, **kw):
    kw.update(LEVELS[level])
    if kw.pop("http", False):
        kw["http"] = modes
    return nghttp2_amd.inflate_blocks(infs, blocks, **kw)


def check(level, res, want, modes, cut=0):
    """res of a call at `level` against want = [(status, fields)] of the
    oracle, one per block the call applied; `cut` more blocks were cut off."""
    lv = LEVELS[level]
    assert len(res) == 2 + sum(3 if k == "http" else 1 for k in lv)
    assert res[0] == [s for s, _ in want] + [BUFFER_ERROR] * cut
    assert res[1] == [f for _, f in want] + [[]] * cut
    flat = [(n, v) for _, fs in want for n, v, _ in fs]
    at = 2
    if "checks" in lv:
        assert res[at].tolist() == [[FC.mask(n), FC.mask(v)] for n, v in flat]
        at += 1
    if "tokens" in lv:
        assert res[at].tolist() == [H.lookup_token(n) for n, _ in flat]
    if "http" in lv:
        runs = [R.run_block([(n, v) for n, v, _ in fs], m, FRESH) for (_, fs), m in zip(want, modes)]
        assert res[-3].tolist() == [v for r in runs for v in r[0]]
        got = [(int(f) & R.FLAGS_COMPARED, int(s), int(c)) for f, s, c in res[-2].tolist()]
        assert got == [(r[1][0] & R.FLAGS_COMPARED,) + r[1][1:] for r in runs] + [FRESH] * cut
        assert res[-1] == [r[2] for r in runs] + [BUFFER_ERROR] * cut


class Conns:
    """The two connections, here and in the oracle."""

    def __init__(self):
        self.infs = [nghttp2_amd.HpackInflater() for _ in ENTRIES]
        self.ref = [HO.Inflater() for _ in ENTRIES]

    def run(self, level, conns, blocks, **kw):
        """One call over blocks[i] on connection conns[i], checked."""
        modes = [MODES[c] for c in conns]
        res = call(level, [self.infs[c] for c in conns], blocks, modes, **kw)
        check(level, res, [self.ref[c].inflate_block(b) for c, b in zip(conns, blocks)], modes)

    def tables_equal(self):
        for a, b in zip(self.infs, self.ref):
            assert a.dynamic_table() == b.table
            assert a.dynamic_table_size() == b.size


# one connection a call: the direct sink; both in one call: the per-block sinks
SHAPES = {"direct": [[0], [1]], "grouped": [[0, 1]]}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("a,b", PAIRS)
def test_level_matrix(a, b, shape):
    cs = Conns()
    for level, block in ((a, block1), (b, block2)):
        for conns in SHAPES[shape]:
            cs.run(level, conns, [block(c) for c in conns])
        cs.tables_equal()


def test_the_blocks_cover_every_verdict():
    seen = set()
    for c, mode in enumerate(MODES):
        ref = HO.Inflater()
        for block in (block1(c), block2(c)):
            st, fs = ref.inflate_block(block)
            assert st == len(fs) > 0
            seen |= set(R.run_block([(n, v) for n, v, _ in fs], mode, FRESH)[0])
    assert seen == {0, R.IGN, R.REMOVE, R.ERR, R.NOT_EXAMINED}


def _size(fields):
    return len(fields), sum(len(n) + len(v) + 2 for n, v, _ in fields)


@pytest.mark.parametrize("a,b", PAIRS)
def test_cut_at_level_b_direct(a, b):
    """One connection: block 2 does not fit (a field, or a byte, too few), so it
    is replayed into scratch, the table restored and the batch cut there."""
    cs = Conns()
    cs.run(a, [0], [block1(0)])
    ref2 = HO.Inflater()
    ref2.inflate_block(block1(0))
    nf, nbytes = _size(ref2.inflate_block(block2(0))[1])
    for caps in ({"nva_cap": nf - 1, "arena_cap": nbytes}, {"nva_cap": nf, "arena_cap": nbytes - 1}):
        res = call(b, [cs.infs[0]], [block2(0)], [MODES[0]], retry=False, **caps)
        check(b, res, [], [], cut=1)
        cs.tables_equal()  # block 2 is unapplied
    cs.run(b, [0], [block2(0)], nva_cap=nf, arena_cap=nbytes)  # the retry: as uncut
    cs.tables_equal()


@pytest.mark.parametrize("a,b", PAIRS)
def test_cut_at_level_b_grouped(a, b):
    """Two connections: the second one's block 2 does not fit, so the tables
    are restored from their snapshots and the first one's block re-applied."""
    cs = Conns()
    cs.run(a, [0, 1], [block1(0), block1(1)])
    want0 = cs.ref[0].inflate_block(block2(0))
    ref1 = HO.Inflater()
    ref1.inflate_block(block1(1))
    sizes = [_size(want0[1]), _size(ref1.inflate_block(block2(1))[1])]
    nf, nbytes = sizes[0][0] + sizes[1][0], sizes[0][1] + sizes[1][1]
    modes = [MODES[0], MODES[1]]
    res = call(b, cs.infs, [block2(0), block2(1)], modes, retry=False, nva_cap=nf - 1, arena_cap=nbytes - 1)
    check(b, res, [want0], modes, cut=1)
    cs.tables_equal()  # connection 0 after block 2, connection 1 still after block 1
    cs.run(b, [1], [block2(1)])  # the retry: as uncut
    cs.tables_equal()


# ---- the four C entry points on one batch
def _c_call(name, nargs):
    """The entry point `name` over blocks 1 and 2 of both connections on fresh
    inflaters, with its first nargs optional arrays: the call's results by name."""
    L = H._inflate_lib()
    conns = [0, 1, 0, 1]
    wire = [block1(0), block1(1), block2(0), block2(1)]
    fresh = [nghttp2_amd.HpackInflater() for _ in ENTRIES]
    nb, cap = len(wire), 256
    bufs = [ctypes.create_string_buffer(b, len(b)) for b in wire]
    ptrs = (ctypes.c_void_p * nb)(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_size_t * nb)(*[len(b) for b in wire])
    ips = (ctypes.c_void_p * nb)(*[fresh[c].p.value for c in conns])
    nva = np.zeros(cap, dtype=H._NV_DTYPE)
    arena = np.zeros(1 << 14, dtype=np.uint8)
    status = np.zeros(nb, dtype=np.int32)
    states = np.empty(nb, dtype=H._HTTP_STATE_DTYPE)
    states[:] = FRESH
    opt = [("checks", np.zeros((cap, 2), dtype=np.uint8)), ("tokens", np.zeros(cap, dtype=np.int32)),
           ("modes", np.array([MODES[c] for c in conns], dtype=np.uint8)), ("states", states),
           ("verdicts", np.zeros(cap, dtype=np.int32)), ("block_http", np.zeros(nb, dtype=np.int32))][:nargs]
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    vp = ctypes.c_void_p
    rv = getattr(L, name)(ips, nb, ptrs, lens, vp(nva.ctypes.data), cap, ctypes.byref(nv_used),
                          vp(arena.ctypes.data), arena.size, ctypes.byref(ar_used), vp(status.ctypes.data),
                          *[vp(a.ctypes.data) for _, a in opt], None)
    out = {"rv": rv, "nv_used": nv_used.value, "ar_used": ar_used.value, "arena": arena.tobytes(),
           "status": status.tolist(), "tables": [i.dynamic_table() for i in fresh]}
    out.update({f: nva[f].tolist() for f in H._NV_DTYPE.names})
    out.update({k: a.tolist() for k, a in opt})
    return out


def test_entry_points_agree():
    """Every array two of the four entry points share is equal: each is the
    _http call with NULL for the arrays it lacks."""
    calls = [_c_call("nghttp2_amd_hd_inflate_blocks", 0), _c_call("nghttp2_amd_hd_inflate_blocks_checked", 1),
             _c_call("nghttp2_amd_hd_inflate_blocks_fields", 2), _c_call("nghttp2_amd_hd_inflate_blocks_http", 6)]
    full = calls[-1]
    assert full["rv"] == 0 and full["nv_used"] == sum(s for s in full["status"]) > 40
    assert [len(c) for c in calls] == [12, 13, 14, 18]
    for c in calls[:-1]:
        assert c == {k: full[k] for k in c}
