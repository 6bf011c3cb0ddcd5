"""nghttp2_amd_hd_dev_fields_http (csrc/hd_fields.hip) behind the device
replay, through nghttp2_amd.DeviceInflaters: every field's check masks, name
token and nghttp2_http_on_header verdict, every block's state and result, in
device memory.

The device is compared with the host inflater (inflate_blocks with checks,
tokens and http on fresh inflaters), with the restatement of the reference's
checks and HTTP step (tests/field_checks_ref.py, tests/http_fields_ref.py) and
with the reference's recorded corpus (tests/golden/http_fields.json) -- never
with itself."""
import random

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd
from tests import field_checks_ref as FC
from tests import hd_parse_ref as P
from tests import http_fields_cases as C
from tests import http_fields_ref as R

pytestmark = pytest.mark.gpu

LEAD, TRAIL = b"\xff" * 3, b"\xff" * 40
CANARY = 0xA5
BAD = hd.NGHTTP2_ERR_INVALID_ARGUMENT
REQ, RESP, TRAILER = R.MODE_REQUEST, 0, R.MODE_TRAILER
FRESH = (0, -1, -1)

_lit = None


def huff():
    global _lit
    if _lit is None:
        _lit = C.huff_lit()
    return _lit


def _t(codec, a, dtype=None):
    a = np.array(a, dtype) if dtype is not None else np.array(a)
    return codec.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(codec.device)


def layout(codec, blocks):
    off = np.cumsum([len(LEAD)] + [len(b) for b in blocks]).astype(np.uint32)
    wire = LEAD + b"".join(blocks) + TRAIL
    return wire, _t(codec, np.frombuffer(wire, np.uint8)), _t(codec, off)


def states_tensor(codec, states):
    a = np.array([tuple(s) for s in states], dtype=hd._HTTP_STATE_DTYPE)
    return codec.torch.from_numpy(a.view(np.uint8).copy()).to(codec.device)


def dev_run(codec, s, blocks, conns, modes, states=None, **kw):
    """The chain with the annotations, read back in inflate_blocks' order."""
    wire, tw, to = layout(codec, blocks)
    kw.setdefault("checks", True)
    kw.setdefault("tokens", True)
    st = None if states is None or modes is None else states_tensor(codec, states)
    r = s.inflate(codec, tw, to, conns, wire_bytes=len(wire), http=modes, http_state=st, **kw)
    return hd.replay_annotated(r)


def host_run(nconn, blocks, conns, modes, states):
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    return infs, nghttp2_amd.inflate_blocks([infs[c] for c in conns], blocks, checks=True, tokens=True, http=modes,
                                            http_state=states)


def same(got, want):
    """Fields, statuses and the five annotation results, one by one."""
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2].tolist() == want[2].tolist()
    assert got[3].tolist() == want[3].tolist()
    assert got[4].tolist() == want[4].tolist()
    assert got[5].tolist() == want[5].tolist()  # (http_flags, status_code, content_length) per block
    assert got[6] == want[6]


def by_restatement(res, modes, states):
    """Masks, tokens and the HTTP results against the byte-level restatement
    (a block whose wire failed: the verdicts of the fields before the error,
    and the status as its result)."""
    flat = [(n, v) for fs in res[1] for n, v, _ in fs]
    assert res[2].tolist() == [[FC.mask(n), FC.mask(v)] for n, v in flat]
    assert res[3].tolist() == [hd.lookup_token(n) for n, _ in flat]
    at = 0
    for i, fs in enumerate(res[1]):
        v, st, result = R.run_block([(n, val) for n, val, _ in fs], modes[i], states[i])
        assert res[4][at:at + len(fs)].tolist() == v, i
        if res[0][i] < 0:
            assert res[6][i] == res[0][i], i
        else:
            got = res[5][i]
            assert (int(got["http_flags"]) & R.FLAGS_COMPARED, int(got["status_code"]), int(got["content_length"])) == \
                (st[0] & R.FLAGS_COMPARED, st[1], st[2]), i
            assert res[6][i] == result, i
        at += len(fs)
    assert at == len(flat)


# ---- the corpus ----

@pytest.mark.parametrize("nconn", [1, 5])
def test_corpus(codec, nconn):
    conns, wire, modes, states = C.wire(huff(), nconn)
    s = nghttp2_amd.DeviceInflaters(nconn, 4096)
    res = dev_run(codec, s, wire, conns, modes, states)
    assert all(x >= 0 for x in res[0])
    want = [f for _, _, fs in C.blocks() for f in fs]
    assert [(n, v) for fs in res[1] for n, v, _ in fs] == want
    C.check_http(res)
    assert res[2].tolist() == [[FC.mask(n), FC.mask(v)] for n, v in want]
    assert res[3].tolist() == [hd.lookup_token(n) for n, _ in want]
    infs, host = host_run(nconn, wire, conns, modes, states)
    same(res, host)
    for c in range(nconn):
        assert s.table(c) == infs[c].dynamic_table()
    assert s.fields_totals()[0] == len(want) and s.fields_totals()[2:] == [0, 0]


def _early_dynamic(block):
    """Does the block resolve a dynamic index before it inserts anything?"""
    for op in hd.parse_block(block)[1]:
        indexed = op["kind"] == hd.OP_INDEXED or (op["kind"] == hd.OP_LITERAL and not op["flags"] & hd.OP_NEW_NAME)
        if indexed and op["value"] > 61:
            return True
        if op["flags"] & hd.OP_INDEX_REQUIRED:
            return False
    return False


@pytest.mark.parametrize("cuts", [(150,), (100, 230)])
def test_carried_state(codec, cuts):
    """The corpus over two and three calls on one set: indexed fields whose
    entries an earlier call inserted get the masks, tokens and verdicts of
    the one host call."""
    nconn = 5
    conns, wire, modes, states = C.wire(huff(), nconn)
    s = nghttp2_amd.DeviceInflaters(nconn, 4096)
    _, host = host_run(nconn, wire, conns, modes, states)
    edges = [0] + list(cuts) + [len(wire)]
    parts = [dev_run(codec, s, wire[a:b], conns[a:b], modes[a:b], states[a:b]) for a, b in zip(edges, edges[1:])]
    got = (sum((p[0] for p in parts), []), sum((p[1] for p in parts), []),
           np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]),
           np.concatenate([p[4] for p in parts]), np.concatenate([p[5] for p in parts]),
           sum((p[6] for p in parts), []))
    same(got, host)
    C.check_http(got)
    for a in cuts:  # a later call's first block of a connection finds an earlier call's entry
        assert any(_early_dynamic(wire[k]) for k in range(a, a + nconn))


# ---- edges ----

def lit(name, value, first=b"\x00"):
    """a literal with a new name, both strings raw; first = 0x40 inserts"""
    return first + P.enc_int(len(name), 7) + name + P.enc_int(len(value), 7) + value


def hlit(name, value):
    """the same with the value Huffman coded (by the oracle): the wire admits
    65,536 bytes a string, so a longer value comes out of a shorter code"""
    from oracle import oracle as O
    pool = np.frombuffer(value + b"\x00", np.uint8)[:-1]
    enc, enc_off = O.encode_batch(pool, np.array([0, len(value)], np.uint32))
    code = enc.tobytes()[:int(enc_off[1])]
    return b"\x00" + P.enc_int(len(name), 7) + name + P.enc_int(len(code), 7, 0x80) + code


def req(*more):
    return lit(b":method", b"GET") + lit(b":scheme", b"https") + lit(b":path", b"/") + lit(b":authority", b"h") + \
        b"".join(more)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_block_counts(codec, n):
    """Blocks of the corpus, each on a connection of its own, at the wave
    edges of k_http_blocks; every fifth block has no field."""
    corpus = C.blocks()
    rng = random.Random(n)
    enc = [C.Encoder(rng, C.raw_lit) for _ in range(n)]
    pick = [corpus[(11 * k + n) % len(corpus)] for k in range(n)]
    modes = [m for m, _, _ in pick]
    states = [st for _, st, _ in pick]
    blocks = [enc[k].block(fs) if k % 5 != 4 else b"" for k, (_, _, fs) in enumerate(pick)]
    conns = list(range(n))
    s = nghttp2_amd.DeviceInflaters(n, 4096)
    res = dev_run(codec, s, blocks, conns, modes, states)
    same(res, host_run(n, blocks, conns, modes, states)[1])
    by_restatement(res, modes, states)


def test_edges(codec):
    big = b"a" * 70000  # (five bits a byte on the wire)
    cases = [
        # (block, mode, state)
        (b"", REQ, FRESH),                                                            # 0: no field
        (b"", RESP, FRESH),
        (lit(b"connection", b"close") + req(lit(b"x", b"y")), REQ, FRESH),            # 2: the first field fails
        (req() + b"\x80" + lit(b"never", b"seen"), REQ, FRESH),                       # 3: four fields, then index 0
        (b"\x82\x84\x80\x86", REQ, FRESH),                                            # 4: HEADER_COMP behind two fields
        (lit(b"connection", b"x") + b"\x82\x80", REQ, FRESH),                         # 5: a stream error, then HEADER_COMP
        (lit(b"x-trailer", b"1") + lit(b"te", b"trailers"), REQ | TRAILER, (R.FLAG__METHOD, -1, -1)),  # 6
        (lit(b"a", b"b") + b"\x82", REQ | TRAILER, FRESH),                            # 7: a pseudo header in a trailer
        (lit(b"Upper", b"v") + req(), REQ, FRESH),                                    # 8: -531
        (lit(b"sp ace", b"v") + req(), REQ, FRESH),                                   # 9: -105, the block goes on
        (lit(b"del\x7f", b"v") + lit(b"x" * 40 + b"Y", b"v") + req(), REQ, FRESH),    # 10: -105, then -531 late in a long name
        (lit(b"", b"v") + req(), REQ, FRESH),                                         # 11: an empty name, then pseudo headers
        (req(lit(b"", b""), lit(b"ok", b"")), REQ, FRESH),                            # 12
        (req(hlit(b"cookie", big), lit(b"content-length", b"70000"), hlit(b"x", big[:-1] + b"\x01")), REQ, FRESH),  # 13
        (lit(b":status", b"200") + hlit(b"content-length", big), RESP, FRESH),        # 14: a long value that is no number
        (lit(b":status", b"204") + lit(b"content-length", b"0"), RESP, FRESH),        # 15: -106
        (lit(b":status", b"200") + lit(b"content-length", b"0" * 30 + b"17"), RESP, (R.FLAG_METH_HEAD, -1, -1)),
        (lit(b":path", b"*") + lit(b":method", b"OPTIONS") + lit(b":scheme", b"http") + lit(b"host", b"h"), REQ, FRESH),
        (lit(b":method", b"CONNECT") + lit(b":authority", b"h:1"), REQ, FRESH),
        (lit(b":method", b"CONNECT") + lit(b":authority", b"h:1"), REQ | R.MODE_PUSH, FRESH),
        (req(lit(b"priority", b"\x01")), REQ, FRESH),
        (req(lit(b"v", b" lead")), REQ, FRESH),
        (req(lit(b"v", b" lead")), REQ | R.MODE_NO_RFC9113_WS, FRESH),
        (lit(b":status", b"200") + hlit(b"content-length", b"0" * 69999 + b"7"), RESP, FRESH),  # 23: and one that is
    ]
    blocks = [c[0] for c in cases]
    modes = [c[1] for c in cases]
    states = [c[2] for c in cases]
    n = len(cases)
    conns = list(range(n))
    s = nghttp2_amd.DeviceInflaters(n, 4096)
    res = dev_run(codec, s, blocks, conns, modes, states)
    same(res, host_run(n, blocks, conns, modes, states)[1])
    st, f, masks, toks, verd, state, bhttp = res
    off = np.cumsum([0] + [len(x) for x in f]).tolist()

    def v(i):
        return verd[off[i]:off[i + 1]].tolist()

    def state_of(i):
        return tuple(int(state[i][k]) for k in ("http_flags", "status_code", "content_length"))

    assert st[0] == 0 and bhttp[:2] == [R.MESSAGING, R.MESSAGING] and state_of(0) == FRESH
    assert v(2) == [R.ERR] + [R.NOT_EXAMINED] * 5 and bhttp[2] == R.ERR
    assert state_of(2) == (R.FLAG_PSEUDO_HEADER_DISALLOWED, -1, -1)  # frozen at the failed field
    assert st[3] == st[4] == st[5] == R.HEADER_COMP
    assert v(3) == [0, 0, 0, 0] and bhttp[3] == R.HEADER_COMP
    assert v(4) == [0, 0] and bhttp[4] == R.HEADER_COMP
    assert state_of(4) == (R.FLAG__METHOD | R.FLAG__PATH | R.FLAG_PATH_REGULAR, -1, -1)
    assert v(5) == [R.ERR, R.NOT_EXAMINED] and bhttp[5] == R.HEADER_COMP
    assert v(6) == [0, 0] and bhttp[6] == 0 and v(7) == [0, R.ERR] and bhttp[7] == R.ERR
    assert v(8)[0] == R.ERR and v(9)[0] == R.IGN and v(9)[1:] == [R.ERR] + [R.NOT_EXAMINED] * 3
    assert v(10)[:2] == [R.IGN, R.ERR]
    assert v(11)[:2] == [R.IGN, R.ERR] and v(12)[4:] == [R.IGN, 0] and bhttp[12] == 0
    assert v(13) == [0] * 6 + [R.IGN] and state_of(13)[2] == 70000 and bhttp[13] == 0
    assert v(14) == [0, R.ERR] and v(15) == [0, R.REMOVE] and state_of(16)[2] == 0
    assert len(f[13][4][1]) == 70000 and v(23) == [0, 0] and state_of(23)[1:] == (200, 7)
    by_restatement(res, modes, states)


def test_informational_response_feeds_the_next_block(codec):
    """A 1xx block's state, still on the device, is the next call's input."""
    s = nghttp2_amd.DeviceInflaters(1, 4096)
    first = [lit(b":status", b"103") + lit(b"link", b"</a>")]
    wire, tw, to = layout(codec, first)
    start = states_tensor(codec, [(R.FLAG_METH_HEAD, -1, -1)])
    r1 = s.inflate(codec, tw, to, [0], wire_bytes=len(wire), http=[RESP], http_state=start)
    second = [lit(b":status", b"200") + lit(b"content-length", b"12")]
    wire, tw, to = layout(codec, second)
    r2 = s.inflate(codec, tw, to, [0], wire_bytes=len(wire), http=_t(codec, [RESP], np.uint8), http_state=r1.http_state,
                   checks=True, tokens=True)
    a, b = hd.replay_annotated(r1), hd.replay_annotated(r2)
    after_1xx = (R.FLAG_METH_HEAD | R.FLAG_EXPECT_FINAL_RESPONSE, -1, -1)
    assert a[2].tolist() == [0, 0] and a[3].tolist() == [after_1xx] and a[4] == [0]
    assert start.cpu().numpy().view(hd._HTTP_STATE_DTYPE).tolist() == [(R.FLAG_METH_HEAD, -1, -1)]  # the input stays
    infs = [nghttp2_amd.HpackInflater()]
    h1 = nghttp2_amd.inflate_blocks(infs, first, http=[RESP], http_state=[(R.FLAG_METH_HEAD, -1, -1)])
    h2 = nghttp2_amd.inflate_blocks(infs, second, checks=True, tokens=True, http=[RESP], http_state=[after_1xx])
    assert a[2].tolist() == h1[2].tolist() and a[3].tolist() == h1[3].tolist() and a[4] == h1[4]
    same(b, h2)
    # HEAD: no body is expected whatever content-length says
    assert b[5].tolist() == [(R.FLAG_METH_HEAD | R.FLAG__STATUS | R.FLAG_PSEUDO_HEADER_DISALLOWED, 200, 0)]


# ---- subsets, canaries, caps: the C call on a replay's tensors ----

def replayed(codec, s, blocks, conns, **kw):
    wire, tw, to = layout(codec, blocks)
    return s.inflate(codec, tw, to, conns, wire_bytes=len(wire), **kw)


def fields_raw(codec, r, n, nva_cap, chk=None, tok=None, modes=None, states=None, verd=None, bhttp=None,
               arena_bytes=None, ws=None, expect=0):
    torch = codec.torch
    L = hd._replay_lib()
    need = L.nghttp2_amd_hd_dev_fields_http_workspace_size(nva_cap, n)
    if ws is None:
        ws = torch.full((need,), CANARY, dtype=torch.uint8, device=codec.device)
    if arena_bytes is None:
        arena_bytes = r.arena.untyped_storage().nbytes()
    rv = L.nghttp2_amd_hd_dev_fields_http(
        hd._p(r.nva), nva_cap, hd._p(r.arena), arena_bytes, hd._p(r.block_nv_off), hd._p(r.status), hd._p(r.totals), n,
        hd._p(chk), hd._p(tok), hd._p(modes), hd._p(states), hd._p(verd), hd._p(bhttp), hd._p(ws), ws.numel(),
        hd._stream(None))
    assert rv == expect
    torch.cuda.synchronize()
    t = np.zeros(4, np.uint32)
    assert L.nghttp2_amd_hd_dev_fields_http_totals(hd._p(ws), t.ctypes.data, hd._stream(None)) == 0
    return t.tolist()


def canary(codec, nbytes):
    return codec.torch.full((nbytes,), CANARY, dtype=codec.torch.uint8, device=codec.device)


def intact(t, start=0):
    return bool((t.cpu().numpy().view(np.uint8)[start:] == CANARY).all())


def _sample():
    """40 corpus blocks on four connections, raw and Huffman literals mixed."""
    conns, wire, modes, states = C.wire(huff(), 4)
    k = slice(0, 40)
    return conns[k], wire[k], modes[k], states[k]


@pytest.mark.parametrize("tight", [True, False])
def test_subsets_and_canaries(codec, tight):
    """checks only, tokens only and http only equal the full call's arrays;
    nothing is written past the field count, with nva_cap at the count and
    with one far above it."""
    torch = codec.torch
    conns, wire, modes, states = _sample()
    n = len(wire)
    _, host = host_run(4, wire, conns, modes, states)
    nf = len(host[3])
    s = nghttp2_amd.DeviceInflaters(4, 4096)
    r = replayed(codec, s, wire, conns)
    assert r.nva.numel() // 24 > 4 * nf
    nva_cap = nf if tight else r.nva.numel() // 24
    room = nva_cap + 64
    m = _t(codec, modes, np.uint8)

    def outputs():
        return canary(codec, 2 * room), canary(codec, 4 * room).view(torch.int32), \
            canary(codec, 4 * room).view(torch.int32), canary(codec, 4 * n + 64).view(torch.int32)

    chk, tok, verd, bhttp = outputs()
    st = states_tensor(codec, states)
    tot = fields_raw(codec, r, n, nva_cap, chk, tok, m, st, verd, bhttp)
    assert tot == [nf, int(r.totals[1].item()), 0, 0]
    full = (chk.cpu().numpy()[:2 * nf].reshape(-1, 2), tok.cpu().numpy()[:nf], verd.cpu().numpy()[:nf],
            st.cpu().numpy().view(hd._HTTP_STATE_DTYPE), bhttp.cpu().numpy()[:n].tolist())
    for got, want in zip(full, host[2:]):
        assert (got == want) if isinstance(want, list) else got.tolist() == want.tolist()
    assert intact(chk, 2 * nf) and intact(tok, 4 * nf) and intact(verd, 4 * nf) and intact(bhttp, 4 * n)
    # checks only
    chk2, tok2, verd2, bhttp2 = outputs()
    fields_raw(codec, r, n, nva_cap, chk=chk2)
    assert torch.equal(chk2, chk) and intact(tok2) and intact(verd2) and intact(bhttp2)
    # tokens only
    chk2, tok2, verd2, bhttp2 = outputs()
    fields_raw(codec, r, n, nva_cap, tok=tok2)
    assert torch.equal(tok2, tok) and intact(chk2) and intact(verd2) and intact(bhttp2)
    # http only; and http without the two optional outputs
    chk2, tok2, verd2, bhttp2 = outputs()
    st2 = states_tensor(codec, states)
    fields_raw(codec, r, n, nva_cap, modes=m, states=st2, verd=verd2, bhttp=bhttp2)
    assert torch.equal(verd2, verd) and torch.equal(bhttp2, bhttp) and torch.equal(st2, st)
    assert intact(chk2) and intact(tok2)
    st3 = states_tensor(codec, states)
    fields_raw(codec, r, n, nva_cap, modes=m, states=st3)
    assert torch.equal(st3, st)
    # nothing asked for: nothing queued, not even the totals word
    ws = canary(codec, hd._replay_lib().nghttp2_amd_hd_dev_fields_http_workspace_size(nva_cap, n))
    fields_raw(codec, r, n, nva_cap, ws=ws)
    assert intact(ws)


def test_overflow_and_short_arena(codec):
    torch = codec.torch
    conns, wire, modes, states = _sample()
    n = len(wire)
    _, host = host_run(4, wire, conns, modes, states)
    nf = len(host[3])
    nb = sum(len(a) + len(b) + 2 for fs in host[1] for a, b, _ in fs)
    m = _t(codec, modes, np.uint8)

    def run(r, **kw):
        out = canary(codec, 2 * nf), canary(codec, 4 * nf), canary(codec, 4 * nf), canary(codec, 4 * n)
        st = states_tensor(codec, states)
        tot = fields_raw(codec, r, n, nf, out[0], out[1].view(torch.int32), m, st, out[2].view(torch.int32),
                         out[3].view(torch.int32), **kw)
        untouched = all(intact(x) for x in out) and torch.equal(st, states_tensor(codec, states))
        return tot, untouched, out, st

    # the arena one byte short: the replay wrote no field, and neither does this call
    s = nghttp2_amd.DeviceInflaters(4, 4096)
    before = [s.state(c) for c in range(4)]
    r = replayed(codec, s, wire, conns, arena_cap=nb - 1)
    assert r.totals.cpu().numpy().view(np.uint32).tolist() == [nf, nb, hd.DEV_OVERFLOW_ARENA, 0]
    tot, untouched, _, _ = run(r)
    assert tot == [0, 0, hd.DEV_FIELDS_NOT_REPLAYED, 0] and untouched
    assert [s.state(c) for c in range(4)] == before
    res = dev_run(codec, s, wire, conns, modes, states)  # the tables are as before: the same call with room
    same(res, host)
    # the wrapper's retry repeats the annotation with the replay: 200 references
    # to a 3,000-byte entry outgrow its first arena of four times the wire
    blocks = [lit(b"big", b"v" * 3000, b"\x40"), b"\xbe" * 200]
    s1 = nghttp2_amd.DeviceInflaters(1, 4096)
    res = dev_run(codec, s1, blocks, [0, 0], [REQ | TRAILER] * 2, [FRESH] * 2)
    assert res[0] == [1, 200] and 4 * sum(map(len, blocks)) + 4096 < 200 * 3000
    same(res, host_run(1, blocks, [0, 0], [REQ | TRAILER] * 2, [FRESH] * 2)[1])
    # arena_bytes below the pool rule: nothing is examined; at the rule: everything
    s = nghttp2_amd.DeviceInflaters(4, 4096)
    r = replayed(codec, s, wire, conns, arena_cap=nb)
    rule = (nb + 15) // 16 * 16 + 16
    assert r.arena.untyped_storage().nbytes() >= rule
    tot, untouched, _, _ = run(r, arena_bytes=rule - 1)
    assert tot == [0, 0, hd.DEV_FIELDS_ARENA_SHORT, 0] and untouched
    tot, untouched, out, st = run(r, arena_bytes=rule)
    assert tot == [nf, nb, 0, 0] and not untouched
    assert out[0].cpu().numpy().reshape(-1, 2).tolist() == host[2].tolist()
    assert out[2].cpu().numpy().view(np.int32).tolist() == host[4].tolist()
    assert st.cpu().numpy().view(hd._HTTP_STATE_DTYPE).tolist() == host[5].tolist()


def test_arguments(codec):
    torch = codec.torch
    L = hd._replay_lib()
    conns, wire, modes, states = _sample()
    n = len(wire)
    s = nghttp2_amd.DeviceInflaters(4, 4096)
    r = replayed(codec, s, wire, conns)
    cap = 64
    need = L.nghttp2_amd_hd_dev_fields_http_workspace_size(cap, n)
    t = torch.zeros(1 << 14, dtype=torch.int32, device=codec.device)
    p = hd._p(t)
    assert need <= 4 * t.numel()
    full = [hd._p(r.nva), cap, hd._p(r.arena), r.arena.untyped_storage().nbytes(), hd._p(r.block_nv_off),
            hd._p(r.status), hd._p(r.totals), n, p, p, p, p, p, p, p, need, None]
    assert L.nghttp2_amd_hd_dev_fields_http(*full) == 0
    for k in (0, 2, 4, 5, 6, 14):  # nva, arena, block_nv_off, out_status, out_totals, workspace
        a = list(full)
        a[k] = None
        assert L.nghttp2_amd_hd_dev_fields_http(*a) == BAD, k
    for k in (10, 11):  # the modes without the states, the states without the modes
        a = list(full)
        a[k] = None
        assert L.nghttp2_amd_hd_dev_fields_http(*a) == BAD, k
        a[12] = a[13] = None
        assert L.nghttp2_amd_hd_dev_fields_http(*a) == BAD, k
    a = list(full)
    a[10] = a[11] = None  # verdicts or results asked for without modes and states
    assert L.nghttp2_amd_hd_dev_fields_http(*a) == BAD
    a[12] = a[13] = None  # masks and tokens only
    assert L.nghttp2_amd_hd_dev_fields_http(*a) == 0
    a = list(full)
    a[15] = need - 1
    assert L.nghttp2_amd_hd_dev_fields_http(*a) == BAD
    a = list(full)
    a[2] = hd.ctypes.c_void_p(r.arena.data_ptr() + 8)  # the arena is 16-byte aligned
    assert L.nghttp2_amd_hd_dev_fields_http(*a) == BAD
    a = [None] * 17
    a[1] = a[3] = a[7] = a[15] = 0
    assert L.nghttp2_amd_hd_dev_fields_http(*a) == 0  # nblocks == 0 touches nothing
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        replayed(codec, s, wire, conns, http=modes[:-1])


def test_two_calls_queued(codec):
    """Two chains with the annotation call at their ends, queued on one
    stream with no host synchronisation between them (wire, offsets, CSR,
    modes and states are on the device before the first; the literal counts
    and the arena's size come from the host): both equal the host's, and the
    second resolves entries the first inserted."""
    torch = codec.torch
    nconn = 5
    conns, wire, modes, states = C.wire(huff(), nconn)
    cut = 150
    _, host = host_run(nconn, wire, conns, modes, states)
    res = []
    for sync in (None, False, True):  # None: the run that warms the allocator
        s = nghttp2_amd.DeviceInflaters(nconn, 4096)
        ready = []
        for a, b in ((0, cut), (cut, len(wire))):
            w, tw, to = layout(codec, wire[a:b])
            nlits = int(sum((ops["name_lit"] >= 0).sum() + (ops["value_lit"] >= 0).sum()
                            for ops in (hd.parse_block(x)[1] for x in wire[a:b])))
            ready.append((len(w), tw, to, s.csr(conns[a:b]), nlits, _t(codec, modes[a:b], np.uint8),
                          states_tensor(codec, states[a:b])))
        torch.cuda.synchronize()
        out = []
        for nbytes, tw, to, csr, T, m, st in ready:  # nothing but launches from here on
            out.append(s.inflate(codec, tw, to, None, wire_bytes=nbytes, nlits=T, arena_cap=1 << 16, csr=csr,
                                 checks=True, tokens=True, http=m, http_state=st))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        res.append([hd.replay_annotated(r) for r in out])
    for parts in res[1:]:
        got = (parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]) + \
            tuple(np.concatenate([parts[0][k], parts[1][k]]) for k in (2, 3, 4, 5)) + (parts[0][6] + parts[1][6],)
        same(got, host)
    assert any(_early_dynamic(wire[k]) for k in range(cut, cut + nconn))
