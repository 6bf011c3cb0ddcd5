"""nghttp2_amd_hd_dev_inflate_blocks and the device-resident inflaters
(csrc/hd_replay.hip) through nghttp2_amd.DeviceInflaters: parse -> gather ->
decode_auto -> replay with the tables in device memory across calls.

The device is compared with the host twin (nghttp2_amd_hd_replay_host, held
to the Python restatement and the recorded reference in
tests/test_replay_host.py), with the host inflater (inflate_blocks) and with
the reference's recorded results -- never with itself."""
import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import hd
from tests import hd_parse_ref as P
from tests import hd_replay_ref as R
from tests import ref_hd_wire_lib as W

pytestmark = pytest.mark.gpu

LEAD, TRAIL = b"\xff" * 3, b"\xff" * 40
CANARY = 0xA5
COMP, NOMEM = hd.NGHTTP2_ERR_HEADER_COMP, hd.NGHTTP2_ERR_NOMEM


def _t(codec, a, dtype=None):
    a = np.array(a, dtype) if dtype is not None else np.array(a)
    return codec.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(codec.device)


def layout(codec, blocks):
    off = np.cumsum([len(LEAD)] + [len(b) for b in blocks]).astype(np.uint32)
    wire = LEAD + b"".join(blocks) + TRAIL
    return wire, _t(codec, np.frombuffer(wire, np.uint8)), _t(codec, off)


def dev_run(codec, s, blocks, conns, **kw):
    """The whole chain on the device: (status, fields, out_totals)."""
    wire, tw, to = layout(codec, blocks)
    r = s.inflate(codec, tw, to, conns, wire_bytes=len(wire), **kw)
    st, f = hd.replay_fields(r.nva, r.arena, r.block_nv_off, r.status)
    return st, f, r.totals.cpu().numpy().view(np.uint32).tolist()


def twin_run(twins, blocks, conns):
    """The same batch on host twins, connection by connection (each one's
    blocks in one call), scattered back to block order."""
    st, f = [None] * len(blocks), [None] * len(blocks)
    for c in sorted(set(conns)):
        mine = [k for k, x in enumerate(conns) if x == c]
        s, ff, _ = R.host_blocks(twins[c], [blocks[k] for k in mine])
        for k, a, b in zip(mine, s, ff):
            st[k], f[k] = a, b
    return st, f


def check_states(s, twins, conns=None):
    for c in (range(len(twins)) if conns is None else conns):
        assert s.state(c) == R.host_state(twins[c]), c


def both(codec, s, twins, blocks, conns, **kw):
    st, f, totals = dev_run(codec, s, blocks, conns, **kw)
    ws, wf = twin_run(twins, blocks, conns)
    for k in range(len(blocks)):
        assert (st[k], f[k]) == (ws[k], wf[k]), (k, conns[k], blocks[k].hex()[:80])
    assert totals[0] == sum(len(x) for x in wf) and totals[2:] == [0, 0]
    assert totals[1] == sum(len(n) + len(v) + 2 for x in wf for n, v, _ in x)
    return st, f


def test_recorded_reference(codec):
    """All 322 inflate connections of the fixture in one set, one block per
    connection per call (product_inflate_batched's round robin), the ichange
    steps through change_table_size in their places."""
    conns = W.connections(side="i")
    assert len(conns) == 322
    s = nghttp2_amd.DeviceInflaters(len(conns), 4096)
    pos = [0] * len(conns)
    last = [([], 0, 4096)] * len(conns)
    ninf = nchg = 0

    def steps_left(ci, op):
        st = conns[ci]["steps"]
        while pos[ci] < len(st) and st[pos[ci]]["op"] not in ("ichange", "inflate"):
            pos[ci] += 1
        return pos[ci] < len(st) and st[pos[ci]]["op"] == op

    while True:
        while True:  # the changes in front of the next blocks, one per connection and call
            todo = [ci for ci in range(len(conns)) if steps_left(ci, "ichange")]
            if not todo:
                break
            rv = s.change_table_size(todo, [conns[ci]["steps"][pos[ci]]["v"] for ci in todo]).cpu().tolist()
            for ci, r in zip(todo, rv):
                step = conns[ci]["steps"][pos[ci]]
                assert r == step["rv"], W.where(conns[ci], pos[ci])
                last[ci] = (step["itable"], step["isize"], step["imax"])
                assert s.state(ci)[:3] == last[ci], W.where(conns[ci], pos[ci])
                pos[ci] += 1
                nchg += 1
        todo = [ci for ci in range(len(conns)) if steps_left(ci, "inflate")]
        if not todo:
            break
        st, f, totals = dev_run(codec, s, [conns[ci]["steps"][pos[ci]]["wire"] for ci in todo], todo)
        assert totals[2] == 0
        for k, ci in enumerate(todo):
            step = conns[ci]["steps"][pos[ci]]
            fields = [(n, v, fl, hd.lookup_token(n)) for n, v, fl in f[k]]
            W.check_inflate_result(step, st[k], fields, W.where(conns[ci], pos[ci]))
            last[ci] = (step["itable"], step["isize"], step["imax"])
            pos[ci] += 1
            ninf += 1
        for ci in range(len(conns)):  # every connection, the ones without a block too
            assert s.state(ci)[:3] == last[ci], conns[ci]["name"]
    assert (ninf, nchg) == (881, 255)


def test_many_blocks_per_connection(codec):
    """Random connections (six blocks each in one call, some corrupted) and
    every placed edge on a connection of its own: equal to inflate_blocks on
    fresh host inflaters and to the host twin, fields and final tables."""
    order, blocks = P.random_blocks(0xE2E, 12, 6, corrupt=0.12)
    edges = [b for _, b in P.edge_blocks()]
    conns = order + list(range(12, 12 + len(edges)))
    blocks = blocks + edges
    nconn, tb = 12 + len(edges), 1 << 17  # (65536-byte literals enter tables)
    s = nghttp2_amd.DeviceInflaters(nconn, tb)
    twins = [hd.HostReplayInflater(tb) for _ in range(nconn)]
    st, f = both(codec, s, twins, blocks, conns)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    hs, hf = nghttp2_amd.inflate_blocks([infs[c] for c in conns], blocks)
    assert (st, f) == (hs, hf)
    for c in range(nconn):
        table, size, mx, _ = s.state(c)
        assert (table, size, mx) == (infs[c].dynamic_table(), infs[c].dynamic_table_size(),
                                     infs[c].max_dynamic_table_size()), c
    check_states(s, twins)
    fails = sum(x < 0 for x in st[:len(order)])
    assert 0 < fails < len(order) // 2


@pytest.mark.parametrize("nconn", [1, 63, 64, 65, 129])
def test_shapes(codec, nconn):
    """Connections without a block at the wave edges, empty blocks, and two
    calls so every table is carried once."""
    _, rnd = P.random_blocks(0x5A + nconn, 4, 8, corrupt=0.2)
    idle = {0, 62, 63, 64, 65, 127, 128, nconn - 1} if nconn > 1 else set()
    conns = [c for c in range(nconn) if c not in idle for _ in range(1 + c % 3)]
    conns = conns[::2] + conns[1::2]  # a connection's blocks are not neighbours
    s = nghttp2_amd.DeviceInflaters(nconn, 4096)
    twins = [hd.HostReplayInflater(4096) for _ in range(nconn)]
    for call in range(2):
        blocks = [rnd[(7 * k + call) % len(rnd)] if k % 5 else b"" for k in range(len(conns))]
        both(codec, s, twins, blocks, conns)
        check_states(s, twins)


def test_only_size_updates_and_one_block(codec):
    s = nghttp2_amd.DeviceInflaters(3, 4096)
    twins = [hd.HostReplayInflater(4096) for _ in range(3)]
    st, f = both(codec, s, twins, [R.size(100), R.size(0) + R.size(50), b""], [0, 2, 2])
    assert st == [0, 0, 0] and f == [[], [], []]
    check_states(s, twins)
    assert s.table_max(0) == 100 and s.table_max(2) == 50 and s.table_max(1) == 4096
    st, f = both(codec, s, twins, [R.ins(b"n", b"v") + b"\xbe"], [1])  # nblocks == 1
    assert st == [2] and s.table(1) == [(b"n", b"v")] and s.table_size(1) == 34


@pytest.mark.parametrize("name", sorted(R.RULES))
def test_rule(codec, name):
    """Every rule's steps, a call per step, beside an idle connection."""
    s = nghttp2_amd.DeviceInflaters(2, 4096)
    twins = [hd.HostReplayInflater(4096) for _ in range(2)]
    for step in R.RULES[name]:
        if isinstance(step, tuple):
            assert s.change_table_size([1], [step[1]]).cpu().tolist() == [twins[1].change_table_size(step[1])]
        else:
            both(codec, s, twins, [step], [1])
        check_states(s, twins)


def test_state_across_calls(codec):
    s = nghttp2_amd.DeviceInflaters(4, 4096)
    twins = [hd.HostReplayInflater(4096) for _ in range(4)]
    huff = b"\x40" + P.huff_lit(5) + P.huff_lit(7)
    # call 1 inserts (raw and Huffman), call 2 references: reads the flipped store
    both(codec, s, twins, [R.ins(b"name", b"value"), huff + R.ins(b"k", b"")], [0, 1])
    st, f = both(codec, s, twins, [b"\xbe", b"\xbe\xbf\x7f\x00" + P.raw_lit(3)], [0, 1])
    assert f[0] == [(b"name", b"value", 0)] and f[1][1] == (b"X" * 5, b"X" * 7, 0)
    # call 3: the entries are carried through the commit a second time
    st, f = both(codec, s, twins, [b"\xbe" + R.ins(b"third", b"3") + b"\xbf", b"\xbe\xbf\xc0"], [0, 1])
    assert f[0][2] == (b"name", b"value", 0) and st[1] == 3
    check_states(s, twins)
    # inserted and evicted inside one call; the self-evicting name referenced
    # in the same call and in the next
    both(codec, s, twins, R.RULES["evict/inside-one-block"] + R.RULES["evict/own-name"][:1], [2, 2, 3])
    check_states(s, twins)
    st, f = both(codec, s, twins, R.RULES["evict/own-name"][1:], [3, 3])
    assert f[0][0] == (b"abcdefgh", b"w" * 20, 0) and st[1] == COMP
    check_states(s, twins)


def _lit_count(blocks):
    ops = R.batch(blocks)[3]
    return int((ops["name_lit"] >= 0).sum() + (ops["value_lit"] >= 0).sum())


def test_two_calls_queued(codec):
    """Two calls queued on one stream with no host synchronisation between
    them equal the same two calls synchronised.  Both calls' wire, offsets
    and CSR are on the device before the first call, and the literal counts
    and the arena's size come from the host, so nothing between the two
    chains copies to or from the device or waits for the stream (a run of
    the same calls on another set first leaves the allocator the blocks it
    hands out).  Call 2 resolves entries call 1 inserted: the random blocks
    come from encoders that index, and connection 8's do so by hand."""
    torch = codec.torch
    order, rnd = P.random_blocks(0x77, 8, 4, corrupt=0.05)
    calls = [(rnd[:16] + [R.ins(b"queued", b"one")], order[:16] + [8]),
             (rnd[16:32] + [b"\xbe" + R.ins(b"q2", b"two") + b"\xbf"], order[16:32] + [8])]
    res = []
    for sync in (None, False, True):  # None: the run that warms the allocator
        s = nghttp2_amd.DeviceInflaters(9, 4096)
        ready = []
        for blocks, conns in calls:
            wire, tw, to = layout(codec, blocks)
            ready.append((len(wire), tw, to, s.csr(conns), _lit_count(blocks)))
        torch.cuda.synchronize()
        out = []
        for nbytes, tw, to, csr, T in ready:  # nothing but launches from here on
            out.append(s.inflate(codec, tw, to, None, wire_bytes=nbytes, nlits=T, arena_cap=1 << 16, csr=csr))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        res.append(([hd.replay_fields(r.nva, r.arena, r.block_nv_off, r.status) for r in out],
                    [s.state(c) for c in range(9)]))
    assert res[1] == res[2]
    twins = [hd.HostReplayInflater(4096) for _ in range(9)]
    assert [twin_run(twins, b, c) for b, c in calls] == [tuple(x) for x in res[1][0]]
    assert res[1][1] == [R.host_state(t) for t in twins]
    st, f = res[1][0][1]
    assert f[16] == [(b"queued", b"one", 0), (b"q2", b"two", 0), (b"queued", b"one", 0)]
    # call 2's random blocks found call 1's entries too: blocks that succeed resolve dynamic indices
    dynamic = 0
    for k, blk in enumerate(calls[1][0][:16]):
        ops = hd.parse_block(blk)[1]
        indexed = (ops["kind"] == hd.OP_INDEXED) | ((ops["kind"] == hd.OP_LITERAL) & ((ops["flags"] & hd.OP_NEW_NAME) == 0))
        dynamic += st[k] >= 0 and bool((indexed & (ops["value"] > 61)).any())
    assert dynamic > 0


def test_literal_count_below_the_batch(codec):
    """A literal count below the parse's fails the fields of the literals
    past it; the decode's arrays are not read past their end."""
    s = nghttp2_amd.DeviceInflaters(2, 4096)
    blocks = [b"\x82\x40" + P.huff_lit(2) + P.huff_lit(3), b"\x00" + P.huff_lit(1) + P.raw_lit(1) + b"\x84"]
    st, f, totals = dev_run(codec, s, blocks, [0, 1], nlits=2, arena_cap=256)
    assert st == [2, COMP] and f == [[(b":method", b"GET", 0), (b"XX", b"XXX", 0)], []] and totals[2] == 0
    assert s.state(1)[3] == (False, True, True) and s.table(0) == [(b"XX", b"XXX")]


def _chain(codec, blocks):
    wire, tw, to = layout(codec, blocks)
    pb = codec.parse_blocks(tw, to, wire_bytes=len(wire))
    pool, lit_off = codec.gather_huffman_literals(tw, pb)
    t = pb.totals.cpu().numpy().view(np.uint32)
    dec = codec.decode_auto(pool, lit_off[:int(t[1]) + 1], enc_bytes=int(t[2]))
    return wire, tw, to, pb, dec


def _raw(codec, s, ch, csr, nva, nva_cap, arena, arena_cap, **over):
    torch = codec.torch
    wire, tw, to, pb, dec = ch
    n = to.numel() - 1
    nv_off = torch.full((n + 1,), -1, dtype=torch.int32, device=codec.device)
    out = torch.full((n,), -1, dtype=torch.int32, device=codec.device)
    tot = torch.full((4,), -1, dtype=torch.int32, device=codec.device)
    need = s.L.nghttp2_amd_hd_dev_inflate_workspace_size(s.nconn, s.table_bytes, pb.ops.shape[0], n)
    ws = torch.zeros(need, dtype=torch.uint8, device=codec.device)
    totals = over.get("totals", pb.totals)
    rv = s.L.nghttp2_amd_hd_dev_inflate_blocks(
        s.p, hd._p(tw), len(wire), hd._p(to), n, hd._p(pb.op_off), hd._p(pb.ops), pb.ops.shape[0],
        hd._p(pb.block_status), hd._p(totals), hd._p(dec[0]), dec[0].numel(), hd._p(dec[1]), hd._p(dec[2]),
        dec[2].numel(), hd._p(csr[0]), hd._p(csr[1]), hd._p(nva), nva_cap, hd._p(arena), arena_cap, hd._p(nv_off), hd._p(out),
        hd._p(tot), hd._p(ws), ws.numel(), hd._stream(None))
    assert rv == 0
    torch.cuda.synchronize()
    return nv_off, out, tot.cpu().numpy().view(np.uint32).tolist()


def test_caps(codec):
    torch = codec.torch
    order, blocks = P.random_blocks(0xCA9, 6, 5, corrupt=0.1)
    warm = [R.ins(b"warm%d" % c, b"up") for c in range(6)]
    twins = [hd.HostReplayInflater(4096) for _ in range(6)]
    twin_run(twins, warm, list(range(6)))
    before = [R.host_state(t) for t in twins]
    ws, wf = twin_run(twins, blocks, order)
    nf, nb = sum(len(x) for x in wf), sum(len(n) + len(v) + 2 for x in wf for n, v, _ in x)
    assert nf > 50

    def canary(n):
        return torch.full((n,), CANARY, dtype=torch.uint8, device=codec.device)

    ch = _chain(codec, blocks)
    for nva_cap, arena_cap, bits in ((nf, nb, 0), (nf - 1, nb, hd.DEV_OVERFLOW_NVA), (nf, nb - 1, hd.DEV_OVERFLOW_ARENA),
                                     (nf - 1, nb - 1, hd.DEV_OVERFLOW_NVA | hd.DEV_OVERFLOW_ARENA)):
        s = nghttp2_amd.DeviceInflaters(6, 4096)
        dev_run(codec, s, warm, list(range(6)))
        csr = s.csr(order)
        nva, arena = canary(24 * (nf + 4)), canary(nb + 64)
        nv_off, out, tot = _raw(codec, s, ch, csr, nva, nva_cap, arena, arena_cap)
        assert tot == [nf, nb, bits, 0]
        # the offsets and statuses are the batch's whatever the caps are
        assert out.cpu().tolist() == ws and nv_off.cpu().tolist() == np.cumsum([0] + [len(x) for x in wf]).tolist()
        if bits:
            assert (nva.cpu().numpy() == CANARY).all() and (arena.cpu().numpy() == CANARY).all()
            assert [s.state(c) for c in range(6)] == before
            # the repeated call with room equals a first call with room
            nva, arena = canary(24 * (nf + 4)), canary(nb + 64)
            nv_off, out, tot = _raw(codec, s, ch, csr, nva, nf, arena, nb)
            assert tot == [nf, nb, 0, 0]
        assert hd.replay_fields(nva[:24 * nf], arena[:nb], nv_off, out) == (ws, wf)
        assert (nva.cpu().numpy()[24 * nf:] == CANARY).all() and (arena.cpu().numpy()[nb:] == CANARY).all()
        check_states(s, twins)


def test_capacity_rule(codec):
    tb = 4096
    s = nghttp2_amd.DeviceInflaters(2, tb)
    twins = [hd.HostReplayInflater(tb) for _ in range(2)]
    assert s.change_table_size([1], [0xFFFFFFFF]).cpu().tolist() == [twins[1].change_table_size(0xFFFFFFFF)] == [0]
    one = R.ins(b"a", b"v" * 991)  # 1024 accounted
    st, f = both(codec, s, twins, [R.size(1 << 30) + one * 4], [1])
    assert st == [4] and s.table_size(1) == tb and s.table_max(1) == 1 << 30
    st, f = both(codec, s, twins, [b"\x82" + R.ins(b"b", b"") + b"\x84", b"\x82", b"\x82"], [1, 0, 1])
    assert st == [NOMEM, 1, COMP] and f[0] == [(b":method", b"GET", 0)]
    check_states(s, twins)
    assert both(codec, s, twins, [b"\x82"], [1])[0] == [COMP]


def test_arguments(codec):
    torch = codec.torch
    L = hd._replay_lib()
    s = nghttp2_amd.DeviceInflaters(2, 4096)
    s.inflate(codec, *layout(codec, [R.ins(b"n", b"v")])[1:], [0])
    before = [s.state(c) for c in range(2)]
    t = torch.zeros(1 << 16, dtype=torch.int32, device=codec.device)
    p = hd._p(t)
    bad = hd.NGHTTP2_ERR_INVALID_ARGUMENT
    need = L.nghttp2_amd_hd_dev_inflate_workspace_size(2, 4096, 1, 1)
    assert 0 < need <= 4 * t.numel()
    full = [s.p, p, 16, p, 1, p, p, 1, p, p, p, 16, p, p, 1, p, p, p, 1, p, 1, p, p, p, p, need, None]
    for k in (0, 1, 3, 5, 6, 8, 9, 10, 12, 13, 15, 16, 17, 19, 21, 22, 23, 24):
        a = list(full)
        a[k] = None
        assert L.nghttp2_amd_hd_dev_inflate_blocks(*a) == bad, k
    a = list(full)
    a[25] = need - 1
    assert L.nghttp2_amd_hd_dev_inflate_blocks(*a) == bad
    a = [None] * 27
    a[2] = a[4] = a[7] = a[11] = a[14] = a[18] = a[20] = a[25] = 0
    assert L.nghttp2_amd_hd_dev_inflate_blocks(*a) == 0  # nblocks == 0 touches nothing
    pp = hd.ctypes.c_void_p()
    for nconn, tb in ((0, 4096), (1, 2048), (1, 4097), (1 << 20, 4096)):
        assert L.nghttp2_amd_hd_dev_inflaters_new(hd.ctypes.byref(pp), nconn, tb, None) == bad
    with pytest.raises(ValueError):
        s.change_table_size([1, 1], [10, 20])
    # parse totals[3] != 0 on entry: nothing is written, the tables stay
    blocks = [b"\xbe\x40" + P.huff_lit(1) + P.huff_lit(2)]
    ch = _chain(codec, blocks)
    flagged = ch[3].totals.clone()
    flagged[3] = hd.PARSE_OVERFLOW_OPS
    nva = torch.full((24 * 8,), CANARY, dtype=torch.uint8, device=codec.device)
    arena = torch.full((256,), CANARY, dtype=torch.uint8, device=codec.device)
    nv_off, out, tot = _raw(codec, s, ch, s.csr([0]), nva, 8, arena, 256, totals=flagged)
    assert (nva.cpu().numpy() == CANARY).all() and (arena.cpu().numpy() == CANARY).all()
    assert nv_off.cpu().tolist() == [-1, -1] and out.cpu().tolist() == [-1] and tot == [0xFFFFFFFF] * 4
    assert [s.state(c) for c in range(2)] == before
    nv_off, out, tot = _raw(codec, s, ch, s.csr([0]), nva, 8, arena, 256)
    assert out.cpu().tolist() == [2] and s.table(0) == [(b"X", b"XX"), (b"n", b"v")]
