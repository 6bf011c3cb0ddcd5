"""nghttp2_amd_hd_dev_deflate_blocks: the device-resident deflaters (the kernels
of csrc/hd_deflate_dev.hip) against the host twin (the same header walked on the
host, its plan spliced with the C oracle's emit_string), the results the
reference itself recorded, the Python restatement and the host deflater --
never against themselves."""
import ctypes

import numpy as np
import pytest
import torch

import nghttp2_amd
from nghttp2_amd import hd
from oracle import hpack_oracle as HO
from tests import hd_deflate_plan_ref as D
from tests import ref_hd_wire_lib as W
from tests.test_deflate_plan_host import recorded_connections

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def pad_fields(fields, extra):
    """nva with `extra` more record slots behind the fields, filled with 0xFF."""
    nva, arena, off = fields
    return torch.cat([nva, torch.full((24 * extra,), 0xFF, dtype=torch.uint8, device=nva.device)]), arena, off


def dev_call(dd, lists, order, out_cap=None, extra=0):
    """One device call: list i on connection order[i].  (wire, status, totals)."""
    fields = pad_fields(dd.upload(lists), extra) if extra else dd.upload(lists)
    out, out_off, st, tot = dd.deflate(fields, *dd.csr(order), out_cap=out_cap)
    return hd.deflated_wire(out, out_off), st.cpu().tolist(), u32(tot)


def twin_call(twins, lists, order):
    """The same call on the twins: every connection's lists in one plan."""
    want = [None] * len(lists)
    for c in sorted(set(order)):
        idx = [i for i, o in enumerate(order) if o == c]
        for i, w in zip(idx, D.twin_wire(twins[c], [lists[i] for i in idx])):
            want[i] = w
    return want


def check_call(dd, twins, lists, order, **kw):
    wire, st, tot = dev_call(dd, lists, order, **kw)
    want = twin_call(twins, lists, order)
    assert tot[2] == 0 and tot[0] == sum(len(w) for w in want)
    for i, (a, b) in enumerate(zip(wire, want)):
        assert a == b, (i, order[i], a.hex()[:120], b.hex()[:120])
    assert st == [len(w) for w in want]
    for c in sorted(set(order)):
        assert dd.state(c) == twins[c].state(), c
    return wire


def make(nconn, table_bytes=4096, deflate_max=None):
    dm = [4096] * nconn if deflate_max is None else [deflate_max] * nconn if np.isscalar(deflate_max) else deflate_max
    return (nghttp2_amd.DeviceDeflaters(nconn, table_bytes, dm, device=DEV),
            [hd.HostDeflatePlanner(table_bytes, m) for m in dm])


def change(dd, twins, conns, values):
    assert dd.change_table_size(conns, values).cpu().tolist() == [0] * len(conns)
    for c, v in zip(conns, values):
        twins[c].change_table_size(v)


def test_recorded_reference_on_the_device():
    """The 73 recorded connections in one set, one block per connection per
    call, the dchange steps in their places: wire and state after every step."""
    conns, left_out = recorded_connections()
    assert (len(conns), left_out) == (73, 3)
    dd = nghttp2_amd.DeviceDeflaters(len(conns), 8192, [c["deflate_max"] for c in conns], device=DEV)
    pos = [0] * len(conns)
    ndef = nchg = 0

    def check_state(ci, s, where):
        table, size, mx = dd.state(ci)
        assert (size, mx) == (s["dsize"], s["dmax"]), where
        assert table == s["dtable"], where
    while True:
        batch = []
        for ci, c in enumerate(conns):
            steps = c["steps"]
            while pos[ci] < len(steps) and steps[pos[ci]]["op"] != "deflate":
                s = steps[pos[ci]]
                if s["op"] == "dchange":
                    assert dd.change_table_size([ci], [s["v"]]).cpu().tolist() == [s["rv"]]
                    check_state(ci, s, W.where(c, pos[ci]))
                    nchg += 1
                pos[ci] += 1
            if pos[ci] < len(steps):
                batch.append(ci)
        if not batch:
            break
        todo = [conns[ci]["steps"][pos[ci]] for ci in batch]
        wire, st, tot = dev_call(dd, [s["nva"] for s in todo], batch)
        assert tot[2] == 0
        for k, (ci, s) in enumerate(zip(batch, todo)):
            where = W.where(conns[ci], pos[ci])
            assert st[k] == s["rv"] and wire[k] == s["wire"], (where, wire[k].hex()[:200])
            check_state(ci, s, where)
            pos[ci] += 1
            ndef += 1
    assert (ndef, nchg) == (256, 16)


@pytest.mark.parametrize("deflate_max", [4096, 256, 0])
def test_several_blocks_per_call(deflate_max):
    order, lists = D.random_lists(77 + deflate_max, 60, 5)
    dd, twins = make(5, 4096, deflate_max)
    check_call(dd, twins, lists[:40], order[:40])
    change(dd, twins, [1, 3], [64, 4096])
    check_call(dd, twins, lists[40:], order[40:])


def name_of(i):
    return bytes([i])  # 256 different 1-byte names: 33 bytes accounted each


POSITIONS = ("newest", "oldest", 63, 64, 65, "absent")


def search_cases():
    out = []
    for n in (0, 1, 63, 64, 65, 127, 128, 256):
        for pos in POSITIONS:
            at = {"newest": 0, "oldest": n - 1, "absent": None}.get(pos, pos)
            if at is not None and not 0 <= at < n:
                continue
            for where in ("ring", "fresh", "straddle"):
                out.append((n, at, where))
    return out


def test_search_edges():
    """Tables of 0 .. 256 entries of 33 bytes; the match at the newest entry,
    the oldest, at positions 63, 64 and 65, and absent; in the ring only
    (filled by an earlier call), in `fresh` only (filled by the same call) and
    straddling both.  Every case is a connection of one set."""
    cases = search_cases()
    assert len(cases) == 3 * (1 + 3 + 3 + 4 + 5 + 6 + 6 + 6)
    tb = 16384  # 256 * 33 bytes
    dd, twins = make(len(cases), tb, tb)
    change(dd, twins, list(range(len(cases))), [tb] * len(cases))
    first, second = [], []
    for n, at, where in cases:
        fill = [(name_of(i), b"") for i in range(n)]  # entry i ends at position n - 1 - i
        hit = name_of(n - 1 - at) if at is not None else b"no"
        # an exact match, a name match with another value (inserted), never indexing, the exact again
        probe = [(hit, b""), (hit, b"other"), (hit, b"secret", 1), (hit, b"")]
        split = {"ring": n, "fresh": 0, "straddle": n // 2}[where]
        first.append(fill[:split])
        second.append(fill[split:] + probe)
    order = list(range(len(cases)))
    check_call(dd, twins, first, order)
    wire = check_call(dd, twins, second, order, extra=5)
    # the twin is not the only witness: the restatement, for every case
    for case, a, b, w in zip(cases, first, second, wire):
        ref = HO.Deflater(tb)
        ref.change_table_size(tb)
        ref.deflate_block(a)
        assert ref.deflate_block(b) == w, case


RULES = {
    # the exact match is older than a name-only match: it wins
    "exact-older": [[(b"x-a", b"1"), (b"x-a", b"2"), (b"x-a", b"1")]],
    # never indexing stops at the first name: the newer entry's index, although an exact one exists
    "never-first-name": [[(b"x-a", b"1"), (b"x-a", b"2")], [(b"x-a", b"1", 1)]],
    # a static token shadowed by a dynamic exact entry; without one, the static table from the token on
    "static-shadowed": [[(b":status", b"299")], [(b":status", b"299"), (b":status", b"404"), (b":status", b"298")]],
    "static-never": [[(b":method", b"GET", 1), (b"cookie", b"short"), (b"authorization", b"x" * 30)]],
    # the insertion evicts the entry the field's own index names
    "evicts-own-index": [[(b"abcdefgh", b"12345678")], [(b"abcdefgh", b"w" * 100)], [(b"abcdefgh", b"x" * 101)]],
    # an entry over 3/4 of the table is not indexed, and the table stays as it is
    "over-three-quarters": [[(b"x-a", b"1"), (b"x-big", b"v" * 180), (b"x-a", b"1")]],
    "no-indexing-names": [[(b":path", b"/a/b"), (b"etag", b"e"), (b"content-length", b"12"), (b"set-cookie", b"s"),
                           (b":path", b"/a/b")]],
    "empty-strings": [[(b"", b""), (b"", b""), (b"x", b""), (b"", b"v")]],
}


@pytest.mark.parametrize("name", sorted(RULES))
def test_rule(name):
    dd, twins = make(1, 4096, 256)
    ref = HO.Deflater(256)
    for hl in RULES[name]:
        assert check_call(dd, twins, [hl], [0]) == [ref.deflate_block(hl)]
    assert dd.state(0) == ([tuple(e) for e in ref.table], ref.size, ref.max)


def test_entry_larger_than_max():
    """An entry larger than max.  A deflater never inserts one -- it is over
    3/4 of the table, so deflate_nv does not index it and the table stays as it
    is (the restatement and the recorded reference agree) -- so the case is
    held where it can occur: limits of 44, 0, 4096 and 45 bytes around 33-byte
    entries, a table emptied by the change itself, and fields deflated under
    each limit."""
    dd, twins = make(1, 4096, 4096)
    ref = HO.Deflater(4096)
    lists = [[(b"a", b"1"), (b"b", b"2")], [(b"c", b""), (b"a", b"1")], [(b"a", b"1"), (b"d" * 40, b"")]]
    assert check_call(dd, twins, lists[:1], [0]) == [ref.deflate_block(lists[0])]
    for v, hl in ((44, lists[1]), (0, lists[2]), (4096, lists[1]), (45, lists[2])):
        change(dd, twins, [0], [v])
        ref.change_table_size(v)
        assert dd.state(0) == ([tuple(e) for e in ref.table], ref.size, ref.max)
        assert check_call(dd, twins, [hl], [0]) == [ref.deflate_block(hl)]
        assert dd.state(0) == ([tuple(e) for e in ref.table], ref.size, ref.max)


def test_filter_collisions():
    """Two different names of one FNV-1a hash: with one in the table and the
    other deflated, a search that trusts the key indexes the wrong entry."""
    a, b = D.colliding_names()
    dd, twins = make(2)
    lists = [[(a, b"v")], [(b, b"v")], [(a, b"v"), (b, b"v"), (b, b"w")], [(b, b"v"), (a, b"v")]]
    wire = check_call(dd, twins, lists, [0, 0, 0, 1])
    ref = HO.Deflater()
    assert wire[:3] == [ref.deflate_block(hl) for hl in lists[:3]]
    assert wire[1][0] == 0x40  # a new name, not an index


LITERALS = [b"", b"\xfe" * 126, b"\xfe" * 127, b"\xfe" * 128, b"a" * 126, b"e" * 170, b"\x00\xff\xfe", b"J" * 70000]


@pytest.mark.parametrize("nconn", [1, 2, 63, 64, 65, 129])
def test_wave_and_grid_edges(nconn):
    """Idle connections between busy ones, blocks with no field, more record
    slots than fields, literals of length 0, at the one- and two-byte length
    prefix, raw chosen over Huffman, and a 70,000-byte value."""
    dd, twins = make(nconn)
    busy = list(range(0, nconn, 2))
    order, lists = [], []
    for k, c in enumerate(busy):
        order += [c, c, c]
        lists += [[], [(b"x-%d" % c, LITERALS[k % len(LITERALS)]), (LITERALS[(k + 1) % 7], b"v")], []]
    check_call(dd, twins, lists, order, extra=3)
    check_call(dd, twins, lists[::-1], order[::-1])
    for c in range(1, nconn, 2):
        assert dd.state(c) == ([], 0, 4096)


def test_state_across_calls_and_queued_calls():
    order, lists = D.random_lists(5, 45, 4)
    dd, twins = make(4)
    for k in range(3):  # three calls, read back between them
        check_call(dd, twins, lists[15 * k:15 * k + 15], order[15 * k:15 * k + 15])
    # two calls queued with no synchronisation between them
    dd2, twins2 = make(4)
    parts = [(lists[:20], order[:20]), (lists[20:], order[20:])]
    fields = [dd2.upload(l) for l, _ in parts]
    csrs = [dd2.csr(o) for _, o in parts]
    torch.cuda.synchronize()
    res = [dd2.deflate(f, *c) for f, c in zip(fields, csrs)]
    for (l, o), (out, out_off, st, tot) in zip(parts, res):
        assert hd.deflated_wire(out, out_off) == twin_call(twins2, l, o) and u32(tot)[2] == 0
    for c in range(4):
        assert dd2.state(c) == twins2[c].state()


def test_overflow_is_all_or_nothing():
    order, lists = D.random_lists(9, 24, 3)
    dd, twins = make(3)
    check_call(dd, twins, lists[:12], order[:12])
    before = [dd.state(c) for c in range(3)]
    want = twin_call(twins, lists[12:], order[12:])
    need = sum(len(w) for w in want)
    fields, csr = dd.upload(lists[12:]), dd.csr(order[12:])
    big = torch.full((need + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    out, out_off, st, tot = dd.deflate(fields, *csr, out=big[64:64 + need - 1])
    assert u32(tot) == [need, u32(tot)[1], hd.DEV_OVERFLOW_WIRE, 0]
    assert bool((big == 0xA5).all())  # out is untouched, and so is what lies around it
    assert st.cpu().tolist() == [len(w) for w in want]
    assert [dd.state(c) for c in range(3)] == before
    out, out_off, st, tot = dd.deflate(fields, *csr, out=big[64:64 + need])  # exactly the need
    assert u32(tot)[0] == need and u32(tot)[2] == 0
    assert hd.deflated_wire(out, out_off) == want
    h = big.cpu().numpy()
    assert (h[:64] == 0xA5).all() and (h[64 + need:] == 0xA5).all()
    assert [dd.state(c) for c in range(3)] == [t.state() for t in twins]


def test_arguments():
    L = hd._dev_deflate_lib()
    bad = hd.NGHTTP2_ERR_INVALID_ARGUMENT
    dd, _ = make(2)
    nva, arena, off = dd.upload([[(b"a", b"b")]])
    cb_off, cb = dd.csr([0])
    out = torch.zeros(256, dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(8, dtype=torch.int32, device=DEV)
    need = L.nghttp2_amd_hd_dev_deflate_workspace_size(2, 4096, 1, arena.numel(), 1)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    full = [dd.p, hd._p(nva), 1, hd._p(arena), arena.numel(), hd._p(off), 1, hd._p(cb_off), hd._p(cb), hd._p(out), 256,
            hd._p(i32), hd._p(i32[2:]), hd._p(i32[4:]), hd._p(ws), need, s]
    assert L.nghttp2_amd_hd_dev_deflate_blocks(*full) == 0
    for k in (0, 1, 3, 5, 7, 8, 9, 11, 12, 13, 14):
        b = list(full)
        b[k] = None
        assert L.nghttp2_amd_hd_dev_deflate_blocks(*b) == bad, k
    for k, v in ((15, need - 1), (2, 0x40000000), (4, 1 << 32), (14, ctypes.c_void_p(ws.data_ptr() + 4))):
        b = list(full)
        b[k] = v
        assert L.nghttp2_amd_hd_dev_deflate_blocks(*b) == bad, k
    b = [None, None, 0, None, 0, None, 0, None, None, None, 0, None, None, None, None, 0, None]
    assert L.nghttp2_amd_hd_dev_deflate_blocks(*b) == 0  # no block: nothing is touched
    torch.cuda.synchronize()
    p = ctypes.c_void_p()
    dm = np.array([4096, 4097], np.uint32)
    assert L.nghttp2_amd_hd_dev_deflaters_new(ctypes.byref(p), 2, 4096, dm.ctypes.data, s) == bad
    assert L.nghttp2_amd_hd_dev_deflaters_new(ctypes.byref(p), 2, 5000, None, s) == bad
    # a block listed by no connection produces no wire; one out of range is skipped
    wire, st, tot = dev_call(dd, [[(b"a", b"b")], [(b"c", b"d")]], [0, 0])
    assert len(wire[0]) and len(wire[1])
    fields = dd.upload([[(b"a", b"b")], [(b"c", b"d")]])
    off2, blk2 = dd.csr([1])  # only block 0, on connection 1
    out, out_off, st, tot = dd.deflate(fields, off2, blk2)
    assert [len(w) for w in hd.deflated_wire(out, out_off)] == [5, 0] and st.cpu().tolist() == [5, 0]


def test_round_trip_on_the_device():
    """deflate -> inflate on the device: fields and flags equal the input and
    both sets' tables agree; then inflate's ReplayedBlocks straight into
    another deflate, with no host array between."""
    order, lists = D.random_lists(21, 40, 6)
    lists = [[f for f in hl if len(f[1]) < 500] for hl in lists]
    dd, twins = make(6)
    fields, csr = dd.upload(lists), dd.csr(order)
    out, out_off, st, tot = dd.deflate(fields, *csr)
    nbytes = u32(tot)[0]
    wire = torch.zeros((nbytes + 15) // 16 * 16 + 32, dtype=torch.uint8, device=DEV)
    wire[:nbytes] = out[:nbytes]
    codec = nghttp2_amd.HuffmanBatchCodec(DEV)
    di = nghttp2_amd.DeviceInflaters(6, 4096, device=DEV)
    r = di.inflate(codec, wire, out_off, order, wire_bytes=nbytes)
    status, got = hd.replay_fields(r.nva, r.arena, r.block_nv_off, r.status)
    assert status == [len(hl) for hl in lists]
    # (a field the deflater never indexes on its own comes back flagged NO_INDEX)
    def never(f):
        return f[0] == b"authorization" or (f[0] == b"cookie" and len(f[1]) < 20)
    assert got == [[(bytes(f[0]), bytes(f[1]), 1 if never(f) else f[2]) for f in hl] for hl in lists]
    for c in range(6):
        assert di.state(c)[:3] == dd.state(c)
    # the reverse: what the inflaters left, deflated again by fresh contexts
    dd2 = nghttp2_amd.DeviceDeflaters(6, 4096, device=DEV)
    out2, out_off2, st2, tot2 = dd2.deflate(r, *csr)
    assert u32(tot2)[2] == 0
    assert hd.deflated_wire(out2, out_off2) == hd.deflated_wire(out, out_off) == twin_call(twins, lists, order)


def test_against_the_host_deflater():
    order, lists = D.random_lists(33, 64, 8)
    dd, _ = make(8)
    wire, st, tot = dev_call(dd, lists, order)
    ds = [nghttp2_amd.HpackDeflater() for _ in range(8)]
    hst, hwire = nghttp2_amd.deflate_blocks([ds[c] for c in order], lists)
    assert (st, wire) == (hst, hwire)
    for c in range(8):
        assert dd.state(c) == (ds[c].dynamic_table(), ds[c].dynamic_table_size(), ds[c].max_dynamic_table_size())
