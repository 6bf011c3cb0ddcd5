"""The commit the device inflaters and the device deflaters share
(hdtable::commit, csrc/hd_devtable.h), on both kinds of set, over one grid: a
single commit with `nold` entries that stay and `nnew` entries that enter, each
count at and around a 64-lane trip.  Every table is held to its host twin
(HostReplayInflater, HostDeflatePlanner), which commits with
hdreplay::commit_host -- never to the other set or to itself.

Every connection's table is made 16384 bytes first (a new context starts at
4096, where 124 entries of 33 bytes fit and the largest cells would evict); the
entries are distinct 1-byte names with empty values, 33 bytes each, so that a
deflater inserts every one.  Per cell: a call that fills `nold` entries; the
grid's commit; the table cut back to its `nold` newest entries by the size
change; the grid's commit again, into the other store buffer; and a call that
only references the oldest and the newest entry.  The cells are the even
connections of one set; the odd ones stay idle."""
import itertools

import pytest

import nghttp2_amd
from nghttp2_amd import hd
from tests import hd_parse_ref as P
from tests import hd_replay_ref as R
from tests.test_dev_deflate_gpu import change, check_call, make, name_of
from tests.test_replay_gpu import both, check_states

pytestmark = pytest.mark.gpu

TB, ROOM = 16384, 33
COUNTS = (0, 1, 63, 64, 65)
CELLS = [(o, n) for o, n in itertools.product(COUNTS, COUNTS) if ROOM * (o + n) <= TB]
NCONN = 2 * len(CELLS) - 1
BUSY = list(range(0, NCONN, 2))


# no pair is left out: the largest holds 130 entries, the store 496
assert len(CELLS) == 25 and max(o + n for o, n in CELLS) == 130 and TB // ROOM == 496


def names(cell, call):
    """The names a cell's call inserts: the fill's, then each grid commit's."""
    nold, nnew = cell
    first = {0: 0, 1: nold, 2: nold + nnew}[call]
    return [name_of(first + i) for i in range(nnew if call else nold)]


def test_inflaters(codec):
    s = nghttp2_amd.DeviceInflaters(NCONN, TB)
    twins = [hd.HostReplayInflater(TB) for _ in range(NCONN)]

    def call(blocks, held):
        both(codec, s, twins, blocks, BUSY)
        check_states(s, twins)  # the idle connections too
        for c, (nold, nnew) in zip(BUSY, CELLS):
            assert len(twins[c].table()) == held(nold, nnew) and twins[c].table_max() == TB, (nold, nnew)

    def set_size(values):
        assert s.change_table_size(BUSY, values).cpu().tolist() == [twins[c].change_table_size(v)
                                                                    for c, v in zip(BUSY, values)]

    def inserts(call_no):
        return [b"".join(R.ins(n, b"") for n in names(cell, call_no)) for cell in CELLS]

    set_size([TB] * len(BUSY))
    call([R.size(TB) + b for b in inserts(0)], lambda nold, nnew: nold)
    call(inserts(1), lambda nold, nnew: nold + nnew)
    set_size([ROOM * nold for nold, _ in CELLS])
    check_states(s, twins)
    set_size([TB] * len(BUSY))
    call([R.size(ROOM * nold) + R.size(TB) + b for (nold, _), b in zip(CELLS, inserts(2))],
         lambda nold, nnew: nold + nnew)
    # the committed descriptors, read by the next call: the newest and the oldest entry
    call([P.enc_int(62, 7, 0x80) + P.enc_int(61 + nold + nnew, 7, 0x80) if nold + nnew else b"\x82"
          for nold, nnew in CELLS], lambda nold, nnew: nold + nnew)
    for c in range(1, NCONN, 2):
        assert s.state(c) == ([], 0, 4096, (False, False, False))


def test_deflaters():
    dd, twins = make(NCONN, TB, TB)

    def call(lists, held):
        check_call(dd, twins, lists, BUSY)  # the wire, and the busy connections' tables
        for c in range(NCONN):
            assert dd.state(c) == twins[c].state(), c
        for c, (nold, nnew) in zip(BUSY, CELLS):
            assert len(twins[c].table()) == held(nold, nnew) and twins[c].table_max() == TB, (nold, nnew)

    def inserts(call_no):
        return [[(n, b"") for n in names(cell, call_no)] for cell in CELLS]

    change(dd, twins, BUSY, [TB] * len(BUSY))
    call(inserts(0), lambda nold, nnew: nold)
    call(inserts(1), lambda nold, nnew: nold + nnew)
    change(dd, twins, BUSY, [ROOM * nold for nold, _ in CELLS])
    change(dd, twins, BUSY, [TB] * len(BUSY))
    call(inserts(2), lambda nold, nnew: nold + nnew)
    # the moved keys, read by the next call's search: the newest and the oldest entry, both indexed
    probe = [[(t.table()[0][0], b""), (t.table()[-1][0], b"")] if t.table() else [] for t in (twins[c] for c in BUSY)]
    call(probe, lambda nold, nnew: nold + nnew)
    for c in range(1, NCONN, 2):
        assert dd.state(c) == ([], 0, 4096)
