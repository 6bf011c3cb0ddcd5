"""What the deflate-plan tests share: the splice of a plan (the twin's or any
other's records) into wire with the C oracle's emit_string for the literals,
adapters of the twin for the recorded reference's replay loop, random header
lists that hit every representation, and the table fillers of the search-edge
cases."""
import random

import numpy as np

from nghttp2_amd import hd
from oracle import oracle as O


def splice(recs, heads, nva, arena, off):
    """[wire of block b]: the head's bytes, then per field its record's bytes,
    the framed name when LIT_NAME is set and the framed value when LIT_VALUE is."""
    raw = arena.tobytes()
    out = []
    for b in range(len(off) - 1):
        w = bytearray(heads[b]["bytes"][:int(heads[b]["nbytes"])].tobytes())
        for k in range(int(off[b]), int(off[b + 1])):
            r, nv = recs[k], nva[k]
            assert int(r["block"]) == b and int(r["reserved"]) == 0 and 1 <= int(r["nbytes"]) <= 6
            w += r["bytes"][:int(r["nbytes"])].tobytes()
            if int(r["lits"]) & hd.PLAN_LIT_NAME:
                w += O.emit_string(raw[int(nv["name_off"]):int(nv["name_off"]) + int(nv["name_len"])])
            if int(r["lits"]) & hd.PLAN_LIT_VALUE:
                w += O.emit_string(raw[int(nv["value_off"]):int(nv["value_off"]) + int(nv["value_len"])])
        out.append(bytes(w))
    return out


def twin_wire(planner, header_lists):
    """The wire of header_lists, every list on planner's connection, in one call."""
    return splice(*planner.plan(header_lists))


class TwinDeflater:
    """The twin behind tests/ref_hd_wire_lib.py's deflater adapter interface."""

    def __init__(self, deflate_max, table_bytes=8192):
        self.p = hd.HostDeflatePlanner(table_bytes, deflate_max)

    def change(self, v):
        return self.p.change_table_size(v)

    def bound(self, nva):
        return 12 + 12 * len(nva) + sum(len(f[0]) + len(f[1]) for f in nva)

    def deflate(self, nva, api):
        w = twin_wire(self.p, [nva])[0]
        return len(w), w

    def state(self):
        return self.p.state()


NAMES = [b":method", b":path", b":status", b":authority", b"accept-encoding", b"cookie", b"authorization",
         b"set-cookie", b"content-length", b"etag", b"x-trace", b"x-a", b"", b"user-agent", b"te", b"x-long-" * 9]
VALUES = [b"GET", b"POST", b"/", b"/index.html", b"200", b"404", b"gzip, deflate", b"", b"a", b"v" * 19, b"w" * 20,
          b"0123456789" * 13, b"\x00\xff\xfe", b"example.org", b"Z" * 127, b"q" * 128, b"{}" * 300]


def random_lists(seed, nlists, nconn, max_fields=9):
    """(conn_of_list, header_lists): a small vocabulary, so names and whole
    fields repeat (indexed, indexed name, new name), with NO_INDEX on some."""
    rng = random.Random(seed)
    order, lists = [], []
    for _ in range(nlists):
        order.append(rng.randrange(nconn))
        hl = []
        for _ in range(rng.randrange(max_fields + 1)):
            n = rng.choice(NAMES)
            v = rng.choice(VALUES) if rng.random() < 0.8 else bytes(rng.randrange(256) for _ in range(rng.randrange(40)))
            hl.append((n, v, 1 if rng.random() < 0.1 else 0))
        lists.append(hl)
    return order, lists


def fnv1a(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def colliding_names(seed=7, length=8):
    """Two different names of `length` lower-case bytes with one FNV-1a hash:
    a seeded birthday search over batches, vectorised with numpy."""
    rng = np.random.default_rng(seed)
    seen_h = np.zeros(0, np.uint32)
    seen_s = np.zeros((0, length), np.uint8)
    while True:
        s = rng.integers(97, 123, size=(1 << 17, length), dtype=np.uint8)
        h = np.full(len(s), 2166136261, np.uint32)
        for k in range(length):
            h = (h ^ s[:, k]) * np.uint32(16777619)
        seen_h = np.concatenate([seen_h, h])
        seen_s = np.concatenate([seen_s, s])
        order = np.argsort(seen_h, kind="stable")
        sh = seen_h[order]
        for i in np.nonzero(sh[1:] == sh[:-1])[0]:
            a, b = seen_s[order[i]].tobytes(), seen_s[order[i + 1]].tobytes()
            if a != b:
                assert fnv1a(a) == fnv1a(b)
                return a, b
