"""tests/golden/ref_hd_wire.json (recorded from the reference's own deflater
and inflater by tests/golden/make_ref_hd_wire.py) for the tests that replay it:
the loader, and one replay loop over a connection's steps for any deflater /
inflater pair behind the small adapter interface below."""
import json
import os

PATH = os.path.join(os.path.dirname(__file__), "golden", "ref_hd_wire.json")

_doc = None


def unpack(x):
    """A fixture string: hex, "=" and ASCII text, or a list of such pieces and
    [unit, count] runs."""
    if isinstance(x, str):
        return x[1:].encode("ascii") if x.startswith("=") else bytes.fromhex(x)
    return b"".join(unpack(p) if isinstance(p, str) else unpack(p[0]) * p[1] for p in x)


def _table(old, delta):
    if delta is None:
        return old
    drop, add = delta
    return [(unpack(n), unpack(v)) for n, v in add] + old[:len(old) - drop]


def load():
    """The fixture as plain records (the generator's docstring has the compact
    layout): connections {family, name, deflate_max, steps}, steps
    {op: dchange | ichange | deflate | inflate, ...} with every string as
    bytes, a roundtrip step's wire and fields written out, and the whole
    dynamic table (dtable / itable) after every step."""
    global _doc
    if _doc is not None:
        return _doc
    doc = json.load(open(PATH))
    conns = []
    for family, name, deflate_max, steps in doc["connections"]:
        tables = {"d": [], "i": []}
        out, last = [], None
        for st in steps:
            kind, side = st[0], st[0][0]
            if kind in ("dc", "ic"):
                s = {"op": side + "change", "v": st[1], "rv": st[2]}
            elif kind == "d":
                s = {"op": "deflate", "nva": [(unpack(n), unpack(v), fl) for n, v, fl in st[1]], "api": st[2],
                     "rv": st[3], "bound": st[4], "wire": None if st[5] is None else unpack(st[5])}
                last = s
            else:
                assert kind == "i"
                rt = st[1] is None
                s = {"op": "inflate", "rt": rt, "wire": last["wire"] if rt else unpack(st[1]), "status": st[2],
                     "fields": [last["nva"][k][:2] + tuple(f) if len(f) == 2 else
                                (unpack(f[0]), unpack(f[1]), f[2], f[3]) for k, f in enumerate(st[3])]}
            s[side + "size"], s[side + "max"] = st[-3], st[-2]
            tables[side] = s[side + "table"] = _table(tables[side], st[-1])
            out.append(s)
        conns.append({"family": family, "name": name, "deflate_max": deflate_max, "steps": out})
    doc["connections"] = conns
    _doc = doc
    return doc


def connections(family=None, side=None):
    """Connections of one family (all: None) that have steps of one side
    ("d": deflate, "i": inflate)."""
    out = []
    for c in load()["connections"]:
        if family is not None and c["family"] != family:
            continue
        ops = {s["op"] for s in c["steps"]}
        if side == "d" and "deflate" not in ops:
            continue
        if side == "i" and "inflate" not in ops:
            continue
        out.append(c)
    return out


def deflate_steps(c):
    return [s for s in c["steps"] if s["op"] in ("dchange", "deflate")]


def inflate_steps(c):
    return [s for s in c["steps"] if s["op"] in ("ichange", "inflate")]


def check_deflate_step(s, d, where):
    """One dchange / deflate step on adapter d, every recorded value.  d has
    change(v) -> rv, deflate(nva, api) -> (rv, wire or None), bound(nva) and
    state() -> (table, size, max)."""
    if s["op"] == "dchange":
        assert d.change(s["v"]) == s["rv"], where
    else:
        assert d.bound(s["nva"]) == s["bound"], where
        rv, wire = d.deflate(s["nva"], s["api"])
        assert rv == s["rv"], (where, rv, s["rv"])
        if s["wire"] is not None:
            assert wire == s["wire"], (where, wire.hex()[:200], s["wire"].hex()[:200])
    table, size, mx = d.state()
    assert (size, mx) == (s["dsize"], s["dmax"]), (where, size, mx, s["dsize"], s["dmax"])
    assert table == s["dtable"], where


def check_inflate_result(s, status, fields, where):
    assert status == s["status"], (where, status, s["status"])
    assert [tuple(f) for f in fields] == s["fields"], where


def check_inflate_step(s, i, where):
    """One ichange / inflate step on adapter i: change(v) -> rv,
    inflate(wire) -> (status, [(name, value, flags, token)]) and state()."""
    if s["op"] == "ichange":
        rv = i.change(s["v"])
        assert rv == s["rv"], (where, rv, s["rv"])
    else:
        status, fields = i.inflate(s["wire"])
        check_inflate_result(s, status, fields, where)
    check_inflate_state(s, i.state(), where)


def check_inflate_state(s, state, where):
    table, size, mx = state
    assert (size, mx) == (s["isize"], s["imax"]), (where, size, mx, s["isize"], s["imax"])
    assert table == s["itable"], where


def where(c, k):
    return "%s / %s, step %d (%s)" % (c["family"], c["name"], k, c["steps"][k]["op"])


# ---------------------------------------------------------------------------
# the product behind the adapter interface, and the batched replays
# ---------------------------------------------------------------------------
class ProductDeflater:
    def __init__(self, deflate_max):
        import nghttp2_amd
        self.m = nghttp2_amd
        self.d = nghttp2_amd.HpackDeflater(deflate_max)

    def change(self, v):
        self.d.change_table_size(v)
        return 0

    def bound(self, nva):
        return self.d.bound(nva)

    def deflate(self, nva, api):
        if api is None:
            st, wire = self.m.deflate_blocks([self.d], [nva])
            return st[0], wire[0]
        if "hd2" in api:
            return self.d.deflate_hd2(nva, api["hd2"])
        rv, parts = self.d.deflate_hd_vec2(nva, api["vec"])
        return rv, b"".join(parts)[:max(rv, 0)]

    def state(self):
        t = self.d.dynamic_table()
        assert self.d.num_table_entries() == 61 + len(t)
        return t, self.d.dynamic_table_size(), self.d.max_dynamic_table_size()


class ProductInflater:
    def __init__(self):
        import nghttp2_amd
        self.m = nghttp2_amd
        self.i = nghttp2_amd.HpackInflater()

    def change(self, v):
        return self.i.change_table_size(v)

    def inflate(self, wire):
        st, f, tk = self.m.inflate_blocks([self.i], [wire], tokens=True)
        assert len(tk) == len(f[0])
        return st[0], [(n, v, fl, int(t)) for (n, v, fl), t in zip(f[0], tk)]

    def state(self):
        t = self.i.dynamic_table()
        assert self.i.num_table_entries() == 61 + len(t)
        return t, self.i.dynamic_table_size(), self.i.max_dynamic_table_size()


def product_deflate_batched(conns):
    """Every connection's deflate steps through deflate_blocks, one block of
    each connection per call (block k of every connection before block k + 1
    of any); table size changes and the api family's deflate_hd2 /
    deflate_hd_vec2 calls run in their places.  Every recorded value and the
    table are checked after every step.  Returns the number of batched calls."""
    import nghttp2_amd
    ds = [ProductDeflater(c["deflate_max"]) for c in conns]
    pos = [0] * len(conns)
    calls = 0
    while True:
        batch = []
        for ci, c in enumerate(conns):
            steps = c["steps"]
            while pos[ci] < len(steps) and not (steps[pos[ci]]["op"] == "deflate" and steps[pos[ci]]["api"] is None):
                if steps[pos[ci]]["op"] in ("dchange", "deflate"):
                    check_deflate_step(steps[pos[ci]], ds[ci], where(c, pos[ci]))
                pos[ci] += 1
            if pos[ci] < len(steps):
                batch.append(ci)
        if not batch:
            return calls
        todo = [conns[ci]["steps"][pos[ci]] for ci in batch]
        for ci, s in zip(batch, todo):
            assert ds[ci].bound(s["nva"]) == s["bound"], where(conns[ci], pos[ci])
        st, wire = nghttp2_amd.deflate_blocks([ds[ci].d for ci in batch], [s["nva"] for s in todo])
        calls += 1
        for k, (ci, s) in enumerate(zip(batch, todo)):
            w = where(conns[ci], pos[ci])
            assert st[k] == s["rv"], (w, st[k], s["rv"])
            if s["wire"] is not None:
                assert wire[k] == s["wire"], (w, wire[k].hex()[:200], s["wire"].hex()[:200])
            table, size, mx = ds[ci].state()
            assert (size, mx) == (s["dsize"], s["dmax"]), w
            assert table == s["dtable"], w
            pos[ci] += 1


def product_inflate_batched(conns):
    """Every connection's inflate steps through inflate_blocks(tokens=True),
    one block of each connection per call, change_table_size calls in their
    places; every recorded value and the table after every step.  Returns the
    number of batched calls."""
    import nghttp2_amd
    infs = [ProductInflater() for _ in conns]
    pos = [0] * len(conns)
    calls = 0
    while True:
        batch = []
        for ci, c in enumerate(conns):
            steps = c["steps"]
            while pos[ci] < len(steps) and steps[pos[ci]]["op"] != "inflate":
                if steps[pos[ci]]["op"] == "ichange":
                    check_inflate_step(steps[pos[ci]], infs[ci], where(c, pos[ci]))
                pos[ci] += 1
            if pos[ci] < len(steps):
                batch.append(ci)
        if not batch:
            return calls
        todo = [conns[ci]["steps"][pos[ci]] for ci in batch]
        st, f, tk = nghttp2_amd.inflate_blocks([infs[ci].i for ci in batch], [s["wire"] for s in todo], tokens=True)
        calls += 1
        assert len(tk) == sum(len(x) for x in f)
        at = 0
        for k, (ci, s) in enumerate(zip(batch, todo)):
            w = where(conns[ci], pos[ci])
            fields = [(n, v, fl, int(t)) for (n, v, fl), t in zip(f[k], tk[at:at + len(f[k])])]
            at += len(f[k])
            check_inflate_result(s, st[k], fields, w)
            check_inflate_state(s, infs[ci].state(), w)
            pos[ci] += 1


def replay_deflate(c, make):
    d = make(c["deflate_max"])
    for k, s in enumerate(c["steps"]):
        if s["op"] in ("dchange", "deflate"):
            check_deflate_step(s, d, where(c, k))


def replay_inflate(c, make):
    i = make()
    for k, s in enumerate(c["steps"]):
        if s["op"] in ("ichange", "inflate"):
            check_inflate_step(s, i, where(c, k))
