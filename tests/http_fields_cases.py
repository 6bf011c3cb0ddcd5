"""The committed corpus of tests/golden/http_fields.json as header blocks on the
wire, for the _http inflate's tests: every block deflated here with a small
encoder of the tests' own (raw or Huffman literals, new and indexed names,
with and without indexing, references to entries that earlier blocks of the
connection inserted), and what tests/http_fields_ref.py expects of it."""
import json
import os
import random

from tests import http_fields_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))

_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(os.path.join(HERE, "golden", "http_fields.json")) as f:
            _golden = json.load(f)
    return _golden


def blocks():
    """[(mode, state tuple, [(name, value)])] of the corpus."""
    return [(b["mode"], tuple(b["state"]), [(bytes.fromhex(n), bytes.fromhex(v)) for n, v in b["fields"]])
            for b in golden()["blocks"]]


def hpack_int(v, prefix, first):
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


# the static table's names, first index of each (RFC 7541 Appendix A)
STATIC_NAME = {b":authority": 1, b":method": 2, b":path": 4, b":scheme": 6, b":status": 8,
               b"content-length": 28, b"host": 38, b"transfer-encoding": 57}


class Encoder:
    """One connection's side of the wire.  It inserts only while the dynamic
    table stays below its 4096 bytes, so nothing is ever evicted and entry k
    (counted from the first insertion) is index 62 + (inserted - 1 - k)."""

    def __init__(self, rng, lit):
        self.rng, self.lit = rng, lit
        self.entries, self.size = [], 0

    def field(self, name, value):
        rng = self.rng
        if (name, value) in self.entries and rng.random() < 0.8:
            k = self.entries.index((name, value))
            return hpack_int(62 + len(self.entries) - 1 - k, 7, 0x80)
        room = len(name) + len(value) + 32
        index = self.size + room <= 3500 and rng.random() < 0.5
        first, prefix = (0x40, 6) if index else rng.choice([(0x00, 4), (0x10, 4)])
        dyn = [k for k, (n, _) in enumerate(self.entries) if n == name]
        if name in STATIC_NAME and rng.random() < 0.6:
            out = hpack_int(STATIC_NAME[name], prefix, first)
        elif dyn and rng.random() < 0.6:
            out = hpack_int(62 + len(self.entries) - 1 - dyn[0], prefix, first)
        else:
            out = bytes([first]) + self.lit(name)
        out += self.lit(value)
        if index:
            self.entries.append((name, value))
            self.size += room
        return out

    def block(self, fields):
        return b"".join(self.field(n, v) for n, v in fields)


def raw_lit(s):
    return hpack_int(len(s), 7, 0) + s


def huff_lit():
    """A Huffman string-literal encoder for the corpus: every distinct string
    encoded once, in one batch, by the oracle."""
    import numpy as np
    from oracle import oracle as O
    strings = sorted({s for _, _, fields in blocks() for nv in fields for s in nv})
    off = np.zeros(len(strings) + 1, dtype=np.uint32)
    np.cumsum([len(s) for s in strings], out=off[1:])
    pool = np.frombuffer(b"".join(strings) + b"\x00", dtype=np.uint8)[:-1]
    enc, enc_off = O.encode_batch(pool, off)
    enc = enc.tobytes()
    code = {s: enc[int(enc_off[i]):int(enc_off[i + 1])] for i, s in enumerate(strings)}
    return lambda s: hpack_int(len(code[s]), 7, 0x80) + code[s]


def wire(lit, nconn, seed=7):
    """The corpus over nconn connections, block i on connection i % nconn:
    (connection numbers, wire blocks, modes, states)."""
    rng = random.Random(seed)
    enc = [Encoder(rng, lit) for _ in range(nconn)]
    conn, out, modes, states = [], [], [], []
    for i, (mode, state, fields) in enumerate(blocks()):
        conn.append(i % nconn)
        out.append(enc[i % nconn].block(fields))
        modes.append(mode)
        states.append(state)
    return conn, out, modes, states


def expected():
    """What the restatement makes of the corpus: (verdicts of all fields in
    order, [state after], [block result])."""
    verdicts, states, results = [], [], []
    for mode, state, fields in blocks():
        v, s, r = R.run_block(fields, mode, state)
        verdicts += v
        states.append(s)
        results.append(r)
    return verdicts, states, results


def check_http(res, nfields_status=True):
    """Compare inflate_blocks(..., http=...)'s last three results with expected()."""
    verdicts, states, results = res[-3], res[-2], res[-1]
    ev, es, er = expected()
    assert verdicts.tolist() == ev
    assert results == er
    got = [(int(f) & R.FLAGS_COMPARED, int(s), int(c))
           for f, s, c in zip(states["http_flags"], states["status_code"], states["content_length"])]
    assert got == [(f & R.FLAGS_COMPARED, s, c) for f, s, c in es]
