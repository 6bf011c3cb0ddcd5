"""The HPACK deflater and inflater against results recorded from the
reference's own nghttp2_hd.c (tests/golden/ref_hd_wire.json, made by
tests/golden/make_ref_hd_wire.py: a driver of ours around the reference's
sources; placed cases in named families).  Here, on the CPU:

- the fixture's shape, its family counts (the ones the generator printed),
  that every recorded error code occurs, and that config1_wire.json is the
  file the reference deflater reproduced;
- the restated oracles (oracle/hpack_oracle.py's Deflater and Inflater, and
  oracle/hpack_inflate_oracle.c behind CInflater) replay every connection and
  equal every recorded value: wire bytes, return codes, bounds, fields with
  flags and tokens, tables, hd_table_bufsize and hd_table_bufsize_max, and
  nghttp2_hd_inflate_change_table_size's return code;
- the product's inflater for the connections that make no GPU call (no
  Huffman literal in any block).  Every deflate connection of the corpus emits
  a literal, which the product frames on the GPU, so the deflater's product
  tests are all in the GPU file.

tests/test_ref_hd_wire_gpu.py runs every connection through the product.
Everything is bit-exact."""
import hashlib
import os

import pytest

from oracle import hpack_oracle as HO
from tests import ref_hd_wire_lib as R

# what tests/golden/make_ref_hd_wire.py printed
FAMILIES = {
    "after_error": {"connections": 34, "deflates": 0, "inflates": 170},
    "api": {"connections": 8, "deflates": 17, "inflates": 0},
    "eviction": {"connections": 6, "deflates": 13, "inflates": 11},
    "huffman": {"connections": 15, "deflates": 0, "inflates": 30},
    "index_widths": {"connections": 6, "deflates": 16, "inflates": 0},
    "indexing": {"connections": 16, "deflates": 37, "inflates": 0},
    "integers": {"connections": 75, "deflates": 0, "inflates": 163},
    "lengths": {"connections": 16, "deflates": 0, "inflates": 34},
    "literals": {"connections": 5, "deflates": 7, "inflates": 0},
    "roundtrip": {"connections": 73, "deflates": 0, "inflates": 252},
    "search": {"connections": 16, "deflates": 81, "inflates": 0},
    "size_updates": {"connections": 41, "deflates": 0, "inflates": 91},
    "table_size": {"connections": 13, "deflates": 51, "inflates": 0},
    "three_quarters": {"connections": 9, "deflates": 40, "inflates": 0},
    "truncated": {"connections": 65, "deflates": 0, "inflates": 130},
}
DEFLATE_FAMILIES = sorted(f for f, n in FAMILIES.items() if n["deflates"])
INFLATE_FAMILIES = sorted(f for f, n in FAMILIES.items() if n["inflates"] and f != "roundtrip") + ["roundtrip"]


def test_fixture_shape_and_families():
    doc = R.load()
    assert doc["families"] == FAMILIES
    got = {}
    for c in doc["connections"]:
        assert set(c) == {"family", "name", "deflate_max", "steps"}
        f = got.setdefault(c["family"], {"connections": 0, "deflates": 0, "inflates": 0})
        f["connections"] += 1
        for s in c["steps"]:
            assert s["op"] in ("dchange", "ichange", "deflate", "inflate")
            f["deflates"] += s["op"] == "deflate"
            f["inflates"] += s["op"] == "inflate" and not s["rt"]
    rt = [c for c in doc["connections"] if any(s["op"] == "inflate" and s["rt"] for s in c["steps"])]
    got["roundtrip"] = {"connections": len(rt), "deflates": 0,
                        "inflates": sum(1 for c in rt for s in c["steps"] if s["op"] == "inflate" and s["rt"])}
    assert got == FAMILIES
    names = [(c["family"], c["name"]) for c in doc["connections"]]
    assert len(set(names)) == len(names)
    assert os.path.getsize(R.PATH) < (1 << 20)


def test_every_recorded_code_occurs():
    """HEADER_COMP from the inflater and (a bad deflater) from the deflater,
    INSUFF_BUFSIZE from deflate_hd2 and deflate_hd_vec2, INVALID_STATE and 0
    from inflate_change_table_size after a failed block; a failed block that
    emitted fields first, and one that left entries in the table."""
    doc = R.load()
    assert doc["error_codes"] == [HO.INSUFF_BUFSIZE, HO.HEADER_COMP, HO.INVALID_STATE]
    steps = [(c, k, s) for c in doc["connections"] for k, s in enumerate(c["steps"])]
    assert any(s["op"] == "inflate" and s["status"] == HO.HEADER_COMP for _, _, s in steps)
    assert any(s["op"] == "inflate" and s["status"] == HO.HEADER_COMP and s["fields"] for _, _, s in steps)
    assert any(s["op"] == "deflate" and s["rv"] == HO.HEADER_COMP for _, _, s in steps)
    for kind in ("hd2", "vec"):
        assert any(s["op"] == "deflate" and s["api"] and kind in s["api"] and s["rv"] == HO.INSUFF_BUFSIZE
                   for _, _, s in steps)
        assert any(s["op"] == "deflate" and s["api"] and kind in s["api"] and s["rv"] > 0 for _, _, s in steps)
    after_fail = {0: 0, HO.INVALID_STATE: 0}
    kept = 0
    for c in doc["connections"]:
        failed = False
        for k, s in enumerate(c["steps"]):
            if s["op"] == "inflate" and s["status"] < 0:
                if not failed and k and len(s["itable"]) > len(c["steps"][k - 1].get("itable", [])):
                    kept += 1
                failed = True
            elif s["op"] == "ichange" and failed:
                after_fail[s["rv"]] += 1
    assert after_fail[0] > 0 and after_fail[HO.INVALID_STATE] > 0, after_fail
    assert kept > 0


def test_config1_wire_is_the_reference_deflaters():
    """The generator deflated config 1's story with the reference, found
    config1_wire.json's wire and final table equal, and recorded the file's
    sha256: the committed file is that file."""
    cfg = R.load()["config1"]
    path = os.path.join(os.path.dirname(R.PATH), "config1_wire.json")
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == cfg["sha256"]
    assert cfg["cases"] == 1000


# ---------------------------------------------------------------------------
# adapters (the interface of tests/ref_hd_wire_lib.py's check_*_step)
# ---------------------------------------------------------------------------
def api_buflen(api):
    if api is None:
        return None
    return api["hd2"] if "hd2" in api else sum(api["vec"])


class OracleDeflater:
    def __init__(self, deflate_max):
        self.d = HO.Deflater(deflate_max)

    def change(self, v):
        self.d.change_table_size(v)
        return 0

    def bound(self, nva):
        return self.d.bound(nva)

    def deflate(self, nva, api):
        return self.d.deflate_hd2(nva, api_buflen(api))

    def state(self):
        return list(self.d.table), self.d.size, self.d.max


class OracleInflater:
    def __init__(self):
        self.i = HO.Inflater()

    def change(self, v):
        return self.i.change_table_size(v)

    def inflate(self, wire):
        st, fields = self.i.inflate_block(wire)
        return st, [(n, v, fl, HO.lookup_token(n)) for n, v, fl in fields]

    def state(self):
        return list(self.i.table), self.i.size, self.i.max


class COracleInflater(OracleInflater):
    def __init__(self):
        self.i = HO.CInflater()

    def state(self):
        return self.i.table, self.i.table_size(), self.i.table_max()


ProductDeflater, ProductInflater = R.ProductDeflater, R.ProductInflater


replay_deflate, replay_inflate = R.replay_deflate, R.replay_inflate


# ---------------------------------------------------------------------------
# the oracles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", DEFLATE_FAMILIES)
def test_oracle_deflater_equals_reference(family):
    conns = R.connections(family, "d")
    assert conns
    for c in conns:
        replay_deflate(c, OracleDeflater)


def _inflate_conns(family):
    if family == "roundtrip":
        return [c for c in R.connections(None, "i") if any(s["op"] == "inflate" and s["rt"] for s in c["steps"])]
    return [c for c in R.connections(family, "i") if any(s["op"] == "inflate" and not s["rt"] for s in c["steps"])]


@pytest.mark.parametrize("family", INFLATE_FAMILIES)
@pytest.mark.parametrize("make", [OracleInflater, COracleInflater], ids=["python", "c"])
def test_oracle_inflater_equals_reference(make, family):
    conns = _inflate_conns(family)
    assert conns
    for c in conns:
        replay_inflate(c, make)


# ---------------------------------------------------------------------------
# the product, where it makes no GPU call
# ---------------------------------------------------------------------------
def wire_has_huffman_literal(b):
    """Whether a wire, sound or not, shows a string literal with the H bit
    before the point where its framing ends (a scan of the representations
    that stops at the first byte it cannot frame)."""
    b = bytes(b)
    pos = 0

    def integer(prefix):
        nonlocal pos
        k = (1 << prefix) - 1
        n = b[pos] & k
        pos += 1
        if n == k:
            shift = 0
            while True:
                c = b[pos]
                pos += 1
                n += (c & 0x7F) << shift
                shift += 7
                if not c & 0x80:
                    break
        return n

    try:
        while pos < len(b):
            c = b[pos]
            if (c & 0xE0) == 0x20:
                integer(5)
            elif c & 0x80:
                integer(7)
            else:
                if c in (0x40, 0x00, 0x10):
                    pos += 1
                    if b[pos] & 0x80:
                        return True
                    n = integer(7)
                    pos += n
                else:
                    integer(6 if c & 0x40 else 4)
                if b[pos] & 0x80:
                    return True
                n = integer(7)
                pos += n
    except IndexError:
        pass
    return False


CPU_INFLATE = [c for c in R.connections(None, "i")
               if not any(s["op"] == "inflate" and wire_has_huffman_literal(s["wire"]) for s in c["steps"])]

def test_product_cpu_subsets_are_substantial():
    """The CPU subsets cover the table, integer, size-update and error
    families (the Huffman literals are the GPU file's)."""
    fams = {c["family"] for c in CPU_INFLATE}
    assert {"integers", "size_updates", "truncated", "after_error", "eviction", "lengths"} <= fams
    assert len(CPU_INFLATE) >= 200


@pytest.mark.parametrize("c", CPU_INFLATE, ids=lambda c: c["family"] + "/" + c["name"])
def test_product_inflate_cpu(c):
    replay_inflate(c, ProductInflater)
