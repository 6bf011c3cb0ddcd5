"""Every connection of tests/golden/ref_hd_wire.json (results recorded from
the reference's own deflater and inflater, tests/golden/make_ref_hd_wire.py)
through the product's front-ends: deflate_blocks, HpackDeflater.bound /
deflate_hd2 / deflate_hd_vec2, inflate_blocks(tokens=True) and the table
getters of both sides, bit-exact, after every step.

- the deflate connections in batches (one block of each connection per
  deflate_blocks call, round-robin as test_fuzz_corpus.py interleaves) and each
  alone, one call per block;
- the api family (bound, deflate_hd2 with buflen needed, needed - 1 and 0,
  deflate_hd_vec2 over one-byte chunks, one chunk, and a total one short);
- the inflate connections (the roundtrip wires included) in batches and each
  alone;
- the after_error and huffman families in every NGHTTP2_AMD_INFLATE_ZC mode,
  each in a fresh child process (the mode is read once per process).

CPU counterpart: tests/test_ref_hd_wire.py."""
import os
import subprocess
import sys

import pytest

from tests import ref_hd_wire_lib as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deflate_connections_in_batches():
    conns = R.connections(None, "d")
    assert len(conns) == 76
    calls = R.product_deflate_batched(conns)
    # as many calls as the longest connection has batched blocks, not one per block
    assert calls == max(sum(1 for s in c["steps"] if s["op"] == "deflate" and s["api"] is None) for c in conns)


def test_deflate_connections_alone():
    """One deflate_blocks call per block (the single-connection path)."""
    for c in R.connections(None, "d"):
        R.replay_deflate(c, R.ProductDeflater)


def test_api_family():
    conns = R.connections("api", "d")
    kinds = set()
    for c in conns:
        R.replay_deflate(c, R.ProductDeflater)
        kinds |= {(k, s["rv"] > 0) for s in c["steps"] if s["op"] == "deflate" and s["api"] for k in s["api"]}
    assert kinds == {("hd2", True), ("hd2", False), ("vec", True), ("vec", False)}
    assert sorted(len(s["nva"]) for c in conns if c["name"] == "bound" for s in c["steps"]
                  if s["op"] == "deflate") == [0, 1, 100]


def test_inflate_connections_in_batches():
    conns = R.connections(None, "i")
    assert len(conns) == 322
    calls = R.product_inflate_batched(conns)
    assert calls == max(sum(1 for s in c["steps"] if s["op"] == "inflate") for c in conns)


def test_inflate_connections_alone():
    """One inflate_blocks call per block."""
    for c in R.connections(None, "i"):
        R.replay_inflate(c, R.ProductInflater)


CHILD = r"""
import sys
sys.path.insert(0, %r)
from tests import ref_hd_wire_lib as R
conns = R.connections("after_error", "i") + R.connections("huffman", "i")
assert len(conns) == 49
R.product_inflate_batched(conns)
for c in conns:
    R.replay_inflate(c, R.ProductInflater)
print("REF-HD-WIRE-OK")
""" % (REPO,)


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_after_error_in_every_pool_mode(mode):
    """NGHTTP2_AMD_INFLATE_ZC is read once per process: a fresh child each."""
    env = dict(os.environ, NGHTTP2_AMD_INFLATE_ZC=mode)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0 and "REF-HD-WIRE-OK" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
