"""The inflater's metadata pool at the sizes where its layout can go wrong:
0..4 Huffman literals in the batch (0 launches nothing; 1 and 3 pad the
numbers to 8 bytes, 2 and 4 do not), and a batch whose Huffman literals are all
empty (the kernels' 16-byte read-ahead past the decoded pool).  Every call
level (plain, checks, tokens, checks + tokens, http) in every pinned-pool mode
(NGHTTP2_AMD_INFLATE_ZC, a fresh child process each).

Each Huffman literal is the Huffman form of a raw literal of a twin batch, and
every result of the call must equal the twin's, which runs on the host alone
(tests/test_inflate_levels.py pins that path)."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# two connections, a block each; the literals in the order they turn Huffman
FIELDS = [[(b"content-length", b"0042"), (b"te", b"trailers")], [(b":status", b"204"), (b"x-custom", b"v\x01bad")]]
ORDER = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 1)]  # (connection, field, name or value)
EMPTY = [[(b"x-empty", b""), (b"", b"")], [(b":path", b"")]]
EMPTY_ORDER = [(0, 0, 1), (0, 1, 0), (1, 0, 1)]


def _huffman(s):
    from oracle import oracle as O
    if not s:
        return b""
    enc, off = O.encode_batch(np.frombuffer(s, dtype=np.uint8), np.array([0, len(s)], dtype=np.uint32))
    return enc[:int(off[1])].tobytes()


def _blocks(fields, huff):
    from tests.http_fields_cases import hpack_int

    def lit(s, h):
        s = _huffman(s) if h else s
        return hpack_int(len(s), 7, 0x80 if h else 0) + s
    return [b"".join(b"\x40" + lit(n, (c, k, 0) in huff) + lit(v, (c, k, 1) in huff) for k, (n, v) in enumerate(fs))
            for c, fs in enumerate(fields)]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        else:
            assert x == y


def run_all():
    """Every batch at every level against its raw twin (the child's body)."""
    import nghttp2_amd
    from oracle import hpack_oracle as HO
    from tests import http_fields_ref as R
    from tests.test_inflate_levels import LEVELS, call
    batches = [(FIELDS, ORDER[:nh]) for nh in range(5)] + [(EMPTY, EMPTY_ORDER)]
    for fields, huff in batches:
        twin, wire = _blocks(fields, ()), _blocks(fields, set(huff))
        assert any(HO.block_has_huffman(b) for b in wire) == bool(huff)
        for level in LEVELS:
            res = []
            for blocks in (twin, wire):
                infs = [nghttp2_amd.HpackInflater() for _ in fields]
                res.append(call(level, infs, blocks, [R.MODE_REQUEST, 0]) + ([i.dynamic_table() for i in infs],))
            assert res[0][0] == [len(fs) for fs in fields], (level, len(huff))
            _same(res[0], res[1])
    print("POOL-LAYOUT-OK")


CHILD = "import sys; sys.path.insert(0, %r); from tests import test_inflate_pool_layout_gpu as P; P.run_all()" % REPO


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_small_literal_counts_equal_the_raw_twin(mode):
    env = dict(os.environ, NGHTTP2_AMD_INFLATE_ZC=mode)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=REPO, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "POOL-LAYOUT-OK" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
