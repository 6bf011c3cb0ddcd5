"""Name tokens from the inflate front-end with Huffman literals
(nghttp2_amd_hd_inflate_blocks_fields: k_name_tokens<true> queued behind the
batch's one decode, the tokens back in the status copy) on the GPU: a random
multi-connection batch from the oracle's deflater with churning tables and
corrupted blocks, every emitted field's token against the oracle's
lookup_token, with and without the check masks, in every
NGHTTP2_AMD_INFLATE_ZC pool mode."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd.workloads import TOKEN_NAMES
from oracle import hpack_oracle as HO

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LONG_NAME = b"x-a-header-name-of-more-than-twenty-eight-bytes"
NCONN = 10  # connections 0..7 from the deflater (tables of 4096 and 256), 8 and 9 turn bad


def make_batch(seed=5):
    """(conns, blocks): 8 connections x 6 blocks of about 8 fields from the
    oracle's deflater (Huffman wherever shorter; a table of 256 bytes on the
    odd connections, so entries are evicted all the time), one block with a
    Huffman-coded name of 47 bytes and a Huffman-coded value of 5,000, and two
    connections whose first block fails inside a Huffman literal (bad padding)
    after it has emitted fields."""
    rng = random.Random(seed)
    names = sorted(TOKEN_NAMES)
    misses = [n[:-1] for n in names[:12]] + [n + b"s" for n in names[12:24]] + [n.upper() for n in names[24:30]]
    custom = [b"x-request-id", b"x-trace", b"x-forwarded-for", LONG_NAME, b"x-b3-traceid-of-some-length-too"]
    defl = [HO.Deflater(4096 if c % 2 == 0 else 256) for c in range(8)]
    conns, blocks = [], []
    for r in range(6):
        for c in range(8):
            fields = []
            for _ in range(rng.randint(5, 11)):
                p = rng.random()
                n = rng.choice(names) if p < 0.6 else rng.choice(misses) if p < 0.75 else rng.choice(custom)
                v = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789/=;. ") for _ in range(rng.randint(0, 48)))
                if rng.random() < 0.3:  # a value seen before: indexed fields and indexed names
                    v = b"v%d" % rng.randint(0, 3)
                fields.append((n, v))
            if r == 2 and c == 3:
                fields.insert(2, (LONG_NAME, bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(5000))))
            conns.append(c)
            blocks.append(defl[c].deflate_block(fields))
        if r == 1:  # a field, a Huffman name (te), then a Huffman name whose padding is no EOS prefix
            conns.append(8)
            blocks.append(b"\x82" + b"\x00\x82\x49\x7f\x01v" + b"\x00\x81\x00\x01v" + b"\x84")
        if r == 3:  # the same inside the value, behind a static name
            conns.append(9)
            blocks.append(b"\x86\x84" + b"\x0f\x10\x81\x00" + b"\x82")
        if r == 4:  # the bad connections again: nothing more from them
            conns += [8, 9]
            blocks += [b"\x82", b"\x82"]
    return conns, blocks


def check_batch():
    """The batch through tokens=True and through checks=True, tokens=True on
    fresh inflaters: statuses and fields against the oracle's inflater, tokens
    against its lookup_token, masks equal to the checked call's."""
    conns, blocks = make_batch()
    assert 40 <= len(blocks) <= 60 and any(HO.block_has_huffman(b) for b in blocks)
    refs = [HO.Inflater() for _ in range(NCONN)]
    want = [refs[c].inflate_block(b) for c, b in zip(conns, blocks)]
    flat = [x for _, fb in want for x in fb]
    want_tk = [HO.lookup_token(n) for n, _, _ in flat]
    assert 300 <= len(flat) <= 600 and sum(t >= 0 for t in want_tk) > 150
    assert [s for s, _ in want].count(nghttp2_amd.NGHTTP2_ERR_HEADER_COMP) == 4
    assert any(n == LONG_NAME and len(v) == 5000 for n, v, _ in flat)
    k8 = conns.index(8)
    assert want[k8] == (nghttp2_amd.NGHTTP2_ERR_HEADER_COMP, [(b":method", b"GET", 0), (b"te", b"v", 0)])
    assert want[conns.index(9)][0] == nghttp2_amd.NGHTTP2_ERR_HEADER_COMP and len(want[conns.index(9)][1]) == 2

    def fresh():
        infs = [nghttp2_amd.HpackInflater() for _ in range(NCONN)]
        return [infs[c] for c in conns]
    st, f, tk = nghttp2_amd.inflate_blocks(fresh(), blocks, tokens=True)
    assert list(zip(st, f)) == want
    assert tk.dtype == np.int32 and tk.tolist() == want_tk
    st_c, f_c, m_c = nghttp2_amd.inflate_blocks(fresh(), blocks, checks=True)
    st_b, f_b, m_b, tk_b = nghttp2_amd.inflate_blocks(fresh(), blocks, checks=True, tokens=True)
    assert list(zip(st_b, f_b)) == want and list(zip(st_c, f_c)) == want
    assert np.array_equal(m_b, m_c) and m_b.shape == (len(flat), 2)
    assert tk_b.tolist() == want_tk
    # one connection alone (the direct sink): connection 3, with the long name and value
    mine = [b for c, b in zip(conns, blocks) if c == 3]
    inf = nghttp2_amd.HpackInflater()
    st1, f1, tk1 = nghttp2_amd.inflate_blocks([inf] * len(mine), mine, tokens=True)
    assert list(zip(st1, f1)) == [w for c, w in zip(conns, want) if c == 3]
    assert tk1.tolist() == [HO.lookup_token(n) for fb in f1 for n, _, _ in fb]
    # an untokened call's entries, referenced by a tokened one
    half = len(blocks) // 2
    infs = fresh()
    st2, f2 = nghttp2_amd.inflate_blocks(infs[:half], blocks[:half])
    st3, f3, tk3 = nghttp2_amd.inflate_blocks(infs[half:], blocks[half:], tokens=True)
    assert list(zip(st2 + st3, f2 + f3)) == want
    assert tk3.tolist() == want_tk[sum(len(x) for x in f2):]


def test_tokens_of_a_huffman_batch():
    check_batch()


def test_tokens_of_a_huffman_batch_in_every_pool_mode():
    """NGHTTP2_AMD_INFLATE_ZC is read once per process: a fresh child per mode,
    each under its own time limit; the first one that fails ends the test."""
    child = "import sys; sys.path.insert(0, %r); from tests import test_inflate_tokens_gpu as T; " \
            "T.check_batch(); print('TOKENS-OK')" % REPO
    for mode in ("0", "1", "2"):
        env = dict(os.environ, NGHTTP2_AMD_INFLATE_ZC=mode)
        r = subprocess.run([sys.executable, "-c", child], env=env, cwd=REPO, capture_output=True, text=True,
                           timeout=110)
        assert r.returncode == 0 and "TOKENS-OK" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
