"""GPU parity on the string-literal grids of tests/boundary_batches.py
(k_encode<FR>, nghttp2_amd_hd_emit_strings_batch): the H/raw tie, the length
prefix's boundaries, raw strings in the round's byte mask, runs of empty
strings, pairs on both sides of 64 bits, string starts at round edges and the
fullest image -- bit-exact against the oracle's emit_string (offsets and every
byte), as built (the one-tile launch where n <= 256), in tiles of <= 256
strings, behind a tile of fill (count + pack launches) and shifted by 1 and 33
strings; the same grids through the plain encode; the bytes past dst_cap; and
a header list that reaches the bytewise path through the deflater.
tests/test_boundary_batches.py proves on the CPU that the grids hit what they
claim.
"""
import functools

import numpy as np
import pytest

from oracle import hpack_oracle as HO
from oracle import oracle as O
from tests import boundary_batches as BB
from tests.test_parity_gpu import check_emit, check_roundtrip, pad16, to_dev

pytestmark = pytest.mark.gpu

FAMILIES = BB.LIT_FAMILIES


@functools.lru_cache(maxsize=None)
def family(name):
    return getattr(BB, name)()


def all_empty_batches():
    return [("all-empty n=%d" % n, BB.lit_all_empty(n)) for n in BB.ALL_EMPTY_N]


@pytest.mark.parametrize("name", FAMILIES)
def test_literals_plain_and_filled(codec, dev, name):
    b = family(name)
    check_emit(codec, dev, b[0], b[1], name)
    if len(b[1]) - 1 > 256:  # every tile alone: the one-tile launch
        for k, (pool, off) in enumerate(BB.tile_chunks(b)):
            check_emit(codec, dev, pool, off, "%s tile %d" % (name, k))
    pool, off = BB.with_fill(b)
    check_emit(codec, dev, pool, off, name + " filled")
    if name == "lit_empties":
        for tag, (pool, off) in all_empty_batches():
            check_emit(codec, dev, pool, off, tag)


@pytest.mark.parametrize("j", [1, 33])
@pytest.mark.parametrize("name", FAMILIES)
def test_literals_shifted(codec, dev, name, j):
    pool, off = BB.shifted(family(name), j)
    check_emit(codec, dev, pool, off, "%s shifted %d" % (name, j))


@pytest.mark.parametrize("name", FAMILIES)
def test_plain_encode_same_grids(codec, dev, name):
    b = family(name)
    check_roundtrip(codec, dev, b[0], b[1], name)
    pool, off = BB.with_fill(b)
    check_roundtrip(codec, dev, pool, off, name + " filled")
    if name == "lit_empties":
        for tag, (pool, off) in all_empty_batches():
            check_roundtrip(codec, dev, pool, off, tag)


@pytest.mark.parametrize("name", FAMILIES)
def test_count_launch_tile_totals(codec, dev, name):
    """k_enc_count<true>'s per-tile totals (prefix + min(E, R) bytes of 256
    strings), read off the literal offsets of the two-launch run."""
    pool, off = BB.with_fill(family(name))
    n = len(off) - 1
    assert n > 256
    src = to_dev(pad16(pool, off[-1]), dev)
    _, do = codec.emit_strings(src, to_dev(off, dev), raw_bytes=int(off[-1]))
    do = do.cpu().numpy().view(np.uint32).astype(np.int64)
    S = BB.literal_strings(pool, off)
    rdo = O.emit_strings_batch(pool, off)[1].astype(np.int64)
    assert np.array_equal(S["lo"], rdo)
    tiles = list(range(0, n, 256)) + [n]
    assert np.array_equal(np.diff(do[tiles]), np.diff(rdo[tiles])), name + ": tile totals"
    assert np.array_equal(np.diff(do), S["PL"] + S["P"]), name + ": literal lengths"


@pytest.mark.parametrize("name", FAMILIES)
def test_no_write_past_capacity(codec, dev, name):
    """dst of exactly emit_strings_bound bytes inside a larger 0xA5 buffer:
    the literals are the oracle's and the bytes at and past dst_cap stay."""
    import torch
    b = family(name)
    for tag, (pool, off) in ((name, b), (name + " filled", BB.with_fill(b))):
        raw, n = int(off[-1]), len(off) - 1
        bound = codec.L.nghttp2_amd_hd_emit_strings_bound(raw, n)
        big = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device=dev)
        dst, do = codec.emit_strings(to_dev(pad16(pool, raw), dev), to_dev(off, dev), raw_bytes=raw,
                                     dst=big[:bound])
        torch.cuda.synchronize()
        rd, rdo = O.emit_strings_batch(pool, off)
        assert np.array_equal(do.cpu().numpy().view(np.uint32), rdo), tag + ": literal offsets"
        out = big.cpu().numpy()
        assert np.array_equal(out[:int(rdo[-1])], rd), tag + ": literals"
        assert (out[bound:] == 0xA5).all(), tag + ": bytes past dst_cap written"
        assert (out[int(rdo[-1]):bound] == 0xA5).all(), tag + ": bytes past the last literal written"


def test_deflater_reaches_bytewise_path(dev):
    """12 never-indexed fields with static names and empty values between two
    ordinary fields: 12 one-byte literals behind one byte (a pair of 100+
    bits, tests/test_boundary_batches.py) -- the product's wire is the oracle
    deflater's, and the product's inflater gives the fields back."""
    import nghttp2_amd
    fields = BB.no_index_fields()
    lists = [fields, fields[:1] + fields[-1:], fields]
    want, r = [], HO.Deflater()
    for hl in lists:
        want.append(r.deflate_block(hl))
    d = nghttp2_amd.HpackDeflater()
    st, wire = nghttp2_amd.deflate_blocks([d] * len(lists), lists)
    assert wire == want and st == [len(w) for w in want]
    assert d.dynamic_table() == [tuple(e) for e in r.table]
    inf = nghttp2_amd.HpackInflater()
    ist, got = nghttp2_amd.inflate_blocks([inf] * len(lists), want)
    rinf = HO.Inflater()
    for k, hl in enumerate(lists):
        assert ist[k] == len(hl)
        assert [(n, v) for n, v, _ in got[k]] == [(n, v) for n, v, _ in hl]
        assert [f & BB.NO_INDEX for _, _, f in got[k]] == [f for _, _, f in hl]
        assert [(n, v) for n, v, _ in rinf.inflate_block(want[k])[1]] == [(n, v) for n, v, _ in hl]
