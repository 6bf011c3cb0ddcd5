"""nghttp2_amd_hd_check_fields_batch (k_check_fields) and the checked inflate
on the GPU, bit-exact against the restatement of nghttp2_check_*
(tests/field_checks_ref.py): batch sizes around a wave and a workgroup, every
byte value, a violating byte at every chunk and round edge of strings at every
alignment, the isolation of a string from the bytes around it, strings whose
violation counts would wrap an 8- or 16-bit field, and the `len` form on the
real output of decode_batch_auto."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nghttp2_amd import workloads as W
from oracle import oracle as O
from tests import field_checks_ref as R
from tests.string_batches import lay_out

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MASKS = {}


def ref_mask(s):
    """R.mask, remembered (the grids repeat strings)."""
    m = _MASKS.get(s)
    if m is None:
        m = _MASKS[s] = R.mask(s)
    return m


def run(codec, dev, strings, lead=b"", tail=b"", gap=None):
    """The masks of `strings` laid back to back after `lead` (bytes before
    off[0]), with `tail` after off[n] and the pool padded by the contract
    (zeros to align_up(off[n], 16) + 16 -- bytes that violate every table)."""
    import torch
    pool, off = lay_out(strings, lead, tail)
    m = codec.check_fields(torch.from_numpy(pool).to(dev), torch.from_numpy(off.view(np.int32)).to(dev))
    return m.cpu().numpy()


def expect(codec, dev, strings, **kw):
    got = run(codec, dev, strings, **kw)
    want = np.array([ref_mask(s) for s in strings], dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), strings[i][:40], len(strings[i]), hex(got[i]), hex(want[i])) for i in bad[:6]]


# strings that pass and that violate each class
BANK = [b"content-type", b":path", b":", b"", b"GET", b"Get", b"/index.html?q=1", b"/a b", b"example.com:443",
        b"user@host", b"ex ample", b"text/html; charset=utf-8", b" lead", b"trail ", b"tab\there", b"\tx",
        b"nul\x00", b"\x7f", b"caf\xc3\xa9", b"a" * 16, b"b" * 17, b"x" * 31 + b"{", b"UPPER-case", b"na:me",
        b"[::1]:8080", b"p%20q", b"q\"uote", b"~tilde`|", b"(paren)", b"a,b;c=d"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mixed_batches(codec, dev, n):
    rng = np.random.Generator(np.random.PCG64(n))
    strings = []
    for k in range(n):
        s = BANK[rng.integers(0, len(BANK))]
        if rng.random() < 0.3:  # a longer run of it, with or without a violating byte inside
            s = s * int(rng.integers(2, 12))
        strings.append(s)
    expect(codec, dev, strings)


def test_every_byte_value(codec, dev):
    expect(codec, dev, [bytes([c]) for c in range(256)] + [b":" + bytes([c]) for c in range(256)])


GRID_LENGTHS = [1, 15, 16, 17, 1024, 1025, 2049]
GRID_POS = [0, 14, 15, 16, 17, 1022, 1023, 1024, 1025]
GRID_BAD = [b"\x00", b"A", b"@", b" "]


def grid_strings(length):
    out = [b"a" * length]
    for pos in sorted({p for p in GRID_POS if p < length} | {length - 1}):
        for bad in GRID_BAD:
            out.append(b"a" * pos + bad + b"a" * (length - pos - 1))
    return out


@pytest.mark.parametrize("length", GRID_LENGTHS)
def test_position_grid(codec, dev, length):
    """One violating byte at every chunk and round edge; the string at pool
    offsets 0, 1, 15 and 16 (a string of that length in front shifts it)."""
    for s in grid_strings(length):
        for shift in (0, 1, 15, 16):
            expect(codec, dev, ([b"a" * shift] if shift else []) + [s])


def test_position_grid_in_one_batch(codec, dev):
    """The grid's strings of every length back to back, at whatever alignment
    that gives them, behind 0..3 leading one-byte strings."""
    strings = [s for length in GRID_LENGTHS for s in grid_strings(length)]
    for lead in range(4):
        expect(codec, dev, [b"a"] * lead + strings)


def test_isolation(codec, dev):
    clean = b"a" * 40
    # neighbours that end and begin with a violating byte inside its first and last chunk
    for pre in (b"aaaa\x00", b"\x00", b"b" * 15 + b"\x00", b"b" * 31 + b" "):
        for post in (b"\x00aaa", b"\x00", b"A" + b"b" * 20):
            for body in (clean, b"a", b"a" * 16, b"a" * (32 - len(pre) % 16)):
                expect(codec, dev, [pre, body, post])
    expect(codec, dev, [b"", clean, b""])
    expect(codec, dev, [b"\x00", b"", clean, b"", b"\x00"])
    # violating bytes just before off[0] and just past off[n]
    for lead in (b"\x00", b"\x00" * 5, b"\x00" * 16, b" A\x00" * 11):
        expect(codec, dev, [clean], lead=lead, tail=b"\x00 A@" * 8)
        expect(codec, dev, [clean, b"", b"a" * 7], lead=lead, tail=b"\x00" * 32)


def test_violation_counts_that_would_wrap(codec, dev):
    """256, 65,536 and 70,000 violating bytes (a packed 8- or 16-bit count of
    them is 0 again), and one violating byte at the end of 70,000 clean ones,
    among short strings in one wave."""
    short = [b"ok", b"", b"A", b"x" * 20, b":status"]
    strings = short + [b"\x00" * 256] + short + [b"\x00" * 65536, b"a"] + [b"\x00" * 70000] + short + \
        [b"a" * 69999 + b"\x00"] + short + [b"a" * 70000, b" " * 256, b"A" * 65536]
    assert len(strings) < 64
    expect(codec, dev, strings)
    expect(codec, dev, strings, lead=b"\x00" * 7)


def test_first_offset_not_zero_and_runs_of_empty_strings(codec, dev):
    expect(codec, dev, [b"abc", b"D"], lead=b"x" * 1000)
    expect(codec, dev, [b"abc"] + [b""] * 70 + [b" d", b"e" * 100] + [b""] * 70)
    expect(codec, dev, [b""] * 70)
    expect(codec, dev, [b""] * 70, lead=b"\x00" * 16)


def test_null_arguments(codec, dev):
    import nghttp2_amd
    L = nghttp2_amd.lib()
    assert L.nghttp2_amd_hd_check_fields_batch(None, None, None, 0, None, None) == 0
    assert L.nghttp2_amd_hd_check_fields_batch(None, None, None, 3, None, None) == \
        nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT


def _decoded_and_checked(codec, dev, pool, off, corrupt=()):
    """Encode (oracle), corrupt the last byte of some encodings, decode_auto,
    then check_fields on (dst, dst_off, status) in the same stream."""
    import torch
    enc, enc_off = O.encode_batch(pool, off)
    enc = enc.copy()
    for i in corrupt:
        enc[int(enc_off[i + 1]) - 1] = 0x00  # a last byte that is no EOS prefix
    E = int(enc_off[-1])
    epool = np.zeros((E + 15) // 16 * 16 + 16, dtype=np.uint8)
    epool[:E] = enc[:E]
    rdst, rdoff, rst, _, _ = O.decode_batch(epool[:E + 16], enc_off)
    dst, dst_off, status = codec.decode_auto(torch.from_numpy(epool).to(dev),
                                             torch.from_numpy(enc_off.view(np.int32)).to(dev), enc_bytes=E)
    mask = codec.check_fields(dst, dst_off, len=status)
    st = status.cpu().numpy()
    assert np.array_equal(st, rst)
    want = np.array([R.CHECK_INVALID if rst[i] < 0 else
                     R.mask(rdst[int(rdoff[i]):int(rdoff[i]) + int(rst[i])].tobytes())
                     for i in range(len(off) - 1)], dtype=np.uint8)
    return mask.cpu().numpy(), want, (dst, dst_off, status)


def test_len_form_on_decode_output_with_task_gaps(codec, dev):
    pool, off = W.gen_mixed_values(200)
    got, want, (dst, dst_off, status) = _decoded_and_checked(codec, dev, pool, off)
    do = dst_off.cpu().numpy().view(np.uint32).astype(np.int64)
    st = status.cpu().numpy()
    assert np.any(do[1:-1] != do[:-2] + st[:-1]), "no task gap in this batch"
    assert np.array_equal(got, want)
    assert not np.any(want == R.CHECK_INVALID)
    # a hand-made length that overruns the next string's offset
    i = 5
    assert do[i + 1] - do[i] == st[i]
    ln = status.clone()
    ln[i] = int(st[i]) + 1
    got2 = codec.check_fields(dst, dst_off, len=ln).cpu().numpy()
    want2 = want.copy()
    want2[i] = R.CHECK_INVALID
    assert np.array_equal(got2, want2)


def test_len_form_with_failed_decodes(codec, dev):
    pool, off = W.gen_pseudo_headers(200)
    corrupt = (3, 64, 199)
    got, want, _ = _decoded_and_checked(codec, dev, pool, off, corrupt=corrupt)
    assert [int(i) for i in np.flatnonzero(want == R.CHECK_INVALID)] == list(corrupt)
    assert np.array_equal(got, want)
    assert all(got[i] == 0x80 for i in corrupt)


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import nghttp2_amd
import bench_rows
from tests import field_checks_ref as R
blocks, conns = bench_rows.make_blocks(8, 8, 4, index=True)
assert len(blocks) == 64
# a ninth connection: a field, then a Huffman name whose padding is no EOS prefix
blocks.append(b"\x82" + b"\x00" + b"\x81\x00" + b"\x01v")
conns.append(8)
a = [nghttp2_amd.HpackInflater() for _ in range(9)]
b = [nghttp2_amd.HpackInflater() for _ in range(9)]
st0, f0 = nghttp2_amd.inflate_blocks([a[c] for c in conns], blocks)
st1, f1, m = nghttp2_amd.inflate_blocks([b[c] for c in conns], blocks, checks=True)
assert (st0, f0) == (st1, f1)
assert st1[-1] == nghttp2_amd.NGHTTP2_ERR_HEADER_COMP and len(f1[-1]) == 1 and min(st1[:-1]) > 0
flat = [x for fb in f1 for x in fb]
assert m.shape == (len(flat), 2)
for k, (n, v, _) in enumerate(flat):
    assert (int(m[k, 0]), int(m[k, 1])) == (R.mask(n), R.mask(v)), (k, n, v)
# the same connections again: names and values now come from the tables too
blocks2 = [bytes([0xbe, 0xbf]) + x for x in blocks[:64]]
st2, f2, m2 = nghttp2_amd.inflate_blocks([b[c] for c in conns[:64]], blocks2, checks=True)
flat = [x for fb in f2 for x in fb]
assert min(st2) > 0 and m2.shape == (len(flat), 2)
for k, (n, v, _) in enumerate(flat):
    assert (int(m2[k, 0]), int(m2[k, 1])) == (R.mask(n), R.mask(v)), (k, n, v)
print("CHECKED-OK")
""" % (REPO, os.path.join(REPO, "tools"))


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_checked_inflate_in_every_pool_mode(mode):
    """NGHTTP2_AMD_INFLATE_ZC is read once per process: a fresh child each."""
    env = dict(os.environ, NGHTTP2_AMD_INFLATE_ZC=mode)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0 and "CHECKED-OK" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
