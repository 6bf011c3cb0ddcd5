"""nghttp2_amd_hd_http_facts_batch (k_http_facts) and the _http inflate on the
GPU, bit-exact against the restatement of nghttp2_http_on_header
(tests/http_fields_ref.py): every byte value, the short literals and their
near misses, parse_uint at its limits, a refused byte at every chunk and round
edge of strings at pool offsets 0, 1, 15 and 16 among neighbours full of
refused bytes, the `len` form on the real output of decode_batch_auto, and
the corpus of tests/golden/http_fields.json deflated with Huffman literals in
every NGHTTP2_AMD_INFLATE_ZC mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nghttp2_amd import workloads as W
from oracle import oracle as O
from tests import http_fields_ref as R
from tests.string_batches import lay_out

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FACTS = {}


def ref_facts(s):
    f = _FACTS.get(s)
    if f is None:
        f = _FACTS[s] = R.facts(s)
    return f


def run(codec, dev, strings, lead=b"", tail=b""):
    """The facts of `strings` laid back to back after `lead` (bytes before
    off[0]), with `tail` after off[n] and the pool padded by the contract."""
    import torch
    pool, off = lay_out(strings, lead, tail)
    f, n = codec.http_facts_batch(torch.from_numpy(pool).to(dev), torch.from_numpy(off.view(np.int32)).to(dev))
    return f.cpu().numpy().view(np.uint32), n.cpu().numpy()


def expect(codec, dev, strings, **kw):
    f, n = run(codec, dev, strings, **kw)
    want = [ref_facts(s) for s in strings]
    got = list(zip(f.tolist(), n.tolist()))
    bad = [i for i in range(len(strings)) if got[i] != want[i]]
    assert not bad, [(i, strings[i][:40], len(strings[i]), got[i], want[i]) for i in bad[:6]]


LITERALS = [b"HEAD", b"HEAd", b"HEA", b"HEADS", b"CONNECT", b"CONNECTS", b"CONNECt", b"OPTIONS", b"OPTIONs",
            b"http", b"HTTP", b"https", b"HTTPS", b"httpx", b"htt", b"TrAiLeRs", b"trailers", b"trailerz",
            b"trailers ", b"*", b"**", b"/", b"/index", b"x/", b"0", b"007", b"", b" ", b" \t \t", b" a",
            b"9223372036854775807", b"9223372036854775808", b"18446744073709551616", b"99999999999999999999",
            b"00009223372036854775807", b"0" * 1000 + b"7", b"0" * 1000, b"0" * 999 + b"x", b"h2+x-y.z", b"2h",
            b"localhost:8080", b"user@host", b"[::1]", b"@", b"H\x00AD", b"\xe8EAD"]


def test_every_byte_value_and_the_literals(codec, dev):
    expect(codec, dev, [bytes([c]) for c in range(256)] + LITERALS)
    # the same at other alignments, and in a batch of more than one workgroup
    expect(codec, dev, LITERALS * 7, lead=b"@" * 3)
    for shift in (1, 5, 9, 15):
        expect(codec, dev, [b"0" * 1000 + b"7", b"0" * 40, b"1" + b"0" * 18, b"1" + b"0" * 19], lead=b"0" * shift)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mixed_batches(codec, dev, n):
    rng = np.random.Generator(np.random.PCG64(n))
    strings = []
    for _ in range(n):
        s = LITERALS[rng.integers(0, len(LITERALS))]
        if rng.random() < 0.3:
            s = s * int(rng.integers(2, 12))
        strings.append(s)
    expect(codec, dev, strings)


GRID_LENGTHS = [1, 15, 16, 17, 1023, 1024, 1025, 65536]
# chunk edges (16 bytes) and round edges (64 chunks: 1024 bytes; the loop takes two rounds a turn)
GRID_POS = [0, 1, 14, 15, 16, 17, 1007, 1008, 1022, 1023, 1024, 1025, 2047, 2048, 65519, 65520]


@pytest.mark.parametrize("length", GRID_LENGTHS)
def test_position_grid(codec, dev, length):
    """One '@' (no authority byte, no scheme byte, no digit), one 'a' (no
    digit) and one '7' (the number's first significant digit: its value, or
    the overflow past 19 digits, depends on where the kernel finds it) at
    every chunk and round edge of a string of zeros -- an authority, a number
    with value 0 -- at pool offsets 0, 1, 15 and 16; the bytes before and
    behind the string are '@', so a byte leaking across its ends shows."""
    base = b"0" * length
    assert ref_facts(base)[0] & (R.FACT_AUTHORITY | R.FACT_UINT) == R.FACT_AUTHORITY | R.FACT_UINT
    strings = [base]
    for pos in sorted({p for p in GRID_POS if p < length} | {length - 1}):
        for bad in (b"@", b"a", b"7"):
            strings.append(base[:pos] + bad + base[pos + 1:])
    # the first significant digit within 19 bytes of the end, at every distance
    strings += [b"0" * (length - k) + b"7" + b"1" * (k - 1) for k in range(1, min(length, 21) + 1)]
    for shift in (0, 1, 15, 16):
        for s in strings:
            expect(codec, dev, [s], lead=b"@" * shift, tail=b"@" * 40)
        # and as a string among strings of '@'
        expect(codec, dev, [b"@" * 17, strings[0], b"@", strings[-1], b"@" * 33], lead=b"@" * shift, tail=b"@" * 40)


def test_whole_string_properties_of_long_strings(codec, dev):
    """70,000 bytes, one refused byte at the end, among short strings of one wave."""
    short = [b"ok", b"", b"HEAD", b"7", b"/"]
    strings = short + [b"a" * 70000, b"a" * 69999 + b"@", b" " * 70000, b" " * 69999 + b"x"] + short + \
        [b"0" * 70000, b"0" * 69999 + b"9", b"0" * 69980 + b"9" * 20, b"1" * 70000, b"a" + b"+" * 69999,
         b"0" * 69981 + b"9223372036854775807", b"0" * 69981 + b"9223372036854775808", b"0" * 35000 + b"5" + b"0" * 18,
         b"0" * 35000 + b"5" + b"0" * 19]
    expect(codec, dev, strings)
    expect(codec, dev, strings, lead=b"@" * 7)


def test_null_arguments(codec, dev):
    import nghttp2_amd
    L = nghttp2_amd.lib()
    assert L.nghttp2_amd_hd_http_facts_batch(None, None, None, 0, None, None, None) == 0
    assert L.nghttp2_amd_hd_http_facts_batch(None, None, None, 3, None, None, None) == \
        nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT


def test_len_form_on_decode_output(codec, dev):
    """decode_batch_auto's (dst, dst_off, status) as is: task gaps between the
    strings, failed strings (INVALID, number -1), and a hand-made overrun."""
    import torch
    pool, off = W.gen_mixed_values(200)
    enc, enc_off = O.encode_batch(pool, off)
    enc = enc.copy()
    corrupt = (3, 64, 199)
    for i in corrupt:
        enc[int(enc_off[i + 1]) - 1] = 0x00  # a last byte that is no EOS prefix
    E = int(enc_off[-1])
    epool = np.zeros((E + 15) // 16 * 16 + 16, dtype=np.uint8)
    epool[:E] = enc[:E]
    rdst, rdoff, rst, _, _ = O.decode_batch(epool[:E + 16], enc_off)
    dst, dst_off, status = codec.decode_auto(torch.from_numpy(epool).to(dev),
                                             torch.from_numpy(enc_off.view(np.int32)).to(dev), enc_bytes=E)
    f, n = codec.http_facts_batch(dst, dst_off, len=status)
    st = status.cpu().numpy()
    assert np.array_equal(st, rst)
    assert np.any(st < 0) and np.any(st > 0)
    do = dst_off.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.any(do[1:-1] != do[:-2] + st[:-1]), "no task gap in this batch"
    want = [(R.FACT_INVALID, -1) if rst[i] < 0 else
            R.facts(rdst[int(rdoff[i]):int(rdoff[i]) + int(rst[i])].tobytes()) for i in range(len(off) - 1)]
    assert list(zip(f.cpu().numpy().view(np.uint32).tolist(), n.cpu().numpy().tolist())) == want
    i = 5
    assert do[i + 1] - do[i] == st[i]
    ln = status.clone()
    ln[i] = int(st[i]) + 1
    f2, n2 = codec.http_facts_batch(dst, dst_off, len=ln)
    want[i] = (R.FACT_INVALID, -1)
    assert list(zip(f2.cpu().numpy().view(np.uint32).tolist(), n2.cpu().numpy().tolist())) == want


CHILD = r"""
import sys
sys.path.insert(0, %r)
import nghttp2_amd
from nghttp2_amd import hd as H
from tests import field_checks_ref as FC
from tests import http_fields_cases as C
lit = C.huff_lit()
want = [f for _, _, fs in C.blocks() for f in fs]
for nconn, kw in ((5, dict(checks=True, tokens=True)), (1, {}), (5, dict(nva_cap=9, arena_cap=700))):
    conn, wire, modes, states = C.wire(lit, nconn)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    res = nghttp2_amd.inflate_blocks([infs[c] for c in conn], wire, http=modes, http_state=states, **kw)
    assert [(n, v) for fs in res[1] for n, v, _ in fs] == want
    if "checks" in kw:
        assert res[2].tolist() == [[FC.mask(n), FC.mask(v)] for n, v in want]
        assert res[3].tolist() == [H.lookup_token(n) for n, _ in want]
    C.check_http(res)
print("HTTP-OK")
""" % (REPO,)


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_http_inflate_in_every_pool_mode(mode):
    """NGHTTP2_AMD_INFLATE_ZC is read once per process: a fresh child each."""
    env = dict(os.environ, NGHTTP2_AMD_INFLATE_ZC=mode)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0 and "HTTP-OK" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
