"""What k_check_fields and k_http_facts have in common (the range rule of
csrc/hd_string_walk.h, the wave walk, the edge fold), held to the same cases over both kernels
against their restatements (tests/field_checks_ref.py, http_fields_ref.py):
the isolation of a string from the bytes around it, offsets that do not start
at 0 and runs of empty strings, the strings that are not examined, and the
exits of the walk's two-buffer loop.  And the one name-token kernel body
through its two entry points (hpack_oracle.name_tokens)."""
import numpy as np
import pytest

from nghttp2_amd import workloads as W
from oracle import hpack_oracle as H
from tests import field_checks_ref as CR
from tests import http_fields_ref as HR
from tests import string_batches as B

pytestmark = pytest.mark.gpu

_REF = {"check": {}, "facts": {}}


def want_of(kernel, s):
    """The restatement's result for string s (None: not examined), remembered."""
    if s is None:
        return CR.CHECK_INVALID if kernel == "check" else (HR.FACT_INVALID, -1)
    r = _REF[kernel].get(s)
    if r is None:
        r = _REF[kernel][s] = CR.mask(s) if kernel == "check" else HR.facts(s)
    return r


def got_of(kernel, codec, dev, pool, off, ln=None):
    import torch
    t_pool = torch.from_numpy(pool).to(dev)
    t_off = torch.from_numpy(np.asarray(off, dtype=np.uint32).view(np.int32)).to(dev)
    t_len = None if ln is None else torch.from_numpy(np.asarray(ln, dtype=np.int32)).to(dev)
    if kernel == "check":
        return codec.check_fields(t_pool, t_off, len=t_len).cpu().numpy().tolist()
    f, n = codec.http_facts_batch(t_pool, t_off, len=t_len)
    return list(zip(f.cpu().numpy().view(np.uint32).tolist(), n.cpu().numpy().tolist()))


def expect(kernel, codec, dev, strings, lead=b"", tail=b""):
    got = got_of(kernel, codec, dev, *B.lay_out(strings, lead, tail))
    want = [want_of(kernel, s) for s in strings]
    bad = [i for i in range(len(strings)) if got[i] != want[i]]
    assert not bad, [(i, strings[i][:40], len(strings[i]), got[i], want[i]) for i in bad[:6]]


KERNELS = ["check", "facts"]
# bytes that change a clean string's result if one leaks into it: 'a' is clean
# for every check, '0' is an authority, a scheme byte and a number of value 0
CLEAN = {"check": b"a", "facts": b"0"}


@pytest.mark.parametrize("kernel", KERNELS)
def test_isolation(codec, dev, kernel):
    c = CLEAN[kernel]
    clean = c * 40
    # neighbours that end and begin with a refused byte inside its first and last chunk
    for pre in (c * 4 + b"\x00", b"\x00", b"b" * 15 + b"\x00", b"b" * 31 + b" ", b"7@"):
        for post in (b"\x00" + c * 3, b"\x00", b"A" + b"b" * 20, b"@7"):
            for body in (clean, c, c * 16, c * (32 - len(pre) % 16)):
                expect(kernel, codec, dev, [pre, body, post])
    expect(kernel, codec, dev, [b"", clean, b""])
    expect(kernel, codec, dev, [b"\x00", b"", clean, b"", b"\x00"])
    # refused bytes just before off[0] and just past off[n]
    for lead in (b"\x00", b"\x00" * 5, b"\x00" * 16, b" A\x00" * 11, b"@7" * 4):
        expect(kernel, codec, dev, [clean], lead=lead, tail=b"\x00 A@" * 8)
        expect(kernel, codec, dev, [clean, b"", c * 7], lead=lead, tail=b"\x00" * 32)


@pytest.mark.parametrize("kernel", KERNELS)
def test_first_offset_not_zero_and_runs_of_empty_strings(codec, dev, kernel):
    expect(kernel, codec, dev, [b"abc", b"D", b"007"], lead=b"x" * 1000)
    expect(kernel, codec, dev, [b"abc"] + [b""] * 70 + [b" d", b"e" * 100, b"0" * 30 + b"5"] + [b""] * 70)
    expect(kernel, codec, dev, [b""] * 70)
    expect(kernel, codec, dev, [b""] * 70, lead=b"\x00" * 16)


@pytest.mark.parametrize("kernel", KERNELS)
def test_strings_that_are_not_examined(codec, dev, kernel):
    """A negative length, a length one past the next offset, descending
    offsets and an off + len that wraps 32 bits: INVALID, nothing read; the
    strings on both sides stay exact."""
    strings = [b"cookie", b"etag", b"42", b":path", b"007", b"host", b"HEAD", b"age", b"trailers", b"https", b"a b",
               b"0"]
    pool, off, ln, exam = B.not_examined(strings)
    want = [want_of(kernel, s) for s in exam]
    assert got_of(kernel, codec, dev, pool, off, ln) == want
    assert [i for i, s in enumerate(exam) if s is None] == [1, 3, 5, 7, 12, 13] and exam[8] == b"trailers"
    # without lengths only the offsets' order can refuse a string: string i is
    # pool[off[i]:off[i+1]], slot filling included (the closing offset is the
    # end of the slots, not the two strings 4 GiB up)
    n = len(strings)
    off = np.append(off[:n], np.uint32(16 * n))
    exam = [None if off[i] > off[i + 1] else pool[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    assert [i for i, s in enumerate(exam) if s is None] == [7] and int(off.max()) == 16 * n
    assert got_of(kernel, codec, dev, pool, off) == [want_of(kernel, s) for s in exam]


@pytest.mark.parametrize("length", B.EXIT_LENGTHS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_two_buffer_loop_exits(codec, dev, kernel, length):
    """One string of `length` bytes among 63 of 0-3 bytes: the wave's chunk
    count on both sides of 64 (one round, the loop's break) and of 128 (the
    second trip), the long string's head and tail chunk partly a neighbour's."""
    marks = {"check": (b"\x00", b"A"), "facts": (b"@", b"7")}[kernel]
    for strings in B.exit_batches(length, CLEAN[kernel], marks, b"@"):
        expect(kernel, codec, dev, strings)


def name_results(codec, dev, pool, off, ln=None):
    import torch
    t_len = None if ln is None else torch.from_numpy(ln).to(dev)
    tok, h = codec.name_tokens(torch.from_numpy(pool).to(dev), torch.from_numpy(off.view(np.int32)).to(dev),
                               len=t_len)
    return tok.cpu().numpy().tolist(), h.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_name_kernel_through_both_entry_points(codec, dev, n):
    """The sizes around a wave and a workgroup: the same names back to back
    through nghttp2_amd_hd_name_tokens_batch and placed among other bytes
    through nghttp2_amd_hd_name_tokens_len_batch."""
    names = sorted(W.TOKEN_NAMES)
    rng = np.random.Generator(np.random.PCG64(n))
    cands = names + [nm[:-1] + bytes([nm[-1] ^ 1]) for nm in names[:20]] + [b"", b"x" * 28, b"y" * 70]
    strings = [cands[int(rng.integers(0, len(cands)))] for _ in range(n)]
    want = tuple(list(x) for x in H.name_tokens(strings))
    assert name_results(codec, dev, *B.lay_out(strings)) == want
    pool, off, ln, placed = B.place([(b"-" + s + b"-control", int(rng.integers(1, 17)), 1, len(s)) for s in strings])
    assert placed == strings
    assert name_results(codec, dev, pool, off, ln) == want


def test_names_past_the_probe_and_the_register_chunks(codec, dev):
    """nghttp2_amd_hd_name_tokens_batch on a name of 33 bytes (past the
    probe's 32) and one of 70 (past the two chunks kept in registers) among
    short ones, at two alignments."""
    long33 = b"access-control-allow-origin" + b"-extra"
    long70 = b"content-security-policy-report-only" * 2
    assert (len(long33), len(long70)) == (33, 70)
    strings = [b"cookie", long33, b"etag", b"", long70, b":path", b"via", long33[:32], b"host"]
    want = tuple(list(x) for x in H.name_tokens(strings))
    assert want[0][1] == -1 and want[0][4] == -1 and want[0][0] >= 0
    assert name_results(codec, dev, *B.lay_out(strings)) == want
    assert name_results(codec, dev, *B.lay_out(strings, lead=b"x" * 7)) == want
