"""Deferred long codes in the 40-byte decoder's pair loop (csrc/hd_huff.hip
dd_run `pair_def`: a code past the 13-bit lookup is read from the
leading-ones table as the lane's next pair's first read).

Every case goes through decode_auto with a mean encoded length above 48
bytes, so the 40-byte instance runs, in batches of 64..512 strings of
100..400 encoded bytes (the one mixed task apart), and is compared with the
oracle on status, fstate, flags and every decoded byte.  The encoded pools
are packed on the host from symbol lists with the project's code table; a
family places its codes at every bit alignment 0..7:

* boundary: every code of 14..30 bits starting 0..29 bits before a 40-byte
  piece boundary (in the last 1..13 bits before it, exactly on it, across it,
  so that the next piece's warm-up must pick its end);
* runs: two, three and sixteen long codes back to back (a long code as both
  entries of a pair);
* last: a long code as the string's last code with 0..7 padding bits;
* cut: a long code cut by the string end (a proper prefix as the tail);
* eos: EOS (30 ones) at each of those places;
* two_sym: a long code directly after and directly before a two-symbol entry;
* lanes_all / lanes_one: every lane of a round, or exactly one, meets a long
  code in the same pair;
* slowest: 64 strings, a 1 KB string of long codes only among 63 short ones.

The same families run once through the bounds-checked build, which may record
no violation site.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from nghttp2_amd.tools.gen_tables import canonical_codes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "nghttp2_amd", "lib", "libnghttp2_amd_hd_bounds.so")
CODES = canonical_codes()[0]  # (code, len) per symbol 0..256
LONGS = [s for s, (c, L) in enumerate(CODES) if L > 13 and s != 256]
EOS = 256
PIECE = 320  # bits of a 40-byte piece
F5 = [ord(c) for c in "012aceiost"]  # 5-bit codes
F6 = [ord(c) for c in " %-./3456789=A_bdfghlmnpru"]  # 6-bit codes
assert all(CODES[s][1] == 5 for s in F5) and all(CODES[s][1] == 6 for s in F6)


def fill(nbits, salt=0):
    """Symbols of 5- and 6-bit codes taking exactly nbits (>= 20) bits."""
    r = nbits % 5
    assert nbits >= 6 * r and nbits >= 0, nbits
    out = [F6[(salt + i) % len(F6)] for i in range(r)]
    out += [F5[(salt + i) % len(F5)] for i in range((nbits - 6 * r) // 5)]
    # (the 6-bit codes spread through the 5-bit ones)
    return out[r:][:len(out) // 2] + out[:r] + out[r:][len(out) // 2:]


def pack(syms, cut=None):
    """The encoded string of the symbols, then `cut` = (symbol, t): the first
    t bits of its code, then ones up to the byte boundary."""
    v, nb = 0, 0
    for s in syms:
        c, L = CODES[s]
        v = (v << L) | c
        nb += L
    if cut is not None:
        c, L = CODES[cut[0]]
        v = (v << cut[1]) | (c >> (L - cut[1]))
        nb += cut[1]
    pad = (-nb) % 8
    v = (v << pad) | ((1 << pad) - 1)
    return v.to_bytes((nb + pad) // 8, "big")


def nbits(syms):
    return sum(CODES[s][1] for s in syms)


def pool_of(strs):
    off = np.zeros(len(strs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in strs])
    return np.frombuffer(b"".join(strs), dtype=np.uint8).copy(), off


def fam_boundary(codes=LONGS, tail=700):
    out = []
    for i, s in enumerate(codes):
        for j in range(30):  # the code starts j bits before the boundary
            m = 1 + (i + j) % 2
            out.append(pack(fill(PIECE * m - j, i + j) + [s] + fill(tail - j % 5, j)))
    return out


def fam_runs(codes=LONGS):
    out = []
    for i in range(len(codes)):
        for r in (2, 3, 16):
            for k in (range(8) if r == 2 else [i % 8]):
                run = [codes[(i + t) % len(codes)] for t in range(r)]
                out.append(pack(fill(280 + k + 8 * (i % 5), i) + run + fill(600, k)))
    return out


def fam_last(codes=LONGS):
    out = []
    for i, s in enumerate(codes):
        for p in range(8):
            P = 900 + (-(CODES[s][1] + p)) % 8 + 8 * (i % 40)
            out.append(pack(fill(P, i + p) + [s]))
    return out


def fam_cut(codes=LONGS):
    out = []
    for i, s in enumerate(codes):
        L = CODES[s][1]
        for t in sorted({1, 7, 8, 12, 13, 14, L // 2, L - 1}):
            P = 900 + (-t) % 8 + 8 * (i % 40)
            out.append(pack(fill(P, i + t), cut=(s, t)))
    return out


def fam_eos():
    out = fam_boundary([EOS]) + fam_last([EOS]) + fam_two_sym([EOS])
    for k in range(8):
        for r in (1, 2, 15):  # after long codes, back to back
            out.append(pack(fill(290 + k, k) + LONGS[k:k + r] + [EOS] + fill(600, k)))
        out.append(pack(fill(290 + k, k) + [EOS, EOS] + LONGS[:3] + fill(600, k)))
    for t in range(1, 30):  # EOS cut by the string end
        out.append(pack(fill(900 + (-t) % 8, t), cut=(EOS, t)))
    return out


def fam_two_sym(codes=LONGS):
    two = [ord("0"), ord("1")]  # 5 + 5 bits: one lookup entry
    out = []
    for i, s in enumerate(codes):
        for k in range(8):
            out.append(pack(fill(240 + k + 8 * (i % 11), i) + two + [s] + two + fill(640, k)))
    return out


def fam_lanes(one):
    """64 strings of 8 pieces, each piece exactly 320 bits with its long code
    at the same bit; `one`: only one piece of the batch has it."""
    out = []
    for k in range(8):
        s = LONGS[(7 * k) % len(LONGS)]
        L = CODES[s][1]
        with_long = fill(100 + k, k) + [s] + fill(PIECE - 100 - k - L, k)
        plain = fill(100 + k, k) + fill(PIECE - 100 - k, k)
        assert nbits(with_long) == PIECE == nbits(plain)
        for i in range(64):
            if one:
                out.append(pack(sum([with_long if (i, p) == (21, 3) else plain for p in range(8)], [])))
            else:
                out.append(pack(with_long * 8))
    return out


def fam_slowest():
    big, n = [], 0
    while n < 8 * 1024 - 30:
        s = LONGS[len(big) % len(LONGS)]
        big.append(s)
        n += CODES[s][1]
    strs = [pack(fill(800 + i, i)) for i in range(63)]
    strs.insert(17, pack(big))
    return strs


FAMILIES = {
    "boundary": fam_boundary, "runs": fam_runs, "last": fam_last, "cut": fam_cut,
    "eos": fam_eos, "two_sym": fam_two_sym, "lanes_all": lambda: fam_lanes(False),
    "lanes_one": lambda: fam_lanes(True), "slowest": fam_slowest,
}


def batches(name):
    """The family's strings as (pool, offsets) batches of 64..512 strings."""
    strs = FAMILIES[name]()
    if name != "slowest":
        assert all(100 <= len(x) <= 400 for x in strs), (name, min(map(len, strs)), max(map(len, strs)))
    step = 64 if name in ("slowest", "lanes_all", "lanes_one") else 512
    out = []
    for a in range(0, len(strs), step):
        part = strs[a:a + step]
        if len(part) < 64:  # (a last batch below 64 strings is filled up from the start)
            part = part + strs[:64 - len(part)]
        pool, off = pool_of(part)
        assert int(off[-1]) > 48 * len(part)  # decode_auto picks the 40-byte instance
        out.append((pool, off))
    return out


def run_family(codec, dev, name):
    from tests.test_parity_gpu import auto_decode_check
    fails = oks = 0
    for b, (enc, eoff) in enumerate(batches(name)):
        st, _ = auto_decode_check(codec, dev, enc, eoff, "%s batch %d" % (name, b), nthreads=8)
        fails += int((st < 0).sum())
        oks += int((st >= 0).sum())
    return oks, fails


def test_families_shape():
    """(CPU) the packer against the oracle's encoder, and the batch rules."""
    from oracle import oracle as O
    syms = fill(333, 3) + LONGS[:5] + fill(77, 1)
    assert pack(syms) == O.encode(bytes(syms))[1]
    assert nbits(fill(23)) == 23 and nbits(fill(PIECE)) == PIECE
    for name in FAMILIES:
        for pool, off in batches(name):
            assert 64 <= len(off) - 1 <= 512


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_deferred_long_family_vs_oracle(codec, dev, name):
    oks, fails = run_family(codec, dev, name)
    if name == "eos":
        assert fails > 0
    elif name != "cut":
        assert fails == 0 and oks > 0


CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import torch
import nghttp2_amd
from tests import test_decode_deferred_long_gpu as D

L = nghttp2_amd.lib()
L.nghttp2_amd_hd__bounds_check.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
s = ctypes.c_uint32(0)
assert L.nghttp2_amd_hd__bounds_check(ctypes.byref(s)) == 0, "not the bounds-checked build"
dev = torch.device("cuda:0")
codec = nghttp2_amd.HuffmanBatchCodec(dev)
for name in sorted(D.FAMILIES):
    D.run_family(codec, dev, name)
    s = ctypes.c_uint32(0)
    assert L.nghttp2_amd_hd__bounds_check(ctypes.byref(s)) == 0
    assert s.value == 0, "%%s: out-of-bounds index at site 0x%%x" %% (name, s.value)
    print("ok", name, flush=True)
print("BOUNDS-OK")
""" % REPO


@pytest.mark.gpu
def test_deferred_long_families_bounds_checked_build():
    env = dict(os.environ, NGHTTP2_AMD_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-u", "-c", CHILD], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and "BOUNDS-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
