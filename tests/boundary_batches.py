"""Boundary-grid batches for the Huffman kernels' exact edges (numpy and the
code table only: no GPU, no torch).

The parity suite's volume tests meet the kernels' edges by chance.  These
generators place them: strings are built as bit strings from the canonical
code table (`CODES`, tests/test_long_codes.py) and cut into bytes, so a
codeword starts a known number of bits before a piece boundary, a string ends
a known number of bits behind one, a task's items sum to an exact byte count,
a pack round carries an exact number of code bits.  Any bit count >= 20 is a
sum of 5- and 6-bit codes, which gives every position.

Decode families return (enc u8, eoff u32[n+1]); encode families (pool, off).
Each has a `*_cases()` companion: one tuple per string (or task) saying what it
was built to hit.  tests/test_boundary_batches.py proves, from the oracle's
tables and the constants in csrc/hd_huff.hip, that the grids hit what they
claim; tests/test_boundary_gpu.py runs them through every entry point against
the oracle.  The arrays are shared and read-only.
"""
import functools
import os
import re

import numpy as np

from tests.test_long_codes import CODES

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nghttp2_amd", "csrc",
                   "hd_huff.hip")

# The kernel constants the grids depend on (csrc/hd_huff.hip; kernel_defaults()
# reads the source, and the CPU test holds the two equal: a retune fails there
# instead of quietly moving the grids off the edges).
DD_IP64 = 96         # item bytes of the header instance (DecHeader)
DD_IP40 = 40         # piece bytes of the long-value instance (DecLong)
DD_OV = 20           # warm-up bytes of a later item
DD_BI64 = 2304       # the header instance's input bytes per round
DD_TS64 = 64         # strings per task unit, header instance
DD_TS40 = 32         # ... long-value instance (two units per task)
DD_LB64 = 13         # lookup bits: a fast pair needs 2 LB - 4 bits before the
DD_LB40 = 13         # stop and 2 LB before the string end
PIECE_BYTES = 64     # piece bytes of the slot decoder (k_decode)
SUB_OV = 24          # ... and its warm-up bytes
EC_ROUND_BYTES = 1024   # k_encode: raw bytes per round (64 chunks of 16)
EC_STORE4_WORDS = 256   # ... an interior round of <= 256 words: four stores
EC_LONG_PAIR_BITS = 32  # ... a pair of codes of >= 32 bits: the round goes bytewise
TASK_STR = 64        # strings per decode task


def kernel_defaults():
    """The same constants as csrc/hd_huff.hip defines them."""
    txt = open(HIP).read()

    def define(name):
        m = re.search(r"^#define %s (\d+)u?\b" % name, txt, re.M)
        assert m, "hd_huff.hip no longer defines " + name
        return int(m.group(1))

    def expr(pattern, what):
        m = re.search(pattern, txt)
        assert m, "hd_huff.hip: %s not found" % what
        return int(m.group(1))

    out = {k: define(k) for k in ("DD_IP64", "DD_IP40", "DD_OV", "DD_BI64", "DD_TS64", "DD_TS40",
                                  "DD_LB64", "DD_LB40", "PIECE_BYTES", "SUB_OV", "TASK_STR")}
    chunks = expr(r"cb < c_stop; cb \+= (\d+)u\)", "k_encode's round loop")
    shift = expr(r"const uint32_t base = cb << (\d+);", "k_encode's chunk size")
    out["EC_ROUND_BYTES"] = chunks << shift
    out["EC_STORE4_WORDS"] = expr(r"nst - 1u < (\d+)u", "k_encode's four-store threshold")
    out["EC_LONG_PAIR_BITS"] = expr(r"plx > \(FR \? 64u : (\d+)u\)", "k_encode's long-pair test") + 1
    return out


LEN = np.array([L for _, L in CODES[:256]], dtype=np.int64)
CODE = np.array([c for c, _ in CODES[:256]], dtype=np.uint64)
LENGTHS = sorted(set(LEN.tolist()))  # the 21 distinct code lengths
BY_LEN = {L: np.nonzero(LEN == L)[0] for L in LENGTHS}
SHORT = np.nonzero(LEN <= 8)[0]

# bit counts that some symbol sequence has (every count >= 20 does: 5s and 6s)
FEAS = np.zeros(160, dtype=bool)
FEAS[0] = True
for _b in range(1, len(FEAS)):
    FEAS[_b] = any(_b >= L and FEAS[_b - L] for L in LENGTHS)
assert FEAS[20:].all()


def feasible(nbits):
    return nbits >= len(FEAS) or bool(FEAS[nbits])


def sym_bits(syms):
    """The code bits of a symbol sequence, one bit per element."""
    syms = np.asarray(syms, dtype=np.int64)
    if syms.size == 0:
        return np.zeros(0, dtype=np.uint8)
    lens = LEN[syms]
    total = int(lens.sum())
    pos = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    sh = (np.repeat(lens, lens) - 1 - pos).astype(np.uint64)
    return ((np.repeat(CODE[syms], lens) >> sh) & np.uint64(1)).astype(np.uint8)


def ones(k):
    return np.ones(k, dtype=np.uint8)


def cut(*bits):
    """Bit arrays, joined, as bytes (a whole number of them)."""
    b = np.concatenate(bits)
    assert b.size % 8 == 0, b.size
    return np.packbits(b).tobytes()


def padded(bits):
    """A bit string with its EOS-prefix padding (ones to the byte)."""
    return cut(bits, ones(-bits.size % 8))


def fives_sixes(nbits, rng):
    """Symbols of 5- and 6-bit codes with exactly nbits code bits."""
    choices = list(range(nbits % 5, nbits // 6 + 1, 5))
    assert choices, "%d bits are no sum of 5s and 6s" % nbits
    n6 = choices[int(rng.integers(len(choices)))]
    n5 = (nbits - 6 * n6) // 5
    lens = np.array([5] * n5 + [6] * n6)
    rng.shuffle(lens)
    return np.where(lens == 5, rng.choice(BY_LEN[5], size=lens.size),
                    rng.choice(BY_LEN[6], size=lens.size))


def any_codes(nbits, rng):
    """Symbols of every code length with exactly nbits code bits."""
    assert feasible(nbits), nbits
    syms, rem = [], nbits
    while rem > 100:
        k = max(1, (rem - 100) // 30)
        s = np.where(rng.random(k) < 0.3, rng.integers(0, 256, size=k), rng.choice(SHORT, size=k))
        syms.append(s)
        rem -= int(LEN[s].sum())
    while rem > 0:
        ls = [L for L in LENGTHS if L <= rem and FEAS[rem - L]]
        L = ls[int(rng.integers(len(ls)))]
        syms.append(np.array([rng.choice(BY_LEN[L])]))
        rem -= L
    return np.concatenate(syms) if syms else np.zeros(0, dtype=np.int64)


def valid_string(E, rng):
    """A valid encoding of exactly E bytes (random symbols, random padding)."""
    if E == 0:
        return b""
    ps = [p for p in range(8) if feasible(8 * E - p)]
    p = ps[int(rng.integers(len(ps)))]
    return padded(sym_bits(any_codes(8 * E - p, rng)))


def batch(strs):
    off = np.zeros(len(strs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in strs])
    pool = np.frombuffer(b"".join(strs), dtype=np.uint8).copy()
    pool.setflags(write=False)  # shared between tests (the offsets stay writable: torch takes them as they are)
    return pool, off


# ---------------------------------------------------------------------------
# decode families
# ---------------------------------------------------------------------------
STRADDLE_BOUNDS = (DD_IP40, PIECE_BYTES, DD_IP64)
# one symbol per distinct code length, and all three 30-bit symbols
STRADDLE_SYMS = tuple(int(BY_LEN[L][0]) for L in LENGTHS if L != 30) + tuple(int(s) for s in BY_LEN[30])


def straddle_plan(bounds=STRADDLE_BOUNDS):
    """(B, k, sym, s, ending): the codeword of sym starts s bits before byte
    B k; ending "more": 64 more code bits follow, "pad": only the padding."""
    return [(B, k, sym, s, ending) for B in bounds for k in (1, 2) for sym in STRADDLE_SYMS
            for s in range(1, int(LEN[sym])) for ending in ("more", "pad")]


@functools.lru_cache(maxsize=None)
def _straddle():
    rng = np.random.default_rng(0x57AD)
    cases = straddle_plan()
    strs = []
    for B, k, sym, s, ending in cases:
        bits = [sym_bits(fives_sixes(8 * B * k - s, rng)), sym_bits([sym])]
        if ending == "more":
            bits.append(sym_bits(fives_sixes(64, rng)))
        strs.append(padded(np.concatenate(bits)))
    return batch(strs) + (cases,)


def straddle():
    """Codewords across a 40-, 64- or 96-byte boundary at every bit position."""
    return _straddle()[:2]


def straddle_cases():
    return _straddle()[2]


def ends_lengths(bounds=STRADDLE_BOUNDS, budget=DD_BI64):
    E = set(range(1, 201))
    E |= {k * B + d for B in bounds for k in range(1, 7) for d in (-1, 0, 1)}
    E |= {budget - 1, budget, budget + 1}
    return sorted(E)


def ends_versions(p):
    """The versions of an (E, p) string.  "first0" / "last0" clear the first /
    last pad bit ("last0" from p = 2: with one pad bit they are one string);
    "ff" appends a whole 0xFF byte (padding longer than 7 bits)."""
    return ["valid"] + (["first0"] if p >= 1 else []) + (["last0"] if p >= 2 else []) + ["ff"]


def ends_accepts(p, version):
    """Whether the reference accepts the version.  Clearing the first of 6 or
    7 pad bits leaves 011111, a complete 6-bit code: one more symbol and a
    valid string.  Every other altered padding is refused (-523)."""
    return version == "valid" or (version == "first0" and p >= 6)


def ends_plan(bounds=STRADDLE_BOUNDS, budget=DD_BI64):
    """(E, p, version) for every E of ends_lengths and every padding p in
    0..7 for which some symbol sequence has 8 E - p bits."""
    return [(E, p, v) for E in ends_lengths(bounds, budget) for p in range(8)
            if 8 * E - p > 0 and feasible(8 * E - p) for v in ends_versions(p)]


@functools.lru_cache(maxsize=None)
def _ends():
    rng = np.random.default_rng(0xE2D5)
    cases = ends_plan()
    strs, body, key = [], None, None
    for E, p, v in cases:
        if key != (E, p):
            key, body = (E, p), sym_bits(any_codes(8 * E - p, rng))
        pad = ones(p)
        if v == "first0":
            pad[0] = 0
        elif v == "last0":
            pad[-1] = 0
        strs.append(cut(body, pad, ones(8 if v == "ff" else 0)))
    return batch(strs) + (cases,)


def ends():
    """Exact encoded lengths E with exact padding p, valid and invalid."""
    return _ends()[:2]


def ends_cases():
    return _ends()[2]


def items_of(lengths, ip):
    """Items of an item-decoder task: max(1, ceil(E / IP)) per string."""
    return int(sum(max(1, -(-int(e) // ip)) for e in lengths))


def tasks_plan(last=33):
    """(name, lengths, items, bytes): the task's strings' encoded lengths, and
    the item count (96-byte items) and input byte sum it is meant to have."""
    plan = []
    for E, items in ((35, 64), (36, 64), (37, 64), (47, 64), (48, 64), (49, 64), (95, 64),
                     (96, 64), (97, 128)):
        plan.append(("uniform %d" % E, [E] * 64, items, 64 * E))
    plan.append(("96 + 63 x 35", [96] + [35] * 63, 64, 2301))
    plan.append(("96 + 63 x 36", [96] + [36] * 63, 64, 2364))
    plan.append(("63 empty + 2400", [0] * 63 + [2400], 63 + 25, 2400))
    plan.append(("2400 + 63 empty", [2400] + [0] * 63, 63 + 25, 2400))
    plan.append(("64 x 1", [1] * 64, 64, 64))
    for lane in (0, 31, 32, 63):
        lens = [36] * 64
        lens[lane] = 97
        plan.append(("97 at lane %d" % lane, lens, 65, 63 * 36 + 97))
    plan.append(("final %d" % last, [36] * last, last, 36 * last))
    return plan


@functools.lru_cache(maxsize=None)
def _tasks(last):
    rng = np.random.default_rng(0x7A5C + last)
    strs, cases = [], []
    for name, lens, items, nbytes in tasks_plan(last):
        cases.append((name, len(strs), len(lens), items, nbytes))
        strs += [valid_string(E, rng) for E in lens]
    for i in range(6, len(strs), 7):  # every 7th string: random bytes
        strs[i] = bytes(rng.integers(0, 256, size=len(strs[i]), dtype=np.uint8))
    return batch(strs) + (cases,)


def tasks(last=33):
    """Whole tasks of 64 strings with exact item counts and byte sums, the
    final one of `last` strings."""
    return _tasks(last)[:2]


def tasks_cases(last=33):
    """(name, first string, strings, items, bytes) per task."""
    return _tasks(last)[2]


@functools.lru_cache(maxsize=None)
def _front(j):
    rng = np.random.default_rng(0x5F + j)
    return batch([valid_string(3, rng) for _ in range(j)])


def shifted(b, j):
    """The batch with j three-byte valid strings in front."""
    enc, eoff = b
    fe, fo = _front(j)
    return (np.concatenate([fe, enc]),
            np.concatenate([fo[:-1], eoff.astype(np.int64) + int(fo[-1])]).astype(np.uint32))


# ---------------------------------------------------------------------------
# encode families
# ---------------------------------------------------------------------------
RW_DELTAS = tuple(range(-70, 71))
RW_STRING = 4096


def _rw_string(start, deltas, rng):
    """4096 bytes of 8-bit-code symbols at pool byte `start`, with 7- and
    10-bit symbols swapped in so that the aligned 1024-byte pool windows inside
    it carry 8192 + delta code bits (the first len(deltas) whole windows), and
    a correction outside those windows that makes the string's bits a multiple
    of 8 (no padding, so the deltas are exact)."""
    s = rng.choice(BY_LEN[8], size=RW_STRING)
    w0 = -(-start // EC_ROUND_BYTES)  # first whole window
    used = np.zeros(RW_STRING, dtype=bool)
    for j, d in enumerate(deltas):
        lo = (w0 + j) * EC_ROUND_BYTES - start
        assert 0 <= lo and lo + EC_ROUND_BYTES <= RW_STRING
        n10 = (d + 1) // 2 if d > 0 else 0
        n7 = (2 * n10 - d) if d > 0 else -d
        at = lo + rng.choice(EC_ROUND_BYTES, size=n10 + n7, replace=False)
        s[at[:n10]] = rng.choice(BY_LEN[10], size=n10)
        s[at[n10:]] = rng.choice(BY_LEN[7], size=n7)
        used[lo:lo + EC_ROUND_BYTES] = True
    fix = int(sum(deltas)) % 8  # that many bits too many for a whole byte
    free = np.nonzero(~used)[0]
    assert free.size >= fix
    s[free[:fix]] = rng.choice(BY_LEN[7], size=fix)
    assert int(LEN[s].sum()) % 8 == 0
    return s.astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _round_words():
    rng = np.random.default_rng(0x40AD)
    strs = []
    ds = list(RW_DELTAS)
    for k in range(0, len(ds), 3):  # pool alignment 0: windows 0..2 of each string
        strs.append(_rw_string(len(b"".join(strs)), ds[k:k + 3], rng))
    strs.append(b"01234")          # ... and again behind a 5-byte string
    for k in range(0, len(ds), 3):
        strs.append(_rw_string(len(b"".join(strs)), ds[k:k + 3], rng))
    return batch(strs)


def round_words():
    """Pack rounds of 8192 + delta code bits, delta in -70..70: both sides of
    the 256-word four-store threshold at every output phase."""
    return _round_words()


LP_PAIRS = ((25, 5), (5, 25), (26, 5), (5, 26), (27, 5), (5, 27), (28, 5), (5, 28), (30, 5), (5, 30),
            (30, 30))  # code lengths summing to 30, 31, 32, 33, 35 and 60
LP_CHUNKS = (0, 1, 63)
LP_SHORT = 20


def _lp_string(nbytes, at, pair, rng, fix_at):
    """nbytes of 5-bit symbols, the pair of code lengths at bytes at, at + 1,
    and 6-bit symbols from byte fix_at on making the bits a multiple of 8."""
    s = rng.choice(BY_LEN[5], size=nbytes)
    s[at] = rng.choice(BY_LEN[pair[0]])
    s[at + 1] = rng.choice(BY_LEN[pair[1]])
    fix = -int(LEN[s].sum()) % 8
    free = [i for i in range(fix_at, nbytes) if i not in (at, at + 1)][:fix]
    assert len(free) == fix
    s[free] = rng.choice(BY_LEN[6], size=fix)
    assert int(LEN[s].sum()) % 8 == 0
    return s.astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _long_pairs():
    rng = np.random.default_rng(0x10A9)
    strs, cases = [], []
    for pair in LP_PAIRS:
        for chunk in LP_CHUNKS:
            for slot in range(8):
                at = 16 * chunk + 2 * slot
                cases.append((len(strs), at, pair, chunk, slot))
                strs.append(_lp_string(EC_ROUND_BYTES, at, pair, rng, 16 * 30))
    for pair in LP_PAIRS:
        for at in range(0, LP_SHORT, 2):
            cases.append((len(strs), at, pair, None, None))
            strs.append(_lp_string(LP_SHORT, at, pair, rng, 0))
    return batch(strs) + (cases,)


def long_pairs():
    """One pair of adjacent codes of 30..60 bits in a round of 5-bit symbols,
    at every pair slot of the round's first, second and last chunk, and in
    20-byte strings (waves with edge rounds only)."""
    return _long_pairs()[:2]


def long_pairs_cases():
    """(string, byte of the pair's first code, (len, len), chunk, slot);
    chunk and slot are None for the 20-byte strings."""
    return _long_pairs()[2]


FILL_STRINGS = 256


@functools.lru_cache(maxsize=None)
def _fill():
    rng = np.random.default_rng(0xF111)
    return batch([bytes(rng.integers(0x20, 0x7F, size=i % 8, dtype=np.uint8))
                  for i in range(FILL_STRINGS)])


def with_fill(b):
    """The batch behind 256 short strings (a whole tile, a multiple of 16
    bytes: the batch's waves and rounds keep their alignment), so it takes the
    count and pack launches, not the one-tile launch."""
    pool, off = b
    fp, fo = _fill()
    assert int(fo[-1]) % 16 == 0
    return (np.concatenate([fp, pool]),
            np.concatenate([fo[:-1], off.astype(np.int64) + int(fo[-1])]).astype(np.uint32))


def pack_rounds(pool, off):
    """k_encode's waves and rounds over a batch, restated: one dict per round
    with its code bits, stored words `nst`, store path ("store4": an interior
    round of <= 256 words; "loop": a longer interior round; "edge": a round
    with bytes of a neighbouring wave's words) and the bit sums of its byte
    pairs (`pairs`, pair j = round bytes 2 j, 2 j + 1; `bytewise` when one
    reaches 32 bits)."""
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    used = int(off[-1])
    raw = np.zeros(used + (-used) % 16 + 16, dtype=np.uint8)  # the padded pool
    raw[:used] = np.asarray(pool)[:used]
    L = LEN[raw]
    P = np.concatenate([[0], np.cumsum(L)])
    bits = P[off[1:]] - P[off[:-1]]
    elen = (bits + 7) // 8
    eo = np.concatenate([[0], np.cumsum(elen)])
    X = np.zeros(len(raw), dtype=np.int64)  # pad bits, at a string's last byte
    ne = np.nonzero(off[1:] > off[:-1])[0]
    X[off[1:][ne] - 1] = (8 * elen - bits)[ne]
    idx = np.arange(len(raw))
    for t0 in range(0, n, 64):
        nstr = min(64, n - t0)
        A, Z = int(off[t0]), int(off[t0 + nstr])
        OA, OZ = int(eo[t0]), int(eo[t0 + nstr])
        c0, c_end = A >> 4, (Z + 15) >> 4
        G0, x = 8 * OA, 0
        for cb in range(c0, c_end, 64):
            first, last = cb == c0, cb + 64 >= c_end
            lo, hi = cb << 4, min((cb + 64) << 4, c_end << 4)
            lens = L[lo:hi] + np.where((idx[lo:hi] >= A) & (idx[lo:hi] < Z), X[lo:hi], 0)
            RA = int(L[lo:A].sum()) if first else 0
            WB = (G0 + x) >> 5
            xe = 8 * (OZ - OA) if last else x + int(lens.sum()) - RA
            nw = ((G0 + xe + 31) >> 5) - WB
            nst = nw if last else ((G0 + xe) >> 5) - WB
            ilo = (OA + 3) // 4 - min(WB, (OA + 3) // 4)
            ihi = max(OZ // 4 - WB, 0)
            interior = ilo == 0 and ihi >= nst
            pairs = lens.reshape(-1, 2).sum(axis=1)
            yield dict(t0=t0, round=(cb - c0) // 64, base=lo, first=first, last=last, bits=xe - x,
                       nst=nst, pairs=pairs, bytewise=bool(pairs.max() >= EC_LONG_PAIR_BITS),
                       store=("store4" if 1 <= nst <= EC_STORE4_WORDS else "loop") if interior
                       else "edge")
            x = xe


# ---------------------------------------------------------------------------
# offsets: a pool whose first offset is not 0
# ---------------------------------------------------------------------------
OFFSET_A0 = (1, 15, 16, 17, 4099)
OFFSET_N = (0, 1, 64, 65, 257, 600)
OFFSET_FILL = ("ff", "random")
NAMES = (b":status", b"content-type", b"te", b"cookie", b"x-unknown-name", b":statusx")


def place(pool, off, a0, fill):
    """The batch's bytes from byte a0 of a buffer of exactly
    align_up(a0 + bytes, 16) + 16 bytes, every other byte `fill` (0xFF, or
    random); returns (buffer, offsets from a0)."""
    off = np.asarray(off).astype(np.int64)
    total = int(off[-1] - off[0])
    size = a0 + total + (-(a0 + total)) % 16 + 16
    if fill == "ff":
        buf = np.full(size, 0xFF, dtype=np.uint8)
    else:
        buf = np.random.default_rng(a0 + total).integers(0, 256, size=size, dtype=np.uint8)
    buf[a0:a0 + total] = np.asarray(pool)[int(off[0]):int(off[-1])]
    return buf, (off - off[0] + a0).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def offset_pool(a0, n, fill):
    """n strings -- random bytes of 0..120, one of 3000 bytes (string n // 2),
    empty strings, a few header names -- placed from byte a0 of an exactly
    sized buffer filled with `fill` around them.  Returns (buffer, offsets,
    rebased pool, rebased offsets): the last two are what the oracle sees."""
    rng = np.random.default_rng(1000 * n + a0)
    strs = []
    for i in range(n):
        if i == n // 2:
            strs.append(bytes(rng.integers(0, 256, size=3000, dtype=np.uint8)))
        elif i % 5 == 3:
            strs.append(b"")
        elif i % 11 == 1:
            strs.append(NAMES[(i // 11) % len(NAMES)])
        else:
            strs.append(bytes(rng.integers(0, 256, size=int(rng.integers(0, 121)), dtype=np.uint8)))
    rpool, roff = batch(strs)
    buf, off = place(rpool, roff, a0, fill)
    return buf, off, rpool, roff
