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
the oracle, tests/test_literal_boundary_gpu.py the string-literal families
(lit_*).  The arrays are shared and read-only.
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
EC_LONG_PAIR_BITS_F = 65  # k_encode<FR>: a pair (code, extras, code) of >= 65 bits: bytewise
EC_M = 16               # image margin (words) before the round's first word
EC_RW = 1072            # image words of the plain instance
EC_RW_F_MARGIN = 112    # ... and the words k_encode<FR> adds (prefixes and pads)
EC_RAW_MASK_BYTES = 32  # k_encode<FR>: round bytes per word of the raw-string mask
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
    out["EC_LONG_PAIR_BITS_F"] = expr(r"plx > \(FR \? (\d+)u : \d+u\)", "k_encode<FR>'s long-pair test") + 1
    out["EC_M"] = expr(r"#define EC_M (\d+)u", "k_encode's image margin")
    m = re.search(r"#define EC_RW \(EC_M \+ (\d+)u \+ (\d+)u\)", txt)
    assert m, "hd_huff.hip: EC_RW not found"
    out["EC_RW"] = out["EC_M"] + int(m.group(1)) + int(m.group(2))
    out["EC_RW_F_MARGIN"] = expr(r"#define EC_RW_F \(EC_RW \+ (\d+)u\)", "k_encode<FR>'s image margin")
    out["EC_RAW_MASK_BYTES"] = expr(r"const uint32_t w0 = base \+ (\d+)u \* w;", "k_encode<FR>'s raw mask word")
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


# ---------------------------------------------------------------------------
# string literals: k_encode<FR> (nghttp2_amd_hd_emit_strings_batch)
# ---------------------------------------------------------------------------
PREFIX_EDGES = (127, 127 + 128, 127 + 128 ** 2, 127 + 128 ** 3, 127 + 128 ** 4)


def prefix7_len(P):
    """Bytes of the 7-bit-prefix integer P (scalar or array)."""
    P = np.asarray(P, dtype=np.int64)
    return 1 + sum((P >= e).astype(np.int64) for e in PREFIX_EDGES)


def literal_strings(pool, off):
    """Per string of a batch, as emit_string decides it: Huffman bytes E, raw
    bytes R, H = E < R, payload P = min(E, R), prefix bytes PL, EOS pad bits
    (Huffman literals only) and the literal offsets lo (n + 1)."""
    off = np.asarray(off).astype(np.int64)
    used = int(off[-1])
    raw = np.zeros(used + (-used) % 16 + 16, dtype=np.uint8)  # the padded pool
    raw[:used] = np.asarray(pool)[:used]
    Pc = np.concatenate([[0], np.cumsum(LEN[raw])])
    bits = Pc[off[1:]] - Pc[off[:-1]]
    E, R = (bits + 7) // 8, np.diff(off)
    H = E < R
    P = np.where(H, E, R)
    PL = prefix7_len(P)
    lo = np.concatenate([[0], np.cumsum(PL + P)])
    return dict(raw=raw, off=off, bits=bits, E=E, R=R, H=H, P=P, PL=PL, lo=lo,
                pad=np.where(H, 8 * E - bits, 0))


def literal_rounds(pool, off):
    """k_encode<FR>'s waves and rounds over a batch, restated like pack_rounds:
    one dict per round.  Per wave: A, Z, XS (the prefix bits of the strings
    that start at A: an initial offset, not extras) and at_a (how many).  Per
    round, over the bytes of its chunks below the wave's last chunk: `bits`
    (8 for a byte of a raw string of the wave, the code length otherwise, 0
    before A in the first chunk), `extras` (the pad of a Huffman string ending
    at the byte plus 8 PL of every string starting right after it), `raw` (the
    mask), `L0` = l0 + x0 and `pairs` = l0 + x0 + l1 for pair j = bytes 2 j,
    2 j + 1 (`bytewise` when one reaches EC_LONG_PAIR_BITS_F), `nw` (words of
    the round from its first word) and `top` (the highest image word a code is
    OR'ed into; the kernel checks top < EC_RW + EC_RW_F_MARGIN, site 0x101)."""
    S = literal_strings(pool, off)
    raw, off, lo = S["raw"], S["off"], S["lo"]
    n = len(off) - 1
    L = LEN[raw]
    wave_a = off[:-1][(np.arange(n) // 64) * 64] if n else np.zeros(0, np.int64)  # A of each string's wave
    ne = S["R"] > 0
    rawb = np.zeros(len(raw), dtype=bool)
    X = np.zeros(len(raw), dtype=np.int64)
    for i in np.nonzero(ne & ~S["H"])[0]:
        rawb[off[i]:off[i + 1]] = True
    np.add.at(X, off[1:][ne & S["H"]] - 1, S["pad"][ne & S["H"]])
    behind = off[:-1] > wave_a  # (the others: XS of their wave)
    np.add.at(X, off[:-1][behind] - 1, 8 * S["PL"][behind])
    idx = np.arange(len(raw))
    for t0 in range(0, n, 64):
        nstr = min(64, n - t0)
        A, Z = int(off[t0]), int(off[t0 + nstr])
        OA, OZ = int(lo[t0]), int(lo[t0 + nstr])
        at_a = off[t0:t0 + nstr] == A
        XS = int(8 * S["PL"][t0:t0 + nstr][at_a].sum())
        c0, c_end = A >> 4, (Z + 15) >> 4
        c_stop = c0 + 1 if c_end == c0 else c_end
        G0, x = 8 * OA, 0
        for cb in range(c0, c_stop, 64):
            first, last = cb == c0, cb + 64 >= c_stop
            b0, b1 = cb << 4, min((cb + 64) << 4, c_end << 4)
            inw = (idx[b0:b1] >= A) & (idx[b0:b1] < Z)
            rmask = inw & rawb[b0:b1]
            bits = np.where(rmask, 8, L[b0:b1])
            if first:
                bits = np.where(idx[b0:b1] < A, 0, bits)
            ext = np.where(inw, X[b0:b1], 0)
            X0 = XS if first else 0
            WB = (G0 + x) >> 5
            tot = bits + ext
            xe = 8 * (OZ - OA) if last else x + int(tot.sum()) + X0
            nw = ((G0 + xe + 31) >> 5) - WB
            starts = ((G0 + x) & 31) + X0 + np.cumsum(tot) - tot
            L0 = bits[0::2] + ext[0::2]
            pairs = L0 + bits[1::2]
            yield dict(t0=t0, round=(cb - c0) // 64, base=b0, first=first, last=last, A=A, Z=Z,
                       XS=XS, at_a=int(at_a.sum()), whole_empty=c_end == c0, bits=bits, extras=ext,
                       raw=rmask, L0=L0, pairs=pairs,
                       bytewise=bool(pairs.size and pairs.max() >= EC_LONG_PAIR_BITS_F), nw=nw,
                       top=EC_M + (int(starts.max()) >> 5) + 2 if starts.size else EC_M)
            x = xe


# sums of exactly k code lengths, k <= 3 (one combination each, for the tails)
_SUMS = [{0: ()}]
for _k in range(3):
    _SUMS.append({})
    for _s, _c in _SUMS[_k].items():
        for _L in LENGTHS:
            _SUMS[_k + 1].setdefault(_s + _L, _c + (_L,))
assert all(b in _SUMS[3] for b in range(15, 61))


def exact_feasible(R, B):
    """Whether R symbols can have exactly B code bits (as syms_exact builds)."""
    return B in _SUMS[R] if R <= 3 else 5 * R <= B <= 20 * R


def syms_exact(R, B, rng):
    """R symbols of mixed code lengths with exactly B code bits."""
    assert exact_feasible(R, B), (R, B)
    lens, rem = [], B
    for r in range(R, 3, -1):  # r symbols left: leave 5 (r-1) .. 20 (r-1) bits
        ok = [L for L in LENGTHS if 5 * (r - 1) <= rem - L <= 20 * (r - 1)]
        L = ok[int(rng.integers(len(ok)))]
        lens.append(L)
        rem -= L
    tail = list(_SUMS[min(R, 3)][rem])
    rng.shuffle(tail)
    lens += tail
    assert sum(lens) == B and len(lens) == R
    return np.array([rng.choice(BY_LEN[L]) for L in lens], dtype=np.int64)


def to_bytes(syms):
    return np.asarray(syms).astype(np.uint8).tobytes()


def fives(k, rng):
    return to_bytes(rng.choice(BY_LEN[5], size=k))


def raw_bytes(k, rng):
    """k bytes >= 0x80 (codes of >= 19 bits: the literal stays raw)."""
    return bytes(rng.integers(0x80, 0x100, size=k, dtype=np.uint8))


def huff_payload(E, rng):
    """A string of 5- and 6-bit-code symbols whose Huffman form has exactly E
    bytes (fewer than its raw bytes), E >= 3."""
    p = int(rng.integers(0, 8))
    s = to_bytes(fives_sixes(8 * E - p, rng))
    assert E < len(s)
    return s


def coded(n, E, rng):
    """n bytes of 5- and 6-bit-code symbols whose Huffman form has E bytes."""
    p = [p for p in range(8) if 5 * n <= 8 * E - p <= 6 * n]
    assert p and E < n, (n, E)
    six = rng.permutation(n) < 8 * E - p[0] - 5 * n
    return to_bytes(np.where(six, rng.choice(BY_LEN[6], size=n), rng.choice(BY_LEN[5], size=n)))


def lead_strings(k, rng):
    """Strings whose literals take k = 0..3 output bytes: none, the empty
    string (00), one raw byte, two raw bytes."""
    return [[], [b""], [raw_bytes(1, rng)], [raw_bytes(2, rng)]][k]


class _Builder:
    """Strings in order, with the pool byte and index of the next one."""

    def __init__(self, rng):
        self.rng, self.strs, self.starts, self.pos, self.out = rng, [], [], 0, 0

    def add(self, s):
        self.starts.append(self.pos)
        self.strs.append(s)
        self.pos += len(s)
        P = min(len(s), (int(LEN[np.frombuffer(s, np.uint8)].sum()) + 7) // 8)
        self.out += int(prefix7_len(P)) + P  # (its literal)
        return len(self.strs) - 1

    def new_wave(self, at16=0):
        """Fillers up to the next wave (a multiple of 64 strings), the last
        one sized so the wave starts at pool byte = at16 (mod 16)."""
        m = (-len(self.strs)) % 64 or 64
        for _ in range(m - 1):
            self.add(fives(3, self.rng))
        self.add(fives(3 + (at16 - (self.pos + 3)) % 16, self.rng))
        assert len(self.strs) % 64 == 0 and self.pos % 16 == at16

    def wave_a(self, i):
        """Pool byte A of the wave of string i (i: the next string at most)."""
        w = i - i % 64
        return self.pos if w == len(self.strs) else self.starts[w]


TIE_R = (1, 2, 3, 15, 16, 17, 127, 128, 255, 1023, 1024, 1025)


def ties_plan():
    """(R, B) for every planned tie case, feasible or not."""
    return [(R, B) for R in TIE_R
            for B in (8 * (R - 1) - 1, 8 * (R - 1), 8 * (R - 1) + 1, 8 * R - 1, 8 * R, 8 * R + 1)]


@functools.lru_cache(maxsize=None)
def _lit_ties():
    rng = np.random.default_rng(0x71E5)
    strs, cases = [b""], [(0, 0, False)]
    for R, B in ties_plan():
        if B >= 0 and exact_feasible(R, B):
            cases.append((R, B, B <= 8 * (R - 1)))
            strs.append(to_bytes(syms_exact(R, B, rng)))
    return batch(strs) + (cases,)


def lit_ties():
    """The H/raw decision: R raw bytes with B code bits on both sides of
    8 (R - 1) (Huffman-coded up to there, E = R - 1) and of 8 R; a Huffman
    form of equal length stays raw.  No string of R bytes has fewer than 5 R
    code bits, and one symbol has a code length: R = 1 exists with B = 7, 8
    only (both raw), R = 2 with B = 15, 16, 17 only."""
    return _lit_ties()[:2]


def lit_ties_cases():
    """(R, B, Huffman-coded) per string."""
    return _lit_ties()[2]


PREFIX_P = (126, 127, 254, 255, 16510, 16511)
PREFIX_P_BIG = (2097278, 2097279)


@functools.lru_cache(maxsize=None)
def _lit_prefix(big):
    rng = np.random.default_rng(0x9F1C)
    strs, cases, out = [], [], 0

    def place(P, kind, align):  # the literal at output byte = align (mod 4)
        nonlocal out
        lead = (align - out) % 4
        strs.extend(lead_strings(lead, rng))
        cases.append((len(strs), P, kind, lead))
        strs.append(raw_bytes(P, rng) if kind == "raw" else huff_payload(P, rng))
        out += lead + int(prefix7_len(P)) + P

    for P in PREFIX_P:
        for kind in ("raw", "huff"):
            for align in range(4):
                place(P, kind, align)
    if big:
        for k, (P, kind) in enumerate((P, kind) for P in PREFIX_P_BIG for kind in ("raw", "huff")):
            place(P, kind, k)
    return batch(strs) + (cases,)


def lit_prefix(big=True):
    """Payloads P on both sides of every prefix-length boundary (126/127: 1/2
    bytes, 254/255: 2/3, 16510/16511: 3/4, and with `big` 2097278/2097279:
    4/5), raw (R = P) and Huffman-coded (E = P), behind leads of 0..3 output
    bytes so the prefix starts at every alignment of the output words (the
    big payloads: one string per side and kind, the four leads spread over
    them).  A 6-byte prefix needs P >= 2^28 + 127, more than
    NGHTTP2_AMD_ENCODE_MAX_STRING (2^32 / 30) allows: it cannot be reached."""
    return _lit_prefix(bool(big))[:2]


def lit_prefix_cases(big=True):
    """(string, P, "raw" / "huff", lead output bytes) per placed string."""
    return _lit_prefix(bool(big))[2]


SPAN_LENS = (1, 2, 31, 32, 33, 64, 1024, 1056)


@functools.lru_cache(maxsize=None)
def _lit_raw_spans():
    rng = np.random.default_rng(0x5A95)
    b, cases = _Builder(rng), []

    def place(ln, o, modulus):
        if (len(b.strs) + 1) % 64 == 0:  # the raw string would start a wave
            b.add(fives(3, rng))
        A = b.wave_a(len(b.strs) + 1)
        b.add(fives(3 + (o - (b.pos + 3 - (A & ~15))) % modulus, rng))  # (Huffman-coded from 3 bytes)
        cases.append((b.add(raw_bytes(ln, rng)), ln, o, modulus))

    for ln in SPAN_LENS:
        for o in range(EC_RAW_MASK_BYTES):
            place(ln, o, EC_RAW_MASK_BYTES)
    for ln in (1024, 1056):  # from a round's first byte: a whole round of raw bytes
        place(ln, 0, EC_ROUND_BYTES)
    b.add(fives(3, rng))
    return batch(b.strs) + (cases,)


def lit_raw_spans():
    """Raw strings of 1..1056 bytes from every byte of a word of the round's
    raw mask, and from a round's first byte, each between two Huffman-coded
    strings."""
    return _lit_raw_spans()[:2]


def lit_raw_spans_cases():
    """(string, length, offset, modulus): the raw string starts `offset`
    bytes (mod modulus) behind its wave's first chunk."""
    return _lit_raw_spans()[2]


EMPTY_RUNS = tuple(range(1, 10)) + (62, 63, 64, 65, 130)
EMPTY_BEHIND = ("h5", "raw", "h30")


def _behind(kind, rng):
    if kind == "h5":
        return fives(4, rng)
    if kind == "raw":
        return raw_bytes(2, rng)
    return fives(11, rng) + to_bytes([rng.choice(BY_LEN[30])])


@functools.lru_cache(maxsize=None)
def _lit_empties():
    rng = np.random.default_rng(0xE3B7)
    b, cases = _Builder(rng), []
    for kind, k, par in ((kind, k, par) for kind in EMPTY_BEHIND for k in EMPTY_RUNS for par in (0, 1)):
        lead = _behind(kind, rng)  # wherever the string count puts them; its last byte even and odd
        if (b.pos + len(lead) - 1) % 2 != par:
            b.add(fives(1, rng))
        cases.append(("run", kind, k, len(b.strs) + 1))
        b.add(lead)
        for _ in range(k):
            b.add(b"")
    for a in (0, 1, 15):
        for kind in EMPTY_BEHIND:
            for k in (1, 3, 63):  # at a wave's start (then a string of `kind`)
                b.new_wave(a)
                cases.append(("start", kind, k, len(b.strs)))
                for _ in range(k):
                    b.add(b"")
                b.add(_behind(kind, rng))
            for k in (1, 5):      # at a wave's end
                b.new_wave(a)
                for _ in range(63 - k):
                    b.add(fives(3, rng))
                cases.append(("end", kind, k, len(b.strs) + 1))
                b.add(_behind(kind, rng))
                for _ in range(k):
                    b.add(b"")
            for waves in (1, 2):  # whole waves
                b.new_wave(a)
                cases.append(("whole", kind, 64 * waves, len(b.strs)))
                for _ in range(64 * waves):
                    b.add(b"")
                b.add(_behind(kind, rng))
    return batch(b.strs) + (cases,)


def lit_empties():
    """Runs of empty strings (literal 00 each) behind a byte with a 5-bit
    code, a raw byte and a 30-bit-code byte: wherever the count puts them, and
    placed at a wave's start, at its end and over whole waves, the wave
    starting at pool byte 0, 1 and 15 (mod 16)."""
    return _lit_empties()[:2]


def lit_empties_cases():
    """(where, behind, run length, first empty string)."""
    return _lit_empties()[2]


def lit_all_empty(n):
    """n empty strings over a zero-byte pool."""
    return np.zeros(0, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint32)


ALL_EMPTY_N = (1, 64, 257)
P64_TARGETS = (("sum", 63), ("sum", 64), ("sum", 65), ("sum", 72), ("L0", 64), ("L0", 69), ("L0", 128))
P64_CHUNKS = (0, 1, 63)
P64_SLOTS = (0, 3, 7)
P64_PL_PAYLOAD = {1: 40, 2: 200, 3: 300}  # a payload with a prefix of 1, 2, 3 bytes


def _p64_solve(what, T, PL, rng):
    """(l0, pad, empties, l1): a Huffman string ending in an l0-bit code with
    `pad` pad bits, `empties` empty strings, then a string with a PL-byte
    prefix starting with an l1-bit code; l0 + pad + 8 (empties + PL) is L0,
    and L0 + l1 the pair sum."""
    sol = []
    for l1 in LENGTHS:
        L0 = T - l1 if what == "sum" else T
        for e in range(0, 16):
            for pad in range(8):
                l0 = L0 - pad - 8 * (e + PL)
                if l0 in LENGTHS:
                    sol.append((l0, pad, e, l1))
    assert sol, (what, T, PL)
    return sol[int(rng.integers(len(sol)))]


def _p64_strings(l0, pad, e, l1, PL, n1, rng):
    """The strings of one case: s1 (n1 bytes, Huffman-coded, ends in the l0
    code with `pad` pad bits), e empty strings, s2."""
    lo = 5 * (n1 - 1)
    F = lo + (-(lo + l0 + pad)) % 8  # 5- and 6-bit codes before the l0 code
    six = rng.permutation(n1 - 1) < F - lo
    s1 = to_bytes(np.where(six, rng.choice(BY_LEN[6], size=n1 - 1), rng.choice(BY_LEN[5], size=n1 - 1)))
    assert int(LEN[np.frombuffer(s1, np.uint8)].sum()) == F
    s1 += to_bytes([rng.choice(BY_LEN[l0])])
    s2 = to_bytes([rng.choice(BY_LEN[l1])]) + huff_payload(P64_PL_PAYLOAD[PL], rng)
    return [s1] + [b""] * e + [s2]


@functools.lru_cache(maxsize=None)
def _lit_pairs64():
    rng = np.random.default_rng(0x9A64)
    b, cases = _Builder(rng), []
    for what, T in P64_TARGETS:
        for chunk in P64_CHUNKS:
            for slot in P64_SLOTS:
                for PL in (1, 2, 3):
                    l0, pad, e, l1 = _p64_solve(what, T, PL, rng)
                    b.new_wave(0)
                    at = EC_ROUND_BYTES + 16 * chunk + 2 * slot  # s1's last byte, from the wave's A
                    b.add(fives(at - 16, rng))
                    cases.append((what, T, chunk, slot, PL, len(b.strs), b.pos + 16, (l0, pad, e, l1)))
                    for s in _p64_strings(l0, pad, e, l1, PL, 17, rng):
                        b.add(s)
    for what, T in P64_TARGETS:  # 20-byte strings, wherever they fall (s1's last byte even)
        for PL in (1, 1, 1):
            l0, pad, e, l1 = _p64_solve(what, T, PL, rng)
            while len(b.strs) % 64 + e + 3 > 64:  # (the case within one wave)
                b.add(fives(3, rng))
            if (b.pos + 19) % 2:
                b.add(fives(1, rng))
            cases.append((what, T, None, None, PL, len(b.strs), b.pos + 19, (l0, pad, e, l1)))
            ss = _p64_strings(l0, pad, e, l1, PL, 20, rng)
            for s in ss[:-1] + [ss[-1][:20]]:
                b.add(s)
    return batch(b.strs) + (cases,)


def lit_pairs64():
    """Both sides of k_encode<FR>'s 64-bit pair limit: a pair (code, extras,
    code) of 63, 64, 65 and 72 bits, and a first code with extras (L0) of 64,
    69 and 128 bits, made of a last code, its pad, a run of empty strings and
    one prefix of 1..3 bytes -- at pair slots 0, 3 and 7 of chunks 0, 1 and 63
    of a wave's second round, and in 20-byte strings."""
    return _lit_pairs64()[:2]


def lit_pairs64_cases():
    """(what, target, chunk, slot, PL, first string, pool byte of the pair's
    first byte, (l0, pad, empties, l1)); chunk and slot None: 20-byte strings."""
    return _lit_pairs64()[2]


EDGE_AT = (1023, 1024, 1025, 2047, 2048, 2049)


@functools.lru_cache(maxsize=None)
def _lit_round_edges():
    rng = np.random.default_rng(0x20ED)
    b, cases = _Builder(rng), []
    for at in EDGE_AT:
        for PL in (1, 2, 3):
            for kind in ("huff", "raw"):
                for lead in range(4):
                    b.new_wave(0)
                    A = b.pos
                    for s in lead_strings(lead, rng):
                        b.add(s)
                    # a coded filler up to `at`, its Huffman bytes chosen so the
                    # string's literal starts at output byte = lead (mod 4)
                    nf = A + at - b.pos
                    E = -(-5 * nf // 8) + 1
                    E += (lead - (b.out + int(prefix7_len(E)) + E)) % 4
                    b.add(coded(nf, E, rng))
                    P = P64_PL_PAYLOAD[PL]
                    cases.append((b.add(raw_bytes(P, rng) if kind == "raw" else huff_payload(P, rng)),
                                  at, PL, kind, lead))
    return batch(b.strs) + (cases,)


def lit_round_edges():
    """A string starting at byte 1023, 1024 and 1025 of its wave's first and
    second round (its prefix attached to the round's last byte, to the next
    round's first): prefixes of 1..3 bytes, Huffman-coded and raw, behind
    leads of 0..3 output bytes."""
    return _lit_round_edges()[:2]


def lit_round_edges_cases():
    """(string, its first byte from the wave's A, PL, kind, lead output bytes)."""
    return _lit_round_edges()[2]


DENSE_LONG = 1024
DENSE_FIVES = 8161  # 31 one-byte strings + 8161 bytes = 8 rounds


@functools.lru_cache(maxsize=None)
def _lit_dense_round():
    rng = np.random.default_rng(0xDE25)
    big = fives(DENSE_FIVES, rng) + to_bytes(rng.choice(BY_LEN[30], size=DENSE_LONG))
    ones_ = [fives(1, rng) if i % 2 else raw_bytes(1, rng) for i in range(63)]
    return batch(ones_[:31] + [big] + ones_[31:])


def lit_dense_round():
    """The fullest image k_encode<FR> reaches: one Huffman-coded string of
    8161 5-bit-code bytes and then 1024 30-bit-code bytes that fill exactly
    one round of the wave (30 x 1024 + 5 x 8161 < 8 x 9185 bits, so E < R),
    with 31 one-byte strings before it and 32 behind."""
    return _lit_dense_round()


LIT_FAMILIES = ("lit_ties", "lit_prefix", "lit_raw_spans", "lit_empties", "lit_pairs64",
                "lit_round_edges", "lit_dense_round")


def tile_chunks(b):
    """The batch cut into batches of <= 256 strings (one-tile launches)."""
    pool, off = b
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    for i in range(0, n, 256):
        j = min(i + 256, n)
        yield (np.asarray(pool)[int(off[i]):int(off[j])], (off[i:j + 1] - off[i]).astype(np.uint32))


NO_INDEX = 0x01  # NGHTTP2_NV_FLAG_NO_INDEX
NO_INDEX_NAMES = (b"accept-charset", b"accept-language", b"accept-ranges", b"accept", b"age", b"allow",
                  b"cache-control", b"content-disposition", b"content-encoding", b"content-language",
                  b"content-location", b"content-range")


def no_index_fields():
    """A header list whose literal batch takes k_encode<FR>'s bytewise path:
    12 never-indexed fields with static-table names and empty values (12
    literals 00, their names indexed) between two ordinary fields, the first
    one's value ending at an even pool byte."""
    return ([(b"x-first", b"value-1234", 0)] + [(n, b"", NO_INDEX) for n in NO_INDEX_NAMES] +
            [(b"x-last", b"v", 0)])


def no_index_literals():
    """The strings the deflater frames for no_index_fields(), in wire order."""
    return batch([b"x-first", b"value-1234"] + [b""] * len(NO_INDEX_NAMES) + [b"x-last", b"v"])
