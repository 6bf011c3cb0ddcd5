"""GPU parity on the edges of k_encode's round loop where its per-byte
bookkeeping can go wrong: a pad at every byte of a chunk and of every width,
string ends that share a dword or a byte pair, empty strings around a padded
one, ends on a chunk's and a round's last byte, long codes next to the pad
(rounds that go bytewise between rounds that do not), every alignment of a
wave's first chunk, one-launch and two-launch batch sizes and waves with one
interior round or none -- through the plain encode and the string-literal
entry point, bit-exact against the oracle (bytes and offsets).  Every batch
is at most 1,024 strings and 64 KB; the builders assert on the CPU, with the
rounds restated by tests/boundary_batches.py, that the batch holds what it
claims.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary_batches as BB
from tests.test_parity_gpu import gpu_emit, gpu_encode

pytestmark = pytest.mark.gpu

SHORT_LENS = (5, 6, 7, 8)
LONG_LENS = tuple(L for L in BB.LENGTHS if L >= 19)  # codes of 19..30 bits
WIDTHS = tuple(range(1, 8))
ROUND = BB.EC_ROUND_BYTES


def sym(L, rng):
    return int(rng.choice(BB.BY_LEN[L]))


def body(k, w, rng):
    """k >= 3 symbols of 5..8-bit codes whose code bits leave a pad of w bits
    (w = 0: none)."""
    assert k >= 3
    lens = [int(x) for x in rng.choice(SHORT_LENS, size=k - 3)]
    need = (-w - sum(lens)) % 8
    tails = [t for t in itertools.product(SHORT_LENS, repeat=3) if sum(t) % 8 == need]
    lens += tails[int(rng.integers(len(tails)))]
    return [sym(L, rng) for L in lens]


def padded_string(k, w, rng, long_len=0, long_last=True):
    """k bytes with a pad of w bits; long_len: one code of that many bits as
    the last byte (the pad follows it) or the one before the last."""
    if not long_len:
        s = body(k, w, rng)
    elif long_last:
        s = body(k - 1, (w + long_len) % 8, rng) + [sym(long_len, rng)]
    else:
        Ls = int(rng.choice(SHORT_LENS))
        s = body(k - 2, (w + long_len + Ls) % 8, rng) + [sym(long_len, rng), sym(Ls, rng)]
    assert len(s) == k and (-int(BB.LEN[s].sum())) % 8 == w
    return bytes(s)


class Stream:
    """Strings appended one after the other; `cur` is the next byte's address."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.strs, self.cur, self.nlong = [], 0, 0

    def add(self, s):
        self.strs.append(s)
        self.cur += len(s)

    def end_at(self, pos, w, spread=0, long_window=False):
        """A string whose last byte is at chunk byte `pos`, pad w; long_window:
        a long code next to the pad when the end lies in the second KB of
        every four (so bytewise and plain rounds alternate within a wave),
        and in the fourth KB a 19-bit code before a pad of at most 4 bits (a
        pair of at most 31 bits: the round stays plain)."""
        k = (pos - self.cur) % 16 + 1
        while k < 5:
            k += 16
        k += spread
        end = self.cur + k - 1
        L, last = 0, True
        if long_window and (end >> 10) & 3 == 1:
            L = LONG_LENS[self.nlong % len(LONG_LENS)]
            self.nlong += 1
            last = self.nlong % 2 == 0
        elif long_window and (end >> 10) & 3 == 3 and w <= 4:
            L = 19
        self.add(padded_string(k, w, self.rng, L, long_last=last))
        assert (self.cur - 1) % 16 == pos

    def batch(self):
        return BB.batch(self.strs)


def ends_and_pads(b):
    """(address of the last byte, pad bits) of a batch's non-empty strings."""
    S = BB.literal_strings(*b)
    ne = S["R"] > 0
    return S["off"][1:][ne] - 1, (8 * S["E"] - S["bits"])[ne]


def assert_grid(b):
    end, pad = ends_and_pads(b)
    have = set(zip((end % 16).tolist(), pad.tolist()))
    assert have >= set(itertools.product(range(16), WIDTHS))


def wave_rounds(b):
    """pack_rounds grouped by wave."""
    out = {}
    for r in BB.pack_rounds(*b):
        out.setdefault(r["t0"], []).append(r)
    return out


def grid(spread, long_window, seed, raw=False):
    """raw: behind every string of the grid one of 1..20 bytes with codes of
    8 bits and more (its Huffman form is no shorter: a raw literal)."""
    st = Stream(seed)
    for pos in range(16):
        for w in WIDTHS:
            st.end_at(pos, w, spread, long_window)
            if raw:
                k = 1 + int(st.rng.integers(20))
                st.add(bytes([sym(8, st.rng) for _ in range(k - 1)] + [sym(LONG_LENS[(pos + w) % len(LONG_LENS)], st.rng)]))
    return st.batch()


@functools.lru_cache(maxsize=None)
def pad_grid_short():
    """16 positions x 7 widths, short strings: a wave is one or two rounds."""
    b = grid(0, False, 0xA11)
    assert_grid(b)
    return b


@functools.lru_cache(maxsize=None)
def pad_grid_rounds():
    """The same grid with strings of 50..70 bytes: waves of several rounds,
    the middle ones interior and on the plain path."""
    b = grid(48, False, 0xA12)
    assert_grid(b)
    w0 = wave_rounds(b)[0]
    assert len(w0) >= 3 and not any(r["bytewise"] for r in w0)
    assert any(r["store"] == "store4" for r in w0[1:-1])
    return b


@functools.lru_cache(maxsize=None)
def pad_specials():
    """Ends on a round's last byte (1023, 2047, ...) with every width; runs of
    one-byte strings (ends in one pair and one dword, pads 3, 2, 1) and of
    two-byte strings (two ends in one dword, pads 6..1); empty strings before
    and after padded ones; a tail that gives the last wave interior rounds."""
    st = Stream(0xA13)
    for w in WIDTHS:  # string i ends on byte 1024 i + 1023
        st.add(padded_string(ROUND, w, st.rng))
    for i in range(48):
        st.add(bytes([sym(SHORT_LENS[i % 3], st.rng)]))
    two = ((5, 5), (5, 6), (5, 7), (5, 8), (6, 8), (7, 8))
    for i in range(48):
        st.add(bytes(sym(L, st.rng) for L in two[i % 6]))
    for w in WIDTHS:
        st.add(b"")
        st.end_at(15, w)
        st.add(b"")
        st.add(b"")
        st.end_at(3 + w, w)
    for i in range(40):
        st.end_at(i % 16, 1 + i % 7, 64)
    b = st.batch()
    end, pad = ends_and_pads(b)
    S = BB.literal_strings(*b)
    assert {int(p) for e, p in zip(end, pad) if e % ROUND == ROUND - 1} >= set(WIDTHS)
    both = (pad[:-1] > 0) & (pad[1:] > 0)
    assert (both & (end[:-1] // 2 == end[1:] // 2)).any(), "two padded ends in one pair"
    assert (both & (end[:-1] // 4 == end[1:] // 4) & (end[:-1] // 2 != end[1:] // 2)).any()
    R, padl = S["R"], 8 * S["E"] - S["bits"]
    assert ((R[:-2] == 0) & (padl[1:-1] > 0) & (R[2:] == 0)).any(), "empty, padded, empty"
    assert {int(p) for e, p in zip(end, pad) if e % 16 == 15} >= set(WIDTHS)
    return b


@functools.lru_cache(maxsize=None)
def long_grid():
    """The grid with a code of 19..30 bits as the padded byte or the one
    before it, in the second KB of every four: within one wave plain rounds,
    bytewise rounds, and a plain round behind a bytewise one."""
    b = grid(48, True, 0xA14)
    assert_grid(b)
    S = BB.literal_strings(*b)
    longb = BB.LEN[S["raw"][:int(S["off"][-1])]] >= 19
    assert longb.sum() >= 12
    ok = False
    for rs in wave_rounds(b).values():
        bw = [r["bytewise"] for r in rs]
        ok |= any(x and not y for x, y in zip(bw, bw[1:])) and any(y and not x for x, y in zip(bw, bw[1:]))
    assert ok, "no wave goes bytewise and back"
    # both sides of the switch: a pair of exactly 31 bits at most in a plain
    # round, pairs of 32 and more in the bytewise ones
    rounds = list(BB.pack_rounds(*b))
    assert any(r["bytewise"] for r in rounds)
    assert any(not r["bytewise"] and r["pairs"].max() >= 19 + 5 for r in rounds)
    return b


@functools.lru_cache(maxsize=None)
def mixed_literals():
    """The long-code grid with a raw literal behind every string: Huffman and
    raw literals alternate in every wave."""
    b = grid(48, True, 0xA18, raw=True)
    assert_grid(b)
    H = BB.literal_strings(*b)["H"]
    assert all(H[t:t + 64].any() and not H[t:t + 64].all() for t in range(0, len(H), 64))
    return b


@functools.lru_cache(maxsize=None)
def long_tiles():
    """A tile with no code over 15 bits, one with a 30-bit code in its middle,
    and a third without again."""
    st = Stream(0xA15)
    for i in range(3 * 256):
        L = 30 if i == 256 + 130 else 0
        st.add(padded_string(20 + i % 9, 1 + i % 7, st.rng, L))
    b = st.batch()
    S = BB.literal_strings(*b)
    per_tile = [int(BB.LEN[S["raw"][int(S["off"][t]):int(S["off"][t + 256])]].max()) for t in (0, 256, 512)]
    assert per_tile[0] <= 15 and per_tile[1] == 30 and per_tile[2] <= 15
    return b


@functools.lru_cache(maxsize=None)
def aligned_waves():
    """16 waves of 64 strings; wave j's first byte at chunk byte j, each of
    about three rounds, pads of every width at every position."""
    st = Stream(0xA16)
    for j in range(16):
        assert st.cur % 16 == j
        for i in range(63):
            st.end_at((5 * i + j) % 16, 1 + (i + j) % 7, 32)
        st.end_at(j, 1 + j % 7, 32)  # the next wave starts one byte further
    b = st.batch()
    assert len(b[1]) - 1 == 1024 and int(b[1][-1]) <= 65536
    assert [int(b[1][64 * j]) % 16 for j in range(16)] == list(range(16))
    assert_grid(b)
    return b


@functools.lru_cache(maxsize=None)
def round_shapes():
    """Wave 0: three rounds (exactly one interior); wave 1: two rounds, wave
    2: one (no interior round)."""
    st = Stream(0xA17)
    for i in range(64):
        st.end_at(i % 16, 1 + i % 7, 32 if i < 48 else 16)
    for i in range(64):
        st.end_at((3 * i) % 16, 1 + i % 7, 16 if i < 32 else 0)
    for i in range(64):
        st.end_at((7 * i) % 16, 1 + i % 7)
    b = st.batch()
    wr = wave_rounds(b)
    assert [len(wr[t]) for t in (0, 64, 128)] == [3, 2, 1]
    assert wr[0][1]["store"] == "store4" and not wr[0][1]["bytewise"]
    return b


def prefix(b, n):
    pool, off = b
    return pool[:int(off[n])], off[:n + 1].copy()


BATCHES = {"pad_grid_short": pad_grid_short, "pad_grid_rounds": pad_grid_rounds,
           "pad_specials": pad_specials, "long_grid": long_grid, "mixed_literals": mixed_literals,
           "long_tiles": long_tiles,
           "aligned_waves": aligned_waves, "round_shapes": round_shapes}
SIZES = (1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def case(name, filled=False, n=None):
    """(pool, off, the oracle's encode, the oracle's literals) of a batch: as
    built, behind a tile of fill (the two-launch instance whatever its size),
    or cut to its first n strings."""
    b = BATCHES[name]()
    if n is not None:
        b = prefix(b, n)
    if filled:
        b = BB.with_fill(b)
    assert len(b[1]) - 1 <= 1024 + BB.FILL_STRINGS and int(b[1][-1]) <= 65536 + 1024
    return b, O.encode_batch(*b), O.emit_strings_batch(*b)


def check(codec, dev, c, tag, literals=False):
    (pool, off), (renc, reo), (rlit, rlo) = c
    if literals:
        got, go, want, wo = gpu_emit(codec, dev, pool, off) + (rlit, rlo)
    else:
        got, go, want, wo = gpu_encode(codec, dev, pool, off) + (renc, reo)
    assert np.array_equal(go, wo), tag + ": offsets"
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        raise AssertionError("%s: byte %d differs (string %d)" % (tag, i, int(np.searchsorted(wo, i, side="right") - 1)))


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
@pytest.mark.parametrize("name", ["pad_grid_short", "pad_grid_rounds", "pad_specials"])
def test_pad_positions(codec, dev, name, filled):
    check(codec, dev, case(name, filled), name)


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
@pytest.mark.parametrize("name", ["long_grid", "mixed_literals", "long_tiles"])
def test_long_code_switch(codec, dev, name, filled):
    check(codec, dev, case(name, filled), name)


@pytest.mark.parametrize("name", ["aligned_waves", "round_shapes"])
def test_wave_alignments_and_round_shapes(codec, dev, name):
    check(codec, dev, case(name), name)
    check(codec, dev, case(name, True), name + " filled")


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(codec, dev, n):
    """The one-launch instance up to 256 strings, two tiles at 257; each also
    behind a tile of fill."""
    check(codec, dev, case("aligned_waves", False, n), "n=%d" % n)
    check(codec, dev, case("aligned_waves", True, n), "n=%d filled" % n)


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
@pytest.mark.parametrize("name", ["pad_grid_short", "pad_grid_rounds", "pad_specials", "long_grid",
                                  "mixed_literals", "aligned_waves"])
def test_string_literals(codec, dev, name, filled):
    check(codec, dev, case(name, filled), name, literals=True)
