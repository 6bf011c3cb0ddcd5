"""GPU parity where the count's one-byte in-chunk prefixes can go wrong
(wave_string_bits: a lane keeps its chunk's 16 exclusive prefixes as bytes,
each 8-byte half counted from 0, the first half's total in byte 8): halves
saturated with 30-bit codes (a total of 240, prefixes up to 210, the largest
the byte fields hold), string starts and ends at in-chunk positions 0, 1, 7,
8, 9 and 15 against each other within a chunk, across neighbouring chunks and
across rounds, the wave's last byte on a chunk and on a round boundary, empty
strings at a wave's start, middle and end, a wave inside one chunk, and batch
sizes on both sides of the one-launch / two-launch switch -- through the
plain encode and the string-literal entry point, bit-exact against the
oracle (bytes and every offset).  Each batch runs as built (at most 256
strings: counted inside the one-tile k_encode) and behind a tile of fill
(counted by k_enc_count).  The builders assert on the CPU that a batch holds
what it claims, and that the oracle's offsets are the code lengths' sums.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary_batches as BB
from tests.test_parity_gpu import gpu_emit, gpu_encode

pytestmark = pytest.mark.gpu

ROUND = BB.EC_ROUND_BYTES
EDGES = (0, 1, 7, 8, 9, 15)
SATURATED = (30, 28, 5)  # code bits of every byte of a saturated batch
SIZES = (1, 63, 64, 65, 255, 256, 257, 300, 600)


def chunk_view(b):
    """(a batch's bytes' code lengths as rows of 16, padded with -1)."""
    pool, off = b
    L = BB.LEN[pool[:int(off[-1])]]
    pad = (-len(L)) % 16
    return np.concatenate([L, np.full(pad, -1, dtype=L.dtype)]).reshape(-1, 16)


@functools.lru_cache(maxsize=None)
def saturated(bits):
    """Strings of 17 bytes, every byte a code of `bits` bits: an end (and the
    next string's start) at every in-chunk position, every chunk's halves at
    8 x bits.  Two waves and a part of a third; the first wave's strings
    cross two rounds."""
    syms = BB.BY_LEN[bits]
    if bits == 30:
        assert sorted(syms.tolist()) == [10, 13, 22]
    rng = np.random.default_rng(0xB100 + bits)
    strs = [bytes(rng.choice(syms, size=17).astype(np.uint8)) for _ in range(150)]
    b = BB.batch(strs)
    off = b[1].astype(np.int64)
    assert {int(x) % 16 for x in off[1:]} == set(range(16))
    C = chunk_view(b)
    full = (C == bits).all(axis=1)
    assert full[:-1].all()
    # every end position lies in a chunk that is saturated on both halves
    assert {int(x) % 16 for x in off[1:] if full[int(x) >> 4]} == set(range(16))
    half = C[full].reshape(-1, 2, 8)
    assert (half.sum(axis=2) == 8 * bits).all() and (np.cumsum(half, axis=2)[:, :, 6] == 7 * bits).all()
    assert int(off[64]) > ROUND  # wave 0 has a second round
    return b


@functools.lru_cache(maxsize=None)
def end_positions():
    """For every start position sa and end position sb of EDGES: a string in
    one chunk (sb >= sa; an empty one when equal), one that ends in the next
    chunk, and one longer than a round (its ends are in different rounds of
    its wave) -- bytes of every code length."""
    rng = np.random.default_rng(0xB200)
    strs, cur, kinds = [], 0, set()

    def add(k):
        nonlocal cur
        strs.append(bytes(rng.integers(0, 256, size=k, dtype=np.uint8)))
        cur += k

    for sa, sb in itertools.product(EDGES, EDGES):
        for kind in ("chunk", "next", "round"):
            if kind == "chunk" and sb < sa:
                continue
            if (sa - cur) % 16:
                add((sa - cur) % 16)
            a = cur
            add(sb - sa + {"chunk": 0, "next": 16, "round": ROUND + 16}[kind])
            assert a % 16 == sa and cur % 16 == sb
            assert {"chunk": (cur >> 4) - (a >> 4) == 0, "next": (cur >> 4) - (a >> 4) == 1,
                    "round": cur - a > ROUND}[kind]
            kinds.add((sa, sb, kind))
    assert len(kinds) == 36 + 36 + 21
    assert len(strs) <= 256 and cur <= 65536
    return BB.batch(strs)


Z_SPANS = (16, ROUND, ROUND + 16, 2 * ROUND)


@functools.lru_cache(maxsize=None)
def wave_ends():
    """Waves of 64 strings whose last byte Z is on a chunk boundary, and for
    two of them on a round boundary of the wave (Z - 16 (A >> 4) = 1024 and
    2048), each with its two last strings empty (both ends at Z: no round
    holds them); the waves start at in-chunk positions 0, 5, 0, 0."""
    rng = np.random.default_rng(0xB300)
    strs, cur = [], 0
    for w, span in enumerate(Z_SPANS):
        assert len(strs) == 64 * w
        A = cur
        total = span - (A & 15)
        cuts = np.sort(rng.integers(0, total + 1, size=61))
        lens = np.diff(np.concatenate([[0], cuts, [total]]))
        if w == 0:
            lens = np.array([5] + [0] * 61)  # the next wave starts at byte 5 ...
        for k in lens.tolist() + [0, 0]:
            strs.append(bytes(rng.integers(0, 256, size=int(k), dtype=np.uint8)))
            cur += int(k)
        if w == 0:
            continue  # ... so this one ends inside its chunk
        assert cur % 16 == 0 and cur - (A & ~15) == span
    b = BB.batch(strs)
    off = b[1].astype(np.int64)
    assert [int(off[64 * w]) % 16 for w in range(4)] == [0, 5, 0, 0]
    return b


@functools.lru_cache(maxsize=None)
def empties():
    """Wave 0: empty strings at its start, middle and end.  Wave 1: 64 strings
    inside one aligned chunk (16 of one byte between empty ones).  Wave 2:
    only empty strings.  Wave 3 (partial): a string behind them."""
    rng = np.random.default_rng(0xB400)
    rb = lambda k: bytes(rng.integers(0, 256, size=k, dtype=np.uint8))
    w0 = [b""] * 3 + [rb(9 + i % 23) for i in range(27)] + [b""] * 4 + [rb(40 + i) for i in range(26)]
    w0.append(rb((-sum(len(s) for s in w0)) % 16 + 16))  # wave 1 starts a chunk
    w0 += [b""] * 3
    w1 = [rb(1) if i % 4 == 1 else b"" for i in range(64)]
    strs = w0 + w1 + [b""] * 64 + [rb(33)]
    assert len(w0) == 64 and sum(len(s) for s in w0) % 16 == 0 and sum(len(s) for s in w1) == 16
    return BB.batch(strs)


@functools.lru_cache(maxsize=None)
def sizes():
    """600 strings of 0..40 bytes, every tenth of 100..1500 (several rounds)."""
    rng = np.random.default_rng(0xB500)
    strs = [bytes(rng.integers(0, 256, size=int(rng.integers(100, 1500) if i % 10 == 9 else rng.integers(0, 41)),
                               dtype=np.uint8)) for i in range(600)]
    return BB.batch(strs)


BATCHES = {"saturated30": lambda: saturated(30), "saturated28": lambda: saturated(28),
           "saturated5": lambda: saturated(5), "end_positions": end_positions, "wave_ends": wave_ends,
           "empties": empties, "sizes": sizes}


@functools.lru_cache(maxsize=None)
def case(name, filled=False, n=None):
    """(batch, the oracle's encode, the oracle's literals): as built, behind
    a tile of fill, or cut to its first n strings."""
    b = BATCHES[name]()
    if n is not None:
        b = (b[0][:int(b[1][n])], b[1][:n + 1].copy())
    if filled:
        b = BB.with_fill(b)
    pool, off = b
    assert len(off) - 1 <= 600 + BB.FILL_STRINGS and int(off[-1]) <= 131072
    enc = O.encode_batch(pool, off)
    # the oracle's offsets are the sums of the code lengths, rounded up
    bits = np.add.reduceat(np.concatenate([BB.LEN[pool[:int(off[-1])]], [0]]),
                           np.minimum(off[:-1].astype(np.int64), int(off[-1])))
    bits[off[1:] == off[:-1]] = 0
    assert np.array_equal(np.diff(enc[1].astype(np.int64)), (bits + 7) // 8)
    return b, enc, O.emit_strings_batch(pool, off)


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
@pytest.mark.parametrize("bits", SATURATED)
def test_saturated_halves(codec, dev, bits, filled):
    check(codec, dev, case("saturated%d" % bits, filled), "saturated %d" % bits)


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
def test_end_positions(codec, dev, filled):
    check(codec, dev, case("end_positions", filled), "end positions")


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
def test_wave_end_on_chunk_and_round_boundary(codec, dev, filled):
    check(codec, dev, case("wave_ends", filled), "wave ends")


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
def test_empty_strings_and_one_chunk_wave(codec, dev, filled):
    check(codec, dev, case("empties", filled), "empties")


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(codec, dev, n):
    """One launch up to 256 strings, the count and the tile sums from 257;
    each also behind a tile of fill (partial last waves in k_enc_count)."""
    check(codec, dev, case("sizes", False, n), "n=%d" % n)
    check(codec, dev, case("sizes", True, n), "n=%d filled" % n)


@pytest.mark.parametrize("filled", [False, True], ids=["built", "filled"])
@pytest.mark.parametrize("name", ["saturated30", "saturated28", "saturated5", "end_positions"])
def test_string_literals(codec, dev, name, filled):
    check(codec, dev, case(name, filled), name, literals=True)
