"""CPU checks of tests/boundary_batches.py: the grids hit what they claim.

Each check rebuilds the plan from the constants csrc/hd_huff.hip defines
(boundary_batches.kernel_defaults reads the source), finds every planned case
in the generated batch by the oracle's decode and the code table alone, and
prints the family's string count; a planned case that is missing or misplaced
fails the test -- nothing is filtered out.
"""
import numpy as np

from oracle import oracle as O
from tests import boundary_batches as BB

K = BB.kernel_defaults()
BOUNDS = (K["DD_IP40"], K["PIECE_BYTES"], K["DD_IP64"])


def strings(b):
    pool, off = b
    return [bytes(pool[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def test_constants_match_kernel():
    for name, v in K.items():
        assert getattr(BB, name) == v, "%s: the grids assume %d, hd_huff.hip has %d" % (
            name, getattr(BB, name), v)
    # the fast-pair limits the straddle and ends grids walk across
    assert 2 * K["DD_LB64"] - 4 == 22 and 2 * K["DD_LB40"] == 26


def test_code_lengths():
    assert len(BB.LENGTHS) == 21 and len(BB.BY_LEN[30]) == 3
    assert len(BB.STRADDLE_SYMS) == 23
    sym = O.tables_ref_layout()[0]
    nbits = np.frombuffer(sym, dtype="<u4").reshape(257, 2)[:256, 0]
    assert np.array_equal(nbits, BB.LEN)  # the oracle's table


def symbol_starts(s):
    """(symbols, bit position of each codeword) of a string the oracle
    accepts (the bits its decoded symbols take, in order)."""
    rv, out, _ = O.decode(s, final=1)
    assert rv >= 0, rv
    syms = np.frombuffer(out, dtype=np.uint8).astype(np.int64)
    ends = np.cumsum(BB.LEN[syms])
    return syms, ends - BB.LEN[syms], int(ends[-1]) if len(ends) else 0


def test_straddle_grid():
    strs, cases = strings(BB.straddle()), BB.straddle_cases()
    print("straddle: %d strings, longest %d bytes" % (len(strs), max(map(len, strs))))
    assert len(strs) == len(cases)
    found = set()
    for s, (B, k, sym, s_bits, ending) in zip(strs, cases):
        syms, starts, nbits = symbol_starts(s)
        at = 8 * B * k - s_bits
        j = int(np.searchsorted(starts, at))
        if j == len(starts) or starts[j] != at or syms[j] != sym:
            continue  # no codeword of sym starts there: misplaced
        tail = nbits - (at + int(BB.LEN[sym]))
        if tail != (64 if ending == "more" else 0) or len(s) != (nbits + 7) // 8:
            continue
        if not (syms[:j] < 256).all() or BB.LEN[syms[:j]].max() > 6 or BB.LEN[syms[j + 1:]].max(initial=0) > 6:
            continue
        found.add((B, k, sym, s_bits, ending))
    missing = [c for c in BB.straddle_plan(BOUNDS) if c not in found]
    assert missing == [], "%d missing or misplaced, e.g. %s" % (len(missing), missing[:5])
    assert max(map(len, strs)) <= 260


def test_ends_grid():
    strs, cases = strings(BB.ends()), BB.ends_cases()
    print("ends: %d strings, %d bytes" % (len(strs), sum(map(len, strs))))
    assert len(strs) == len(cases)
    # the plan, from the kernel's constants and a DP of this test's own
    feas = [True] + [False] * 63
    for b in range(1, 64):
        feas[b] = any(b >= L and feas[b - L] for L in set(BB.LEN.tolist()))
    plan = set()
    for E in BB.ends_lengths(BOUNDS, K["DD_BI64"]):
        for p in range(8):
            nb = 8 * E - p
            if nb > 0 and (nb >= 64 or feas[nb]):
                plan |= {(E, p, v) for v in ["valid", "ff"] + ["first0"] * (p >= 1) + ["last0"] * (p >= 2)}
    assert {E for E, _, _ in plan} >= set(range(1, 201)) | {2303, 2304, 2305, 39, 40, 41, 575, 576, 577}
    assert {p for _, p, _ in plan} == set(range(8))
    found = set()
    for s, (E, p, v) in zip(strs, cases):
        if len(s) != E + (v == "ff"):
            continue
        rv, out, ctx = O.decode(s, final=1)
        if (rv >= 0) != BB.ends_accepts(p, v) or (rv < 0 and rv != O.NGHTTP2_ERR_HEADER_COMP):
            continue
        if v == "valid":  # exactly p pad bits behind the last symbol
            syms = np.frombuffer(out, dtype=np.uint8).astype(np.int64)
            if 8 * E - int(BB.LEN[syms].sum()) != p:
                continue
        found.add((E, p, v))
    missing = sorted(plan - found)
    assert missing == [], "%d missing, e.g. %s" % (len(missing), missing[:5])
    assert set(cases) == plan
    # the one altered padding the reference accepts: 011111 is a 6-bit code
    assert sum(1 for E, p, v in cases if v != "valid" and BB.ends_accepts(p, v)) == \
        sum(1 for E, p, v in cases if v == "first0" and p >= 6)


def test_tasks_grid():
    for last in (1, 31, 32, 33):
        enc, eoff = BB.tasks(last)
        cases = BB.tasks_cases(last)
        lens = np.diff(eoff.astype(np.int64))
        print("tasks(last=%d): %d strings in %d tasks, %d bytes" % (last, len(lens), len(cases),
                                                                   int(eoff[-1])))
        wrong = []
        for name, start, count, items, nbytes in cases:
            e = lens[start:start + count]
            got = (start % K["TASK_STR"], int(sum(max(1, -(-int(x) // K["DD_IP64"])) for x in e)),
                   int(e.sum()))
            if got != (0, items, nbytes) or (count != K["TASK_STR"] and start + count != len(lens)):
                wrong.append((name, got))
        assert wrong == []
        by = {c[0]: c for c in cases}
        # the budget: 64 x 36 bytes fill a round exactly, 37 spill into a second
        assert by["uniform 36"][4] == K["DD_BI64"] and by["uniform 37"][4] > K["DD_BI64"]
        assert by["uniform 96"][3] == 64 and by["uniform 97"][3] == 128
        assert by["97 at lane 0"][3] == 65 and by["final %d" % last][2] == last
        assert by["63 empty + 2400"][3] == 63 + 2400 // K["DD_IP64"]
        ss = strings((enc, eoff))
        for i, s in enumerate(ss):
            if i % 7 != 6:  # (every 7th is random bytes)
                assert O.decode(s, final=1)[0] >= 0, i


def test_shifted():
    b = BB.straddle()
    for j in (0, 1, 33):
        enc, eoff = BB.shifted(b, j)
        assert len(eoff) == len(b[1]) + j and int(eoff[j]) == 3 * j
        for s in strings((enc, eoff))[:j]:
            assert len(s) == 3 and O.decode(s, final=1)[0] >= 0
        assert np.array_equal(enc[3 * j:], b[0])
        assert np.array_equal(eoff[j:].astype(np.int64) - 3 * j, b[1])


def test_round_words_grid():
    plain = BB.round_words()
    assert int(plain[1][-1]) > 0 and len(plain[1]) - 1 <= 256  # one tile without the fill
    for tag, (pool, off) in (("plain", plain), ("filled", BB.with_fill(plain))):
        n = len(off) - 1
        deltas, words = {}, {}
        for r in BB.pack_rounds(pool, off):
            if r["store"] == "edge" or r["first"] or r["last"]:
                continue
            deltas.setdefault(r["bits"] - 8 * K["EC_ROUND_BYTES"], set()).add(r["store"])
            words.setdefault(r["nst"], set()).add(r["store"])
        print("round_words %s: %d strings, %d bytes, interior rounds of %d..%d words" % (
            tag, n, int(off[-1] - off[0]), min(words), max(words)))
        missing = [d for d in range(-70, 71) if d not in deltas]
        assert missing == [], missing
        T = K["EC_STORE4_WORDS"]
        assert all(words[w] == {"store4"} for w in words if w <= T)
        assert all(words[w] == {"loop"} for w in words if w > T)
        assert {T - 2, T - 1, T, T + 1, T + 2} <= set(words)
        assert ((n > 256) == (tag == "filled"))
    # each string at pool alignment 0 and again behind the 5-byte string
    lens = np.diff(plain[1].astype(np.int64))
    assert sorted(set(lens.tolist())) == [5, 4096]
    k = int(np.nonzero(lens == 5)[0][0])
    assert k == len(lens) - 1 - k and (plain[1][:k + 1] % 4096 == 0).all()
    # 8-bit-code symbols but for the swapped bytes
    assert (BB.LEN[plain[0]] == 8).mean() > 0.97


def test_long_pairs_grid():
    plain = BB.long_pairs()
    cases = BB.long_pairs_cases()
    sums = {30, 31, 32, 33, 35, 60}
    for tag, (pool, off), shift in (("plain", plain, 0), ("filled", BB.with_fill(plain), BB.FILL_STRINGS)):
        print("long_pairs %s: %d strings, %d bytes" % (tag, len(off) - 1, int(off[-1] - off[0])))
        rounds = {(r["t0"], r["base"]): r for r in BB.pack_rounds(pool, off)}
        bases = sorted(rounds)
        found, short = set(), set()
        for i, at, pair, chunk, slot in cases:
            q = int(off[i + shift]) + at
            t0 = (i + shift) // 64 * 64
            key = max(b for b in bases if b[0] == t0 and b[1] <= q)
            r = rounds[key]
            j = (q - key[1]) >> 1
            if r["pairs"][j] != sum(pair) or (BB.LEN[pool[q]], BB.LEN[pool[q + 1]]) != pair:
                continue
            if chunk is None:  # a 20-byte string: the slot its pool position gives
                short.add((sum(pair), j % 8))
                continue
            big = np.nonzero(r["pairs"] >= 30)[0]
            if big.tolist() != [j] or (j // 8, j % 8) != (chunk, slot):
                continue
            if r["bytewise"] != (sum(pair) >= K["EC_LONG_PAIR_BITS"]) or (q - key[1]) >= K["EC_ROUND_BYTES"]:
                continue
            found.add((pair, chunk, slot))
        plan = {(pair, chunk, slot) for pair in BB.LP_PAIRS for chunk in (0, 1, 63) for slot in range(8)}
        assert sorted(plan - found) == []
        assert {sum(p) for p in BB.LP_PAIRS} == sums
        assert {s for s, _ in short} == sums and {j for _, j in short} == set(range(8))
        assert sum(1 for c in cases if c[3] is None) == len(BB.LP_PAIRS) * 10


def test_with_fill_keeps_alignment():
    pool, off = BB.with_fill(BB.long_pairs())
    assert int(off[BB.FILL_STRINGS]) % 16 == 0 and BB.FILL_STRINGS == 256
    assert np.diff(off[:BB.FILL_STRINGS + 1].astype(np.int64)).max() <= 7


def test_offset_pool_shape():
    total = 0
    for a0 in BB.OFFSET_A0:
        for n in BB.OFFSET_N:
            for fill in BB.OFFSET_FILL:
                buf, off, rpool, roff = BB.offset_pool(a0, n, fill)
                total += n
                end = int(off[-1])
                assert int(off[0]) == a0 and len(off) == n + 1 and int(roff[0]) == 0
                assert len(buf) == (end + 15) // 16 * 16 + 16
                assert np.array_equal(off.astype(np.int64) - a0, roff)
                assert np.array_equal(buf[a0:end], rpool)
                outside = np.concatenate([buf[:a0], buf[end:]])
                if fill == "ff":
                    assert (outside == 0xFF).all()
                else:
                    assert len(set(outside.tolist())) > 8
                lens = np.diff(roff.astype(np.int64))
                if n:
                    assert lens.max() == 3000
                if n >= 64:
                    assert (lens == 0).sum() >= 10 and lens[lens < 3000].max() > 100
    print("offset_pool: %d pools, %d strings" % (len(BB.OFFSET_A0) * len(BB.OFFSET_N) * 2, total))
    assert BB.OFFSET_A0 == (1, 15, 16, 17, 4099) and BB.OFFSET_N == (0, 1, 64, 65, 257, 600)
