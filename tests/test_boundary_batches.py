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


# ---- string literals (k_encode<FR>): the grids through BB.literal_rounds ----
RW_F = K["EC_RW"] + K["EC_RW_F_MARGIN"]
LONG_F = K["EC_LONG_PAIR_BITS_F"]


def lit_views(b):
    """(tag, string shift, strings, rounds) of a family as built and behind
    the fill; the model's literal offsets must be the oracle's, and every
    round must fit k_encode<FR>'s image."""
    for tag, (pool, off), shift in (("plain", b, 0), ("filled", BB.with_fill(b), BB.FILL_STRINGS)):
        S = BB.literal_strings(pool, off)
        assert np.array_equal(S["lo"], O.emit_strings_batch(pool, off)[1]), tag
        rounds = list(BB.literal_rounds(pool, off))
        assert max(r["top"] for r in rounds) < RW_F and K["EC_M"] + max(r["nw"] for r in rounds) <= RW_F
        yield tag, shift, S, rounds


def round_of(rounds, t0, q):
    """The round of wave t0 that holds pool byte q."""
    return max((r for r in rounds if r["t0"] == t0 and r["base"] <= q), key=lambda r: r["base"])


def test_literal_constants():
    assert LONG_F == 65 and K["EC_RW_F_MARGIN"] == 112 and K["EC_RAW_MASK_BYTES"] == 32
    assert BB.prefix7_len(np.array([0, 126, 127, 254, 255, 16510, 16511, 2097278, 2097279])).tolist() == \
        [1, 1, 2, 2, 3, 3, 4, 4, 5]
    # a 6-byte prefix is out of reach: 2^28 + 127 > NGHTTP2_AMD_ENCODE_MAX_STRING
    assert BB.PREFIX_EDGES[4] == 2 ** 28 + 127 > 0xFFFFFFFF // 30


def test_lit_ties_grid():
    cases = BB.lit_ties_cases()
    left_out = sorted(set(BB.ties_plan()) - {(R, B) for R, B, _ in cases})
    # no such string: fewer than 5 R code bits, or one symbol with no such code
    assert left_out == [(1, -1), (1, 0), (1, 1), (1, 9), (2, 7), (2, 8), (2, 9)]
    assert all(B < 5 * R or (R == 1 and B not in BB.LENGTHS) for R, B in left_out)
    big = [(R, B) for R, B in BB.ties_plan() if R >= 3]
    assert sum(1 for c in big if c in left_out) <= 0.05 * len(big)
    for tag, shift, S, rounds in lit_views(BB.lit_ties()):
        print("lit_ties %s: %d strings (%d of %d planned cases are no string)" % (
            tag, len(cases), len(left_out), len(BB.ties_plan())))
        for i, (R, B, huff) in enumerate(cases):
            k = i + shift
            assert (S["R"][k], S["bits"][k], bool(S["H"][k])) == (R, B, huff), (R, B)
            assert S["P"][k] == (R - 1 if huff else R)
        assert cases[0] == (0, 0, False) and S["PL"][shift] == 1 and S["P"][shift] == 0
        assert not any(h for R, _, h in cases if R <= 1)
        for R in BB.TIE_R[2:]:  # both sides, and the tie itself (E = R stays raw)
            got = {B - 8 * (R - 1): h for r, B, h in cases if r == R}
            assert got == {-1: True, 0: True, 1: False, 7: False, 8: False, 9: False}, R
        assert {B - 8 for R, B, h in cases if R == 2} == {7, 8, 9}


def test_lit_prefix_grid():
    cases = BB.lit_prefix_cases()
    want = {126: 1, 127: 2, 254: 2, 255: 3, 16510: 3, 16511: 4, 2097278: 4, 2097279: 5}
    for tag, shift, S, rounds in lit_views(BB.lit_prefix()):
        print("lit_prefix %s: %d strings, %d bytes" % (tag, len(S["R"]) - shift, int(S["off"][-1])))
        align = {}
        for i, P, kind, lead in cases:
            k = i + shift
            assert S["P"][k] == P and S["PL"][k] == want[P] and bool(S["H"][k]) == (kind == "huff")
            assert (S["R"][k] == P) == (kind == "raw")
            align.setdefault((P, kind), set()).add(int(S["lo"][k]) % 4)
        assert set(align) == {(P, kind) for P in want for kind in ("raw", "huff")}
        assert all(a == {0, 1, 2, 3} for (P, _), a in align.items() if P < 2 ** 20)
        assert set().union(*(a for (P, _), a in align.items() if P >= 2 ** 20)) == {0, 1, 2, 3}
        assert {c[3] for c in cases} == {0, 1, 2, 3}  # leads of 0..3 output bytes
    small = BB.lit_prefix(big=False)
    assert int(small[1][-1]) < 400000 and len(BB.lit_prefix_cases(big=False)) == len(cases) - 4


def test_lit_raw_spans_grid():
    cases = BB.lit_raw_spans_cases()
    W = K["EC_RAW_MASK_BYTES"]
    for tag, shift, S, rounds in lit_views(BB.lit_raw_spans()):
        print("lit_raw_spans %s: %d strings, %d bytes" % (tag, len(S["R"]) - shift, int(S["off"][-1])))
        off = S["off"]
        seen, full_words, crossing = set(), {}, 0
        for i, ln, o, modulus in cases:
            k = i + shift
            A16 = int(off[k - k % 64]) & ~15
            a, b = int(off[k]) - A16, int(off[k + 1]) - A16
            assert k % 64 and (a % modulus, b - a, bool(S["H"][k])) == (o, ln, False)
            assert S["H"][k - 1] and S["H"][k + 1] and S["R"][k - 1] >= 2  # coded bytes on both sides
            seen.add((ln, a % W))
            full_words.setdefault(ln, set()).add(b // W - -(-a // W) if b // W > -(-a // W) else 0)
            crossing += a // K["EC_ROUND_BYTES"] != (b - 1) // K["EC_ROUND_BYTES"]
        assert seen >= {(ln, o) for ln in BB.SPAN_LENS for o in range(W)}
        assert full_words[31] == {0} and full_words[32] == {0, 1} and 1 in full_words[33] and \
            full_words[64] == {1, 2} and max(full_words[1056]) == 33
        assert crossing >= 32
        order = set()
        for r in rounds:
            inw = (r["base"] + np.arange(len(r["raw"])) < r["Z"]) & (r["bits"] > 0)
            ev, od = r["raw"][0::2], r["raw"][1::2]
            both = inw[0::2] & inw[1::2]
            order |= {"raw,coded"} if (both & ev & ~od).any() else set()
            order |= {"coded,raw"} if (both & ~ev & od).any() else set()
            if len(r["raw"]) == K["EC_ROUND_BYTES"] and r["raw"].all():
                order.add("full round")
            if r["raw"].size % W == 0 and r["raw"].reshape(-1, W).all(axis=1).any():
                order.add("full word")
        assert order == {"raw,coded", "coded,raw", "full round", "full word"}


def test_lit_empties_grid():
    cases = BB.lit_empties_cases()
    for tag, shift, S, rounds in lit_views(BB.lit_empties()):
        print("lit_empties %s: %d strings, %d bytes, %d bytewise rounds" % (
            tag, len(S["R"]) - shift, int(S["off"][-1]), sum(r["bytewise"] for r in rounds)))
        off, last = S["off"], BB.LEN[S["raw"]]
        ext = {}
        for r in rounds:
            for j in np.nonzero(r["extras"])[0]:
                ext[r["base"] + int(j)] = int(r["extras"][j])
        hit = set()
        for where, kind, k, first in cases:
            f = first + shift
            assert (S["R"][f:f + k] == 0).all() and (where == "start" or S["R"][f - 1] > 0)
            if where == "start":
                assert f % 64 == 0 and S["R"][f + k] > 0
            if where == "whole":
                assert f % 64 == 0 and k % 64 == 0
            if where == "end":
                assert (f + k) % 64 == 0
            if where in ("run", "end"):  # the byte before the run, by kind
                q = int(off[f]) - 1
                if kind == "raw":
                    assert not S["H"][f - 1]
                else:
                    assert S["H"][f - 1] and last[q] == (5 if kind == "h5" else 30)
                if f % 64:  # the pad, the run's prefixes and the next string's, up to the wave's end
                    here = np.arange(f, min(f + k + 1, f - f % 64 + 64))
                    assert (off[here] == q + 1).all()
                    assert ext[q] == int(S["pad"][f - 1]) + 8 * int(S["PL"][here].sum()), (where, kind, k)
                    hit.add((kind, k, q % 2))
        assert hit >= {(kind, k, p) for kind in BB.EMPTY_BEHIND for k in range(1, 10) for p in (0, 1)}
        assert {k for w, _, k, _ in cases if w == "run"} == set(BB.EMPTY_RUNS)
        waves = {}
        for r in rounds:
            if r["first"]:
                waves[r["t0"]] = r
        assert {r["A"] & 15 for r in waves.values() if r["whole_empty"]} == {0}
        assert sum(r["whole_empty"] for r in waves.values()) >= 6  # c_end == c0
        assert {r["A"] & 15 for r in waves.values() if r["A"] == r["Z"]} >= {0, 1, 15}
        assert {(r["A"] & 15, r["at_a"]) for r in waves.values() if r["Z"] > r["A"]} >= {
            (a, k + 1) for a in (0, 1, 15) for k in (1, 3, 63)} | {(a, 1) for a in (0, 1, 15)}
        assert any(r["bytewise"] for r in rounds) and any(not r["bytewise"] for r in rounds)
    for n in BB.ALL_EMPTY_N:
        pool, off = BB.lit_all_empty(n)
        assert pool.size == 0 and len(off) == n + 1
        rounds = list(BB.literal_rounds(pool, off))
        assert len(rounds) == -(-n // 64) and all(r["whole_empty"] and r["XS"] == 8 * r["at_a"] for r in rounds)


def test_lit_pairs64_grid():
    cases = BB.lit_pairs64_cases()
    for tag, shift, S, rounds in lit_views(BB.lit_pairs64()):
        print("lit_pairs64 %s: %d strings, %d bytes, %d bytewise rounds of %d" % (
            tag, len(S["R"]) - shift, int(S["off"][-1]), sum(r["bytewise"] for r in rounds), len(rounds)))
        fo = int(S["off"][shift])
        found, short = set(), set()
        for what, T, chunk, slot, PL, first, q, (l0, pad, e, l1) in cases:
            k, q = first + shift, q + fo
            r = round_of(rounds, k - k % 64, q)
            at = q - r["base"]
            assert at % 2 == 0 and S["H"][k] and S["pad"][k] == pad and S["PL"][k + e + 1] == PL
            assert (S["R"][k + 1:k + e + 1] == 0).all() and S["H"][k + e + 1]
            j = at >> 1
            assert r["L0"][j] == l0 + pad + 8 * (e + PL) and r["pairs"][j] == r["L0"][j] + l1
            assert (r["pairs"][j] if what == "sum" else r["L0"][j]) == T
            if chunk is None:
                short.add((what, T))
                continue
            assert (r["round"], at >> 4, (at & 15) >> 1) == (1, chunk, slot) and not r["first"]
            # the only long pair of its round: the round's path is this pair's
            assert r["pairs"].max() == r["pairs"][j] and (r["pairs"] >= 61).sum() == 1
            assert r["bytewise"] == (r["pairs"][j] >= LONG_F)
            found.add((what, T, chunk, slot, PL))
        assert found == {(w, T, c, s, PL) for w, T in BB.P64_TARGETS for c in BB.P64_CHUNKS
                         for s in BB.P64_SLOTS for PL in (1, 2, 3)}
        assert short == set(BB.P64_TARGETS)
        assert {T for w, T in BB.P64_TARGETS if w == "sum"} == {LONG_F - 2, LONG_F - 1, LONG_F, 72}
        assert {T for w, T in BB.P64_TARGETS if w == "L0"} == {64, 69, 128}


def test_lit_round_edges_grid():
    cases = BB.lit_round_edges_cases()
    RB = K["EC_ROUND_BYTES"]
    assert BB.EDGE_AT == (RB - 1, RB, RB + 1, 2 * RB - 1, 2 * RB, 2 * RB + 1)
    for tag, shift, S, rounds in lit_views(BB.lit_round_edges()):
        print("lit_round_edges %s: %d strings, %d bytes" % (tag, len(S["R"]) - shift, int(S["off"][-1])))
        off = S["off"]
        align = {}
        for i, at, PL, kind, lead in cases:
            k = i + shift
            A = int(off[k - k % 64])
            assert A % 16 == 0 and int(off[k]) - A == at and S["PL"][k] == PL
            assert bool(S["H"][k]) == (kind == "huff") and S["H"][k - 1]
            r = round_of(rounds, k - k % 64, A + at - 1)  # the prefix: extras of the byte before
            assert r["round"] == (at - 1) // RB
            assert r["extras"][(at - 1) % RB] == int(S["pad"][k - 1]) + 8 * PL
            align.setdefault((at, PL, kind), set()).add(int(S["lo"][k]) % 4)
        assert len(align) == 36 and all(a == {0, 1, 2, 3} for a in align.values())


def test_lit_dense_round_grid():
    for tag, shift, S, rounds in lit_views(BB.lit_dense_round()):
        k = shift + 31
        assert len(S["R"]) - shift == 64 and S["H"][k] and S["R"][k] == BB.DENSE_FIVES + BB.DENSE_LONG
        assert (np.delete(S["R"][shift:], 31) == 1).all()
        dense = [r for r in rounds if len(r["bits"]) == K["EC_ROUND_BYTES"] and (r["bits"] == 30).all()]
        assert len(dense) == 1 and not dense[0]["first"] and not dense[0]["last"]
        assert dense[0]["nw"] >= 30 * K["EC_ROUND_BYTES"] // 32 and not dense[0]["bytewise"]
        print("lit_dense_round %s: a round of %d words, image top %d of %d" % (
            tag, dense[0]["nw"], max(r["top"] for r in rounds), RW_F))


def test_no_index_fields_literal_batch():
    """The deflater's literal batch for no_index_fields() is what
    no_index_literals() says (each literal, framed, in the oracle deflater's
    wire in that order, and nothing but representation bytes between), and
    it has a pair of more than 64 bits: the bytewise path, from the wire."""
    from oracle import hpack_oracle as HO
    assert BB.NO_INDEX == HO.NO_INDEX
    fields = BB.no_index_fields()
    wire = HO.Deflater().deflate_block(fields)
    st, got = HO.Inflater().inflate_block(wire)
    assert [(n, v) for n, v, _ in got] == [(n, v) for n, v, _ in fields]
    assert [f for _, _, f in got] == [f for _, _, f in fields]
    pool, off = BB.no_index_literals()
    lit, lo = O.emit_strings_batch(pool, off)
    at, between = 0, 0
    for i in range(len(off) - 1):
        k = wire.find(bytes(lit[lo[i]:lo[i + 1]]), at)
        assert k >= at
        between += k - at
        at = k + int(lo[i + 1] - lo[i])
    # representation bytes: 40 for a new name, 1f xx for a static index >= 15 never indexed
    assert at == len(wire) and between == 2 + 2 * len(BB.NO_INDEX_NAMES)
    rounds = list(BB.literal_rounds(pool, off))
    assert len(rounds) == 1 and rounds[0]["bytewise"]
    assert rounds[0]["pairs"].max() >= 8 * len(BB.NO_INDEX_NAMES) + 5 >= LONG_F


def test_tile_chunks():
    b = BB.lit_raw_spans()
    parts = list(BB.tile_chunks(b))
    assert all(len(o) - 1 <= 256 and int(o[0]) == 0 for _, o in parts)
    assert b"".join(bytes(p) for p, _ in parts) == bytes(b[0])
    assert sum(len(o) - 1 for _, o in parts) == len(b[1]) - 1


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
