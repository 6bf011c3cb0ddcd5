"""The deferred long codes of the 40-byte decoder's pair loop (csrc/hd_huff.hip
dd_run, `pair_def`), restated on the CPU over the product's generated tables.

A lane whose second lookup returns 0 keeps the index of the long code at its
new window and reads `long1` there as the NEXT pair's first read.  Checked:

* the index the loop computes (leading-bit count without long_index's clamps,
  the five bits after the first zero) names the true code for every window
  class of tests/test_long_codes.py whose lookup is 0, and EOS (30 ones and
  more) is never deferred;
* a staged long entry goes through the lookup entry's field extraction (put2,
  DD_ADV) unchanged: one symbol, used = L1 = the code's length, never 0, and
  the entry a lane takes after a long code of more than DD_DEFW bits carries
  no symbol and no bits;
* the warm-up's boundary pick after a last pair that held a deferred long
  code agrees with a bit-serial walk on 100,000 seeded streams.
"""
import numpy as np

from tests.test_long_codes import CODES, inc_array, inc_define, true_code

BITS = 13
DEFW = 15  # csrc/hd_huff.hip DD_DEFW
E_EOS = 0x8000
LONG1 = inc_array("hd_huff_long1", "")
LUT = inc_array("hd_huff_lut13")
N0, ROWS = inc_define("HD_HUFF_LONG1_N0"), inc_define("HD_HUFF_LONG1_ROWS")
M32 = 0xFFFFFFFF


def staged(v):
    """stage_dec_tables: a long1 word as a lookup-style entry."""
    v = int(v)
    sym, L = v & 511, v >> 9
    return (sym & 255) | (L << 8) | (1 << 13) | (L << 27) | (E_EOS if sym == 256 else 0)


def used(e):
    return e >> 27


def l1(e):
    return (e >> 8) & 31


def cnt8(e):
    return (e >> 10) & 0x18


def ffbh_i32(w):
    """v_ffbh_i32: leading bits equal to the sign bit; all equal: -1 (as u32)."""
    s = w >> 31
    x = (w ^ (M32 if s else 0)) & M32
    return M32 if x == 0 else 32 - x.bit_length()


def defer_index(w):
    """pair_def's index into long1 and its EOS test for the window w."""
    n1 = ffbh_i32(w)
    li = ((n1 - N0) * 32 + (((w << (n1 & 31)) & M32) >> 26)) & M32
    return li, n1 >= 30


def window_classes():
    for n1 in range(33):
        for b in range(32):
            if n1 >= 32:
                lo = hi = M32
            else:
                head = ((M32 << (32 - n1)) & M32) if n1 else 0
                rest = 31 - n1
                if rest >= 5:
                    lo = head | (b << (rest - 5))
                    hi = lo | ((1 << (rest - 5)) - 1)
                else:
                    if b & ((1 << (5 - rest)) - 1):
                        continue
                    lo = hi = head | (b >> (5 - rest))
            yield lo
            yield hi


def test_deferred_index_names_the_code():
    seen, eos = set(), 0
    for w in window_classes():
        if LUT[w >> (32 - BITS)] != 0:
            continue
        li, is_eos = defer_index(w)
        sym, L = true_code(w) if ffbh_i32(w) < 30 else (256, 30)
        if is_eos:
            assert sym == 256, "window %08x" % w
            eos += 1
            continue
        assert li < 32 * ROWS, "window %08x" % w
        e = staged(LONG1[li])
        assert (e & 255, used(e)) == (sym, L) and not e & E_EOS, "window %08x" % w
        seen.add(sym)
    assert eos > 0
    assert {s for s, (c, L) in enumerate(CODES) if L > BITS and s != 256} <= seen


def test_long_entry_fields_through_put2():
    for v in LONG1:
        e = staged(v)
        L = int(v) >> 9
        assert e != 0 and 14 <= L <= 30
        assert used(e) == L and l1(e) == L and cnt8(e) == 8
        assert (e >> 16) & 255 == 0 and e & 255 == (int(v) & 255)
        # more than DD_DEFW bits: the sign bit, and never a lookup entry's
        assert (used(e) > DEFW) == (L > DEFW)
    assert max(used(int(e)) for e in LUT) <= BITS <= DEFW
    assert not any(int(e) & E_EOS for e in LUT)
    assert E_EOS != 0 and used(E_EOS) == 0 and cnt8(E_EOS) == 0 and l1(E_EOS) == 0
    assert DEFW + BITS < 32  # a pair advances less than a word (DD_ADV)


def _window(bits, pos):
    """32 stream bits from pos (bits: a str of '0'/'1', padded with zeros)."""
    return int(bits[pos:pos + 32].ljust(32, "0"), 2)


def _warmup_model(bits, bstop):
    """dd_run<SYNC, LDEF 1> from bit 0 with the string end far away: the pair
    loop and the boundary pick.  Returns (entry, long code in the last pair)."""
    bp, di_long, G2 = 0, None, bstop - 1
    pb = le1 = le2 = 0
    had_long = False
    while bp <= G2:
        w = _window(bits, bp)
        e1 = staged(LONG1[di_long]) if di_long is not None else int(LUT[w >> (32 - BITS)])
        had_long = di_long is not None
        u1 = used(e1)
        e2 = int(LUT[((w << u1) & M32) >> (32 - BITS)])
        if u1 > DEFW:
            e2 = E_EOS
        pb, le1, le2 = bp, e1, e2
        bp += u1 + used(e2)
        wn = _window(bits, bp)
        li, is_eos = defer_index(wn)
        di_long = None
        if e2 == 0:
            assert not is_eos
            di_long = li
    assert bp >= bstop
    c1 = pb + (l1(le1) if le1 else 0)
    c2 = pb + used(le1)
    c3 = c2 + (l1(le2) if le2 else 0)
    c4 = c2 + (used(le2) if le2 else 0)
    entry = c1 if c1 >= bstop else c2 if c2 >= bstop else c3 if c3 >= bstop else c4
    return entry, had_long


def test_warmup_boundary_pick_vs_bit_serial_walk():
    rng = np.random.default_rng(0xDEFE44ED)
    longs = [s for s, (c, L) in enumerate(CODES) if L > BITS and s != 256]
    shorts = [s for s, (c, L) in enumerate(CODES) if L <= BITS]
    code_bits = [format(c, "0%db" % L) for c, L in CODES]
    done = 0
    while done < 100000:
        pick_long = rng.random((4096, 14)) < 0.4
        batch = np.where(pick_long, rng.choice(longs, size=(4096, 14)),
                         rng.choice(shorts, size=(4096, 14))).tolist()
        frac = rng.random((4096, 4)).tolist()
        for syms, fr in zip(batch, frac):
            if done >= 100000:
                break
            bits = "".join(code_bits[s] for s in syms)
            ends, p = [], 0
            for s in syms:
                p += CODES[s][1]
                ends.append(p)
            for f in fr:
                bstop = 1 + int(f * (ends[5] - 1))
                entry, had_long = _warmup_model(bits, bstop)
                if not had_long:
                    continue
                want = min(x for x in ends if x >= bstop)
                assert entry == want, (syms, bstop, entry, want)
                done += 1
