"""Batch builders the string-scan tests share (check_fields, http_facts_batch,
name_tokens): strings laid out in the batch layout (byte pool + uint32
offsets[n+1], optionally a length per string) with chosen bytes around them."""
import numpy as np


def padded(body, end=None):
    """A pool holding `body`, zero padded to the contract's readable size for
    strings that end at `end` (default: the body's end)."""
    end = len(body) if end is None else end
    pool = np.zeros(max((end + 15) // 16 * 16 + 16, 16), dtype=np.uint8)
    pool[:len(body)] = np.frombuffer(bytes(body), dtype=np.uint8)[:pool.size]
    return pool


def lay_out(strings, lead=b"", tail=b""):
    """`strings` back to back after `lead` (bytes before off[0]), with `tail`
    after off[n] and the pool padded by the contract (zeros to
    align_up(off[n], 16) + 16).  Returns (pool, off)."""
    off = np.zeros(len(strings) + 1, dtype=np.uint32)
    off[0] = len(lead)
    np.cumsum([len(s) for s in strings], out=off[1:])
    off[1:] += len(lead)
    body = lead + b"".join(strings) + tail
    end = int(off[-1])
    size = max((end + 15) // 16 * 16 + 16, len(body))
    pool = np.zeros(size, dtype=np.uint8)
    pool[:len(body)] = np.frombuffer(body, dtype=np.uint8)
    return pool, off


SLOT = 96  # bytes per placed string: a multiple of 16, so off & 15 is the position's


def place(items):
    """items: (context bytes, at, start, length) -- the string is
    context[start:start+length], placed at offset `at` of its own slot with the
    rest of the context around it.  Returns (pool, off, len, strings)."""
    n = len(items)
    body = bytearray(SLOT * n + SLOT)
    off = np.zeros(n + 1, dtype=np.uint32)
    ln = np.zeros(n, dtype=np.int32)
    strings = []
    for i, (ctx, at, start, length) in enumerate(items):
        base = SLOT * i + at - start  # the context's first byte
        assert base >= SLOT * i and base + len(ctx) <= SLOT * (i + 1)
        body[base:base + len(ctx)] = ctx
        off[i] = SLOT * i + at
        ln[i] = length
        strings.append(bytes(ctx[start:start + length]))
    off[n] = SLOT * n
    return padded(body, SLOT * n), off, ln, strings


def not_examined(strings, slot=16):
    """`strings` (at least 10, each shorter than `slot`) one per slot, the
    slots filled with '@', and a length per string; then the ways a string is
    not examined: a negative length (strings 1 and 3), a length one past the
    next offset (5), descending offsets (7 starts past 8, which -- from a
    lower offset up to 9's -- is examined with 7's slot as its bytes), and two
    more strings 4 GiB up whose off + len wraps 32 bits (the first refused by
    its length, the second by the closing offset below it).  Returns (pool,
    off, len, expected strings with None for one that is not examined)."""
    n = len(strings)
    assert n >= 10 and all(len(s) < slot for s in strings)
    body = bytearray(b"".join(s.ljust(slot, b"@") for s in strings))
    off = [slot * k for k in range(n)]
    ln = [len(s) for s in strings]
    want = list(strings)
    ln[1], ln[3] = -523, -502
    ln[5] = slot + 1
    off[7], off[8] = slot * 7 + 8, slot * 7
    body[slot * 7:slot * 8] = strings[8].ljust(slot, b"@")
    for i in (1, 3, 5, 7):
        want[i] = None
    off += [0xFFFFFFA0, 0xFFFFFFF0, slot * n]
    ln += [200, 4]
    want += [None, None]
    return padded(body, slot * n), np.array(off, dtype=np.uint32), np.array(ln, dtype=np.int32), want


# The walk of k_check_fields and k_http_facts takes a wave's bytes as 64
# chunks of 16 bytes a round, two rounds a loop trip: with one string of L
# bytes among 63 of 0-3 bytes, these L are the smallest at which the wave's
# chunk count crosses 64 (one round, the loop's break) and 128 (the second trip).
EXIT_LENGTHS = [1008, 1024, 1040, 2032, 2048, 2064]
EXIT_SHIFTS = [0, 1, 15]


def exit_batches(length, clean, marks, neighbour):
    """Batches of 64 strings: one of `length` bytes that starts at pool offset
    0, 1 and 15 behind strings of `neighbour` bytes, the rest (0-3 bytes of
    `neighbour`, few or many of them nonempty) behind it, so its head and
    tail chunk are partly a neighbour's.  The long string is `clean` bytes
    with one of `marks` at its first and last byte and on both sides of
    every round edge of the pool (byte 1024 k) inside it."""
    out = []
    for shift in EXIT_SHIFTS:
        front = {0: [], 1: [neighbour], 15: [neighbour * 3] * 5}[shift]
        pos = {0, length - 1}
        for edge in (1024, 2048):
            pos |= {p - shift for p in (edge - 1, edge) if 0 <= p - shift < length}
        longs = [clean * length]
        for p in sorted(pos):
            for m in marks:
                longs.append(clean * p + m + clean * (length - p - 1))
        k = 63 - len(front)
        for rest in ([neighbour * (i % 4) for i in range(k)],               # some 94 bytes behind it
                     [neighbour * (3 if i in (0, 40) else 0) for i in range(k)]):  # six
            for s in longs:
                out.append(front + [s] + rest)
    return out


def wave_chunks(strings):
    """The count of 16-byte chunks the strings of one wave span, laid out from offset 0."""
    return (sum(len(s) for s in strings) + 15) // 16
