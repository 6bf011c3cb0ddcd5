"""The representation layer of an HPACK header block, restated in Python for
the tests of nghttp2_amd_hd_parse_block and nghttp2_amd_hd_parse_blocks_batch
(tests/test_parse_blocks.py, tests/test_parse_blocks_gpu.py):

- parse(): the cut of a block into representations, written from
  lib/nghttp2_hd.c:1942-1985 (opcode dispatch) and :882-945 (decode_length)
  with the record of include/nghttp2_amd_hd.h;
- replay(): the records of one block against an oracle.hpack_oracle.Inflater's
  table (the table logic is the oracle's own: _get, _add, _shrink and its
  state), so parse + replay can be held against a whole inflate;
- the placed blocks both test files use: integers at every prefix width,
  literal lengths at the edges, cuts in the middle of a representation."""
import numpy as np

from oracle import hpack_oracle as HO

SIZE, INDEXED, LITERAL = 0, 1, 2
INDEX_REQUIRED, NO_INDEX, NEW_NAME, NAME_HUFF, VALUE_HUFF = 0x01, 0x02, 0x04, 0x08, 0x10
MAX_NV = 65536
U32 = 0xFFFFFFFF
FIELDS = ("kind", "flags", "reserved", "value", "name_off", "name_len", "value_off", "value_len",
          "name_lit", "value_lit")


class _Cut(Exception):
    pass


def parse(block, base=0, lit0=0):
    """(ok, ops): ops are tuples in FIELDS order, offsets plus base, Huffman
    literals numbered from lit0; ok is False when the bytes after the last
    completed representation are none."""
    b = bytes(block)
    pos = 0
    ops = []
    nlit = lit0

    def integer(prefix):
        nonlocal pos
        if pos >= len(b):
            raise _Cut()
        k = (1 << prefix) - 1
        n = b[pos] & k
        pos += 1
        if n < k:
            return n
        shift = 0
        while True:
            if pos >= len(b):
                raise _Cut()
            c = b[pos]
            pos += 1
            add = c & 0x7F
            if shift >= 32 or add > (U32 >> shift):
                raise _Cut()
            add <<= shift
            if add > U32 - n:
                raise _Cut()
            n += add
            if not c & 0x80:
                return n
            shift += 7

    def literal():
        nonlocal pos
        if pos >= len(b):
            raise _Cut()
        huff = bool(b[pos] & 0x80)
        n = integer(7)
        if n > MAX_NV or len(b) - pos < n:
            raise _Cut()
        at = pos
        pos += n
        return at, n, huff

    try:
        while pos < len(b):
            c = b[pos]
            if (c & 0xE0) == 0x20:
                ops.append((SIZE, 0, 0, integer(5), 0, 0, 0, 0, -1, -1))
                continue
            if c & 0x80:
                ops.append((INDEXED, 0, 0, integer(7), 0, 0, 0, 0, -1, -1))
                continue
            flags = (INDEX_REQUIRED if c & 0x40 else 0) | (NO_INDEX if (c & 0xF0) == 0x10 else 0)
            value = 0
            no, nl, name_lit, value_lit = 0, 0, -1, -1
            k = nlit
            if c in (0x40, 0x00, 0x10):
                flags |= NEW_NAME
                pos += 1
                at, nl, huff = literal()
                no = base + at
                if huff:
                    flags |= NAME_HUFF
                    name_lit = k
                    k += 1
            else:
                value = integer(6 if c & 0x40 else 4)
            at, vl, huff = literal()
            if huff:
                flags |= VALUE_HUFF
                value_lit = k
                k += 1
            nlit = k
            ops.append((LITERAL, flags, 0, value, no, nl, base + at, vl, name_lit, value_lit))
    except _Cut:
        return False, ops
    return True, ops


def as_tuples(ops):
    """A numpy OP_DTYPE array as parse()'s tuples."""
    return [tuple(int(r[f]) for f in FIELDS) for r in ops]


def wire_literal(wire):
    """get_lit for replay(): a literal's bytes from the wire, a Huffman one
    through the C oracle (None: the decode fails, -523)."""
    from oracle import oracle as O

    def get(op, which):
        kind, flags, _, _, no, nl, vo, vl, _, _ = op
        off, n, huff = (no, nl, flags & NAME_HUFF) if which == "name" else (vo, vl, flags & VALUE_HUFF)
        s = bytes(wire[off:off + n])
        if not huff:
            return s
        rv, out, ctx = O.decode(s, final=1)
        return None if rv < 0 or O.failure_state(ctx) else out
    return get


def replay(inf, ok, ops, get_lit, first_byte):
    """One block's records (parse's or the product's, as tuples) against
    inf, an oracle.hpack_oracle.Inflater: (status, fields) as its
    inflate_block returns them, and its state left as inflate_block leaves
    it.  get_lit(op, "name" | "value") gives a literal's bytes, None when its
    Huffman decode fails; first_byte is the block's first byte, None for an
    empty block (which state a failed block leaves depends on it)."""
    fields = []
    if inf.bad:
        return HO.HEADER_COMP, fields
    good, head = True, True
    for op in ops:
        kind, flags, _, value = op[:4]
        if inf.expect_size and kind != SIZE:
            good = False
            break
        if kind == SIZE:
            if not head or value > min(inf.min_max, inf.settings_max):
                good = False
                break
            inf.min_max = U32
            inf.expect_size = False
            inf.max = value
            inf._shrink()
            continue
        head = False
        if kind == INDEXED or not flags & NEW_NAME:
            if value == 0 or value > len(inf.table) + 61:
                good = False
                break
        if kind == INDEXED:
            n, v = inf._get(value - 1)
            fields.append((n, v, 0))
            continue
        name = get_lit(op, "name") if flags & NEW_NAME else inf._get(value - 1)[0]
        val = get_lit(op, "value") if name is not None else None
        if name is None or val is None:
            good = False
            break
        if flags & INDEX_REQUIRED:
            inf._add(name, val)
        fields.append((name, val, HO.NO_INDEX if flags & NO_INDEX else 0))
    if good and (not ok or inf.expect_size):
        good = False
    if not good:
        first_is_size = first_byte is not None and (first_byte & 0xE0) == 0x20
        inf.bad = True
        inf.mid_block = not (inf.expect_size and not first_is_size)
        return HO.HEADER_COMP, fields
    return len(fields), fields


# ---------------------------------------------------------------------------
# placed blocks
# ---------------------------------------------------------------------------
def enc_int(v, prefix, first=0):
    """The shortest RFC 7541 5.1 form of v (any size) under `first`'s bits."""
    k = (1 << prefix) - 1
    if v < k:
        return bytes([first | v])
    out = [first | k]
    v -= k
    while v >= 128:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


# prefix width -> (opcode bits, what completes the representation)
WIDTHS = {4: (0x00, b"\x01a"), 5: (0x20, b""), 6: (0x40, b"\x01a"), 7: (0x80, b"")}

# 'X' has the 8-bit code 0xfc (RFC 7541 Appendix B), so a run of 0xfc is a
# valid Huffman literal of the same number of bytes
HX = 0xFC


def huff_lit(n):
    return enc_int(n, 7, 0x80) + bytes([HX]) * n


def raw_lit(n, c=b"r"):
    return enc_int(n, 7, 0x00) + c * n


def integer_blocks():
    """Every integer case at every prefix width, each a block of its own:
    (name, block)."""
    out = []
    for w, (first, tail) in sorted(WIDTHS.items()):
        k = (1 << w) - 1
        cases = {
            "max-1": bytes([first | (k - 1)]),
            "max+0": bytes([first | k, 0x00]),
            "max+127": bytes([first | k, 0x7F]),
            "max+128": bytes([first | k, 0x80, 0x01]),
            "u32max": enc_int(U32, w, first),
            "u32max+1": enc_int(U32 + 1, w, first),
            "shift32": bytes([first | k, 0x80, 0x80, 0x80, 0x80, 0x80, 0x01]),
            "shift28-carry": bytes([first | k, 0x80, 0x80, 0x80, 0x80, 0x10]),
            "cut-prefix": bytes([first | k]),
            "cut-cont": bytes([first | k, 0x80]),
            "cut-cont4": bytes([first | k, 0xFF, 0xFF, 0xFF, 0xFF]),
        }
        for name, head in cases.items():
            if name.startswith("cut"):  # the block ends inside the integer
                out.append(("int%d/%s" % (w, name), head))
                out.append(("int%d/%s/mid" % (w, name), b"\x82" + head))
                continue
            out.append(("int%d/%s" % (w, name), head + tail))
            # behind a good representation, and with one behind it
            out.append(("int%d/%s/mid" % (w, name), b"\x82" + head + tail + b"\x84"))
    return out


def literal_blocks():
    out = []
    for n in (0, 1, 15, 16, 17, 65536, 65537):
        out.append(("huff-value/%d" % n, b"\x00" + raw_lit(3, b"n") + huff_lit(n)))
        out.append(("huff-name/%d" % n, b"\x40" + huff_lit(n) + raw_lit(2, b"v")))
        out.append(("raw-value/%d" % n, b"\x10" + huff_lit(2) + raw_lit(n)))
    good = b"\x00" + huff_lit(4) + huff_lit(9)
    out += [
        ("len=left", b"\x82" + good),
        ("len=left+1", b"\x82" + good[:-1]),
        ("len=left+1/raw", b"\x41" + raw_lit(5)[:-1]),
        ("mid-opcode/newname", b"\x82\x00"),
        ("mid-opcode/name-len", b"\x40\x01"),
        ("mid-opcode/no-value", b"\x00" + huff_lit(3)),
        ("mid-opcode/indname-no-value", b"\x44"),
        ("size/first", enc_int(4096, 5, 0x20) + b"\x82" + good),
        ("size/middle", b"\x82" + enc_int(100, 5, 0x20) + good),
        ("size/last", good + b"\x82" + enc_int(0, 5, 0x20)),
        ("size/twice", b"\x20\x3f\xe1\x1f\x82"),
        ("indexed/0", b"\x80"),
        ("indexed/run", bytes(range(0x81, 0xBE))),
    ]
    return out


def edge_blocks():
    return integer_blocks() + literal_blocks()


def random_blocks(seed, nconn, nblk, corrupt=0.15):
    """Blocks of nconn connections, nblk each, from tests/test_inflate.py's
    random encoder (Huffman and raw literals, every representation), some
    corrupted or cut: (connection of block k, blocks)."""
    from tests.test_inflate import _encode_block, _random_fields
    rng = np.random.Generator(np.random.PCG64(seed))
    enc_tables = [[] for _ in range(nconn)]
    order, blocks = [], []
    for _ in range(nblk):
        for c in rng.permutation(nconn):
            fields = _random_fields(rng, int(rng.integers(1, 12)))
            blk = _encode_block(rng, enc_tables[c], fields, 4096)
            r = rng.random()
            if r < corrupt / 3:
                blk = blk[:max(0, len(blk) - int(rng.integers(1, 6)))]
            elif r < corrupt:
                at = int(rng.integers(0, len(blk)))
                blk = blk[:at] + bytes([blk[at] ^ int(rng.integers(1, 256))]) + blk[at + 1:]
            order.append(int(c))
            blocks.append(blk)
    return order, blocks
