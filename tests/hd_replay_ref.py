"""What tests/test_replay_host.py and tests/test_replay_gpu.py share: blocks
laid side by side with the host parse's records, their Huffman literals
decoded through the C oracle into the decode's layout (dst, dst_off, status),
the host twin run over them, and the blocks built for each rule of the
replay."""
import numpy as np

from nghttp2_amd import hd
from tests import hd_parse_ref as P


def batch(blocks, lead=b""):
    """lead + blocks side by side, parsed on the host block by block: (wire,
    block_off, op_off, ops, block_status) with the records' offsets positions
    in wire and their literal numbers the batch's."""
    off = np.cumsum([len(lead)] + [len(b) for b in blocks]).astype(np.uint32)
    recs, op_off, status, nlit = [], [0], [], 0
    for a, blk in zip(off.tolist(), blocks):
        rv, ops = hd.parse_block(blk)
        assert rv in (0, hd.NGHTTP2_ERR_HEADER_COMP)
        ops = ops.copy()
        ops["value_off"][ops["kind"] == hd.OP_LITERAL] += a
        ops["name_off"][(ops["flags"] & hd.OP_NEW_NAME) != 0] += a
        k = int((ops["name_lit"] >= 0).sum() + (ops["value_lit"] >= 0).sum())
        ops["name_lit"][ops["name_lit"] >= 0] += nlit
        ops["value_lit"][ops["value_lit"] >= 0] += nlit
        nlit += k
        recs.append(ops)
        status.append(len(ops) if rv == 0 else rv)
        op_off.append(op_off[-1] + len(ops))
    ops = np.concatenate(recs) if recs else np.zeros(0, hd.OP_DTYPE)
    return lead + b"".join(blocks), off, np.array(op_off, np.uint32), ops, np.array(status, np.int32)


def oracle_decode(wire, ops):
    """The Huffman literals of ops decoded by the C oracle, in the decode's
    output layout: (dst uint8, dst_off uint32[T], status int32[T]); a literal
    that fails has status -523."""
    from oracle import oracle as O
    lits = {}
    for r in ops:
        for f, o, n in (("name_lit", "name_off", "name_len"), ("value_lit", "value_off", "value_len")):
            if r[f] >= 0:
                lits[int(r[f])] = wire[int(r[o]):int(r[o]) + int(r[n])]
    assert sorted(lits) == list(range(len(lits)))
    out, dst_off, status = [], [], []
    at = 0
    for k in range(len(lits)):
        rv, dec, ctx = O.decode(lits[k], final=1)
        bad = rv < 0 or O.failure_state(ctx)
        dec = b"" if bad else bytes(dec)
        dst_off.append(at)
        status.append(hd.NGHTTP2_ERR_HEADER_COMP if bad else len(dec))
        out.append(dec + b"\xee" * 3)  # (the decode's strings are not back to back either)
        at += len(dec) + 3
    return np.frombuffer(b"".join(out), np.uint8), np.array(dst_off, np.uint32), np.array(status, np.int32)


def host_blocks(inf, blocks, **caps):
    """blocks, in order, on inf (an hd.HostReplayInflater) in ONE call:
    (status[i], fields[i], out_totals)."""
    if not blocks:
        return [], [], None
    wire, off, op_off, ops, st = batch(blocks)
    dst, dst_off, status = oracle_decode(wire, ops)
    totals, nva, arena, nv_off, out = inf.replay(wire, off, op_off, ops, st, dst, dst_off, status, **caps)
    s, f = hd.replay_fields(nva, arena, nv_off, out)
    return s, f, totals


def host_state(inf):
    return inf.table(), inf.table_size(), inf.table_max(), inf.flags()


def ins(name, value):
    """a literal with incremental indexing and a new name, both raw"""
    return b"\x40" + P.enc_int(len(name), 7) + name + P.enc_int(len(value), 7) + value


def size(v):
    return P.enc_int(v, 5, 0x20)


BAD_HUFF = P.enc_int(4, 7, 0x80) + b"\xff" * 4  # EOS inside the string

# name -> the steps of one connection: a block, or ("change", value)
RULES = {
    "size/first": [size(100) + b"\x82"],
    "size/second": [size(100) + size(50) + b"\x82", ins(b"a", b"b")],
    "size/after-field": [b"\x82" + size(100), b"\x82"],
    "size/above-settings": [size(4097) + b"\x82", b"\x82"],
    "size/at-settings": [size(4096) + b"\x82"],
    "size/above-min-after-shrink": [ins(b"k", b"v"), ("change", 100), ("change", 4096), size(200) + b"\x82",
                                    ("change", 50)],
    "size/at-min-after-shrink": [ins(b"k", b"v"), ("change", 100), ("change", 4096), size(100) + size(4096) + b"\xbe",
                                 ("change", 50)],
    "expect/missing": [("change", 100), b"\x82", ("change", 200), b"\x82"],        # mid_block clear
    "expect/missing-empty": [("change", 100), b"", ("change", 200), size(10)],
    "expect/leading-size-fails": [("change", 100), size(200) + b"\x82", ("change", 300)],  # mid_block set
    "expect/met": [("change", 100), size(80) + b"\x82", ("change", 4096), b"\x82", size(4096) + b"\x82"],
    "index/0": [b"\x82\x80\x84", b"\x82"],
    "index/name-0": [b"\x40" + P.raw_lit(1), b"\x82"],
    "index/last-and-past": [ins(b"abc", b"def") + b"\xbe" + b"\x7e" + P.raw_lit(2) + b"\xbf" + b"\xc0", b"\xbe"],
    "index/past": [ins(b"abc", b"def") + b"\xbe\xbf", b"\x82"],
    "index/name-past": [ins(b"abc", b"def") + b"\x0f\x30" + P.raw_lit(2)],  # name index 63
    "entry/larger-than-max": [size(64) + ins(b"a", b"b") + ins(b"n" * 20, b"v" * 20) + b"\x82", b"\xbe", b"\x82"],
    "entry/exactly-max": [size(64) + ins(b"a", b"b") + ins(b"n" * 16, b"v" * 16) + b"\xbe", b"\xbe\xbf"],
    "evict/own-name": [size(80) + ins(b"abcdefgh", b"12345678") + b"\x7e" + P.raw_lit(20, b"w") + b"\xbe",
                       b"\xbe\x7e" + P.raw_lit(21, b"x") + b"\xbe", b"\xbe\xbf"],
    "evict/inside-one-block": [size(100) + ins(b"first", b"1") + ins(b"second", b"2") + ins(b"third", b"3") + b"\xbe\xbf",
                               b"\xbe\xbf\xc0"],
    "huff/bad-name-good-value": [b"\x82\x40" + BAD_HUFF + P.huff_lit(3) + b"\x84", b"\x82"],
    "huff/good-name-bad-value": [b"\x40" + P.huff_lit(3) + BAD_HUFF, b"\x82"],
    "huff/indexed-name-bad-value": [b"\x41" + BAD_HUFF, b"\x82"],
    "huff/insert-and-reference": [b"\x40" + P.huff_lit(5) + P.huff_lit(7) + b"\xbe", b"\xbe\x7e" + P.huff_lit(0)],
    "parse/cut-after-fields": [b"\x82\x84\x40\x05ab", b"\x82"],
    "no-index": [b"\x10" + P.raw_lit(2, b"n") + P.raw_lit(2, b"v") + b"\x1f\x00" + P.huff_lit(2)],
    "empty": [b"", b"\x82", b""],
}
