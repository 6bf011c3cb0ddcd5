"""nghttp2_amd_hd_parse_blocks_batch and nghttp2_amd_hd_gather_literals_batch
on the GPU (csrc/hd_parse.hip), through HuffmanBatchCodec.parse_blocks and
.gather_huffman_literals.

Every batch is compared record for record with the host twin
(nghttp2_amd_hd_parse_block, itself held to the Python restatement and the
recorded reference results in tests/test_parse_blocks.py): the records with
their offsets moved to the block's place in the wire and their literal
numbers to the batch's, op_off, lit_base, block_status, totals, and the
gathered pool byte for byte.  End to end, parse -> gather -> decode_auto ->
the Python replay (tests/hd_parse_ref.py) equals inflate_blocks on fresh
inflaters: status, fields and tables.

The wire always starts at an odd offset behind poison bytes and has poison
behind its last block (0xFF: a continuation byte and an opcode with a full
prefix, so a walk that left its block would go on)."""
import numpy as np
import pytest

from nghttp2_amd import hd
from oracle import hpack_oracle as HO
from tests import hd_parse_ref as P

pytestmark = pytest.mark.gpu

LEAD, TRAIL = b"\xff" * 3, b"\xff" * 40
CANARY = 0xA5


def _t(codec, a):
    return codec.torch.from_numpy(np.array(a)).to(codec.device)  # (a writable copy)


def layout(blocks):
    """LEAD + blocks + TRAIL and the blocks' offsets."""
    off = np.cumsum([len(LEAD)] + [len(b) for b in blocks]).astype(np.uint32)
    return LEAD + b"".join(blocks) + TRAIL, off


def expected(wire, off):
    """What the batch must give, from the host twin block by block:
    (ops OP_DTYPE[], op_off, lit_base, block_status, totals[3], the Huffman
    literals' bytes in order)."""
    recs, nops, nlits, status, lits = [], [0], [0], [], []
    nbytes = 0
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        if a > b:  # not examined
            status.append(hd.NGHTTP2_ERR_HEADER_COMP)
            nops.append(nops[-1])
            nlits.append(nlits[-1])
            continue
        rv, ops = hd.parse_block(wire[a:b])
        assert rv in (0, hd.NGHTTP2_ERR_HEADER_COMP)
        ops = ops.copy()
        lit = ops["kind"] == hd.OP_LITERAL
        ops["value_off"][lit] += a
        ops["name_off"][(ops["flags"] & hd.OP_NEW_NAME) != 0] += a
        k = 0
        for r in ops:  # the twin numbers a block's literals from 0
            for f, fl, o, n in (("name_lit", hd.OP_NAME_HUFF, "name_off", "name_len"),
                                ("value_lit", hd.OP_VALUE_HUFF, "value_off", "value_len")):
                if r["flags"] & fl:
                    assert r[f] == k
                    k += 1
                    lits.append(wire[int(r[o]):int(r[o]) + int(r[n])])
                    nbytes += int(r[n])
                else:
                    assert r[f] == -1
        ops["name_lit"][ops["name_lit"] >= 0] += nlits[-1]
        ops["value_lit"][ops["value_lit"] >= 0] += nlits[-1]
        recs.append(ops)
        status.append(len(ops) if rv == 0 else rv)
        nops.append(nops[-1] + len(ops))
        nlits.append(nlits[-1] + k)
    allops = np.concatenate(recs) if recs else np.zeros(0, hd.OP_DTYPE)
    return allops, nops, nlits, status, [nops[-1], nlits[-1], nbytes], lits


def run(codec, wire, off, **caps):
    """parse + gather on the device, everything read back."""
    torch = codec.torch
    tw = _t(codec, np.frombuffer(wire, np.uint8))
    to = _t(codec, np.asarray(off, np.uint32).view(np.int32))
    pb = codec.parse_blocks(tw, to, wire_bytes=len(wire), ops_cap=caps.get("ops_cap"))
    pool, lit_off = codec.gather_huffman_literals(tw, pb, lits_cap=caps.get("lits_cap"),
                                                  pool_cap=caps.get("pool_cap"))
    torch.cuda.synchronize()
    totals = pb.totals.cpu().numpy().view(np.uint32)
    return {"pb": pb, "pool_t": pool, "lit_off_t": lit_off, "totals": [int(x) for x in totals],
            "op_off": pb.op_off.cpu().numpy().view(np.uint32), "lit_base": pb.lit_base.cpu().numpy().view(np.uint32),
            "status": pb.block_status.cpu().numpy(), "pool": pool.cpu().numpy(),
            "lit_off": lit_off.cpu().numpy().view(np.uint32)}


def check(codec, wire, off, **caps):
    ops, nops, nlits, status, totals, lits = expected(wire, off)
    got = run(codec, wire, off, **caps)
    assert got["totals"] == totals + [0]
    assert got["op_off"].tolist() == nops
    assert got["lit_base"].tolist() == nlits
    assert got["status"].tolist() == status
    rec = hd.ops_to_numpy(got["pb"].ops, len(ops))
    if rec.tobytes() != ops.tobytes():
        bad = next(j for j in range(len(ops)) if rec[j].tobytes() != ops[j].tobytes())
        block = int(np.searchsorted(np.asarray(nops), bad, side="right")) - 1
        raise AssertionError("record %d (block %d): got %r, want %r" % (bad, block, rec[bad], ops[bad]))
    lo = got["lit_off"]
    assert lo[0] == 0 and lo[:len(lits) + 1].tolist() == np.cumsum([0] + [len(s) for s in lits]).tolist()
    assert got["pool"][:int(lo[len(lits)])].tobytes() == b"".join(lits)
    got["ops"], got["nops"] = ops, nops
    return got


def mixed_blocks(n, seed):
    """n blocks: random ones (some corrupted or cut), placed edges, and empty
    blocks at the start, in the middle and at the end of a wave's 64."""
    order, rnd = P.random_blocks(seed, 6, 8, corrupt=0.25)
    small = [b for _, b in P.edge_blocks() if len(b) < 64]
    blocks = [(rnd[k % len(rnd)] if k % 3 else small[(k // 3) % len(small)]) for k in range(n)]
    for k in (0, 31, 63, 64, 127, 128, n - 1):
        if 0 <= k < n:
            blocks[k] = b""
    return blocks


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_block_counts(codec, n):
    blocks = mixed_blocks(n, 0x5EED + n)
    if n == 1:
        blocks = [P.random_blocks(7, 1, 1, corrupt=0)[1][0]]
    wire, off = layout(blocks)
    got = check(codec, wire, off)
    if n >= 63:
        assert got["totals"][1] > 20 and (got["status"] < 0).any() and (got["status"] > 0).any()


@pytest.mark.parametrize("n", [1, 64, 130])
def test_all_empty(codec, n):
    got = check(codec, b"", np.zeros(n + 1, np.uint32))
    assert got["totals"] == [0, 0, 0, 0] and got["status"].tolist() == [0] * n
    wire, off = layout([b""] * n)
    check(codec, wire, off)


def test_edges(codec):
    """Every placed integer and literal edge, one block each in one batch:
    a block that ends inside a representation is followed by a block whose
    first bytes would complete it."""
    names, blocks = zip(*P.edge_blocks())
    wire, off = layout(list(blocks))
    got = check(codec, wire, off)
    st = dict(zip(names, got["status"].tolist()))
    for w in (4, 5, 6, 7):
        for name in ("max-1", "max+0", "max+127", "max+128", "u32max"):
            assert st["int%d/%s" % (w, name)] == 1 and st["int%d/%s/mid" % (w, name)] == 3
        for name in ("u32max+1", "shift32", "shift28-carry", "cut-prefix", "cut-cont", "cut-cont4"):
            assert st["int%d/%s" % (w, name)] == hd.NGHTTP2_ERR_HEADER_COMP
            assert st["int%d/%s/mid" % (w, name)] == hd.NGHTTP2_ERR_HEADER_COMP
        k = got["nops"][names.index("int%d/u32max" % w)]
        assert got["ops"][k]["value"] == 0xFFFFFFFF
    for n in (0, 1, 15, 16, 17, 65536):
        assert st["huff-value/%d" % n] == st["huff-name/%d" % n] == st["raw-value/%d" % n] == 1
    assert st["huff-value/65537"] == st["huff-name/65537"] == st["raw-value/65537"] == hd.NGHTTP2_ERR_HEADER_COMP
    assert st["len=left"] == 2 and st["len=left+1"] == hd.NGHTTP2_ERR_HEADER_COMP
    assert st["size/first"] == st["size/middle"] == st["size/last"] == 3


def test_isolation(codec):
    good = b"\x82" + b"\x00" + P.huff_lit(5) + P.huff_lit(20) + b"\xbe"
    # a failing block between two good ones; the failing ones end inside an
    # integer or a literal that the next block's bytes would complete
    for bad in (b"\x84\xff", b"\x84\x00" + P.huff_lit(3) + b"\x85", b"\x84\x7f\x80", b"\x84\x40\x83"):
        wire, off = layout([good, bad, good, bad])
        got = check(codec, wire, off)
        assert got["status"].tolist() == [3, hd.NGHTTP2_ERR_HEADER_COMP] * 2
        assert (got["op_off"][2] - got["op_off"][1]) == 1  # the 0x84 before the failure
    # every alignment of a block's start
    for lead in range(17):
        blocks = [b"\x82" * lead, good, b"\x00" + P.huff_lit(17) + P.raw_lit(16), good]
        wire, off = layout(blocks)
        check(codec, wire, off)


def test_decreasing_offsets(codec):
    x = b"\x82\x86" + b"\x00" + P.huff_lit(4) + P.huff_lit(6)
    y = b"\x40" + P.raw_lit(3) + P.huff_lit(9) + b"\x84"
    wire = LEAD + x + y + TRAIL
    a = len(LEAD) + len(x)
    # block 1 runs backwards: not read, HEADER_COMP, nothing counted; block 2
    # starts inside block 0's last literal
    off = np.array([len(LEAD), a, a - 3, a + len(y), a + len(y)], np.uint32)
    got = check(codec, wire, off, ops_cap=2 * len(wire))
    assert got["status"][1] == hd.NGHTTP2_ERR_HEADER_COMP and got["op_off"][1] == got["op_off"][2]
    assert got["status"][0] == 3 and got["status"][3] == 0


def test_numbering(codec):
    """lit_base, name_lit and value_lit by the rule, stated by hand: blocks in
    order, representations in order, a name before its value, and the
    literals of a block that fails later are numbered too."""
    h, r = P.huff_lit, P.raw_lit
    blocks = [
        b"\x00" + h(2) + h(3) + b"\x82" + b"\x40" + r(2) + h(1),  # 0 1 | - | - 2
        b"\x82",                                                    # none
        b"\x10" + h(1) + r(1) + b"\x00" + h(1) + b"\x85",          # 3 - | fails: value cut
        b"",
        b"\x44" + h(7) + b"\x00" + r(1) + r(1) + b"\x00" + h(0) + h(0),  # - 4 | - - | 5 6
    ]
    wire, off = layout(blocks)
    got = check(codec, wire, off)
    assert got["lit_base"].tolist() == [0, 3, 3, 4, 4, 7]
    assert got["status"].tolist() == [3, 1, hd.NGHTTP2_ERR_HEADER_COMP, 0, 3]
    assert [(int(o["name_lit"]), int(o["value_lit"])) for o in got["ops"]] == \
        [(0, 1), (-1, -1), (-1, 2), (-1, -1), (3, -1), (-1, 4), (-1, -1), (5, 6)]
    assert got["totals"] == [8, 7, 2 + 3 + 1 + 1 + 7, 0]


def _raw_parse(codec, wire, off, ops, ops_cap):
    """The C call on tensors of the test's own (canaries)."""
    torch = codec.torch
    n = len(off) - 1
    tw = _t(codec, np.frombuffer(wire, np.uint8))
    to = _t(codec, np.asarray(off, np.uint32).view(np.int32))
    op_off = torch.zeros(n + 1, dtype=torch.int32, device=codec.device)
    lit_base = torch.zeros(n + 1, dtype=torch.int32, device=codec.device)
    status = torch.zeros(n, dtype=torch.int32, device=codec.device)
    totals = torch.zeros(4, dtype=torch.int32, device=codec.device)
    ws = torch.zeros(hd.parse_blocks_bound(len(wire), n)[3], dtype=torch.uint8, device=codec.device)
    rv = codec.L.nghttp2_amd_hd_parse_blocks_batch(
        hd._p(tw), hd._p(to), n, hd._p(op_off), hd._p(ops), ops_cap, hd._p(status), hd._p(lit_base),
        hd._p(totals), hd._p(ws), ws.numel(), hd._stream(None))
    assert rv == 0
    return tw, op_off, lit_base, status, totals


def _raw_gather(codec, tw, wire_bytes, ops, ops_cap, totals, lit_off, lits_cap, pool, pool_cap):
    rv = codec.L.nghttp2_amd_hd_gather_literals_batch(
        hd._p(tw), wire_bytes, hd._p(ops), ops_cap, hd._p(totals), hd._p(lit_off), lits_cap, hd._p(pool),
        pool_cap, hd._stream(None))
    assert rv == 0


def test_caps(codec):
    torch = codec.torch
    blocks = mixed_blocks(200, 0xCA95)
    wire, off = layout(blocks)
    want, nops, nlits, status, totals, lits = expected(wire, off)
    total, T, nbytes = totals
    assert total > 300 and T > 100

    def canary(nbytes_):
        return torch.full((nbytes_,), CANARY, dtype=torch.uint8, device=codec.device)

    for cap in (total, total - 1):
        ops = canary(32 * (total + 8))
        tw, op_off, lit_base, st, tot = _raw_parse(codec, wire, off, ops, cap)
        lit_off = canary(4 * (T + 9))
        pool = canary(nbytes + 64)
        _raw_gather(codec, tw, len(wire), ops, cap, tot, lit_off, T, pool, nbytes)
        torch.cuda.synchronize()
        over = cap < total
        assert tot.cpu().numpy().view(np.uint32).tolist() == totals + [hd.PARSE_OVERFLOW_OPS if over else 0]
        # the offsets and statuses are the batch's whatever the cap is
        assert op_off.cpu().numpy().tolist() == nops and st.cpu().numpy().tolist() == status
        h = ops.cpu().numpy()
        assert h[:32 * cap].tobytes() == want[:cap].tobytes()
        assert (h[32 * cap:] == CANARY).all()
        if over:  # the gather leaves an incomplete batch alone
            assert (lit_off.cpu().numpy() == CANARY).all() and (pool.cpu().numpy() == CANARY).all()
        else:
            assert pool.cpu().numpy()[:nbytes].tobytes() == b"".join(lits)
            assert (pool.cpu().numpy()[nbytes:] == CANARY).all()
            assert (lit_off.cpu().numpy()[4 * (T + 1):] == CANARY).all()

    ops = canary(32 * total)
    tw, op_off, lit_base, st, tot0 = _raw_parse(codec, wire, off, ops, total)
    for lits_cap, pool_cap, flag in ((T, nbytes - 1, hd.PARSE_OVERFLOW_POOL), (T - 1, nbytes, hd.PARSE_OVERFLOW_LITS)):
        tot = tot0.clone()
        lit_off = canary(4 * (T + 9))
        pool = canary(nbytes + 64)
        _raw_gather(codec, tw, len(wire), ops, total, tot, lit_off, lits_cap, pool, pool_cap)
        torch.cuda.synchronize()
        assert tot.cpu().numpy().view(np.uint32).tolist() == totals + [flag]
        assert (pool.cpu().numpy() == CANARY).all()
        lo = lit_off.cpu().numpy()
        if flag == hd.PARSE_OVERFLOW_POOL:  # the offsets are valid, no byte is copied
            assert lo[:4 * (T + 1)].view(np.uint32).tolist() == np.cumsum([0] + [len(s) for s in lits]).tolist()
            assert (lo[4 * (T + 1):] == CANARY).all()
        else:
            assert (lo == CANARY).all()


def test_arguments(codec):
    L = codec.L
    t = codec.torch.zeros(64, dtype=codec.torch.int32, device=codec.device)
    p = hd._p(t)
    bad = hd.NGHTTP2_ERR_INVALID_ARGUMENT
    assert L.nghttp2_amd_hd_parse_blocks_batch(None, None, 0, None, None, 0, None, None, None, None, 0, None) == 0
    full = [p, p, 1, p, p, 1, p, p, p, p, 64, None]
    for k in (0, 1, 3, 4, 6, 7, 8, 9):
        a = list(full)
        a[k] = None
        assert L.nghttp2_amd_hd_parse_blocks_batch(*a) == bad, k
    a = list(full)
    a[10] = 4
    assert L.nghttp2_amd_hd_parse_blocks_batch(*a) == bad
    gfull = [p, 16, p, 1, p, p, 1, p, 16, None]
    for k in (0, 2, 4, 5, 7):
        a = list(gfull)
        a[k] = None
        assert L.nghttp2_amd_hd_gather_literals_batch(*a) == bad, k


def _end_to_end(codec, order, blocks):
    import nghttp2_amd
    wire, off = layout(blocks)
    got = check(codec, wire, off)
    T, nbytes = got["totals"][1], got["totals"][2]
    dec = dec_off = dec_st = None
    if T:
        dst, dst_off, st = codec.decode_auto(got["pool_t"], got["lit_off_t"][:T + 1], enc_bytes=nbytes)
        codec.torch.cuda.synchronize()
        dec, dec_off, dec_st = dst.cpu().numpy(), dst_off.cpu().numpy().view(np.uint32), st.cpu().numpy()

    def get_lit(op, which):
        _, flags, _, _, no, nl, vo, vl, name_lit, value_lit = op
        o, n, huff, k = (no, nl, flags & P.NAME_HUFF, name_lit) if which == "name" else \
            (vo, vl, flags & P.VALUE_HUFF, value_lit)
        if not huff:
            return wire[o:o + n]
        if dec_st[k] < 0:
            return None
        return dec[int(dec_off[k]):int(dec_off[k]) + int(dec_st[k])].tobytes()

    nconn = max(order) + 1
    refs = [HO.Inflater() for _ in range(nconn)]
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    st, f = nghttp2_amd.inflate_blocks([infs[c] for c in order], blocks)
    ops = P.as_tuples(hd.ops_to_numpy(got["pb"].ops, got["totals"][0]))
    fails = 0
    for k, (c, blk) in enumerate(zip(order, blocks)):
        mine = ops[got["nops"][k]:got["nops"][k + 1]]
        rs, rf = P.replay(refs[c], got["status"][k] >= 0, mine, get_lit, blk[0] if blk else None)
        assert (st[k], f[k]) == (rs, rf), (k, c, blk.hex()[:120])
        fails += rs < 0
    for c in range(nconn):
        assert infs[c].dynamic_table() == [tuple(e) for e in refs[c].table], c
    return fails


def test_end_to_end_random_connections(codec):
    order, blocks = P.random_blocks(0xE2E, 12, 6, corrupt=0.12)
    fails = _end_to_end(codec, order, blocks)
    assert 0 < fails < len(blocks) // 2


def test_end_to_end_edges(codec):
    """Every placed block on a connection of its own (65536-byte Huffman
    literals among them: the long-string decoder behind the gather)."""
    blocks = [b for _, b in P.edge_blocks()]
    _end_to_end(codec, list(range(len(blocks))), blocks)
