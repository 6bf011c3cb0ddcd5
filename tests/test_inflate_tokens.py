"""Name tokens from the inflate front-end (nghttp2_amd_hd_inflate_blocks_fields:
nv_tokens[k] = lookup_token of field k's name, as nghttp2_hd_inflate_hd_nv sets
nv.token, lib/nghttp2_hd.c:1340, :1811) on blocks whose literals are all raw:
such a batch makes no GPU call, so these run without one.  The expected token
is always the oracle's lookup_token (oracle/hpack_oracle.py, pinned to the
reference by tests/golden/name_tokens.json) of the emitted name; the fields
and statuses are checked against the oracle's inflater on the way."""
import random

import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd.workloads import TOKEN_NAMES
from oracle import hpack_oracle as HO

HEADER_COMP = nghttp2_amd.NGHTTP2_ERR_HEADER_COMP


def _int(v, prefix, first):
    k = (1 << prefix) - 1
    if v < k:
        return bytes([first | v])
    out = [first | k]
    v -= k
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _lit(s):
    return _int(len(s), 7, 0) + s


def indexed(i):
    return _int(i, 7, 0x80)


def new_name(n, v, first=0x40):
    """A literal with a new name: first = 0x40 (indexed), 0x00 (not), 0x10 (never)."""
    return bytes([first]) + _lit(n) + _lit(v)


def idx_name(i, v, first=0x40):
    return _int(i, 6 if first == 0x40 else 4, first) + _lit(v)


def near_misses(name):
    out = [name[:-1] + bytes([name[-1] ^ 1]), name[:-1], name + b"x", name.upper()]
    return [n for n in out if n != name]


NAMES = sorted(TOKEN_NAMES)
MISSES = sorted({m for n in NAMES for m in near_misses(n)} - set(NAMES))


def run(conns, blocks, infs=None, nconn=None, **kw):
    """inflate_blocks(tokens=True) of blocks[i] on connection conns[i]; checks
    the statuses, fields and tokens against the oracle and returns them (and the
    inflaters and the oracle's, to go on with)."""
    nconn = max(conns) + 1 if nconn is None else nconn
    if infs is None:
        infs = ([nghttp2_amd.HpackInflater() for _ in range(nconn)], [HO.Inflater() for _ in range(nconn)])
    st, f, tk = nghttp2_amd.inflate_blocks([infs[0][c] for c in conns], blocks, tokens=True, **kw)
    for k, (c, b) in enumerate(zip(conns, blocks)):
        assert (st[k], f[k]) == infs[1][c].inflate_block(b), (k, c)
    flat = [x for fb in f for x in fb]
    assert tk.dtype == np.int32 and tk.shape == (len(flat),)
    want = [HO.lookup_token(n) for n, _, _ in flat]
    assert tk.tolist() == want, [(k, flat[k][0], int(tk[k]), want[k]) for k in range(len(flat))
                                 if tk[k] != want[k]][:8]
    return st, f, tk, infs


# one connection: the direct sink; two, interleaved: the per-block sinks
SHAPES = {"direct": lambda n: [0] * n, "grouped": lambda n: [k & 1 for k in range(n)]}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_static_index(shape):
    blocks = [b"".join(indexed(i) for i in range(1, 62)), b"".join(indexed(i) for i in range(61, 0, -1))]
    st, f, tk, _ = run(SHAPES[shape](2), blocks)
    assert st == [61, 61]
    assert tk[:61].tolist() == [HO.lookup_token(n) for n, _ in HO.STATIC]
    assert tk[1] == 1 and tk[2] == 1 and tk[7] == 7 and tk[13] == 7  # the FIRST static index of a name


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("first", [0x00, 0x10, 0x40])
def test_static_names_with_literal_values(shape, first):
    blocks = [b"".join(idx_name(i, b"v%d" % i, first) for i in range(1, 32)),
              b"".join(idx_name(i, b"", first) for i in range(32, 62))]
    st, _, _, _ = run(SHAPES[shape](2), blocks)
    assert st == [31, 30]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("first", [0x00, 0x40])
def test_raw_new_names(shape, first):
    names = NAMES + MISSES + [b"", b"x" * 27, b"x" * 28, b"y" * 300]
    assert len(NAMES) == 59
    blocks = [b"".join(new_name(n, b"v", first) for n in names[k::4]) for k in range(4)]
    _, _, tk, _ = run(SHAPES[shape](4), blocks)
    assert sorted(t for t in tk.tolist() if t >= 0) == sorted(HO.lookup_token(n) for n in NAMES)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dynamic_entries_after_insertion(shape):
    ins = [b"cookie", b"x-custom", b":path", b"Cookie", b"te", b""]
    conns = SHAPES[shape](4)
    blocks = [b"".join(new_name(n, b"value-%d" % k) for k, n in enumerate(ins)) for _ in range(2)]
    # both connections: every entry as an indexed field, then as an indexed name
    # with and without a further insertion (which shifts the indices)
    refs = b"".join(indexed(62 + k) for k in range(len(ins))) + \
        b"".join(idx_name(62 + k, b"w", 0x00) for k in range(len(ins))) + \
        b"".join(idx_name(62 + 2 * k, b"z") for k in range(len(ins)))
    blocks += [refs, refs]
    st, _, _, infs = run(conns, blocks)
    assert min(st) > 0
    # and in a later call, from the tables as that call left them
    run([0], [b"".join(indexed(62 + k) for k in range(12))], infs=infs)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_entries_from_an_untokened_call(shape):
    """An entry that a plain (or checked) call inserted carries no token: it is
    looked up at its first tokened reference, as an indexed field or a name."""
    conns = SHAPES[shape](2)
    infs = ([nghttp2_amd.HpackInflater() for _ in range(2)], [HO.Inflater() for _ in range(2)])
    ins = [new_name(b"content-length", b"12") + new_name(b"x-a", b"1") + idx_name(31, b"text/plain"),
           new_name(b"via", b"1.1 a") + new_name(b"viary", b"") + new_name(b"priority", b"u=1")]
    st, f = nghttp2_amd.inflate_blocks([infs[0][c] for c in conns], ins)
    for c, b, s_, f_ in zip(conns, ins, st, f):
        assert (s_, f_) == infs[1][c].inflate_block(b)
    seen = [indexed(62), indexed(63)]  # a checked call fills the masks, not the tokens
    st, f, m = nghttp2_amd.inflate_blocks([infs[0][c] for c in conns], seen, checks=True)
    for c, b, s_, f_ in zip(conns, seen, st, f):
        assert (s_, f_) == infs[1][c].inflate_block(b)
    refs = [indexed(62) + idx_name(63, b"q", 0x00) + idx_name(64, b"r") + indexed(65),
            indexed(63) + indexed(64) + idx_name(62, b"s", 0x10)]
    run(conns, refs, infs=infs)
    run(conns, refs, infs=infs)  # now from the descriptors


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_eviction_and_reinsertion_of_a_name(shape):
    """A table of 120 bytes holds two of these entries: every insertion from
    the third on evicts, and the same names come back under new indices."""
    conns = SHAPES[shape](6)
    size = _int(120, 5, 0x20)
    blocks = []
    for k in range(6):
        b = size if k < 2 else b""
        for j in range(5):
            b += new_name([b"cookie", b"x-id", b"etag"][(k + j) % 3], b"0123456789" * 2)
            b += indexed(62) + indexed(63 if j else 62)
        blocks.append(b)
    _, _, _, infs = run(conns, blocks)
    assert all(r.size <= 120 and len(r.table) == 2 for r in infs[1][:max(conns) + 1])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_insertion_that_evicts_its_own_names_entry(shape):
    """An indexed-name literal whose insertion evicts the entry the name came
    from (the table holds one entry of this size): the field and the new
    entry keep the name's token."""
    conns = SHAPES[shape](4)
    val = b"v" * 30
    one = _int(80, 5, 0x20) + new_name(b"set-cookie", val) + idx_name(62, b"w" * 30) + indexed(62) + \
        idx_name(62, b"u" * 30) + indexed(62)
    two = idx_name(62, b"t" * 30) + indexed(62) + new_name(b"Set-Cookie", val) + idx_name(62, val) + indexed(62)
    st, f, tk, infs = run(conns, [one, one, two, two])
    assert len(infs[1][0].table) == 1
    assert tk[:5].tolist() == [54] * 5


def _mixed_block(rng, ndyn):
    """Raw-literal blocks over the token names and their near misses: indexed
    static and dynamic references, new and indexed names, with and without
    insertion, size updates at the block start."""
    b = b""
    if rng.random() < 0.15:  # (ndyn: entries the table surely holds, and its limit)
        ndyn[1] = rng.choice([0, 4096])
        b += _int(ndyn[1], 5, 0x20)
        ndyn[0] = 0 if ndyn[1] == 0 else ndyn[0]
    for _ in range(rng.randint(0, 10)):
        r = rng.random()
        if r < 0.2:
            b += indexed(rng.randint(1, 61))
        elif r < 0.45 and ndyn[0]:
            k = 62 + rng.randint(0, ndyn[0] - 1)
            first = rng.choice([0x00, 0x10, 0x40])
            b += indexed(k) if rng.random() < 0.5 else idx_name(k, b"d" * rng.randint(0, 20), first)
        elif r < 0.8:
            n = rng.choice(NAMES) if rng.random() < 0.6 else rng.choice(MISSES)
            first = rng.choice([0x00, 0x40, 0x40])
            b += new_name(n, bytes(rng.randint(32, 126) for _ in range(rng.randint(0, 60))), first)
            if first == 0x40 and ndyn[1]:
                ndyn[0] = min(ndyn[0] + 1, 6)
        else:
            b += idx_name(rng.randint(1, 61), b"x" * rng.randint(0, 40), 0x00)
    return b


def _mixed_batch(seed, nconn):
    rng = random.Random(seed)
    ndyn = [[0, 4096] for _ in range(nconn)]
    conns = [rng.randrange(nconn) for _ in range(rng.randint(20, 40))]
    return conns, [_mixed_block(rng, ndyn[c]) for c in conns]


@pytest.mark.parametrize("nconn", [1, 5])
@pytest.mark.parametrize("cap", [3, 12, 40])
def test_cut_and_retry_gives_the_uncut_tokens(nconn, cap):
    """Buffers small enough that the batch is cut (snapshot, restore, re-apply)
    and resubmitted: the same tokens, masks, fields and tables as one uncut call."""
    for seed in range(4):
        conns, blocks = _mixed_batch(100 * cap + seed, nconn)
        st0, f0, tk0, whole = run(conns, blocks, nconn=nconn)
        st1, f1, tk1, cut = run(conns, blocks, nconn=nconn, nva_cap=cap, arena_cap=cap * 30, retry=True)
        assert (st0, f0) == (st1, f1)
        assert np.array_equal(tk0, tk1)
        for a, b in zip(whole[0], cut[0]):
            assert a.dynamic_table() == b.dynamic_table()
        # the cut itself, without the retry: the blocks before it with their tokens
        infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
        st2, f2, tk2 = nghttp2_amd.inflate_blocks([infs[c] for c in conns], blocks, tokens=True, nva_cap=cap,
                                                  arena_cap=cap * 30, retry=False)
        done = [k for k in range(len(blocks)) if st2[k] != nghttp2_amd.NGHTTP2_ERR_BUFFER_ERROR]
        assert done == list(range(len(done))) and f2[:len(done)] == f0[:len(done)]
        assert len(done) < len(blocks), "the batch was not cut"
        nf = sum(len(x) for x in f2)
        assert tk2.shape == (nf,) and np.array_equal(tk2, tk0[:nf])
        # tables and descriptors after the cut serve a tokened call
        st3, f3, tk3 = nghttp2_amd.inflate_blocks([infs[c] for c in conns[len(done):]], blocks[len(done):],
                                                  tokens=True)
        assert (st3, f3) == (st0[len(done):], f0[len(done):]) and np.array_equal(tk3, tk0[nf:])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_header_comp_keeps_the_tokens_before_the_error(shape):
    conns = SHAPES[shape](4)
    bad = indexed(2) + new_name(b"upgrade", b"h2c") + indexed(7) + indexed(0) + indexed(3)
    good = indexed(4) + new_name(b"keep-alive", b"1")
    st, f, tk, _ = run(conns, [good, bad, good, good])
    if shape == "grouped":  # connection 1 fails at its first block, connection 0 goes on
        assert st == [2, HEADER_COMP, 2, HEADER_COMP]
        assert tk.tolist() == [3, 63, 1, 65, 5, 3, 63]
    else:
        assert st == [2, HEADER_COMP, HEADER_COMP, HEADER_COMP]
        assert tk.tolist() == [3, 63, 1, 65, 5]
    # a Huffman-free block cut off inside a literal: the fields parsed before it
    st, f, tk, _ = run([0], [indexed(5) + new_name(b"te", b"trailers") + b"\x40\x05ab"])
    assert st == [HEADER_COMP] and tk.tolist() == [3, 61]


@pytest.mark.parametrize("nconn", [1, 5])
def test_without_tokens_nothing_changes(nconn):
    conns, blocks = _mixed_batch(7, nconn)

    def fresh():
        infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
        return [infs[c] for c in conns]
    plain = nghttp2_amd.inflate_blocks(fresh(), blocks)
    explicit = nghttp2_amd.inflate_blocks(fresh(), blocks, checks=False, tokens=False)
    assert len(plain) == 2 and plain == explicit
    st_c, f_c, m_c = nghttp2_amd.inflate_blocks(fresh(), blocks, checks=True)
    st_t, f_t, tk = nghttp2_amd.inflate_blocks(fresh(), blocks, tokens=True)
    both = nghttp2_amd.inflate_blocks(fresh(), blocks, checks=True, tokens=True)
    assert len(both) == 4
    assert (st_c, f_c) == plain and (st_t, f_t) == plain and both[:2] == plain
    assert both[2].dtype == np.uint8 and np.array_equal(both[2], m_c)
    assert both[3].dtype == np.int32 and np.array_equal(both[3], tk)


def test_c_call_argument_forms():
    """nv_tokens without nv_checks, an empty batch, and the first *nva_used
    entries only: the rest of nv_tokens is not written."""
    import ctypes
    from nghttp2_amd import hd
    L = hd._inflate_lib()
    vp = ctypes.c_void_p
    nv_used, ar_used = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.nghttp2_amd_hd_inflate_blocks_fields(None, 0, None, None, None, 0, ctypes.byref(nv_used), None, 0,
                                                  ctypes.byref(ar_used), None, None, None, None) == 0
    assert (nv_used.value, ar_used.value) == (0, 0)
    inf = nghttp2_amd.HpackInflater()
    block = np.frombuffer(indexed(2) + new_name(b"etag", b"x"), dtype=np.uint8)
    ptrs = np.array([block.ctypes.data], dtype=np.uint64)
    lens = np.array([block.size], dtype=np.uint64)
    infs = np.array([inf.p.value], dtype=np.uint64)
    nva = np.empty(8, dtype=hd._NV_DTYPE)
    arena = np.empty(256, dtype=np.uint8)
    st = np.empty(1, dtype=np.int32)
    tk = np.full(8, 12345, dtype=np.int32)
    rv = L.nghttp2_amd_hd_inflate_blocks_fields(vp(infs.ctypes.data), 1, vp(ptrs.ctypes.data), vp(lens.ctypes.data),
                                                vp(nva.ctypes.data), 8, ctypes.byref(nv_used), vp(arena.ctypes.data),
                                                256, ctypes.byref(ar_used), vp(st.ctypes.data), None,
                                                vp(tk.ctypes.data), None)
    assert rv == 0 and st[0] == 2 and nv_used.value == 2
    assert tk.tolist() == [1, 33] + [12345] * 6
