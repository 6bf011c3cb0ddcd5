"""nghttp2_amd_hd_name_tokens_len_batch (k_name_tokens<true>) on the GPU: name
tokens and FNV-1a hashes of strings given by (pool, off, len), bit-exact
against the oracle's lookup_token / name_hash (oracle/hpack_oracle.py, pinned
to the reference by tests/golden/name_tokens.json) on exactly the len bytes:
every token name and its near misses at every alignment and across the 16- and
32-byte chunk edges with hostile bytes around them, batch sizes around a wave
and a workgroup, strings that are not examined, the hash-free form and its
early exit, and the real output of decode_batch_auto."""
import numpy as np
import pytest

import nghttp2_amd
from nghttp2_amd import workloads as W
from oracle import hpack_oracle as H
from oracle import oracle as O
from tests.string_batches import padded, place

pytestmark = pytest.mark.gpu

NAMES = sorted(W.TOKEN_NAMES)
INVALID, NONE = nghttp2_amd.TOKEN_INVALID, nghttp2_amd.TOKEN_NONE


def near_misses(name):
    return [name[:-1] + bytes([name[-1] ^ 1]), name[:-1], name + b"x", name.upper()]


def tokens(codec, dev, pool, off, ln=None, want_hash=True):
    import torch
    t_pool = torch.from_numpy(pool).to(dev)
    t_off = torch.from_numpy(np.asarray(off, dtype=np.uint32).view(np.int32)).to(dev)
    t_len = None if ln is None else torch.from_numpy(np.asarray(ln, dtype=np.int32)).to(dev)
    r = codec.name_tokens(t_pool, t_off, len=t_len, want_hash=want_hash)
    if not want_hash:
        return r.cpu().numpy()
    return r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32)


def expect(codec, dev, pool, off, ln, strings):
    """Token and hash of every string against the oracle on its own bytes, and
    the same tokens from the hash-free form."""
    tok, h = tokens(codec, dev, pool, off, ln)
    wt, wh = H.name_tokens(strings)
    bad = [(i, strings[i][:40], int(tok[i]), wt[i], hex(int(h[i])), hex(wh[i]))
           for i in range(len(strings)) if tok[i] != wt[i] or h[i] != wh[i]]
    assert not bad, bad[:6]
    assert np.array_equal(tokens(codec, dev, pool, off, ln, want_hash=False), np.array(wt, dtype=np.int32))


def positions(length):
    """off & 15 in {0, 1, 3, 15}, and offsets that put the string across a
    16-byte and a 32-byte chunk edge."""
    half = max(1, length // 2)
    return sorted({0, 1, 3, 15, 16 - half, 32 - half, 31})


def test_position_grid(codec, dev):
    rng = np.random.Generator(np.random.PCG64(1))
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz-:", dtype=np.uint8)
    strs = list(NAMES)
    for nm in NAMES:
        strs += near_misses(nm)
    for length in (0, 1, 27, 28, 31, 32, 33):
        strs.append(alphabet[rng.integers(0, alphabet.size, size=length)].tobytes())
        strs.append(b"access-control-allow-origin"[:length].ljust(length, b"n"))
    items = []
    for s in strs:
        for at in positions(len(s)):
            # name characters on both sides, so a byte too many on either
            # side is a different name, not an obvious non-name
            fill = alphabet[rng.integers(0, alphabet.size, size=32)].tobytes()
            lead = fill[:min(16, at)]
            items.append((lead + s + fill[16:], at, len(lead), len(s)))
    expect(codec, dev, *place(items))


def test_filler_that_continues_a_token_name(codec, dev):
    """The bytes around the string spell a longer (or another) token name:
    every proper prefix and suffix of every token name inside that name, a
    token name inside another one's context, at three alignments."""
    items = []
    for at in (0, 3, 15):
        items.append((b"content-length", at, 0, 7))       # "content", "-length" behind it
        items.append((b"viary", at, 0, 3))                # "via" followed by "ry"
        items.append((b"::status", at + 1, 1, 7))         # ":status" preceded by ':'
        items.append((b"content-length", at + 8, 8, 6))   # "length"
        items.append((b"accept-encoding", at, 0, 6))      # "accept" is a token name itself
        items.append((b"if-none-match", at + 8, 8, 5))    # "match"
        items.append((b"proxy-connection", at + 6, 6, 10))  # "connection" inside proxy-connection
        items.append((b"keep-alive", at + 5, 5, 0))       # empty, inside a name
        for nm in NAMES:
            for k in range(1, len(nm)):
                items.append((nm, at, 0, k))
                items.append((nm, at + k, k, len(nm) - k))
    pool, off, ln, strings = place(items)
    assert strings[0] == b"content" and strings[1] == b"via" and strings[2] == b":status"
    expect(codec, dev, pool, off, ln, strings)
    tok, _ = tokens(codec, dev, pool, off, ln)
    assert tok[:3].tolist() == [NONE, 59, 7] and tok[4] == 18 and tok[6] == 62


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_workgroup_and_wave_edges(codec, dev, n):
    rng = np.random.Generator(np.random.PCG64(n))
    cands = NAMES + [m for nm in NAMES[:20] for m in near_misses(nm)] + [b"", b"x" * 28, b"y" * 70]
    items = []
    for k in range(n):
        s = cands[int(rng.integers(0, len(cands)))]
        ctx = b"-" + s + b"-control"
        items.append((ctx, int(rng.integers(1, 17)), 1, len(s)))
    expect(codec, dev, *place(items))


def test_strings_that_are_not_examined(codec, dev):
    """A negative length (a failed decode's status), a length one past the next
    offset, descending offsets and an off + len that wraps 32 bits: token -2,
    hash 0, nothing read; the strings on both sides stay exact."""
    names = [b"cookie", b"etag", b"te", b":path", b"via", b"host", b"date", b"age", b"link", b"from", b"vary",
             b"range"]
    body = b"".join(nm.ljust(16, b"-") for nm in names)
    off = [16 * k for k in range(len(names))]
    ln = [len(nm) for nm in names]
    want = [H.lookup_token(nm) for nm in names]
    wh = [H.name_hash(nm) for nm in names]

    def bad(i):
        want[i], wh[i] = INVALID, 0
    ln[1] = -523
    bad(1)
    ln[3] = -502
    bad(3)
    ln[5] = 17  # off[5] + 17 = off[6] + 1
    bad(5)
    # descending offsets: string 7 starts past string 8; string 8 (from a
    # lower offset up to string 9's) is examined
    off[7] = 16 * 7 + 8
    off[8] = 16 * 7
    bad(7)
    body = bytearray(body)
    body[16 * 7:16 * 8] = b"link".ljust(16, b"-")
    want[8], wh[8] = H.lookup_token(b"link"), H.name_hash(b"link")
    # off + len wraps 32 bits: the last two offsets lie 4 GiB up, where no
    # string is examined -- the first by its length, the second by the
    # closing offset below it
    off += [0xFFFFFFA0, 0xFFFFFFF0, 16 * len(names)]
    ln += [200, 4]
    want += [INVALID, INVALID]
    wh += [0, 0]
    pool = padded(body, 16 * len(names))
    tok, h = tokens(codec, dev, pool, off, ln)
    assert tok.tolist() == want
    assert h.tolist() == wh
    assert tokens(codec, dev, pool, off, ln, want_hash=False).tolist() == want
    assert want.count(INVALID) == 6 and want[0] == 31 and want[2] == 61 and want[4] == 59 and want[6] == 32


def test_hash_free_form_and_its_early_exit(codec, dev):
    rng = np.random.Generator(np.random.PCG64(5))
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz-", dtype=np.uint8)

    def rnd(k):
        return alphabet[rng.integers(0, alphabet.size, size=k)].tobytes()
    strs = []
    for k in range(200):
        r = k % 10
        strs.append(NAMES[k % len(NAMES)] if r < 6 else rnd(28) if r == 6 else rnd(100) if r == 7 else
                    rnd(70000) if k in (58, 129) else rnd(int(rng.integers(0, 28))))
    pool, off = W.names_to_pool(strs)
    pool = padded(pool[:int(off[-1])].tobytes())
    tok, h = tokens(codec, dev, pool, off)
    wt, wh = H.name_tokens(strs)
    assert tok.tolist() == wt and h.tolist() == wh
    assert tokens(codec, dev, pool, off, want_hash=False).tolist() == wt
    ln = np.diff(off.astype(np.int64)).astype(np.int32)
    assert tokens(codec, dev, pool, off, ln, want_hash=False).tolist() == wt
    # the early exit: strings longer than every token name, lying mostly or
    # wholly past the end of a pool that is sized for the short strings in
    # front of them.  The hash-free form reads none of their bytes: -1 each.
    short = [NAMES[k % len(NAMES)] for k in range(70)] + [b"x" * 27, b"access-control-allow-origin"]
    body = b"".join(short)
    end = len(body)
    off = np.zeros(len(short) + 5, dtype=np.uint32)
    np.cumsum([len(s) for s in short], out=off[1:len(short) + 1])
    longs = [28, 100, 70000, 70000]  # from `end` on: the first starts inside the pool's padding
    off[len(short) + 1:] = end + np.cumsum(longs)
    ln = np.array([len(s) for s in short] + longs, dtype=np.int32)
    got = tokens(codec, dev, padded(body, end), off, ln, want_hash=False)
    assert got.tolist() == [H.lookup_token(s) for s in short] + [NONE] * 4
    assert got[-5] == 19 and got[-6] == NONE


def test_on_decode_output_with_task_gaps_and_failed_strings(codec, dev):
    import torch
    pool, off = W.gen_names(300, seed=11, long_frac=0.0)
    enc, enc_off = O.encode_batch(pool, off)
    enc = enc.copy()
    for i in (3, 64, 130, 299):
        while enc_off[i + 1] == enc_off[i]:  # (an empty name has no byte to corrupt)
            i -= 1
        enc[int(enc_off[i + 1]) - 1] = 0x00  # a last byte that is no EOS prefix
    E = int(enc_off[-1])
    epool = np.zeros((E + 15) // 16 * 16 + 16, dtype=np.uint8)
    epool[:E] = enc[:E]
    rdst, rdoff, rst, _, _ = O.decode_batch(epool[:E + 16], enc_off)
    dst, dst_off, status = codec.decode_auto(torch.from_numpy(epool).to(dev),
                                             torch.from_numpy(enc_off.view(np.int32)).to(dev), enc_bytes=E)
    tok, h = codec.name_tokens(dst, dst_off, len=status)
    only = codec.name_tokens(dst, dst_off, len=status, want_hash=False)
    st = status.cpu().numpy()
    do = dst_off.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(st, rst)
    assert np.any(do[1:-1] != do[:-2] + np.maximum(st[:-1], 0)), "no task gap in this batch"
    assert 3 <= int((rst < 0).sum()) <= 4
    dec = [None if rst[i] < 0 else rdst[int(rdoff[i]):int(rdoff[i]) + int(rst[i])].tobytes() for i in range(300)]
    want = [INVALID if s is None else H.lookup_token(s) for s in dec]
    wh = [0 if s is None else H.name_hash(s) for s in dec]
    assert tok.cpu().numpy().tolist() == want
    assert h.cpu().numpy().view(np.uint32).tolist() == wh
    assert only.cpu().numpy().tolist() == want
    assert sum(t >= 0 for t in want) > 100


def test_without_len_the_new_symbol_equals_the_old(codec, dev):
    import ctypes
    import torch
    pool, off = W.gen_names(5000, seed=3, long_frac=0.1)
    n = len(off) - 1
    t_pool = torch.from_numpy(padded(pool[:int(off[-1])].tobytes())).to(dev)
    t_off = torch.from_numpy(off.view(np.int32)).to(dev)
    tok0, h0 = codec.name_tokens(t_pool, t_off)
    tok1 = torch.empty(n, dtype=torch.int32, device=dev)
    h1 = torch.empty(n, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    rv = codec.L.nghttp2_amd_hd_name_tokens_len_batch(vp(t_pool.data_ptr()), vp(t_off.data_ptr()), None, n,
                                                      vp(tok1.data_ptr()), vp(h1.data_ptr()),
                                                      vp(torch.cuda.current_stream().cuda_stream))
    assert rv == 0
    torch.cuda.synchronize()
    assert torch.equal(tok0, tok1) and torch.equal(h0, h1)
    assert int((tok0 >= 0).sum()) > 1000


def test_null_arguments(codec, dev):
    import ctypes
    import torch
    L = nghttp2_amd.lib()
    f = L.nghttp2_amd_hd_name_tokens_len_batch
    assert f(None, None, None, 0, None, None, None) == 0
    assert f(None, None, None, 3, None, None, None) == nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(args[0], args[1], None, 1, args[2], None, None) == nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT
    # the old call still refuses a NULL hash
    assert L.nghttp2_amd_hd_name_tokens_batch(p, p, 1, p, None, None) == nghttp2_amd.NGHTTP2_ERR_INVALID_ARGUMENT
