"""GPU parity on the boundary grids of tests/boundary_batches.py: codewords
across 40-, 64- and 96-byte piece boundaries at every bit position, strings
ending at exact bit distances around them, tasks with exact item counts and
round byte sums, pack rounds on both sides of the 256-word store threshold,
code pairs on both sides of 32 bits, encode_count, and pools whose first
offset is not 0 -- every entry point against the oracle, bit-exact (status,
{fstate, flags}, offsets, every written byte).  tests/test_boundary_batches.py
proves on the CPU that the grids hit what they claim.
"""
import numpy as np
import pytest

from oracle import hpack_oracle as H
from oracle import oracle as O
from tests import boundary_batches as BB
from tests.test_parity_gpu import (auto_decode_check, check_decode, check_dense_layout, check_emit,
                                   check_roundtrip, pad16, to_dev)

pytestmark = pytest.mark.gpu

PICKS = (None, "items64", "pieces40")


def dense_check(codec, dev, enc, eoff, tag, pick):
    """decode_auto: status, context and bytes (auto_decode_check), and the
    dense layout with every byte the reference writes (check_dense_layout)."""
    import torch
    auto_decode_check(codec, dev, enc, eoff, tag, pick=pick)
    n, E = len(eoff) - 1, int(eoff[-1])
    dst = torch.zeros(codec.decode_bound(E, n), dtype=torch.uint8, device=dev)
    dst, do, st = codec.decode_auto(to_dev(pad16(enc, E), dev), to_dev(eoff, dev), enc_bytes=E,
                                    dst=dst, pick=pick)
    torch.cuda.synchronize()
    check_dense_layout(dst.cpu().numpy(), do.cpu().numpy().view(np.uint32), enc, eoff, tag)


def fsm_check(codec, dev, src, so, ref, tag):
    """decode_fsm into the oracle's slots: status, context and whole slots."""
    import torch
    rd, rdo, rst, rfs, rfl = ref
    dst = torch.zeros(int(rdo[-1]) + 16, dtype=torch.uint8, device=dev)
    st, fs, fl = codec.decode_fsm(src, so, to_dev(rdo, dev), dst)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), rst), tag + ": fsm status"
    assert np.array_equal(fs.cpu().numpy().view(np.uint16), rfs), tag + ": fsm fstate"
    assert np.array_equal(fl.cpu().numpy(), rfl), tag + ": fsm flags"
    assert np.array_equal(dst.cpu().numpy()[:int(rdo[-1])], rd[:int(rdo[-1])]), tag + ": fsm bytes"


def decode_family(codec, dev, b, tag):
    for j in (0, 1, 33):
        enc, eoff = BB.shifted(b, j)
        t = "%s shifted %d" % (tag, j)
        check_decode(codec, dev, enc, eoff, t)
        for pick in PICKS:
            dense_check(codec, dev, enc, eoff, "%s %s" % (t, pick), pick)
        fsm_check(codec, dev, to_dev(pad16(enc, eoff[-1]), dev), to_dev(eoff, dev),
                  O.decode_batch(enc, eoff), t)


def test_straddle(codec, dev):
    decode_family(codec, dev, BB.straddle(), "straddle")


def test_ends(codec, dev):
    b = BB.ends()
    decode_family(codec, dev, b, "ends")
    # the altered paddings fail as the reference says (-523), but for 011111
    rst = O.decode_batch(*b)[2]
    for (E, p, v), st in zip(BB.ends_cases(), rst):
        assert (st >= 0 if BB.ends_accepts(p, v) else st == -523), (E, p, v, st)


@pytest.mark.parametrize("last", [1, 31, 32, 33])
def test_tasks(codec, dev, last):
    decode_family(codec, dev, BB.tasks(last), "tasks(last=%d)" % last)


@pytest.mark.parametrize("family", ["round_words", "long_pairs"])
def test_encode_family(codec, dev, family):
    b = getattr(BB, family)()
    for tag, (pool, off) in ((family, b), (family + " filled", BB.with_fill(b))):
        check_roundtrip(codec, dev, pool, off, tag)
        check_emit(codec, dev, pool, off, tag)


def count_check(codec, dev, pool, off, tag, stream=None):
    import torch
    n = len(off) - 1
    want = np.array([O.encode_count(bytes(pool[int(off[i]):int(off[i + 1])])) for i in range(n)],
                    dtype=np.int64)
    src, so = to_dev(pad16(pool, off[-1]), dev), to_dev(off, dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the inputs were copied there)
    got = codec.encode_count(src, so, stream=stream)
    (stream or torch.cuda.current_stream()).synchronize()
    got = got.cpu().numpy().view(np.uint32).astype(np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: encode_count differs at %s (gpu %s, ref %s)" % (
        tag, bad[:5], got[bad[:5]], want[bad[:5]])


def test_encode_count(codec, dev):
    """nghttp2_amd_hd_huff_encode_count_batch (k_enc_count with byte counts
    out and no tile sums) against the oracle's per-string encode_count."""
    import torch
    from nghttp2_amd import workloads as W
    cases = []
    for family in ("round_words", "long_pairs"):
        b = getattr(BB, family)()
        cases += [(family, b), (family + " filled", BB.with_fill(b))]
    for n in (1, 64, 257, 3000):
        cases.append(("allbytes n=%d" % n, W.gen_all_bytes(n, seed=70 + n)))
    cases.append(("all-empty", W._pool_from_lengths(np.zeros(300, np.int64), np.zeros(0, np.uint8))))
    for tag, (pool, off) in cases:
        count_check(codec, dev, pool, off, tag)
    side = torch.cuda.Stream(dev)
    for tag, (pool, off) in cases[2:6]:
        count_check(codec, dev, pool, off, tag + " (side stream)", stream=side)


@pytest.mark.parametrize("fill", BB.OFFSET_FILL)
@pytest.mark.parametrize("a0", BB.OFFSET_A0)
def test_first_offset(codec, dev, a0, fill):
    """src_off[0] = a0 > 0, the pool buffer passed as it is (exactly the
    documented padding, 0xFF or random bytes around the strings): every entry
    point equals the oracle on the rebased copy."""
    import torch
    for n in BB.OFFSET_N:
        tag = "a0=%d n=%d %s" % (a0, n, fill)
        buf, off, rpool, roff = BB.offset_pool(a0, n, fill)
        raw = int(roff[-1])
        src, so = torch.from_numpy(buf).to(dev), to_dev(off, dev)
        renc, reoff = O.encode_batch(rpool, roff) if n else (np.zeros(0, np.uint8), np.zeros(1, np.uint32))
        E = int(reoff[-1])
        # encode, encode_count, emit_strings
        enc, eo = codec.encode(src, so, raw_bytes=raw)
        eo = eo.cpu().numpy().view(np.uint32)
        assert np.array_equal(eo, reoff), tag + ": encoded offsets"
        assert np.array_equal(enc.cpu().numpy()[:E], renc[:E]), tag + ": encoded bytes"
        cnt = codec.encode_count(src, so).cpu().numpy().view(np.uint32)
        assert np.array_equal(cnt, np.diff(reoff.astype(np.int64))), tag + ": encode_count"
        lit, lo = codec.emit_strings(src, so, raw_bytes=raw)
        rlit, rlo = O.emit_strings_batch(rpool, roff) if n else (np.zeros(0, np.uint8), np.zeros(1, np.uint32))
        lo = lo.cpu().numpy().view(np.uint32)
        assert np.array_equal(lo, rlo), tag + ": literal offsets"
        assert np.array_equal(lit.cpu().numpy()[:int(rlo[-1])], rlit[:int(rlo[-1])]), tag + ": literals"
        # name tokens and hashes
        tok, h = codec.name_tokens(src, so)
        et, eh = H.name_tokens([bytes(rpool[int(roff[i]):int(roff[i + 1])]) for i in range(n)])
        assert np.array_equal(tok.cpu().numpy(), np.array(et, dtype=np.int32)), tag + ": tokens"
        assert np.array_equal(h.cpu().numpy().view(np.uint32), np.array(eh, dtype=np.uint32)), tag + ": hashes"
        # the decoders: the oracle's encoding of the same strings, placed the same way
        dbuf, doff = BB.place(renc, reoff, a0, fill)
        dsrc, dso = torch.from_numpy(dbuf).to(dev), to_dev(doff, dev)
        ref = O.decode_batch(renc, reoff)
        rd, rdo, rst, rfs, rfl = ref
        slots = codec.decode_slots(dso).cpu().numpy().view(np.uint32)
        assert np.array_equal(slots, rdo), tag + ": decode_slots"
        dst = torch.zeros(int(rdo[-1]) + 16, dtype=torch.uint8, device=dev)
        _, _, st, fs, fl = codec.decode(dsrc, dso, dst_off=to_dev(rdo, dev), dst=dst, want_ctx=True)
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), rst), tag + ": decode status"
        assert np.array_equal(fs.cpu().numpy().view(np.uint16), rfs), tag + ": decode fstate"
        assert np.array_equal(fl.cpu().numpy(), rfl), tag + ": decode flags"
        assert np.array_equal(dst.cpu().numpy()[:int(rdo[-1])], rd[:int(rdo[-1])]), tag + ": decode bytes"
        assert np.array_equal(rst, np.diff(roff.astype(np.int64)))
        for pick in PICKS:
            dst = torch.zeros(codec.decode_bound(E, n), dtype=torch.uint8, device=dev)
            dst, do, st, fs, fl = codec.decode_auto(dsrc, dso, enc_bytes=E, dst=dst, want_ctx=True,
                                                    pick=pick)
            torch.cuda.synchronize()
            t = "%s %s" % (tag, pick)
            assert np.array_equal(st.cpu().numpy(), rst), t + ": auto status"
            assert np.array_equal(fs.cpu().numpy().view(np.uint16), rfs), t + ": auto fstate"
            assert np.array_equal(fl.cpu().numpy(), rfl), t + ": auto flags"
            do = do.cpu().numpy().view(np.uint32)
            if n == 0:
                assert do[0] == 0, t
            # (the layout rule with x = off - off[0], and every decoded byte)
            check_dense_layout(dst.cpu().numpy(), do, dbuf, doff, t)
        fsm_check(codec, dev, dsrc, dso, ref, tag)
