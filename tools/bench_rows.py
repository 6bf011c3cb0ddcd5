#!/usr/bin/env python3
"""Throughput of the SURVEY.md 8(f) rows built beside the hot path:

  emit     nghttp2_amd_hd_emit_strings_batch: HPACK string literals
           (emit_string, lib/nghttp2_hd.c:1001-1044) for the config-2 batch,
           device-resident; GB/s of raw in + literals out.
  inflate  nghttp2_amd_hd_inflate_blocks: header blocks of many connections
           (host memory), Huffman literals decoded in one GPU batch per
           call; wire MB/s and fields/s, with the split between host passes
           and the GPU round trip.
  names    nghttp2_amd_hd_name_tokens_batch: lookup_token + name_hash
           (lib/nghttp2_hd.c:137, :536) over 1M header names, device-resident;
           algorithmic bytes sum(L) + 12 N (name bytes + offset in, token +
           hash out) over the kernel time (HIP events on its stream).
  check    nghttp2_amd_hd_check_fields_batch: nghttp2_check_* masks of 1M
           mixed values and of the config-2 pseudo-headers, device-resident,
           alternated with the encode count (k_enc_count<false>: the same
           bytes, one LDS lookup per byte) on the same pools; best of the
           steps by HIP events, GB/s of R + 5 N bytes.
  inflate_checked  nghttp2_amd_hd_inflate_blocks_checked against
           nghttp2_amd_hd_inflate_blocks on the 2,048-block batch, alternated:
           what the check launch and the mask bytes in the copy back cost.
  names_len  nghttp2_amd_hd_name_tokens_len_batch against
           nghttp2_amd_hd_name_tokens_batch on the 1M names, alternated call by
           call (the len form with a hash: the same walk plus one load per
           lane), and its hash-free form on 1M mixed values: what the early
           exit leaves of a pool of strings that are mostly no names.
  inflate_fields  nghttp2_amd_hd_inflate_blocks_fields with both arrays
           against nghttp2_amd_hd_inflate_blocks_checked on the 2,048-block
           batch, alternated; and with NGHTTP2_AMD_OTHER_LIB naming another
           build of the library (the parent commit's), its _checked against
           this build's in the same process: the existing call must not have
           become slower.
  http_facts  nghttp2_amd_hd_http_facts_batch against
           nghttp2_amd_hd_check_fields_batch on the check row's two pools,
           alternated call by call: the same walk, loads and ballots, plus
           the string lane's own reads; and on 4,096 numbers of 16 KiB of zeros.
  inflate_http  nghttp2_amd_hd_inflate_blocks_http against
           nghttp2_amd_hd_inflate_blocks_fields with both arrays on the
           and the plain nghttp2_amd_hd_inflate_blocks on the 2,048-block
           batch, alternated; with NGHTTP2_AMD_OTHER_LIB, that build's three
           calls against this build's in the same process.

  parse    nghttp2_amd_hd_parse_blocks_batch + nghttp2_amd_hd_gather_literals_batch
           on the 2,048-block batch: the six launches between two HIP events
           on device-resident wire, and again with the wire's H2D copy in
           front, alternated; beside them, in the same process, the host
           phases they restate (`parse blocks`, `number+copy`) from
           nghttp2_amd_hd_inflate_blocks' own trace (NGHTTP2_AMD_TRACE=1, which
           the row sets: run it alone, or first).  Several runs; the spread
           of the runs' medians is reported.

  dev_deflate  nghttp2_amd_hd_dev_deflate_blocks on the 2,048-list batch with
           resident fields against nghttp2_amd_hd_deflate_blocks on the same
           lists from host memory, alternated, fresh contexts each run; two
           batches: lists that repeat (indexed: the search) and all new
           values (insertions and evictions).  dev_deflate_repeat and
           dev_deflate_new run one batch (for a kernel trace of it).

With NGHTTP2_AMD_OTHER_LIB the names, check, names_len and http_facts rows
also make the same call from that build, alternated call by call with this
build's on the same resident pools (the `other_*` figures).

Prints one JSON object.  Not the bench.py contract (that is the hot path
itself); the numbers go to DESIGN.md."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def other_codec(dev):
    """A codec whose string-scan calls (name_tokens, check_fields,
    http_facts_batch) go to the build NGHTTP2_AMD_OTHER_LIB names; None without it."""
    path = os.environ.get("NGHTTP2_AMD_OTHER_LIB")
    if not path:
        return None
    import ctypes
    import nghttp2_amd
    c = nghttp2_amd.HuffmanBatchCodec(dev)
    P = ctypes.CDLL(path)
    for f in ("nghttp2_amd_hd_name_tokens_batch", "nghttp2_amd_hd_name_tokens_len_batch",
              "nghttp2_amd_hd_check_fields_batch", "nghttp2_amd_hd_http_facts_batch"):
        getattr(P, f).argtypes = getattr(c.L, f).argtypes
    c.L = P
    return c


def alternate(calls, steps):
    """`calls` (label -> function) alternated call by call on the current
    stream, each call between two HIP events: best and median in us per label."""
    import torch
    s = torch.cuda.current_stream()
    for _ in range(5):
        for c in calls.values():
            c()
    ev = {k: [] for k in calls}
    for _ in range(steps):
        for k, c in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            c()
            b.record(s)
            ev[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, v in ev.items():
        t = [a.elapsed_time(b) * 1e3 for a, b in v]
        out[k + "_us_best"] = round(min(t), 2)
        out[k + "_us_median"] = round(float(np.median(t)), 2)
    return out


def bench_emit(steps=20, cfg=2):
    """emit_strings on the config-2 (pseudo-headers) or config-3 (mixed
    values) batch: wall time per batch, and the launch pair's time by HIP
    events on its stream; roofline bytes R + F + 12 N (raw in, literals out,
    offsets) per batch against 8 TB/s."""
    import torch
    import nghttp2_amd
    from nghttp2_amd import workloads as W
    from oracle import oracle as O
    dev = torch.device("cuda:0")
    pool, off = W.gen_pseudo_headers(1 << 20) if cfg == 2 else W.gen_mixed_values(1 << 20)
    raw = int(off[-1])
    n = len(off) - 1
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    src = torch.from_numpy(pool).to(dev)
    so = torch.from_numpy(off.view(np.int32)).to(dev)
    dst, do = codec.emit_strings(src, so, raw_bytes=raw)
    torch.cuda.synchronize()
    # parity on a sample of the batch
    k = 20000
    rd, rdo = O.emit_strings_batch(pool, off[:k + 1])
    assert np.array_equal(do[:k + 1].cpu().numpy().view(np.uint32), rdo)
    assert np.array_equal(dst[:int(rdo[-1])].cpu().numpy(), rd)
    for _ in range(3):
        codec.emit_strings(src, so, raw_bytes=raw, dst=dst, dst_off=do)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        codec.emit_strings(src, so, raw_bytes=raw, dst=dst, dst_off=do)
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / steps
    s = torch.cuda.current_stream()
    ev = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        codec.emit_strings(src, so, raw_bytes=raw, dst=dst, dst_off=do)
        b.record(s)
        ev.append((a, b))
    torch.cuda.synchronize()
    tk = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e-3
    F = int(do[-1].item())
    alg = raw + F + 12 * n
    return {"config": cfg, "strings": n, "raw_bytes": raw, "literal_bytes": F,
            "ms_per_batch": round(t * 1e3, 4), "GBps_raw_plus_out": round((raw + F) / t / 1e9, 1),
            "roofline": {"kernels": "k_enc_count<true> + k_encode<true>", "launch_pair_ms": round(tk * 1e3, 4),
                         "alg_bytes": alg, "achieved_GBps": round(alg / tk / 1e9, 1),
                         "frac_of_8TBps": round(alg / tk / 8e12, 4)}}


def bench_names(steps=50, long_frac=0.02):
    import torch
    import nghttp2_amd
    from nghttp2_amd import workloads as W
    from oracle import hpack_oracle as H
    dev = torch.device("cuda:0")
    pool, off = W.gen_names(1 << 20, long_frac=long_frac)
    n, raw = len(off) - 1, int(off[-1])
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    names = torch.from_numpy(pool).to(dev)
    no = torch.from_numpy(off.view(np.int32)).to(dev)
    tok, h = codec.name_tokens(names, no)
    torch.cuda.synchronize()
    k = 20000  # parity on a sample
    et, eh = H.name_tokens([pool[off[i]:off[i + 1]].tobytes() for i in range(k)])
    assert np.array_equal(tok[:k].cpu().numpy(), np.array(et, np.int32))
    assert np.array_equal(h[:k].cpu().numpy().view(np.uint32), np.array(eh, np.uint32))
    for _ in range(5):
        codec.name_tokens(names, no, token=tok, hash=h)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(steps):
        codec.name_tokens(names, no, token=tok, hash=h)
    e1.record(s)
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / 1e3 / steps
    B = raw + 12 * n
    other = other_codec(dev)
    ab = alternate({"this": lambda: codec.name_tokens(names, no, token=tok, hash=h),
                    "other": lambda: other.name_tokens(names, no, token=tok, hash=h)}, steps) if other else {}
    return {"names": n, "name_bytes": raw, "us_per_batch": round(t * 1e6, 2),
            "GBps_algorithmic": round(B / t / 1e9, 1), "hbm_frac": round(B / t / 8.0e12, 4),
            "Gnames_per_s": round(n / t / 1e9, 3), "long_wave_frac": long_frac, **ab}


def bench_check(steps=30):
    """check_fields against encode_count, alternated call by call on the same
    device-resident pool in one process; each call between two HIP events,
    the best of the steps of each."""
    import torch
    import nghttp2_amd
    from nghttp2_amd import workloads as W
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import field_checks_ref as R
    dev = torch.device("cuda:0")
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    other = other_codec(dev)
    n = 1 << 20
    out = {}
    for label, (pool, off) in (("mixed_1M", W.gen_mixed_range(W.mixed_lengths(n), 0, n, threads=8)),
                               ("pseudo_1M", W.gen_pseudo_headers(n))):
        raw = int(off[-1])
        src = torch.from_numpy(pool).to(dev)
        so = torch.from_numpy(off.view(np.int32)).to(dev)
        mask = codec.check_fields(src, so)
        cnt = codec.encode_count(src, so)
        torch.cuda.synchronize()
        k = 5000  # parity on a sample
        got = mask[:k].cpu().numpy()
        assert all(int(got[i]) == R.mask(pool[off[i]:off[i + 1]].tobytes()) for i in range(k))
        s = torch.cuda.current_stream()
        for _ in range(5):
            codec.check_fields(src, so, mask=mask)
            codec.encode_count(src, so, enc_len=cnt)
        ev = []
        for _ in range(steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(s)
            codec.check_fields(src, so, mask=mask)
            e[1].record(s)
            e[2].record(s)
            codec.encode_count(src, so, enc_len=cnt)
            e[3].record(s)
            ev.append(e)
        torch.cuda.synchronize()
        tc = min(e[0].elapsed_time(e[1]) for e in ev) * 1e-3
        te = min(e[2].elapsed_time(e[3]) for e in ev) * 1e-3
        B = raw + 5 * n
        out[label] = {"strings": n, "raw_bytes": raw, "check_us": round(tc * 1e6, 2),
                      "encode_count_us": round(te * 1e6, 2), "check_over_count": round(tc / te, 3),
                      "check_GBps_R_plus_5N": round(B / tc / 1e9, 1),
                      "count_GBps_R_plus_5N": round(B / te / 1e9, 1),
                      "check_us_median": round(float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e3, 2),
                      "encode_count_us_median": round(float(np.median([e[2].elapsed_time(e[3]) for e in ev])) * 1e3, 2)}
        if other:
            out[label].update(alternate({"this_check": lambda: codec.check_fields(src, so, mask=mask),
                                         "other_check": lambda: other.check_fields(src, so, mask=mask)}, steps))
    return out


def bench_names_len(steps=30):
    """The three forms alternated call by call on device-resident pools, each
    call between two HIP events, best and median of the steps."""
    import torch
    import nghttp2_amd
    from nghttp2_amd import workloads as W
    from oracle import hpack_oracle as H
    dev = torch.device("cuda:0")
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    n = 1 << 20
    other = other_codec(dev)

    def timed(calls):
        return alternate(calls, steps)

    pool, off = W.gen_names(n)
    raw = int(off[-1])
    names = torch.from_numpy(pool).to(dev)
    no = torch.from_numpy(off.view(np.int32)).to(dev)
    ln = torch.from_numpy(np.diff(off.astype(np.int64)).astype(np.int32)).to(dev)
    tok, h = codec.name_tokens(names, no)
    tok2, h2 = codec.name_tokens(names, no, len=ln)
    tok3 = codec.name_tokens(names, no, len=ln, want_hash=False)
    torch.cuda.synchronize()
    assert torch.equal(tok, tok2) and torch.equal(h, h2) and torch.equal(tok, tok3)
    k = 20000  # parity on a sample
    et, _ = H.name_tokens([pool[off[i]:off[i + 1]].tobytes() for i in range(k)])
    assert np.array_equal(tok3[:k].cpu().numpy(), np.array(et, np.int32))
    rows = {"names_1M": {"names": n, "name_bytes": raw, **timed({
        "old": lambda: codec.name_tokens(names, no, token=tok, hash=h),
        "len_hash": lambda: codec.name_tokens(names, no, token=tok2, hash=h2, len=ln),
        "len_nohash": lambda: codec.name_tokens(names, no, token=tok3, len=ln, want_hash=False),
        **({"other_old": lambda: other.name_tokens(names, no, token=tok, hash=h),
            "other_len_hash": lambda: other.name_tokens(names, no, token=tok2, hash=h2, len=ln),
            "other_len_nohash": lambda: other.name_tokens(names, no, token=tok3, len=ln, want_hash=False)}
           if other else {})})}}
    r = rows["names_1M"]
    r["len_hash_over_old_best"] = round(r["len_hash_us_best"] / r["old_us_best"], 3)
    r["len_hash_over_old_median"] = round(r["len_hash_us_median"] / r["old_us_median"], 3)
    pool, off = W.gen_mixed_range(W.mixed_lengths(n), 0, n, threads=8)
    raw = int(off[-1])
    src = torch.from_numpy(pool).to(dev)
    so = torch.from_numpy(off.view(np.int32)).to(dev)
    ln = torch.from_numpy(np.diff(off.astype(np.int64)).astype(np.int32)).to(dev)
    tv = codec.name_tokens(src, so, len=ln, want_hash=False)
    tvh, hv = codec.name_tokens(src, so, len=ln)
    torch.cuda.synchronize()
    assert torch.equal(tv, tvh)
    rows["mixed_values_1M"] = {"strings": n, "raw_bytes": raw,
                               "strings_up_to_max_token_len": int((ln <= 27).sum().item()), **timed({
                                   "len_nohash": lambda: codec.name_tokens(src, so, token=tv, len=ln, want_hash=False),
                                   "len_hash": lambda: codec.name_tokens(src, so, token=tvh, hash=hv, len=ln),
                                   **({"other_len_nohash": lambda: other.name_tokens(src, so, token=tv, len=ln,
                                                                                     want_hash=False),
                                       "other_len_hash": lambda: other.name_tokens(src, so, token=tvh, hash=hv,
                                                                                   len=ln)} if other else {})})}
    return rows


def bench_inflate_fields(nconn=256, per_conn=8, fields=16, alternations=15):
    """The C call of the 2,048-block inflate row, alternated call by call (no
    indexing: every call sees the same tables): plain, checked, tokens and
    both arrays; with NGHTTP2_AMD_OTHER_LIB, that build's checked call too."""
    import ctypes
    import statistics
    import nghttp2_amd
    from nghttp2_amd import hd
    blocks, conns = make_blocks(nconn, per_conn, fields)
    wire = sum(len(b) for b in blocks)
    L = hd._inflate_lib()
    m = len(blocks)
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    nva_cap, arena_cap = wire + 16, 8 * wire + 4096
    nva = (hd._Nv * nva_cap)()
    arena = (ctypes.c_uint8 * arena_cap)()
    chk = (ctypes.c_uint8 * (2 * nva_cap))()
    tk = (ctypes.c_int32 * nva_cap)()
    stc = (ctypes.c_int32 * m)()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    import torch
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    ip = (ctypes.c_void_p * m)(*[infs[c].p.value for c in conns])
    calls = {}

    def fields_call(c, t):
        def f():
            t0 = time.perf_counter()
            rv = L.nghttp2_amd_hd_inflate_blocks_fields(ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used),
                                                        arena, arena_cap, ctypes.byref(ar_used), stc, c, t, s)
            dt = time.perf_counter() - t0
            assert rv == 0
            return dt
        return f
    calls["plain"] = fields_call(None, None)
    calls["checked"] = fields_call(chk, None)
    calls["tokens"] = fields_call(None, tk)
    calls["fields"] = fields_call(chk, tk)
    other = os.environ.get("NGHTTP2_AMD_OTHER_LIB")
    if other:
        P = ctypes.CDLL(other)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        P.nghttp2_amd_hd_inflate_new.argtypes = [ctypes.POINTER(vp)]
        P.nghttp2_amd_hd_inflate_blocks_checked.argtypes = L.nghttp2_amd_hd_inflate_blocks_checked.argtypes
        pin = []
        for _ in range(nconn):
            q = vp()
            assert P.nghttp2_amd_hd_inflate_new(ctypes.byref(q)) == 0
            pin.append(q.value)
        pip = (ctypes.c_void_p * m)(*[pin[c] for c in conns])

        def other_checked():
            t0 = time.perf_counter()
            rv = P.nghttp2_amd_hd_inflate_blocks_checked(pip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used),
                                                         arena, arena_cap, ctypes.byref(ar_used), stc, chk, s)
            dt = time.perf_counter() - t0
            assert rv == 0
            return dt
        calls["other_checked"] = other_checked
    for _ in range(3):
        for c in calls.values():
            c()
    ts = {k: [] for k in calls}
    for _ in range(alternations):
        for k, c in calls.items():
            ts[k].append(c())
    nf = nv_used.value
    out = {"blocks": m, "connections": nconn, "fields": nf, "wire_bytes": wire, "alternations": alternations}
    for k, v in ts.items():
        out[k + "_s_best"] = round(min(v), 6)
        out[k + "_s_median"] = round(statistics.median(v), 6)
        out[k + "_s_worst"] = round(max(v), 6)
    out["fields_minus_checked_us_median"] = round((out["fields_s_median"] - out["checked_s_median"]) * 1e6, 1)
    out["fields_minus_checked_us_best"] = round((out["fields_s_best"] - out["checked_s_best"]) * 1e6, 1)
    if other:
        out["checked_minus_other_checked_us_median"] = round(
            (out["checked_s_median"] - out["other_checked_s_median"]) * 1e6, 1)
        out["checked_minus_other_checked_us_best"] = round(
            (out["checked_s_best"] - out["other_checked_s_best"]) * 1e6, 1)
    return out


def bench_http_facts(steps=30):
    """http_facts_batch against check_fields, alternated call by call on the
    check row's two device-resident pools in one process; each call between
    two HIP events, the best of the steps of each.  The yardstick is the
    same walk with the same loads."""
    import torch
    import nghttp2_amd
    from nghttp2_amd import workloads as W
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tests import http_fields_ref as R
    dev = torch.device("cuda:0")
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    other = other_codec(dev)
    n = 1 << 20
    out = {}
    # a pool a peer could send: 4,096 numbers of 16 KiB, all '0' but a last digit
    nz, lz = 4096, 16384
    zeros = np.full(nz * lz + 32, ord("0"), dtype=np.uint8)
    zeros[lz - 1:nz * lz:lz] = ord("7")
    zoff = (np.arange(nz + 1, dtype=np.uint64) * lz).astype(np.uint32)
    for label, (pool, off) in (("mixed_1M", W.gen_mixed_range(W.mixed_lengths(n), 0, n, threads=8)),
                               ("pseudo_1M", W.gen_pseudo_headers(n)),
                               ("zeros_16K_x4096", (zeros, zoff))):
        n = len(off) - 1
        raw = int(off[-1])
        src = torch.from_numpy(pool).to(dev)
        so = torch.from_numpy(off.view(np.int32)).to(dev)
        mask = codec.check_fields(src, so)
        facts, number = codec.http_facts_batch(src, so)
        torch.cuda.synchronize()
        k = min(n, 5000) if label != "zeros_16K_x4096" else 64  # parity on a sample
        gf, gn = facts[:k].cpu().numpy().view(np.uint32), number[:k].cpu().numpy()
        assert all((int(gf[i]), int(gn[i])) == R.facts(pool[off[i]:off[i + 1]].tobytes()) for i in range(k))
        s = torch.cuda.current_stream()
        for _ in range(5):
            codec.http_facts_batch(src, so, facts=facts, number=number)
            codec.check_fields(src, so, mask=mask)
        ev = []
        for _ in range(steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(s)
            codec.http_facts_batch(src, so, facts=facts, number=number)
            e[1].record(s)
            e[2].record(s)
            codec.check_fields(src, so, mask=mask)
            e[3].record(s)
            ev.append(e)
        torch.cuda.synchronize()
        th = min(e[0].elapsed_time(e[1]) for e in ev) * 1e-3
        tc = min(e[2].elapsed_time(e[3]) for e in ev) * 1e-3
        out[label] = {"strings": n, "raw_bytes": raw, "http_facts_us": round(th * 1e6, 2),
                      "check_us": round(tc * 1e6, 2), "http_facts_over_check": round(th / tc, 3),
                      "http_facts_GBps_R_plus_16N": round((raw + 16 * n) / th / 1e9, 1),
                      "check_GBps_R_plus_5N": round((raw + 5 * n) / tc / 1e9, 1),
                      "http_facts_us_median": round(float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e3, 2),
                      "check_us_median": round(float(np.median([e[2].elapsed_time(e[3]) for e in ev])) * 1e3, 2)}
        if other:
            out[label].update(alternate(
                {"this_http_facts": lambda: codec.http_facts_batch(src, so, facts=facts, number=number),
                 "other_http_facts": lambda: other.http_facts_batch(src, so, facts=facts, number=number)}, steps))
    return out


def bench_inflate_http(nconn=256, per_conn=8, fields=16, alternations=15):
    """The C call of the 2,048-block inflate row, alternated call by call (no
    indexing: every call sees the same tables): _fields with both arrays and
    _http with all its arrays, and the plain call; with NGHTTP2_AMD_OTHER_LIB,
    that build's three too.  Every block is run as a request on a fresh state, so every
    one of its fields is stepped (asserted: no field is left unexamined) and
    the request's block end runs."""
    import ctypes
    import statistics
    import nghttp2_amd
    from nghttp2_amd import hd
    blocks, conns = make_blocks(nconn, per_conn, fields)
    wire = sum(len(b) for b in blocks)
    L = hd._inflate_lib()
    m = len(blocks)
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    nva_cap, arena_cap = wire + 16, 8 * wire + 4096
    nva = (hd._Nv * nva_cap)()
    arena = (ctypes.c_uint8 * arena_cap)()
    chk = (ctypes.c_uint8 * (2 * nva_cap))()
    tk = (ctypes.c_int32 * nva_cap)()
    vd = (ctypes.c_int32 * nva_cap)()
    stc = (ctypes.c_int32 * m)()
    bh = (ctypes.c_int32 * m)()
    modes = (ctypes.c_uint8 * m)()
    states = (hd.HttpState * m)()
    for i in range(m):
        modes[i] = hd.HTTP_MODE_REQUEST
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    import torch
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    ip = (ctypes.c_void_p * m)(*[infs[c].p.value for c in conns])

    def timed(f):
        def g():
            t0 = time.perf_counter()
            rv = f()
            dt = time.perf_counter() - t0
            assert rv == 0
            return dt
        return g

    def http_call(lib, ip):
        def f():
            for i in range(m):
                states[i].http_flags, states[i].status_code, states[i].content_length = 0, -1, -1
            return timed(lambda: lib.nghttp2_amd_hd_inflate_blocks_http(
                ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used), arena, arena_cap, ctypes.byref(ar_used), stc,
                chk, tk, modes, states, vd, bh, s))()
        return f

    def three(lib, ip, prefix):  # the _fields, _http and plain calls of one build on its own inflaters
        return {prefix + "fields": timed(lambda: lib.nghttp2_amd_hd_inflate_blocks_fields(
                    ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used), arena, arena_cap, ctypes.byref(ar_used),
                    stc, chk, tk, s)),
                prefix + "http": http_call(lib, ip),
                prefix + "plain": timed(lambda: lib.nghttp2_amd_hd_inflate_blocks(
                    ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used), arena, arena_cap, ctypes.byref(ar_used),
                    stc, s))}
    calls = three(L, ip, "")
    other = os.environ.get("NGHTTP2_AMD_OTHER_LIB")
    if other:
        P = ctypes.CDLL(other)
        vp = ctypes.c_void_p
        P.nghttp2_amd_hd_inflate_new.argtypes = [ctypes.POINTER(vp)]
        for fn in ("nghttp2_amd_hd_inflate_blocks", "nghttp2_amd_hd_inflate_blocks_fields",
                   "nghttp2_amd_hd_inflate_blocks_http"):
            getattr(P, fn).argtypes = getattr(L, fn).argtypes
        pin = []
        for _ in range(nconn):
            q = vp()
            assert P.nghttp2_amd_hd_inflate_new(ctypes.byref(q)) == 0
            pin.append(q.value)
        calls.update(three(P, (ctypes.c_void_p * m)(*[pin[c] for c in conns]), "other_"))
    for _ in range(3):
        for c in calls.values():
            c()
    ts = {k: [] for k in calls}
    for _ in range(alternations):
        for k, c in calls.items():
            ts[k].append(c())
    # what the last _http call left: every field stepped, every block ended
    calls["http"]()
    verdicts = np.frombuffer(vd, dtype=np.int32)[:nv_used.value]
    results = np.frombuffer(bh, dtype=np.int32)[:m]
    assert not np.any(verdicts == hd.HTTP_NOT_EXAMINED) and not np.any(verdicts == hd.NGHTTP2_ERR_HTTP_HEADER)
    assert not np.any(results == hd.NGHTTP2_ERR_HTTP_HEADER)
    out = {"blocks": m, "connections": nconn, "fields": nv_used.value, "wire_bytes": wire,
           "alternations": alternations, "mode": "request",
           "fields_stepped": int(verdicts.size), "verdicts_ok": int(np.sum(verdicts == 0)),
           "verdicts_ignored": int(np.sum(verdicts == hd.NGHTTP2_ERR_IGN_HTTP_HEADER)),
           "blocks_ok": int(np.sum(results == 0)),
           "blocks_messaging_error": int(np.sum(results == hd.NGHTTP2_ERR_HTTP_MESSAGING))}
    for k, v in ts.items():
        out[k + "_s_best"] = round(min(v), 6)
        out[k + "_s_median"] = round(statistics.median(v), 6)
        out[k + "_s_worst"] = round(max(v), 6)
    out["http_minus_fields_us_median"] = round((out["http_s_median"] - out["fields_s_median"]) * 1e6, 1)
    out["http_minus_fields_us_best"] = round((out["http_s_best"] - out["fields_s_best"]) * 1e6, 1)
    if other:
        for k in ("fields", "http", "plain"):
            for stat in ("median", "best"):
                out["%s_minus_other_%s_us_%s" % (k, k, stat)] = round(
                    (out["%s_s_%s" % (k, stat)] - out["other_%s_s_%s" % (k, stat)]) * 1e6, 1)
    return out


def bench_inflate_checked(nconn=256, per_conn=8, fields=16, alternations=15):
    """The C call of the 2,048-block inflate row with and without nv_checks,
    alternated call by call (no indexing: every call sees the same tables);
    best and median of each, and the difference."""
    import ctypes
    import statistics
    import nghttp2_amd
    from nghttp2_amd import hd
    blocks, conns = make_blocks(nconn, per_conn, fields)
    wire = sum(len(b) for b in blocks)
    L = hd._inflate_lib()
    m = len(blocks)
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    nva_cap, arena_cap = wire + 16, 8 * wire + 4096
    nva = (hd._Nv * nva_cap)()
    arena = (ctypes.c_uint8 * arena_cap)()
    chk = (ctypes.c_uint8 * (2 * nva_cap))()
    stc = (ctypes.c_int32 * m)()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    import torch
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    ip = (ctypes.c_void_p * m)(*[infs[c].p.value for c in conns])

    def call(checked):
        t0 = time.perf_counter()
        rv = L.nghttp2_amd_hd_inflate_blocks_checked(ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used),
                                                     arena, arena_cap, ctypes.byref(ar_used), stc,
                                                     chk if checked else None, s)
        t = time.perf_counter() - t0
        assert rv == 0
        return t
    for _ in range(3):
        call(True), call(False)
    tp, tc = [], []
    for _ in range(alternations):
        tp.append(call(False))
        tc.append(call(True))
    nf = nv_used.value
    return {"blocks": m, "connections": nconn, "fields": nf, "wire_bytes": wire, "alternations": alternations,
            "plain_s_best": round(min(tp), 6), "checked_s_best": round(min(tc), 6),
            "plain_s_median": round(statistics.median(tp), 6), "checked_s_median": round(statistics.median(tc), 6),
            "extra_us_best": round((min(tc) - min(tp)) * 1e6, 1),
            "extra_us_median": round((statistics.median(tc) - statistics.median(tp)) * 1e6, 1),
            "checked_over_plain_median": round(statistics.median(tc) / statistics.median(tp), 3)}


def make_blocks(nconn, per_conn, fields_per_block, seed=7, index=False):
    """Header blocks of two indexed static fields and `fields_per_block`
    literal fields with a new name (Huffman when shorter), without indexing
    or (`index`) with incremental indexing, so every field enters the
    connection's dynamic table and evicts older ones."""
    from oracle import oracle as O
    from nghttp2_amd import workloads as W
    rng = np.random.Generator(np.random.PCG64(seed))
    pool, off = W.gen_mixed_values(nconn * per_conn * fields_per_block, seed=seed, hi=120)
    names = [b"cookie", b"user-agent", b"x-request-id", b"accept", b"referer", b"x-trace"]
    blocks, conns = [], []
    v = 0
    for r in range(per_conn):
        for c in range(nconn):
            out = bytearray(b"\x82\x87")  # :method GET, :scheme https
            for _ in range(fields_per_block):
                name = names[rng.integers(0, len(names))]
                val = bytes(pool[off[v]:off[v + 1]])
                v += 1
                out.append(0x40 if index else 0x00)  # literal, new name
                out += O.emit_string(name)
                out += O.emit_string(val)
            blocks.append(bytes(out))
            conns.append(c)
    return blocks, conns


def bench_inflate(nconn=256, per_conn=8, fields=16, reps=5, index=False):
    """The batched inflate front-end on `nconn` connections x `per_conn`
    blocks of `fields` literal fields: the C call alone
    (nghttp2_amd_hd_inflate_blocks: host parse, one GPU decode of every
    Huffman literal with its H2D/D2H, host replay, placement), timed around
    the ctypes call with the arrays built once, and the Python wrapper
    (inflate_blocks: marshalling the blocks in and the fields out) around it.
    Without `index` the blocks insert nothing into the tables, so repeated
    calls see the same state; with it every call starts from fresh
    inflaters (made outside the timed region)."""
    import ctypes
    import nghttp2_amd
    from nghttp2_amd import hd
    from oracle import hpack_oracle as HO
    blocks, conns = make_blocks(nconn, per_conn, fields, index=index)
    wire = sum(len(b) for b in blocks)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    # the wrapper, parity on the first connection's blocks against the restatement
    best_py = None
    for r in range(reps):
        if index and r:
            infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
        t0 = time.perf_counter()
        st, f = nghttp2_amd.inflate_blocks([infs[c] for c in conns], blocks)
        t = time.perf_counter() - t0
        best_py = t if best_py is None or t < best_py else best_py
    ref = HO.Inflater()
    for k, (c, b) in enumerate(zip(conns, blocks)):
        if c == 0:
            assert ref.inflate_block(b) == (st[k], f[k])
    nf = sum(len(x) for x in f)
    # the C call alone
    L = hd._inflate_lib()
    m = len(blocks)
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    ip = (ctypes.c_void_p * m)(*[infs[c].p.value for c in conns])
    nva_cap, arena_cap = wire + 16, 8 * wire + 4096
    nva = (hd._Nv * nva_cap)()
    arena = (ctypes.c_uint8 * arena_cap)()
    stc = (ctypes.c_int32 * m)()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    import torch
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    best_c = None
    for _ in range(3 * reps):
        if index:
            fresh = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
            ip = (ctypes.c_void_p * m)(*[fresh[c].p.value for c in conns])
        t0 = time.perf_counter()
        rv = L.nghttp2_amd_hd_inflate_blocks(ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used),
                                             arena, arena_cap, ctypes.byref(ar_used), stc, s)
        t = time.perf_counter() - t0
        assert rv == 0 and nv_used.value == nf
        best_c = t if best_c is None or t < best_c else best_c
    assert list(stc) == list(st)
    # CPU baseline: the oracle's C inflater (oracle/hpack_inflate_oracle.c,
    # the same algorithm, fresh inflaters per run) on 1 and 16 threads
    cpu = {}
    for t in (1, 16):
        best = None
        for _ in range(3):
            dt, nfc = HO.c_inflate_batch_timed(blocks, conns, nconn, t)
            assert nfc == nf
            best = dt if best is None or dt < best else best
        cpu["cpu_port_%dt_s" % t] = round(best, 5)
        cpu["cpu_port_%dt_wire_MBps" % t] = round(wire / best / 1e6, 1)
    return {"blocks": len(blocks), "connections": nconn, "fields": nf, "wire_bytes": wire, **cpu,
            "incremental_indexing": index,
            "c_s_per_call": round(best_c, 5), "c_wire_MBps": round(wire / best_c / 1e6, 1),
            "c_fields_per_s": round(nf / best_c),
            "py_s_per_call": round(best_py, 4), "py_wire_MBps": round(wire / best_py / 1e6, 1),
            "note": "c: nghttp2_amd_hd_inflate_blocks alone (host parse, one GPU decode of every "
                    "Huffman literal with H2D/D2H, host replay, placement), best of %d; py: the "
                    "inflate_blocks wrapper, Python marshalling in and out included" % (3 * reps)}


def bench_inflate_alt(nconn=256, per_conn=8, fields=16, alternations=7, index=False):
    """The batched inflate front-end's C call against the 16-thread CPU port
    of the same inflater (oracle/hpack_inflate_oracle.c) on the same blocks,
    in one process, alternating: each alternation times 5 front-end calls and
    3 CPU-port runs and keeps the median of each; the row reports the
    medians over the alternations and their ratio (the host threads are a
    share of a larger machine and swing between runs, so neither side is
    timed in isolation)."""
    import ctypes
    import statistics
    import nghttp2_amd
    from nghttp2_amd import hd
    from oracle import hpack_oracle as HO
    blocks, conns = make_blocks(nconn, per_conn, fields, index=index)
    wire = sum(len(b) for b in blocks)
    L = hd._inflate_lib()
    m = len(blocks)
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    nva_cap, arena_cap = wire + 16, 8 * wire + 4096
    nva = (hd._Nv * nva_cap)()
    arena = (ctypes.c_uint8 * arena_cap)()
    stc = (ctypes.c_int32 * m)()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    import torch
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    ip = (ctypes.c_void_p * m)(*[infs[c].p.value for c in conns])
    nf = None
    gpu_med, cpu_med = [], []
    for a in range(alternations):
        ts = []
        for _ in range(5):
            if index:
                fresh = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
                ip = (ctypes.c_void_p * m)(*[fresh[c].p.value for c in conns])
            t0 = time.perf_counter()
            rv = L.nghttp2_amd_hd_inflate_blocks(ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used),
                                                 arena, arena_cap, ctypes.byref(ar_used), stc, s)
            ts.append(time.perf_counter() - t0)
            assert rv == 0
            nf = nv_used.value if nf is None else nf
            assert nv_used.value == nf
        gpu_med.append(statistics.median(ts))
        cs = []
        for _ in range(3):
            dt, nfc = HO.c_inflate_batch_timed(blocks, conns, nconn, 16)
            assert nfc == nf
            cs.append(dt)
        cpu_med.append(statistics.median(cs))
    g, c = statistics.median(gpu_med), statistics.median(cpu_med)
    return {"blocks": m, "connections": nconn, "fields": nf, "wire_bytes": wire,
            "incremental_indexing": index, "alternations": alternations,
            "c_s_per_call_median": round(g, 6), "c_wire_MBps": round(wire / g / 1e6, 1),
            "cpu_port_16t_s_median": round(c, 6), "cpu_port_16t_wire_MBps": round(wire / c / 1e6, 1),
            "ratio_front_end_over_cpu16": round(c / g, 3),
            "per_alternation_c_s": [round(x, 6) for x in gpu_med],
            "per_alternation_cpu16_s": [round(x, 6) for x in cpu_med]}


def bench_parse(nconn=256, per_conn=8, fields=16, runs=5, steps=20):
    """Parse + gather of the 2,048-block batch on the GPU (the C calls on
    tensors allocated once) against the inflater's host phases that do the
    same work, in one process, alternating: each run times `steps` calls of
    each GPU form between HIP events (and wall time around the calls and a
    stream synchronisation, the figure a host caller would wait for), then
    five traced nghttp2_amd_hd_inflate_blocks calls.  The row reports each
    run's medians and the spread of those medians over the runs."""
    import ctypes
    import re
    import statistics
    import tempfile
    os.environ["NGHTTP2_AMD_TRACE"] = "1"
    import torch
    import nghttp2_amd
    from nghttp2_amd import hd
    blocks, conns = make_blocks(nconn, per_conn, fields)
    m = len(blocks)
    wire = b"".join(blocks)
    W = len(wire)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    dev = torch.device("cuda:0")
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    L = codec.L
    pinned = torch.from_numpy(np.frombuffer(bytearray(wire), np.uint8)).pin_memory()
    tw = pinned.to(dev)
    tw2 = torch.empty_like(tw)
    to = torch.from_numpy(off.view(np.int32)).to(dev)
    ops_cap, lits_cap, pool_cap, ws_bytes = hd.parse_blocks_bound(W, m)
    i32, u8 = torch.int32, torch.uint8
    ops = torch.empty((ops_cap, 8), dtype=i32, device=dev)
    op_off, lit_base = torch.empty(m + 1, dtype=i32, device=dev), torch.empty(m + 1, dtype=i32, device=dev)
    status, totals = torch.empty(m, dtype=i32, device=dev), torch.empty(4, dtype=i32, device=dev)
    ws = torch.empty(ws_bytes, dtype=u8, device=dev)
    lit_off = torch.empty(lits_cap + 1, dtype=i32, device=dev)
    pool = torch.empty(pool_cap, dtype=u8, device=dev)
    st = hd._stream(None)
    p = hd._p

    def parse(w):
        rv = L.nghttp2_amd_hd_parse_blocks_batch(p(w), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base),
                                                 p(totals), p(ws), ws_bytes, st)
        assert rv == 0

    def gather(w):
        rv = L.nghttp2_amd_hd_gather_literals_batch(p(w), W, p(ops), ops_cap, p(totals), p(lit_off), lits_cap,
                                                    p(pool), pool_cap, st)
        assert rv == 0

    def both():
        parse(tw)
        gather(tw)

    def with_h2d():
        tw2.copy_(pinned, non_blocking=True)
        parse(tw2)
        gather(tw2)

    calls = {"parse": lambda: parse(tw), "gather": lambda: gather(tw), "parse_gather": both,
             "h2d_parse_gather": with_h2d}
    # what the batch holds, checked against the host twin once
    both()
    torch.cuda.synchronize()
    tot = [int(x) for x in totals.cpu().numpy().view(np.uint32)]
    twin = [hd.parse_block(b)[1] for b in blocks]
    assert tot[0] == sum(len(o) for o in twin) and tot[3] == 0
    assert status.cpu().numpy().tolist() == [len(o) for o in twin]
    huff = [(b, int(r[o]), int(r[n])) for b, t in zip(blocks, twin) for r in t
            for f, o, n in ((hd.OP_NAME_HUFF, "name_off", "name_len"), (hd.OP_VALUE_HUFF, "value_off", "value_len"))
            if r["flags"] & f]
    assert tot[1] == len(huff) and tot[2] == sum(n for _, _, n in huff)
    assert pool.cpu().numpy()[:tot[2]].tobytes() == b"".join(b[o:o + n] for b, o, n in huff)

    # the inflater's C call, traced
    LI = hd._inflate_lib()
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    nva_cap, arena_cap = W + 16, 8 * W + 4096
    nva = (hd._Nv * nva_cap)()
    arena = (ctypes.c_uint8 * arena_cap)()
    stc = (ctypes.c_int32 * m)()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    ip = (ctypes.c_void_p * m)(*[infs[c].p.value for c in conns])

    def inflate():
        t0 = time.perf_counter()
        rv = LI.nghttp2_amd_hd_inflate_blocks(ip, m, ptrs, lens, nva, nva_cap, ctypes.byref(nv_used), arena,
                                              arena_cap, ctypes.byref(ar_used), stc, st)
        assert rv == 0
        return (time.perf_counter() - t0) * 1e6

    def traced(n):
        """n inflate calls with the library's stderr trace captured:
        (call us, {phase: us}) per call."""
        sys.stderr.flush()
        with tempfile.TemporaryFile() as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                wall = [inflate() for _ in range(n)]
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode("ascii", "replace")
        ph = [dict((k.strip(), float(v)) for k, v in re.findall(r" ([a-z+ ]+?)=([0-9.]+)us", ln))
              for ln in text.splitlines() if ln.startswith("[nghttp2_amd inflate]")]
        return wall, ph

    for _ in range(3):
        inflate()
    per_run = []
    s = torch.cuda.current_stream()
    for _ in range(runs):
        r = alternate(calls, steps)
        for k, c in calls.items():  # wall: the calls and a synchronisation
            ts = []
            for _ in range(steps):
                s.synchronize()
                t0 = time.perf_counter()
                c()
                s.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            r[k + "_wall_us_median"] = round(statistics.median(ts), 1)
        wall, ph = traced(5)
        r["inflate_call_us_median"] = round(statistics.median(wall), 1)
        for name in ("parse blocks", "number+copy"):
            v = [x[name] for x in ph if name in x]
            r["host_" + name.replace(" ", "_") + "_us_median"] = round(statistics.median(v), 1) if v else None
        per_run.append(r)
    keys = [k for k in per_run[0] if k.endswith("_median")]
    spread = {}
    for k in keys:
        v = [r[k] for r in per_run if r[k] is not None]
        if v:
            spread[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v)}
    return {"blocks": m, "connections": nconn, "wire_bytes": W, "ops": tot[0], "huffman_literals": tot[1],
            "huffman_bytes": tot[2], "runs": runs, "steps": steps, "over_runs": spread, "per_run": per_run,
            "note": "GPU forms: HIP events around the C calls on preallocated tensors (_us_*), and wall time "
                    "around the calls and a stream synchronisation (_wall_us_median); host phases: the "
                    "inflater's own trace of the same batch, medians of 5 calls per run"}


def bench_dev_inflate(nconn=256, per_conn=8, fields=16, runs=5, steps=20):
    """The device-resident chain parse + gather + decode_auto +
    nghttp2_amd_hd_dev_inflate_blocks on the 2,048-block batch (resident
    wire, the C calls on tensors allocated once, the decode's string count
    known on the host) against nghttp2_amd_hd_inflate_blocks on the same
    blocks, in one process, alternating call by call with fresh contexts
    each run: each run times `steps` calls of the chain between HIP events
    and as wall time around the calls and one stream synchronisation, and
    `steps` host calls as wall time.  The row reports each run's medians and
    the spread of those medians over the runs."""
    import ctypes
    import statistics
    import torch
    import nghttp2_amd
    from nghttp2_amd import hd
    blocks, conns = make_blocks(nconn, per_conn, fields)
    m = len(blocks)
    wire = b"".join(blocks)
    W = len(wire)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    dev = torch.device("cuda:0")
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    L = hd._replay_lib()
    tw = torch.from_numpy(np.frombuffer(bytearray(wire), np.uint8)).to(dev)
    to = torch.from_numpy(off.view(np.int32)).to(dev)
    # the batch's sizes, the results to hold the timed calls to, and the host call's own results
    first = nghttp2_amd.DeviceInflaters(nconn, 4096)
    r0 = first.inflate(codec, tw, to, conns)
    want = hd.replay_fields(r0.nva, r0.arena, r0.block_nv_off, r0.status)
    nfields, nbytes = (int(x) for x in r0.totals.cpu().numpy().view(np.uint32)[:2])
    hs, hf = nghttp2_amd.inflate_blocks(_fresh_for(conns, nconn), blocks)
    assert (hs, hf) == want
    ops_cap, lits_cap, pool_cap, ws_bytes = hd.parse_blocks_bound(W, m)
    i32, u8 = torch.int32, torch.uint8
    ops = torch.empty((ops_cap, 8), dtype=i32, device=dev)
    op_off, lit_base = torch.empty(m + 1, dtype=i32, device=dev), torch.empty(m + 1, dtype=i32, device=dev)
    status, totals = torch.empty(m, dtype=i32, device=dev), torch.empty(4, dtype=i32, device=dev)
    ws = torch.empty(ws_bytes, dtype=u8, device=dev)
    lit_off = torch.empty(lits_cap + 1, dtype=i32, device=dev)
    pool = torch.empty(pool_cap, dtype=u8, device=dev)
    st = hd._stream(None)
    p = hd._p
    L.nghttp2_amd_hd_parse_blocks_batch(p(tw), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base), p(totals),
                                        p(ws), ws_bytes, st)
    tot = [int(x) for x in totals.cpu().numpy().view(np.uint32)]
    T, E = tot[1], tot[2]
    dst = torch.empty(codec.decode_bound(E, T), dtype=u8, device=dev)
    dst_off, dstatus = torch.empty(T + 1, dtype=i32, device=dev), torch.empty(T, dtype=i32, device=dev)
    nva = torch.empty(24 * ops_cap, dtype=u8, device=dev)
    arena = torch.empty(nbytes, dtype=u8, device=dev)
    nv_off, out_status = torch.empty(m + 1, dtype=i32, device=dev), torch.empty(m, dtype=i32, device=dev)
    out_totals = torch.empty(4, dtype=i32, device=dev)
    csr_off, csr_blk = first.csr(conns)
    rws = torch.empty(L.nghttp2_amd_hd_dev_inflate_workspace_size(nconn, 4096, ops_cap, m), dtype=u8, device=dev)
    cur = {}

    def chain():
        rv = L.nghttp2_amd_hd_parse_blocks_batch(p(tw), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base),
                                                 p(totals), p(ws), ws_bytes, st)
        rv |= L.nghttp2_amd_hd_gather_literals_batch(p(tw), W, p(ops), ops_cap, p(totals), p(lit_off), lits_cap,
                                                     p(pool), pool_cap, st)
        rv |= L.nghttp2_amd_hd_huff_decode_batch_auto(p(pool), p(lit_off), T, E, p(dst), dst.numel(), p(dst_off),
                                                      p(dstatus), None, None, st)
        rv |= L.nghttp2_amd_hd_dev_inflate_blocks(
            cur["set"].p, p(tw), W, p(to), m, p(op_off), p(ops), ops_cap, p(status), p(totals), p(dst), dst.numel(),
            p(dst_off), p(dstatus), T, p(csr_off), p(csr_blk), p(nva), ops_cap, p(arena), nbytes, p(nv_off),
            p(out_status), p(out_totals), p(rws), rws.numel(), st)
        assert rv == 0

    LI = hd._inflate_lib()
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    hnva_cap, harena_cap = W + 16, 8 * W + 4096
    hnva = (hd._Nv * hnva_cap)()
    harena = (ctypes.c_uint8 * harena_cap)()
    stc = (ctypes.c_int32 * m)()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()

    def inflate():
        t0 = time.perf_counter()
        rv = LI.nghttp2_amd_hd_inflate_blocks(cur["ip"], m, ptrs, lens, hnva, hnva_cap, ctypes.byref(nv_used), harena,
                                              harena_cap, ctypes.byref(ar_used), stc, st)
        assert rv == 0
        return (time.perf_counter() - t0) * 1e6

    s = torch.cuda.current_stream()
    per_run = []
    for _ in range(runs):
        cur["set"] = nghttp2_amd.DeviceInflaters(nconn, 4096)
        cur["infs"] = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
        cur["ip"] = (ctypes.c_void_p * m)(*[cur["infs"][c].p.value for c in conns])
        for _ in range(3):
            chain()
            inflate()
        ev, host, wall = [], [], []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            chain()
            b.record(s)
            ev.append((a, b))
            host.append(inflate())
        torch.cuda.synchronize()
        for _ in range(steps):
            s.synchronize()
            t0 = time.perf_counter()
            chain()
            s.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
            inflate()
        t = [a.elapsed_time(b) * 1e3 for a, b in ev]
        per_run.append({"chain_us_best": round(min(t), 2), "chain_us_median": round(float(np.median(t)), 2),
                        "chain_wall_us_median": round(statistics.median(wall), 1),
                        "inflate_call_us_median": round(statistics.median(host), 1)})
    # the timed calls' last results are the batch's
    got = hd.replay_fields(nva, arena, nv_off, out_status)
    assert got == want and out_totals.cpu().numpy().view(np.uint32).tolist() == [nfields, nbytes, 0, 0]
    spread = {}
    for k in [k for k in per_run[0] if k.endswith("_median")]:
        v = [r[k] for r in per_run]
        spread[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v)}
    return {"blocks": m, "connections": nconn, "wire_bytes": W, "ops": tot[0], "huffman_literals": T,
            "huffman_bytes": E, "fields": nfields, "arena_bytes": nbytes, "runs": runs, "steps": steps,
            "over_runs": spread, "per_run": per_run,
            "note": "chain: parse + gather + decode_batch_auto + dev_inflate_blocks, the C calls on preallocated "
                    "tensors with resident wire; HIP events around the calls (_us_*) and wall time around the "
                    "calls and one stream synchronisation (_wall_us_median); inflate_call: "
                    "nghttp2_amd_hd_inflate_blocks on the same blocks from host memory, wall time"}


def bench_dev_inflate_http(nconn=256, per_conn=8, fields=16, runs=5, steps=20):
    """bench_dev_inflate's batch and method with the annotations: the device
    chain with nghttp2_amd_hd_dev_fields_http at its end (masks, tokens,
    verdicts, states and block results, every block a request on a fresh
    stream) against nghttp2_amd_hd_inflate_blocks_http on the same blocks
    from host memory, and the chain without the new call as the parent has
    it.  The three alternate call by call, fresh contexts each run.  The new
    call runs with nva_cap = the parse's bound, as the replay does, and
    (chain_http_tight) with nva_cap = the batch's field count."""
    import ctypes
    import statistics
    import torch
    import nghttp2_amd
    from nghttp2_amd import hd
    blocks, conns = make_blocks(nconn, per_conn, fields)
    m = len(blocks)
    wire = b"".join(blocks)
    W = len(wire)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    dev = torch.device("cuda:0")
    codec = nghttp2_amd.HuffmanBatchCodec(dev)
    L = hd._replay_lib()
    tw = torch.from_numpy(np.frombuffer(bytearray(wire), np.uint8)).to(dev)
    to = torch.from_numpy(off.view(np.int32)).to(dev)
    modes = [hd.HTTP_MODE_REQUEST] * m
    # the batch's sizes and the results to hold the timed calls to: the host call's
    first = nghttp2_amd.DeviceInflaters(nconn, 4096)
    want = hd.replay_annotated(first.inflate(codec, tw, to, conns, checks=True, tokens=True, http=modes))
    host = nghttp2_amd.inflate_blocks(_fresh_for(conns, nconn), blocks, checks=True, tokens=True, http=modes)
    assert want[:2] == host[:2] and want[6] == host[6]
    assert all(a.tolist() == b.tolist() for a, b in zip(want[2:6], host[2:6]))
    nfields = len(host[3])
    nbytes = sum(len(n) + len(v) + 2 for fs in host[1] for n, v, _ in fs)
    ops_cap, lits_cap, pool_cap, ws_bytes = hd.parse_blocks_bound(W, m)
    i32, u8 = torch.int32, torch.uint8
    ops = torch.empty((ops_cap, 8), dtype=i32, device=dev)
    op_off, lit_base = torch.empty(m + 1, dtype=i32, device=dev), torch.empty(m + 1, dtype=i32, device=dev)
    status, totals = torch.empty(m, dtype=i32, device=dev), torch.empty(4, dtype=i32, device=dev)
    ws = torch.empty(ws_bytes, dtype=u8, device=dev)
    lit_off = torch.empty(lits_cap + 1, dtype=i32, device=dev)
    pool = torch.empty(pool_cap, dtype=u8, device=dev)
    st = hd._stream(None)
    p = hd._p
    L.nghttp2_amd_hd_parse_blocks_batch(p(tw), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base), p(totals),
                                        p(ws), ws_bytes, st)
    tot = [int(x) for x in totals.cpu().numpy().view(np.uint32)]
    T, E = tot[1], tot[2]
    dst = torch.empty(codec.decode_bound(E, T), dtype=u8, device=dev)
    dst_off, dstatus = torch.empty(T + 1, dtype=i32, device=dev), torch.empty(T, dtype=i32, device=dev)
    nva = torch.empty(24 * ops_cap, dtype=u8, device=dev)
    arena_bytes = (nbytes + 15) // 16 * 16 + 16  # the pool rule
    arena = torch.empty(arena_bytes, dtype=u8, device=dev)
    nv_off, out_status = torch.empty(m + 1, dtype=i32, device=dev), torch.empty(m, dtype=i32, device=dev)
    out_totals = torch.empty(4, dtype=i32, device=dev)
    csr_off, csr_blk = first.csr(conns)
    rws = torch.empty(L.nghttp2_amd_hd_dev_inflate_workspace_size(nconn, 4096, ops_cap, m), dtype=u8, device=dev)
    fws = torch.empty(L.nghttp2_amd_hd_dev_fields_http_workspace_size(ops_cap, m), dtype=u8, device=dev)
    chk = torch.empty(2 * ops_cap, dtype=u8, device=dev)
    tok, verd = torch.empty(ops_cap, dtype=i32, device=dev), torch.empty(ops_cap, dtype=i32, device=dev)
    dmodes = torch.from_numpy(np.array(modes, np.uint8)).to(dev)
    fresh = torch.from_numpy(np.array([(0, -1, -1)] * m, hd._HTTP_STATE_DTYPE).view(np.uint8).copy()).to(dev)
    dstate, bhttp = fresh.clone(), torch.empty(m, dtype=i32, device=dev)
    cur = {}

    def chain():
        rv = L.nghttp2_amd_hd_parse_blocks_batch(p(tw), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base),
                                                 p(totals), p(ws), ws_bytes, st)
        rv |= L.nghttp2_amd_hd_gather_literals_batch(p(tw), W, p(ops), ops_cap, p(totals), p(lit_off), lits_cap,
                                                     p(pool), pool_cap, st)
        rv |= L.nghttp2_amd_hd_huff_decode_batch_auto(p(pool), p(lit_off), T, E, p(dst), dst.numel(), p(dst_off),
                                                      p(dstatus), None, None, st)
        rv |= L.nghttp2_amd_hd_dev_inflate_blocks(
            cur["set"].p, p(tw), W, p(to), m, p(op_off), p(ops), ops_cap, p(status), p(totals), p(dst), dst.numel(),
            p(dst_off), p(dstatus), T, p(csr_off), p(csr_blk), p(nva), ops_cap, p(arena), nbytes, p(nv_off),
            p(out_status), p(out_totals), p(rws), rws.numel(), st)
        assert rv == 0

    def chain_http(cap=ops_cap):
        chain()
        dstate.copy_(fresh)  # (the streams' states are the call's input: fresh ones each time)
        rv = L.nghttp2_amd_hd_dev_fields_http(p(nva), cap, p(arena), arena_bytes, p(nv_off), p(out_status),
                                              p(out_totals), m, p(chk), p(tok), p(dmodes), p(dstate), p(verd),
                                              p(bhttp), p(fws), fws.numel(), st)
        assert rv == 0

    LI = hd._inflate_lib()
    keep = [ctypes.create_string_buffer(b, len(b)) for b in blocks]
    ptrs = (ctypes.c_void_p * m)(*[ctypes.cast(k, ctypes.c_void_p) for k in keep])
    lens = (ctypes.c_size_t * m)(*[len(b) for b in blocks])
    hnva_cap, harena_cap = W + 16, 8 * W + 4096
    hnva = (hd._Nv * hnva_cap)()
    harena = (ctypes.c_uint8 * harena_cap)()
    stc, hbhttp = (ctypes.c_int32 * m)(), (ctypes.c_int32 * m)()
    hchk = (ctypes.c_uint8 * (2 * hnva_cap))()
    htok, hverd = (ctypes.c_int32 * hnva_cap)(), (ctypes.c_int32 * hnva_cap)()
    hmodes = (ctypes.c_uint8 * m)(*modes)
    hfresh = np.array([(0, -1, -1)] * m, hd._HTTP_STATE_DTYPE)
    hstate = hfresh.copy()
    nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()

    def inflate_http():
        t0 = time.perf_counter()
        hstate[:] = hfresh
        rv = LI.nghttp2_amd_hd_inflate_blocks_http(cur["ip"], m, ptrs, lens, hnva, hnva_cap, ctypes.byref(nv_used),
                                                   harena, harena_cap, ctypes.byref(ar_used), stc, hchk, htok, hmodes,
                                                   ctypes.c_void_p(hstate.ctypes.data), hverd, hbhttp, st)
        assert rv == 0
        return (time.perf_counter() - t0) * 1e6

    def tight():
        chain_http(nfields)

    forms = {"chain": chain, "chain_http": chain_http, "chain_http_tight": tight}
    s = torch.cuda.current_stream()
    per_run = []
    for _ in range(runs):
        cur["set"] = nghttp2_amd.DeviceInflaters(nconn, 4096)
        cur["infs"] = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
        cur["ip"] = (ctypes.c_void_p * m)(*[cur["infs"][c].p.value for c in conns])
        for _ in range(3):
            for f in forms.values():
                f()
            inflate_http()
        ev, hostt, wall = {k: [] for k in forms}, [], {k: [] for k in forms}
        for _ in range(steps):
            for k, f in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                f()
                b.record(s)
                ev[k].append((a, b))
            hostt.append(inflate_http())
        torch.cuda.synchronize()
        for _ in range(steps):
            for k, f in forms.items():
                s.synchronize()
                t0 = time.perf_counter()
                f()
                s.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e6)
            inflate_http()
        r = {"inflate_http_call_us_median": round(statistics.median(hostt), 1)}
        for k in forms:
            t = [a.elapsed_time(b) * 1e3 for a, b in ev[k]]
            r[k + "_us_best"] = round(min(t), 2)
            r[k + "_us_median"] = round(float(np.median(t)), 2)
            r[k + "_wall_us_median"] = round(statistics.median(wall[k]), 1)
        per_run.append(r)
    # the timed calls' last results are the batch's, and the host's
    chain_http()
    torch.cuda.synchronize()
    assert hd.replay_fields(nva, arena[:nbytes], nv_off, out_status) == tuple(host[:2])
    assert chk.cpu().numpy()[:2 * nfields].reshape(-1, 2).tolist() == host[2].tolist()
    assert tok.cpu().numpy()[:nfields].tolist() == host[3].tolist()
    assert verd.cpu().numpy()[:nfields].tolist() == host[4].tolist()
    assert dstate.cpu().numpy().view(hd._HTTP_STATE_DTYPE).tolist() == host[5].tolist() == hstate.tolist()
    assert bhttp.cpu().tolist() == host[6] == list(hbhttp)
    spread = {}
    for k in [k for k in per_run[0] if k.endswith("_median")]:
        v = [r[k] for r in per_run]
        spread[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v)}
    return {"blocks": m, "connections": nconn, "wire_bytes": W, "ops": tot[0], "huffman_literals": T,
            "huffman_bytes": E, "fields": nfields, "arena_bytes": nbytes, "nva_cap": ops_cap, "runs": runs,
            "steps": steps, "over_runs": spread, "per_run": per_run,
            "note": "chain: parse + gather + decode_batch_auto + dev_inflate_blocks as in the dev_inflate row; "
                    "chain_http: the same followed by nghttp2_amd_hd_dev_fields_http (all five outputs, a copy of "
                    "the fresh states in front) with nva_cap = the parse's bound; chain_http_tight: with nva_cap = "
                    "the batch's fields; HIP events around the calls (_us_*) and wall time around the calls and one "
                    "stream synchronisation (_wall_us_median); inflate_http_call: "
                    "nghttp2_amd_hd_inflate_blocks_http on the same blocks from host memory, wall time"}


def make_lists(nconn, per_conn, fields_per_block, repeat, seed=7):
    """make_blocks' batch as header lists: two static fields and
    `fields_per_block` literal fields per list, block r of every connection
    before block r + 1 of any.  `repeat`: a connection sends one list per_conn
    times (names of its own, values of at most 64 bytes, so the table holds
    the list and from the second block on every field is indexed: the search
    is the work).  Else every value is new (six names): every field is a
    name match, an insertion and evictions."""
    from nghttp2_amd import workloads as W
    rng = np.random.Generator(np.random.PCG64(seed))
    nv = nconn * fields_per_block * (1 if repeat else per_conn)
    pool, off = W.gen_mixed_values(nv, seed=seed, hi=64 if repeat else 120)
    names = [b"cookie", b"user-agent", b"x-request-id", b"accept", b"referer", b"x-trace"]
    lists, conns = [], []
    v = 0
    for r in range(per_conn):
        for c in range(nconn):
            hl = [(b":method", b"GET"), (b":scheme", b"https")]
            for k in range(fields_per_block):
                if repeat:
                    i = c * fields_per_block + k
                    hl.append((b"x-h%02d" % k, bytes(pool[off[i]:off[i + 1]])))
                else:
                    hl.append((names[rng.integers(0, len(names))], bytes(pool[off[v]:off[v + 1]])))
                    v += 1
            lists.append(hl)
            conns.append(c)
    return lists, conns


def bench_dev_deflate(nconn=256, per_conn=8, fields=16, runs=5, steps=20, batches=("repeat", "new")):
    """nghttp2_amd_hd_dev_deflate_blocks on bench_dev_inflate's batch shape
    (2,048 lists, 256 connections, 18 fields; resident fields, the C call on
    tensors allocated once) against nghttp2_amd_hd_deflate_blocks on the same
    lists from host memory, in one process, alternating call by call with
    fresh contexts each run: each run times `steps` device calls between HIP
    events and as wall time around the call and one stream synchronisation,
    and `steps` host calls as wall time.  Two batches (make_lists): `repeat`,
    the steady state, and `new`.  The row reports each run's medians and the
    spread of those medians over the runs."""
    import ctypes
    import statistics
    import torch
    import nghttp2_amd
    from nghttp2_amd import hd
    dev = torch.device("cuda:0")
    L = hd._dev_deflate_lib()
    LD = hd._deflate_lib()
    p = hd._p
    i32, u8 = torch.int32, torch.uint8
    out_rows = {}
    for batch in batches:
        lists, conns = make_lists(nconn, per_conn, fields, batch == "repeat")
        m = len(lists)
        first = nghttp2_amd.DeviceDeflaters(nconn, 4096)
        tn, ta, to = first.upload(lists)
        nf = sum(len(hl) for hl in lists)
        ab = ta.numel()
        csr_off, csr_blk = first.csr(conns)
        # the results to hold the timed calls to: the host deflater's on fresh contexts
        ds = [nghttp2_amd.HpackDeflater() for _ in range(nconn)]
        hst, hwire = nghttp2_amd.deflate_blocks([ds[c] for c in conns], lists)
        r0 = first.deflate((tn, ta, to), csr_off, csr_blk)
        assert hd.deflated_wire(r0[0], r0[1]) == hwire
        cap = first.bound(m, nf, ab)
        out = torch.empty(cap, dtype=u8, device=dev)
        out_off, out_status = torch.empty(m + 1, dtype=i32, device=dev), torch.empty(m, dtype=i32, device=dev)
        out_totals = torch.empty(4, dtype=i32, device=dev)
        ws = torch.empty(L.nghttp2_amd_hd_dev_deflate_workspace_size(nconn, 4096, nf, ab, m), dtype=u8, device=dev)
        st = hd._stream(None)
        cur = {}

        def device():
            rv = L.nghttp2_amd_hd_dev_deflate_blocks(cur["set"].p, p(tn), nf, p(ta), ab, p(to), m, p(csr_off),
                                                     p(csr_blk), p(out), cap, p(out_off), p(out_status),
                                                     p(out_totals), p(ws), ws.numel(), st)
            assert rv == 0

        # the host call's arguments, built once: an nghttp2_nv array over one joined buffer
        flat = [f for hl in lists for f in hl]
        joined = np.frombuffer(b"".join(x for n_, v_ in flat for x in (n_, v_)), np.uint8)
        plen = np.fromiter((len(x) for n_, v_ in flat for x in (n_, v_)), np.uint64, count=2 * nf)
        pstart = np.zeros(2 * nf, np.uint64)
        np.cumsum(plen[:-1], out=pstart[1:])
        hnva = np.zeros(nf, hd._NVIN_DTYPE)
        hnva["name"], hnva["value"] = pstart[0::2] + np.uint64(joined.ctypes.data), pstart[1::2] + np.uint64(joined.ctypes.data)
        hnva["namelen"], hnva["valuelen"] = plen[0::2], plen[1::2]
        hoffs = np.zeros(m + 1, np.uint32)
        np.cumsum([len(hl) for hl in lists], out=hoffs[1:])
        hout, hout_off, hstat = np.empty(cap, np.uint8), np.zeros(m + 1, np.uint32), np.zeros(m, np.int32)
        vp = ctypes.c_void_p

        def host():
            t0 = time.perf_counter()
            rv = LD.nghttp2_amd_hd_deflate_blocks(vp(cur["dp"].ctypes.data), m, vp(hnva.ctypes.data),
                                                  vp(hoffs.ctypes.data), vp(hout.ctypes.data), cap,
                                                  vp(hout_off.ctypes.data), vp(hstat.ctypes.data), st)
            assert rv == 0
            return (time.perf_counter() - t0) * 1e6

        s = torch.cuda.current_stream()
        per_run = []
        for _ in range(runs):
            cur["set"] = nghttp2_amd.DeviceDeflaters(nconn, 4096)
            cur["ds"] = [nghttp2_amd.HpackDeflater() for _ in range(nconn)]
            cur["dp"] = np.fromiter((cur["ds"][c].p.value for c in conns), np.uint64, count=m)
            for _ in range(3):
                device()
                host()
            ev, hostt, wall = [], [], []
            for _ in range(steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                device()
                b.record(s)
                ev.append((a, b))
                hostt.append(host())
            torch.cuda.synchronize()
            for _ in range(steps):
                s.synchronize()
                t0 = time.perf_counter()
                device()
                s.synchronize()
                wall.append((time.perf_counter() - t0) * 1e6)
                host()
            t = [a.elapsed_time(b) * 1e3 for a, b in ev]
            per_run.append({"device_us_best": round(min(t), 2), "device_us_median": round(float(np.median(t)), 2),
                            "device_wall_us_median": round(statistics.median(wall), 1),
                            "deflate_call_us_median": round(statistics.median(hostt), 1)})
        # the timed calls' last results: both sides made the same calls on contexts of the same age
        tot = out_totals.cpu().numpy().view(np.uint32).tolist()
        oo = hout_off.tolist()
        assert tot[2] == 0 and tot[0] == oo[m]
        assert hd.deflated_wire(out, out_off) == [hout[oo[i]:oo[i + 1]].tobytes() for i in range(m)]
        spread = {}
        for k in [k for k in per_run[0] if k.endswith("_median")]:
            v = [r[k] for r in per_run]
            spread[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v)}
        out_rows[batch] = {"lists": m, "connections": nconn, "fields": nf, "arena_bytes": ab, "wire_bytes": tot[0],
                           "literal_pool_bytes": tot[1], "runs": runs, "steps": steps, "over_runs": spread,
                           "per_run": per_run}
    out_rows["note"] = ("device: nghttp2_amd_hd_dev_deflate_blocks, the C call on preallocated tensors with resident "
                        "fields; HIP events around the call (_us_*) and wall time around the call and one stream "
                        "synchronisation (_wall_us_median); deflate_call: nghttp2_amd_hd_deflate_blocks on the same "
                        "lists from host memory, wall time; the last timed calls' wires are asserted equal")
    return out_rows


def _fresh_for(conns, nconn):
    import nghttp2_amd
    infs = [nghttp2_amd.HpackInflater() for _ in range(nconn)]
    return [infs[c] for c in conns]


if __name__ == "__main__":
    rows = sys.argv[1:] or ["emit", "emit3", "inflate", "names"]
    fns = {"emit": bench_emit, "emit3": lambda: bench_emit(cfg=3), "inflate": bench_inflate,
           "inflate_index": lambda: bench_inflate(index=True),
           "inflate_alt": bench_inflate_alt,
           "inflate_alt_index": lambda: bench_inflate_alt(index=True),
           "names": bench_names,
           "check": bench_check,
           "inflate_checked": bench_inflate_checked,
           "names_len": bench_names_len,
           "inflate_fields": bench_inflate_fields,
           "http_facts": bench_http_facts,
           "inflate_http": bench_inflate_http,
           "parse": bench_parse,
           "dev_inflate": bench_dev_inflate,
           "dev_inflate_http": bench_dev_inflate_http,
           "dev_deflate": bench_dev_deflate,
           "dev_deflate_repeat": lambda: bench_dev_deflate(batches=("repeat",)),
           "dev_deflate_new": lambda: bench_dev_deflate(batches=("new",)),
           "names_short": lambda: bench_names(long_frac=0.0)}
    print(json.dumps({r: fns[r]() for r in rows}, indent=1))
