#!/usr/bin/env python3
"""One-process A/B of library builds (tools/diag/lib_*.so, e.g. the parent
commit's library and a second copy of it as the control) on the batch of
tools/bench_rows.py's dev_inflate, dev_inflate_http and inflate_http rows
(2,048 blocks, 256 connections): the device chain, the chain with
dev_fields_http, and the host _http call, of every such library and of the
tree's own build ("change").  Every build's results are compared first, the nv
records byte for byte; then the builds alternate call by call, each timed call
on a drained stream (a call queued behind another build's measures something
else than one that starts on an idle queue), the order rotating with the step,
fresh contexts each run.  Reported: every run's medians, and per run each
build's difference to `parent`.  RUNS, STEPS.  Prints one JSON object."""
import ctypes
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import torch
import nghttp2_amd
from nghttp2_amd import hd
import bench_rows as BR

RUNS, STEPS = int(os.environ.get("RUNS", "5")), int(os.environ.get("STEPS", "21"))
nconn, per_conn, fields = 256, 8, 16
blocks, conns = BR.make_blocks(nconn, per_conn, fields)
m = len(blocks)
wire = b"".join(blocks)
W = len(wire)
off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
dev = torch.device("cuda:0")
codec = nghttp2_amd.HuffmanBatchCodec(dev)
L0 = hd._replay_lib()
LI0 = hd._inflate_lib()
FNS = ["nghttp2_amd_hd_parse_blocks_batch", "nghttp2_amd_hd_gather_literals_batch",
       "nghttp2_amd_hd_huff_decode_batch_auto", "nghttp2_amd_hd_dev_inflate_blocks",
       "nghttp2_amd_hd_dev_inflate_workspace_size", "nghttp2_amd_hd_dev_fields_http_workspace_size",
       "nghttp2_amd_hd_dev_fields_http", "nghttp2_amd_hd_dev_inflaters_new", "nghttp2_amd_hd_dev_inflaters_del",
       "nghttp2_amd_hd_inflate_blocks_http"]
libs = {"change": L0}
for p in sorted(glob.glob(os.path.join(HERE, "lib_*.so"))):
    P = ctypes.CDLL(p, mode=ctypes.RTLD_LOCAL)
    for fn in FNS:
        src = getattr(LI0 if fn == "nghttp2_amd_hd_inflate_blocks_http" else L0, fn)
        getattr(P, fn).argtypes, getattr(P, fn).restype = src.argtypes, src.restype
    P.nghttp2_amd_hd_inflate_new.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    libs[os.path.basename(p)[4:-3]] = P
L0.nghttp2_amd_hd_inflate_new.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
print("libs", list(libs), file=sys.stderr, flush=True)

tw = torch.from_numpy(np.frombuffer(bytearray(wire), np.uint8)).to(dev)
to = torch.from_numpy(off.view(np.int32)).to(dev)
modes = [hd.HTTP_MODE_REQUEST] * m
first = nghttp2_amd.DeviceInflaters(nconn, 4096)
want = hd.replay_annotated(first.inflate(codec, tw, to, conns, checks=True, tokens=True, http=modes))
host = nghttp2_amd.inflate_blocks(BR._fresh_for(conns, nconn), blocks, checks=True, tokens=True, http=modes)
assert want[:2] == host[:2] and want[6] == host[6]
nfields = len(host[3])
nbytes = sum(len(n) + len(v) + 2 for fs in host[1] for n, v, _ in fs)
ops_cap, lits_cap, pool_cap, ws_bytes = hd.parse_blocks_bound(W, m)
i32, u8 = torch.int32, torch.uint8
E_ = lambda n, dt=i32: torch.empty(n, dtype=dt, device=dev)
ops = torch.empty((ops_cap, 8), dtype=i32, device=dev)
op_off, lit_base, status, totals = E_(m + 1), E_(m + 1), E_(m), E_(4)
ws, lit_off, pool = E_(ws_bytes, u8), E_(lits_cap + 1), E_(pool_cap, u8)
st = hd._stream(None)
p = hd._p
L0.nghttp2_amd_hd_parse_blocks_batch(p(tw), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base), p(totals),
                                     p(ws), ws_bytes, st)
tot = [int(x) for x in totals.cpu().numpy().view(np.uint32)]
T, E = tot[1], tot[2]
dst = E_(codec.decode_bound(E, T), u8)
dst_off, dstatus = E_(T + 1), E_(T)
nva = E_(24 * ops_cap, u8)
arena_bytes = (nbytes + 15) // 16 * 16 + 16
arena = E_(arena_bytes, u8)
nv_off, out_status, out_totals = E_(m + 1), E_(m), E_(4)
csr_off, csr_blk = first.csr(conns)
rws_n = max(L.nghttp2_amd_hd_dev_inflate_workspace_size(nconn, 4096, ops_cap, m) for L in libs.values())
fws_n = max(L.nghttp2_amd_hd_dev_fields_http_workspace_size(ops_cap, m) for L in libs.values())
assert len({L.nghttp2_amd_hd_dev_inflate_workspace_size(nconn, 4096, ops_cap, m) for L in libs.values()}) == 1
assert len({L.nghttp2_amd_hd_dev_fields_http_workspace_size(ops_cap, m) for L in libs.values()}) == 1
rws, fws = E_(rws_n, u8), E_(fws_n, u8)
chk, tok, verd = E_(2 * ops_cap, u8), E_(ops_cap), E_(ops_cap)
dmodes = torch.from_numpy(np.array(modes, np.uint8)).to(dev)
fresh = torch.from_numpy(np.array([(0, -1, -1)] * m, hd._HTTP_STATE_DTYPE).view(np.uint8).copy()).to(dev)
dstate, bhttp = fresh.clone(), E_(m)
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
cur = {}


def fresh_contexts():
    for k, L in libs.items():
        old = cur.get(k)
        if old:
            L.nghttp2_amd_hd_dev_inflaters_del(old["set"])
        s = ctypes.c_void_p()
        assert L.nghttp2_amd_hd_dev_inflaters_new(ctypes.byref(s), nconn, 4096, st) == 0
        infs = []
        for _ in range(nconn):
            q = ctypes.c_void_p()
            assert L.nghttp2_amd_hd_inflate_new(ctypes.byref(q)) == 0
            infs.append(q.value)
        cur[k] = {"set": s, "ip": (ctypes.c_void_p * m)(*[infs[c] for c in conns])}
    torch.cuda.synchronize()


def chain(k):
    L = libs[k]
    rv = L.nghttp2_amd_hd_parse_blocks_batch(p(tw), p(to), m, p(op_off), p(ops), ops_cap, p(status), p(lit_base),
                                             p(totals), p(ws), ws_bytes, st)
    rv |= L.nghttp2_amd_hd_gather_literals_batch(p(tw), W, p(ops), ops_cap, p(totals), p(lit_off), lits_cap, p(pool),
                                                 pool_cap, st)
    rv |= L.nghttp2_amd_hd_huff_decode_batch_auto(p(pool), p(lit_off), T, E, p(dst), dst.numel(), p(dst_off),
                                                  p(dstatus), None, None, st)
    rv |= L.nghttp2_amd_hd_dev_inflate_blocks(
        cur[k]["set"], p(tw), W, p(to), m, p(op_off), p(ops), ops_cap, p(status), p(totals), p(dst), dst.numel(),
        p(dst_off), p(dstatus), T, p(csr_off), p(csr_blk), p(nva), ops_cap, p(arena), nbytes, p(nv_off),
        p(out_status), p(out_totals), p(rws), rws.numel(), st)
    assert rv == 0


def chain_http(k):
    chain(k)
    dstate.copy_(fresh)
    rv = libs[k].nghttp2_amd_hd_dev_fields_http(p(nva), ops_cap, p(arena), arena_bytes, p(nv_off), p(out_status),
                                                p(out_totals), m, p(chk), p(tok), p(dmodes), p(dstate), p(verd),
                                                p(bhttp), p(fws), fws.numel(), st)
    assert rv == 0


def host_http(k):
    t0 = time.perf_counter()
    hstate[:] = hfresh
    rv = libs[k].nghttp2_amd_hd_inflate_blocks_http(cur[k]["ip"], m, ptrs, lens, hnva, hnva_cap, ctypes.byref(nv_used),
                                                    harena, harena_cap, ctypes.byref(ar_used), stc, hchk, htok, hmodes,
                                                    ctypes.c_void_p(hstate.ctypes.data), hverd, hbhttp, st)
    assert rv == 0
    return (time.perf_counter() - t0) * 1e6


# every build's results, against the host call's and against each other
fresh_contexts()
same = {}
for k in libs:
    for t in (nva, arena, chk, tok, verd, bhttp, nv_off, out_status, out_totals):
        t.zero_()
    chain_http(k)
    torch.cuda.synchronize()
    assert hd.replay_fields(nva, arena[:nbytes], nv_off, out_status) == tuple(host[:2]), k
    assert chk.cpu().numpy()[:2 * nfields].reshape(-1, 2).tolist() == host[2].tolist(), k
    assert tok.cpu().numpy()[:nfields].tolist() == host[3].tolist(), k
    assert verd.cpu().numpy()[:nfields].tolist() == host[4].tolist(), k
    assert dstate.cpu().numpy().view(hd._HTTP_STATE_DTYPE).tolist() == host[5].tolist(), k
    assert bhttp.cpu().tolist() == host[6], k
    assert out_totals.cpu().numpy().view(np.uint32).tolist() == [nfields, nbytes, 0, 0], k
    host_http(k)
    assert list(hbhttp) == host[6] and hstate.tolist() == host[5].tolist(), k
    assert list(hverd)[:nfields] == host[4].tolist(), k
    # the records' raw bytes, padding included
    same[k] = nva[:24 * nfields].cpu().numpy().tobytes()
assert len(set(same.values())) == 1, "the builds' nv records differ in their raw bytes"
print("results equal across", list(libs), file=sys.stderr, flush=True)

s = torch.cuda.current_stream()
forms = {"chain": chain, "chain_http": chain_http}
per_run = []
for run in range(RUNS):
    fresh_contexts()
    for _ in range(3):
        for k in libs:
            for f in forms.values():
                f(k)
            host_http(k)
    ev = {(k, n): [] for k in libs for n in forms}
    hostt = {k: [] for k in libs}
    names = list(libs)
    for step in range(STEPS):
        # every timed call starts on a drained stream, and the builds take turns at going first
        order = names[step % len(names):] + names[:step % len(names)]
        for n, f in forms.items():
            for k in order:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.synchronize()
                a.record(s)
                f(k)
                b.record(s)
                ev[(k, n)].append((a, b))
        for k in order:
            s.synchronize()
            hostt[k].append(host_http(k))
    torch.cuda.synchronize()
    r = {}
    for k in libs:
        for n in forms:
            r["%s.%s_us_median" % (k, n)] = round(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[(k, n)]])), 2)
        r["%s.host_http_us_median" % k] = round(statistics.median(hostt[k]), 1)
    per_run.append(r)
    print("run", run, json.dumps(r), file=sys.stderr, flush=True)
rows = {}
for n in ("chain", "chain_http", "host_http"):
    row = {}
    for k in libs:
        v = [r["%s.%s_us_median" % (k, n)] for r in per_run]
        row[k] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
    for k in libs:
        if k != "parent":
            d = [round(r["%s.%s_us_median" % (k, n)] - r["parent.%s_us_median" % n], 2) for r in per_run]
            row[k + "_minus_parent_per_run"] = d
    rows[n] = row
print(json.dumps({"blocks": m, "connections": nconn, "fields": nfields, "arena_bytes": nbytes, "runs": RUNS,
                  "steps": STEPS, "libs": list(libs), "rows": rows, "per_run": per_run,
                  "note": "chain = parse + gather + decode_batch_auto + dev_inflate_blocks (the dev_inflate row), "
                          "chain_http = the same + dev_fields_http (the dev_inflate_http row), HIP events; host_http = "
                          "nghttp2_amd_hd_inflate_blocks_http from host memory (the inflate_http row), wall time; "
                          "the builds alternate call by call, each call on a drained stream, the order rotating; parent2 is a second copy of the parent's library"},
                 indent=1))
del first
