"""nghttp2_amd_hd_deflate_plan_host (csrc/hd_deflate_plan.h walked on the host;
no GPU): the field step of the device deflaters -- indexing decision, table
search, insertion with eviction, representation bytes, pending size updates --
over the same header, ring, keys and stores the device contexts use.

The twin's plan is spliced into wire in Python with the C oracle's emit_string
(tests/hd_deflate_plan_ref.py) and held against every deflate step the
reference itself recorded (tests/golden/ref_hd_wire.json) and against the
Python restatement (oracle.hpack_oracle.Deflater) on random batches."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from nghttp2_amd import hd
from oracle import hpack_oracle as HO
from tests import hd_deflate_plan_ref as D
from tests import ref_hd_wire_lib as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recorded_connections():
    """The deflate connections that can be expressed here, and how many were
    left out: those with a step whose recorded rv is negative (deflate_hd2 /
    deflate_hd_vec2 one byte short; overflow is all or nothing here)."""
    conns = W.connections(side="d")
    keep = [c for c in conns if not any(s["op"] == "deflate" and s["rv"] < 0 for s in c["steps"])]
    return keep, len(conns) - len(keep)


def test_recorded_reference():
    conns, left_out = recorded_connections()
    assert (len(conns), left_out) == (73, 3)
    ndef = nchg = 0
    maxes = set()
    for c in conns:
        maxes.add(c["deflate_max"])
        d = D.TwinDeflater(c["deflate_max"])
        for k, s in enumerate(c["steps"]):
            if s["op"] not in ("dchange", "deflate"):
                continue
            W.check_deflate_step(dict(s, api=None), d, W.where(c, k))
            ndef += s["op"] == "deflate"
            nchg += s["op"] == "dchange"
    assert (ndef, nchg) == (256, 16)
    assert min(maxes) == 0 and max(maxes) == 8192
    assert any(len(v) == 70000 for c in conns for s in c["steps"] if s["op"] == "deflate" for _, v, _ in s["nva"])


@pytest.mark.parametrize("deflate_max", [4096, 256, 0])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_batches_against_restatement(seed, deflate_max):
    nconn = 5
    order, lists = D.random_lists(seed * 1000 + deflate_max, 60, nconn)
    kinds = set()
    for c in range(nconn):
        mine = [hl for o, hl in zip(order, lists) if o == c]
        # block by block
        twin, ref = hd.HostDeflatePlanner(4096, deflate_max), HO.Deflater(deflate_max)
        want = []
        for k, hl in enumerate(mine):
            if k == len(mine) // 2:  # a change of the table size in the middle, then back
                for v in (64, 4096):
                    twin.change_table_size(v)
                    ref.change_table_size(v)
            recs, heads, nva, arena, off = twin.plan([hl])
            kinds.update((int(r["bytes"][0]) & 0xC0, int(r["lits"])) for r in recs)
            want.append(ref.deflate_block(hl))
            assert D.splice(recs, heads, nva, arena, off) == [want[-1]], (c, k)
            assert twin.state() == ([tuple(e) for e in ref.table], ref.size, ref.max), (c, k)
        # the same blocks in one call: the walk carries the table across them
        both, ref = hd.HostDeflatePlanner(4096, deflate_max), HO.Deflater(deflate_max)
        want = [ref.deflate_block(hl) for hl in mine]
        assert D.twin_wire(both, mine) == want
        assert both.state() == ([tuple(e) for e in ref.table], ref.size, ref.max)
    if deflate_max == 4096:  # indexed, indexed name and new name all occurred
        assert {(0x80, 0), (0x40, 2), (0x40, 3)} <= kinds


def test_insertion_evicts_the_entry_its_index_names():
    """deflate_nv inserts after the search and before the emit: the indexed
    name may be the entry the insertion evicts."""
    twin, ref = hd.HostDeflatePlanner(4096, 256), HO.Deflater(256)
    lists = [[(b"abcdefgh", b"12345678")], [(b"abcdefgh", b"w" * 100)], [(b"abcdefgh", b"x" * 101)]]
    want = [ref.deflate_block(hl) for hl in lists]
    assert D.twin_wire(twin, lists) == want
    assert twin.state() == ([tuple(e) for e in ref.table], ref.size, ref.max)
    assert want[2][0] == 0x40 | 62 and len(ref.table) == 1


def test_hash_is_a_filter_only():
    a, b = D.colliding_names()
    assert a != b and hd.name_hash(a) == hd.name_hash(b)
    twin, ref = hd.HostDeflatePlanner(), HO.Deflater()
    lists = [[(a, b"v")], [(b, b"v")], [(a, b"v"), (b, b"v")]]
    assert D.twin_wire(twin, lists) == [ref.deflate_block(hl) for hl in lists]
    assert twin.table() == [(b, b"v"), (a, b"v")]


def test_arguments():
    L = hd._dev_deflate_lib()
    bad = hd.NGHTTP2_ERR_INVALID_ARGUMENT
    p = hd.HostDeflatePlanner()
    a = np.zeros(64, np.uint32)
    q = a.ctypes.data
    full = [p.hdr.ctypes.data, p.ring.ctypes.data, p.keys.ctypes.data, p.store.ctypes.data, 4096, q, q, 64, q, 1, q, q]
    assert L.nghttp2_amd_hd_deflate_plan_host(*full) == 0
    for k in (0, 1, 2, 3, 8, 11):
        b = list(full)
        b[k] = None
        assert L.nghttp2_amd_hd_deflate_plan_host(*b) == bad, k
    for tb in (0, 2048, 4097, 6144):
        b = list(full)
        b[4] = tb
        assert L.nghttp2_amd_hd_deflate_plan_host(*b) == bad, tb
    b = list(full)
    b[9] = 0
    b[0] = None
    assert L.nghttp2_amd_hd_deflate_plan_host(*b) == 0  # no block: nothing is touched
    # a deflate_max the store could not hold is refused
    assert L.nghttp2_amd_hd_deflate_plan_host_init(p.hdr.ctypes.data, 4096, 4097) == bad
    assert L.nghttp2_amd_hd_deflate_plan_host_init(p.hdr.ctypes.data, 8192, 8192) == 0


def test_walk_under_sanitizers(tmp_path):
    """tests/c/deflate_plan_sanitize.cpp: the header's walk over generated
    fields in a stand-alone program under ASan + UBSan, checked against a
    model it keeps itself.  No Python process is involved in the run and
    nothing is preloaded."""
    # (clang links the sanitizer runtimes into the program itself)
    cxx = next((c for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler for the sanitizer program"
    exe = str(tmp_path / "deflate_plan_sanitize")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(REPO, "nghttp2_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "c", "deflate_plan_sanitize.cpp")], check=True, timeout=300)
    p = subprocess.run([exe, "300", "1"], capture_output=True, timeout=300)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "deflate_plan_sanitize: ok" in p.stdout.decode(), err[-3000:]
    assert "AddressSanitizer" not in err and "runtime error:" not in err
