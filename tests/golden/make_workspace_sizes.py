#!/usr/bin/env python3
"""Record tests/golden/workspace_sizes.json: what the four workspace size
functions of a built library answer.  The sizes are ABI (callers allocate what
the functions return), so the fixture is recorded once, from the library of the
commit before the layouts were rewritten on hdhost::Carve (3a0de59; the device
deflaters' from 8b29492, the commit that added them), and a later build is held
to it byte for byte (tests/test_workspace_sizes.py).  No GPU call is made.

Usage: python3 tests/golden/make_workspace_sizes.py [libnghttp2_amd_hd.so] [commit] [deflate commit]
(the commits name where the library's layouts come from: the device deflaters'
sizes, and the other three)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NCONN, TABLE_BYTES, OPS_CAP, NBLOCKS = (1, 2, 65), (4096, 8192), (0, 1, 63, 64, 65), (1, 2, 3, 64)
NVA_CAP = (0, 1, 3, 4, 63, 64, 255, 256, 257, 2**31 - 1, 2**31)
PARSE_N = (0, 1, 3, 4, 64)
DEFLATE_NVA_CAP, DEFLATE_ARENA, DEFLATE_NBLOCKS = (0, 1, 63, 64, 65), (0, 31, 32, 33), (1, 64)


def sizes(L):
    """{function: [[arguments..., size]]} of the library L."""
    u32, u64, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nghttp2_amd_hd_dev_inflate_workspace_size.argtypes = [u32, u32, sz, u32]
    L.nghttp2_amd_hd_dev_inflate_workspace_size.restype = sz
    L.nghttp2_amd_hd_dev_fields_http_workspace_size.argtypes = [sz, u32]
    L.nghttp2_amd_hd_dev_fields_http_workspace_size.restype = sz
    L.nghttp2_amd_hd_parse_blocks_bound.argtypes = [u64, u32] + [ctypes.POINTER(sz)] * 4
    L.nghttp2_amd_hd_dev_deflate_workspace_size.argtypes = [u32, u32, sz, sz, u32]
    L.nghttp2_amd_hd_dev_deflate_workspace_size.restype = sz

    def parse_ws(n):
        ws = sz()
        assert L.nghttp2_amd_hd_parse_blocks_bound(0, n, None, None, None, ctypes.byref(ws)) == 0
        return ws.value
    return {
        "nghttp2_amd_hd_dev_inflate_workspace_size": [
            [c, t, o, n, L.nghttp2_amd_hd_dev_inflate_workspace_size(c, t, o, n)]
            for c in NCONN for t in TABLE_BYTES for o in OPS_CAP for n in NBLOCKS],
        "nghttp2_amd_hd_dev_fields_http_workspace_size": [
            [c, L.nghttp2_amd_hd_dev_fields_http_workspace_size(c, 1)] for c in NVA_CAP],
        "nghttp2_amd_hd_parse_blocks_bound.ws_bytes": [[n, parse_ws(n)] for n in PARSE_N],
        "nghttp2_amd_hd_dev_deflate_workspace_size": [
            [c, t, v, a, n, L.nghttp2_amd_hd_dev_deflate_workspace_size(c, t, v, a, n)]
            for c in NCONN for t in TABLE_BYTES for v in DEFLATE_NVA_CAP for a in DEFLATE_ARENA
            for n in DEFLATE_NBLOCKS],
    }


def main():
    repo = os.path.dirname(os.path.dirname(HERE))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(repo, "nghttp2_amd", "lib", "libnghttp2_amd_hd.so")
    data = {"recorded_from": sys.argv[2] if len(sys.argv) > 2 else "3a0de59",
            "deflate_recorded_from": sys.argv[3] if len(sys.argv) > 3 else "8b29492", **sizes(ctypes.CDLL(path))}
    out = os.path.join(HERE, "workspace_sizes.json")
    with open(out, "w") as f:  # one case a line
        f.write("{\n" + ",\n".join(
            '"%s": %s' % (k, json.dumps(v) if isinstance(v, str) else "[\n" + ",\n".join(json.dumps(r) for r in v) + "\n]")
            for k, v in data.items()) + "\n}\n")
    print("wrote %s from %s" % (out, path))


if __name__ == "__main__":
    main()
