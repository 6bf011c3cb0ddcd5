"""nghttp2_amd_hd_dev_fields_http without a GPU: the declaration and the
export, the workspace size against the header's layout, and hd_http.h's step
(now compiled for the device too) still held to the reference's recorded
verdicts through the host entry points."""
import os
import re
import subprocess

from nghttp2_amd import hd as H
from tests import http_fields_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nghttp2_amd_hd_dev_fields_http", "nghttp2_amd_hd_dev_fields_http_workspace_size",
         "nghttp2_amd_hd_dev_fields_http_totals")


def test_header_declares_and_library_exports():
    with open(os.path.join(REPO, "include", "nghttp2_amd_hd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"NGHTTP2_AMD_EXTERN\s+\w+\s+%s\(" % name, header), name
    for bit in ("NGHTTP2_AMD_HD_DEV_FIELDS_NOT_REPLAYED", "NGHTTP2_AMD_HD_DEV_FIELDS_ARENA_SHORT"):
        assert "#define " + bit in header
    out = subprocess.run(["nm", "-D", "--defined-only", H.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in exported, name
    L = H._replay_lib()
    assert L.nghttp2_amd_hd_dev_fields_http(*([None, 0, None, 0, None, None, None, 0] + [None] * 6 + [None, 0, None])) == 0
    assert L.nghttp2_amd_hd_dev_fields_http_totals(None, None, None) == H.NGHTTP2_ERR_INVALID_ARGUMENT


def test_step_still_gives_the_recorded_verdicts():
    """tests/golden/http_fields.json through nghttp2_amd_hd_http_on_header and
    the block ends: the host compiles hd_http.h's step from the text the
    kernel compiles."""
    g = C.golden()
    mask = g["flags_compared"]
    for i, b in enumerate(g["blocks"]):
        st = H.HttpState(*b["state"])
        mode, verdicts, stopped = b["mode"], [], False
        for n, v in b["fields"]:
            name, value = bytes.fromhex(n), bytes.fromhex(v)
            if stopped:
                verdicts.append(H.HTTP_NOT_EXAMINED)
                continue
            f, num = H.http_facts(value)
            rv = H.http_on_header(st, mode, name, len(value), H.lookup_token(name), H.check_field(name),
                                  H.check_field(value), f, num)
            verdicts.append(rv)
            stopped = rv == H.NGHTTP2_ERR_HTTP_HEADER
        assert verdicts == b["verdicts"], i
        end = None
        if not stopped and not mode & H.HTTP_MODE_TRAILER:
            end = H.http_on_request_headers(st, mode) if mode & H.HTTP_MODE_REQUEST else H.http_on_response_headers(st)
        assert end == b["end"], i
        assert (st.http_flags & mask, st.status_code, st.content_length) == \
            (b["state_after"][0] & mask, *b["state_after"][1:]), i


def _round16(x):
    return (x + 15) // 16 * 16


def documented(c):
    """The header's layout: the totals word, the three views, the values'
    numbers and facts, the tokens and the masks, each rounded up to 16."""
    parts = [16, 4 * (2 * c + 1), 4 * 2 * c, 4 * (c + 1), 4 * c, 4 * (c + 1), 4 * c, 8 * c, 4 * c, 4 * c, 2 * c]
    return sum(_round16(p) for p in parts)


def test_workspace_size():
    size = H._replay_lib().nghttp2_amd_hd_dev_fields_http_workspace_size
    caps = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 1000, 4097, 1 << 20]
    for c in caps:
        views = 4 * (2 * c + 1) + 8 * c + 2 * (4 * (c + 1) + 4 * c)
        assert size(c, 1) == documented(c) >= views + 12 * c + 2 * c + 4 * c + 16, c
        for nb in (1, 64, 65, 100000):  # monotone in both arguments
            assert size(c, nb) >= size(c, 1)
            assert size(c + 1, nb) >= size(c, nb)
    assert [size(c, 7) for c in caps] == sorted(size(c, 7) for c in caps)
