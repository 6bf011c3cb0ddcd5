"""The workspace sizes are ABI: callers allocate what the *_workspace_size
functions return.  tests/golden/workspace_sizes.json holds what the library
answered before the layouts were rewritten on one carver (hdhost::Carve,
recorded by tests/golden/make_workspace_sizes.py); every size must still be
that, to the byte.  The counts are those at which a misplaced rounding or a
lost `+ 1` shows.  No GPU."""
import itertools
import json
import os

from nghttp2_amd import hd as H
from tests.golden import make_workspace_sizes as M

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")) as f:
    GOLDEN = json.load(f)


def test_fixture_holds_the_cases():
    rows = GOLDEN["nghttp2_amd_hd_dev_inflate_workspace_size"]
    assert [tuple(r[:4]) for r in rows] == list(itertools.product((1, 2, 65), (4096, 8192), (0, 1, 63, 64, 65),
                                                                  (1, 2, 3, 64)))
    assert [r[0] for r in GOLDEN["nghttp2_amd_hd_dev_fields_http_workspace_size"]] == \
        [0, 1, 3, 4, 63, 64, 255, 256, 257, 2**31 - 1, 2**31]
    assert [r[0] for r in GOLDEN["nghttp2_amd_hd_parse_blocks_bound.ws_bytes"]] == [0, 1, 3, 4, 64]
    rows = GOLDEN["nghttp2_amd_hd_dev_deflate_workspace_size"]
    assert [tuple(r[:5]) for r in rows] == list(itertools.product((1, 2, 65), (4096, 8192), (0, 1, 63, 64, 65),
                                                                  (0, 31, 32, 33), (1, 64)))


def test_sizes_are_the_recorded_ones():
    got = M.sizes(H.lib())
    for name, rows in got.items():
        assert len(rows) == len(GOLDEN[name]), name
        for g, want in zip(rows, GOLDEN[name]):
            assert g == want, (name, g, want)
