"""The batches of tests/string_batches.py that the GPU tests of the
string walk run (tests/test_string_walk_gpu.py), on the CPU: the shapes are
the ones they claim to be, every offset and length stays inside the pool
where a string is examined, and the restatements take every string."""
import numpy as np
import pytest

from tests import field_checks_ref as CR
from tests import http_fields_ref as HR
from tests import string_batches as B


@pytest.mark.parametrize("length", B.EXIT_LENGTHS)
def test_exit_batches_cross_one_round_and_one_trip(length):
    batches = B.exit_batches(length, b"0", (b"@", b"7"), b"@")
    chunks = set()
    for strings in batches:
        assert len(strings) == 64 and sum(len(s) == length for s in strings) == 1
        assert all(len(s) <= 3 for s in strings if len(s) != length)
        pool, off = B.lay_out(strings)
        assert int(off[-1]) <= pool.size - 16
        k = [len(s) for s in strings].index(length)
        assert int(off[k]) in B.EXIT_SHIFTS
        chunks.add(B.wave_chunks(strings))
    # the fewest chunks a batch of this length spans: at 64 and 128 the loop
    # ends after a first round, past them it goes on
    assert min(chunks) == {1008: 64, 1024: 65, 1040: 66, 2032: 128, 2048: 129, 2064: 130}[length]
    seen = {s for strings in batches for s in strings}
    for s in seen:
        assert 0 <= CR.mask(s) < 0x80
        f, n = HR.facts(s)
        assert f != HR.FACT_INVALID and n >= -1


def test_not_examined_reads_inside_the_pool():
    strings = [b"cookie", b"etag", b"42", b":path", b"007", b"host", b"HEAD", b"age", b"trailers", b"https", b"a b",
               b"0"]
    pool, off, ln, exam = B.not_examined(strings)
    assert len(off) == len(ln) + 1 == len(exam) + 1 == 15
    for i, s in enumerate(exam):
        o0, o1, l = int(off[i]), int(off[i + 1]), int(ln[i])
        valid = o0 <= o1 and 0 <= l <= o1 - o0  # the kernels' rule (csrc/hd_string_walk.h)
        assert valid == (s is not None)
        if valid:
            assert o0 + l <= pool.size - 16 and pool[o0:o0 + l].tobytes() == s
    assert [i for i, s in enumerate(exam) if s is None] == [1, 3, 5, 7, 12, 13]
