#!/usr/bin/env python3
"""Generate tests/golden/field_checks.json from the reference's own data.

BUILD-CONTAINER ONLY (reads /root/reference as text; never runs on the GPU
box).  The five byte tables of lib/nghttp2_helper.c (VALID_HD_NAME_CHARS,
VALID_HD_VALUE_CHARS, VALID_METHOD_CHARS, VALID_PATH_CHARS,
VALID_AUTHORITY_CHARS, :346-548) are read as data -- (byte, class) pairs --
and only results are recorded:

- one_byte[c], colon_byte[c]: for the one-byte string c and for ":" + c, the
  seven results in the order of `order` (1 = the reference function returns 1:
  nghttp2_check_header_name, _header_value, _header_value_rfc9113, _method,
  _path, _authority, and nghttp2_check_nonempty_header_name(...) == 1), each
  computed as the function's documented walk over its table (:360-558);
- vectors: the strings of test_nghttp2_check_header_name / _header_value /
  _header_value_rfc9113 (tests/nghttp2_helper_test.c:161-210) as hex with
  the expectation the test asserts;
- table_sha256: sha256 of each table's 256 class bytes.

Usage: python3 tests/golden/make_field_checks.py
"""
import ast
import hashlib
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
TABLES = ["VALID_HD_NAME_CHARS", "VALID_HD_VALUE_CHARS", "VALID_METHOD_CHARS", "VALID_PATH_CHARS",
          "VALID_AUTHORITY_CHARS"]
ORDER = ["header_name", "header_value", "header_value_rfc9113", "method", "path", "authority",
         "nonempty_header_name_is_1"]


def c_byte(tok):
    tok = tok.strip()
    if tok.startswith("'"):
        return ord(ast.literal_eval(tok))
    return int(tok.rstrip("Uu"), 0)


def read_tables():
    text = open(os.path.join(REF, "lib", "nghttp2_helper.c")).read()
    out = {}
    for name in TABLES:
        start = text.index("static const uint8_t %s[256] = {" % name)
        body = text[start:text.index("};", start)]
        t = bytearray(256)
        for m in re.finditer(r"\[('(?:\\.|[^'\\])'|0x[0-9A-Fa-f]+)\]\s*=\s*(\d+)", body):
            t[c_byte(m.group(1))] = int(m.group(2))
        out[name] = bytes(t)
    return out


def results(T, s):
    name, value, method, path, auth = (T[k] for k in TABLES)
    n = s[1:] if s[:1] == b":" else s
    r_name = int(len(s) > 0 and len(n) > 0 and all(name[c] == 1 for c in n))
    r_value = int(all(value[c] for c in s))
    r_9113 = int(len(s) == 0 or (s[0] not in b" \t" and s[-1] not in b" \t" and r_value == 1))
    r_method = int(len(s) > 0 and all(method[c] for c in s))
    r_path = int(all(path[c] for c in s))
    r_auth = int(all(auth[c] for c in s))
    r_lower = int(all(name[c] == 1 for c in s))
    return [r_name, r_value, r_9113, r_method, r_path, r_auth, r_lower]


def test_vectors():
    text = open(os.path.join(REF, "tests", "nghttp2_helper_test.c")).read()
    out = []
    for fn in ("header_name", "header_value", "header_value_rfc9113"):
        start = text.index("void test_nghttp2_check_%s(void) {" % fn)
        body = text[start:text.index("\n}\n", start)]
        arrays = {}
        for m in re.finditer(r"static const uint8_t (\w+)\[\] = \{(.*?)\};", body, re.S):
            vals = bytes(c_byte(t) for t in m.group(2).split(",") if t.strip())
            arrays[m.group(1)] = vals[:-1]  # nghttp2_strlen_lit: without the terminator
        for m in re.finditer(r"assert_(true|false)\(check_%s\((.*?)\)\);" % fn, body):
            arg = m.group(2).strip()
            s = arrays[arg] if arg in arrays else ast.literal_eval("b" + arg)
            out.append([fn, s.hex(), 1 if m.group(1) == "true" else 0])
    return out


def main():
    T = read_tables()
    data = {"source": "lib/nghttp2_helper.c:346-558 (tables and walks), "
                      "tests/nghttp2_helper_test.c:161-210 (vectors)",
            "order": ORDER,
            "one_byte": [results(T, bytes([c])) for c in range(256)],
            "colon_byte": [results(T, b":" + bytes([c])) for c in range(256)],
            "vectors": test_vectors(),
            "table_sha256": {k: hashlib.sha256(T[k]).hexdigest() for k in TABLES}}
    for fn, hx, want in data["vectors"]:  # the walks above against the reference's own expectations
        assert results(T, bytes.fromhex(hx))[ORDER.index(fn)] == want, (fn, hx)
    assert len(data["vectors"]) == 7 + 7 + 11, len(data["vectors"])
    path = os.path.join(HERE, "field_checks.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=0)
        f.write("\n")
    print("wrote %s: %d vectors" % (path, len(data["vectors"])))


if __name__ == "__main__":
    main()
