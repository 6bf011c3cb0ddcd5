#!/usr/bin/env python3
"""Generate tests/golden/http_fields.json from the reference's own functions.

BUILD-CONTAINER ONLY (compiles /root/reference sources; never runs on the GPU
box).  A small C driver of our own is written into a temporary directory and
compiled together with the reference's lib/nghttp2_http.c (included as text,
so its static helpers can be called), nghttp2_helper.c and what those need;
nghttp2ver.h is made from its .in template.  The binary stays in the
temporary directory.  The driver calls nghttp2_http_on_header and the two
block-end functions on hand-built nghttp2_stream / nghttp2_session /
nghttp2_frame values over the corpus below and records only results:

- blocks: per block its mode, the state before it and its fields (name and
  value as hex) -- the corpus -- and the verdict per field, the state after
  the block and the block-end result (null when it is not run: after a stream
  error, as lib/nghttp2_session.c:3643-3664 stops examining the stream, and
  for a trailer).  Tokens come from the product's own pinned lookup_token
  (tests/golden/name_tokens.json pins that one).
- one_byte[c]: [facts, number] of the one-byte string c, each fact computed by
  the reference's static helper (check_authority, check_scheme, memieq, lws,
  parse_uint) or, for the comparisons the reference writes inline, by the
  same expression in the driver.
- uints: parse_uint at INT64_MAX, INT64_MAX + 1, 20 digits and more.
- authority_sha256: sha256 of the private VALID_AUTHORITY_CHARS table.

The priority field's structured value is outside the product's scope, so the
corpus carries only priority values that parse (or that fail the byte check),
and http_flags are compared without NGHTTP2_HTTP_FLAG_PRIORITY.

Usage: python3 tests/golden/make_http_fields.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

REQ, PUSH, TRAILER, CONNPROTO, NOWS = 1, 2, 4, 8, 0x10
FRESH = (0, -1, -1)
METH_CONNECT, METH_HEAD, EXPECT_FINAL = 0x80, 0x100, 0x4000

REQ4 = [(":scheme", "https"), (":method", "GET"), (":authority", "localhost"), (":path", "/")]


def B(mode, fields, state=FRESH):
    return {"mode": mode, "state": list(state),
            "fields": [[n.encode("latin-1").hex() if isinstance(n, str) else bytes(n).hex(),
                        v.encode("latin-1").hex() if isinstance(v, str) else bytes(v).hex()]
                       for n, v in fields]}


def corpus():
    c = []
    # ---- tests/nghttp2_session_test.c:10849-12200, the header-only vectors
    # test_nghttp2_http_mandatory_headers: responses
    for f in ([("server", "foo")],
              [(":status", "200"), (":status", "200")],
              [(":status", "200"), (":scheme", "https")],
              [("server", "foo"), (":status", "200")],
              [(":status", "2000")],
              [(":status", "200"), ("content-length", "-1")],
              [(":status", "200"), ("content-length", "0"), ("content-length", "0")],
              [(":status", "200"), ("connection", "close")],
              [(":status", "100"), ("content-length", "0")],
              [(":status", "204"), ("content-length", "0")],
              [(":status", "204"), ("content-length", "100")],
              [(":status", "101")],
              [(":status", "200"), ("host", "/localhost")],
              [(":status", "022")],
              [(":status", "20")]):
        c.append(B(0, f))
    # requests
    for f in ([(":scheme", "https"), (":method", "GET"), (":authority", "localhost")],
              [(":method", "CONNECT"), (":scheme", "https"), (":path", "/"), (":authority", "localhost")],
              [(":scheme", "https"), (":path", "/"), (":method", "CONNECT"), (":authority", "localhost")],
              REQ4 + [(":path", "/")],
              [(":scheme", "https"), (":method", "POST"), (":authority", "localhost"), (":path", "/"),
               ("content-length", "-1")],
              [(":scheme", "https"), (":method", "POST"), (":authority", "localhost"), (":path", "/"),
               ("content-length", "0"), ("content-length", "0")],
              REQ4 + [("connection", "close")],
              [(":scheme", "https"), (":method", "GET"), (":authority", "\r\nlocalhost"), (":path", "/")],
              [(":scheme", "https"), (":method", "GET"), ("foo", "\r\n"), (":authority", "localhost"),
               (":path", "/")],
              [(":path", "*"), (":scheme", "https"), (":authority", "localhost"), (":method", "GET")],
              [(":scheme", "https"), (":authority", "localhost"), (":method", "GET"), (":path", "*")],
              [(":path", "*"), (":scheme", "https"), (":authority", "localhost"), (":method", "OPTIONS")],
              [(":scheme", "https"), (":authority", "localhost"), (":method", "OPTIONS"), (":path", "*")],
              [(":method", "CONNECT"), (":authority", "localhost")]):
        c.append(B(REQ, f))
    connectproto = [(":scheme", "https"), (":path", "/"), (":method", "CONNECT"), (":authority", "localhost"),
                    (":protocol", "websocket")]
    c.append(B(REQ, connectproto))
    c.append(B(REQ | CONNPROTO, connectproto))
    c.append(B(REQ | CONNPROTO, [(":scheme", "https"), (":path", "/"), (":method", "GET"),
                                 (":authority", "localhost"), (":protocol", "websocket")]))
    c.append(B(REQ | CONNPROTO, [(":scheme", "https"), (":method", "CONNECT"), (":authority", "localhost"),
                                 (":protocol", "websocket")]))
    c.append(B(REQ | CONNPROTO, [(":scheme", "http"), (":path", "/"), (":method", "CONNECT"),
                                 ("host", "localhost"), (":protocol", "websocket")]))
    # test_nghttp2_http_content_length / _mismatch / _non_final_response
    c.append(B(0, [(":status", "200"), ("te", "trailers"), ("content-length", "9000000000")]))
    c.append(B(REQ, [(":path", "/"), (":method", "PUT"), (":scheme", "https"), ("te", "trailers"),
                     ("host", "localhost"), ("content-length", "9000000000")]))
    c.append(B(REQ, [(":path", "/"), (":method", "PUT"), (":authority", "localhost"), (":scheme", "https"),
                     ("content-length", "20")]))
    c.append(B(0, [(":status", "200"), ("content-length", "20")]))
    c.append(B(0, [(":status", "100")]))
    c.append(B(0, [(":status", "200"), ("content-length", "5")], (EXPECT_FINAL, -1, -1)))
    # test_nghttp2_http_trailer_headers, _ignore_regular_header
    c.append(B(REQ | TRAILER, [("foo", "bar")], (0x2E4F, -1, -1)))
    c.append(B(REQ | TRAILER, [(":path", "/")], (0x2E4F, -1, -1)))
    c.append(B(REQ, [(":authority", "localhost"), (":scheme", "https"), (":path", "/"), (":method", "GET"),
                     ("foo", "\x00zzz"), ("bar", "buzz")]))
    # test_nghttp2_http_ignore_content_length, _record_request_method
    c.append(B(0, [(":status", "304"), ("content-length", "20")]))
    c.append(B(REQ, [(":authority", "localhost"), (":method", "CONNECT"), ("content-length", "999999")]))
    c.append(B(0, [(":status", "200"), ("content-length", "0")], (METH_CONNECT, -1, -1)))
    c.append(B(0, [(":status", "200"), ("content-length", "9999")], (METH_CONNECT, -1, -1)))
    # test_nghttp2_http_push_promise, _head_method_upgrade_workaround
    c.append(B(REQ | PUSH, [(":method", "GET")]))
    c.append(B(REQ | PUSH, REQ4))
    c.append(B(PUSH, [(":status", "200")], (0, -1, -1)))
    c.append(B(0, [(":status", "200"), ("content-length", "1000000007")], (0x400, -1, -1)))
    c.append(B(0, [(":status", "200"), ("content-length", "1000000007")], (METH_HEAD, -1, -1)))
    # test_nghttp2_http_no_rfc9113_leading_and_trailing_ws_validation
    ws = [(":path", "/"), (":method", "GET"), (":authority", "localhost"), (":scheme", "https"),
          ("foo", "bar ")]
    c.append(B(REQ, ws))
    c.append(B(REQ | NOWS, ws))

    # ---- every case label, early return and mode bit not met above
    # the name checks of nghttp2_http_on_header
    c.append(B(REQ, REQ4 + [("", "empty-name"), ("ok", "1")]))
    c.append(B(REQ, [("", "x")] + REQ4))                      # an empty name disallows pseudo-headers
    c.append(B(REQ, REQ4 + [("Upper", "x"), ("later", "y")]))  # 2: upper case
    c.append(B(REQ, REQ4 + [("b\x00d", "x"), ("later", "y")]))   # 0: another bad byte
    c.append(B(REQ, REQ4 + [("b dU", "x")]))                   # the first bad byte decides: 0
    c.append(B(REQ, REQ4 + [("bU d", "x")]))                   # ... 2
    c.append(B(REQ, REQ4 + [("a:b", "x")]))                    # ':' inside a name
    c.append(B(REQ, [(":unknown", "x")] + REQ4))
    c.append(B(0, [(":unknown", "x")]))
    c.append(B(REQ, REQ4 + [(":status", "200")]))
    # :authority, host
    c.append(B(REQ, [(":authority", "user@host")]))
    c.append(B(REQ, [(":authority", "")]))
    c.append(B(REQ, [(":authority", "a"), (":authority", "b")]))
    c.append(B(REQ, [(":scheme", "https"), (":method", "GET"), (":path", "/"), ("host", "user@host")]))
    c.append(B(REQ, [(":scheme", "https"), (":method", "GET"), (":path", "/"), ("host", "[::1]:8080")]))
    c.append(B(REQ, [(":scheme", "https"), (":method", "GET"), (":path", "/"), ("host", "")]))
    c.append(B(REQ, [(":scheme", "https"), (":method", "GET"), (":path", "/"), ("host", "a"), ("host", "b")]))
    c.append(B(REQ, REQ4 + [("host", "localhost")]))
    # :method
    for m in ("HEAD", "HEAd", "OPTIONS", "OPTIONs", "CONNECTS", "CONNECt", "DELETET", "PATCHES", "G T", ""):
        c.append(B(REQ, [(":scheme", "https"), (":authority", "localhost"), (":path", "/"), (":method", m)]))
    c.append(B(REQ, [(":method", "GET"), (":method", "GET")]))
    c.append(B(REQ | PUSH, [(":method", "CONNECT"), (":authority", "localhost")]))
    c.append(B(REQ | PUSH, [(":scheme", "https"), (":authority", "localhost"), (":path", "/"),
                            (":method", "HEAD"), ("content-length", "7")]))
    # :path
    for p in ("/a b", "", "*", "**", "x", "/\xff"):
        c.append(B(REQ, [(":scheme", "http"), (":method", "GET"), (":authority", "localhost"), (":path", p)]))
    c.append(B(REQ, [(":scheme", "ftp"), (":method", "GET"), (":authority", "localhost"), (":path", "x")]))
    # :scheme
    for s in ("HTTP", "hTTpS", "httpx", "h", "1http", "a+b-c.d9", "ht tp", "", "http:"):
        c.append(B(REQ, [(":scheme", s), (":method", "GET"), (":authority", "localhost"), (":path", "rel")]))
    c.append(B(REQ, [(":scheme", "a"), (":scheme", "b")]))
    # :protocol
    base = [(":scheme", "https"), (":path", "/"), (":method", "CONNECT"), (":authority", "localhost")]
    for mode in (REQ | CONNPROTO, REQ | CONNPROTO | NOWS):
        for v in ("websocket", " websocket", "websocket\t", " \t ", "", "web\x01socket", "a b"):
            c.append(B(mode, base + [(":protocol", v)]))
    c.append(B(REQ | CONNPROTO, base + [(":protocol", "a"), (":protocol", "b")]))
    c.append(B(REQ | PUSH | CONNPROTO, [(":scheme", "https"), (":path", "/"), (":method", "GET"),
                                        (":authority", "localhost"), (":protocol", "websocket")]))
    # content-length (request)
    for v in ("", "0", "007", "9223372036854775807", "9223372036854775808", "12a", " 1", "1 ",
              "00000000000000000000000000000042", "99999999999999999999"):
        c.append(B(REQ, REQ4 + [("content-length", v)]))
    # disallowed fields, te
    for n in ("connection", "keep-alive", "proxy-connection", "transfer-encoding", "upgrade"):
        c.append(B(REQ, REQ4 + [(n, "x"), ("after", "y")]))
        c.append(B(0, [(":status", "200"), (n, "x"), ("after", "y")]))
    for v in ("trailers", "TrAiLeRs", "trailer", "trailers ", "gzip", ""):
        c.append(B(REQ, REQ4 + [("te", v)]))
        c.append(B(0, [(":status", "200"), ("te", v)]))
    # priority (values that parse, or that fail the byte check)
    for mode in (REQ, REQ | NOWS, REQ | PUSH, REQ | TRAILER):
        st = (0x2E4F, -1, -1) if mode & TRAILER else FRESH
        lead = [] if mode & TRAILER else REQ4
        for v in ("u=3, i", "u=1", " u=1", "u=1\x01", ""):
            c.append(B(mode, lead + [("priority", v), ("x", "y")], st))
    c.append(B(0, [(":status", "200"), ("priority", " u=1")]))
    # regular fields, both whitespace rules, both directions
    for mode in (REQ, REQ | NOWS, 0, NOWS):
        lead = REQ4 if mode & REQ else [(":status", "200")]
        for v in ("", "a", " a", "a\t", "a b", "\x7f", "\x80\xff", "a\nb"):
            c.append(B(mode, lead + [("x-field", v)]))
    # :status and the response's content-length
    for v in ("200", "100", "199", "101", "099", "999", "1000", "2x0", "", "20 ", "+20"):
        c.append(B(0, [(":status", v), ("content-length", "1")]))
    for st in ("204", "304", "200", "299", "300", "103"):
        for v in ("0", "00", "5", "x", ""):
            c.append(B(0, [(":status", st), ("content-length", v)]))
            c.append(B(0, [(":status", st), ("content-length", v)], (METH_CONNECT, -1, -1)))
            c.append(B(0, [(":status", st), ("content-length", v)], (METH_HEAD, -1, -1)))
    c.append(B(0, [(":status", "204"), ("content-length", "0"), ("content-length", "0")]))
    c.append(B(0, [(":status", "200"), ("content-length", "1"), ("content-length", "1")]))
    c.append(B(0, [(":status", "200")], (METH_HEAD | 0x200, -1, -1)))
    c.append(B(0, [(":status", "200"), (":status", "200")], (EXPECT_FINAL | METH_HEAD, -1, -1)))
    c.append(B(TRAILER, [("grpc-status", "0")], (0x60, 200, -1)))
    c.append(B(TRAILER, [(":status", "200")], (0x60, 200, -1)))
    c.append(B(TRAILER, [("content-length", "4")], (0x60, 200, -1)))
    c.append(B(TRAILER, [], (0x60, 200, -1)))
    c.append(B(REQ, []))
    c.append(B(0, []))
    # the block ends
    c.append(B(REQ, [(":method", "CONNECT")]))
    c.append(B(REQ, [(":method", "CONNECT"), (":authority", "h"), (":path", "/")]))
    c.append(B(REQ, [(":method", "CONNECT"), (":authority", "h"), ("content-length", "3")]))
    c.append(B(REQ, [(":scheme", "https"), (":method", "GET"), (":path", "/")]))
    c.append(B(REQ | CONNPROTO, [(":scheme", "https"), (":path", "/"), (":method", "CONNECT"),
                                 (":protocol", "websocket"), ("host", "h")]))
    c.append(B(REQ, [(":scheme", "http"), (":method", "OPTIONS"), (":authority", "h"), (":path", "x")]))
    c.append(B(REQ | PUSH, [(":scheme", "https"), (":method", "OPTIONS"), (":authority", "h"), (":path", "*"),
                            ("content-length", "9")]))
    return c


DRIVER = r"""
/* Our own driver around the reference's nghttp2_http.c (included as text for
   its static helpers). */
#include "nghttp2_http.c"
#include <stdio.h>
#include <stdlib.h>

static size_t unhex(const char *h, uint8_t *out) {
  size_t n = 0;
  if (h[0] == '-') return 0;
  for (; h[0] && h[1]; h += 2) {
    unsigned v;
    sscanf(h, "%2x", &v);
    out[n++] = (uint8_t)v;
  }
  return n;
}

static uint32_t facts_of(const uint8_t *s, size_t len, int64_t *num) {
  uint32_t f = 0;
  if (check_authority(s, len)) f |= 0x001;
  if (check_scheme(s, len)) f |= 0x002;
  if ((len == 4 && memieq("http", s, 4)) || (len == 5 && memieq("https", s, 5))) f |= 0x004;
  if (lstreq("HEAD", s, len)) f |= 0x008;
  if (lstreq("CONNECT", s, len)) f |= 0x010;
  if (lstreq("OPTIONS", s, len)) f |= 0x020;
  if (len > 0 && s[0] == '/') f |= 0x040;
  if (len == 1 && s[0] == '*') f |= 0x080;
  if (lstrieq("trailers", s, len)) f |= 0x100;
  if (lws(s, len)) f |= 0x200;
  *num = parse_uint(s, len);
  if (*num != -1) f |= 0x400;
  return f;
}

int main(void) {
  static char name_h[400000], value_h[400000];
  static uint8_t name_b[200000], value_b[200000];
  char cmd[16];
  nghttp2_session *session = calloc(1, sizeof(nghttp2_session));
  while (scanf("%15s", cmd) == 1) {
    if (cmd[0] == 'S') { /* S hex: the facts of one string */
      int64_t num;
      size_t n;
      uint32_t f;
      scanf("%399999s", value_h);
      n = unhex(value_h, value_b);
      f = facts_of(value_b, n, &num);
      printf("S %u %lld\n", f, (long long)num);
      continue;
    }
    if (cmd[0] == 'T') { /* the private authority table */
      int i;
      printf("T");
      for (i = 0; i < 256; ++i) printf(" %d", VALID_AUTHORITY_CHARS[i]);
      printf("\n");
      continue;
    }
    /* B mode flags status cl nfields, then nfields lines "token namehex valuehex" */
    unsigned mode, flags;
    int status, nf, i, stopped = 0, end = 2;
    long long cl;
    nghttp2_stream stream;
    nghttp2_frame frame;
    scanf("%u %u %d %lld %d", &mode, &flags, &status, &cl, &nf);
    memset(&stream, 0, sizeof(stream));
    memset(&frame, 0, sizeof(frame));
    stream.stream_id = (mode & 2) ? 2 : 1;
    stream.http_flags = flags;
    stream.status_code = status;
    stream.content_length = cl;
    stream.http_extpri = NGHTTP2_EXTPRI_DEFAULT_URGENCY;
    if (mode & 0x10) stream.flags |= NGHTTP2_STREAM_FLAG_NO_RFC9113_LEADING_AND_TRAILING_WS_VALIDATION;
    session->server = (mode & 1) ? 1 : 0;
    session->pending_enable_connect_protocol = (mode & 8) ? 1 : 0;
    frame.hd.type = ((mode & 1) && (mode & 2)) ? NGHTTP2_PUSH_PROMISE : NGHTTP2_HEADERS;
    frame.hd.stream_id = 1;
    printf("B");
    for (i = 0; i < nf; ++i) {
      int token;
      nghttp2_rcbuf nb, vb;
      nghttp2_hd_nv nv;
      scanf("%d %399999s %399999s", &token, name_h, value_h);
      if (stopped) {
        printf(" 1");
        continue;
      }
      memset(&nb, 0, sizeof(nb));
      memset(&vb, 0, sizeof(vb));
      nb.base = name_b;
      nb.len = unhex(name_h, name_b);
      name_b[nb.len] = 0;
      vb.base = value_b;
      vb.len = unhex(value_h, value_b);
      value_b[vb.len] = 0;
      nv.name = &nb;
      nv.value = &vb;
      nv.token = token;
      nv.flags = 0;
      {
        int rv = nghttp2_http_on_header(session, &stream, &frame, &nv, (mode & 4) ? 1 : 0);
        printf(" %d", rv);
        if (rv == NGHTTP2_ERR_HTTP_HEADER) stopped = 1;
      }
    }
    if (!stopped && !(mode & 4))
      end = (mode & 1) ? nghttp2_http_on_request_headers(&stream, &frame)
                       : nghttp2_http_on_response_headers(&stream);
    printf(" | %u %d %lld %d\n", stream.http_flags, (int)stream.status_code, (long long)stream.content_length,
           end);
  }
  return 0;
}
"""


def build_driver(tmp):
    inc = os.path.join(tmp, "nghttp2")
    os.makedirs(inc)
    ver = open(os.path.join(REF, "lib", "includes", "nghttp2", "nghttp2ver.h.in")).read()
    ver = ver.replace("@PACKAGE_VERSION@", "0.0.0").replace("@PACKAGE_VERSION_NUM@", "0x000000")
    open(os.path.join(inc, "nghttp2ver.h"), "w").write(ver)
    open(os.path.join(tmp, "driver.c"), "w").write(DRIVER)
    exe = os.path.join(tmp, "driver")
    lib = os.path.join(REF, "lib")
    srcs = [os.path.join(tmp, "driver.c")] + [os.path.join(lib, f) for f in
                                              ("nghttp2_helper.c", "sfparse.c", "nghttp2_extpri.c", "nghttp2_mem.c")]
    subprocess.run(["gcc", "-O1", "-w", "-DNGHTTP2_STATICLIB", "-I", tmp, "-I", lib,
                    "-I", os.path.join(lib, "includes"), "-o", exe] + srcs, check=True)
    return exe


def main():
    from nghttp2_amd import hd as H  # the product's pinned lookup_token
    blocks = corpus()
    specials = [b"9223372036854775807", b"9223372036854775808", b"18446744073709551616",
                b"99999999999999999999", b"00009223372036854775807", b"0" * 1000 + b"7", b"0" * 40]
    lines = []
    for b in blocks:
        lines.append("B %d %d %d %d %d" % (b["mode"], b["state"][0], b["state"][1], b["state"][2],
                                           len(b["fields"])))
        for n, v in b["fields"]:
            lines.append("%d %s %s" % (H.lookup_token(bytes.fromhex(n)), n or "-", v or "-"))
    for c in range(256):
        lines.append("S %02x" % c)
    for s in specials:
        lines.append("S " + s.hex())
    lines.append("T")
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                             check=True).stdout.splitlines()
    assert len(out) == len(blocks) + 256 + len(specials) + 1, len(out)
    for b, line in zip(blocks, out):
        assert line.startswith("B"), line
        left, right = line[1:].split("|")
        b["verdicts"] = [int(x) for x in left.split()]
        fl, st, cl, end = (int(x) for x in right.split())
        b["state_after"] = [fl, st, cl]
        b["end"] = None if end == 2 else end
        assert len(b["verdicts"]) == len(b["fields"])
    rest = out[len(blocks):]
    sres = [[int(x) for x in line.split()[1:]] for line in rest[:256 + len(specials)]]
    table = bytes(int(x) for x in rest[-1].split()[1:])
    assert len(table) == 256
    data = {"source": "lib/nghttp2_http.c:41-511 through a driver (nghttp2_http_on_header, "
                      "nghttp2_http_on_request_headers, nghttp2_http_on_response_headers and the static "
                      "helpers); tests/nghttp2_session_test.c:10849-12200 (the header-only vectors)",
            "flags_compared": 0xFFFFFFFF & ~0x10000,
            "blocks": blocks,
            "one_byte": sres[:256],
            "uints": [[s.hex(), r[0], r[1]] for s, r in zip(specials, sres[256:])],
            "authority_sha256": hashlib.sha256(table).hexdigest()}
    path = os.path.join(HERE, "http_fields.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=0)
        f.write("\n")
    print("wrote %s: %d blocks" % (path, len(blocks)))


if __name__ == "__main__":
    main()
