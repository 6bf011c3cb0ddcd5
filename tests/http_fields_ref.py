"""nghttp2_http_on_header and its helpers (lib/nghttp2_http.c:41-511) restated
in Python from the grammars they implement: the checker of
nghttp2_amd_hd_http_facts, nghttp2_amd_hd_http_facts_batch, the host step
(nghttp2_amd_hd_http_on_header and the two block ends) and the _http inflate.
tests/golden/http_fields.json (results recorded from the reference's own
functions, tests/golden/make_http_fields.py) pins it.

Unlike the library, this works on the bytes: every test of the reference is
written out over the value itself."""
import hashlib
import string

from tests import field_checks_ref as FC

FACT_AUTHORITY, FACT_SCHEME, FACT_SCHEME_HTTP, FACT_METH_HEAD = 0x001, 0x002, 0x004, 0x008
FACT_METH_CONNECT, FACT_METH_OPTIONS, FACT_PATH_SLASH, FACT_PATH_ASTERISK = 0x010, 0x020, 0x040, 0x080
FACT_TE_TRAILERS, FACT_LWS, FACT_UINT, FACT_INVALID = 0x100, 0x200, 0x400, 0x80000000

FLAG__AUTHORITY, FLAG__PATH, FLAG__METHOD, FLAG__SCHEME, FLAG_HOST, FLAG__STATUS = 1, 2, 4, 8, 0x10, 0x20
FLAG_REQ_HEADERS = FLAG__METHOD | FLAG__PATH | FLAG__SCHEME
FLAG_PSEUDO_HEADER_DISALLOWED = 0x40
FLAG_METH_CONNECT, FLAG_METH_HEAD, FLAG_METH_OPTIONS, FLAG_METH_UPGRADE_WORKAROUND = 0x80, 0x100, 0x200, 0x400
FLAG_METH_ALL = FLAG_METH_CONNECT | FLAG_METH_HEAD | FLAG_METH_OPTIONS | FLAG_METH_UPGRADE_WORKAROUND
FLAG_PATH_REGULAR, FLAG_PATH_ASTERISK, FLAG_SCHEME_HTTP = 0x800, 0x1000, 0x2000
FLAG_EXPECT_FINAL_RESPONSE, FLAG__PROTOCOL, FLAG_PRIORITY, FLAG_BAD_PRIORITY = 0x4000, 0x8000, 0x10000, 0x20000
# what the library keeps of http_flags (the priority field's parse is the caller's)
FLAGS_COMPARED = 0xFFFFFFFF & ~FLAG_PRIORITY

MODE_REQUEST, MODE_PUSH, MODE_TRAILER, MODE_CONNECT_PROTOCOL, MODE_NO_RFC9113_WS = 1, 2, 4, 8, 0x10

IGN, REMOVE, ERR, MESSAGING, HEADER_COMP = -105, -106, -531, -532, -523
NOT_EXAMINED = 1
INT64_MAX = (1 << 63) - 1

_ALPHA = frozenset(string.ascii_letters.encode())
_DIGIT = frozenset(string.digits.encode())
# lib/nghttp2_http.c's own authority table: RFC 3986 3.2 without userinfo's "@"
HTTP_AUTHORITY = FC.AUTHORITY - frozenset(b"@")
# RFC 3986 3.1: scheme = ALPHA *( ALPHA / DIGIT / "+" / "-" / "." )
SCHEME_TAIL = _ALPHA | _DIGIT | frozenset(b"+-.")

# NGHTTP2_TOKEN_* (lib/nghttp2_hd.h)
TOKENS = {b":authority": 0, b":method": 1, b":path": 3, b":scheme": 5, b":status": 7,
          b"content-length": 27, b"host": 37, b"transfer-encoding": 56, b"te": 61, b"connection": 62,
          b"keep-alive": 63, b"proxy-connection": 64, b"upgrade": 65, b":protocol": 66, b"priority": 67}
DISALLOWED = (b"connection", b"keep-alive", b"proxy-connection", b"transfer-encoding", b"upgrade")


def check_authority(s):
    return all(c in HTTP_AUTHORITY for c in s)


def check_scheme(s):
    return len(s) > 0 and s[0] in _ALPHA and all(c in SCHEME_TAIL for c in s[1:])


def lws(s):
    return all(c in b" \t" for c in s)


def parse_uint(s):
    if not s or any(c not in _DIGIT for c in s):
        return -1
    d = s.lstrip(b"0") or b"0"  # leading zeros never overflow
    if len(d) > 19:  # 10^19 > INT64_MAX
        return -1
    n = int(d)
    return n if n <= INT64_MAX else -1


def parse_status_code(s):
    if len(s) != 3 or any(c not in _DIGIT for c in s) or s[0:1] == b"0":
        return -1
    return int(s)


def facts(s):
    """(NGHTTP2_AMD_HTTP_FACT_* bits, parse_uint's value or -1) of one string."""
    s = bytes(s)
    f = 0
    if check_authority(s):
        f |= FACT_AUTHORITY
    if check_scheme(s):
        f |= FACT_SCHEME
    if s.lower() in (b"http", b"https"):
        f |= FACT_SCHEME_HTTP
    f |= {b"HEAD": FACT_METH_HEAD, b"CONNECT": FACT_METH_CONNECT, b"OPTIONS": FACT_METH_OPTIONS}.get(s, 0)
    if s[:1] == b"/":
        f |= FACT_PATH_SLASH
    if s == b"*":
        f |= FACT_PATH_ASTERISK
    if s.lower() == b"trailers":
        f |= FACT_TE_TRAILERS
    if lws(s):
        f |= FACT_LWS
    n = parse_uint(s)
    if n != -1:
        f |= FACT_UINT
    return f, n


def authority_table_sha256():
    return hashlib.sha256(bytes(int(c in HTTP_AUTHORITY) for c in range(256))).hexdigest()


def token_of(name):
    """lookup_token for the names the step switches on; any other name the
    step treats alike, -1 or not, except a pseudo-header's -1."""
    return TOKENS.get(bytes(name), -1)


class State:
    def __init__(self, http_flags=0, status_code=-1, content_length=-1):
        self.http_flags, self.status_code, self.content_length = http_flags, status_code, content_length

    def astuple(self):
        return (self.http_flags, self.status_code, self.content_length)


def _pseudo(st, value, flag):
    if (st.http_flags & flag) or not value:
        return False
    st.http_flags |= flag
    return True


def _value_ok(mode, value):
    if mode & MODE_NO_RFC9113_WS:
        return bool(FC.check_header_value(value))
    return bool(FC.check_header_value_rfc9113(value))


def _request(st, mode, name, value):
    if name == b":authority":
        if not check_authority(value) or not _pseudo(st, value, FLAG__AUTHORITY):
            return ERR
    elif name == b":method":
        if not FC.check_method(value) or not _pseudo(st, value, FLAG__METHOD):
            return ERR
        if value == b"HEAD":
            st.http_flags |= FLAG_METH_HEAD
        elif value == b"CONNECT":
            if mode & MODE_PUSH:
                return ERR
            st.http_flags |= FLAG_METH_CONNECT
        elif value == b"OPTIONS":
            st.http_flags |= FLAG_METH_OPTIONS
    elif name == b":path":
        if not FC.check_path(value) or not _pseudo(st, value, FLAG__PATH):
            return ERR
        if value[:1] == b"/":
            st.http_flags |= FLAG_PATH_REGULAR
        elif value == b"*":
            st.http_flags |= FLAG_PATH_ASTERISK
    elif name == b":scheme":
        if not check_scheme(value) or not _pseudo(st, value, FLAG__SCHEME):
            return ERR
        if value.lower() in (b"http", b"https"):
            st.http_flags |= FLAG_SCHEME_HTTP
    elif name == b":protocol":
        if not (mode & MODE_CONNECT_PROTOCOL) or not _pseudo(st, value, FLAG__PROTOCOL):
            return ERR
        if mode & MODE_NO_RFC9113_WS:
            if lws(value) or not FC.check_header_value(value):
                return ERR
        elif not FC.check_header_value_rfc9113(value):
            return ERR
    elif name == b"host":
        if not check_authority(value):
            return IGN
        if not _pseudo(st, value, FLAG_HOST):
            return ERR
    elif name == b"content-length":
        if st.content_length != -1:
            return ERR
        st.content_length = parse_uint(value)
        if st.content_length == -1:
            return ERR
    elif name in DISALLOWED:
        return ERR
    elif name == b"te":
        if value.lower() != b"trailers":
            return ERR
    elif name == b"priority":
        if not _value_ok(mode, value):
            st.http_flags &= ~FLAG_PRIORITY
            st.http_flags |= FLAG_BAD_PRIORITY
            return IGN
    else:
        if name[:1] == b":":
            return ERR
        if not _value_ok(mode, value):
            return IGN
    return 0


def _response(st, mode, name, value):
    if name == b":status":
        if not _pseudo(st, value, FLAG__STATUS):
            return ERR
        st.status_code = parse_status_code(value)
        if st.status_code in (-1, 101):
            return ERR
    elif name == b"content-length":
        if st.status_code == 204:
            if st.content_length != -1 or value != b"0":
                return ERR
            st.content_length = 0
            return REMOVE
        if st.status_code // 100 == 1 and st.status_code >= 0:
            return ERR
        if st.status_code // 100 == 2 and (st.http_flags & FLAG_METH_CONNECT):
            return REMOVE
        if st.content_length != -1:
            return ERR
        st.content_length = parse_uint(value)
        if st.content_length == -1:
            return ERR
    elif name in DISALLOWED:
        return ERR
    elif name == b"te":
        if value.lower() != b"trailers":
            return ERR
    else:
        if name[:1] == b":":
            return ERR
        if not _value_ok(mode, value):
            return IGN
    return 0


def on_header(st, mode, name, value, token=None):
    """nghttp2_http_on_header; token defaults to lookup_token(name)."""
    name, value = bytes(name), bytes(value)
    if token is None:
        token = token_of(name)
    if not name:
        st.http_flags |= FLAG_PSEUDO_HEADER_DISALLOWED
        return IGN
    if name[:1] == b":":
        if token == -1 or (mode & MODE_TRAILER) or (st.http_flags & FLAG_PSEUDO_HEADER_DISALLOWED):
            return ERR
    else:
        st.http_flags |= FLAG_PSEUDO_HEADER_DISALLOWED
        for c in name:  # nghttp2_check_nonempty_header_name: the first refused byte decides
            if c not in FC.NAME:
                return ERR if c in string.ascii_uppercase.encode() else IGN
    if mode & MODE_REQUEST:
        return _request(st, mode, name, value)
    return _response(st, mode, name, value)


def _check_path(st):
    f = st.http_flags
    return not (f & FLAG_SCHEME_HTTP) or bool(f & FLAG_PATH_REGULAR) or \
        bool((f & FLAG_METH_OPTIONS) and (f & FLAG_PATH_ASTERISK))


def on_request_headers(st, mode):
    f = st.http_flags
    if not (f & FLAG__PROTOCOL) and (f & FLAG_METH_CONNECT):
        if (f & (FLAG__SCHEME | FLAG__PATH)) or not (f & FLAG__AUTHORITY):
            return -1
        st.content_length = -1
    else:
        if (f & FLAG_REQ_HEADERS) != FLAG_REQ_HEADERS or not (f & (FLAG__AUTHORITY | FLAG_HOST)):
            return -1
        if (f & FLAG__PROTOCOL) and (not (f & FLAG_METH_CONNECT) or not (f & FLAG__AUTHORITY)):
            return -1
        if not _check_path(st):
            return -1
    if mode & MODE_PUSH:
        st.http_flags &= FLAG_METH_ALL
        st.content_length = -1
    return 0


def on_response_headers(st):
    if not (st.http_flags & FLAG__STATUS):
        return -1
    if st.status_code // 100 == 1 and st.status_code >= 0:
        st.http_flags = (st.http_flags & FLAG_METH_ALL) | FLAG_EXPECT_FINAL_RESPONSE
        st.content_length = -1
        st.status_code = -1
        return 0
    st.http_flags &= ~FLAG_EXPECT_FINAL_RESPONSE
    if (st.http_flags & FLAG_METH_HEAD) or st.status_code in (304, 204):
        st.content_length = 0
    elif st.http_flags & (FLAG_METH_CONNECT | FLAG_METH_UPGRADE_WORKAROUND):
        st.content_length = -1
    return 0


def run_block(fields, mode, state):
    """One block as the _http inflate treats it: (verdicts, state after the
    block as a tuple, block result).  state: (http_flags, status_code,
    content_length) before the block."""
    st = State(*state)
    verdicts, result, stopped = [], 0, False
    for name, value in fields:
        if stopped:
            verdicts.append(NOT_EXAMINED)
            continue
        rv = on_header(st, mode, name, value)
        verdicts.append(rv)
        if rv == ERR:
            stopped, result = True, ERR
    if not stopped and not (mode & MODE_TRAILER):
        rv = on_request_headers(st, mode) if mode & MODE_REQUEST else on_response_headers(st)
        if rv:
            result = MESSAGING
    return verdicts, st.astuple(), result
