"""The reference's header-field checks (nghttp2_check_*, lib/nghttp2_helper.c:
346-558) restated from the RFC character classes they implement: the checker
of nghttp2_amd_hd_check_field, nghttp2_amd_hd_check_fields_batch and the
checked inflate.  tests/golden/field_checks.json (results recorded from the
reference's own tables, tests/golden/make_field_checks.py) pins it."""
import hashlib
import string

CHECK_NAME, CHECK_VALUE, CHECK_VALUE_RFC9113, CHECK_METHOD = 0x01, 0x02, 0x04, 0x08
CHECK_PATH, CHECK_AUTHORITY, CHECK_NAME_LOWER, CHECK_INVALID = 0x10, 0x20, 0x40, 0x80
# the golden's order of results -> bit
ORDER_BITS = [CHECK_NAME, CHECK_VALUE, CHECK_VALUE_RFC9113, CHECK_METHOD, CHECK_PATH,
              CHECK_AUTHORITY, CHECK_NAME_LOWER]

_ALPHA = string.ascii_letters.encode()
_DIGIT = string.digits.encode()
# RFC 9110 5.6.2 tchar
TCHAR = frozenset(b"!#$%&'*+-.^_`|~" + _DIGIT + _ALPHA)
# a field name as HTTP/2 carries it (RFC 9113 8.2.1): tchar, no upper case
NAME = TCHAR - frozenset(string.ascii_uppercase.encode())
VCHAR = frozenset(range(0x21, 0x7F))
OBS_TEXT = frozenset(range(0x80, 0x100))
# RFC 9110 5.5 field-content bytes
VALUE = VCHAR | OBS_TEXT | frozenset(b" \t")
PATH = VCHAR | OBS_TEXT
# RFC 3986 3.2: unreserved / sub-delims / "%" of pct-encoded / ":" / "@" / "[" "]"
AUTHORITY = frozenset(_ALPHA + _DIGIT + b"-._~" + b"!$&'()*+,;=" + b"%:@[]")


def check_header_name(s):
    if not s:
        return 0
    if s[:1] == b":":
        s = s[1:]
        if not s:
            return 0
    return int(all(c in NAME for c in s))


def check_nonempty_header_name_is_1(s):
    return int(all(c in NAME for c in s))


def check_header_value(s):
    return int(all(c in VALUE for c in s))


def check_header_value_rfc9113(s):
    if not s:
        return 1
    if s[0] in b" \t" or s[-1] in b" \t":
        return 0
    return check_header_value(s)


def check_method(s):
    return int(len(s) > 0 and all(c in TCHAR for c in s))


def check_path(s):
    return int(all(c in PATH for c in s))


def check_authority(s):
    return int(all(c in AUTHORITY for c in s))


FUNCS = [check_header_name, check_header_value, check_header_value_rfc9113, check_method,
         check_path, check_authority, check_nonempty_header_name_is_1]


def results(s):
    """The seven results in the golden's order."""
    s = bytes(s)
    return [f(s) for f in FUNCS]


def mask(s):
    """The NGHTTP2_AMD_CHECK_* mask of one string."""
    m = 0
    for bit, r in zip(ORDER_BITS, results(s)):
        if r:
            m |= bit
    return m


def table_sha256():
    """sha256 of each reference table as the classes above give it (the name
    table's classes: 1 lower-case name byte, 2 upper-case letter, 0 else)."""
    def tbl(f):
        return hashlib.sha256(bytes(f(c) for c in range(256))).hexdigest()
    upper = frozenset(string.ascii_uppercase.encode())
    return {"VALID_HD_NAME_CHARS": tbl(lambda c: 1 if c in NAME else 2 if c in upper else 0),
            "VALID_HD_VALUE_CHARS": tbl(lambda c: int(c in VALUE)),
            "VALID_METHOD_CHARS": tbl(lambda c: int(c in TCHAR)),
            "VALID_PATH_CHARS": tbl(lambda c: int(c in PATH)),
            "VALID_AUTHORITY_CHARS": tbl(lambda c: int(c in AUTHORITY))}
