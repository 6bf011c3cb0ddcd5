// hd_http.h -- nghttp2_http_on_header split into value facts and a byte-free step.
//
// The reference validates every field an inflater hands over with
// nghttp2_http_on_header (lib/nghttp2_http.c:405-447): a switch on nv.token
// that scans the value's bytes (check_authority without '@', check_scheme,
// lws, parse_uint, parse_status_code, comparisons against "HEAD", "http",
// "trailers", ...) and keeps the stream's http_flags, content_length and
// status_code.  Here the byte work that the NGHTTP2_AMD_CHECK_* masks
// (hd_field_classes.h) do not cover is one more per-string result, the value
// facts: NGHTTP2_AMD_HTTP_FACT_* and parse_uint's number.  The whole-string
// ones are ORs of four per-byte classes, as the masks are; the comparisons
// against short literals use the string's first 8 bytes and its length.  The
// step itself (on_header below) is then a pure function of token, masks,
// facts and number, and BlockRun at the end is the one driver of it: a
// block's fields in order, the stop at the first stream error, the block end.
//
// Shared by the host function (nghttp2_amd_hd_http_facts) and the GPU kernel
// (k_http_facts, the class table staged in LDS) for the facts, and by the
// inflater's replay (hd_inflate.cpp) and k_http_blocks of hd_fields.hip, which
// both run a block through BlockRun.
// Plain C++17, no HIP: included by .cpp and .hip sources alike.
#ifndef NGHTTP2_AMD_HD_HTTP_H
#define NGHTTP2_AMD_HD_HTTP_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_field_classes.h"

#if defined(__HIPCC__)
#define HDHTTP_FN __host__ __device__ inline
#else
#define HDHTTP_FN inline
#endif

namespace hdhttp {

// violation bits of a byte's class
constexpr uint8_t kNotAuthority = 0x01;   // not a byte of lib/nghttp2_http.c's authority table (no '@')
constexpr uint8_t kNotSchemeTail = 0x02;  // not ALPHA / DIGIT / "+" / "-" / "." (RFC 3986 3.1)
constexpr uint8_t kNotDigit = 0x04;
constexpr uint8_t kNotBlank = 0x08;  // not SP / HT
// not '0': no fact is an OR of it; the kernel finds a number's first
// significant digit with it, as the first chunk of the string that holds one
constexpr uint8_t kNotZero = 0x10;
constexpr uint8_t kBallots = 5;  // the five above are taken as wave ballots
// position class: the first byte of a scheme
constexpr uint8_t kNotAlpha = 0x20;

constexpr uint8_t byte_class(uint32_t c) {
  using namespace hdcls;
  uint8_t k = 0;
  if (!is_authority(c) || c == '@') k |= kNotAuthority;
  const bool alpha = is_lower(c) || is_upper(c);
  if (!(alpha || is_digit(c) || c == '+' || c == '-' || c == '.')) k |= kNotSchemeTail;
  if (!is_digit(c)) k |= kNotDigit;
  if (!(c == ' ' || c == '\t')) k |= kNotBlank;
  if (c != '0') k |= kNotZero;
  if (!alpha) k |= kNotAlpha;
  return k;
}
struct Table {
  uint8_t cls[256];
};
constexpr Table make_table() {
  Table t{};
  for (uint32_t c = 0; c < 256; ++c) t.cls[c] = byte_class(c);
  return t;
}
constexpr Table kTable = make_table();

// a literal of at most 8 bytes as the little-endian word of its bytes
constexpr uint64_t lit8(const char *s) {
  uint64_t w = 0;
  for (uint32_t i = 0; s[i]; ++i) w |= (uint64_t)(uint8_t)s[i] << (8 * i);
  return w;
}
// 0x20 in each of the low n bytes: ORed into a word it maps 'A'..'Z' onto
// 'a'..'z', and no other byte onto a lower-case letter (x | 0x20 == t for a
// lower-case t exactly when x is t or its upper-case form), so an equality
// with a lower-case literal afterwards is the reference's memieq
constexpr uint64_t fold(uint32_t n) { return 0x2020202020202020ull >> (8 * (8 - n)); }

// The facts of an examined string from its length, the OR of its bytes'
// classes (`all`), the OR of every byte but the first (`rest`), the first
// byte's class, `head` = its first min(len, 8) bytes as a little-endian word
// (zero above them), and whether its digits overflow parse_uint (asked for
// only when all is free of kNotDigit and len > 0).
HDHTTP_FN uint32_t facts_of(size_t len, uint32_t all, uint32_t rest, uint32_t first, uint64_t head,
                            bool overflow) {
  uint32_t f = 0;
  if (!(all & kNotAuthority)) f |= NGHTTP2_AMD_HTTP_FACT_AUTHORITY;
  if (!(all & kNotBlank)) f |= NGHTTP2_AMD_HTTP_FACT_LWS;
  if (len == 0) return f;
  if (!(first & kNotAlpha) && !(rest & kNotSchemeTail)) f |= NGHTTP2_AMD_HTTP_FACT_SCHEME;
  if (!(all & kNotDigit) && !overflow) f |= NGHTTP2_AMD_HTTP_FACT_UINT;
  if ((head & 0xFFu) == '/') f |= NGHTTP2_AMD_HTTP_FACT_PATH_SLASH;
  if (len == 1 && head == lit8("*")) f |= NGHTTP2_AMD_HTTP_FACT_PATH_ASTERISK;
  if (len == 4 && head == lit8("HEAD")) f |= NGHTTP2_AMD_HTTP_FACT_METH_HEAD;
  if (len == 7 && head == lit8("CONNECT")) f |= NGHTTP2_AMD_HTTP_FACT_METH_CONNECT;
  if (len == 7 && head == lit8("OPTIONS")) f |= NGHTTP2_AMD_HTTP_FACT_METH_OPTIONS;
  if ((len == 4 && (head | fold(4)) == lit8("http")) || (len == 5 && (head | fold(5)) == lit8("https")))
    f |= NGHTTP2_AMD_HTTP_FACT_SCHEME_HTTP;
  if (len == 8 && (head | fold(8)) == lit8("trailers")) f |= NGHTTP2_AMD_HTTP_FACT_TE_TRAILERS;
  return f;
}

// parse_uint (lib/nghttp2_http.c:65-89) of a string known to be all digits
// and not empty: -1 at the first overflow past INT64_MAX.  Leading zeros are
// skipped; what is left overflows for certain past 19 digits (the smallest
// 20-digit number is above INT64_MAX), so the exact loop runs 19 times at most.
template <class Bytes>
HDHTTP_FN int64_t digits_value(const Bytes &s, size_t len) {
  size_t i = 0;
  while (i < len && s[i] == '0') ++i;
  if (len - i > 19) return -1;
  uint64_t n = 0;
  for (; i < len; ++i) {
    const uint32_t c = (uint32_t)s[i] - '0';
    if (n > ((uint64_t)INT64_MAX - c) / 10) return -1;
    n = n * 10 + c;
  }
  return (int64_t)n;
}

// One host string (nghttp2_amd_hd_http_facts).
inline uint32_t http_facts(const uint8_t *s, size_t len, int64_t *number) {
  int64_t num = -1;
  uint32_t f;
  if (len == 0) {
    f = facts_of(0, 0, 0, 0, 0, false);
  } else {
    uint32_t rest = 0;
    for (size_t i = 1; i < len; ++i) rest |= kTable.cls[s[i]];
    const uint32_t first = kTable.cls[s[0]], all = first | rest;
    uint64_t head = 0;
    for (size_t i = 0; i < len && i < 8; ++i) head |= (uint64_t)s[i] << (8 * i);
    if (!(all & kNotDigit)) num = digits_value(s, len);
    f = facts_of(len, all, rest, first, head, num < 0);
  }
  if (number) *number = num;
  return f;
}

// ---- the per-field step and the block ends (lib/nghttp2_http.c:91-511) ----

// NGHTTP2_TOKEN_* (lib/nghttp2_hd.h:56-116) the step switches on
enum : int32_t {
  kTok_Authority = 0, kTok_Method = 1, kTok_Path = 3, kTok_Scheme = 5, kTok_Status = 7,
  kTokContentLength = 27, kTokHost = 37, kTokTransferEncoding = 56, kTokTe = 61, kTokConnection = 62,
  kTokKeepAlive = 63, kTokProxyConnection = 64, kTokUpgrade = 65, kTok_Protocol = 66, kTokPriority = 67
};

typedef nghttp2_amd_hd_http_state State;

// one field as the step sees it
struct Field {
  const uint8_t *name;
  size_t name_len, value_len;
  int32_t token;
  uint32_t name_mask, value_mask, facts;
  int64_t number;
  // the name's first byte where the caller holds it already (k_http_blocks
  // loads it ahead of the step), else -1: it is read from `name`
  int32_t name0 = -1;
};
HDHTTP_FN uint32_t first_byte(const Field &f) { return f.name0 >= 0 ? (uint32_t)f.name0 : f.name[0]; }

HDHTTP_FN bool check_pseudo_header(State *st, const Field &f, uint32_t flag) {  // :91-98
  if ((st->http_flags & flag) || f.value_len == 0) return false;
  st->http_flags |= flag;
  return true;
}
HDHTTP_FN bool check_header_value(uint32_t mode, const Field &f) {  // :178-186
  return (f.value_mask &
          ((mode & NGHTTP2_AMD_HTTP_MODE_NO_RFC9113_WS) ? NGHTTP2_AMD_CHECK_VALUE : NGHTTP2_AMD_CHECK_VALUE_RFC9113)) != 0;
}
HDHTTP_FN bool disallowed(int32_t token) {
  return token == kTokConnection || token == kTokKeepAlive || token == kTokProxyConnection ||
         token == kTokTransferEncoding || token == kTokUpgrade;
}

HDHTTP_FN int request_on_header(State *st, uint32_t mode, const Field &f) {  // :188-334
  const int kErr = NGHTTP2_AMD_ERR_HTTP_HEADER, kIgn = NGHTTP2_AMD_ERR_IGN_HTTP_HEADER;
  switch (f.token) {
  case kTok_Authority:
    if (!(f.facts & NGHTTP2_AMD_HTTP_FACT_AUTHORITY) || !check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG__AUTHORITY))
      return kErr;
    break;
  case kTok_Method:
    if (!(f.value_mask & NGHTTP2_AMD_CHECK_METHOD) || !check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG__METHOD))
      return kErr;
    if (f.facts & NGHTTP2_AMD_HTTP_FACT_METH_HEAD) {
      st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_METH_HEAD;
    } else if (f.facts & NGHTTP2_AMD_HTTP_FACT_METH_CONNECT) {
      if (mode & NGHTTP2_AMD_HTTP_MODE_PUSH) return kErr;  // no CONNECT for push
      st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT;
    } else if (f.facts & NGHTTP2_AMD_HTTP_FACT_METH_OPTIONS) {
      st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_METH_OPTIONS;
    }
    break;
  case kTok_Path:
    if (!(f.value_mask & NGHTTP2_AMD_CHECK_PATH) || !check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG__PATH))
      return kErr;
    if (f.facts & NGHTTP2_AMD_HTTP_FACT_PATH_SLASH)
      st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_PATH_REGULAR;
    else if (f.facts & NGHTTP2_AMD_HTTP_FACT_PATH_ASTERISK)
      st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_PATH_ASTERISK;
    break;
  case kTok_Scheme:
    if (!(f.facts & NGHTTP2_AMD_HTTP_FACT_SCHEME) || !check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG__SCHEME))
      return kErr;
    if (f.facts & NGHTTP2_AMD_HTTP_FACT_SCHEME_HTTP) st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_SCHEME_HTTP;
    break;
  case kTok_Protocol:
    if (!(mode & NGHTTP2_AMD_HTTP_MODE_CONNECT_PROTOCOL) ||
        !check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG__PROTOCOL))
      return kErr;
    if (mode & NGHTTP2_AMD_HTTP_MODE_NO_RFC9113_WS) {
      if ((f.facts & NGHTTP2_AMD_HTTP_FACT_LWS) || !(f.value_mask & NGHTTP2_AMD_CHECK_VALUE)) return kErr;
    } else if (!(f.value_mask & NGHTTP2_AMD_CHECK_VALUE_RFC9113)) {
      return kErr;
    }
    break;
  case kTokHost:
    if (!(f.facts & NGHTTP2_AMD_HTTP_FACT_AUTHORITY)) return kIgn;
    if (!check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG_HOST)) return kErr;
    break;
  case kTokContentLength:
    if (st->content_length != -1) return kErr;
    st->content_length = (f.facts & NGHTTP2_AMD_HTTP_FACT_UINT) ? f.number : -1;
    if (st->content_length == -1) return kErr;
    break;
  case kTokConnection:
  case kTokKeepAlive:
  case kTokProxyConnection:
  case kTokTransferEncoding:
  case kTokUpgrade:
    return kErr;
  case kTokTe:
    if (!(f.facts & NGHTTP2_AMD_HTTP_FACT_TE_TRAILERS)) return kErr;
    break;
  case kTokPriority:
    if (!check_header_value(mode, f)) {
      st->http_flags &= ~NGHTTP2_AMD_HTTP_FLAG_PRIORITY;
      st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_BAD_PRIORITY;
      return kIgn;
    }
    // (the structured value's parse, :308-321, is the caller's)
    break;
  default:
    if (first_byte(f) == ':') return kErr;
    if (!check_header_value(mode, f)) return kIgn;
  }
  return 0;
}

HDHTTP_FN int response_on_header(State *st, uint32_t mode, const Field &f) {  // :336-403
  const int kErr = NGHTTP2_AMD_ERR_HTTP_HEADER;
  const bool uint_ok = (f.facts & NGHTTP2_AMD_HTTP_FACT_UINT) != 0;
  switch (f.token) {
  case kTok_Status:
    if (!check_pseudo_header(st, f, NGHTTP2_AMD_HTTP_FLAG__STATUS)) return kErr;
    // parse_status_code: three digits, the first not '0'
    st->status_code = uint_ok && f.value_len == 3 && f.number >= 100 ? (int32_t)f.number : -1;
    if (st->status_code == -1 || st->status_code == 101) return kErr;
    break;
  case kTokContentLength:
    if (st->status_code == 204) {
      if (st->content_length != -1) return kErr;
      if (!(uint_ok && f.value_len == 1 && f.number == 0)) return kErr;  // lstrieq("0", ...)
      st->content_length = 0;
      return NGHTTP2_AMD_ERR_REMOVE_HTTP_HEADER;
    }
    if (st->status_code / 100 == 1) return kErr;
    if (st->status_code / 100 == 2 && (st->http_flags & NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT))
      return NGHTTP2_AMD_ERR_REMOVE_HTTP_HEADER;
    if (st->content_length != -1) return kErr;
    st->content_length = uint_ok ? f.number : -1;
    if (st->content_length == -1) return kErr;
    break;
  case kTokConnection:
  case kTokKeepAlive:
  case kTokProxyConnection:
  case kTokTransferEncoding:
  case kTokUpgrade:
    return kErr;
  case kTokTe:
    if (!(f.facts & NGHTTP2_AMD_HTTP_FACT_TE_TRAILERS)) return kErr;
    break;
  default:
    if (first_byte(f) == ':') return kErr;
    if (!check_header_value(mode, f)) return NGHTTP2_AMD_ERR_IGN_HTTP_HEADER;
  }
  return 0;
}

// `cls` is hdcls::kTable's bytes where the caller runs: a kernel passes its
// device copy (the name loop below indexes it)
HDHTTP_FN int on_header(State *st, uint32_t mode, const Field &f,
                        const uint8_t *cls = hdcls::kTable.cls) {  // :405-447
  if (f.name_len == 0) {
    st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED;
    return NGHTTP2_AMD_ERR_IGN_HTTP_HEADER;
  }
  if (first_byte(f) == ':') {
    if (f.token == -1 || (mode & NGHTTP2_AMD_HTTP_MODE_TRAILER) ||
        (st->http_flags & NGHTTP2_AMD_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED))
      return NGHTTP2_AMD_ERR_HTTP_HEADER;
  } else {
    st->http_flags |= NGHTTP2_AMD_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED;
    if (!(f.name_mask & NGHTTP2_AMD_CHECK_NAME_LOWER)) {
      // nghttp2_check_nonempty_header_name's first refused byte: an
      // upper-case letter is 2 (a stream error), any other 0 (ignored)
      for (size_t i = 0; i < f.name_len; ++i)
        if (cls[f.name[i]] & hdcls::kBadName)
          return hdcls::is_upper(f.name[i]) ? NGHTTP2_AMD_ERR_HTTP_HEADER : NGHTTP2_AMD_ERR_IGN_HTTP_HEADER;
    }
  }
  if (mode & NGHTTP2_AMD_HTTP_MODE_REQUEST) return request_on_header(st, mode, f);
  return response_on_header(st, mode, f);
}

HDHTTP_FN bool check_path(const State *st) {  // :111-116
  return (st->http_flags & NGHTTP2_AMD_HTTP_FLAG_SCHEME_HTTP) == 0 ||
         ((st->http_flags & NGHTTP2_AMD_HTTP_FLAG_PATH_REGULAR) ||
          ((st->http_flags & NGHTTP2_AMD_HTTP_FLAG_METH_OPTIONS) &&
           (st->http_flags & NGHTTP2_AMD_HTTP_FLAG_PATH_ASTERISK)));
}

HDHTTP_FN int on_request_headers(State *st, uint32_t mode) {  // :449-484
  const uint32_t fl = st->http_flags;
  if (!(fl & NGHTTP2_AMD_HTTP_FLAG__PROTOCOL) && (fl & NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT)) {
    if ((fl & (NGHTTP2_AMD_HTTP_FLAG__SCHEME | NGHTTP2_AMD_HTTP_FLAG__PATH)) ||
        (fl & NGHTTP2_AMD_HTTP_FLAG__AUTHORITY) == 0)
      return -1;
    st->content_length = -1;
  } else {
    if ((fl & NGHTTP2_AMD_HTTP_FLAG_REQ_HEADERS) != NGHTTP2_AMD_HTTP_FLAG_REQ_HEADERS ||
        (fl & (NGHTTP2_AMD_HTTP_FLAG__AUTHORITY | NGHTTP2_AMD_HTTP_FLAG_HOST)) == 0)
      return -1;
    if ((fl & NGHTTP2_AMD_HTTP_FLAG__PROTOCOL) &&
        ((fl & NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT) == 0 || (fl & NGHTTP2_AMD_HTTP_FLAG__AUTHORITY) == 0))
      return -1;
    if (!check_path(st)) return -1;
  }
  if (mode & NGHTTP2_AMD_HTTP_MODE_PUSH) {  // a PUSH_PROMISE: the fields are reused for the response
    st->http_flags &= NGHTTP2_AMD_HTTP_FLAG_METH_ALL;
    st->content_length = -1;
  }
  return 0;
}

HDHTTP_FN int on_response_headers(State *st) {  // :486-511
  if ((st->http_flags & NGHTTP2_AMD_HTTP_FLAG__STATUS) == 0) return -1;
  if (st->status_code / 100 == 1) {  // non-final response
    st->http_flags = (st->http_flags & NGHTTP2_AMD_HTTP_FLAG_METH_ALL) | NGHTTP2_AMD_HTTP_FLAG_EXPECT_FINAL_RESPONSE;
    st->content_length = -1;
    st->status_code = -1;
    return 0;
  }
  st->http_flags &= ~NGHTTP2_AMD_HTTP_FLAG_EXPECT_FINAL_RESPONSE;
  const bool expect_body = (st->http_flags & NGHTTP2_AMD_HTTP_FLAG_METH_HEAD) == 0 && st->status_code / 100 != 1 &&
                           st->status_code != 304 && st->status_code != 204;
  if (!expect_body)
    st->content_length = 0;
  else if (st->http_flags & (NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT | NGHTTP2_AMD_HTTP_FLAG_METH_UPGRADE_WORKAROUND))
    st->content_length = -1;
  return 0;
}

// One block's fields in order on its stream's state, and the block's end.
// After the first stream error the reference stops calling
// nghttp2_http_on_header for the stream (lib/nghttp2_session.c:3643-3664): the
// later fields are not examined and the state stays.
struct BlockRun {
  State st;       // in: before the block; out: after it
  uint32_t mode;  // NGHTTP2_AMD_HTTP_MODE_*
  bool stopped = false;
  int32_t result = 0;  // 0, ERR_HTTP_HEADER, ERR_HTTP_MESSAGING or the wire's failure
  HDHTTP_FN int step(const Field &f, const uint8_t *cls = hdcls::kTable.cls) {
    if (stopped) return NGHTTP2_AMD_HTTP_NOT_EXAMINED;
    const int rv = on_header(&st, mode, f, cls);
    if (rv == NGHTTP2_AMD_ERR_HTTP_HEADER) {
      stopped = true;
      result = rv;
    }
    return rv;
  }
  // wire_status: the inflater's status of the block.  A failed wire (or the
  // store's capacity) is the result and there is no block end; a sound one
  // ends with the block-end function of the mode, but for trailers.
  HDHTTP_FN void finish(int32_t wire_status) {
    if (wire_status < 0) {
      result = wire_status;
    } else if (!stopped && !(mode & NGHTTP2_AMD_HTTP_MODE_TRAILER)) {
      const int rv = (mode & NGHTTP2_AMD_HTTP_MODE_REQUEST) ? on_request_headers(&st, mode) : on_response_headers(&st);
      if (rv) result = NGHTTP2_AMD_ERR_HTTP_MESSAGING;
    }
  }
};

}  // namespace hdhttp

#endif  // NGHTTP2_AMD_HD_HTTP_H
