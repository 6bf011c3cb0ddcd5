// hd_field_classes.h -- byte classes of nghttp2's header-field checks.
//
// The reference validates a decoded field with table-driven byte scans
// (nghttp2_check_header_name / _header_value / _header_value_rfc9113 /
// _method / _path / _authority, lib/nghttp2_helper.c:346-558, called from
// nghttp2_http_on_header, lib/nghttp2_http.c:405-447): one 256-entry table
// per check and an AND over the string.  Here the five tables are one: a
// byte per input byte holding five "this byte violates table k" bits, written
// from the grammars the tables restate (RFC 9110 5.1 / 5.5 / 5.6.2, RFC 3986
// 3.2 / 2.2 / 2.3), plus two marker bits for the bytes the checks treat by
// position (':' leading a name, SP / HT at the ends of a value).  A string
// passes check k exactly when the OR of its bytes' classes has bit k clear.
//
// The table is built at compile time and shared by the host function
// (nghttp2_amd_hd_check_field), the inflater's replay and the GPU kernel
// (k_check_fields, staged in LDS).  Plain C++17, no HIP: included by .cpp and
// .hip sources alike.
#ifndef NGHTTP2_AMD_HD_FIELD_CLASSES_H
#define NGHTTP2_AMD_HD_FIELD_CLASSES_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"

namespace hdcls {

// violation bits of a byte's class
constexpr uint8_t kBadName = 0x01;       // not a lower-case field-name byte
constexpr uint8_t kBadValue = 0x02;      // not a field-value byte
constexpr uint8_t kBadMethod = 0x04;     // not a token byte
constexpr uint8_t kBadPath = 0x08;       // not a :path byte
constexpr uint8_t kBadAuthority = 0x10;  // not an authority byte
constexpr uint8_t kBadAll = 0x1F;
// position markers
constexpr uint8_t kColon = 0x20;  // ':'
constexpr uint8_t kBlank = 0x40;  // SP or HT

constexpr bool in_set(uint32_t c, const char *set) {
  for (; *set; ++set)
    if ((uint8_t)*set == c) return true;
  return false;
}
constexpr bool is_digit(uint32_t c) { return c >= '0' && c <= '9'; }
constexpr bool is_lower(uint32_t c) { return c >= 'a' && c <= 'z'; }
constexpr bool is_upper(uint32_t c) { return c >= 'A' && c <= 'Z'; }
// tchar (RFC 9110 5.6.2): "!" / "#" / "$" / "%" / "&" / "'" / "*" / "+" / "-"
// / "." / "^" / "_" / "`" / "|" / "~" / DIGIT / ALPHA
constexpr bool is_tchar(uint32_t c) {
  return is_digit(c) || is_lower(c) || is_upper(c) || in_set(c, "!#$%&'*+-.^_`|~");
}
constexpr bool is_vchar(uint32_t c) { return c >= 0x21 && c <= 0x7E; }
constexpr bool is_obs_text(uint32_t c) { return c >= 0x80 && c <= 0xFF; }
// authority = [ userinfo "@" ] host [ ":" port ] (RFC 3986 3.2): unreserved,
// sub-delims, the "%" of pct-encoded, ":" and "@", and the brackets of an
// IP-literal
constexpr bool is_authority(uint32_t c) {
  return is_digit(c) || is_lower(c) || is_upper(c) || in_set(c, "-._~") || in_set(c, "!$&'()*+,;=") ||
         in_set(c, "%:@[]");
}

constexpr uint8_t byte_class(uint32_t c) {
  uint8_t k = 0;
  // a field name as HTTP/2 carries it: token bytes, none of them upper case
  // (RFC 9113 8.2.1)
  if (!is_tchar(c) || is_upper(c)) k |= kBadName;
  // field-content: HT, SP, VCHAR, obs-text (RFC 9110 5.5)
  if (!(c == '\t' || c == ' ' || is_vchar(c) || is_obs_text(c))) k |= kBadValue;
  if (!is_tchar(c)) k |= kBadMethod;
  // :path as nghttp2 accepts it: any visible byte or obs-text, no blanks
  if (!(is_vchar(c) || is_obs_text(c))) k |= kBadPath;
  if (!is_authority(c)) k |= kBadAuthority;
  if (c == ':') k |= kColon;
  if (c == ' ' || c == '\t') k |= kBlank;
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

// The result mask of a string from its length, the OR of its bytes' classes
// (`all`), the OR of the classes of every byte but the first (`rest`), and the
// classes of its first and last byte.  len == 0: all four are 0.
constexpr uint8_t mask_of(size_t len, uint32_t all, uint32_t rest, uint32_t first, uint32_t last) {
  uint32_t m = 0;
  // nghttp2_check_header_name: not empty, a leading ':' skipped, ":" alone refused
  const uint32_t nm = (first & kColon) ? rest : all;
  if (len != 0 && !((first & kColon) && len == 1) && !(nm & kBadName)) m |= NGHTTP2_AMD_CHECK_NAME;
  if (!(all & kBadValue)) {
    m |= NGHTTP2_AMD_CHECK_VALUE;
    if (!((first | last) & kBlank)) m |= NGHTTP2_AMD_CHECK_VALUE_RFC9113;
  }
  if (len != 0 && !(all & kBadMethod)) m |= NGHTTP2_AMD_CHECK_METHOD;
  if (!(all & kBadPath)) m |= NGHTTP2_AMD_CHECK_PATH;
  if (!(all & kBadAuthority)) m |= NGHTTP2_AMD_CHECK_AUTHORITY;
  if (!(all & kBadName)) m |= NGHTTP2_AMD_CHECK_NAME_LOWER;
  return (uint8_t)m;
}

// One host string (nghttp2_amd_hd_check_field).
inline uint8_t check_field(const uint8_t *s, size_t len) {
  if (len == 0) return mask_of(0, 0, 0, 0, 0);
  uint32_t rest = 0;
  for (size_t i = 1; i < len; ++i) rest |= kTable.cls[s[i]];
  const uint32_t first = kTable.cls[s[0]];
  return mask_of(len, first | rest, rest, first, kTable.cls[s[len - 1]]);
}

}  // namespace hdcls

#endif  // NGHTTP2_AMD_HD_FIELD_CLASSES_H
