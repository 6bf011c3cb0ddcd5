// hd_static.h -- the HPACK static table (RFC 7541 Appendix A), stated once for
// the host layers (hd_inflate.cpp, hd_deflate.cpp: static_entry) and for the
// device replay (hd_replay.hip: kStaticPool, copied into constant memory).
// Plain C++17, no HIP.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "hd_tokens.h"

namespace hdhost {

constexpr uint32_t kEntryOverhead = 32;  // NGHTTP2_HD_ENTRY_OVERHEAD
constexpr uint32_t kStaticLen = 61;
// RFC 7541 Appendix A
constexpr const char *kStatic[kStaticLen][2] = {
    {":authority", ""}, {":method", "GET"}, {":method", "POST"}, {":path", "/"},
    {":path", "/index.html"}, {":scheme", "http"}, {":scheme", "https"}, {":status", "200"},
    {":status", "204"}, {":status", "206"}, {":status", "304"}, {":status", "400"},
    {":status", "404"}, {":status", "500"}, {"accept-charset", ""},
    {"accept-encoding", "gzip, deflate"}, {"accept-language", ""}, {"accept-ranges", ""},
    {"accept", ""}, {"access-control-allow-origin", ""}, {"age", ""}, {"allow", ""},
    {"authorization", ""}, {"cache-control", ""}, {"content-disposition", ""},
    {"content-encoding", ""}, {"content-language", ""}, {"content-length", ""},
    {"content-location", ""}, {"content-range", ""}, {"content-type", ""}, {"cookie", ""},
    {"date", ""}, {"etag", ""}, {"expect", ""}, {"expires", ""}, {"from", ""}, {"host", ""},
    {"if-match", ""}, {"if-modified-since", ""}, {"if-none-match", ""}, {"if-range", ""},
    {"if-unmodified-since", ""}, {"last-modified", ""}, {"link", ""}, {"location", ""},
    {"max-forwards", ""}, {"proxy-authenticate", ""}, {"proxy-authorization", ""},
    {"range", ""}, {"referer", ""}, {"refresh", ""}, {"retry-after", ""}, {"server", ""},
    {"set-cookie", ""}, {"strict-transport-security", ""}, {"transfer-encoding", ""},
    {"user-agent", ""}, {"vary", ""}, {"via", ""}, {"www-authenticate", ""}};

// The entries' lengths ([i][0] name, [i][1] value), and the longest of each.
struct StaticLens {
  uint32_t len[kStaticLen][2];
  uint32_t max[2];
};
constexpr StaticLens make_static_lens() {
  StaticLens t{};
  for (uint32_t i = 0; i < kStaticLen; ++i)
    for (int w = 0; w < 2; ++w) {
      t.len[i][w] = hdtok::cstr_len(kStatic[i][w]);
      if (t.len[i][w] > t.max[w]) t.max[w] = t.len[i][w];
    }
  return t;
}
constexpr StaticLens kStaticLens = make_static_lens();
static_assert(kStaticLens.max[0] == 27 && kStaticLens.max[1] == 13, "access-control-allow-origin, gzip, deflate");
// static entry idx (0-based, < kStaticLen)
inline void static_entry(uint32_t idx, const char **name, size_t *nl, const char **value, size_t *vl) {
  *name = kStatic[idx][0];
  *nl = kStaticLens.len[idx][0];
  *value = kStatic[idx][1];
  *vl = kStaticLens.len[idx][1];
}

// The same table as one byte pool, for code that addresses strings by offset
// and length (the replay's references): entry i's name is
// bytes[off[i][0], +len[i][0]), its value bytes[off[i][1], +len[i][1]).
constexpr uint32_t static_pool_bytes() {
  uint32_t n = 0;
  for (uint32_t i = 0; i < kStaticLen; ++i) n += kStaticLens.len[i][0] + kStaticLens.len[i][1];
  return n;
}
constexpr uint32_t kStaticPoolBytes = static_pool_bytes();
struct StaticPool {
  uint16_t off[kStaticLen][2];
  uint16_t len[kStaticLen][2];
  uint8_t bytes[(kStaticPoolBytes + 15u) & ~15u];
};
constexpr StaticPool make_static_pool() {
  StaticPool p{};
  uint32_t at = 0;
  for (uint32_t i = 0; i < kStaticLen; ++i)
    for (int w = 0; w < 2; ++w) {
      p.off[i][w] = (uint16_t)at;
      p.len[i][w] = (uint16_t)kStaticLens.len[i][w];
      for (uint32_t k = 0; k < kStaticLens.len[i][w]; ++k) p.bytes[at++] = (uint8_t)kStatic[i][w][k];
    }
  return p;
}
constexpr StaticPool kStaticPool = make_static_pool();

}  // namespace hdhost
