// hd_host.h -- what the host layers above the C ABI share (hd_inflate.cpp,
// hd_deflate.cpp, hd_sharded.cpp): the HPACK static table with its lengths
// computed at compile time, the HIP error reports (hip_rv is the kernel
// layers' own, the .hip files'), and the growable device and pinned host
// buffers the layers stage their batches in.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/nghttp2_amd_hd.h"
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
// `what` names the failed call; the sharded engine, which names none, passes nullptr
inline bool hip_ok(hipError_t e, const char *layer, const char *what) {
  if (e == hipSuccess) return true;
  if (what)
    fprintf(stderr, "nghttp2_amd_hd (%s): %s: %s\n", layer, what, hipGetErrorString(e));
  else
    fprintf(stderr, "nghttp2_amd_hd (%s): HIP error %s\n", layer, hipGetErrorString(e));
  return false;
}
// The C ABI's report of a launch or runtime call of the kernel layers (the
// .hip files, which name no layer): 0, or the message and FATAL.
inline int hip_rv(hipError_t e) {
  if (e == hipSuccess) return 0;
  fprintf(stderr, "nghttp2_amd_hd: HIP error %s\n", hipGetErrorString(e));
  return NGHTTP2_AMD_ERR_FATAL;
}
inline size_t round16(size_t x) { return (x + 15u) & ~size_t(15); }
// Buffers that grow and never shrink.  Their owner releases them explicitly: no
// destructor calls HIP (the engines' singletons outlive the runtime at exit).
struct Buf {
  void *p = nullptr;
  size_t cap = 0;
  template <class T> T *as() const { return static_cast<T *>(p); }
};
// On the current device.  padded: a grown buffer gets round16(need) + 256
// bytes (the sharded engine's policy), else exactly need.
struct DevBuf : Buf {
  bool reserve(size_t need, const char *layer, const char *what = "hipMalloc", bool padded = false) {
    if (need <= cap) return true;
    release();
    if (padded) need = round16(need) + 256;
    if (!hip_ok(hipMalloc(&p, need), layer, what)) return false;
    cap = need;
    return true;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
// In pinned host memory.  mapped: mapped into the device's address space and
// coherent (a pool the kernels read or write directly; a non-coherent mapping
// measured the same, profiles/r05/inflate/pin_modes.log), else plain pinned
// memory the device only reaches by DMA copies.
struct PinnedBuf : Buf {
  bool reserve(size_t need, const char *layer, bool mapped) {
    if (need <= cap) return true;
    release();
    const unsigned flags = mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault;
    if (!hip_ok(hipHostMalloc(&p, need, flags), layer, "hipHostMalloc")) return false;
    cap = need;
    return true;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace hdhost
