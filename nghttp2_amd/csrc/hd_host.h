// hd_host.h -- what the host layers above the C ABI share (hd_inflate.cpp,
// hd_deflate.cpp, hd_sharded.cpp): the HPACK static table (hd_static.h), the
// HIP error reports (hip_rv is the kernel layers' own, the .hip files'), the
// workspace carver of the .hip files' layouts, and the growable device and
// pinned host buffers the layers stage their batches in.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_static.h"
#include "hd_tokens.h"

namespace hdhost {

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
inline uint32_t clamp32(size_t x) { return x > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)x; }
// A caller's workspace cut into arrays, one after the other: take<T>(count)
// is the next one, at the next multiple of `align` (a power of two).  With
// base = nullptr only the offsets count: total() is what the layout needs,
// the size the *_workspace_size functions report (part of the ABI).
struct Carve {
  void *base;
  size_t at = 0;
  template <class T> T *take(size_t count, size_t align = 16) {
    const size_t from = (at + align - 1u) & ~(align - 1u);
    at = from + count * sizeof(T);
    return reinterpret_cast<T *>((uintptr_t)base + from);
  }
  size_t total() const { return round16(at); }
};
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
