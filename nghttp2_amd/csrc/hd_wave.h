// hd_wave.h -- the device helpers the kernels of hd_huff.hip, hd_check.hip,
// hd_http.hip and hd_names.hip (the LDS pointer type) share:
// address-space-explicit LDS pointer types, the hand-over between lanes of
// one wave through LDS, DPP row shifts, and the helpers over a chunk of 16
// class bytes held as four dwords.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Address-space-explicit pointers, so LDS staging compiles to ds_* and
// global output to global_* (never flat_*).
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

// A wave's LDS accesses before this point are complete and visible to all of
// its lanes after it (release fence, wave barrier, acquire fence): the
// hand-over between lanes of one wave through LDS, no workgroup barrier.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One DPP step of a wave-wide scan (row shifts within 16-lane rows, then row
// broadcasts of lanes 15 and 31): VALU only, no LDS round trips.  Lanes whose
// DPP source lies outside the row read 0, the identity of add / max / or over
// unsigned values.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp0(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {  // uniform result
  v = max(v, dpp0<0x111>(v));
  v = max(v, dpp0<0x112>(v));
  v = max(v, dpp0<0x114>(v));
  v = max(v, dpp0<0x118>(v));
  v = max(v, dpp0<0x142, 0xa>(v));
  v = max(v, dpp0<0x143, 0xc>(v));
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ uint64_t ones64(uint32_t k) {  // the low k bits, k <= 64
  return k >= 64u ? ~0ull : (1ull << k) - 1ull;
}

// OR of the class bytes [lo, hi) of a chunk's sixteen (0 <= lo, hi <= 16; an
// empty range gives 0)
__device__ __forceinline__ uint32_t or_bytes(const uint32_t w[4], uint32_t lo, uint32_t hi) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // the bytes of dword k inside the range: [l, h) of its four
    const int32_t l = max((int32_t)lo - 4 * k, 0), h = min((int32_t)hi - 4 * k, 4);
    if (l < h) {
      const uint32_t below_h = h == 4 ? 0xFFFFFFFFu : (1u << (8 * h)) - 1u;
      r |= w[k] & below_h & ~((1u << (8 * l)) - 1u);
    }
  }
  r |= r >> 16;
  return (r | (r >> 8)) & 0xFFu;
}
__device__ __forceinline__ uint32_t byte_at(const uint32_t w[4], uint32_t i) {
  const uint32_t d = i >> 2;
  const uint32_t x = d == 0 ? w[0] : d == 1 ? w[1] : d == 2 ? w[2] : w[3];
  return (x >> (8u * (i & 3u))) & 0xFFu;
}
// the first of the class bytes [lo, hi) of a chunk's sixteen with `bit` set, or 16
__device__ __forceinline__ uint32_t first_with(const uint32_t w[4], uint32_t bit, uint32_t lo, uint32_t hi) {
  uint32_t r = 16u;
#pragma unroll
  for (int i = 15; i >= 0; --i)
    if ((uint32_t)i >= lo && (uint32_t)i < hi && ((w[i >> 2] >> (8 * (i & 3))) & bit)) r = (uint32_t)i;
  return r;
}
