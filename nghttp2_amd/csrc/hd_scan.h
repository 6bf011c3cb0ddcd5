// hd_scan.h -- the one-workgroup exclusive prefix the scan kernels share
// (k_parse_scan, k_lit_scan of hd_parse.hip; k_replay_scan of hd_replay.hip):
// k_tile_prefix64's scheme over uint32 counts with 64-bit sums, so a total
// past the uint32 offsets is seen, not wrapped.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdscan {

constexpr uint32_t SC_WG = 1024;  // the scans: one workgroup

// The exclusive prefix of x[0, n), by one workgroup of SC_WG threads
// (k_tile_prefix64's scheme: a thread owns a contiguous share, the shares'
// sums are scanned across the wave and the waves' sums through LDS).
// scan_sums leaves the thread's share [b, e) and the sum before it and
// returns the total; scan_write stores the prefixes and the total at out[0, n]
// (out may be x itself: the prefix in place).
struct Share {
  uint32_t b, e;
  uint64_t run;
};
__device__ __forceinline__ uint64_t scan_sums(const uint32_t *x, uint32_t n, uint64_t *wsum, Share *sh) {
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t per = n / SC_WG + (n % SC_WG ? 1u : 0u);
  const uint32_t b = min(t * per, n), e = min(b + per, n);
  uint64_t s = 0;
  // (the share's loads are independent: unrolled, eight are in flight at a
  // time -- one by one, their latency was the whole kernel: DESIGN.md 2.12)
#pragma unroll 8
  for (uint32_t i = b; i < e; ++i) s += x[i];
  uint64_t inc = s;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint64_t v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (lane == 63u) wsum[wv] = inc;
  __syncthreads();
  uint64_t run = inc - s, total = 0;
  for (uint32_t w = 0; w < SC_WG / 64u; ++w) {
    if (w < wv) run += wsum[w];
    total += wsum[w];
  }
  sh->b = b;
  sh->e = e;
  sh->run = run;
  return total;
}
__device__ __forceinline__ void scan_write(const uint32_t *x, uint32_t *out, uint32_t n, const Share &sh,
                                           uint64_t total) {
  uint64_t run = sh.run;
  uint32_t i = sh.b;
  // (a thread reads x[i] before it stores out[i], and only its share; eight
  // loads ahead of the eight stores)
  for (; i + 8u <= sh.e; i += 8u) {
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = x[i + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      out[i + k] = (uint32_t)run;
      run += v[k];
    }
  }
  for (; i < sh.e; ++i) {
    const uint32_t v = x[i];
    out[i] = (uint32_t)run;
    run += v;
  }
  if (threadIdx.x == 0) out[n] = (uint32_t)total;
}

}  // namespace hdscan
