// hd_check.hip -- batched header-field validation (nghttp2_check_*) for gfx950.
//
// Reference: the table-driven byte scans of lib/nghttp2_helper.c:346-558
// (nghttp2_check_header_name, _nonempty_header_name, _header_value,
// _header_value_rfc9113, _method, _path, _authority), which
// nghttp2_http_on_header (lib/nghttp2_http.c:405-447) runs on every name and
// value the inflater emits.  Here N strings in the batch layout (byte pool +
// uint32 offsets[N+1], optionally a length per string: the output of
// decode_batch_auto) give mask[N], one NGHTTP2_AMD_CHECK_* byte per string.
//
// Layout and bound: k_enc_count's walk (hd_huff.hip).  A wave owns 64
// consecutive strings, reads the bytes they span as aligned 16-byte chunks,
// 64 per round (one per lane, two rounds in flight), whatever the string
// lengths: a 4 KB cookie among 63 short strings costs every lane the same.
// A check is a predicate over a string's bytes -- "no byte of [a, b) violates
// table k" -- so nothing is counted and no length can wrap anything:
//   chunk lane   one LDS lookup per byte in the 256-byte class table
//                (hd_field_classes.h: five violation bits and two position
//                markers per byte); the chunk's 16 class bytes go to the
//                wave's LDS scratch, their OR to five wave ballots, the
//                round's "chunk is dirty for class k" bits as scalar pairs;
//   string lane  ORs the ballot bits of the chunks strictly inside its
//                string into five accumulators, and keeps the class bytes of
//                the two chunks at its ends (its head and tail chunk); after
//                the last round it masks those two to its own byte range.
// Bytes outside [a, b) -- a neighbour's in a shared chunk, the gaps between
// decode tasks, the pool padding, the bytes before the first string -- reach
// no string: the ballots are taken only over chunks that lie wholly inside
// it, and the two edge chunks are masked by byte.
// HBM traffic: the strings' bytes + 4 (or 8, with lengths) in, 1 out per
// string -- a byte scan, no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_field_classes.h"
#include "hd_host.h"
#include "hd_string_walk.h"

namespace {

constexpr uint32_t CK_WG = 256;  // four waves, 64 strings each

__constant__ hdcls::Table kClsTable = hdcls::kTable;

__global__ __launch_bounds__(CK_WG) void k_check_fields(const uint8_t *__restrict__ pool,
                                                        const uint32_t *__restrict__ off,
                                                        const int32_t *__restrict__ len, uint32_t n,
                                                        uint8_t *__restrict__ mask) {
  // (the table as k_enc_count's lenT: one byte per entry, four entries a bank)
  __shared__ uint8_t clsT_[256];
  // a round's class bytes, 16 per chunk lane; two buffers, one per round of
  // the unrolled loop, so a round needs one hand-over, not two
  __shared__ alignas(16) uint32_t scratch[CK_WG / 64][2][256];
  static_assert(CK_WG == 256, "one table entry per thread");
  clsT_[threadIdx.x] = kClsTable.cls[threadIdx.x];
  __syncthreads();  // the only workgroup barrier
  const lds_u8 *clsT = (const lds_u8 *)clsT_;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * CK_WG + 64u * wv;  // the wave's strings
  if (t0 >= n) return;
  const uint32_t nstr = min(n - t0, 64u);
  const bool sl = lane < nstr;
  // string l in lane l: bytes [a, b); a string that is not examined is empty
  // here and reads nothing
  hdwalk::Range r = {0u, 0u, false};
  if (sl) r = hdwalk::string_range(off, len, t0 + lane);
  const uint32_t a = r.a, b = r.b;
  const bool valid = r.valid;
  // the wave's span [A, Z): from its first examined string to the furthest end
  const uint32_t A = ~wave_max(valid ? ~a : 0u), Z = wave_max(b);
  const bool any = __ballot(valid) != 0ull;
  const uint32_t c0 = any ? A >> 4 : 0u;
  const uint32_t c_end = any ? (Z + 15u) >> 4 : 0u;
  const bool ne = a < b;
  // the string's head and tail chunk (one and the same for a string inside a chunk)
  const uint32_t ca = a >> 4, cz = ne ? (b - 1u) >> 4 : ca;
  uint32_t H[4] = {0, 0, 0, 0}, T[4] = {0, 0, 0, 0};
  uint32_t acc[5] = {0, 0, 0, 0, 0};  // class k: dirty chunks strictly between head and tail
  // one round: the 64 chunks from chunk cb, this lane's in qv
  auto round = [&](uint32_t cb, const uint4 &qv, bool ok, lds_u32 *buf) {
    const uint32_t wd[4] = {qv.x, qv.y, qv.z, qv.w};
    u32x4 cw;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      cw[k] = (uint32_t)clsT[wd[k] & 0xFFu] | ((uint32_t)clsT[(wd[k] >> 8) & 0xFFu] << 8) |
              ((uint32_t)clsT[(wd[k] >> 16) & 0xFFu] << 16) | ((uint32_t)clsT[wd[k] >> 24] << 24);
    // (lane strides of 16 bytes: the least a 16-byte store can take)
    *(lds_u32x4 *)(buf + 4u * lane) = cw;
    uint32_t o = cw[0] | cw[1] | cw[2] | cw[3];
    o |= o >> 16;
    o |= o >> 8;
    if (!ok) o = 0;  // a chunk past the wave's bytes
    uint64_t dirty[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) dirty[k] = __ballot((o >> k) & 1u);
    wave_lds_sync();
    // the string's head and tail chunk, when this round holds them
    const uint32_t ra = ca - cb, rz = cz - cb;
    if (ne && ra < 64u) {
      const u32x4 v = *(const lds_u32x4 *)(buf + 4u * ra);
      H[0] = v.x, H[1] = v.y, H[2] = v.z, H[3] = v.w;
    }
    if (ne && rz < 64u) {
      const u32x4 v = *(const lds_u32x4 *)(buf + 4u * rz);
      T[0] = v.x, T[1] = v.y, T[2] = v.z, T[3] = v.w;
    }
    // its chunks strictly between the two, in this round: lanes [lo, hi)
    // (chunk numbers are below 2^28: the pool is below 4 GiB)
    const int32_t lo = max((int32_t)(ca + 1u) - (int32_t)cb, 0), hi = min((int32_t)cz - (int32_t)cb, 64);
    if (lo < hi) {
      const uint64_t m = ones64((uint32_t)hi) & ~ones64((uint32_t)lo);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const uint64_t t = dirty[k] & m;
        acc[k] |= (uint32_t)t | (uint32_t)(t >> 32);
      }
    }
  };
  // every lane loads on every round (a chunk past the wave's bytes at a
  // clamped index, not used): the count of loads in flight is the same on
  // every path, so the loop waits for the older of two, not for both
  const uint32_t c_last = max(c_end, c0 + 1u) - 1u;
  auto load = [&](uint32_t c, bool &ok) -> uint4 {
    ok = c < c_end;
    return *reinterpret_cast<const uint4 *>(pool + ((size_t)min(c, c_last) << 4));
  };
  lds_u32 *buf0 = (lds_u32 *)scratch[wv][0], *buf1 = (lds_u32 *)scratch[wv][1];
  bool oka, okb;
  uint4 qa = load(c0 + lane, oka), qb = load(c0 + 64u + lane, okb);
  for (uint32_t cb = c0; cb < c_end; cb += 128u) {
    round(cb, qa, oka, buf0);
    qa = load(cb + 128u + lane, oka);
    if (cb + 64u >= c_end) break;
    round(cb + 64u, qb, okb, buf1);
    qb = load(cb + 192u + lane, okb);
  }
  if (!sl) return;
  uint32_t m = NGHTTP2_AMD_CHECK_INVALID;
  if (valid) {
    uint32_t all = 0, rest = 0, first = 0, last = 0;
    if (ne) {
      const uint32_t p = a & 15u, q = ((b - 1u) & 15u) + 1u;  // [p, 16) of the head, [0, q) of the tail
      const bool same = ca == cz;
#pragma unroll
      for (int k = 0; k < 5; ++k) rest |= acc[k] ? 1u << k : 0u;
      if (!same) rest |= or_bytes(T, 0u, q);
      rest |= or_bytes(H, p + 1u, same ? q : 16u);
      first = byte_at(H, p);
      last = byte_at(T, q - 1u);
      all = rest | first;
    }
    m = hdcls::mask_of(b - a, all, rest, first, last);
  }
  mask[t0 + lane] = (uint8_t)m;
}

}  // namespace

extern "C" {

int nghttp2_amd_hd_check_fields_batch(const uint8_t *pool, const uint32_t *off, const int32_t *len,
                                      uint32_t n, uint8_t *mask, void *stream) {
  if (n == 0) return 0;
  if (!pool || !off || !mask) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_check_fields, dim3((n + CK_WG - 1u) / CK_WG), dim3(CK_WG), 0, (hipStream_t)stream,
                     pool, off, len, n, mask);
  return hdhost::hip_rv(hipGetLastError());
}

uint8_t nghttp2_amd_hd_check_field(const uint8_t *s, size_t len) {
  if (!s) len = 0;
  return hdcls::check_field(s, len);
}

}  // extern "C"
