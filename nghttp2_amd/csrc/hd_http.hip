// hd_http.hip -- batched value facts of nghttp2_http_on_header for gfx950.
//
// Reference: the byte work of http_request_on_header / http_response_on_header
// (lib/nghttp2_http.c:188-403) that the nghttp2_check_* masks (hd_check.hip)
// do not cover: check_authority without '@' (:168-176), check_scheme
// (:118-140), lws (:142-150), parse_uint (:65-89) and the comparisons against
// "HEAD" / "CONNECT" / "OPTIONS", "http" / "https", "trailers", "*" and "/".
// N strings in the batch layout (byte pool + uint32 offsets[N+1], optionally a
// length per string: the output of decode_batch_auto) give facts[N]
// (NGHTTP2_AMD_HTTP_FACT_*) and number[N] (parse_uint's value or -1).
//
// Layout and bound: k_check_fields' walk (hd_check.hip), a second instance
// with its own class table (hd_http.h: five class bits per byte).  A wave
// owns 64 consecutive strings and reads the bytes they span as aligned
// 16-byte chunks, 64 per round, whatever the string lengths; the whole-string
// properties are ORs of per-byte classes, taken as wave ballots over the
// chunks strictly inside a string and by byte over its head and tail chunk,
// so bytes outside [a, b) reach no string and no wave waits on its longest
// string for them.
// What is left belongs to the string's own lane: the comparisons against the
// short literals read the string's first min(len, 8) bytes (a second read of
// its head chunk, cached), and a string that turned out to be all digits is
// evaluated there from its first byte that is not '0': at most 19 digits, read
// and run through parse_uint's exact overflow test (more than 19 overflow for
// certain).  That position comes out of the walk as well -- the fifth ballot
// is "the chunk holds a byte that is not '0'", a string lane keeps the first
// such chunk strictly inside its string and looks into its class bytes in
// the round's LDS scratch once -- so no lane walks a run of leading zeros:
// the work per string is bounded whatever the bytes are.
// HBM traffic: the strings' bytes + 4 (or 8, with lengths) in, 12 out per
// string -- a byte scan, no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_host.h"
#include "hd_http.h"
#include "hd_string_walk.h"

namespace {

constexpr uint32_t HF_WG = 256;  // four waves, 64 strings each
constexpr int NB = hdhttp::kBallots;

__constant__ hdhttp::Table kHttpTable = hdhttp::kTable;

__global__ __launch_bounds__(HF_WG) void k_http_facts(const uint8_t *__restrict__ pool,
                                                      const uint32_t *__restrict__ off,
                                                      const int32_t *__restrict__ len, uint32_t n,
                                                      uint32_t *__restrict__ facts,
                                                      int64_t *__restrict__ number) {
  __shared__ uint8_t clsT_[256];
  __shared__ alignas(16) uint32_t scratch[HF_WG / 64][2][256];
  static_assert(HF_WG == 256, "one table entry per thread");
  static_assert(hdhttp::kNotDigit == 1u << 2 && hdhttp::kNotZero == 1u << (NB - 1), "the ballots the walk names");
  clsT_[threadIdx.x] = kHttpTable.cls[threadIdx.x];
  __syncthreads();  // the only workgroup barrier
  const lds_u8 *clsT = (const lds_u8 *)clsT_;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * HF_WG + 64u * wv;  // the wave's strings
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
  const uint32_t ca = a >> 4, cz = ne ? (b - 1u) >> 4 : ca;
  uint32_t H[4] = {0, 0, 0, 0}, T[4] = {0, 0, 0, 0};
  uint32_t acc[NB] = {0, 0, 0, 0, 0};  // class k: dirty chunks strictly between head and tail
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  uint32_t nz = kNone;  // pool offset of the first byte that is not '0' in those chunks
  auto round = [&](uint32_t cb, const uint4 &qv, bool ok, lds_u32 *buf) {
    const uint32_t wd[4] = {qv.x, qv.y, qv.z, qv.w};
    u32x4 cw;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      cw[k] = (uint32_t)clsT[wd[k] & 0xFFu] | ((uint32_t)clsT[(wd[k] >> 8) & 0xFFu] << 8) |
              ((uint32_t)clsT[(wd[k] >> 16) & 0xFFu] << 16) | ((uint32_t)clsT[wd[k] >> 24] << 24);
    *(lds_u32x4 *)(buf + 4u * lane) = cw;
    uint32_t o = cw[0] | cw[1] | cw[2] | cw[3];
    o |= o >> 16;
    o |= o >> 8;
    if (!ok) o = 0;  // a chunk past the wave's bytes
    uint64_t dirty[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) dirty[k] = __ballot((o >> k) & 1u);
    wave_lds_sync();
    const uint32_t ra = ca - cb, rz = cz - cb;
    if (ne && ra < 64u) {
      const u32x4 v = *(const lds_u32x4 *)(buf + 4u * ra);
      H[0] = v.x, H[1] = v.y, H[2] = v.z, H[3] = v.w;
    }
    if (ne && rz < 64u) {
      const u32x4 v = *(const lds_u32x4 *)(buf + 4u * rz);
      T[0] = v.x, T[1] = v.y, T[2] = v.z, T[3] = v.w;
    }
    const int32_t lo = max((int32_t)(ca + 1u) - (int32_t)cb, 0), hi = min((int32_t)cz - (int32_t)cb, 64);
    if (lo < hi) {
      const uint64_t m = ones64((uint32_t)hi) & ~ones64((uint32_t)lo);
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const uint64_t t = dirty[k] & m;
        acc[k] |= (uint32_t)t | (uint32_t)(t >> 32);
      }
      // (rounds come in ascending order: the first hit is the earliest)
      const uint64_t tz = dirty[NB - 1] & m;
      if (nz == kNone && tz) {
        const uint32_t idx = (uint32_t)__builtin_ctzll(tz);
        // a chunk that also holds a byte that is no digit: the string is no
        // number and the position is never asked for (any value but kNone
        // ends the search) -- the common case, which then reads nothing
        if ((dirty[2] >> idx) & 1ull) {
          nz = 0u;
        } else {
          const u32x4 v = *(const lds_u32x4 *)(buf + 4u * idx);
          const uint32_t cw4[4] = {v.x, v.y, v.z, v.w};
          nz = ((cb + idx) << 4) + first_with(cw4, hdhttp::kNotZero, 0u, 16u);
        }
      }
    }
  };
  // every lane loads on every round (a chunk past the wave's bytes at a
  // clamped index, not used), as k_check_fields
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
  uint32_t f = NGHTTP2_AMD_HTTP_FACT_INVALID;
  int64_t num = -1;
  if (valid) {
    uint32_t all = 0, rest = 0, first = 0;
    uint64_t head = 0;
    if (ne) {
      const uint32_t p = a & 15u, q = ((b - 1u) & 15u) + 1u;  // [p, 16) of the head, [0, q) of the tail
      const bool same = ca == cz;
#pragma unroll
      for (int k = 0; k < NB; ++k) rest |= acc[k] ? 1u << k : 0u;
      if (!same) rest |= or_bytes(T, 0u, q);
      rest |= or_bytes(H, p + 1u, same ? q : 16u);
      first = byte_at(H, p);
      all = rest | first;
      // the string's own first bytes, [a, min(a + 8, b)): inside the string
      const uint32_t hn = min(b - a, 8u);
      for (uint32_t i = 0; i < hn; ++i) head |= (uint64_t)pool[(size_t)a + i] << (8u * i);
      // all digits: the value, from the first byte that is not '0' -- in
      // the head chunk's own bytes, else in the chunks between, else in the
      // tail's -- to the end: z in [a, b), at most 19 bytes of it are read
      if (!(all & hdhttp::kNotDigit)) {
        uint32_t z = kNone;
        const uint32_t hz = first_with(H, hdhttp::kNotZero, p, same ? q : 16u);
        if (hz < 16u) {
          z = (ca << 4) + hz;
        } else if (nz != kNone) {
          z = nz;
        } else if (!same) {
          const uint32_t tz = first_with(T, hdhttp::kNotZero, 0u, q);
          if (tz < 16u) z = (cz << 4) + tz;
        }
        num = z == kNone ? 0 : hdhttp::digits_value(pool + (size_t)z, (size_t)(b - z));
      }
    }
    f = hdhttp::facts_of(b - a, all, rest, first, head, num < 0);
  }
  facts[t0 + lane] = f;
  number[t0 + lane] = num;
}

}  // namespace

extern "C" {

int nghttp2_amd_hd_http_facts_batch(const uint8_t *pool, const uint32_t *off, const int32_t *len, uint32_t n,
                                    uint32_t *facts, int64_t *number, void *stream) {
  if (n == 0) return 0;
  if (!pool || !off || !facts || !number) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_http_facts, dim3((n + HF_WG - 1u) / HF_WG), dim3(HF_WG), 0, (hipStream_t)stream, pool, off,
                     len, n, facts, number);
  return hdhost::hip_rv(hipGetLastError());
}

uint32_t nghttp2_amd_hd_http_facts(const uint8_t *s, size_t len, int64_t *number) {
  if (!s) len = 0;
  return hdhttp::http_facts(s, len, number);
}

int nghttp2_amd_hd_http_on_header(nghttp2_amd_hd_http_state *state, uint32_t mode, const uint8_t *name,
                                  size_t name_len, size_t value_len, int32_t token, uint8_t name_mask,
                                  uint8_t value_mask, uint32_t value_facts, int64_t value_number) {
  if (!state) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  if (!name) name_len = 0;
  return hdhttp::on_header(state, mode,
                           hdhttp::Field{name, name_len, value_len, token, name_mask, value_mask, value_facts,
                                         value_number});
}

int nghttp2_amd_hd_http_on_request_headers(nghttp2_amd_hd_http_state *state, uint32_t mode) {
  if (!state) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  return hdhttp::on_request_headers(state, mode);
}

int nghttp2_amd_hd_http_on_response_headers(nghttp2_amd_hd_http_state *state) {
  if (!state) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  return hdhttp::on_response_headers(state);
}

}  // extern "C"
