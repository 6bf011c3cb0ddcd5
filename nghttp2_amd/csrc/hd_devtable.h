// hd_devtable.h -- a set of HPACK dynamic tables in device memory, stated once.
//
// What the device inflaters (hd_replay.hip) and the device deflaters
// (hd_deflate_dev.hip) share: the set -- per connection a 32-byte header, a
// ring of table_bytes / 32 entry descriptors, for the deflaters a parallel
// array of keys, and two byte stores of table_bytes -- with its allocation,
// read-back and change of a table size; what a walk leaves the commit (Left);
// the wave's copy of byte runs; and the commit.  The walk, its table and the
// header and descriptors a commit leaves are hd_replay.h's, as is the host's
// commit.  HIP: included by the two .hip files only.
#ifndef NGHTTP2_AMD_HD_DEVTABLE_H
#define NGHTTP2_AMD_HD_DEVTABLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <vector>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_host.h"
#include "hd_replay.h"

namespace hdtable {

using hdreplay::Conn;
using hdreplay::Entry;
using hdreplay::Ref;

// The two public set types are this and nothing more.
struct Set {
  uint32_t nconn, table_bytes;
  Conn *hdr;      // [nconn]
  Entry *ring;    // [nconn][table_bytes / 32]
  uint32_t *key;  // [nconn][table_bytes / 32], or null (the inflaters)
  uint8_t *store; // [nconn][2][table_bytes]
};

// (a table reference is a uint32 offset into the set's store allocation)
inline bool set_args_ok(const void *set_ptr, uint32_t nconn, uint32_t table_bytes) {
  return set_ptr && nconn != 0 && hdreplay::table_bytes_ok(table_bytes) &&
         (uint64_t)nconn * 2u * table_bytes <= 0xFFFFFFFFull;
}
template <class S>
void set_del(S *set) {
  if (!set) return;
  if (set->hdr) (void)hipFree(set->hdr);
  if (set->ring) (void)hipFree(set->ring);
  if (set->key) (void)hipFree(set->key);
  if (set->store) (void)hipFree(set->store);
  delete set;
}
// A set with its device memory, for arguments that are set_args_ok; the
// headers are the caller's to fill.
template <class S>
int set_new(S **set_ptr, uint32_t nconn, uint32_t table_bytes, bool with_key) {
  S *s = new (std::nothrow) S();
  if (!s) return NGHTTP2_AMD_ERR_NOMEM;
  s->nconn = nconn;
  s->table_bytes = table_bytes;
  const size_t slots = table_bytes / hdreplay::kOverhead;
  if (hipMalloc((void **)&s->hdr, (size_t)nconn * sizeof(Conn)) != hipSuccess ||
      hipMalloc((void **)&s->ring, (size_t)nconn * slots * sizeof(Entry)) != hipSuccess ||
      (with_key && hipMalloc((void **)&s->key, (size_t)nconn * slots * sizeof(uint32_t)) != hipSuccess) ||
      hipMalloc((void **)&s->store, (size_t)nconn * 2u * table_bytes) != hipSuccess) {
    set_del(s);
    return NGHTTP2_AMD_ERR_NOMEM;
  }
  *set_ptr = s;
  return 0;
}

// One connection's header, its live entries (hdreplay::ring_entries) and its
// current store buffer to the host; both copies are waited for.
inline int set_read(const Set *set, uint32_t conn, Conn *hdr, uint32_t *entries, uint8_t *bytes, void *stream) {
  if (!set || conn >= set->nconn || !hdr || !entries || !bytes) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t tb = set->table_bytes, slots = tb / hdreplay::kOverhead;
  std::vector<Entry> ring(slots);
  hipError_t e = hipMemcpyAsync(hdr, set->hdr + conn, sizeof(Conn), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(ring.data(), set->ring + (size_t)conn * slots, slots * sizeof(Entry), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(bytes, set->store + (size_t)(2u * conn + (hdr->cur & 1u)) * tb, tb, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hdhost::hip_rv(e);
  return hdreplay::ring_entries(*hdr, ring.data(), slots, entries) ? 0 : NGHTTP2_AMD_ERR_FATAL;
}

constexpr uint32_t CS_WG = 64;  // k_change_size: one wave, 64 changes

// Change i sets connection conn[i]'s table size by Rule, a lane per change:
// Rule()(header, ring, table_bytes, value) is the change's result.
template <class Rule>
__global__ __launch_bounds__(CS_WG) void k_change_size(Conn *__restrict__ hdr, const Entry *__restrict__ ring,
                                                       uint32_t nconn, uint32_t table_bytes,
                                                       const uint32_t *__restrict__ conn,
                                                       const uint32_t *__restrict__ value, int32_t *__restrict__ rv,
                                                       uint32_t n) {
  const uint32_t i = blockIdx.x * CS_WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = conn[i];
  if (c >= nconn) {
    rv[i] = NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
    return;
  }
  Conn h = hdr[c];
  rv[i] = Rule()(&h, ring + (size_t)c * (table_bytes / hdreplay::kOverhead), table_bytes, value[i]);
  hdr[c] = h;
}
template <class Rule>
int set_change_size(Set *set, const uint32_t *conn, const uint32_t *value, int32_t *rv, uint32_t n, void *stream) {
  if (n == 0) return 0;
  if (!set || !conn || !value || !rv) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_change_size<Rule>, dim3((n + CS_WG - 1u) / CS_WG), dim3(CS_WG), 0, (hipStream_t)stream,
                     set->hdr, (const Entry *)set->ring, set->nconn, set->table_bytes, conn, value, rv, n);
  return hdhost::hip_rv(hipGetLastError());
}

// What a walk (k_replay, k_deflate_plan) leaves k_commit for a connection
// that had blocks.
struct Left {  // 64 bytes
  Conn h;
  uint32_t nnew, nhead, nold, walked;
  uint32_t pad[4];
};

// The wave copies the byte runs of the lanes with `has`, one lane's after the
// other, its lanes on consecutive bytes.  A lane has two runs, r0 and then r1
// behind it (a name and its value; an empty r1 for a single run), to
// out[d, ...), each with a NUL behind it when nul.  src is the source policy:
// it turns a broadcast run into a pointer, src.ptr(off, ls), and its length,
// src.len(ls), and says whether byte b of a run at off is there to be read,
// src.readable(off, b).  Every store is below cap.  D is the type of d and
// cap: uint64_t, or uint32_t where the destination is smaller than 4 GiB.
template <class Src, class D>
__device__ __forceinline__ void wave_copy(const Src &src, bool has, Ref r0, Ref r1, D d, uint8_t *out, D cap,
                                          bool nul, uint32_t lane) {
  uint64_t m = __ballot(has);
  while (m) {
    const int l = __builtin_ctzll(m);
    m &= m - 1ull;
    const uint32_t o0 = (uint32_t)__builtin_amdgcn_readlane((int)r0.off, l);
    const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)r0.ls, l);
    const uint32_t o1 = (uint32_t)__builtin_amdgcn_readlane((int)r1.off, l);
    const uint32_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)r1.ls, l);
    D t0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)d, l);
    if constexpr (sizeof(D) == 8) {
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)d >> 32), l);
      t0 |= (D)hi << 32;
    }
    const uint32_t n0 = src.len(w0), n1 = src.len(w1);
    const D t1 = t0 + n0 + (nul ? 1u : 0u);
    const uint8_t *f0 = src.ptr(o0, w0), *f1 = src.ptr(o1, w1);
    // (the part of each run whose stores lie below cap, found once: the byte loops test no store)
    const uint32_t m0 = t0 >= cap ? 0u : cap - t0 < n0 ? (uint32_t)(cap - t0) : n0;
    const uint32_t m1 = t1 >= cap ? 0u : cap - t1 < n1 ? (uint32_t)(cap - t1) : n1;
    // (a run is seldom longer than a trip: interleaved or unrolled loops only cost registers)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (uint32_t b = lane; b < m0; b += 64u)
      if (src.readable(o0, b)) out[t0 + b] = f0[b];
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (uint32_t b = lane; b < m1; b += 64u)
      if (src.readable(o1, b)) out[t1 + b] = f1[b];
    if (nul && lane == 0u) {
      if (t0 + n0 < cap) out[t0 + n0] = 0u;
      if (t1 + n1 < cap) out[t1 + n1] = 0u;
    }
  }
}

// A single run per lane, no NUL.
template <class Src, class D>
__device__ __forceinline__ void wave_copy(const Src &src, bool has, Ref r, D d, uint8_t *out, D cap, uint32_t lane) {
  wave_copy(src, has, r, Ref{0u, 0u}, d, out, cap, false, lane);
}

// One byte array with its size as a source: a run's ls is its plain length,
// and the bytes of it the array holds are readable.
struct Span {
  const uint8_t *base;
  uint64_t bytes;
  __device__ const uint8_t *ptr(uint32_t off, uint32_t) const { return base + off; }
  __device__ uint32_t len(uint32_t ls) const { return ls; }
  __device__ bool readable(uint32_t off, uint32_t b) const { return (uint64_t)off + b < bytes; }
};

// The commit of connection c by one wave: the live entries' bytes go back to
// back into the connection's other store buffer, their descriptors become
// table references, with kKeys the keys of the entries that entered move from
// fresh_key to ring_key, and the header is written back with the
// current-buffer bit flipped.  Src is a wave_copy policy over Refs with
// src.ok(Ref): the Ref lies inside its store.  An entry whose Refs do not, or
// whose bytes the buffer cannot hold, is committed empty: nothing is read
// through it and every byte stored is below table_bytes.
template <bool kKeys, class Src>
__device__ __forceinline__ void commit(const Src &src, uint32_t c, uint32_t lane, const Left *left, const Entry *fresh,
                                       const uint32_t *fresh_key, Conn *hdr, Entry *ring, uint32_t *ring_key,
                                       uint8_t *store, uint32_t table_bytes) {
  const Left l = left[c];
  if (!l.walked) return;
  const uint32_t slots = table_bytes / hdreplay::kOverhead, mask = slots - 1u;
  Entry *cring = ring + (size_t)c * slots;
  const Entry *cfresh = fresh + (size_t)c * slots;
  const Conn after = hdreplay::committed_conn(l.h, l.nnew, l.nold, mask);
  const uint32_t cur_off = (2u * c + (l.h.cur & 1u)) * table_bytes;
  uint8_t *to = store + (size_t)(2u * c + after.cur) * table_bytes;
  const uint32_t count = min(after.count, slots), head = after.head;
  // The slots of the entries that stay, ring[h.head + j], are the slots they
  // end in, head + nnew + j: a lane reads the descriptor it then replaces,
  // and the fresh entries go in front of them, into slots no live entry has.
  // So an entry that stays keeps its key too.
  uint32_t run = 0;
  for (uint32_t i0 = 0; i0 < count; i0 += 64u) {
    const uint32_t i = i0 + lane;
    const bool live = i < count;
    Entry e = {};
    if (live) {
      if (i < l.nnew) {
        e = cfresh[(l.nhead + i) & mask];
        if constexpr (kKeys)
          ring_key[(size_t)c * slots + ((head + i) & mask)] = fresh_key[(size_t)c * slots + ((l.nhead + i) & mask)];
      } else {
        e = cring[(l.h.head + (i - l.nnew)) & mask];
        e.name.off += cur_off;
        e.value.off += cur_off;
      }
    }
    const uint32_t nl = hdreplay::ref_len(e.name), vl = hdreplay::ref_len(e.value);
    const bool ok = live && src.ok(e.name) && src.ok(e.value);
    const uint32_t len = ok ? nl + vl : 0u;
    uint32_t inc = len;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    const uint32_t at = run + inc - len;
    const bool fits = ok && (uint64_t)at + len <= table_bytes;
    wave_copy(src, fits, e.name, e.value, at, to, table_bytes, false, lane);
    if (live) cring[(head + i) & mask] = hdreplay::committed_entry(at, fits ? nl : 0u, fits ? vl : 0u);
    run += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  }
  if (lane == 0u) hdr[c] = after;
}

}  // namespace hdtable

#endif  // NGHTTP2_AMD_HD_DEVTABLE_H
