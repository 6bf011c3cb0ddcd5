// hd_replay.hip -- device-resident HPACK inflaters: parsed blocks into fields, for gfx950.
//
// Reference: the table half of nghttp2_hd_inflate_hd_nv (hd_replay.h, the one
// statement of the walk, shared with the host twin below).  A set of decoding
// contexts lives in device memory: per connection a 32-byte header, a ring of
// table_bytes / 32 entry descriptors and two byte stores of table_bytes.  The
// set (its allocation, read-back and change of a table size), the wave's copy
// of byte runs and the commit are hd_devtable.h's, shared with the device
// deflaters; the host's commit and the ring's read-out are hd_replay.h's.
//
// nghttp2_amd_hd_dev_inflate_blocks, one clear of 2 (n + 1) counters and four
// launches behind parse -> gather -> decode:
//   k_replay       one lane per connection, 64 connections per one-wave
//                  workgroup: the lane walks its connection's blocks in order
//                  and leaves one FieldRef per record, the blocks' field
//                  counts, arena bytes and statuses, and the table as the
//                  call leaves it (header, the ring of this call's
//                  insertions) in the workspace.  Serial, dependent loads at
//                  per-lane addresses: a latency, not a bandwidth.  No LDS.
//   k_replay_scan  one workgroup (hd_scan.h): block_nv_off, the blocks' arena
//                  bases, out_totals with the overflow bits.
//   k_emit         a wave per 64 consecutive records: each lane writes its
//                  field's nghttp2_amd_hd_nv, then the wave copies the fields'
//                  name, NUL, value, NUL one after the other with its lanes
//                  on consecutive bytes (k_gather's shape).
//   k_commit       a wave per connection that had blocks: hdtable::commit
//                  over the four stores.
// With an overflow bit in out_totals[2], k_emit and k_commit do nothing: no
// field is written and every table is as before the call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_devtable.h"
#include "hd_host.h"
#include "hd_replay.h"
#include "hd_scan.h"

struct nghttp2_amd_hd_dev_inflaters : hdtable::Set {};  // (key stays null)

namespace {

using hdreplay::Conn;
using hdreplay::Entry;
using hdreplay::FieldRef;
using hdreplay::Ref;
using hdscan::SC_WG;
using hdtable::Left;

constexpr uint32_t RP_WG = 64;   // k_replay, k_init: one wave, 64 connections
constexpr uint32_t EM_WG = 256;  // k_emit: four waves, 64 records each
constexpr uint32_t CM_WG = 64;   // k_commit: one wave, one connection

__constant__ hdhost::StaticPool d_static = hdhost::kStaticPool;

// The workspace: blk_count[n + 1], blk_bytes[n + 1] (cleared by the call),
// left[nconn], fresh[nconn][slots], fref[ops_cap].
struct Ws {
  uint32_t *blk_count, *blk_bytes;
  Left *left;
  Entry *fresh;
  FieldRef *fref;
  size_t clear_bytes, total;
};
__host__ Ws ws_layout(void *base, uint32_t nconn, uint32_t table_bytes, size_t ops_cap, uint32_t n) {
  Ws w;
  hdhost::Carve c{base};
  w.blk_count = c.take<uint32_t>((size_t)n + 1u, 4);  // (the two counter arrays are one span: one clear)
  w.blk_bytes = c.take<uint32_t>((size_t)n + 1u, 4);
  w.clear_bytes = c.at;
  w.left = c.take<Left>(nconn);
  w.fresh = c.take<Entry>((size_t)nconn * (table_bytes / hdreplay::kOverhead));
  w.fref = c.take<FieldRef>(ops_cap);
  w.total = c.total();
  return w;
}

struct FrefStore {
  FieldRef *fref;
  uint32_t base, cap;
  __device__ void operator()(uint32_t k, const FieldRef &fr) const {
    const uint32_t idx = base + k;
    if (idx >= base && idx < cap) fref[idx] = fr;
  }
};

__global__ __launch_bounds__(RP_WG) void k_init(Conn *__restrict__ hdr, uint32_t nconn) {
  const uint32_t c = blockIdx.x * RP_WG + threadIdx.x;
  if (c >= nconn) return;
  Conn h;
  hdreplay::conn_init(&h);
  hdr[c] = h;
}

struct ChangeSize {  // hdtable::k_change_size's rule
  __device__ int operator()(Conn *h, const Entry *ring, uint32_t table_bytes, uint32_t v) const {
    return hdreplay::change_table_size(h, ring, table_bytes, v);
  }
};

__global__ __launch_bounds__(RP_WG) void k_replay(
    const Conn *__restrict__ hdr, const Entry *__restrict__ ring, uint32_t nconn, uint32_t table_bytes,
    const uint8_t *__restrict__ wire, uint64_t wire_bytes, const uint32_t *__restrict__ block_off, uint32_t n,
    const uint32_t *__restrict__ op_off, const nghttp2_amd_hd_op *__restrict__ ops, uint32_t ops_cap,
    const int32_t *__restrict__ block_status, const uint32_t *__restrict__ totals,
    const uint32_t *__restrict__ dst_off, const int32_t *__restrict__ status, uint32_t nlits,
    const uint32_t *__restrict__ conn_blk_off, const uint32_t *__restrict__ conn_blk, int32_t *__restrict__ out_status,
    uint32_t *__restrict__ blk_count, uint32_t *__restrict__ blk_bytes, Left *__restrict__ left,
    Entry *__restrict__ fresh, FieldRef *__restrict__ fref) {
  const uint32_t c = blockIdx.x * RP_WG + threadIdx.x;
  if (c >= nconn) return;
  const uint32_t b0 = conn_blk_off[c], b1 = min(conn_blk_off[c + 1], n);
  if (b0 >= b1) {  // a connection without blocks
    left[c].walked = 0u;
    return;
  }
  if (totals[3]) return;  // the parse's results are not complete
  const uint32_t nops = min(totals[0], ops_cap);
  const uint32_t slots = table_bytes / hdreplay::kOverhead;
  const Conn h0 = hdr[c];
  hdreplay::Table t;
  hdreplay::table_open(&t, h0, ring + (size_t)c * slots, fresh + (size_t)c * slots, table_bytes,
                       (2u * c + (h0.cur & 1u)) * table_bytes);
  const hdreplay::Lits lits = {dst_off, status, min(totals[1], nlits)};  // (never past the decode's arrays)
  for (uint32_t j = b0; j < b1; ++j) {
    const uint32_t b = conn_blk[j];
    if (b >= n) continue;
    const uint32_t r0 = min(op_off[b], nops), r1 = min(op_off[b + 1], nops);
    const uint32_t w0 = block_off[b], w1 = block_off[b + 1];
    const bool first_is_size = hdreplay::block_first_is_size(wire, wire_bytes, w0, w1);
    const hdreplay::BlockResult r =
        hdreplay::walk_block(&t, b, ops + r0, r1 > r0 ? r1 - r0 : 0u, block_status[b] >= 0, first_is_size, lits,
                             &d_static, FrefStore{fref, r0, ops_cap});
    out_status[b] = r.status;
    blk_count[b] = r.fields;
    blk_bytes[b] = r.bytes;
  }
  left[c] = Left{t.h, t.nnew, t.nhead, t.nold, 1u, {0u, 0u, 0u, 0u}};
}

__global__ __launch_bounds__(SC_WG) void k_replay_scan(const uint32_t *__restrict__ totals,
                                                       const uint32_t *blk_count, uint32_t *blk_bytes, uint32_t n,
                                                       uint32_t nva_cap, uint32_t arena_cap,
                                                       uint32_t *block_nv_off, uint32_t *__restrict__ out_totals) {
  __shared__ uint64_t wsum[2][SC_WG / 64];
  if (totals[3]) return;
  hdscan::Share s0, s1;
  const uint64_t t0 = hdscan::scan_sums(blk_count, n, wsum[0], &s0);
  const uint64_t t1 = hdscan::scan_sums(blk_bytes, n, wsum[1], &s1);
  if (!hdreplay::totals_wide(t0, t1)) {
    hdscan::scan_write(blk_count, block_nv_off, n, s0, t0);
    hdscan::scan_write(blk_bytes, blk_bytes, n, s1, t1);
  }
  if (threadIdx.x == 0) hdreplay::write_totals(t0, t1, nva_cap, arena_cap, out_totals);
}

// The four stores a Ref can name, with their sizes: a Ref that reaches past
// its store is not read (hdtable::wave_copy's and hdtable::commit's policy).
struct Stores {
  const uint8_t *base[4];
  uint64_t bytes[4];
  __device__ bool ok(Ref r) const {
    const uint32_t src = hdreplay::ref_src(r);  // (selected, not indexed: the struct stays in registers)
    const uint64_t lim = src == hdreplay::SRC_STATIC ? bytes[0]
                         : src == hdreplay::SRC_WIRE ? bytes[1]
                         : src == hdreplay::SRC_POOL ? bytes[2]
                         : src == hdreplay::SRC_TABLE ? bytes[3]
                                                      : 0u;
    return (uint64_t)r.off + hdreplay::ref_len(r) <= lim;
  }
  __device__ const uint8_t *ptr(uint32_t off, uint32_t ls) const {
    const uint32_t src = ls >> 24;
    return (src == hdreplay::SRC_STATIC ? base[0]
            : src == hdreplay::SRC_WIRE ? base[1]
            : src == hdreplay::SRC_POOL ? base[2]
                                        : base[3]) + off;
  }
  __device__ uint32_t len(uint32_t ls) const { return ls & 0xFFFFFFu; }
  __device__ bool readable(uint32_t, uint32_t) const { return true; }  // (a Ref that is ok)
};

__global__ __launch_bounds__(EM_WG) void k_emit(Stores stores, const uint32_t *__restrict__ totals,
                                                const uint32_t *__restrict__ op_off, uint32_t n, uint32_t ops_cap,
                                                const FieldRef *__restrict__ fref,
                                                const uint32_t *__restrict__ block_nv_off,
                                                const uint32_t *__restrict__ arena_base,
                                                const uint32_t *__restrict__ out_totals,
                                                nghttp2_amd_hd_nv *__restrict__ nva, uint32_t nva_cap,
                                                uint8_t *__restrict__ arena, uint32_t arena_cap) {
  if (totals[3] || out_totals[2]) return;
  stores.base[0] = d_static.bytes;
  const uint32_t nops = min(totals[0], ops_cap);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t0 = (blockIdx.x * (EM_WG / 64u) + (threadIdx.x >> 6)) * 64u;  // the wave's records
  if (t0 >= nops) return;
  const uint32_t r = t0 + lane;
  FieldRef fr = {};
  fr.block = hdreplay::kNoField;
  if (r < nops) fr = fref[r];
  // a field of a block the walk covered: the record lies in its block and the
  // ordinal below the block's count (a block no connection lists counts 0)
  bool has = fr.block < n;
  uint32_t idx = 0, at = 0;
  if (has) {
    const uint32_t f0 = block_nv_off[fr.block], f1 = block_nv_off[fr.block + 1];
    has = r >= op_off[fr.block] && r < op_off[fr.block + 1] && fr.ordinal < f1 - f0 && stores.ok(fr.name) &&
          stores.ok(fr.value);
    idx = f0 + fr.ordinal;
    at = arena_base[fr.block] + fr.before;
    has = has && idx < nva_cap;
  }
  if (has) hdreplay::field_nv(fr, at, &nva[idx]);
  hdtable::wave_copy(stores, has, fr.name, fr.value, (uint64_t)at, arena, (uint64_t)arena_cap, true, lane);
}

__global__ __launch_bounds__(CM_WG) void k_commit(Stores stores, const uint32_t *__restrict__ totals,
                                                  const uint32_t *__restrict__ out_totals,
                                                  const Left *__restrict__ left, const Entry *__restrict__ fresh,
                                                  Conn *__restrict__ hdr, Entry *ring, uint8_t *store,
                                                  uint32_t table_bytes) {
  if (totals[3] || out_totals[2]) return;
  stores.base[0] = d_static.bytes;
  hdtable::commit<false>(stores, blockIdx.x, threadIdx.x, left, fresh, nullptr, hdr, ring, nullptr, store, table_bytes);
}

using hdhost::clamp32;
using hdreplay::table_bytes_ok;

}  // namespace

extern "C" {

int nghttp2_amd_hd_dev_inflaters_new(nghttp2_amd_hd_dev_inflaters **set_ptr, uint32_t nconn, uint32_t table_bytes,
                                     void *stream) {
  if (!hdtable::set_args_ok(set_ptr, nconn, table_bytes)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  nghttp2_amd_hd_dev_inflaters *s = nullptr;
  int rv = hdtable::set_new(&s, nconn, table_bytes, false);
  if (rv) return rv;
  hipLaunchKernelGGL(k_init, dim3((nconn + RP_WG - 1u) / RP_WG), dim3(RP_WG), 0, (hipStream_t)stream, s->hdr, nconn);
  rv = hdhost::hip_rv(hipGetLastError());
  if (rv) {
    hdtable::set_del(s);
    return rv;
  }
  *set_ptr = s;
  return 0;
}

void nghttp2_amd_hd_dev_inflaters_del(nghttp2_amd_hd_dev_inflaters *set) { hdtable::set_del(set); }

int nghttp2_amd_hd_dev_inflaters_change_table_size(nghttp2_amd_hd_dev_inflaters *set, const uint32_t *conn,
                                                   const uint32_t *value, int32_t *rv, uint32_t n, void *stream) {
  return hdtable::set_change_size<ChangeSize>(set, conn, value, rv, n, stream);
}

int nghttp2_amd_hd_dev_inflaters_read(nghttp2_amd_hd_dev_inflaters *set, uint32_t conn, nghttp2_amd_hd_dev_conn *hdr,
                                      uint32_t *entries, uint8_t *bytes, void *stream) {
  return hdtable::set_read(set, conn, hdr, entries, bytes, stream);
}

size_t nghttp2_amd_hd_dev_inflate_workspace_size(uint32_t nconn, uint32_t table_bytes, size_t ops_cap,
                                                 uint32_t nblocks) {
  return ws_layout(nullptr, nconn, table_bytes, ops_cap, nblocks).total;
}

int nghttp2_amd_hd_dev_inflate_blocks(nghttp2_amd_hd_dev_inflaters *set, const uint8_t *wire, size_t wire_bytes,
                                      const uint32_t *block_off, uint32_t nblocks, const uint32_t *op_off,
                                      const nghttp2_amd_hd_op *ops, size_t ops_cap, const int32_t *block_status,
                                      const uint32_t *totals, const uint8_t *dst, size_t dst_bytes,
                                      const uint32_t *dst_off, const int32_t *status, uint32_t nlits,
                                      const uint32_t *conn_blk_off, const uint32_t *conn_blk,
                                      nghttp2_amd_hd_nv *nva, size_t nva_cap, uint8_t *arena, size_t arena_cap,
                                      uint32_t *block_nv_off, int32_t *out_status, uint32_t *out_totals,
                                      void *workspace, size_t ws_bytes, void *stream) {
  const uint32_t n = nblocks;
  if (n == 0) return 0;
  if (!set || !wire || !block_off || !op_off || !ops || !block_status || !totals || !dst || !dst_off || !status ||
      !conn_blk_off || !conn_blk || (!nva && nva_cap) || (!arena && arena_cap) || !block_nv_off || !out_status ||
      !out_totals || !workspace)
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const uint32_t cap = clamp32(ops_cap), nconn = set->nconn, tb = set->table_bytes;
  const Ws w = ws_layout(workspace, nconn, tb, cap, n);
  if (ws_bytes < w.total) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  // (store 0 is the kernels' own constant pool)
  const Stores stores = {{nullptr, wire, dst, set->store},
                         {hdhost::kStaticPoolBytes, wire_bytes, dst_bytes, (uint64_t)nconn * 2u * tb}};
  // (a block no connection lists counts no field and no byte)
  hipError_t e = hipMemsetAsync(w.blk_count, 0, w.clear_bytes, st);
  if (e != hipSuccess) return hdhost::hip_rv(e);
  hipLaunchKernelGGL(k_replay, dim3((nconn + RP_WG - 1u) / RP_WG), dim3(RP_WG), 0, st, (const Conn *)set->hdr,
                     (const Entry *)set->ring, nconn, tb, wire, (uint64_t)wire_bytes, block_off, n, op_off, ops, cap,
                     block_status, totals, dst_off, status, nlits, conn_blk_off, conn_blk, out_status, w.blk_count,
                     w.blk_bytes, w.left, w.fresh, w.fref);
  hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(SC_WG), 0, st, totals, (const uint32_t *)w.blk_count, w.blk_bytes, n,
                     clamp32(nva_cap), clamp32(arena_cap), block_nv_off, out_totals);
  if (cap)
    hipLaunchKernelGGL(k_emit, dim3((cap + EM_WG - 1u) / EM_WG), dim3(EM_WG), 0, st, stores, totals, op_off, n, cap,
                       (const FieldRef *)w.fref, (const uint32_t *)block_nv_off, (const uint32_t *)w.blk_bytes,
                       (const uint32_t *)out_totals, nva, clamp32(nva_cap), arena, clamp32(arena_cap));
  hipLaunchKernelGGL(k_commit, dim3(nconn), dim3(CM_WG), 0, st, stores, totals, (const uint32_t *)out_totals,
                     (const Left *)w.left, (const Entry *)w.fresh, set->hdr, set->ring, set->store, tb);
  return hdhost::hip_rv(hipGetLastError());
}

/* ---- the host twin: the same walk over host arrays, no GPU call ---- */

void nghttp2_amd_hd_replay_host_init(nghttp2_amd_hd_dev_conn *hdr) {
  if (hdr) hdreplay::conn_init(hdr);
}

int nghttp2_amd_hd_replay_host_change_table_size(nghttp2_amd_hd_dev_conn *hdr, const void *ring, uint32_t table_bytes,
                                                 uint32_t value) {
  if (!hdr || !ring || !table_bytes_ok(table_bytes)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  return hdreplay::change_table_size(hdr, (const Entry *)ring, table_bytes, value);
}

int nghttp2_amd_hd_replay_host(nghttp2_amd_hd_dev_conn *hdr, void *ring_, uint8_t *store, uint32_t table_bytes,
                               const uint8_t *wire, size_t wire_bytes, const uint32_t *block_off, uint32_t nblocks,
                               const uint32_t *op_off, const nghttp2_amd_hd_op *ops, const int32_t *block_status,
                               const uint8_t *dst, const uint32_t *dst_off, const int32_t *status, uint32_t nlits,
                               nghttp2_amd_hd_nv *nva, size_t nva_cap, uint8_t *arena, size_t arena_cap,
                               uint32_t *block_nv_off, int32_t *out_status, uint32_t *out_totals) {
  const uint32_t n = nblocks;
  if (n == 0) return 0;
  if (!hdr || !ring_ || !store || !table_bytes_ok(table_bytes) || !wire || !ops || !block_off || !op_off || !block_status ||
      (!nva && nva_cap) || (!arena && arena_cap) || !block_nv_off || !out_status || !out_totals ||
      (nlits && (!dst || !dst_off || !status)) || hdr->count > table_bytes / hdreplay::kOverhead)
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  Entry *ring = (Entry *)ring_;
  const uint32_t slots = table_bytes / hdreplay::kOverhead;
  std::vector<Entry> fresh(slots);
  std::vector<FieldRef> fref(op_off[n] - op_off[0]);
  const uint32_t cur = hdr->cur & 1u;
  hdreplay::Table t;
  hdreplay::table_open(&t, *hdr, ring, fresh.data(), table_bytes, cur * table_bytes);
  const hdreplay::Lits lits = {dst_off, status, nlits};
  uint64_t fields = 0, bytes = 0;
  std::vector<uint64_t> base(n);
  for (uint32_t b = 0; b < n; ++b) {
    const uint32_t w0 = block_off[b], w1 = block_off[b + 1];
    const bool first_is_size = hdreplay::block_first_is_size(wire, wire_bytes, w0, w1);
    FieldRef *out = fref.data() + (op_off[b] - op_off[0]);
    const hdreplay::BlockResult r =
        hdreplay::walk_block(&t, b, ops + op_off[b], op_off[b + 1] - op_off[b], block_status[b] >= 0, first_is_size,
                             lits, &hdhost::kStaticPool, [out](uint32_t k, const FieldRef &fr) { out[k] = fr; });
    out_status[b] = r.status;
    block_nv_off[b] = (uint32_t)fields;
    base[b] = bytes;
    fields += r.fields;
    bytes += r.bytes;
  }
  block_nv_off[n] = (uint32_t)fields;
  hdreplay::write_totals(fields, bytes, nva_cap, arena_cap, out_totals);
  if (out_totals[2]) return 0;  // all or nothing: no field, and the table as it was
  const uint8_t *stores[4] = {hdhost::kStaticPool.bytes, wire, dst, store};
  auto bytes_of = [&](Ref r) { return stores[hdreplay::ref_src(r)] + r.off; };
  for (const FieldRef &fr : fref) {
    if (fr.block == hdreplay::kNoField) continue;
    nghttp2_amd_hd_nv &nv = nva[block_nv_off[fr.block] + fr.ordinal];
    hdreplay::field_nv(fr, (uint32_t)base[fr.block] + fr.before, &nv);
    if (nv.name_len) memcpy(arena + nv.name_off, bytes_of(fr.name), nv.name_len);
    arena[nv.name_off + nv.name_len] = 0;
    if (nv.value_len) memcpy(arena + nv.value_off, bytes_of(fr.value), nv.value_len);
    arena[nv.value_off + nv.value_len] = 0;
  }
  *hdr = hdreplay::commit_host(t, ring, store, table_bytes, bytes_of);
  return 0;
}

}  // extern "C"
