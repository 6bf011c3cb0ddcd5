// hd_deflate_dev.hip -- device-resident HPACK deflaters: header lists into wire, for gfx950.
//
// Reference: nghttp2_hd_deflate_hd_bufs (hd_deflate_plan.h, the one statement
// of the field step, shared with the host twin below).  A set of encoding
// contexts lives in device memory: per connection a 32-byte header, a ring of
// table_bytes / 32 entry descriptors with a parallel array of keys (the FNV-1a
// hash of each entry's name) and two byte stores of table_bytes -- the
// inflaters' layout plus the keys.  The set, the wave's copy of byte runs and
// the commit are hd_devtable.h's, shared with the device inflaters; the host's
// commit and the ring's read-out are hd_replay.h's.
//
// nghttp2_amd_hd_dev_deflate_blocks, one clear of the plan and the launches:
//   k_name_view     a lane per field slot: the names as a string view of the
//                   arena, for nghttp2_amd_hd_name_tokens_len_batch (hd_names.hip,
//                   unchanged, with the hash).  (k_field_views of hd_fields.hip
//                   reads a replay's out_totals and writes two views the
//                   deflate has no use for; this is its names part, with the
//                   field count read from block_nv_off[n].)
//   k_deflate_plan  a wave per connection: the connection's blocks and their
//                   fields in order -- an insertion changes the table the next
//                   field searches -- and per field the search with the lanes
//                   on 64 table entries at a time, newest first: key and name
//                   length per lane, a ballot, the candidates confirmed from
//                   the lowest lane up with the wave's lanes on consecutive
//                   bytes.  Everything else is wave-uniform (every lane
//                   computes it; lane 0 stores the records).  The call's
//                   insertions go to `fresh` in the workspace: every lane
//                   stores the same descriptor to the same slot, so a lane that
//                   later loads the slot reads what it wrote itself.  No LDS.
//   k_lit_scan      one workgroup (hd_scan.h): two literal slots per field
//                   slot, name and value, an unused one the empty string; their
//                   lengths into the literal pool's offsets.
//   k_lit_gather    a wave per 64 slots copies the literals from the arena into
//                   the pool, its lanes on consecutive bytes (k_emit's shape).
//   nghttp2_amd_hd_emit_strings_batch (hd_huff.hip, unchanged) frames them.
//   k_field_len     a lane per field slot: the record's bytes plus the framed
//                   lengths of its used slots.
//   k_wire_scan     one workgroup: the fields' prefix, the blocks' lengths
//                   (head and fields), out_off, out_status, out_totals.
//   k_place_wire    a lane per block copies its head, a wave per 64 fields the
//                   representation bytes and the framed literals, in wire order.
//   k_commit        a wave per connection that had blocks: hdtable::commit
//                   over the two stores, with the keys of the entries that entered.
// With an overflow bit in out_totals[2], k_place_wire and k_commit do nothing:
// no wire is written and every table is as before the call.
// Every store to global memory is plain C++ (vector stores).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_deflate_plan.h"
#include "hd_devtable.h"
#include "hd_host.h"
#include "hd_scan.h"

struct nghttp2_amd_hd_dev_deflaters : hdtable::Set {};

static_assert(sizeof(nghttp2_amd_hd_plan_rec) == 16 && sizeof(nghttp2_amd_hd_plan_head) == 16,
              "the plan's layouts are part of the ABI");

namespace {

using hdplan::Bytes;
using hdplan::Field;
using hdplan::Keys;
using hdplan::Match;
using hdreplay::Conn;
using hdreplay::Entry;
using hdreplay::Ref;
using hdreplay::Table;
using hdscan::SC_WG;
using hdtable::Left;
using hdtable::Span;

constexpr uint32_t PL_WG = 64;   // k_deflate_plan, k_commit: one wave, one connection
constexpr uint32_t LN_WG = 256;  // the kernels with a lane per field slot
constexpr uint32_t kMaxCap = 0x3FFFFFFFu;  // 2 * nva_cap + 1 literal offsets are uint32 counts
constexpr uint32_t kBitWire = NGHTTP2_AMD_HD_DEV_OVERFLOW_WIRE, kBitPool = NGHTTP2_AMD_HD_DEV_OVERFLOW_POOL,
                   kBitU32 = NGHTTP2_AMD_HD_DEV_OVERFLOW_U32;

__constant__ hdhost::StaticPool d_static = hdhost::kStaticPool;
__constant__ hdtok::Table d_tokens = hdtok::kTable;

// The workspace.  recs, heads and lit_len are one span, cleared by the call: a
// field or block no connection lists has no bytes and no literal.
struct Ws {
  uint4 *recs;        // [cap] nghttp2_amd_hd_plan_rec
  uint4 *heads;       // [n] nghttp2_amd_hd_plan_head
  uint32_t *lit_len;  // [2 cap]
  size_t clear_bytes;
  uint32_t *name_off;  // [cap + 1]
  int32_t *name_len;   // [cap]
  int32_t *tokens;     // [cap]
  uint32_t *hashes;    // [cap]
  Left *left;          // [nconn]
  Entry *fresh;        // [nconn][slots]
  uint32_t *fresh_key; // [nconn][slots]
  uint32_t *lit_off;   // [2 cap + 1]
  uint32_t *wtot;      // [4] {literal pool bytes, bits, 0, 0}
  uint32_t *frm_off;   // [2 cap + 1]
  uint32_t *flen;      // [cap]
  uint32_t *fpre;      // [cap + 1]
  uint32_t *blen;      // [n]
  uint8_t *pool, *frm;
  void *emit_ws;
  size_t pool_bytes, frm_cap, emit_ws_bytes, total;
};
__host__ Ws ws_layout(void *base, uint32_t nconn, uint32_t table_bytes, size_t cap, size_t arena_bytes, uint32_t n) {
  Ws w;
  hdhost::Carve c{base};
  const size_t slots = table_bytes / hdreplay::kOverhead;
  w.recs = c.take<uint4>(cap);
  w.heads = c.take<uint4>(n);
  w.lit_len = c.take<uint32_t>(2 * cap);
  w.clear_bytes = c.at;
  w.name_off = c.take<uint32_t>(cap + 1);
  w.name_len = c.take<int32_t>(cap);
  w.tokens = c.take<int32_t>(cap);
  w.hashes = c.take<uint32_t>(cap);
  w.left = c.take<Left>(nconn);
  w.fresh = c.take<Entry>((size_t)nconn * slots);
  w.fresh_key = c.take<uint32_t>((size_t)nconn * slots);
  w.lit_off = c.take<uint32_t>(2 * cap + 1);
  w.wtot = c.take<uint32_t>(4);
  w.frm_off = c.take<uint32_t>(2 * cap + 1);
  w.flen = c.take<uint32_t>(cap);
  w.fpre = c.take<uint32_t>(cap + 1);
  w.blen = c.take<uint32_t>(n);
  w.pool_bytes = hdhost::round16(arena_bytes) + 32u;  // (the pool rule's slack behind the literals)
  w.pool = c.take<uint8_t>(w.pool_bytes);
  w.frm_cap = nghttp2_amd_hd_emit_strings_bound(arena_bytes, (uint32_t)(2 * cap));
  w.frm = c.take<uint8_t>(w.frm_cap);
  w.emit_ws_bytes = nghttp2_amd_hd_emit_strings_workspace_size(arena_bytes, (uint32_t)(2 * cap));
  w.emit_ws = c.take<uint8_t>(w.emit_ws_bytes);
  w.total = c.total();
  return w;
}

__device__ __forceinline__ uint32_t rec_nbytes(const uint4 &r) { return (r.y >> 16) & 0xFFu; }
__device__ __forceinline__ uint32_t rec_lits(const uint4 &r) { return r.y >> 24; }
__device__ __forceinline__ uint32_t head_nbytes(const uint4 &h) { return h.w & 0xFFu; }
// byte i (< 12) of a record's or a head's bytes
__device__ __forceinline__ uint32_t word_byte(const uint4 &r, uint32_t i) {
  const uint32_t w = i < 4u ? r.x : i < 8u ? r.y : r.z;
  return (w >> (8u * (i & 3u))) & 0xFFu;
}

// The names of the field slots as a string view.  T, the view's end, leaves
// the pool rule's slack inside arena_bytes; a slot at or past the field count
// is a string the names kernel does not examine.
__global__ __launch_bounds__(LN_WG) void k_name_view(const nghttp2_amd_hd_nv *__restrict__ nva, uint32_t cap,
                                                     uint32_t arena_bytes, const uint32_t *__restrict__ block_nv_off,
                                                     uint32_t n, uint32_t *__restrict__ name_off,
                                                     int32_t *__restrict__ name_len) {
  const uint32_t k = blockIdx.x * LN_WG + threadIdx.x;
  if (k > cap) return;
  const uint32_t nf = min(block_nv_off[n], cap);
  const uint32_t T = arena_bytes >= 32u ? (arena_bytes - 16u) & ~15u : 0u;
  uint32_t no = T;
  int32_t nl = -1;
  if (k < nf) {
    no = min(nva[k].name_off, T);
    nl = (int32_t)min(nva[k].name_len, 0x7FFFFFFFu);
  }
  name_off[k] = no;
  if (k < cap) name_len[k] = nl;
}

struct ChangeSize {  // hdtable::k_change_size's rule
  __device__ int operator()(Conn *h, const Entry *ring, uint32_t table_bytes, uint32_t v) const {
    hdplan::change_table_size(h, ring, table_bytes, v);
    return 0;
  }
};

// The two stores a deflater's Ref can name, with their sizes: a Ref that
// reaches past its store is not read (hdtable::wave_copy's and
// hdtable::commit's policy).
struct Stores {
  Bytes by;
  uint64_t store_bytes, arena_bytes;
  __device__ bool ok(Ref r) const {
    const uint32_t src = hdreplay::ref_src(r);
    const uint64_t lim = src == hdplan::SRC_ARENA ? arena_bytes : src == hdreplay::SRC_TABLE ? store_bytes : 0u;
    return (uint64_t)r.off + hdreplay::ref_len(r) <= lim;
  }
  __device__ const uint8_t *ptr(uint32_t off, uint32_t ls) const { return hdplan::ref_ptr(by, Ref{off, ls}); }
  __device__ uint32_t len(uint32_t ls) const { return ls & 0xFFFFFFu; }
  __device__ bool readable(uint32_t, uint32_t) const { return true; }  // (a Ref that is ok)
};

// The dynamic table searched by a wave (hdplan::search_serial's result): 64
// entries per trip, newest first.  A lane takes one entry: key, descriptor,
// name length.  The lowest candidate lane is the newest; a candidate counts
// when the wave, its lanes on consecutive bytes, finds the name equal.
struct WaveSearch {
  Stores s;
  uint32_t lane;
  __device__ bool eq(const uint8_t *a, const uint8_t *b, uint32_t n) const {
    for (uint32_t o = 0; o < n; o += 64u) {
      const uint32_t i = o + lane;
      const bool ne = i < n && a[i] != b[i];
      if (__ballot(ne)) return false;
    }
    return true;
  }
  __device__ Match operator()(const Table &t, const Keys &k, const Field &f, bool name_only) const {
    Match m = {0u, false, false};
    const uint32_t count = t.h.count;
    for (uint32_t i0 = 0; i0 < count; i0 += 64u) {
      const uint32_t i = i0 + lane;
      Entry e = {};
      bool cand = false;
      if (i < count) {
        const uint32_t key = hdplan::key_get(t, k, i);
        e = hdreplay::table_get(t, i);
        cand = key == f.hash && hdreplay::ref_len(e.name) == f.name_len && s.ok(e.name) && s.ok(e.value);
      }
      uint64_t cm = __ballot(cand);
      while (cm) {
        const int l = __builtin_ctzll(cm);
        cm &= cm - 1ull;
        const Ref en = {(uint32_t)__builtin_amdgcn_readlane((int)e.name.off, l),
                        (uint32_t)__builtin_amdgcn_readlane((int)e.name.ls, l)};
        const Ref ev = {(uint32_t)__builtin_amdgcn_readlane((int)e.value.off, l),
                        (uint32_t)__builtin_amdgcn_readlane((int)e.value.ls, l)};
        if (!eq(hdplan::ref_ptr(s.by, en), s.by.arena + f.name_off, f.name_len)) continue;
        if (!m.found) {
          m.found = true;
          m.idx = i0 + (uint32_t)l;
          if (name_only) return m;
        }
        // (an exact match beats an older name match only when it is exact on the bytes)
        if (hdreplay::ref_len(ev) == f.value_len &&
            eq(hdplan::ref_ptr(s.by, ev), s.by.arena + f.value_off, f.value_len)) {
          m.idx = i0 + (uint32_t)l;
          m.exact = true;
          return m;
        }
      }
    }
    return m;
  }
};

__global__ __launch_bounds__(PL_WG) void k_deflate_plan(
    const Conn *__restrict__ hdr, const Entry *__restrict__ ring, const uint32_t *__restrict__ ring_key,
    const uint8_t *__restrict__ store, uint32_t nconn, uint32_t table_bytes,
    const nghttp2_amd_hd_nv *__restrict__ nva, uint32_t cap, const uint8_t *__restrict__ arena, uint32_t arena_bytes,
    const uint32_t *__restrict__ block_nv_off, uint32_t n, const uint32_t *__restrict__ conn_blk_off,
    const uint32_t *__restrict__ conn_blk, const int32_t *__restrict__ tokens, const uint32_t *__restrict__ hashes,
    Left *__restrict__ left, Entry *fresh, uint32_t *fresh_key, uint4 *__restrict__ recs, uint4 *__restrict__ heads,
    uint32_t *__restrict__ lit_len) {
  // `fresh` and `fresh_key` are neither const nor __restrict__, and must stay so: the kernel stores to
  // them and loads them again, every lane its own store.  Because the same pointer is stored to, the
  // compiler issues those loads as vector loads; marked read-only or no-alias they could become scalar
  // loads, which go through a cache the vector stores do not update.
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  const uint32_t b0 = conn_blk_off[c], b1 = min(conn_blk_off[c + 1], n);
  if (b0 >= b1) {  // a connection without blocks
    if (lane == 0u) left[c].walked = 0u;
    return;
  }
  const uint32_t nf = min(block_nv_off[n], cap);
  const uint32_t slots = table_bytes / hdreplay::kOverhead;
  const Conn h0 = hdr[c];
  Table t;
  hdreplay::table_open(&t, h0, ring + (size_t)c * slots, fresh + (size_t)c * slots, table_bytes,
                       (2u * c + (h0.cur & 1u)) * table_bytes);
  const Keys keys = {ring_key + (size_t)c * slots, fresh_key + (size_t)c * slots};
  const WaveSearch search = {{{store, arena}, (uint64_t)nconn * 2u * table_bytes, arena_bytes}, lane};
  for (uint32_t j = b0; j < b1; ++j) {
    const uint32_t b = conn_blk[j];
    if (b >= n) continue;
    const uint32_t f0 = min(block_nv_off[b], nf), f1 = min(block_nv_off[b + 1], nf);
    const hdplan::Head hd = hdplan::plan_head(&t.h);
    if (lane == 0u)
      heads[b] = make_uint4((uint32_t)hd.lo, (uint32_t)(hd.lo >> 32), (uint32_t)hd.hi, (uint32_t)(hd.hi >> 32));
    for (uint32_t k = f0; k < f1; ++k) {
      Field f;
      f.name_off = nva[k].name_off;
      f.name_len = nva[k].name_len;
      f.value_off = nva[k].value_off;
      f.value_len = nva[k].value_len;
      f.flags = nva[k].flags;
      f.token = tokens[k];
      f.hash = hashes[k];
      // a string the arena does not hold is an empty one
      bool own = f.token == NGHTTP2_AMD_TOKEN_INVALID;
      if (f.name_len > hdplan::kMaxString || (uint64_t)f.name_off + f.name_len > arena_bytes) {
        f.name_off = f.name_len = 0u;
        own = true;
      }
      if (f.value_len > hdplan::kMaxString || (uint64_t)f.value_off + f.value_len > arena_bytes)
        f.value_off = f.value_len = 0u;
      if (own) {  // a name the names kernel did not examine
        f.hash = hdplan::name_hash(arena + f.name_off, f.name_len);
        f.token = hdplan::lookup_token_in(&d_tokens, arena + f.name_off, f.name_len, f.hash);
      }
      const uint64_t w = hdplan::plan_field(&t, keys, search.s.by, &d_static, f, search);
      if (lane == 0u) {
        const uint32_t lits = (uint32_t)(w >> 56);
        recs[k] = make_uint4((uint32_t)w, (uint32_t)(w >> 32), b, 0u);
        *reinterpret_cast<uint2 *>(lit_len + 2u * k) = make_uint2(lits & hdplan::kLitName ? f.name_len : 0u,
                                                                  lits & hdplan::kLitValue ? f.value_len : 0u);
      }
    }
  }
  if (lane == 0u) left[c] = Left{t.h, t.nnew, t.nhead, t.nold, 1u, {0u, 0u, 0u, 0u}};
}

// The literal slots' lengths into the pool's offsets.  More bytes than the
// pool holds (strings that overlap) or than uint32: every slot is empty, and
// the bit stops the placement and the commit.
__global__ __launch_bounds__(SC_WG) void k_lit_scan(const uint32_t *lit_len, uint32_t n2, uint32_t pool_cap,
                                                    uint32_t *lit_off, uint32_t *__restrict__ wtot) {
  __shared__ uint64_t wsum[SC_WG / 64];
  hdscan::Share s;
  const uint64_t total = hdscan::scan_sums(lit_len, n2, wsum, &s);
  const bool wide = (total >> 32) != 0, over = total > pool_cap;
  if (!wide && !over) {
    hdscan::scan_write(lit_len, lit_off, n2, s, total);
  } else {
    for (uint32_t i = s.b; i < s.e; ++i) lit_off[i] = 0u;
    if (threadIdx.x == 0) lit_off[n2] = 0u;
  }
  if (threadIdx.x == 0) {
    wtot[0] = wide ? 0xFFFFFFFFu : (uint32_t)total;
    wtot[1] = (wide ? kBitU32 : 0u) | (over ? kBitPool : 0u);
    wtot[2] = wtot[3] = 0u;
  }
}

__global__ __launch_bounds__(LN_WG) void k_lit_gather(const nghttp2_amd_hd_nv *__restrict__ nva, uint32_t cap,
                                                      const uint8_t *__restrict__ arena, uint32_t arena_bytes,
                                                      const uint32_t *__restrict__ lit_off,
                                                      uint8_t *__restrict__ pool, uint64_t pool_cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = (blockIdx.x * (LN_WG / 64u) + (threadIdx.x >> 6)) * 64u + lane;  // the literal slot
  uint32_t off = 0, len = 0, at = 0;
  if (j < 2u * cap) {
    at = lit_off[j];
    len = lit_off[j + 1u] - at;
    if (len) off = j & 1u ? nva[j >> 1].value_off : nva[j >> 1].name_off;
  }
  hdtable::wave_copy(Span{arena, arena_bytes}, len != 0u, Ref{off, len}, (uint64_t)at, pool, pool_cap, lane);
}

__global__ __launch_bounds__(LN_WG) void k_field_len(const uint4 *__restrict__ recs, uint32_t cap,
                                                     const uint32_t *__restrict__ frm_off,
                                                     uint32_t *__restrict__ flen) {
  const uint32_t k = blockIdx.x * LN_WG + threadIdx.x;
  if (k >= cap) return;
  const uint4 r = recs[k];
  const uint32_t a = frm_off[2u * k], b = frm_off[2u * k + 1u], c = frm_off[2u * k + 2u], lits = rec_lits(r);
  flen[k] = rec_nbytes(r) + (lits & hdplan::kLitName ? b - a : 0u) + (lits & hdplan::kLitValue ? c - b : 0u);
}

__global__ __launch_bounds__(SC_WG) void k_wire_scan(const uint32_t *flen, uint32_t cap, const uint4 *__restrict__ heads,
                                                     const uint32_t *__restrict__ block_nv_off, uint32_t n,
                                                     const uint32_t *__restrict__ frm_off,
                                                     const uint32_t *__restrict__ wtot, uint64_t out_cap,
                                                     uint32_t *fpre, uint32_t *blen, uint32_t *out_off,
                                                     int32_t *__restrict__ out_status,
                                                     uint32_t *__restrict__ out_totals) {
  __shared__ uint64_t wsum[2][SC_WG / 64];
  uint32_t bits = wtot[1];
  if (frm_off[2u * cap] == NGHTTP2_AMD_OFF_OVERFLOW) bits |= kBitU32;  // (emit_strings' own mark)
  hdscan::Share s0, s1;
  const uint64_t tf = hdscan::scan_sums(flen, cap, wsum[0], &s0);
  if (tf >> 32) bits |= kBitU32;
  uint64_t W = 0;
  if (!(bits & kBitU32)) {  // (uniform: every thread holds the same bits)
    hdscan::scan_write(flen, fpre, cap, s0, tf);
    __syncthreads();
    const uint32_t nf = min(block_nv_off[n], cap);
    const uint32_t per = n / SC_WG + (n % SC_WG ? 1u : 0u);
    const uint32_t bb = min(threadIdx.x * per, n), be = min(bb + per, n);
    for (uint32_t b = bb; b < be; ++b) {
      const uint32_t f0 = min(block_nv_off[b], nf), f1 = min(block_nv_off[b + 1], nf);
      blen[b] = head_nbytes(heads[b]) + (f1 > f0 ? fpre[f1] - fpre[f0] : 0u);
    }
    __syncthreads();
    W = hdscan::scan_sums(blen, n, wsum[1], &s1);
    if (W >> 32) {
      bits |= kBitU32;
    } else {
      hdscan::scan_write(blen, out_off, n, s1, W);
      for (uint32_t b = bb; b < be; ++b) out_status[b] = (int32_t)blen[b];
      if (W > out_cap) bits |= kBitWire;
    }
  }
  if (threadIdx.x == 0) {
    out_totals[0] = bits & kBitU32 ? 0xFFFFFFFFu : (uint32_t)W;
    out_totals[1] = wtot[0];
    out_totals[2] = bits;
    out_totals[3] = 0u;
  }
}

__global__ __launch_bounds__(LN_WG) void k_place_wire(const uint32_t *__restrict__ out_totals,
                                                      const uint4 *__restrict__ recs, uint32_t cap,
                                                      const uint4 *__restrict__ heads,
                                                      const uint32_t *__restrict__ block_nv_off, uint32_t n,
                                                      const uint32_t *__restrict__ fpre,
                                                      const uint32_t *__restrict__ frm_off,
                                                      const uint8_t *__restrict__ frm, uint64_t frm_cap,
                                                      const uint32_t *__restrict__ out_off, uint8_t *__restrict__ out,
                                                      uint64_t out_cap) {
  if (out_totals[2]) return;
  const uint32_t gid = blockIdx.x * LN_WG + threadIdx.x, lane = threadIdx.x & 63u;
  if (gid < n) {  // the block's head
    const uint4 h = heads[gid];
    const uint64_t at = out_off[gid];
    for (uint32_t i = 0, nb = min(head_nbytes(h), 12u); i < nb; ++i)
      if (at + i < out_cap) out[at + i] = (uint8_t)word_byte(h, i);
  }
  const uint32_t nf = min(block_nv_off[n], cap);
  if (gid - lane >= nf) return;  // (the wave's first field)
  const uint32_t k = gid;
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (k < nf) r = recs[k];
  const uint32_t nb = min(rec_nbytes(r), 6u), lits = rec_lits(r), b = r.z;
  // a field a connection walked: the record names its block, and lies in it
  bool has = k < nf && nb != 0u && b < n;
  uint64_t at = 0;
  uint32_t a = 0, m = 0, e = 0;
  if (has) {
    const uint32_t f0 = block_nv_off[b], f1 = block_nv_off[b + 1];
    has = k >= f0 && k < f1;
    if (has) {
      at = (uint64_t)out_off[b] + head_nbytes(heads[b]) + (fpre[k] - fpre[f0]);
      a = frm_off[2u * k];
      m = frm_off[2u * k + 1u];
      e = frm_off[2u * k + 2u];
      for (uint32_t i = 0; i < nb; ++i)
        if (at + i < out_cap) out[at + i] = (uint8_t)word_byte(r, i);
    }
  }
  const bool ln = has && (lits & hdplan::kLitName), lv = has && (lits & hdplan::kLitValue);
  const uint32_t nlen = ln ? m - a : 0u, vlen = lv ? e - m : 0u;
  const Span framed = {frm, frm_cap};  // (a pass for the names, a pass for the values)
  hdtable::wave_copy(framed, nlen != 0u, Ref{a, nlen}, at + nb, out, out_cap, lane);
  hdtable::wave_copy(framed, vlen != 0u, Ref{m, vlen}, at + nb + nlen, out, out_cap, lane);
}

__global__ __launch_bounds__(PL_WG) void k_commit(Stores s, const uint32_t *__restrict__ out_totals,
                                                  const Left *__restrict__ left, const Entry *__restrict__ fresh,
                                                  const uint32_t *__restrict__ fresh_key, Conn *__restrict__ hdr,
                                                  Entry *ring, uint32_t *__restrict__ ring_key, uint8_t *store,
                                                  uint32_t table_bytes) {
  if (out_totals[2]) return;
  hdtable::commit<true>(s, blockIdx.x, threadIdx.x, left, fresh, fresh_key, hdr, ring, ring_key, store, table_bytes);
}

using hdhost::clamp32;
using hdreplay::table_bytes_ok;

// a string of the arena, or the empty one (the kernel's rule)
void fit_string(uint32_t *off, uint32_t *len, size_t arena_bytes) {
  if (*len > hdplan::kMaxString || (uint64_t)*off + *len > arena_bytes) *off = *len = 0u;
}

}  // namespace

extern "C" {

int nghttp2_amd_hd_dev_deflaters_new(nghttp2_amd_hd_dev_deflaters **set_ptr, uint32_t nconn, uint32_t table_bytes,
                                     const uint32_t *deflate_max, void *stream) {
  if (!hdtable::set_args_ok(set_ptr, nconn, table_bytes)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  std::vector<Conn> init(nconn);
  for (uint32_t c = 0; c < nconn; ++c) {
    const uint32_t dm = deflate_max ? deflate_max[c] : hdreplay::kDefaultMax;
    if (dm > table_bytes) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
    hdplan::conn_init(&init[c], dm);
  }
  nghttp2_amd_hd_dev_deflaters *s = nullptr;
  const int rv = hdtable::set_new(&s, nconn, table_bytes, true);
  if (rv) return rv;
  // (the headers come from host memory that ends with this call: the copy is waited for)
  hipError_t e = hipMemcpyAsync(s->hdr, init.data(), (size_t)nconn * sizeof(Conn), hipMemcpyHostToDevice,
                                (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    hdtable::set_del(s);
    return hdhost::hip_rv(e);
  }
  *set_ptr = s;
  return 0;
}

void nghttp2_amd_hd_dev_deflaters_del(nghttp2_amd_hd_dev_deflaters *set) { hdtable::set_del(set); }

int nghttp2_amd_hd_dev_deflaters_change_table_size(nghttp2_amd_hd_dev_deflaters *set, const uint32_t *conn,
                                                   const uint32_t *value, int32_t *rv, uint32_t n, void *stream) {
  return hdtable::set_change_size<ChangeSize>(set, conn, value, rv, n, stream);
}

int nghttp2_amd_hd_dev_deflaters_read(nghttp2_amd_hd_dev_deflaters *set, uint32_t conn, nghttp2_amd_hd_dev_conn *hdr,
                                      uint32_t *entries, uint8_t *bytes, void *stream) {
  return hdtable::set_read(set, conn, hdr, entries, bytes, stream);
}

size_t nghttp2_amd_hd_dev_deflate_workspace_size(uint32_t nconn, uint32_t table_bytes, size_t nva_cap,
                                                 size_t arena_bytes, uint32_t nblocks) {
  if (nva_cap > kMaxCap) nva_cap = kMaxCap;
  if (arena_bytes > 0xFFFFFFFFu) arena_bytes = 0xFFFFFFFFu;
  return ws_layout(nullptr, nconn, table_bytes, nva_cap, arena_bytes, nblocks).total;
}

int nghttp2_amd_hd_dev_deflate_blocks(nghttp2_amd_hd_dev_deflaters *set, const nghttp2_amd_hd_nv *nva, size_t nva_cap,
                                      const uint8_t *arena, size_t arena_bytes, const uint32_t *block_nv_off,
                                      uint32_t nblocks, const uint32_t *conn_blk_off, const uint32_t *conn_blk,
                                      uint8_t *out, size_t out_cap, uint32_t *out_off, int32_t *out_status,
                                      uint32_t *out_totals, void *workspace, size_t ws_bytes, void *stream) {
  const uint32_t n = nblocks;
  if (n == 0) return 0;
  if (!set || (nva_cap && (!nva || !arena)) || nva_cap > kMaxCap || arena_bytes > 0xFFFFFFFFu ||
      ((uintptr_t)arena & 15u) || !block_nv_off || !conn_blk_off || !conn_blk || (!out && out_cap) || !out_off ||
      !out_status || !out_totals || !workspace || ((uintptr_t)workspace & 15u))
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const uint32_t cap = (uint32_t)nva_cap, ab = (uint32_t)arena_bytes, nconn = set->nconn, tb = set->table_bytes;
  const Ws w = ws_layout(workspace, nconn, tb, cap, ab, n);
  if (ws_bytes < w.total) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const Stores stores = {{set->store, arena}, (uint64_t)nconn * 2u * tb, ab};
  // (a field or block no connection lists has no bytes and no literal)
  hipError_t e = hipMemsetAsync(w.recs, 0, w.clear_bytes, st);
  if (e != hipSuccess) return hdhost::hip_rv(e);
  hipLaunchKernelGGL(k_name_view, dim3(cap / LN_WG + 1u), dim3(LN_WG), 0, st, nva, cap, ab, block_nv_off, n,
                     w.name_off, w.name_len);
  int rv = hdhost::hip_rv(hipGetLastError());
  if (!rv && cap) rv = nghttp2_amd_hd_name_tokens_len_batch(arena, w.name_off, w.name_len, cap, w.tokens, w.hashes, stream);
  if (rv) return rv;
  hipLaunchKernelGGL(k_deflate_plan, dim3(nconn), dim3(PL_WG), 0, st, (const Conn *)set->hdr, (const Entry *)set->ring,
                     (const uint32_t *)set->key, (const uint8_t *)set->store, nconn, tb, nva, cap, arena, ab,
                     block_nv_off, n, conn_blk_off, conn_blk, (const int32_t *)w.tokens, (const uint32_t *)w.hashes,
                     w.left, w.fresh, w.fresh_key, w.recs, w.heads, w.lit_len);
  hipLaunchKernelGGL(k_lit_scan, dim3(1), dim3(SC_WG), 0, st, (const uint32_t *)w.lit_len, 2u * cap, ab, w.lit_off,
                     w.wtot);
  if (cap)
    hipLaunchKernelGGL(k_lit_gather, dim3((2u * cap + LN_WG - 1u) / LN_WG), dim3(LN_WG), 0, st, nva, cap, arena, ab,
                       (const uint32_t *)w.lit_off, w.pool, (uint64_t)w.pool_bytes);
  rv = hdhost::hip_rv(hipGetLastError());
  if (!rv)
    rv = nghttp2_amd_hd_emit_strings_batch(w.pool, w.lit_off, 2u * cap, ab, w.frm, w.frm_cap, w.frm_off, w.emit_ws,
                                           w.emit_ws_bytes, stream);
  if (rv) return rv;
  if (cap)
    hipLaunchKernelGGL(k_field_len, dim3((cap + LN_WG - 1u) / LN_WG), dim3(LN_WG), 0, st, (const uint4 *)w.recs, cap,
                       (const uint32_t *)w.frm_off, w.flen);
  hipLaunchKernelGGL(k_wire_scan, dim3(1), dim3(SC_WG), 0, st, (const uint32_t *)w.flen, cap, (const uint4 *)w.heads,
                     block_nv_off, n, (const uint32_t *)w.frm_off, (const uint32_t *)w.wtot, (uint64_t)out_cap, w.fpre,
                     w.blen, out_off, out_status, out_totals);
  const uint32_t lanes = cap > n ? cap : n;
  hipLaunchKernelGGL(k_place_wire, dim3((lanes + LN_WG - 1u) / LN_WG), dim3(LN_WG), 0, st,
                     (const uint32_t *)out_totals, (const uint4 *)w.recs, cap, (const uint4 *)w.heads, block_nv_off, n,
                     (const uint32_t *)w.fpre, (const uint32_t *)w.frm_off, (const uint8_t *)w.frm,
                     (uint64_t)w.frm_cap, (const uint32_t *)out_off, out, (uint64_t)out_cap);
  hipLaunchKernelGGL(k_commit, dim3(nconn), dim3(PL_WG), 0, st, stores, (const uint32_t *)out_totals,
                     (const Left *)w.left, (const Entry *)w.fresh, (const uint32_t *)w.fresh_key, set->hdr, set->ring,
                     set->key, set->store, tb);
  return hdhost::hip_rv(hipGetLastError());
}

/* ---- the host twin: the same walk over host arrays, no GPU call ---- */

int nghttp2_amd_hd_deflate_plan_host_init(nghttp2_amd_hd_dev_conn *hdr, uint32_t table_bytes, uint32_t deflate_max) {
  if (!hdr || !table_bytes_ok(table_bytes) || deflate_max > table_bytes) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hdplan::conn_init(hdr, deflate_max);
  return 0;
}

int nghttp2_amd_hd_deflate_plan_host_change_table_size(nghttp2_amd_hd_dev_conn *hdr, const void *ring,
                                                       uint32_t table_bytes, uint32_t value) {
  if (!hdr || !ring || !table_bytes_ok(table_bytes)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hdplan::change_table_size(hdr, (const Entry *)ring, table_bytes, value);
  return 0;
}

int nghttp2_amd_hd_deflate_plan_host(nghttp2_amd_hd_dev_conn *hdr, void *ring_, uint32_t *keys, uint8_t *store,
                                     uint32_t table_bytes, const nghttp2_amd_hd_nv *nva, const uint8_t *arena,
                                     size_t arena_bytes, const uint32_t *block_nv_off, uint32_t nblocks,
                                     nghttp2_amd_hd_plan_rec *recs, nghttp2_amd_hd_plan_head *heads) {
  const uint32_t n = nblocks;
  if (n == 0) return 0;
  if (!hdr || !ring_ || !keys || !store || !table_bytes_ok(table_bytes) || !block_nv_off || !heads ||
      arena_bytes > 0xFFFFFFFFu || hdr->count > table_bytes / hdreplay::kOverhead || hdr->max > table_bytes ||
      (block_nv_off[n] && (!nva || !arena || !recs)))
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  Entry *ring = (Entry *)ring_;
  const uint32_t slots = table_bytes / hdreplay::kOverhead;
  std::vector<Entry> fresh(slots);
  std::vector<uint32_t> fresh_key(slots);
  Table t;
  hdreplay::table_open(&t, *hdr, ring, fresh.data(), table_bytes, (hdr->cur & 1u) * table_bytes);
  const Keys k = {keys, fresh_key.data()};
  const Bytes by = {store, arena};
  for (uint32_t b = 0; b < n; ++b) {
    const hdplan::Head hd = hdplan::plan_head(&t.h);
    memcpy(&heads[b], &hd, sizeof hd);
    for (uint32_t i = block_nv_off[b]; i < block_nv_off[b + 1]; ++i) {
      Field f = {nva[i].name_off, nva[i].name_len, nva[i].value_off, nva[i].value_len, nva[i].flags, 0u, 0};
      fit_string(&f.name_off, &f.name_len, arena_bytes);
      fit_string(&f.value_off, &f.value_len, arena_bytes);
      f.hash = hdplan::name_hash(arena + f.name_off, f.name_len);
      f.token = hdplan::lookup_token_in(&hdtok::kTable, arena + f.name_off, f.name_len, f.hash);
      const uint64_t w = hdplan::plan_field(&t, k, by, &hdhost::kStaticPool, f,
                                            [&by](const Table &tt, const Keys &kk, const Field &ff, bool name_only) {
                                              return hdplan::search_serial(tt, kk, by, ff, name_only);
                                            });
      memcpy(&recs[i], &w, sizeof w);
      recs[i].block = b;
      recs[i].reserved = 0u;
    }
  }
  *hdr = hdreplay::commit_host(t, ring, store, table_bytes, [&by](Ref r) { return hdplan::ref_ptr(by, r); }, keys,
                               fresh_key.data());
  return 0;
}

}  // extern "C"
