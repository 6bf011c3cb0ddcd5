// hd_replay.h -- what the representations of a header block mean, stated once.
//
// hd_parse.h cuts a block into nghttp2_amd_hd_op records without any table
// state; this is the other half of nghttp2_hd_inflate_hd_nv
// (lib/nghttp2_hd.c:1919-2281 with in_final, hd_inflate_commit_indexed /
// _newname / _indname :1780-1875, add_hd_table_incremental :1130-1195,
// nghttp2_hd_inflate_change_table_size :1290-1322): index resolution against
// the connection's dynamic table, insertion with eviction, the size update
// rules, the sticky bad state, and the fields emitted up to an error.
//
// The walk moves no bytes.  Every name and value is a Ref -- a source, an
// offset and a length -- into one of four stores that do not change while a
// call runs: the static table's pool, the wire (raw literals), the Huffman
// decode's output pool, and the connection's table store as it was when the
// call began.  A table entry is two Refs; an indexed name inherits the Ref of
// the entry it resolves; eviction drops descriptors.  So an insertion that
// evicts the entry its own name comes from still points at bytes nothing
// overwrites.
//
// The connection's descriptor ring is read, never written: the entries a call
// inserts go to a ring of their own (`fresh`), and because HPACK inserts at
// the front and evicts at the back, the table during the call is
//   fresh[0, nnew)  then  ring[0, nold)      (newest first)
// with nold only ever falling.  The persistent state changes in the commit.
//
// Shared by the host twin (nghttp2_amd_hd_replay_host) and the GPU kernels
// (k_replay, one lane per connection; k_change_size), and with the walk what
// both sides do around it (at the end of this file): a block's first_is_size,
// out_totals, a field's record, the header and descriptors a commit leaves.
// The host's commit and the read-out of a ring close the file; the device's
// commit is hd_devtable.h's.  Plain C++17, no HIP.
#ifndef NGHTTP2_AMD_HD_REPLAY_H
#define NGHTTP2_AMD_HD_REPLAY_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_parse.h"
#include "hd_static.h"

#if defined(__HIPCC__)
#define HDREPLAY_FN __host__ __device__ inline
#else
#define HDREPLAY_FN inline
#endif

namespace hdreplay {

typedef nghttp2_amd_hd_dev_conn Conn;
static_assert(sizeof(Conn) == 32, "the header's layout is part of the ABI");

constexpr uint32_t kExpectSize = NGHTTP2_AMD_HD_DEV_EXPECT_SIZE, kBad = NGHTTP2_AMD_HD_DEV_BAD,
                   kMidBlock = NGHTTP2_AMD_HD_DEV_MID_BLOCK;
constexpr uint32_t kOverhead = hdhost::kEntryOverhead;
constexpr uint32_t kDefaultMax = 4096;  // NGHTTP2_HD_DEFAULT_MAX_BUFFER_SIZE
// a set's table_bytes: a power of two, 4096 or more
inline bool table_bytes_ok(uint32_t tb) { return tb >= 4096u && (tb & (tb - 1u)) == 0u; }

enum : uint32_t { SRC_STATIC = 0, SRC_WIRE = 1, SRC_POOL = 2, SRC_TABLE = 3 };

// `len` bytes at `off` of store `src`; ls = len | src << 24 (a string literal
// is at most 65536 bytes).  A SRC_TABLE offset counts from the start of the
// set's store allocation in a Ref the walk hands out, and from the start of
// the connection's current store buffer in the persistent ring.
struct Ref {
  uint32_t off, ls;
};
HDREPLAY_FN Ref make_ref(uint32_t src, uint32_t off, uint32_t len) { return Ref{off, len | (src << 24)}; }
HDREPLAY_FN uint32_t ref_len(Ref r) { return r.ls & 0xFFFFFFu; }
HDREPLAY_FN uint32_t ref_src(Ref r) { return r.ls >> 24; }

struct Entry {  // 16 bytes: a ring slot
  Ref name, value;
};
HDREPLAY_FN uint32_t entry_room(const Entry &e) { return ref_len(e.name) + ref_len(e.value) + kOverhead; }

// One emitted field, at the index of the record that emitted it.  block ==
// kNoField marks a record that emitted none.
constexpr uint32_t kNoField = 0xFFFFFFFFu;
struct FieldRef {  // 32 bytes
  Ref name, value;
  uint32_t block;    // the block's index in the batch
  uint32_t ordinal;  // the field's ordinal in its block
  uint32_t before;   // arena bytes of the block's fields before it
  uint32_t flags;    // NGHTTP2_NV_FLAG_NO_INDEX or 0
};

HDREPLAY_FN void conn_init(Conn *h) {
  h->max = h->settings_max = kDefaultMax;
  h->min_max = UINT32_MAX;
  h->size = h->count = h->head = h->flags = h->cur = 0;
}

// A connection's table while a call walks its blocks.
struct Table {
  Conn h;               // h.count = nnew + nold; h.head stays the ring's
  const Entry *ring;    // the persistent ring (table_bytes / 32 slots)
  Entry *fresh;         // this call's insertions, as many slots
  uint32_t mask;        // slots - 1
  uint32_t table_bytes; // the store's capacity
  uint32_t store_off;   // where the connection's current store buffer starts
  uint32_t nnew, nhead, nold;
};
HDREPLAY_FN void table_open(Table *t, const Conn &h, const Entry *ring, Entry *fresh, uint32_t table_bytes,
                            uint32_t store_off) {
  t->h = h;
  t->ring = ring;
  t->fresh = fresh;
  t->mask = table_bytes / kOverhead - 1u;
  t->table_bytes = table_bytes;
  t->store_off = store_off;
  t->nnew = t->nhead = 0;
  t->nold = h.count;
}
// dynamic entry i, 0 the newest
HDREPLAY_FN Entry table_get(const Table &t, uint32_t i) {
  if (i < t.nnew) return t.fresh[(t.nhead + i) & t.mask];
  Entry e = t.ring[(t.h.head + (i - t.nnew)) & t.mask];
  e.name.off += t.store_off;
  e.value.off += t.store_off;
  return e;
}
HDREPLAY_FN void table_evict(Table *t) {  // the oldest entry; h.count > 0
  uint32_t room;
  if (t->nold) {
    room = entry_room(t->ring[(t->h.head + t->nold - 1u) & t->mask]);
    --t->nold;
  } else {
    room = entry_room(t->fresh[(t->nhead + t->nnew - 1u) & t->mask]);
    --t->nnew;
  }
  --t->h.count;
  t->h.size -= room;
}
HDREPLAY_FN void table_shrink(Table *t) {
  while (t->h.size > t->h.max && t->h.count) table_evict(t);
}
// add_hd_table_incremental.  False: the HPACK maximum admits the entry and
// the store cannot hold it (the set's capacity rule).
HDREPLAY_FN bool table_add(Table *t, const Entry &e) {
  const uint32_t room = entry_room(e);
  while ((uint64_t)t->h.size + room > t->h.max && t->h.count) table_evict(t);
  if (room > t->h.max) return true;  // larger than the maximum: the table is empty now, nothing enters
  if ((uint64_t)t->h.size + room > t->table_bytes) return false;
  t->nhead = (t->nhead - 1u) & t->mask;
  t->fresh[t->nhead] = e;
  ++t->nnew;
  ++t->h.count;
  t->h.size += room;
  return true;
}

// nghttp2_hd_inflate_change_table_size on a connection between calls (no
// fresh entries: the ring is the table).
HDREPLAY_FN int change_table_size(Conn *h, const Entry *ring, uint32_t table_bytes, uint32_t v) {
  if (h->flags & kMidBlock) return NGHTTP2_AMD_ERR_INVALID_STATE;
  h->settings_max = v;
  if (h->max > v) {
    h->flags |= kExpectSize;
    h->min_max = v;
    h->max = v;
    const uint32_t mask = table_bytes / kOverhead - 1u;
    while (h->size > h->max && h->count) {
      h->size -= entry_room(ring[(h->head + h->count - 1u) & mask]);
      --h->count;
    }
  }
  return 0;
}

// The Huffman decode's results: literal k is dst[dst_off[k], +status[k]) when
// status[k] >= 0, and failed when it is negative.  nlits bounds k.
struct Lits {
  const uint32_t *dst_off;
  const int32_t *status;
  uint32_t nlits;
};
// A record's name (which = 0) or value literal; false when its decode failed.
HDREPLAY_FN bool literal_ref(const nghttp2_amd_hd_op &op, int which, const Lits &lits, Ref *out) {
  const hdparse::Literal l = hdparse::literal(op, which);
  if (!l.huff) {
    *out = make_ref(SRC_WIRE, l.off, l.len);
    return true;
  }
  const uint32_t k = (uint32_t)l.lit;
  if (k >= lits.nlits) return false;
  const int32_t st = lits.status[k];
  if (st < 0 || (uint32_t)st > 0xFFFFFFu) return false;
  *out = make_ref(SRC_POOL, lits.dst_off[k], (uint32_t)st);
  return true;
}

struct BlockResult {
  int32_t status;   // the number of fields, NGHTTP2_AMD_ERR_HEADER_COMP or NGHTTP2_AMD_ERR_NOMEM
  uint32_t fields;  // emitted, an error's included
  uint32_t bytes;   // their arena bytes (name, NUL, value, NUL), saturating
};

// One block's records ops[0, nops) against the table.  parse_ok: the parse's
// status of the block is not an error; first_is_size: the block's first byte
// opens a size update.  sink(k, fr) receives one FieldRef per record k, in
// order: the field the record emitted, or block == kNoField.  sp is the
// static table's pool (host: &hdhost::kStaticPool; device: its constant copy).
template <class Sink>
HDREPLAY_FN BlockResult walk_block(Table *t, uint32_t block, const nghttp2_amd_hd_op *ops, uint32_t nops,
                                   bool parse_ok, bool first_is_size, const Lits &lits,
                                   const hdhost::StaticPool *sp, Sink &&sink) {
  BlockResult r = {0, 0u, 0u};
  FieldRef none = {};
  none.block = kNoField;
  uint32_t k = 0;
  int32_t err = 0;
  if (t->h.flags & kBad) {
    err = NGHTTP2_AMD_ERR_HEADER_COMP;
  } else {
    bool head = true;
    uint64_t bytes = 0;
    for (; k < nops; ++k) {
      const nghttp2_amd_hd_op op = ops[k];
      const bool is_size = op.kind == NGHTTP2_AMD_HD_OP_SIZE;
      if ((t->h.flags & kExpectSize) && !is_size) break;
      if (is_size) {
        const uint32_t bound = t->h.min_max < t->h.settings_max ? t->h.min_max : t->h.settings_max;
        if (!head || op.value > bound) break;
        t->h.min_max = UINT32_MAX;
        t->h.flags &= ~kExpectSize;
        t->h.max = op.value;
        table_shrink(t);
        sink(k, none);
        continue;
      }
      head = false;
      const bool indexed = op.kind == NGHTTP2_AMD_HD_OP_INDEXED;
      const bool new_name = !indexed && (op.flags & NGHTTP2_AMD_HD_OP_NEW_NAME);
      Entry e = {};
      if (!new_name) {
        if (op.value == 0u || op.value > t->h.count + hdhost::kStaticLen) break;
        const uint32_t idx = op.value - 1u;
        if (idx < hdhost::kStaticLen) {
          e.name = make_ref(SRC_STATIC, sp->off[idx][0], sp->len[idx][0]);
          e.value = make_ref(SRC_STATIC, sp->off[idx][1], sp->len[idx][1]);
        } else {
          e = table_get(*t, idx - hdhost::kStaticLen);
        }
      }
      if (!indexed) {
        if (new_name && !literal_ref(op, 0, lits, &e.name)) break;
        if (!literal_ref(op, 1, lits, &e.value)) break;
        if ((op.flags & NGHTTP2_AMD_HD_OP_INDEX_REQUIRED) && !table_add(t, e)) {
          err = NGHTTP2_AMD_ERR_NOMEM;
          break;
        }
      }
      FieldRef fr;
      fr.name = e.name;
      fr.value = e.value;
      fr.block = block;
      fr.ordinal = r.fields;
      fr.before = bytes > UINT32_MAX ? UINT32_MAX : (uint32_t)bytes;
      fr.flags = !indexed && (op.flags & NGHTTP2_AMD_HD_OP_NO_INDEX) ? 1u : 0u;
      sink(k, fr);
      ++r.fields;
      bytes += (uint64_t)ref_len(e.name) + ref_len(e.value) + 2u;
    }
    r.bytes = bytes > UINT32_MAX ? UINT32_MAX : (uint32_t)bytes;
    if (!err && (k < nops || !parse_ok || (t->h.flags & kExpectSize))) err = NGHTTP2_AMD_ERR_HEADER_COMP;
    if (err) {
      // (a missing expected size update leaves the reference in
      // EXPECT_TABLE_SIZE, where a change of the table size is still taken;
      // any other failure leaves it in the middle of the block)
      const bool expect_state = err == NGHTTP2_AMD_ERR_HEADER_COMP && (t->h.flags & kExpectSize) && !first_is_size;
      t->h.flags |= kBad;
      if (!expect_state) t->h.flags |= kMidBlock;
    }
  }
  for (; k < nops; ++k) sink(k, none);
  r.status = err ? err : (int32_t)r.fields;
  return r;
}

// Whether block wire[w0, w1) opens with a size update (walk_block's first_is_size).
HDREPLAY_FN bool block_first_is_size(const uint8_t *wire, uint64_t wire_bytes, uint32_t w0, uint32_t w1) {
  return w0 < w1 && w0 < wire_bytes && hdparse::first_is_size(wire + w0, w1 - w0);
}

// A call's out_totals from its fields and arena bytes: a sum past uint32
// saturates both counts, and any overflow bit means nothing was emitted.
HDREPLAY_FN bool totals_wide(uint64_t fields, uint64_t bytes) { return ((fields | bytes) >> 32) != 0; }
HDREPLAY_FN void write_totals(uint64_t fields, uint64_t bytes, uint64_t nva_cap, uint64_t arena_cap,
                              uint32_t *out_totals) {
  const bool wide = totals_wide(fields, bytes);
  out_totals[0] = wide ? 0xFFFFFFFFu : (uint32_t)fields;
  out_totals[1] = wide ? 0xFFFFFFFFu : (uint32_t)bytes;
  out_totals[2] = (wide ? NGHTTP2_AMD_HD_DEV_OVERFLOW_U32 : 0u) | (fields > nva_cap ? NGHTTP2_AMD_HD_DEV_OVERFLOW_NVA : 0u) |
                  (bytes > arena_cap ? NGHTTP2_AMD_HD_DEV_OVERFLOW_ARENA : 0u);
  out_totals[3] = 0u;
}

// The record of a field whose name, NUL, value, NUL start at arena offset
// `at`, into *out (all 24 bytes: the padding behind flags is written as zero,
// which a record returned by value would not promise).
HDREPLAY_FN void field_nv(const FieldRef &fr, uint32_t at, nghttp2_amd_hd_nv *out) {
  nghttp2_amd_hd_nv nv = {};
  nv.block = fr.block;
  nv.name_off = at;
  nv.name_len = ref_len(fr.name);
  nv.value_off = at + nv.name_len + 1u;
  nv.value_len = ref_len(fr.value);
  nv.flags = (uint8_t)fr.flags;
  *out = nv;
}

// The commit.  The live entries, newest first, go to slots head, head + 1, ...
// of the ring, their bytes back to back into the store's other buffer: the
// header it leaves, and the descriptor of an entry whose nl + vl bytes are at
// `at` of that buffer.
HDREPLAY_FN Conn committed_conn(const Conn &h, uint32_t nnew, uint32_t nold, uint32_t mask) {
  Conn c = h;
  c.head = (h.head - nnew) & mask;
  c.count = nnew + nold;
  c.cur = (h.cur & 1u) ^ 1u;
  return c;
}
HDREPLAY_FN Entry committed_entry(uint32_t at, uint32_t nl, uint32_t vl) {
  return Entry{make_ref(SRC_TABLE, at, nl), make_ref(SRC_TABLE, at + nl, vl)};
}

// The commit on the host, after a walk over t: the live entries' bytes back
// to back into the other buffer of `store` (the connection's two buffers of
// table_bytes), their descriptors into `ring` (the ring t reads: an entry that
// stays keeps its slot, a fresh one goes to a slot no live entry has), and
// with keys the keys of the entries that entered from fresh_key to ring_key.
// bytes_of(Ref) is where a Ref's bytes lie.  Returns the header after.
template <class BytesOf>
inline Conn commit_host(const Table &t, Entry *ring, uint8_t *store, uint32_t table_bytes, BytesOf &&bytes_of,
                        uint32_t *ring_key = nullptr, const uint32_t *fresh_key = nullptr) {
  const Conn after = committed_conn(t.h, t.nnew, t.nold, t.mask);
  uint8_t *to = store + (size_t)after.cur * table_bytes;
  if (ring_key)
    for (uint32_t i = 0; i < t.nnew; ++i) ring_key[(after.head + i) & t.mask] = fresh_key[(t.nhead + i) & t.mask];
  uint32_t at = 0;
  for (uint32_t i = 0; i < after.count; ++i) {
    const Entry e = table_get(t, i);
    const uint32_t nl = ref_len(e.name), vl = ref_len(e.value);
    if (nl) memcpy(to + at, bytes_of(e.name), nl);
    if (vl) memcpy(to + at + nl, bytes_of(e.value), vl);
    ring[(after.head + i) & t.mask] = committed_entry(at, nl, vl);
    at += nl + vl;
  }
  return after;
}

// A ring read out: the live entries, newest first, entry i's name offset,
// name length, value offset, value length into entries[4 i ..].  False, and
// nothing written, for a header that counts more entries than the ring has.
inline bool ring_entries(const Conn &h, const Entry *ring, uint32_t slots, uint32_t *entries) {
  if (h.count > slots) return false;
  for (uint32_t i = 0; i < h.count; ++i) {
    const Entry d = ring[(h.head + i) & (slots - 1u)];
    entries[4 * i + 0] = d.name.off;
    entries[4 * i + 1] = ref_len(d.name);
    entries[4 * i + 2] = d.value.off;
    entries[4 * i + 3] = ref_len(d.value);
  }
  return true;
}

}  // namespace hdreplay

#endif  // NGHTTP2_AMD_HD_REPLAY_H
