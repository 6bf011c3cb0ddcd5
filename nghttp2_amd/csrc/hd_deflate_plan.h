// hd_deflate_plan.h -- what one header field becomes on the wire, stated once.
//
// The table half of nghttp2_hd_deflate_hd_bufs (lib/nghttp2_hd.c:1469-1505):
// the pending table size updates at a block's head (:1477-1494), and per field
// deflate_nv (:1373-1467) -- the indexing decision (hd_deflate_decide_indexing,
// :1358-1371), the search of the dynamic and the static table (search_hd_table,
// search_static_table, :1201-1249), the insertion with eviction
// (add_hd_table_incremental, :1130-1195) after the search and before the emit,
// and the representation bytes (emit_indexed_block / emit_indname_block /
// emit_newname_block / emit_table_size, :975-1128).  What it leaves per field
// is a plan record: the representation bytes in front of the literals and which
// of name and value are string literals.  Framing the literals (emit_string) is
// nghttp2_amd_hd_emit_strings_batch's.
//
// The table is hd_replay.h's: the ring, Ref, Entry, the `fresh` ring of a
// call's insertions, table_add / table_evict / table_shrink and the commit.
// One more Ref source names the caller's field arena, which does not change
// while a call runs, so the walk moves no bytes here either.  A deflater entry
// also carries the key its search filters on, the FNV-1a hash of its name
// (hdtok::name_hash), in an array parallel to the ring (the same slot index).
// The hash is a filter only: a match is always confirmed on the bytes.
//
// How the dynamic table is searched is each side's own -- the host twin walks
// it entry by entry (search_serial), k_deflate_plan with a wave's lanes on 64
// entries at a time -- with one result: the newest exact match, else the newest
// name match; the first name match when never indexing.
//
// Shared by the host deflater (hd_deflate.cpp: the indexing decision, the token
// constants, the prefix integer), the host twin (nghttp2_amd_hd_deflate_plan_host)
// and the GPU kernels (hd_deflate_dev.hip).  Plain C++17, no HIP.
#ifndef NGHTTP2_AMD_HD_DEFLATE_PLAN_H
#define NGHTTP2_AMD_HD_DEFLATE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_replay.h"
#include "hd_static.h"
#include "hd_tokens.h"

#define HDPLAN_FN HDREPLAY_FN

namespace hdplan {

using hdreplay::Conn;
using hdreplay::Entry;
using hdreplay::Ref;
using hdreplay::Table;
using hdreplay::ref_len;
using hdreplay::ref_src;

constexpr uint32_t kNotify = NGHTTP2_AMD_HD_DEV_NOTIFY;  // notify_table_size_change
constexpr uint32_t SRC_ARENA = 4;                        // the caller's field arena (after hdreplay's four)
constexpr uint32_t kLitName = NGHTTP2_AMD_HD_PLAN_LIT_NAME, kLitValue = NGHTTP2_AMD_HD_PLAN_LIT_VALUE;
constexpr uint32_t kMaxString = 0xFFFFFFu;  // a Ref's length field

enum Mode { WITH_INDEXING, WITHOUT_INDEXING, NEVER_INDEXING };  // nghttp2_hd.h

// the NGHTTP2_TOKEN_* values (lib/nghttp2_hd.h:57-108) the indexing decision names
constexpr int32_t kTokenPath = 3, kTokenAge = 20, kTokenAuthorization = 22, kTokenContentLength = 27,
                  kTokenCookie = 31, kTokenEtag = 33, kTokenIfModifiedSince = 39, kTokenIfNoneMatch = 40,
                  kTokenLocation = 45, kTokenSetCookie = 54;
constexpr int32_t kLastStaticToken = 60;  // NGHTTP2_TOKEN_WWW_AUTHENTICATE

// deflate_nv's indexing mode (lib/nghttp2_hd.c:1373-1400): never index
// authorization, short cookies and fields flagged NO_INDEX; else
// hd_deflate_decide_indexing (:1358-1371).
HDPLAN_FN Mode decide_indexing(int32_t token, uint64_t namelen, uint64_t valuelen, uint32_t flags,
                               uint64_t bufsize_max) {
  if (token == kTokenAuthorization || (token == kTokenCookie && valuelen < 20) || (flags & 1u)) return NEVER_INDEXING;
  if (token == kTokenPath || token == kTokenAge || token == kTokenContentLength || token == kTokenEtag ||
      token == kTokenIfModifiedSince || token == kTokenIfNoneMatch || token == kTokenLocation ||
      token == kTokenSetCookie || namelen + valuelen + hdhost::kEntryOverhead > bufsize_max * 3 / 4)
    return WITHOUT_INDEXING;
  return WITH_INDEXING;
}

// RFC 7541 5.1 prefix integer (encode_length, lib/nghttp2_hd.c:840-863): at
// most 6 bytes for a uint32, byte i in bits [8 i, 8 i + 8) of v.
struct Packed {
  uint64_t v;
  uint32_t n;
};
HDPLAN_FN Packed put_int(uint32_t n, uint32_t prefix, uint32_t first) {
  const uint32_t k = (1u << prefix) - 1u;
  if (n < k) return Packed{first | n, 1u};
  Packed p = {first | k, 1u};
  n -= k;
  for (; n >= 128u; n >>= 7) p.v |= (uint64_t)(0x80u | (n & 0x7Fu)) << (8u * p.n++);
  p.v |= (uint64_t)n << (8u * p.n++);
  return p;
}

// A plan record's first 8 bytes (nghttp2_amd_hd_plan_rec: bytes[6], nbytes, lits).
HDPLAN_FN uint64_t rec_word(Packed p, uint32_t lits) { return p.v | (uint64_t)p.n << 48 | (uint64_t)lits << 56; }

// nghttp2_hd_deflate_new2 (lib/nghttp2_hd.c:721-748): the table starts at
// min(4096, deflate_max), and a smaller maximum is announced by a size update.
// settings_max holds deflate_hd_table_bufsize_max.
HDPLAN_FN void conn_init(Conn *h, uint32_t deflate_max) {
  h->settings_max = deflate_max;
  h->max = deflate_max < hdreplay::kDefaultMax ? deflate_max : hdreplay::kDefaultMax;
  h->min_max = UINT32_MAX;
  h->size = h->count = h->head = h->cur = 0;
  h->flags = deflate_max < hdreplay::kDefaultMax ? kNotify : 0u;
}

// nghttp2_hd_deflate_change_table_size (:1274-1288) on a connection between
// calls (no fresh entries: the ring is the table).
HDPLAN_FN void change_table_size(Conn *h, const Entry *ring, uint32_t table_bytes, uint32_t v) {
  const uint32_t next = v < h->settings_max ? v : h->settings_max;
  h->max = next;
  h->min_max = h->min_max < next ? h->min_max : next;
  h->flags |= kNotify;
  const uint32_t mask = table_bytes / hdreplay::kOverhead - 1u;
  while (h->size > h->max && h->count) {
    h->size -= hdreplay::entry_room(ring[(h->head + h->count - 1u) & mask]);
    --h->count;
  }
}

// The block head (:1477-1494): the pending size updates -- min_max first when
// it is below max, then max -- as the 16 bytes of a nghttp2_amd_hd_plan_head
// (bytes[12], nbytes, 0, 0, 0), in two words.
struct Head {
  uint64_t lo, hi;
};
HDPLAN_FN Head plan_head(Conn *h) {
  Head r = {0u, 0u};
  if (!(h->flags & kNotify)) return r;
  const uint32_t mn = h->min_max;
  h->flags &= ~kNotify;
  h->min_max = UINT32_MAX;
  Packed a = {0u, 0u};
  if (h->max > mn) a = put_int(mn, 5, 0x20);
  const Packed b = put_int(h->max, 5, 0x20);
  r.lo = a.v | (b.v << (8u * a.n));
  r.hi = a.n ? b.v >> (64u - 8u * a.n) : 0u;
  r.hi |= (uint64_t)(a.n + b.n) << 32;
  return r;
}
HDPLAN_FN uint32_t head_bytes(const Head &h) { return (uint32_t)(h.hi >> 32) & 0xFFu; }

// The keys of a connection's entries: parallel to the ring and to `fresh`.
struct Keys {
  const uint32_t *ring;
  uint32_t *fresh;
};
// dynamic entry i's key, 0 the newest (hdreplay::table_get's addressing)
HDPLAN_FN uint32_t key_get(const Table &t, const Keys &k, uint32_t i) {
  if (i < t.nnew) return k.fresh[(t.nhead + i) & t.mask];
  return k.ring[(t.h.head + (i - t.nnew)) & t.mask];
}

// The two byte stores a deflater's Ref can name: the set's table store (a
// SRC_TABLE offset counts from the start of it, as table_get hands it out)
// and the caller's arena.
struct Bytes {
  const uint8_t *store, *arena;
};
HDPLAN_FN const uint8_t *ref_ptr(const Bytes &by, Ref r) {
  return (ref_src(r) == SRC_ARENA ? by.arena : by.store) + r.off;
}

// One field: where its strings lie in the arena, its flags
// (NGHTTP2_NV_FLAG_NO_INDEX = 1), its name's hash and token.
struct Field {
  uint32_t name_off, name_len, value_off, value_len, flags, hash;
  int32_t token;
};

// lookup_token and name_hash, restated from hd_tokens.h and not moved:
// hdtok::lookup_token probes hdtok::kTable by name, which device code cannot
// address (the kernels hold a __constant__ copy, k_name_tokens one in LDS), and
// both hdtok functions are host-only inlines of a header the names kernel's
// translation unit shares, which this change leaves as it is.  These take the
// table by pointer -- the host's hdtok::kTable, or the kernels' constant copy --
// and are what the plan kernel runs for a name the names kernel did not
// examine, and what the host twin runs for every name.  Same probe, same hash
// (tests/test_deflate_plan_host.py holds the twin to the reference's tokens
// through the recorded wire).
HDPLAN_FN int32_t lookup_token_in(const hdtok::Table *tab, const uint8_t *p, uint32_t n, uint32_t h) {
  for (uint32_t slot = h & (hdtok::kSlots - 1u);; slot = (slot + 1u) & (hdtok::kSlots - 1u)) {
    const uint32_t m = tab->meta[slot];
    if (m == 0) return -1;
    if (tab->hash[slot] != h || hdtok::meta_len(m) != n) continue;
    const uint8_t *q = tab->names + hdtok::meta_off(m);
    uint32_t i = 0;
    while (i < n && q[i] == p[i]) ++i;
    if (i == n) return (int32_t)hdtok::meta_token(m);
  }
}
HDPLAN_FN uint32_t name_hash(const uint8_t *p, uint32_t n) {
  uint32_t h = hdtok::kFnvBasis;
  for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * hdtok::kFnvPrime;
  return h;
}

HDPLAN_FN bool bytes_eq(const uint8_t *a, const uint8_t *b, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// What a search of the dynamic table answers: entry idx (0 the newest) has the
// field's name (found), and its value too (exact).
struct Match {
  uint32_t idx;
  bool found, exact;
};
// search_hd_table's walk (:1225-1249), newest first: an exact match wins, else
// the newest name match; name_only stops at the first name match.
HDPLAN_FN Match search_serial(const Table &t, const Keys &k, const Bytes &by, const Field &f, bool name_only) {
  Match m = {0u, false, false};
  for (uint32_t i = 0; i < t.h.count; ++i) {
    if (key_get(t, k, i) != f.hash) continue;
    const Entry e = hdreplay::table_get(t, i);
    if (ref_len(e.name) != f.name_len || !bytes_eq(ref_ptr(by, e.name), by.arena + f.name_off, f.name_len)) continue;
    if (!m.found) {
      m.found = true;
      m.idx = i;
      if (name_only) break;
    }
    if (ref_len(e.value) == f.value_len && bytes_eq(ref_ptr(by, e.value), by.arena + f.value_off, f.value_len)) {
      m.idx = i;
      m.exact = true;
      break;
    }
  }
  return m;
}

// deflate_nv for one field: the first 8 bytes of its plan record.  search(t,
// keys, f, name_only) answers a Match for the dynamic table as it is before
// the field's own insertion; sp is the static table's pool.
template <class Search>
HDPLAN_FN uint64_t plan_field(Table *t, const Keys &k, const Bytes &by, const hdhost::StaticPool *sp, const Field &f,
                              Search &&search) {
  const Mode mode = decide_indexing(f.token, f.name_len, f.value_len, f.flags, t->h.max);
  const bool name_only = mode == NEVER_INDEXING;
  const Match m = search(*t, k, f, name_only);
  bool exact = m.found && m.exact, have = m.found;
  uint32_t idx = hdhost::kStaticLen + m.idx;
  // a static name without a dynamic exact match searches the static table
  // from its token on (search_static_table, :1201-1223)
  if (!exact && f.token >= 0 && f.token <= kLastStaticToken) {
    have = true;
    idx = (uint32_t)f.token;
    if (!name_only) {
      const uint32_t tok = (uint32_t)f.token;
      for (uint32_t s = tok; s < hdhost::kStaticLen; ++s) {
        if (sp->len[s][0] != sp->len[tok][0] ||
            !bytes_eq(sp->bytes + sp->off[s][0], sp->bytes + sp->off[tok][0], sp->len[tok][0]))
          break;  // (the entries of one name lie side by side)
        if (sp->len[s][1] == f.value_len && bytes_eq(sp->bytes + sp->off[s][1], by.arena + f.value_off, f.value_len)) {
          exact = true;
          idx = s;
          break;
        }
      }
    }
  }
  if (exact) return rec_word(put_int(idx + 1u, 7, 0x80), 0u);  // emit_indexed_block (:975-993)
  // the insertion: after the search, before the emit, so an indexed name may
  // name an entry this insertion evicts
  if (mode == WITH_INDEXING) {
    const Entry e = {hdreplay::make_ref(SRC_ARENA, f.name_off, f.name_len),
                     hdreplay::make_ref(SRC_ARENA, f.value_off, f.value_len)};
    (void)hdreplay::table_add(t, e);  // (max <= table_bytes: the store holds what the maximum admits)
    if ((uint64_t)hdreplay::entry_room(e) <= t->h.max && t->nnew) k.fresh[t->nhead] = f.hash;
  }
  const uint32_t first = mode == WITH_INDEXING ? 0x40u : mode == WITHOUT_INDEXING ? 0x00u : 0x10u;
  if (!have) return rec_word(Packed{first, 1u}, kLitName | kLitValue);  // emit_newname_block (:1104-1128)
  return rec_word(put_int(idx + 1u, mode == WITH_INDEXING ? 6 : 4, first), kLitValue);  // emit_indname_block
}

}  // namespace hdplan

#endif  // NGHTTP2_AMD_HD_DEFLATE_PLAN_H
