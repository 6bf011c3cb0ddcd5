// hd_deflate.cpp -- batched HPACK deflate front-end (the
// deflate side of rows 1 and 3).
//
// Host C++ above the C ABI.  Deflates many header lists (blocks of one or
// many connections) per call; every string literal of the batch is framed by
// ONE GPU call (nghttp2_amd_hd_emit_strings_batch: Huffman-or-raw choice,
// H bit, length prefix, payload) instead of one emit_string per literal:
//   pass 1  per block in order, against its deflater's dynamic table: table
//           size updates, the table search, the indexing decision and the
//           insertion -- the representation bytes, and the literals to frame;
//   GPU     H2D of the literal strings, emit_strings, D2H of the literals;
//   pass 2  the wire of each block: representation bytes and framed literals
//           in order.
// Output equals nghttp2_hd_deflate_hd2 (nghttp2.h:6127) per block:
// nghttp2_hd_deflate_hd_bufs (lib/nghttp2_hd.c:1469-1505), deflate_nv
// (:1373-1467), search_hd_table / search_static_table / hd_map_find
// (:1201-1249, :566-589), hd_deflate_decide_indexing (:1358-1371),
// emit_indexed_block / emit_indname_block / emit_newname_block /
// emit_table_size (:975-1128), add_hd_table_incremental (:1130-1195).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <deque>
#include <unordered_map>
#include <mutex>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/nghttp2_amd_hd.h"
#include "../../include/nghttp2_amd_hd_testing.h"
#include "hd_deflate_plan.h"
#include "hd_host.h"
#include "host_threads.h"

namespace {

using namespace hdhost;  // the static table, hip_ok, DevBuf / PinnedBuf
const char *const kLayer = "deflate";  // (in hip_ok's messages)

// the indexing modes and decision, the token constants and the prefix integer
// are hd_deflate_plan.h's, shared with the device deflaters
using hdplan::Mode;
using hdplan::NEVER_INDEXING;
using hdplan::WITH_INDEXING;
using hdplan::WITHOUT_INDEXING;
using hdplan::kLastStaticToken;

// the name (which = 0) or value (1) of static entry s is these bytes
bool static_is(uint32_t s, int which, const uint8_t *p, size_t len) {
  return kStaticLens.len[s][which] == len && memcmp(kStatic[s][which], p, len) == 0;
}

// lookup_token (lib/nghttp2_hd.c:137) and name_hash (:536-547): one FNV-1a
// pass and a hashed probe (hd_tokens.h), shared with the GPU kernel.
using hdtok::name_hash;
struct Entry {
  std::string name, value;
  uint32_t hash;
};

// RFC 7541 5.1 prefix integer (hdplan::put_int), appended to out
void put_int(std::string &out, uint32_t n, uint32_t prefix, uint8_t first) {
  const hdplan::Packed p = hdplan::put_int(n, prefix, first);
  for (uint32_t i = 0; i < p.n; ++i) out.push_back((char)(uint8_t)(p.v >> (8u * i)));
}

}  // namespace

struct nghttp2_amd_hd_deflater {
  std::deque<Entry> table;  // front = most recent
  // name hash -> insertion sequence numbers of the entries with that hash,
  // oldest first (the reference's hd_map buckets, lib/nghttp2_hd.c:549-611);
  // the entry with sequence q sits at table[next_seq - 1 - q]
  std::unordered_map<uint32_t, std::deque<uint64_t>> by_hash;
  uint64_t next_seq = 0;
  size_t bufsize = 0;
  size_t bufsize_max;                   // ctx.hd_table_bufsize_max
  size_t deflate_max;                   // deflate_hd_table_bufsize_max
  size_t min_max = UINT32_MAX;          // min_hd_table_bufsize_max
  bool notify = false;                  // notify_table_size_change
  bool bad = false;

  void evict_oldest() {
    const Entry &e = table.back();
    bufsize -= e.name.size() + e.value.size() + kEntryOverhead;
    auto it = by_hash.find(e.hash);
    it->second.pop_front();  // the oldest entry is the oldest of its bucket
    if (it->second.empty()) by_hash.erase(it);
    table.pop_back();
  }
  void shrink() {
    while (bufsize > bufsize_max && !table.empty()) evict_oldest();
  }
  void add(const uint8_t *n, size_t nl, const uint8_t *v, size_t vl, uint32_t h) {
    const size_t room = nl + vl + kEntryOverhead;
    while (bufsize + room > bufsize_max && !table.empty()) evict_oldest();
    if (room > bufsize_max) return;
    table.push_front(Entry{std::string((const char *)n, nl), std::string((const char *)v, vl), h});
    by_hash[h].push_back(next_seq++);
    bufsize += room;
  }
};

namespace {

struct Engine {
  std::mutex mu;
  PinnedBuf h_in, h_out, h_off;  // strings in, framed literals out, uint32 offsets of both
  DevBuf d_in, d_out, d_off, d_ws;
  PinnedBuf h_nt;  // name hashes, then tokens
  DevBuf d_nt;
};
// Batches of at least this many field names take their tokens and hashes
// from one k_name_tokens launch (NGHTTP2_AMD_GPU_NAMES_MIN; 0 = always);
// smaller ones from the host lookup, which costs less than a GPU round trip.
std::atomic<uint32_t> g_names_min{[] {
  const char *e = getenv("NGHTTP2_AMD_GPU_NAMES_MIN");
  return e ? (uint32_t)strtoul(e, nullptr, 10) : 2048u;
}()};
Engine &engine() {
  static Engine e;
  return e;
}
// Fault injection for the error paths (tests only, like the reference's
// failmalloc suite, tests/failmalloc_test.c): the next n GPU stages of
// nghttp2_amd_hd_deflate_blocks fail before any HIP call.
std::atomic<int> g_fail_gpu{0};
bool fault_inject_gpu() {
  int k = g_fail_gpu.load();
  while (k > 0)
    if (g_fail_gpu.compare_exchange_weak(k, k - 1)) return true;
  return false;
}

// One piece of a block's wire: representation bytes, then up to two
// literals (indices into the batch's literal list, -1 = none).
struct Piece {
  std::string bytes;
  int32_t lit[2] = {-1, -1};
};
using Lits = std::vector<std::pair<const uint8_t *, uint32_t>>;  // a block's literals: bytes, length

// Pass 1's result: per block its pieces and the literals to frame; block i's
// literals are the batch's litbase[i] + j, their bytes from rawbase[i] in the pool.
struct Batch {
  std::vector<std::vector<Piece>> pieces;
  std::vector<Lits> lits;
  std::vector<uint32_t> litbase;
  std::vector<uint64_t> rawbase;
};
// The framed literals (pass 2's input): literal g is bytes[off[g] .. off[g + 1]).
struct Framed {
  const uint8_t *bytes = nullptr;
  const uint32_t *off = nullptr;
};

// ---- the phases of nghttp2_amd_hd_deflate_blocks, each named after the trace mark that closes it
using nghttp2_amd_host::parallel_for;

// "names": the token and hash of every field name of the batch (lookup_token,
// name_hash; deflate_nv, lib/nghttp2_hd.c:1388-1393) from one GPU launch over
// the batch's names, before any deflater changes (a failure here leaves them
// as they were).  fnt: hash[nf], then token[nf].  Holds the engine's lock.
int stage_name_tokens(const nghttp2_amd_nv *names, uint32_t nf, void *stream, std::vector<uint32_t> *fnt) {
  std::vector<uint64_t> nbase(nf + 1, 0);
  for (uint32_t k = 0; k < nf; ++k) nbase[k + 1] = nbase[k] + names[k].namelen;
  const uint64_t nraw = nbase[nf];
  if (nraw > UINT32_MAX) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const size_t in_bytes = ((size_t)nraw + 15u) / 16u * 16u + 16u;
  const size_t off_bytes = ((size_t)nf + 1u) * sizeof(uint32_t), nt_bytes = 2u * (size_t)nf * sizeof(uint32_t);
  std::lock_guard<std::mutex> guard(engine().mu);
  Engine &E = engine();
  hipStream_t st = (hipStream_t)stream;
  if (!E.h_in.reserve(in_bytes, kLayer, false) || !E.h_off.reserve(off_bytes, kLayer, false) ||
      !E.h_nt.reserve(nt_bytes, kLayer, false) || !E.d_in.reserve(in_bytes, kLayer) ||
      !E.d_off.reserve(off_bytes, kLayer) || !E.d_nt.reserve(nt_bytes, kLayer))
    return NGHTTP2_AMD_ERR_NOMEM;
  uint8_t *const h_in = E.h_in.as<uint8_t>();
  uint32_t *const h_off = E.h_off.as<uint32_t>(), *const h_nt = E.h_nt.as<uint32_t>();
  parallel_for(nf, 4096, [&](size_t k) {
    h_off[k] = (uint32_t)nbase[k];
    if (names[k].namelen) memcpy(h_in + nbase[k], names[k].name, names[k].namelen);
  });
  h_off[nf] = (uint32_t)nraw;
  memset(h_in + nraw, 0, in_bytes - nraw);
  if (fault_inject_gpu() ||
      !hip_ok(hipMemcpyAsync(E.d_in.p, h_in, in_bytes, hipMemcpyHostToDevice, st), kLayer, "H2D") ||
      !hip_ok(hipMemcpyAsync(E.d_off.p, h_off, off_bytes, hipMemcpyHostToDevice, st), kLayer, "H2D"))
    return NGHTTP2_AMD_ERR_FATAL;
  uint32_t *const d_nt = E.d_nt.as<uint32_t>();
  const int rv = nghttp2_amd_hd_name_tokens_batch(E.d_in.as<uint8_t>(), E.d_off.as<uint32_t>(), nf,
                                                  (int32_t *)(d_nt + nf), d_nt, stream);
  if (rv) return rv;
  if (!hip_ok(hipMemcpyAsync(h_nt, d_nt, nt_bytes, hipMemcpyDeviceToHost, st), kLayer, "D2H") ||
      !hip_ok(hipStreamSynchronize(st), kLayer, "sync"))
    return NGHTTP2_AMD_ERR_FATAL;
  fnt->assign(h_nt, h_nt + 2u * (size_t)nf);
  return 0;
}

// deflate_nv's indexing mode (hdplan::decide_indexing)
Mode decide_indexing(int32_t token, const nghttp2_amd_nv &nv, size_t bufsize_max) {
  return hdplan::decide_indexing(token, nv.namelen, nv.valuelen, nv.flags, bufsize_max);
}

// search_hd_table (lib/nghttp2_hd.c:1225-1249): the dynamic table newest
// first (an exact match, else the newest name match; name only when never
// indexing); a static name without a dynamic exact match searches the static
// table instead (search_static_table, :1201-1223).  The 0-based index of the
// match, or -1; *exact: name and value both match.
int64_t search_tables(const nghttp2_amd_hd_deflater *d, const nghttp2_amd_nv &nv, uint32_t nh, int32_t token,
                      bool name_only, bool *exact) {
  int64_t idx = -1;
  *exact = false;
  auto bucket = d->by_hash.find(nh);
  if (bucket != d->by_hash.end()) {
    const std::deque<uint64_t> &seqs = bucket->second;
    for (size_t r = seqs.size(); r-- > 0;) {  // newest first
      const size_t t = (size_t)(d->next_seq - 1u - seqs[r]);
      const Entry &e = d->table[t];
      if (e.name.size() != nv.namelen || memcmp(e.name.data(), nv.name, nv.namelen) != 0) continue;
      if (idx < 0) {
        idx = (int64_t)(kStaticLen + t);
        if (name_only) break;
      }
      if (e.value.size() == nv.valuelen && memcmp(e.value.data(), nv.value, nv.valuelen) == 0) {
        *exact = true;
        return (int64_t)(kStaticLen + t);
      }
    }
  }
  if (token < 0 || token > kLastStaticToken) return idx;
  if (!name_only)
    for (uint32_t s = (uint32_t)token; s < kStaticLen && static_is(s, 0, nv.name, nv.namelen); ++s)
      if (static_is(s, 1, nv.value, nv.valuelen)) {
        *exact = true;
        return s;
      }
  return token;
}

// deflate_nv (lib/nghttp2_hd.c:1373-1467) for one field with name hash nh and
// token: its piece appended to P, its literals to L, the deflater's table
// updated (add_hd_table_incremental).
void deflate_nv(nghttp2_amd_hd_deflater *d, const nghttp2_amd_nv &nv, uint32_t nh, int32_t token,
                std::vector<Piece> &P, Lits &L) {
  auto lit = [&L](const uint8_t *p, size_t len) {
    L.emplace_back(p, (uint32_t)len);
    return (int32_t)L.size() - 1;
  };
  const Mode mode = decide_indexing(token, nv, d->bufsize_max);
  bool exact;
  const int64_t idx = search_tables(d, nv, nh, token, mode == NEVER_INDEXING, &exact);
  Piece pc;
  if (exact) {  // emit_indexed_block (:975-993)
    put_int(pc.bytes, (uint32_t)idx + 1u, 7, 0x80);
    P.push_back(pc);
    return;
  }
  if (mode == WITH_INDEXING) d->add(nv.name, nv.namelen, nv.value, nv.valuelen, nh);
  const uint8_t first = mode == WITH_INDEXING ? 0x40 : mode == WITHOUT_INDEXING ? 0x00 : 0x10;
  if (idx < 0) {  // emit_newname_block (:1104-1128)
    pc.bytes.push_back((char)first);
    pc.lit[0] = lit(nv.name, nv.namelen);
  } else {  // emit_indname_block (:1062-1102)
    put_int(pc.bytes, (uint32_t)idx + 1u, mode == WITH_INDEXING ? 6 : 4, first);
  }
  pc.lit[1] = lit(nv.value, nv.valuelen);
  P.push_back(pc);
}

// nghttp2_hd_deflate_hd_bufs (lib/nghttp2_hd.c:1469-1505) for block i, its
// fields nva[0 .. n): the pending table size updates, then each field.  fnt:
// the fields' hashes and tokens from stage_name_tokens (fnt[k] and
// fnt[fnt_tok + k]), or null for the host lookup.
int32_t deflate_block(nghttp2_amd_hd_deflater *d, const nghttp2_amd_nv *nva, uint32_t n, const uint32_t *fnt,
                      uint32_t fnt_tok, std::vector<Piece> &P, Lits &L) {
  if (d->bad) return NGHTTP2_AMD_ERR_HEADER_COMP;
  if (d->notify) {  // :1477-1494
    const size_t mn = d->min_max;
    d->notify = false;
    d->min_max = UINT32_MAX;
    Piece pc;
    if (d->bufsize_max > mn) put_int(pc.bytes, (uint32_t)mn, 5, 0x20);
    put_int(pc.bytes, (uint32_t)d->bufsize_max, 5, 0x20);
    P.push_back(pc);
  }
  for (uint32_t k = 0; k < n; ++k) {
    const nghttp2_amd_nv &nv = nva[k];
    const uint32_t nh = fnt ? fnt[k] : name_hash(nv.name, nv.namelen);
    const int32_t token = fnt ? (int32_t)fnt[fnt_tok + k] : hdtok::lookup_token(nv.name, nv.namelen, nh);
    deflate_nv(d, nv, nh, token, P, L);
  }
  return 0;
}

// "tables" -- pass 1: every block's representations against its deflater's
// table; one task per connection, its lists in batch order (connections are
// independent).  Then the batch's literal numbering.
void deflate_tables(nghttp2_amd_hd_deflater *const *deflaters, uint32_t nblocks, const nghttp2_amd_nv *nva,
                    const uint32_t *block_nv_off, const std::vector<uint32_t> &fnt, int32_t *block_status,
                    Batch *B) {
  B->pieces.resize(nblocks);
  B->lits.resize(nblocks);
  const uint32_t f0 = block_nv_off[0], nf = block_nv_off[nblocks] - f0;
  // the batch's lists per connection, in batch order; the parallel region
  // only reads `lists` (a vector indexed by connection number)
  std::unordered_map<nghttp2_amd_hd_deflater *, uint32_t> conn_of;
  std::vector<std::vector<uint32_t>> lists;
  for (uint32_t i = 0; i < nblocks; ++i) {
    auto it = conn_of.emplace(deflaters[i], (uint32_t)lists.size()).first;
    if (it->second == lists.size()) lists.emplace_back();
    lists[it->second].push_back(i);
  }
  parallel_for(lists.size(), 1, [&](size_t c) {
    for (uint32_t i : lists[c]) {
      const uint32_t a = block_nv_off[i];
      block_status[i] = deflate_block(deflaters[i], nva + a, block_nv_off[i + 1] - a,
                                      fnt.empty() ? nullptr : fnt.data() + (a - f0), nf, B->pieces[i], B->lits[i]);
    }
  });
  B->litbase.assign(nblocks + 1, 0);
  B->rawbase.assign(nblocks + 1, 0);
  for (uint32_t i = 0; i < nblocks; ++i) {
    uint64_t r = 0;
    for (auto &l : B->lits[i]) r += l.second;
    B->litbase[i + 1] = B->litbase[i] + (uint32_t)B->lits[i].size();
    B->rawbase[i + 1] = B->rawbase[i] + r;
  }
}

// "gpu": every literal of the batch framed in one launch (emit_string): H2D
// of the literal pool and its offsets, emit_strings, D2H of the framed
// offsets and then of the framed bytes they total.  Called with the engine's
// lock held; *fr points into the engine's pinned pools.
int frame_literals(Engine &E, uint32_t nblocks, const Batch &B, void *stream, Framed *fr) {
  const uint32_t nl = B.litbase[nblocks];
  if (!nl) return 0;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t raw = B.rawbase[nblocks];
  // uint32 offsets: the framed literals (raw + <= 6 prefix bytes each)
  if (nghttp2_amd_hd_emit_strings_bound(raw, nl) > UINT32_MAX) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const size_t in_bytes = ((size_t)raw + 15u) / 16u * 16u + 16u;
  const size_t out_bytes = nghttp2_amd_hd_emit_strings_bound(raw, nl);
  const size_t ws = nghttp2_amd_hd_emit_strings_workspace_size(raw, nl);
  const size_t slots = (size_t)nl + 1u, off_bytes = 2u * slots * sizeof(uint32_t);  // raw, then framed
  if (!E.h_in.reserve(in_bytes, kLayer, false) || !E.h_out.reserve(out_bytes, kLayer, false) ||
      !E.h_off.reserve(off_bytes, kLayer, false) || !E.d_in.reserve(in_bytes, kLayer) ||
      !E.d_out.reserve(out_bytes, kLayer) || !E.d_ws.reserve(ws, kLayer) || !E.d_off.reserve(off_bytes, kLayer))
    return NGHTTP2_AMD_ERR_NOMEM;
  uint8_t *const h_in = E.h_in.as<uint8_t>();
  uint32_t *const h_off = E.h_off.as<uint32_t>(), *const d_off = E.d_off.as<uint32_t>();
  // the literal pool and its offsets, block by block
  parallel_for(nblocks, 256, [&](size_t i) {
    uint32_t o = (uint32_t)B.rawbase[i];
    uint32_t k = B.litbase[i];
    for (auto &l : B.lits[i]) {
      h_off[k++] = o;
      if (l.second) memcpy(h_in + o, l.first, l.second);
      o += l.second;
    }
  });
  h_off[nl] = (uint32_t)raw;
  memset(h_in + raw, 0, in_bytes - raw);
  uint32_t *d_fo = d_off + slots, *h_fo = h_off + slots;
  if (fault_inject_gpu() ||
      !hip_ok(hipMemcpyAsync(E.d_in.p, h_in, in_bytes, hipMemcpyHostToDevice, st), kLayer, "H2D") ||
      !hip_ok(hipMemcpyAsync(d_off, h_off, slots * sizeof(uint32_t), hipMemcpyHostToDevice, st), kLayer, "H2D"))
    return NGHTTP2_AMD_ERR_FATAL;
  const int rv = nghttp2_amd_hd_emit_strings_batch(E.d_in.as<uint8_t>(), d_off, nl, raw, E.d_out.as<uint8_t>(),
                                                   out_bytes, d_fo, E.d_ws.p, ws, stream);
  if (rv) return rv;
  if (!hip_ok(hipMemcpyAsync(h_fo, d_fo, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, st), kLayer, "D2H") ||
      !hip_ok(hipStreamSynchronize(st), kLayer, "sync"))
    return NGHTTP2_AMD_ERR_FATAL;
  if (!hip_ok(hipMemcpyAsync(E.h_out.p, E.d_out.p, h_fo[nl], hipMemcpyDeviceToHost, st), kLayer, "D2H") ||
      !hip_ok(hipStreamSynchronize(st), kLayer, "sync"))
    return NGHTTP2_AMD_ERR_FATAL;
  *fr = Framed{E.h_out.as<uint8_t>(), h_fo};
  return 0;
}

// Block i's wire in order, as runs of bytes: f(ptr, len) for each piece's
// representation bytes and then each of its framed literals.
template <class F>
void for_each_run(const Batch &B, size_t i, const Framed &fr, F &&f) {
  for (const Piece &pc : B.pieces[i]) {
    f((const uint8_t *)pc.bytes.data(), pc.bytes.size());
    for (int j = 0; j < 2; ++j) {
      if (pc.lit[j] < 0) continue;
      const uint32_t g = B.litbase[i] + (uint32_t)pc.lit[j];
      f(fr.bytes + fr.off[g], (size_t)(fr.off[g + 1] - fr.off[g]));
    }
  }
}

// "wire" -- pass 2: each block's wire size, placement in block order, then
// the bytes.  Returns 0, or BUFFER_ERROR when a block did not fit.
// *stop_piece (a single-block call's, or null): the piece of a block that did
// not fit at which the room ran out.
int place_wire(nghttp2_amd_hd_deflater *const *deflaters, uint32_t nblocks, const Batch &B, const Framed &fr,
               uint8_t *out, size_t out_cap, uint32_t *out_off, int32_t *block_status, uint32_t *stop_piece) {
  std::vector<size_t> need(nblocks, 0);
  parallel_for(nblocks, 256, [&](size_t i) {
    size_t n = 0;
    for_each_run(B, i, fr, [&](const uint8_t *, size_t len) { n += len; });
    need[i] = n;
  });
  size_t o = 0;
  int ret = 0;
  out_off[0] = 0;
  for (uint32_t i = 0; i < nblocks; ++i) {
    if (block_status[i] == 0 && deflaters[i]->bad) {
      // an earlier block of this deflater ran out of room in this call:
      // later ones fail as nghttp2_hd_deflate_hd_bufs does (:1475-1477)
      block_status[i] = NGHTTP2_AMD_ERR_HEADER_COMP;
    } else if (block_status[i] == 0 && (o + need[i] > out_cap || o + need[i] > UINT32_MAX)) {
      // INSUFF_BUFSIZE in nghttp2_hd_deflate_hd2 (:1546-1547); the deflater turns bad
      block_status[i] = NGHTTP2_AMD_ERR_BUFFER_ERROR;
      deflaters[i]->bad = true;
      ret = NGHTTP2_AMD_ERR_BUFFER_ERROR;
      if (stop_piece) {
        size_t n = o;
        uint32_t k = 0;
        for (const Piece &pc : B.pieces[i]) {
          n += pc.bytes.size();
          for (int j = 0; j < 2; ++j)
            if (pc.lit[j] >= 0) {
              const uint32_t g = B.litbase[i] + (uint32_t)pc.lit[j];
              n += fr.off[g + 1] - fr.off[g];
            }
          if (n > out_cap) break;
          ++k;
        }
        *stop_piece = k;
      }
    } else if (block_status[i] == 0) {
      block_status[i] = (int32_t)need[i];
      o += need[i];
    }
    out_off[i + 1] = (uint32_t)o;
  }
  parallel_for(nblocks, 256, [&](size_t i) {
    if (block_status[i] < 0) return;
    uint8_t *w = out + out_off[i];
    for_each_run(B, i, fr, [&](const uint8_t *p, size_t len) {
      memcpy(w, p, len);
      w += len;
    });
  });
  return ret;
}

}  // namespace

extern "C" {

// test hooks (include/nghttp2_amd_hd_testing.h)
void nghttp2_amd_hd__test_fail_deflate_gpu(int n) { g_fail_gpu.store(n); }
void nghttp2_amd_hd__set_gpu_names_min(uint32_t n) { g_names_min.store(n); }

int nghttp2_amd_hd_deflate_new(nghttp2_amd_hd_deflater **deflater_ptr,
                               size_t max_deflate_dynamic_table_size) {
  if (!deflater_ptr) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  nghttp2_amd_hd_deflater *d = new (std::nothrow) nghttp2_amd_hd_deflater();
  if (!d) return NGHTTP2_AMD_ERR_NOMEM;
  // nghttp2_hd_deflate_new2 (lib/nghttp2_hd.c:721-748): the table starts at
  // min(4096, max_deflate) and a smaller maximum is announced by a size update
  d->deflate_max = max_deflate_dynamic_table_size;
  d->bufsize_max = 4096;
  if (max_deflate_dynamic_table_size < 4096) {
    d->notify = true;
    d->bufsize_max = max_deflate_dynamic_table_size;
  }
  *deflater_ptr = d;
  return 0;
}

void nghttp2_amd_hd_deflate_del(nghttp2_amd_hd_deflater *deflater) { delete deflater; }

int nghttp2_amd_hd_deflate_change_table_size(nghttp2_amd_hd_deflater *d,
                                             size_t settings_max_dynamic_table_size) {
  if (!d) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const size_t next = settings_max_dynamic_table_size < d->deflate_max
                          ? settings_max_dynamic_table_size : d->deflate_max;
  d->bufsize_max = next;
  d->min_max = d->min_max < next ? d->min_max : next;
  d->notify = true;
  d->shrink();
  return 0;
}

size_t nghttp2_amd_hd_deflate_get_num_table_entries(nghttp2_amd_hd_deflater *d) {
  return d ? d->table.size() + kStaticLen : 0;
}

int nghttp2_amd_hd_deflate_get_table_entry(nghttp2_amd_hd_deflater *d, size_t idx,
                                           const uint8_t **name, size_t *namelen,
                                           const uint8_t **value, size_t *valuelen) {
  if (!d || idx == 0 || idx > d->table.size() + kStaticLen) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  --idx;
  if (idx < kStaticLen) {
    const char *n, *v;
    static_entry((uint32_t)idx, &n, namelen, &v, valuelen);
    *name = (const uint8_t *)n;
    *value = (const uint8_t *)v;
  } else {
    const Entry &e = d->table[idx - kStaticLen];
    *name = (const uint8_t *)e.name.data();
    *namelen = e.name.size();
    *value = (const uint8_t *)e.value.data();
    *valuelen = e.value.size();
  }
  return 0;
}

size_t nghttp2_amd_hd_deflate_get_dynamic_table_size(nghttp2_amd_hd_deflater *d) {
  return d ? d->bufsize : 0;
}

size_t nghttp2_amd_hd_deflate_get_max_dynamic_table_size(nghttp2_amd_hd_deflater *d) {
  return d ? d->bufsize_max : 0;
}

// nghttp2_hd_deflate_bound (lib/nghttp2_hd.c:1596-1621): two size updates of
// at most 6 bytes, per field two 6-byte length prefixes plus the raw bytes.
size_t nghttp2_amd_hd_deflate_bound(nghttp2_amd_hd_deflater *d, const nghttp2_amd_nv *nva,
                                    size_t nvlen) {
  (void)d;
  size_t n = 12 + 12 * nvlen;
  for (size_t i = 0; i < nvlen; ++i) n += nva[i].namelen + nva[i].valuelen;
  return n;
}

}  // extern "C"

namespace {
int deflate_blocks_impl(nghttp2_amd_hd_deflater *const *deflaters, uint32_t nblocks, const nghttp2_amd_nv *nva,
                        const uint32_t *block_nv_off, uint8_t *out, size_t out_cap, uint32_t *out_off,
                        int32_t *block_status, void *stream, uint32_t *stop_piece) {
  if (nblocks == 0) {
    if (out_off) out_off[0] = 0;
    return 0;
  }
  if (!deflaters || !block_nv_off || !out_off || !block_status || (!nva && block_nv_off[nblocks]))
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < nblocks; ++i)
    if (!deflaters[i] || block_nv_off[i] > block_nv_off[i + 1]) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;

  nghttp2_amd_host::Pool::CallScope scope;  // workers spin between this call's phases only
  nghttp2_amd_host::Phases ph("deflate");
  const uint32_t f0 = block_nv_off[0], nf = block_nv_off[nblocks] - f0;
  std::vector<uint32_t> fnt;  // the names' hashes and tokens; empty: looked up on the host
  if (nf && nf >= g_names_min.load()) {
    if (const int rv = stage_name_tokens(nva + f0, nf, stream, &fnt)) return rv;
    ph.mark("names");
  }
  Batch B;
  deflate_tables(deflaters, nblocks, nva, block_nv_off, fnt, block_status, &B);
  ph.mark("tables");
  // Pass 1 has changed the deflaters (entries inserted, size updates
  // consumed).  From here on a failure leaves the encoder tables ahead of
  // what the peer will receive, so every deflater of the batch turns bad and
  // every block not failed already reports the error, as
  // nghttp2_hd_deflate_hd_bufs sets ctx.bad on each failure path
  // (lib/nghttp2_hd.c:1509-1516).
  auto fail_batch = [&](int rv) {
    for (uint32_t i = 0; i < nblocks; ++i) {
      deflaters[i]->bad = true;
      if (block_status[i] >= 0) block_status[i] = rv;
      out_off[i + 1] = 0;
    }
    out_off[0] = 0;
    return rv;
  };
  std::lock_guard<std::mutex> guard(engine().mu);
  Framed fr;
  if (const int rv = frame_literals(engine(), nblocks, B, stream, &fr)) return fail_batch(rv);
  ph.mark("gpu");
  const int ret = place_wire(deflaters, nblocks, B, fr, out, out_cap, out_off, block_status, stop_piece);
  ph.mark("wire");
  return ret;
}
}  // namespace

extern "C" {

int nghttp2_amd_hd_deflate_blocks(nghttp2_amd_hd_deflater *const *deflaters, uint32_t nblocks,
                                  const nghttp2_amd_nv *nva, const uint32_t *block_nv_off,
                                  uint8_t *out, size_t out_cap, uint32_t *out_off,
                                  int32_t *block_status, void *stream) {
  return deflate_blocks_impl(deflaters, nblocks, nva, block_nv_off, out, out_cap, out_off, block_status, stream,
                             nullptr);
}

ptrdiff_t nghttp2_amd_hd_deflate_hd2(nghttp2_amd_hd_deflater *deflater, uint8_t *buf, size_t buflen,
                                     const nghttp2_amd_nv *nva, size_t nvlen, void *stream) {
  if (!deflater || (!buf && buflen) || (!nva && nvlen) || nvlen > UINT32_MAX)
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const uint32_t nv_off[2] = {0, (uint32_t)nvlen};
  uint32_t out_off[2] = {0, 0};
  int32_t st = 0;
  uint8_t none = 0;
  // (the table before the block: see below)
  std::unique_ptr<nghttp2_amd_hd_deflater> before(deflater->bad ? nullptr : new nghttp2_amd_hd_deflater(*deflater));
  uint32_t stop = 0;
  const int rv = deflate_blocks_impl(&deflater, 1, nva, nv_off, buf ? buf : &none, buflen, out_off, &st, stream,
                                     &stop);
  if (st == NGHTTP2_AMD_ERR_BUFFER_ERROR) {  // :1546-1547
    // The reference deflates field by field and stops at the representation
    // that does not fit, after that field's table insertion (deflate_nv
    // inserts, then emits); the passes above have inserted every field of the
    // list.  So the table is put back and the fields up to that one are
    // deflated again (stop counts the pending size updates' piece).
    if (before) {
      const uint32_t lead = before->notify ? 1u : 0u;
      const uint32_t nfields = stop < lead ? 0u : std::min<uint32_t>(stop - lead + 1u, (uint32_t)nvlen);
      *deflater = std::move(*before);
      std::vector<Piece> P;
      Lits L;
      deflate_block(deflater, nva, nfields, nullptr, 0, P, L);
      deflater->bad = true;
    }
    return NGHTTP2_AMD_ERR_INSUFF_BUFSIZE;
  }
  if (st < 0) return st;
  if (rv < 0) return rv;
  return (ptrdiff_t)st;
}

ptrdiff_t nghttp2_amd_hd_deflate_hd_vec2(nghttp2_amd_hd_deflater *deflater, const nghttp2_amd_vec *vec,
                                         size_t veclen, const nghttp2_amd_nv *nva, size_t nvlen,
                                         void *stream) {
  if (!deflater || (!vec && veclen)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  size_t total = 0;
  for (size_t i = 0; i < veclen; ++i) {
    if (!vec[i].base && vec[i].len) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
    total += vec[i].len;
  }
  // one chunk: the wire straight into it
  if (veclen == 1) return nghttp2_amd_hd_deflate_hd2(deflater, vec[0].base, vec[0].len, nva, nvlen, stream);
  // else the wire into one contiguous scratch buffer, then across the chunks
  // in order (nghttp2_bufs_wrap_init2 fills them one by one).  The scratch is
  // not zero-filled and is capped at the list's bound (an output always fits
  // that, so the cap changes no result).  On INSUFF_BUFSIZE the chunks are
  // left untouched, where the reference leaves the bytes it had written.
  const size_t cap = std::min(total, nghttp2_amd_hd_deflate_bound(deflater, nva, nvlen));
  std::unique_ptr<uint8_t[]> tmp(new (std::nothrow) uint8_t[cap ? cap : 1]);
  if (!tmp) return NGHTTP2_AMD_ERR_NOMEM;
  const ptrdiff_t n = nghttp2_amd_hd_deflate_hd2(deflater, tmp.get(), cap, nva, nvlen, stream);
  if (n < 0) return n;
  size_t o = 0;
  for (size_t i = 0; i < veclen && o < (size_t)n; ++i) {
    const size_t k = std::min(vec[i].len, (size_t)n - o);
    memcpy(vec[i].base, tmp.get() + o, k);
    o += k;
  }
  return n;
}

}  // extern "C"
