// hd_inflate.cpp -- batched HPACK inflate front-end.
//
// Host C++ above the C ABI.  Inflates many complete header blocks (of one or
// many connections) per call and sends every Huffman literal of the batch
// through ONE GPU decode (nghttp2_amd_hd_huff_decode_batch_auto), instead of
// one nghttp2_hd_huff_decode per literal:
//   pass 1  cut each block into its representations (hd_parse.h's walk and
//           record, the device path's: the wire is self-delimiting, no table
//           state needed), collecting the Huffman literals into one pinned
//           pool;
//   GPU     H2D, batch decode, D2H (async on the caller's stream);
//   pass 2  replay the blocks in batch order against each inflater's dynamic
//           table -- index resolution, insertion with eviction, table size
//           updates -- and emit the header fields.
// Semantics follow nghttp2_hd_inflate_hd_nv (lib/nghttp2_hd.c:1919-2281) with
// in_final = 1 and nghttp2_hd_inflate_end_headers after each block:
// decode_length (:882-945) with its overflow and maximum checks, the table
// size update rules (:1942-2003, nghttp2_hd_inflate_change_table_size
// :1290-1322), commit_indexed / newname / indname (:1780-1875),
// add_hd_table_incremental (:1130-1195), and the sticky bad state (:1932).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_field_classes.h"
#include "hd_host.h"
#include "hd_http.h"
#include "hd_parse.h"
#include "hd_tokens.h"
#include "host_threads.h"

namespace {

using namespace hdhost;  // the static table, hip_ok, DevBuf / PinnedBuf
const char *const kLayer = "inflate";  // (in hip_ok's messages)
const uint32_t kDefaultTable = 4096;   // NGHTTP2_HD_DEFAULT_MAX_BUFFER_SIZE

// The dynamic table (lib/nghttp2_hd.c hd_ringbuf + nghttp2_hd_entry, restated
// without a heap object per entry): entry descriptors in a power-of-two ring,
// the entries' name/value bytes in one byte ring, each entry contiguous (an
// entry that would cross the ring's end starts at 0 and the tail is skipped).
// Insertion and eviction allocate nothing once the rings have grown to the
// connection's working size; a ring that cannot place an entry is compacted
// into one twice as large.
// An entry also carries what is known of its bytes, an Ann: filled at
// insertion with what the inserting call computed, and at the first reference
// by a call that wants more (entry_ann), so an indexed field costs an annotated
// call no byte scan.
const uint8_t kUnchecked = NGHTTP2_AMD_CHECK_INVALID;
const int8_t kTokUnknown = -3;  // (below NGHTTP2_AMD_TOKEN_INVALID; a token is -1..67)
const uint32_t kFactUnknown = NGHTTP2_AMD_HTTP_FACT_INVALID;
// Which annotations a call wants: the check masks (a checked call), the name
// tokens (a tokened call), the HTTP verdicts (an _http call, which needs the
// other two as well).
struct Want {
  bool checks, tokens, http;
  constexpr Want(bool c, bool t, bool h) : checks(c || h), tokens(t || h), http(h) {}
  bool any() const { return checks || tokens; }
};
// The annotations of one field; by default nothing is known.
struct Ann {
  uint8_t cn = kUnchecked, cv = kUnchecked;  // the NGHTTP2_AMD_CHECK_* masks of name and value
  int8_t tk = kTokUnknown;                   // the name's token (lookup_token)
  uint32_t vf = kFactUnknown;                // the value's HTTP facts and number (hd_http.h)
  int64_t vn = -1;
  // the members w asks for that are not known yet, from the bytes
  void fill_name(const uint8_t *n, size_t nl, Want w) {
    if (w.checks && cn == kUnchecked) cn = hdcls::check_field(n, nl);
    if (w.tokens && tk == kTokUnknown) tk = (int8_t)hdtok::lookup_token(n, nl);
  }
  void fill_value(const uint8_t *v, size_t vl, Want w) {
    if (w.checks && cv == kUnchecked) cv = hdcls::check_field(v, vl);
    if (w.http && vf == kFactUnknown) vf = hdhttp::http_facts(v, vl, &vn);
  }
};
struct DynTable {
  struct Ent {
    size_t off;
    uint32_t nl, vl;
    Ann ann;
  };
  std::vector<Ent> ents;   // ring, capacity a power of two
  size_t e_first = 0;      // oldest entry
  size_t count = 0;
  std::vector<uint8_t> buf;  // byte ring

  const Ent &newest(size_t k) const {  // k = 0: the most recent (dynamic index 62)
    return ents[(e_first + count - 1 - k) & (ents.size() - 1)];
  }
  Ent &newest(size_t k) { return ents[(e_first + count - 1 - k) & (ents.size() - 1)]; }
  const uint8_t *name(const Ent &e) const { return buf.data() + e.off; }
  const uint8_t *value(const Ent &e) const { return buf.data() + e.off + e.nl; }
  size_t bytes(const Ent &e) const { return (size_t)e.nl + e.vl; }
  void pop_oldest() {
    e_first = (e_first + 1) & (ents.size() - 1);
    --count;
  }
  // offset for s contiguous bytes, or SIZE_MAX.  Occupied: [head, tail)
  // unwrapped, or [head, cap) + [0, tail) once the newest entry sits before
  // the oldest; placements keep one byte free before head so the two stay
  // distinguishable.
  size_t place(size_t s) const {
    const size_t cap = buf.size();
    if (count == 0) return s <= cap ? 0 : SIZE_MAX;
    const Ent &o = ents[e_first], &w = newest(0);
    const size_t head = o.off, tail = w.off + bytes(w);
    if (w.off >= head) {  // unwrapped
      if (cap - tail >= s) return tail;
      return s < head ? 0 : SIZE_MAX;
    }
    return tail + s < head ? tail : SIZE_MAX;
  }
  void grow(size_t need) {  // compact the entries, oldest first, into a larger ring
    size_t live = 0;
    for (size_t k = 0; k < count; ++k) live += bytes(newest(k));
    std::vector<uint8_t> nb(std::max<size_t>(std::max<size_t>(2 * buf.size(), 2 * (live + need) + 2), 256));
    size_t at = 0;
    for (size_t k = count; k-- > 0;) {
      Ent &e = ents[(e_first + count - 1 - k) & (ents.size() - 1)];
      if (bytes(e)) memcpy(nb.data() + at, buf.data() + e.off, bytes(e));
      e.off = at;
      at += bytes(e);
    }
    buf.swap(nb);
  }
  // n / v must not point into this table (the caller passes copies)
  void push(const uint8_t *n, size_t nl, const uint8_t *v, size_t vl, const Ann &a) {
    if (count == ents.size()) {  // grow the descriptor ring, oldest first
      std::vector<Ent> ne(ents.empty() ? 16 : 2 * ents.size());
      for (size_t k = 0; k < count; ++k) ne[k] = ents[(e_first + k) & (ents.size() - 1)];
      ents.swap(ne);
      e_first = 0;
    }
    size_t at = place(nl + vl);
    if (at == SIZE_MAX) {
      grow(nl + vl);
      at = place(nl + vl);
    }
    if (nl) memcpy(buf.data() + at, n, nl);
    if (vl) memcpy(buf.data() + at + nl, v, vl);
    ents[(e_first + count) & (ents.size() - 1)] = Ent{at, (uint32_t)nl, (uint32_t)vl, a};
    ++count;
  }
};
static_assert(sizeof(DynTable::Ent) == 32, "the replay is sensitive to the descriptor's size");

}  // namespace

struct nghttp2_amd_hd_inflater {
  DynTable table;
  size_t bufsize = 0;
  size_t bufsize_max = kDefaultTable;           // ctx.hd_table_bufsize_max
  size_t settings_max = kDefaultTable;          // settings_hd_table_bufsize_max
  size_t min_max = UINT32_MAX;                  // min_hd_table_bufsize_max
  size_t max_nl = 0, max_vl = 0;                // longest name / value ever inserted (bounds)
  bool expect_size = false;                     // NGHTTP2_HD_STATE_EXPECT_TABLE_SIZE
  bool bad = false;                             // ctx.bad
  // a block failed outside NGHTTP2_HD_STATE_EXPECT_TABLE_SIZE: fail: (:2283-2287)
  // leaves the state where it was and the caller of a failed block does not
  // call end_headers (lib/nghttp2_session.c:3556-3690), so
  // nghttp2_hd_inflate_change_table_size answers INVALID_STATE from then on
  bool mid_block = false;
  uint64_t batch_gen = 0;                       // the inflate_blocks call that last grouped it
  uint32_t batch_conn = 0;                      // its connection number in that call

  void evict_oldest() {
    bufsize -= table.bytes(table.ents[table.e_first]) + kEntryOverhead;
    table.pop_oldest();
  }
  void shrink() {  // hd_context_shrink_table_size
    while (bufsize > bufsize_max && table.count) evict_oldest();
  }
  // add_hd_table_incremental (:1130-1195): evict until the entry fits, then
  // insert it unless it is larger than the whole table.  n / v are copies
  // outside the table (the caller's emitted field), so a name taken from an
  // entry that this insertion evicts stays valid, as in the reference.
  // a: what the inserting call knows of the field.
  void add(const uint8_t *n, size_t nl, const uint8_t *v, size_t vl, const Ann &a) {
    const size_t room = nl + vl + kEntryOverhead;
    while (bufsize + room > bufsize_max && table.count) evict_oldest();
    if (room > bufsize_max) return;
    table.push(n, nl, v, vl, a);
    bufsize += room;
    max_nl = std::max(max_nl, nl);
    max_vl = std::max(max_vl, vl);
  }
  size_t max_index() const { return table.count + kStaticLen; }  // get_max_index
  // entry idx of the index space, 0-based (idx < max_index()): static, then
  // the dynamic table newest first
  void entry(size_t idx, const char **n, size_t *nl, const char **v, size_t *vl) const {
    if (idx < kStaticLen) return static_entry((uint32_t)idx, n, nl, v, vl);
    const DynTable::Ent &e = table.newest(idx - kStaticLen);
    *n = (const char *)table.name(e);
    *nl = e.nl;
    *v = (const char *)table.value(e);
    *vl = e.vl;
  }
  // the annotations of entry idx (as entry()) that w asks for: the static
  // table's are all computed once per process; a dynamic entry's are in its
  // descriptor, where this fills in what w asks for and no earlier call has
  const Ann &entry_ann(size_t idx, Want w) {
    if (idx < kStaticLen) {
      struct Anns {
        Ann a[kStaticLen];
      };
      static const Anns st = [] {
        Anns t;
        for (uint32_t i = 0; i < kStaticLen; ++i) {
          t.a[i].fill_name((const uint8_t *)kStatic[i][0], kStaticLens.len[i][0], Want(true, true, true));
          t.a[i].fill_value((const uint8_t *)kStatic[i][1], kStaticLens.len[i][1], Want(true, true, true));
        }
        return t;
      }();
      return st.a[idx];
    }
    DynTable::Ent &e = table.newest(idx - kStaticLen);
    e.ann.fill_name(table.name(e), e.nl, w);
    e.ann.fill_value(table.value(e), e.vl, w);
    return e.ann;
  }
};

namespace {

using hdparse::Literal;  // a record's name or value string literal (hdparse::literal)

// One block of the batch: its representations (pass 1, hdparse::walk: offsets
// are positions in the block, Huffman literals numbered within the block until
// number_block adds the block's base) and the block's bytes.
struct alignas(128) Block {  // (aligned as BlockOut)
  std::vector<nghttp2_amd_hd_op> ops;  // (kept across calls: no allocation once grown)
  const uint8_t *in = nullptr;         // the block's bytes, for the records' raw literals
  bool parse_ok = true;
  bool first_is_size = false;  // the block's first byte opens a table size update
  // the output bound's parts (pass 1): fields, bytes other than dynamic-table
  // references, and the number of those references
  uint64_t nv = 0, ar = 0, ndyn = 0;
  // the longest name and value any literal of the block can emit (a Huffman
  // one at its decode bound): with the table's and the static table's
  // longest, they bound what a dynamic-table reference of the block emits
  uint64_t lit_name = 0, lit_val = 0;
};
// (the replay walks a block's records in place, two to a cache line; a block's
// own state stays within the one line its alignment gives it)
static_assert(sizeof(nghttp2_amd_hd_op) == 32 && sizeof(Block) == 128, "the replay is sensitive to the record's size");

// One emitted field: its name\0value\0 run's place in the bytes it was written
// to, and what of its annotations the caller may have asked for.
struct Rec {
  uint32_t name_off, name_len, value_off, value_len;
  uint8_t flags;
  uint8_t cn, cv;  // the check masks of name and value (a checked call)
  int8_t tk;       // the name's token (a tokened call)
  int32_t vd;      // the field's HTTP verdict (an _http call)
  Rec(size_t at, size_t nl, size_t vl, uint8_t fl, const Ann &a, int32_t verdict)
      : name_off((uint32_t)at), name_len((uint32_t)nl), value_off((uint32_t)(at + nl + 1)), value_len((uint32_t)vl),
        flags(fl), cn(a.cn), cv(a.cv), tk(a.tk), vd(verdict) {}
};
static_assert(sizeof(Rec) == 24, "the replay is sensitive to the record's size");
// The caller's per-field arrays: the fields and their bytes, and the masks,
// tokens and verdicts of the calls that ask for them (else nullptr).
struct FieldOut {
  nghttp2_amd_hd_nv *nva;
  uint8_t *arena;
  uint8_t *checks;    // two masks per field
  int32_t *tokens;    // a token per field
  int32_t *verdicts;  // a verdict per field
  // field k of the call: r of block `block`, whose bytes are at arena + base
  void put(size_t k, uint32_t block, uint32_t base, const Rec &r) const {
    nva[k] = nghttp2_amd_hd_nv{block, base + r.name_off, r.name_len, base + r.value_off, r.value_len, r.flags};
    if (checks) checks[2 * k] = r.cn, checks[2 * k + 1] = r.cv;
    if (tokens) tokens[k] = r.tk;
    if (verdicts) verdicts[k] = r.vd;
  }
};
// a field's name\0value\0 run at d, NUL-terminated like the reference's rcbufs (:2112, :2201)
void put_bytes(uint8_t *d, const char *n, size_t nl, const char *v, size_t vl) {
  if (nl) memcpy(d, n, nl);
  d[nl] = 0;
  if (vl) memcpy(d + nl + 1, v, vl);
  d[nl + 1 + vl] = 0;
}
// A growable byte buffer written through a raw pointer (no per-append
// capacity check or zero fill): a block's name\0value\0 runs.
struct ByteBuf {
  std::unique_ptr<uint8_t[]> p;
  size_t n = 0, cap = 0;
  void clear() { n = 0; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  const uint8_t *data() const { return p.get(); }
  uint8_t *room(size_t k) {  // k more bytes at the end
    if (n + k > cap) {
      const size_t nc = std::max<size_t>(2 * cap, std::max<size_t>(n + k, 256));
      std::unique_ptr<uint8_t[]> q(new uint8_t[nc]);
      if (n) memcpy(q.get(), p.get(), n);
      p.swap(q);
      cap = nc;
    }
    uint8_t *r = p.get() + n;
    n += k;
    return r;
  }
};
// (128-byte aligned: neighbouring blocks belong to different connections, so
// different replay threads; on shared lines every emit's size update would
// bounce the line between cores)
struct alignas(128) BlockOut {
  std::vector<Rec> recs;
  ByteBuf bytes;
  int32_t status = 0;
  nghttp2_amd_hd_http_state hst{};  // an _http call: the state after the block, and the block's result
  int32_t hres = 0;
};

struct Engine {
  std::mutex mu;
  PinnedBuf h_pool;  // Huffman literals in
  PinnedBuf h_out;   // decoded literals out
  PinnedBuf h_meta;  // uint32: offsets in, then slots and status out ((nh + 1) each), facts, tokens, masks
  DevBuf d_in, d_out, d_meta;  // their device copies (the modes that copy)
  std::vector<BlockOut> outs;
  // pass 1 state, kept across calls (under mu)
  std::vector<Block> bl;
  std::vector<uint32_t> nhuff;
  std::vector<uint64_t> hbytes;
  std::vector<uint32_t> hoff;
  uint64_t gen = 0;  // inflate_blocks calls (the connections' grouping stamp)
  std::vector<nghttp2_amd_hd_inflater *> conns;
  std::vector<uint32_t> cstart, corder;  // blocks per connection, in batch order
};
Engine &engine() {
  static Engine e;
  return e;
}

// Where pass 2 finds a literal's bytes: the wire, or the decoded pool.
struct LitSrc {
  const uint8_t *dec;
  const uint32_t *slot;
  const int32_t *st;
  const uint8_t *chk;  // a checked call: the decoded literals' check masks (the GPU's)
  const int32_t *tok;  // a tokened call: the decoded literals' tokens (the GPU's)
  const uint32_t *fct;  // an _http call: the decoded literals' HTTP facts and numbers (the GPU's)
  const int64_t *num;
  // literal l of a block whose bytes are at in; false: -523 (bad padding or
  // EOS, hd_inflate_read_huff :1740-1750)
  bool get(const uint8_t *in, const Literal &l, const char **p, size_t *n) const {
    if (!l.huff) {
      *p = (const char *)in + l.off;
      *n = l.len;
      return true;
    }
    const int32_t s = st[l.lit];
    if (s < 0) return false;
    *p = (const char *)dec + slot[l.lit];
    *n = (size_t)s;
    return true;
  }
  // what w asks for of a field whose value literal, and name literal unless
  // the name is an entry's (nullptr), get() returned: a raw literal is scanned
  // here (on the replay's thread), a Huffman one was scanned behind its decode
  Ann ann(const uint8_t *in, const Literal *name, const Literal &val, Want w) const {
    Ann a;
    if (name && !name->huff) {
      a.fill_name(in + name->off, name->len, w);
    } else if (name) {
      if (w.checks) a.cn = chk[name->lit];
      if (w.tokens) a.tk = (int8_t)tok[name->lit];
    }
    if (!val.huff) {
      a.fill_value(in + val.off, val.len, w);
    } else {
      if (w.checks) a.cv = chk[val.lit];
      if (w.http) a.vf = fct[val.lit], a.vn = num[val.lit];
    }
    return a;
  }
};

// What one dynamic-table reference of block b can emit (name + value): any
// entry it can reach is one in the table now or one the block inserts, whose
// name is a literal's, a static entry's or an older entry's and whose value
// is a literal's.  So the longest name / value inserted so far, the static
// table's and the block's literals bound it -- and so does the table limit
// (round 6: the limit alone made a table of UINT32_MAX bytes send every
// block with a dynamic reference through the slow copy-and-replay path).
uint64_t dyn_ref_bound(const nghttp2_amd_hd_inflater *c, uint64_t lit_name, uint64_t lit_val) {
  const uint64_t lim = std::min<uint64_t>(std::max<size_t>({64u, c->settings_max, c->bufsize_max}), UINT32_MAX);
  const uint64_t n = std::max<uint64_t>({c->max_nl, kStaticLens.max[0], lit_name});
  const uint64_t v = std::max<uint64_t>({c->max_vl, kStaticLens.max[1], lit_val});
  return std::min(lim, n + v);
}
// (the bounds saturate at UINT64_MAX: a table limit near SIZE_MAX must not
// wrap them)
uint64_t sat_add(uint64_t a, uint64_t b) { return a > UINT64_MAX - b ? UINT64_MAX : a + b; }
// A block's arena bound: its own bytes plus its dynamic-table references at
// ref_max each (dyn_ref_bound).
uint64_t block_ar_bound(const Block &b, uint64_t ref_max) {
  return sat_add(b.ar, b.ndyn && ref_max > UINT64_MAX / b.ndyn ? UINT64_MAX : b.ndyn * ref_max);
}

// Pass 2 for one block against its inflater (in order within a connection):
// hd_inflate_commit_indexed / newname / indname (:1780-1875), the table size
// update rules (:1942-2003), add_hd_table_incremental, and the end-of-block
// checks; the bad state is sticky (:1932-1934, :2276).
// A block's fields go to a sink: its own buffers (BlockSink, placed in block
// order after a parallel replay), or straight into the caller's arena and
// field array (DirectSink: one connection, output bound within the caps).
struct BlockSink {
  BlockOut &out;
  void begin() {
    out.recs.clear();
    out.bytes.clear();
  }
  void emit(const char *n, size_t nl, const char *v, size_t vl, uint8_t flags, const Ann &a, int32_t vd) {
    out.recs.emplace_back(out.bytes.size(), nl, vl, flags, a, vd);
    put_bytes(out.bytes.room(nl + vl + 2), n, nl, v, vl);
  }
  // the field just emitted (the table copies it from here)
  const uint8_t *last_name() const { return (const uint8_t *)out.bytes.data() + out.recs.back().name_off; }
  const uint8_t *last_value() const { return (const uint8_t *)out.bytes.data() + out.recs.back().value_off; }
  void finish(int32_t status) { out.status = status; }
  int32_t count() const { return (int32_t)out.recs.size(); }
};
struct DirectSink {
  const FieldOut &fo;
  int32_t *status;
  size_t ar = 0, nv = 0, nv0 = 0;
  uint32_t block = 0;
  void begin() { nv0 = nv; }
  void emit(const char *n, size_t nl, const char *v, size_t vl, uint8_t flags, const Ann &a, int32_t vd) {
    fo.put(nv++, block, 0, Rec(ar, nl, vl, flags, a, vd));
    put_bytes(fo.arena + ar, n, nl, v, vl);
    ar += nl + vl + 2;
  }
  const uint8_t *last_name() const { return fo.arena + fo.nva[nv - 1].name_off; }
  const uint8_t *last_value() const { return fo.arena + fo.nva[nv - 1].value_off; }
  void finish(int32_t st) { status[block] = st; }
  int32_t count() const { return (int32_t)(nv - nv0); }
};

// An _http call's view of one block: the driver k_http_blocks runs
// (hd_http.h), its fields built from the annotations.
typedef hdhttp::BlockRun HttpRun;
hdhttp::Field http_field(const char *n, size_t nl, size_t vl, const Ann &a) {
  return hdhttp::Field{(const uint8_t *)n, nl, vl, a.tk, a.cn, a.cv, a.vf, a.vn};
}

// want: the annotations every emitted field carries.  http: an _http call
// (want.http) -- every emitted field with its verdict, the block's state and
// result in *http; else nullptr.
template <class Sink>
void replay_block(nghttp2_amd_hd_inflater *inf, const Block &b, const LitSrc &ls, Want want, HttpRun *http,
                  Sink &out) {
  out.begin();
  bool ok = !inf->bad;
  bool head = true;  // size updates only at the head of a block
  for (size_t k = 0; ok && k < b.ops.size(); ++k) {
    const nghttp2_amd_hd_op &op = b.ops[k];
    if (inf->expect_size && op.kind != NGHTTP2_AMD_HD_OP_SIZE) {
      ok = false;
      break;
    }
    if (op.kind == NGHTTP2_AMD_HD_OP_SIZE) {
      if (!head || op.value > (inf->min_max < inf->settings_max ? inf->min_max : inf->settings_max)) {
        ok = false;
        break;
      }
      inf->expect_size = false;
      inf->min_max = UINT32_MAX;
      inf->bufsize_max = op.value;
      inf->shrink();
      continue;
    }
    head = false;
    const char *n, *v;
    size_t nl, vl;
    if (op.kind == NGHTTP2_AMD_HD_OP_INDEXED) {  // hd_inflate_commit_indexed
      if (op.value == 0 || op.value > inf->max_index()) {
        ok = false;
        break;
      }
      inf->entry(op.value - 1, &n, &nl, &v, &vl);
      static const Ann kNone;
      const Ann &a = want.any() ? inf->entry_ann(op.value - 1, want) : kNone;
      out.emit(n, nl, v, vl, 0, a, http ? http->step(http_field(n, nl, vl, a)) : 0);
      continue;
    }
    const bool new_name = (op.flags & NGHTTP2_AMD_HD_OP_NEW_NAME) != 0;
    const Literal name = hdparse::literal(op, 0), val = hdparse::literal(op, 1);
    const Ann *name_ann = nullptr;  // an indexed name's
    if (new_name) {  // hd_inflate_commit_newname
      if (!ls.get(b.in, name, &n, &nl)) {
        ok = false;
        break;
      }
    } else {  // hd_inflate_commit_indname
      if (op.value == 0 || op.value > inf->max_index()) {
        ok = false;
        break;
      }
      const char *v0;
      size_t vl0;
      inf->entry(op.value - 1, &n, &nl, &v0, &vl0);
      if (want.any()) name_ann = &inf->entry_ann(op.value - 1, want);
    }
    if (!ls.get(b.in, val, &v, &vl)) {
      ok = false;
      break;
    }
    Ann a = ls.ann(b.in, new_name ? &name : nullptr, val, want);
    if (name_ann) a.cn = name_ann->cn, a.tk = name_ann->tk;
    const uint8_t flags = (op.flags & NGHTTP2_AMD_HD_OP_NO_INDEX) ? 1u : 0u;  // NGHTTP2_NV_FLAG_NO_INDEX
    out.emit(n, nl, v, vl, flags, a, http ? http->step(http_field(n, nl, vl, a)) : 0);
    if (op.flags & NGHTTP2_AMD_HD_OP_INDEX_REQUIRED)  // the table copies the field just emitted
      inf->add(out.last_name(), nl, out.last_value(), vl, a);
  }
  // truncated or malformed wire after the parsed representations; and a
  // block that ends while a table size update is still expected
  // (lib/nghttp2_hd.c:2259-2266)
  if (ok && (!b.parse_ok || inf->expect_size)) ok = false;
  if (!ok) {
    // Where the reference's state stays: a block that starts while an update
    // is expected and does not open with one fails on its first byte (or at
    // its end, being empty) still in EXPECT_TABLE_SIZE (:1942-1949,
    // :2259-2266); every other failure is in the middle of a representation.
    if (!inf->bad) inf->mid_block = !(inf->expect_size && !b.first_is_size);
    inf->bad = true;
    if (http) http->finish(NGHTTP2_AMD_ERR_HEADER_COMP);
    out.finish(NGHTTP2_AMD_ERR_HEADER_COMP);  // the fields before the error stay emitted
  } else {
    if (http) http->finish(0);
    out.finish(out.count());
  }
}

// ---- the phases of nghttp2_amd_hd_inflate_blocks, each named after the trace mark that closes it
using nghttp2_amd_host::parallel_for;
using nghttp2_amd_host::Phases;

// The caller's output buffers.
struct Dest {
  FieldOut fo;
  size_t nva_cap, *nva_used;
  size_t arena_cap, *arena_used;
  int32_t *block_status;
  // an _http call: a mode per block, the streams' states in and out, and a
  // result per block (may be nullptr); else all nullptr
  const uint8_t *block_modes;
  nghttp2_amd_hd_http_state *block_state;
  int32_t *block_http;
  HttpRun run(uint32_t i) const { return HttpRun{block_state[i], block_modes[i]}; }
  void set_http(uint32_t i, const nghttp2_amd_hd_http_state &st, int32_t res) const {
    block_state[i] = st;
    if (block_http) block_http[i] = res;
  }
};

// The parts of a parsed block's output bound: a field per representation,
// its name and value NUL-terminated; a literal's bytes (a Huffman one at its
// decode bound); a static-table reference at its entry's own length, a
// dynamic one counted (dyn_ref_bound bounds it at replay).
void bound_block(Block &b) {
  b.nv = b.ar = b.ndyn = b.lit_name = b.lit_val = 0;
  auto lit_len = [](const Literal &l) -> uint64_t {
    return l.huff ? (uint64_t)l.len * 8u / 5u + 1u : (uint64_t)l.len;
  };
  auto ref = [&](uint32_t idx, bool name_only) {
    if (idx >= 1 && idx <= kStaticLen)
      b.ar += kStaticLens.len[idx - 1][0] + (name_only ? 0 : kStaticLens.len[idx - 1][1]);
    else
      ++b.ndyn;
  };
  for (const nghttp2_amd_hd_op &op : b.ops) {
    if (op.kind == NGHTTP2_AMD_HD_OP_SIZE) continue;
    ++b.nv;
    b.ar += 2u;
    if (op.kind == NGHTTP2_AMD_HD_OP_INDEXED) {
      ref(op.value, false);
    } else {
      if (op.flags & NGHTTP2_AMD_HD_OP_NEW_NAME) {
        const uint64_t n = lit_len(hdparse::literal(op, 0));
        b.ar += n;
        b.lit_name = std::max(b.lit_name, n);
      } else {
        ref(op.value, true);
      }
      const uint64_t v = lit_len(hdparse::literal(op, 1));
      b.ar += v;
      b.lit_val = std::max(b.lit_val, v);
    }
  }
}

// "parse blocks" -- pass 1: every block cut into its representations by
// hdparse::walk (lib/nghttp2_hd.c:1942-1985 opcode dispatch, string literals,
// the truncation rule: stated there, once) and bounded; the walk's counts are
// the block's Huffman literals and their bytes (stateless: one task per block,
// so the literals are numbered within the block).  The engine's per-block
// buffers are kept across calls, so a warm call allocates nothing here; a call
// far below an earlier large batch releases the surplus (a high-water mark of 2x +
// 4096 blocks), so one large batch does not pin its footprint for the process's life.
void parse_blocks(Engine &E, uint32_t nblocks, const uint8_t *const *blocks, const size_t *block_lens) {
  auto trim = [nblocks](auto &v) {
    if (v.size() > 2u * (size_t)nblocks + 4096u) {
      v.resize(nblocks);
      v.shrink_to_fit();
    }
  };
  trim(E.bl), trim(E.outs);
  if (E.bl.size() < nblocks) E.bl.resize(nblocks);
  E.nhuff.assign(nblocks + 1, 0);   // Huffman literals per block, then prefix
  E.hbytes.assign(nblocks + 1, 0);  // their bytes per block, then prefix
  parallel_for(nblocks, 64, [&](size_t i) {
    // a malformed block keeps the representations before the error: the
    // reference emits those fields before it fails
    Block &b = E.bl[i];
    const uint32_t len = (uint32_t)block_lens[i];  // (the entry point refuses a longer block)
    b.in = blocks[i];
    b.first_is_size = hdparse::first_is_size(b.in, len);
    b.ops.clear();
    b.ops.reserve(len / 4 + 1);
    const hdparse::Counts c =
        hdparse::walk(b.in, 0u, len, 0u, [&b](uint32_t, const nghttp2_amd_hd_op &op) { b.ops.push_back(op); });
    b.parse_ok = c.ok;
    E.nhuff[i + 1] = c.lits;
    E.hbytes[i + 1] = c.lit_bytes;
    bound_block(b);
  });
}

// "number+copy": each block gives its Huffman literals their numbers in the batch (pass 1's
// block-local number plus k0, the Huffman literals of the blocks before: the walk's wire order,
// a name before its value) and copies their bytes into the pinned input pool from o on, in one
// parallel pass (round 5; before: numbering, then a separate gather).
// (by-value arguments: the loop reads nothing that may share a line with parallel_for's counter)
void number_block(Block &b, uint32_t k0, uint32_t o, uint8_t *hp, uint32_t *hoff) {
  for (nghttp2_amd_hd_op &op : b.ops) {
    if (op.kind != NGHTTP2_AMD_HD_OP_LITERAL) continue;
    for (int which = 0; which < 2; ++which) {
      const Literal l = hdparse::literal(op, which);
      if (!l.huff) continue;
      const uint32_t k = k0 + (uint32_t)l.lit;
      (which ? op.value_lit : op.name_lit) = (int32_t)k;
      memcpy(hp + o, b.in + l.off, l.len);
      o += l.len;
      hoff[k + 1] = o;
    }
  }
}
void number_and_copy(Engine &E, uint32_t nblocks) {
  E.hoff[0] = 0;
  parallel_for(nblocks, 64, [&E](size_t i) {
    number_block(E.bl[i], E.nhuff[i], (uint32_t)E.hbytes[i], E.h_pool.as<uint8_t>(), E.hoff.data());
  });
}

// NGHTTP2_AMD_INFLATE_ZC, read once per process (tests/test_inflate_zc.py
// runs the RFC and random-connection cases under each mode in its own
// process).  2, the default: the kernel reads the literals and offsets
// straight from the mapped pinned pools (zero-copy in: no H2D copies or their
// launch latencies) and its output is copied out -- DMA lands it in whole lines.
// 1: the output too goes through the mapped pool.  0: explicit copies both ways.
int zc_mode() {
  static const int mode = [] {
    const char *e = getenv("NGHTTP2_AMD_INFLATE_ZC");
    return e && (atoi(e) == 0 || atoi(e) == 1) ? atoi(e) : 2;
  }();
  return mode;
}

// "pools", "number+copy", "gpu issued": every Huffman literal of the batch
// in one decode, queued on the caller's stream.  The pinned pools are sized
// first, so number_and_copy can fill the input pool in place.  *ls says where
// replay finds the decoded literals once the stream has been waited for.
// A checked call queues nghttp2_amd_hd_check_fields_batch over the decode's
// (dst, slots, status) right behind it; the masks, a byte per literal, sit
// behind the status words and come back with them in the same copy.
// A tokened call queues nghttp2_amd_hd_name_tokens_len_batch (no hash: a
// literal longer than every token name is not read) over the same three
// arrays behind that; the tokens, an int32 per literal, sit between the status
// words and the masks and come back in that copy too.  Values get a token as
// names do (pass 1 numbers the literals without telling them apart); the
// replay reads the names' only.
// An _http call queues nghttp2_amd_hd_http_facts_batch behind those two; the
// numbers, an int64 per literal at the next 8-byte boundary behind the status
// words, and the facts, a uint32 per literal behind them, come before the
// tokens and come back in that copy as well.  Names get facts as values do;
// the replay reads the values' only.
//
// MetaLayout is that pool for nh Huffman literals, as byte offsets from its
// base (the device's copy, the mapped pool and the host's pool alike):
//   [offsets: nh + 1 uint32, in] [slots: nh + 1 uint32] [status: nh int32]
//   [pad to 8] [numbers: nh int64] [facts: nh uint32]      -- an _http call
//   [tokens: nh int32]                                      -- a tokened call
//   [masks: nh bytes]                                       -- a checked call
// What follows `slots` comes back: the slots in one copy, [status, end) in another.
struct MetaLayout {
  size_t words;  // the bytes of nh + 1 of them: the offsets section, and the slots section
  size_t offsets = 0, slots, status, numbers, facts, tokens, masks, end;
  size_t size;  // of the pool (sized as if the status section, too, had nh + 1 words)
  constexpr MetaLayout(uint32_t nh, Want w)
      : words(((size_t)nh + 1u) * sizeof(uint32_t)),
        slots(words),
        status(2u * words),
        numbers(w.http ? (status + nh * sizeof(int32_t) + 7u) / 8u * 8u : status + nh * sizeof(int32_t)),
        facts(numbers + (w.http ? nh * sizeof(int64_t) : 0u)),
        tokens(facts + (w.http ? nh * sizeof(uint32_t) : 0u)),
        masks(tokens + (w.tokens ? nh * sizeof(int32_t) : 0u)),
        end(masks + (w.checks ? nh : 0u)),
        size(end + sizeof(int32_t)) {}
  template <class T>
  static T *at(void *base, size_t off) {
    return (T *)((uint8_t *)base + off);
  }
};
// (the numbers are read and written as int64: 8-aligned for either parity of nh)
static_assert(MetaLayout(1, Want(false, false, true)).numbers == 24 && MetaLayout(2, Want(false, false, true)).numbers == 32 &&
                  MetaLayout(3, Want(false, false, true)).numbers % 8 == 0 && MetaLayout(3, Want(true, true, false)).masks == 56,
              "the metadata pool's layout");

int stage_decode(Engine &E, uint32_t nblocks, Want want, void *stream, Phases &ph, LitSrc *ls) {
  for (uint32_t i = 0; i < nblocks; ++i) {
    E.nhuff[i + 1] += E.nhuff[i];
    E.hbytes[i + 1] += E.hbytes[i];
  }
  const uint32_t nh = E.nhuff[nblocks];
  const uint64_t hb = E.hbytes[nblocks];
  // uint32 offsets into the batch's literal pool (and uint32 decode slots):
  // a batch past them is refused before any connection state changes
  if (hb > UINT32_MAX || (nh && nghttp2_amd_hd_huff_decode_bound(hb, nh) > UINT32_MAX))
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  if (E.hoff.size() < (size_t)nh + 1) E.hoff.resize((size_t)nh + 1);
  const int mode = zc_mode();
  const bool zero_copy = mode == 1;
  const size_t in_bytes = ((size_t)hb + 15u) / 16u * 16u + 16u;
  const size_t out_bytes = nh ? nghttp2_amd_hd_huff_decode_bound(hb, nh) : 0;
  // (the check reads whole 16-byte chunks up to the last slot's end, and one
  // at it when every literal is empty; the token lookup reads at most one
  // chunk past the chunk a literal ends in)
  const size_t out_alloc = out_bytes + (want.any() ? 16u : 0u);
  const MetaLayout ml(nh, want);
  // (the output pool is a D2H copy target unless the kernel writes it
  // through the mapping, mode 1; the input pools are mapped unless mode 0;
  // mode 2 needs no device copy of the input)
  if (nh && (!E.h_pool.reserve(in_bytes, kLayer, mode != 0) || !E.h_out.reserve(out_alloc, kLayer, zero_copy) ||
             !E.h_meta.reserve(ml.size, kLayer, mode != 0) ||
             (!zero_copy && ((mode == 0 && !E.d_in.reserve(in_bytes, kLayer)) ||
                             !E.d_out.reserve(out_alloc, kLayer) || !E.d_meta.reserve(ml.size, kLayer)))))
    return NGHTTP2_AMD_ERR_NOMEM;
  ph.mark("pools");
  number_and_copy(E, nblocks);
  ph.mark("number+copy");
  *ls = LitSrc{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!nh) return 0;
  hipStream_t st = (hipStream_t)stream;
  void *const h_meta = E.h_meta.p;
  memset(E.h_pool.as<uint8_t>() + hb, 0, in_bytes - hb);
  memcpy(h_meta, E.hoff.data(), ml.words);
  // a failure after the first copy or launch is queued drains the stream
  // before returning: GPU work still in flight must not land in the pinned
  // pools after the next call has filled them
  auto drain = [st](int rv) {
    (void)hipStreamSynchronize(st);
    return rv;
  };
  // the pinned pools as the device sees them: input and offsets unless mode
  // 0, the output in mode 1
  void *m_in = nullptr, *m_out = nullptr, *m_meta = nullptr;
  if (mode != 0 && (hipHostGetDevicePointer(&m_in, E.h_pool.p, 0) != hipSuccess ||
                    (zero_copy && hipHostGetDevicePointer(&m_out, E.h_out.p, 0) != hipSuccess) ||
                    hipHostGetDevicePointer(&m_meta, E.h_meta.p, 0) != hipSuccess))
    return NGHTTP2_AMD_ERR_FATAL;
  const uint8_t *src = mode != 0 ? (const uint8_t *)m_in : E.d_in.as<uint8_t>();
  const uint32_t *src_off = mode != 0 ? (const uint32_t *)m_meta : E.d_meta.as<uint32_t>();
  uint8_t *dst = zero_copy ? (uint8_t *)m_out : E.d_out.as<uint8_t>();
  void *const d_meta = zero_copy ? m_meta : E.d_meta.p;  // where the kernels write
  uint32_t *d_slot = ml.at<uint32_t>(d_meta, ml.slots);
  int32_t *d_st = ml.at<int32_t>(d_meta, ml.status);
  if (mode == 0 && (hipMemcpyAsync(E.d_in.p, E.h_pool.p, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
                    hipMemcpyAsync(E.d_meta.p, h_meta, ml.words, hipMemcpyHostToDevice, st) != hipSuccess))
    return drain(NGHTTP2_AMD_ERR_FATAL);
  int rv = nghttp2_amd_hd_huff_decode_batch_auto(src, src_off, nh, hb, dst, out_bytes, d_slot, d_st, nullptr, nullptr,
                                                 stream);
  if (!rv && want.checks)
    rv = nghttp2_amd_hd_check_fields_batch(dst, d_slot, d_st, nh, ml.at<uint8_t>(d_meta, ml.masks), stream);
  if (!rv && want.tokens)
    rv = nghttp2_amd_hd_name_tokens_len_batch(dst, d_slot, d_st, nh, ml.at<int32_t>(d_meta, ml.tokens), nullptr, stream);
  if (!rv && want.http)
    rv = nghttp2_amd_hd_http_facts_batch(dst, d_slot, d_st, nh, ml.at<uint32_t>(d_meta, ml.facts),
                                         ml.at<int64_t>(d_meta, ml.numbers), stream);
  if (rv) return drain(rv);
  if (!zero_copy &&
      (hipMemcpyAsync(E.h_out.p, dst, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(ml.at<void>(h_meta, ml.slots), d_slot, ml.words, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(ml.at<void>(h_meta, ml.status), d_st, ml.end - ml.status, hipMemcpyDeviceToHost, st) !=
           hipSuccess))
    return drain(NGHTTP2_AMD_ERR_FATAL);
  *ls = LitSrc{E.h_out.as<uint8_t>(),
               ml.at<uint32_t>(h_meta, ml.slots),
               ml.at<int32_t>(h_meta, ml.status),
               want.checks ? ml.at<uint8_t>(h_meta, ml.masks) : nullptr,
               want.tokens ? ml.at<int32_t>(h_meta, ml.tokens) : nullptr,
               want.http ? ml.at<uint32_t>(h_meta, ml.facts) : nullptr,
               want.http ? ml.at<int64_t>(h_meta, ml.numbers) : nullptr};
  return 0;
}

// "group": the batch's blocks per connection, in batch order -- conns, and
// connection c's blocks corder[cstart[c] .. cstart[c + 1]).  A connection is
// numbered at its first block by a stamp in the inflater, no hash lookups.
void group_by_connection(Engine &E, nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks) {
  std::vector<uint32_t> &cstart = E.cstart, &corder = E.corder;
  auto &conns = E.conns;
  conns.clear();
  const uint64_t gen = ++E.gen;
  for (uint32_t i = 0; i < nblocks; ++i) {
    nghttp2_amd_hd_inflater *c = inflaters[i];
    if (c->batch_gen != gen) {
      c->batch_gen = gen;
      c->batch_conn = (uint32_t)conns.size();
      conns.push_back(c);
    }
  }
  cstart.assign(conns.size() + 1, 0);
  corder.resize(nblocks);
  for (uint32_t i = 0; i < nblocks; ++i) ++cstart[inflaters[i]->batch_conn + 1];
  for (size_t c = 0; c < conns.size(); ++c) cstart[c + 1] += cstart[c];
  std::vector<uint32_t> fill(cstart.begin(), cstart.end() - 1);
  for (uint32_t i = 0; i < nblocks; ++i) corder[fill[inflaters[i]->batch_conn]++] = i;
}

// "bound": whether an upper bound of the batch's output (pass 1's per-block
// parts, a dynamic-table reference at dyn_ref_bound) can pass the caller's
// caps.  Only then can the batch be cut, so only then are the tables snapshotted.
bool may_cut(const Engine &E, nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks, const Dest &d) {
  std::vector<uint64_t> run_ln(E.conns.size(), 0), run_lv(E.conns.size(), 0);
  uint64_t nv_bound = 0, ar_bound = 0;
  for (uint32_t i = 0; i < nblocks; ++i) {
    const nghttp2_amd_hd_inflater *c = inflaters[i];
    const Block &b = E.bl[i];
    // (a connection's earlier blocks of the batch insert before this one:
    // their literals count too -- the running maxima)
    const uint32_t cn = c->batch_conn;
    run_ln[cn] = std::max(run_ln[cn], b.lit_name);
    run_lv[cn] = std::max(run_lv[cn], b.lit_val);
    const uint64_t ar_b = block_ar_bound(b, dyn_ref_bound(c, run_ln[cn], run_lv[cn]));
    nv_bound += b.nv;
    ar_bound = sat_add(ar_bound, ar_b);
    if (nv_bound > d.nva_cap || ar_bound > d.arena_cap) return true;
  }
  return false;
}

// One replayed block's fields into the caller's arrays: field nv_base on, bytes at ar_base.
void place_block(const BlockOut &o, uint32_t block, size_t nv_base, size_t ar_base, const FieldOut &fo) {
  if (!o.bytes.empty()) memcpy(fo.arena + ar_base, o.bytes.data(), o.bytes.size());
  for (const Rec &r : o.recs) fo.put(nv_base++, block, (uint32_t)ar_base, r);
}

// "replay direct" -- pass 2 for a batch of one connection (a serial replay
// anyway): fields straight into the caller's arena and array in block order,
// no per-block buffers, no placement pass (round 5: config 1's 1,000 blocks
// of one connection).  A block whose own output bound may pass the caps is
// replayed into a scratch buffer from a copy of the table, and placed if it
// fits, else the table is restored and the batch cut there.
int replay_direct(Engine &E, uint32_t nblocks, const LitSrc &ls, Want want, const Dest &d, void *stream, Phases &ph) {
  if (ls.st && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return NGHTTP2_AMD_ERR_FATAL;
  ph.mark("gpu wait");
  nghttp2_amd_hd_inflater *c = E.conns[0];
  DirectSink ds{d.fo, d.block_status};
  const bool htp = want.http;
  uint32_t cut = nblocks;
  for (uint32_t i = 0; i < nblocks; ++i) {
    const Block &b = E.bl[i];
    // (bounds from the table as it is now: the earlier blocks' inserts are
    // in it, and in max_nl / max_vl)
    const uint64_t ar_b = block_ar_bound(b, dyn_ref_bound(c, b.lit_name, b.lit_val));
    ds.block = i;
    HttpRun hr = htp ? d.run(i) : HttpRun{};
    if (ds.nv + b.nv <= d.nva_cap && ar_b <= d.arena_cap - ds.ar) {
      replay_block(c, b, ls, want, htp ? &hr : nullptr, ds);
      if (htp) d.set_http(i, hr.st, hr.result);
      continue;
    }
    nghttp2_amd_hd_inflater keep = *c;
    BlockOut scratch;
    BlockSink bs{scratch};
    replay_block(c, b, ls, want, htp ? &hr : nullptr, bs);
    if (ds.nv + scratch.recs.size() > d.nva_cap || scratch.bytes.size() > d.arena_cap - ds.ar) {
      *c = std::move(keep);
      cut = i;
      break;
    }
    place_block(scratch, i, ds.nv, ds.ar, d.fo);
    if (htp) d.set_http(i, hr.st, hr.result);
    ds.nv += scratch.recs.size();
    ds.ar += scratch.bytes.size();
    d.block_status[i] = scratch.status;
  }
  for (uint32_t j = cut; j < nblocks; ++j) {
    d.block_status[j] = NGHTTP2_AMD_ERR_BUFFER_ERROR;
    if (d.block_http) d.block_http[j] = NGHTTP2_AMD_ERR_BUFFER_ERROR;  // (its state stays as the caller put it)
  }
  ph.mark("replay direct");
  *d.nva_used = ds.nv;
  *d.arena_used = ds.ar;
  return cut < nblocks ? NGHTTP2_AMD_ERR_BUFFER_ERROR : 0;
}

// "replay", "place" -- pass 2 for several connections: each connection's
// blocks in batch order against its table (one task per connection), fields
// into per-block buffers, then placed in block order.  A batch that outgrows
// the caller's buffers is cut at the first block that does not fit, and the tables
// replayed up to there from snapshots (a copy of every table, if cut_possible).
int replay_grouped(Engine &E, nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks, const LitSrc &ls,
                   Want want, const Dest &d, bool cut_possible, void *stream, Phases &ph) {
  const std::vector<nghttp2_amd_hd_inflater *> &conns = E.conns;
  std::vector<nghttp2_amd_hd_inflater> snap;
  if (cut_possible) {
    snap.reserve(conns.size());
    for (auto *c : conns) snap.push_back(*c);
  }
  if (ls.st && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return NGHTTP2_AMD_ERR_FATAL;
  ph.mark("gpu wait");
  // per-block field buffers, kept across calls (under the engine's lock):
  // replay allocates only while they grow
  std::vector<BlockOut> &outs = E.outs;
  if (outs.size() < nblocks) outs.resize(nblocks);
  const bool htp = want.http;
  parallel_for(conns.size(), 1, [&](size_t c) {
    for (uint32_t j = E.cstart[c]; j < E.cstart[c + 1]; ++j) {
      const uint32_t i = E.corder[j];
      BlockSink bs{outs[i]};
      // (the caller's state is read here and written when the block is placed)
      HttpRun hr = htp ? d.run(i) : HttpRun{};
      replay_block(conns[c], E.bl[i], ls, want, htp ? &hr : nullptr, bs);
      if (htp) outs[i].hst = hr.st, outs[i].hres = hr.result;
    }
  });
  ph.mark("replay");
  std::vector<size_t> nv_base(nblocks + 1, 0), ar_base(nblocks + 1, 0);
  uint32_t cut = nblocks;
  for (uint32_t i = 0; i < nblocks; ++i) {
    nv_base[i + 1] = nv_base[i] + outs[i].recs.size();
    ar_base[i + 1] = ar_base[i] + outs[i].bytes.size();
    if (nv_base[i + 1] > d.nva_cap || ar_base[i + 1] > d.arena_cap) {
      cut = i;
      break;
    }
  }
  if (cut < nblocks && !cut_possible) {
    // the bound missed an output that fits no cap: the tables are past the
    // cut with no snapshot to restore, so the batch fails and its inflaters
    // turn bad (an internal error, never expected)
    for (auto *c : conns) c->bad = true;
    for (uint32_t j = 0; j < nblocks; ++j) d.block_status[j] = NGHTTP2_AMD_ERR_FATAL;
    *d.nva_used = 0;
    *d.arena_used = 0;
    return NGHTTP2_AMD_ERR_FATAL;
  }
  if (cut < nblocks) {  // restore, then re-apply the blocks before the cut
    for (size_t c = 0; c < conns.size(); ++c) *conns[c] = std::move(snap[c]);
    BlockOut scratch;
    BlockSink ss{scratch};
    // (the tables carry the values' facts as the first replay left them in
    // the entries: the states are not written yet, so each block starts from
    // the caller's again)
    for (uint32_t i = 0; i < cut; ++i) {
      HttpRun hr = htp ? d.run(i) : HttpRun{};
      replay_block(inflaters[i], E.bl[i], ls, want, htp ? &hr : nullptr, ss);
    }
    for (uint32_t j = cut; j < nblocks; ++j) {
      d.block_status[j] = NGHTTP2_AMD_ERR_BUFFER_ERROR;
      if (d.block_http) d.block_http[j] = NGHTTP2_AMD_ERR_BUFFER_ERROR;
    }
  }
  parallel_for(cut, 256, [&](size_t i) {
    place_block(outs[i], (uint32_t)i, nv_base[i], ar_base[i], d.fo);
    d.block_status[i] = outs[i].status;
    if (htp) d.set_http((uint32_t)i, outs[i].hst, outs[i].hres);
  });
  ph.mark("place");
  *d.nva_used = nv_base[cut];
  *d.arena_used = ar_base[cut];
  return cut < nblocks ? NGHTTP2_AMD_ERR_BUFFER_ERROR : 0;
}

}  // namespace

extern "C" {

// The prefix integer (RFC 7541 5.1) as nghttp2_hd_decode_length
// (lib/nghttp2_hd.c:882-945): the first byte's low `prefix` bits, then
// 7-bit groups least significant first while the top bit is set; the value
// must stay within uint32 (a group at a shift of 32 or more, or one that
// carries past UINT32_MAX, is -1).  `initial`/`shift` continue a partial
// integer from an earlier call (initial == 0: a fresh one).
ptrdiff_t nghttp2_amd_hd_decode_length(uint32_t *res, size_t *shift_ptr, int *fin, uint32_t initial,
                                       size_t shift, const uint8_t *in, const uint8_t *last,
                                       size_t prefix) {
  const uint8_t *p = in;
  uint32_t v = initial;
  *shift_ptr = 0;
  *fin = 0;
  if (p == last) {  // (nothing to read: the state stays as it was)
    *res = v;
    *shift_ptr = shift;
    return 0;
  }
  if (v == 0) {  // the prefix byte
    const uint32_t mask = (1u << prefix) - 1u;
    const uint32_t low = *p++ & mask;
    if (low < mask) {
      *res = low;
      *fin = 1;
      return 1;
    }
    v = mask;
  }
  for (; p != last; shift += 7) {
    const uint8_t b = *p++;
    const uint32_t grp = b & 0x7Fu;
    if (shift >= 32 || grp > (UINT32_MAX >> shift)) return -1;
    const uint32_t add = grp << shift;
    if (add > UINT32_MAX - v) return -1;
    v += add;
    if (!(b & 0x80u)) {
      *res = v;
      *shift_ptr = shift;
      *fin = 1;
      return p - in;
    }
  }
  *res = v;
  *shift_ptr = shift;
  return p - in;
}

int nghttp2_amd_hd_inflate_new(nghttp2_amd_hd_inflater **inflater_ptr) {
  if (!inflater_ptr) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  *inflater_ptr = new (std::nothrow) nghttp2_amd_hd_inflater();
  return *inflater_ptr ? 0 : NGHTTP2_AMD_ERR_NOMEM;
}

void nghttp2_amd_hd_inflate_del(nghttp2_amd_hd_inflater *inflater) { delete inflater; }

int nghttp2_amd_hd_inflate_change_table_size(nghttp2_amd_hd_inflater *inf,
                                             size_t settings_max_dynamic_table_size) {
  if (!inf) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  if (inf->mid_block) return NGHTTP2_AMD_ERR_INVALID_STATE;  // :1292-1298
  inf->settings_max = settings_max_dynamic_table_size;
  if (inf->bufsize_max > settings_max_dynamic_table_size) {
    inf->expect_size = true;
    inf->min_max = settings_max_dynamic_table_size;
    inf->bufsize_max = settings_max_dynamic_table_size;
    inf->shrink();
  }
  return 0;
}

size_t nghttp2_amd_hd_inflate_get_num_table_entries(nghttp2_amd_hd_inflater *inf) {
  return inf ? inf->max_index() : 0;
}

int nghttp2_amd_hd_inflate_get_table_entry(nghttp2_amd_hd_inflater *inf, size_t idx,
                                           const uint8_t **name, size_t *namelen,
                                           const uint8_t **value, size_t *valuelen) {
  if (!inf || idx == 0 || idx > inf->max_index()) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const char *n, *v;
  inf->entry(idx - 1, &n, namelen, &v, valuelen);
  *name = (const uint8_t *)n;
  *value = (const uint8_t *)v;
  return 0;
}

size_t nghttp2_amd_hd_inflate_get_dynamic_table_size(nghttp2_amd_hd_inflater *inf) {
  return inf ? inf->bufsize : 0;
}

size_t nghttp2_amd_hd_inflate_get_max_dynamic_table_size(nghttp2_amd_hd_inflater *inf) {
  return inf ? inf->bufsize_max : 0;
}

int nghttp2_amd_hd_inflate_blocks(nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks,
                                  const uint8_t *const *blocks, const size_t *block_lens,
                                  nghttp2_amd_hd_nv *nva, size_t nva_cap, size_t *nva_used,
                                  uint8_t *arena, size_t arena_cap, size_t *arena_used,
                                  int32_t *block_status, void *stream) {
  return nghttp2_amd_hd_inflate_blocks_checked(inflaters, nblocks, blocks, block_lens, nva, nva_cap, nva_used,
                                               arena, arena_cap, arena_used, block_status, nullptr, stream);
}

int nghttp2_amd_hd_inflate_blocks_checked(nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks,
                                          const uint8_t *const *blocks, const size_t *block_lens,
                                          nghttp2_amd_hd_nv *nva, size_t nva_cap, size_t *nva_used,
                                          uint8_t *arena, size_t arena_cap, size_t *arena_used,
                                          int32_t *block_status, uint8_t *nv_checks, void *stream) {
  return nghttp2_amd_hd_inflate_blocks_fields(inflaters, nblocks, blocks, block_lens, nva, nva_cap, nva_used, arena,
                                              arena_cap, arena_used, block_status, nv_checks, nullptr, stream);
}

int nghttp2_amd_hd_inflate_blocks_fields(nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks,
                                         const uint8_t *const *blocks, const size_t *block_lens,
                                         nghttp2_amd_hd_nv *nva, size_t nva_cap, size_t *nva_used,
                                         uint8_t *arena, size_t arena_cap, size_t *arena_used,
                                         int32_t *block_status, uint8_t *nv_checks, int32_t *nv_tokens,
                                         void *stream) {
  return nghttp2_amd_hd_inflate_blocks_http(inflaters, nblocks, blocks, block_lens, nva, nva_cap, nva_used, arena,
                                            arena_cap, arena_used, block_status, nv_checks, nv_tokens, nullptr,
                                            nullptr, nullptr, nullptr, stream);
}

int nghttp2_amd_hd_inflate_blocks_http(nghttp2_amd_hd_inflater *const *inflaters, uint32_t nblocks,
                                       const uint8_t *const *blocks, const size_t *block_lens,
                                       nghttp2_amd_hd_nv *nva, size_t nva_cap, size_t *nva_used, uint8_t *arena,
                                       size_t arena_cap, size_t *arena_used, int32_t *block_status,
                                       uint8_t *nv_checks, int32_t *nv_tokens, const uint8_t *block_modes,
                                       nghttp2_amd_hd_http_state *block_state, int32_t *nv_verdicts,
                                       int32_t *block_http, void *stream) {
  if (nva_used) *nva_used = 0;
  if (arena_used) *arena_used = 0;
  if (nblocks == 0) return 0;
  if (!inflaters || !blocks || !block_lens || !block_status || !nva_used || !arena_used)
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < nblocks; ++i)
    if (!inflaters[i] || (!blocks[i] && block_lens[i]) || block_lens[i] > UINT32_MAX)
      return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  // an _http call: the modes and the states are its input, so both are needed
  const bool http = block_modes || block_state || nv_verdicts || block_http;
  if (http && (!block_modes || !block_state)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;

  nghttp2_amd_host::Pool::CallScope scope;  // workers spin between this call's phases only
  Phases ph("inflate");
  std::lock_guard<std::mutex> guard(engine().mu);
  Engine &E = engine();
  const Want want(nv_checks != nullptr, nv_tokens != nullptr, http);
  const Dest dest{{nva, arena, nv_checks, nv_tokens, nv_verdicts}, nva_cap, nva_used, arena_cap, arena_used,
                  block_status, block_modes, block_state, block_http};
  parse_blocks(E, nblocks, blocks, block_lens);
  ph.mark("parse blocks");
  LitSrc ls;
  if (const int rv = stage_decode(E, nblocks, want, stream, ph, &ls)) return rv;
  ph.mark("gpu issued");
  // (the decode runs while the host groups the blocks by connection and
  // bounds the output; replay waits for it)
  group_by_connection(E, inflaters, nblocks);
  ph.mark("group");
  const bool cut_possible = may_cut(E, inflaters, nblocks, dest);
  ph.mark("bound");
  if (E.conns.size() == 1) return replay_direct(E, nblocks, ls, want, dest, stream, ph);
  return replay_grouped(E, inflaters, nblocks, ls, want, dest, cut_possible, stream, ph);
}

}  // extern "C"
