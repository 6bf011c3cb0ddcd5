// replay_sanitize.cpp -- the replay's walk (csrc/hd_replay.h) over generated
// records, for a run under AddressSanitizer + UndefinedBehaviorSanitizer on
// the CPU.  A stand-alone program: it includes the header, links nothing of
// the library and makes no GPU call.
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I nghttp2_amd/csrc -o replay_sanitize tests/c/replay_sanitize.cpp && ./replay_sanitize [rounds] [seed]
//
// Every round builds one connection (a small ring, so it wraps and fills),
// commits what the walk leaves with the host twin's commit
// (hdreplay::commit_host) over stores of exactly the bytes a reference may
// name, reads the ring out (hdreplay::ring_entries), and checks that every
// reference handed out lies inside its store and that the accounted size is
// the entries' sum.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hd_replay.h"

using namespace hdreplay;

static uint64_t rng_state = 1;
static uint32_t rnd(uint32_t n) {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 2685821657736338717ull) >> 33) % n;
}

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "replay_sanitize: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) | 1u : 1u;
  const uint32_t tb = 4096, slots = tb / kOverhead, wire_bytes = 1u << 12, nlits = 64;
  const uint32_t pool_bytes = (1u << 16) + 2000u;  // (the furthest a decoded literal below can end)
  uint64_t fields = 0, fails = 0, nomem = 0;
  for (int round = 0; round < rounds; ++round) {
    Conn h;
    conn_init(&h);
    std::vector<Entry> ring(slots), fresh(slots);
    std::vector<uint8_t> wire(wire_bytes, 'w'), pool(pool_bytes, 'p'), store(2 * tb);
    std::vector<uint32_t> entries(4 * slots);
    std::vector<uint32_t> dst_off(nlits);
    std::vector<int32_t> status(nlits);
    for (uint32_t k = 0; k < nlits; ++k) {
      dst_off[k] = rnd(1u << 16);
      status[k] = rnd(64) ? (int32_t)rnd(k % 7 ? 90 : 2000) : NGHTTP2_AMD_ERR_HEADER_COMP;
    }
    const Lits lits = {dst_off.data(), status.data(), nlits};
    uint32_t cur = 0;
    for (int call = 0; call < 6; ++call) {
      if (rnd(3) == 0) {
        const uint32_t v = rnd(4) ? rnd(2 * tb) : UINT32_MAX;
        const int rv = change_table_size(&h, ring.data(), tb, v);
        CHECK(rv == 0 || (rv == NGHTTP2_AMD_ERR_INVALID_STATE && (h.flags & kMidBlock)));
      }
      Table t;
      table_open(&t, h, ring.data(), fresh.data(), tb, cur * tb);
      for (uint32_t b = 0, nb = 1 + rnd(4); b < nb; ++b) {
        std::vector<nghttp2_amd_hd_op> ops(rnd(24));
        for (auto &op : ops) {
          const bool first = &op == ops.data();
          op = nghttp2_amd_hd_op{};
          op.name_lit = op.value_lit = -1;
          const uint32_t kind = first ? rnd(4) : 1 + rnd(11);
          if (kind == 0 || (!first && rnd(300) == 0)) {
            op.kind = NGHTTP2_AMD_HD_OP_SIZE;
            op.value = rnd(8) ? rnd(t.h.settings_max < t.h.min_max ? t.h.settings_max | 1u : t.h.min_max | 1u) : rnd(1u << 20);
          } else if (kind < 5) {
            op.kind = NGHTTP2_AMD_HD_OP_INDEXED;
            op.value = rnd(100) ? 1 + rnd(61 + t.h.count) : rnd(2) ? 0u : 62 + t.h.count + rnd(3);
          } else {
            op.kind = NGHTTP2_AMD_HD_OP_LITERAL;
            uint32_t fl = (rnd(2) ? NGHTTP2_AMD_HD_OP_INDEX_REQUIRED : rnd(2) ? NGHTTP2_AMD_HD_OP_NO_INDEX : 0u);
            if (rnd(2)) {
              fl |= NGHTTP2_AMD_HD_OP_NEW_NAME;
              op.name_len = rnd(40);
              op.name_off = rnd(wire_bytes - op.name_len);
              if (rnd(2)) {
                fl |= NGHTTP2_AMD_HD_OP_NAME_HUFF;
                op.name_lit = (int32_t)(rnd(100) ? rnd(nlits) : nlits + rnd(2));  // (rarely past the decode's)
              }
            } else {
              op.value = rnd(100) ? 1 + rnd(61 + t.h.count) : 62 + t.h.count;
            }
            op.value_len = rnd(8) ? rnd(120) : rnd(1500);
            op.value_off = rnd(wire_bytes - op.value_len);
            if (rnd(2)) {
              fl |= NGHTTP2_AMD_HD_OP_VALUE_HUFF;
              op.value_lit = (int32_t)rnd(nlits);
            }
            op.flags = (uint8_t)fl;
          }
        }
        std::vector<FieldRef> fref(ops.size() + 1);
        FieldRef *out = fref.data();
        const bool bad_before = (t.h.flags & kBad) != 0;
        const BlockResult r = walk_block(&t, b, ops.data(), (uint32_t)ops.size(), rnd(50) != 0, rnd(4) == 0, lits,
                                         &hdhost::kStaticPool, [out](uint32_t k, const FieldRef &fr) { out[k] = fr; });
        CHECK(r.status == (int32_t)r.fields || r.status == NGHTTP2_AMD_ERR_HEADER_COMP ||
              r.status == NGHTTP2_AMD_ERR_NOMEM);
        CHECK(!bad_before || (r.status == NGHTTP2_AMD_ERR_HEADER_COMP && r.fields == 0));
        CHECK((r.status < 0) == ((t.h.flags & kBad) != 0));
        uint32_t seen = 0, bytes = 0;
        for (size_t k = 0; k < ops.size(); ++k) {
          if (fref[k].block == kNoField) continue;
          CHECK(fref[k].block == b && fref[k].ordinal == seen && fref[k].before == bytes);
          for (const Ref x : {fref[k].name, fref[k].value}) {
            const uint64_t end = (uint64_t)x.off + ref_len(x);
            const uint32_t src = ref_src(x);
            CHECK(src <= SRC_TABLE);
            CHECK(src != SRC_STATIC || end <= hdhost::kStaticPoolBytes);
            CHECK(src != SRC_WIRE || end <= wire_bytes);
            CHECK(src != SRC_TABLE || (x.off >= cur * tb && end <= (cur + 1) * tb));
          }
          ++seen;
          bytes += ref_len(fref[k].name) + ref_len(fref[k].value) + 2u;
        }
        CHECK(seen == r.fields && bytes == r.bytes);
        fields += r.fields;
        fails += r.status == NGHTTP2_AMD_ERR_HEADER_COMP;
        nomem += r.status == NGHTTP2_AMD_ERR_NOMEM;
        CHECK(t.h.count == t.nnew + t.nold && t.h.count <= slots && t.h.size <= tb);
        CHECK(t.h.size <= t.h.max || t.h.count == 0);
      }
      // the host twin's commit: the entries' bytes back to back in the other buffer
      const uint8_t *stores[4] = {hdhost::kStaticPool.bytes, wire.data(), pool.data(), store.data()};
      h = commit_host(t, ring.data(), store.data(), tb, [&](Ref r) { return stores[ref_src(r)] + r.off; });
      CHECK(h.count == t.nnew + t.nold && h.head == ((t.h.head - t.nnew) & t.mask) && h.cur == (cur ^ 1u));
      cur = h.cur;
      CHECK(ring_entries(h, ring.data(), slots, entries.data()));
      uint32_t at = 0, size = 0;
      for (uint32_t i = 0; i < h.count; ++i) {
        const uint32_t nl = entries[4 * i + 1], vl = entries[4 * i + 3];
        CHECK(entries[4 * i] == at && entries[4 * i + 2] == at + nl);
        at += nl + vl;
        size += nl + vl + kOverhead;
      }
      CHECK(at <= tb && size == t.h.size);
    }
  }
  printf("replay_sanitize: ok (%d rounds, %llu fields, %llu failed blocks, %llu NOMEM)\n", rounds,
         (unsigned long long)fields, (unsigned long long)fails, (unsigned long long)nomem);
  return 0;
}
