// deflate_plan_sanitize.cpp -- the deflaters' field step (csrc/hd_deflate_plan.h)
// over generated fields, for a run under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU.  A stand-alone program: it includes
// the header, links nothing of the library and makes no GPU call.
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I nghttp2_amd/csrc -o deflate_plan_sanitize tests/c/deflate_plan_sanitize.cpp && \
//       ./deflate_plan_sanitize [rounds] [seed]
//
// Every round builds one connection, walks calls of several blocks over an
// arena of exactly the fields' bytes (so a read past a string is a read past
// the allocation), commits what the walk leaves with the host twin's commit
// (hdreplay::commit_host), and checks the table, read out with
// hdreplay::ring_entries, against a model kept beside it: a deque of strings
// with the reference's insertion and eviction, searched by plain comparison.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "hd_deflate_plan.h"

using namespace hdplan;

static uint64_t rng_state = 1;
static uint32_t rnd(uint32_t n) {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 2685821657736338717ull) >> 33) % n;
}

#define CHECK(c)                                                                         \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      fprintf(stderr, "deflate_plan_sanitize: %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

typedef std::pair<std::string, std::string> NV;

static const char *const kNames[] = {":method", ":path", ":status", "cookie", "authorization", "set-cookie",
                                     "accept-encoding", "x-a", "x-b", "", "te", "x-some-longer-name"};

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) | 1u : 1u;
  const uint32_t tb = 4096, slots = tb / hdreplay::kOverhead, mask = slots - 1u;
  uint64_t fields = 0, indexed = 0, inserted = 0;
  for (int round = 0; round < rounds; ++round) {
    Conn h;
    const uint32_t deflate_max = rnd(4) ? 4096u : rnd(4097);
    conn_init(&h, deflate_max);
    std::vector<Entry> ring(slots), fresh(slots);
    std::vector<uint32_t> keys(slots), fresh_key(slots);
    std::vector<uint8_t> store(2 * tb);
    std::vector<uint32_t> entries(4 * slots);
    std::deque<NV> model;
    uint32_t model_size = 0;
    for (int call = 0; call < 6; ++call) {
      if (rnd(3) == 0) {
        hdplan::change_table_size(&h, ring.data(), tb, rnd(4) ? rnd(2 * tb) : UINT32_MAX);
        CHECK(h.max <= deflate_max && (h.flags & kNotify));
        while (model_size > h.max && !model.empty()) {
          model_size -= (uint32_t)(model.back().first.size() + model.back().second.size()) + 32u;
          model.pop_back();
        }
        CHECK(model.size() == h.count && model_size == h.size);
      }
      // the call's fields: an arena of exactly their bytes
      const uint32_t nb = 1 + rnd(3);
      std::vector<std::vector<NV>> lists(nb);
      std::vector<uint8_t> arena;
      std::vector<Field> fs;
      for (auto &l : lists)
        for (uint32_t k = 0, nk = rnd(12); k < nk; ++k) {
          NV nv(kNames[rnd(sizeof kNames / sizeof *kNames)], std::string());
          const uint32_t vl = rnd(8) ? rnd(6) : rnd(8) ? rnd(200) : rnd(5000);
          for (uint32_t i = 0; i < vl; ++i) nv.second.push_back((char)('a' + rnd(vl < 6 ? 2 : 26)));
          Field f = {};
          f.name_off = (uint32_t)arena.size();
          f.name_len = (uint32_t)nv.first.size();
          arena.insert(arena.end(), nv.first.begin(), nv.first.end());
          f.value_off = (uint32_t)arena.size();
          f.value_len = (uint32_t)nv.second.size();
          arena.insert(arena.end(), nv.second.begin(), nv.second.end());
          f.flags = rnd(10) == 0;
          fs.push_back(f);
          l.push_back(nv);
        }
      if (arena.empty()) arena.push_back(0);  // (a pointer to form offsets from)
      Table t;
      hdreplay::table_open(&t, h, ring.data(), fresh.data(), tb, (h.cur & 1u) * tb);
      const Keys k = {keys.data(), fresh_key.data()};
      const Bytes by = {store.data(), arena.data()};
      uint32_t at_field = 0;
      for (uint32_t b = 0; b < nb; ++b) {
        const bool notify = (t.h.flags & kNotify) != 0;
        const Head hd = plan_head(&t.h);
        CHECK(head_bytes(hd) <= 12u && (head_bytes(hd) != 0u) == notify && !(t.h.flags & kNotify));
        for (const NV &nv : lists[b]) {
          Field f = fs[at_field++];
          f.hash = name_hash(arena.data() + f.name_off, f.name_len);
          f.token = lookup_token_in(&hdtok::kTable, arena.data() + f.name_off, f.name_len, f.hash);
          // the model's search: the newest exact match, else the newest name match
          int64_t want_idx = -1;
          bool want_exact = false;
          const Mode mode = decide_indexing(f.token, f.name_len, f.value_len, f.flags, t.h.max);
          for (size_t i = 0; i < model.size(); ++i) {
            if (model[i].first != nv.first) continue;
            if (want_idx < 0) {
              want_idx = (int64_t)i;
              if (mode == NEVER_INDEXING) break;
            }
            if (model[i].second == nv.second) {
              want_idx = (int64_t)i;
              want_exact = true;
              break;
            }
          }
          const Match m = search_serial(t, k, by, f, mode == NEVER_INDEXING);
          CHECK(m.found == (want_idx >= 0) && m.exact == want_exact && (!m.found || m.idx == (uint32_t)want_idx));
          const uint64_t w = plan_field(&t, k, by, &hdhost::kStaticPool, f,
                                        [&by](const Table &tt, const Keys &kk, const Field &ff, bool name_only) {
                                          return search_serial(tt, kk, by, ff, name_only);
                                        });
          const uint32_t nbytes = (uint32_t)(w >> 48) & 0xFFu, lits = (uint32_t)(w >> 56), first = (uint32_t)w & 0xFFu;
          CHECK(nbytes >= 1u && nbytes <= 6u && lits <= 3u && lits != 1u);
          CHECK((first & 0x80u) ? lits == 0u : (lits & kLitValue) != 0u);
          ++fields;
          indexed += (first & 0x80u) != 0;
          if (!(first & 0x80u) && (first & 0x40u)) {  // with indexing: the model's add_hd_table_incremental
            const uint32_t room = f.name_len + f.value_len + 32u;
            while (model_size + room > t.h.max && !model.empty()) {
              model_size -= (uint32_t)(model.back().first.size() + model.back().second.size()) + 32u;
              model.pop_back();
            }
            if (room <= t.h.max) {
              model.push_front(nv);
              model_size += room;
              ++inserted;
            }
          }
          CHECK(t.h.count == t.nnew + t.nold && t.h.count == model.size() && t.h.size == model_size);
          CHECK(t.h.size <= t.h.max && t.h.count <= slots);
        }
      }
      // the host twin's commit (the model's bytes fit the buffer it writes)
      uint32_t model_bytes = 0;
      for (const NV &nv : model) model_bytes += (uint32_t)(nv.first.size() + nv.second.size());
      CHECK(model_bytes <= tb);
      h = hdreplay::commit_host(t, ring.data(), store.data(), tb, [&by](Ref r) { return ref_ptr(by, r); }, keys.data(),
                                fresh_key.data());
      // the committed table is the model, entry for entry, with its keys
      CHECK(h.count == model.size() && hdreplay::ring_entries(h, ring.data(), slots, entries.data()));
      for (uint32_t i = 0; i < h.count; ++i) {
        const uint32_t *e = &entries[4 * i];
        const uint8_t *base = store.data() + (size_t)h.cur * tb;
        CHECK(std::string((const char *)base + e[0], e[1]) == model[i].first);
        CHECK(std::string((const char *)base + e[2], e[3]) == model[i].second);
        CHECK(keys[(h.head + i) & mask] == name_hash((const uint8_t *)model[i].first.data(), (uint32_t)model[i].first.size()));
      }
    }
  }
  printf("deflate_plan_sanitize: ok (%d rounds, %llu fields, %llu indexed, %llu inserted)\n", rounds,
         (unsigned long long)fields, (unsigned long long)indexed, (unsigned long long)inserted);
  return 0;
}
