// hd_parse.h -- the representation layer of an HPACK header block, stated once.
//
// A header block is a run of representations (RFC 7541 6): dynamic table size
// updates, indexed fields, and literal fields whose name is an index or a
// string literal and whose value is a string literal.  Each one delimits
// itself -- an opcode byte, prefix integers, string literals with their
// lengths -- so a block is cut into representations without any table state.
// walk() is that cut: nghttp2_hd_inflate_hd_nv's opcode dispatch
// (lib/nghttp2_hd.c:1942-1985) and decode_length (:882-945, with in_final: an
// integer the block end cuts off fails), restated over a byte pointer and a
// length.  What the representations mean -- index resolution, insertion,
// eviction, the size update rules -- stays with the replay.
//
// One walk serves counting and writing: the sink receives every completed
// representation as an nghttp2_amd_hd_op, and the counts come out of the same
// statements whether the sink stores the record or drops it, so a count pass
// and a write pass over the same bytes cannot disagree.
//
// Shared by the host function (nghttp2_amd_hd_parse_block), pass 1 of the host
// inflater (hd_inflate.cpp: parse_blocks) and the GPU kernels (k_parse_blocks,
// one lane per block); both replays (hd_replay.h: walk_block, hd_inflate.cpp:
// replay_block) read the record's string literals through literal() below.
// Plain C++17, no HIP: included by .cpp and .hip sources alike.  No table, no
// array: on the device the walk keeps its state in registers.
#ifndef NGHTTP2_AMD_HD_PARSE_H
#define NGHTTP2_AMD_HD_PARSE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"

#if defined(__HIPCC__)
#define HDPARSE_FN __host__ __device__ inline
#else
#define HDPARSE_FN inline
#endif

namespace hdparse {

static_assert(sizeof(nghttp2_amd_hd_op) == 32, "the record's layout is part of the ABI");

constexpr uint32_t kMaxNv = 65536;  // NGHTTP2_HD_MAX_NV

// The prefix integer (RFC 7541 5.1) at in[*pos] of a block of len bytes, by
// the rules of nghttp2_amd_hd_decode_length: a group at a shift of 32 or
// more, or one that carries the value past UINT32_MAX, fails, and so does an
// integer the block end cuts off.  The groups that can pass sit at shifts 0,
// 7, .. 28, so an integer is at most six bytes and the loop at most five
// rounds.  On success *pos is past the integer.
// Every parser of a whole block reads its integers here, the host inflater
// included.  nghttp2_amd_hd_decode_length (hd_inflate.cpp) is the other
// statement of the integer: public, and resumable across input chunks, which
// a walk on the device has no use for.  tests/test_parse_blocks.py
// (test_read_int_agrees_with_decode_length) holds the two to each other.
HDPARSE_FN bool read_int(const uint8_t *in, uint32_t len, uint32_t *pos, uint32_t prefix, uint32_t *out) {
  uint32_t p = *pos;
  if (p >= len) return false;
  const uint32_t mask = (1u << prefix) - 1u;
  uint32_t v = in[p++] & mask;
  if (v == mask) {
    bool fin = false;
    for (uint32_t shift = 0; shift < 32u; shift += 7u) {
      if (p >= len) return false;
      const uint32_t b = in[p++];
      const uint32_t grp = b & 0x7Fu;
      if (grp > (UINT32_MAX >> shift)) return false;
      const uint32_t add = grp << shift;
      if (add > UINT32_MAX - v) return false;
      v += add;
      if (!(b & 0x80u)) {
        fin = true;
        break;
      }
    }
    // (a sixth group would sit at shift 35: refused whether it is there or
    // the block ends first)
    if (!fin) return false;
  }
  *pos = p;
  *out = v;
  return true;
}

// A string literal at in[*pos]: the H bit, a 7-bit-prefix length of at most
// NGHTTP2_HD_MAX_NV that the block's remaining bytes cover, then the bytes
// [*off, *off + *n).
HDPARSE_FN bool read_lit(const uint8_t *in, uint32_t len, uint32_t *pos, uint32_t *off, uint32_t *n, bool *huff) {
  if (*pos >= len) return false;
  *huff = (in[*pos] & 0x80u) != 0;
  if (!read_int(in, len, pos, 7, n) || *n > kMaxNv || len - *pos < *n) return false;
  *off = *pos;
  *pos += *n;
  return true;
}

// Byte b0 opens a dynamic table size update (001xxxxx).
HDPARSE_FN bool is_size_update(uint32_t b0) { return (b0 & 0xE0u) == 0x20u; }
// The first byte of the block in[0, len) opens one.  Which state a failed
// block leaves its inflater in depends on it (the replays' first_is_size).
HDPARSE_FN bool first_is_size(const uint8_t *in, uint32_t len) { return len > 0u && is_size_update(in[0]); }

// A record's name (which = 0) or value (which = 1) string literal: where its
// bytes are and how many, whether they are Huffman-coded, and then its number
// among the Huffman literals (else -1).  The one decoding of the record's
// flag bits and literal fields; without NEW_NAME a LITERAL's name is {0, 0,
// false, -1}.
struct Literal {
  uint32_t off, len;
  bool huff;
  int32_t lit;
};
HDPARSE_FN Literal literal(const nghttp2_amd_hd_op &op, int which) {
  if (which) return Literal{op.value_off, op.value_len, (op.flags & NGHTTP2_AMD_HD_OP_VALUE_HUFF) != 0, op.value_lit};
  return Literal{op.name_off, op.name_len, (op.flags & NGHTTP2_AMD_HD_OP_NAME_HUFF) != 0, op.name_lit};
}

// What a block holds: its completed representations, the Huffman literals
// among their string literals and those literals' encoded bytes; ok is false
// when the bytes after the last completed representation are no
// representation (the counts then cover what came before, which the replay
// still emits).
struct Counts {
  uint32_t ops, lits, lit_bytes;
  bool ok;
};

// A sink that drops the records: the count pass.
struct NoSink {
  HDPARSE_FN void operator()(uint32_t, const nghttp2_amd_hd_op &) const {}
};

// The block in[0, len).  sink(k, op) receives the k-th completed
// representation; its offsets are positions in the block plus base (the
// block's place in a wire pool), its Huffman literals are numbered from lit0
// in wire order, a name before its value.
template <class Sink>
HDPARSE_FN Counts walk(const uint8_t *in, uint32_t base, uint32_t len, uint32_t lit0, Sink &&sink) {
  Counts c = {0u, 0u, 0u, false};
  uint32_t pos = 0;
  for (;;) {  // (every round consumes at least the opcode byte; a break is a failure)
    if (pos >= len) {
      c.ok = true;
      break;
    }
    nghttp2_amd_hd_op op = {};
    op.name_lit = op.value_lit = -1;
    const uint32_t b0 = in[pos];
    uint32_t lits = 0, lit_bytes = 0;
    if (is_size_update(b0)) {  // dynamic table size update
      op.kind = NGHTTP2_AMD_HD_OP_SIZE;
      if (!read_int(in, len, &pos, 5, &op.value)) break;
    } else if (b0 & 0x80u) {  // indexed
      op.kind = NGHTTP2_AMD_HD_OP_INDEXED;
      if (!read_int(in, len, &pos, 7, &op.value)) break;
    } else {
      op.kind = NGHTTP2_AMD_HD_OP_LITERAL;
      const bool indexing = (b0 & 0x40u) != 0;
      uint32_t fl = (indexing ? NGHTTP2_AMD_HD_OP_INDEX_REQUIRED : 0u) |
                    ((b0 & 0xF0u) == 0x10u ? NGHTTP2_AMD_HD_OP_NO_INDEX : 0u);
      uint32_t off, n;
      bool huff;
      if (b0 == 0x40u || b0 == 0x00u || b0 == 0x10u) {  // a new name
        fl |= NGHTTP2_AMD_HD_OP_NEW_NAME;
        ++pos;
        if (!read_lit(in, len, &pos, &off, &n, &huff)) break;
        op.name_off = base + off;
        op.name_len = n;
        if (huff) {
          fl |= NGHTTP2_AMD_HD_OP_NAME_HUFF;
          op.name_lit = (int32_t)(lit0 + c.lits + lits);
          ++lits;
          lit_bytes += n;
        }
      } else if (!read_int(in, len, &pos, indexing ? 6u : 4u, &op.value)) {
        break;
      }
      if (!read_lit(in, len, &pos, &off, &n, &huff)) break;
      op.value_off = base + off;
      op.value_len = n;
      if (huff) {
        fl |= NGHTTP2_AMD_HD_OP_VALUE_HUFF;
        op.value_lit = (int32_t)(lit0 + c.lits + lits);
        ++lits;
        lit_bytes += n;
      }
      op.flags = (uint8_t)fl;
    }
    sink(c.ops, op);
    ++c.ops;
    c.lits += lits;
    c.lit_bytes += lit_bytes;
  }
  return c;
}

}  // namespace hdparse

#endif  // NGHTTP2_AMD_HD_PARSE_H
