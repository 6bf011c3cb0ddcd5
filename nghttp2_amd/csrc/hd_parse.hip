// hd_parse.hip -- header blocks into representations and Huffman literals, for gfx950.
//
// Reference: the representation layer of nghttp2_hd_inflate_hd_nv
// (lib/nghttp2_hd.c:1942-1985 opcode dispatch, decode_length :882-945, the
// string literal's H bit and length), which needs no table state: every block
// of a batch is cut into its representations on its own (hd_parse.h, the one
// statement of the walk, shared with the host function below).
//
// nghttp2_amd_hd_parse_blocks_batch, three launches:
//   k_parse_blocks<false>  one lane per block, 64 consecutive blocks per wave:
//                          the lane walks its block serially and leaves the
//                          block's representations, Huffman literals and
//                          Huffman bytes in op_off[i], lit_base[i] and the
//                          workspace.  The walk's loads are single bytes at
//                          per-lane addresses, divergent by nature; its loops
//                          are bounded by the block's length (an integer by
//                          six bytes).  No LDS, no table, no scratch.
//   k_parse_scan           one workgroup: the three counts become exclusive
//                          uint32 prefixes in place (64-bit sums, so a total
//                          past the offsets is seen, not wrapped), totals[].
//   k_parse_blocks<true>   the same walk, storing each record at
//                          ops[op_off[i] + k] when that is below ops_cap.
// nghttp2_amd_hd_gather_literals_batch, three launches:
//   k_lit_lens             a lane per record: lit_off[k] = the encoded length
//                          of Huffman literal k;
//   k_lit_scan             one workgroup: lit_off becomes the literals' pool
//                          offsets (back to back), lit_off[T] the pool's end;
//   k_gather               a wave per 64 consecutive records: the records'
//                          Huffman literals one after the other, the wave's
//                          lanes on consecutive bytes of the literal
//                          (coalesced for header-sized strings).
// Both read their counts from totals[] on the device, so parse, gather and the
// decode's launch follow each other on a stream with no host round trip but
// the decode's own n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_host.h"
#include "hd_parse.h"
#include "hd_scan.h"

namespace {

using hdscan::SC_WG;
using hdscan::Share;
using hdscan::scan_sums;
using hdscan::scan_write;

constexpr uint32_t PB_WG = 64;    // k_parse_blocks: one wave, 64 blocks (latency bound: many small workgroups)
constexpr uint32_t GL_WG = 256;   // k_lit_lens, k_gather

// a record into ops[base + k], when that is a place below cap
struct OpStore {
  nghttp2_amd_hd_op *ops;
  uint32_t base, cap;
  __host__ __device__ void operator()(uint32_t k, const nghttp2_amd_hd_op &op) const {
    const uint32_t idx = base + k;
    if (idx >= base && idx < cap) ops[idx] = op;
  }
};

template <bool WRITE>
__global__ __launch_bounds__(PB_WG) void k_parse_blocks(const uint8_t *__restrict__ wire,
                                                        const uint32_t *__restrict__ block_off, uint32_t n,
                                                        uint32_t *__restrict__ op_off,
                                                        nghttp2_amd_hd_op *__restrict__ ops, uint32_t ops_cap,
                                                        int32_t *__restrict__ block_status,
                                                        uint32_t *__restrict__ lit_base,
                                                        uint32_t *__restrict__ byte_base,
                                                        const uint32_t *__restrict__ totals) {
  const uint32_t i = blockIdx.x * PB_WG + threadIdx.x;
  if (i >= n) return;
  if (WRITE && (totals[3] & NGHTTP2_AMD_HD_PARSE_OVERFLOW_U32)) return;  // the offsets are not valid
  // a block that is not examined is empty here and reads nothing
  const uint32_t o0 = block_off[i], o1 = block_off[i + 1];
  const bool valid = o0 <= o1;
  const uint32_t len = valid ? o1 - o0 : 0u;
  const uint8_t *in = wire + o0;
  if (WRITE) {
    const hdparse::Counts c = hdparse::walk(in, o0, len, lit_base[i], OpStore{ops, op_off[i], ops_cap});
    block_status[i] = valid && c.ok ? (int32_t)c.ops : NGHTTP2_AMD_ERR_HEADER_COMP;
  } else {
    const hdparse::Counts c = hdparse::walk(in, o0, len, 0u, hdparse::NoSink{});
    op_off[i] = c.ops;
    lit_base[i] = c.lits;
    byte_base[i] = c.lit_bytes;
  }
}

__global__ __launch_bounds__(SC_WG) void k_parse_scan(uint32_t *__restrict__ op_off, uint32_t *__restrict__ lit_base,
                                                      uint32_t *__restrict__ byte_base, uint32_t n, uint32_t ops_cap,
                                                      uint32_t *__restrict__ totals) {
  __shared__ uint64_t wsum[3][SC_WG / 64];
  Share s0, s1, s2;
  const uint64_t t0 = scan_sums(op_off, n, wsum[0], &s0);
  const uint64_t t1 = scan_sums(lit_base, n, wsum[1], &s1);
  const uint64_t t2 = scan_sums(byte_base, n, wsum[2], &s2);
  const bool wide = ((t0 | t1 | t2) >> 32) != 0;
  if (!wide) {
    scan_write(op_off, op_off, n, s0, t0);
    scan_write(lit_base, lit_base, n, s1, t1);
    scan_write(byte_base, byte_base, n, s2, t2);
  }
  if (threadIdx.x == 0) {
    totals[0] = wide ? 0xFFFFFFFFu : (uint32_t)t0;
    totals[1] = wide ? 0xFFFFFFFFu : (uint32_t)t1;
    totals[2] = wide ? 0xFFFFFFFFu : (uint32_t)t2;
    totals[3] = (wide ? NGHTTP2_AMD_HD_PARSE_OVERFLOW_U32 : 0u) |
                (t0 > ops_cap ? NGHTTP2_AMD_HD_PARSE_OVERFLOW_OPS : 0u);
  }
}

__global__ __launch_bounds__(GL_WG) void k_lit_lens(const nghttp2_amd_hd_op *__restrict__ ops, uint32_t ops_cap,
                                                    const uint32_t *__restrict__ totals,
                                                    uint32_t *__restrict__ lit_off, uint32_t lits_cap) {
  if (totals[3]) return;
  const uint32_t nops = min(totals[0], ops_cap), T = totals[1];
  const uint32_t j = blockIdx.x * GL_WG + threadIdx.x;
  if (T > lits_cap || j >= nops) return;
  const nghttp2_amd_hd_op op = ops[j];
  if ((op.flags & NGHTTP2_AMD_HD_OP_NAME_HUFF) && (uint32_t)op.name_lit < T) lit_off[(uint32_t)op.name_lit] = op.name_len;
  if ((op.flags & NGHTTP2_AMD_HD_OP_VALUE_HUFF) && (uint32_t)op.value_lit < T)
    lit_off[(uint32_t)op.value_lit] = op.value_len;
}

__global__ __launch_bounds__(SC_WG) void k_lit_scan(uint32_t *__restrict__ totals, uint32_t *__restrict__ lit_off,
                                                    uint32_t lits_cap, uint64_t pool_cap) {
  __shared__ uint64_t wsum[SC_WG / 64];
  // (every thread reads the flags here; thread 0 stores them only behind
  // scan_sums' barrier or on a path all threads leave together)
  if (totals[3]) return;
  const uint32_t T = totals[1];
  if (T > lits_cap) {
    if (threadIdx.x == 0) totals[3] = NGHTTP2_AMD_HD_PARSE_OVERFLOW_LITS;
    return;
  }
  Share sh;
  const uint64_t P = scan_sums(lit_off, T, wsum, &sh);
  if (P >> 32) {
    if (threadIdx.x == 0) totals[3] = NGHTTP2_AMD_HD_PARSE_OVERFLOW_U32;
    return;
  }
  scan_write(lit_off, lit_off, T, sh, P);
  if (threadIdx.x == 0 && P > pool_cap) totals[3] = NGHTTP2_AMD_HD_PARSE_OVERFLOW_POOL;
}

__global__ __launch_bounds__(GL_WG) void k_gather(const uint8_t *__restrict__ wire, uint64_t wire_bytes,
                                                  const nghttp2_amd_hd_op *__restrict__ ops, uint32_t ops_cap,
                                                  const uint32_t *__restrict__ totals,
                                                  const uint32_t *__restrict__ lit_off, uint8_t *__restrict__ pool,
                                                  uint64_t pool_cap) {
  if (totals[3]) return;
  const uint32_t nops = min(totals[0], ops_cap), T = totals[1];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t0 = (blockIdx.x * (GL_WG / 64u) + (threadIdx.x >> 6)) * 64u;  // the wave's records
  if (t0 >= nops) return;
  nghttp2_amd_hd_op op = {};
  if (t0 + lane < nops) op = ops[t0 + lane];
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const bool huff = (op.flags & (which ? NGHTTP2_AMD_HD_OP_VALUE_HUFF : NGHTTP2_AMD_HD_OP_NAME_HUFF)) != 0;
    const uint32_t k = (uint32_t)(which ? op.value_lit : op.name_lit);
    const uint32_t src = which ? op.value_off : op.name_off, len = which ? op.value_len : op.name_len;
    uint32_t dst = 0;
    bool has = huff && k < T && len > 0u && (uint64_t)src + len <= wire_bytes;
    if (has) {
      dst = lit_off[k];
      has = (uint64_t)dst + len <= pool_cap;
    }
    uint64_t m = __ballot(has);
    while (m) {  // one literal at a time, the lanes on consecutive bytes
      const int l = __builtin_ctzll(m);
      m &= m - 1ull;
      const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)src, l);
      const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)dst, l);
      const uint32_t nb = (uint32_t)__builtin_amdgcn_readlane((int)len, l);
      for (uint32_t b = lane; b < nb; b += 64u) pool[(size_t)d + b] = wire[(size_t)s + b];
    }
  }
}

size_t ws_need(uint32_t n) {  // the workspace is byte_base[n + 1]
  hdhost::Carve c{nullptr};
  c.take<uint32_t>((size_t)n + 1u);
  return c.total();
}
using hdhost::clamp32;

}  // namespace

extern "C" {

int nghttp2_amd_hd_parse_block(const uint8_t *in, size_t len, nghttp2_amd_hd_op *ops, size_t ops_cap,
                               size_t *nops) {
  if (!nops || (!in && len) || (!ops && ops_cap) || len > 0xFFFFFFFFu) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const hdparse::Counts c = hdparse::walk(in, 0u, (uint32_t)len, 0u, OpStore{ops, 0u, clamp32(ops_cap)});
  *nops = c.ops;
  if (c.ops > ops_cap) return NGHTTP2_AMD_ERR_BUFFER_ERROR;
  return c.ok ? 0 : NGHTTP2_AMD_ERR_HEADER_COMP;
}

int nghttp2_amd_hd_parse_blocks_bound(uint64_t wire_bytes, uint32_t nblocks, size_t *ops_cap, size_t *lits_cap,
                                      size_t *pool_cap, size_t *ws_bytes) {
  if (wire_bytes > 0xFFFFFFFFu) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const size_t w = (size_t)wire_bytes;
  if (ops_cap) *ops_cap = w ? w : 1u;
  if (lits_cap) *lits_cap = w ? w : 1u;
  if (pool_cap) *pool_cap = hdhost::round16(w) + 16u;
  if (ws_bytes) *ws_bytes = ws_need(nblocks);
  return 0;
}

int nghttp2_amd_hd_parse_blocks_batch(const uint8_t *wire, const uint32_t *block_off, uint32_t nblocks,
                                      uint32_t *op_off, nghttp2_amd_hd_op *ops, size_t ops_cap,
                                      int32_t *block_status, uint32_t *lit_base, uint32_t *totals, void *workspace,
                                      size_t ws_bytes, void *stream) {
  const uint32_t n = nblocks;
  if (n == 0) return 0;
  if (!wire || !block_off || !op_off || (!ops && ops_cap) || !block_status || !lit_base || !totals || !workspace ||
      ws_bytes < ws_need(n))
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  uint32_t *byte_base = (uint32_t *)workspace;
  const uint32_t cap = clamp32(ops_cap);
  const dim3 grid((n + PB_WG - 1u) / PB_WG);
  hipLaunchKernelGGL(k_parse_blocks<false>, grid, dim3(PB_WG), 0, st, wire, block_off, n, op_off, ops, cap,
                     block_status, lit_base, byte_base, totals);
  hipLaunchKernelGGL(k_parse_scan, dim3(1), dim3(SC_WG), 0, st, op_off, lit_base, byte_base, n, cap, totals);
  hipLaunchKernelGGL(k_parse_blocks<true>, grid, dim3(PB_WG), 0, st, wire, block_off, n, op_off, ops, cap,
                     block_status, lit_base, byte_base, totals);
  return hdhost::hip_rv(hipGetLastError());
}

int nghttp2_amd_hd_gather_literals_batch(const uint8_t *wire, size_t wire_bytes, const nghttp2_amd_hd_op *ops,
                                         size_t ops_cap, uint32_t *totals, uint32_t *lit_off, size_t lits_cap,
                                         uint8_t *pool, size_t pool_cap, void *stream) {
  if (!wire || !ops || !totals || !lit_off || !pool) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t cap = clamp32(ops_cap), lcap = clamp32(lits_cap);
  const dim3 grid((cap + GL_WG - 1u) / GL_WG);
  if (cap)
    hipLaunchKernelGGL(k_lit_lens, grid, dim3(GL_WG), 0, st, ops, cap, (const uint32_t *)totals, lit_off, lcap);
  hipLaunchKernelGGL(k_lit_scan, dim3(1), dim3(SC_WG), 0, st, totals, lit_off, lcap, (uint64_t)pool_cap);
  if (cap)
    hipLaunchKernelGGL(k_gather, grid, dim3(GL_WG), 0, st, wire, (uint64_t)wire_bytes, ops, cap,
                       (const uint32_t *)totals, (const uint32_t *)lit_off, pool, (uint64_t)pool_cap);
  return hdhost::hip_rv(hipGetLastError());
}

}  // extern "C"
