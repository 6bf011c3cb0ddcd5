// hd_fields.hip -- what the session needs of a replayed block, on the device:
// every field's NGHTTP2_AMD_CHECK_* masks, its name token and
// nghttp2_http_on_header's verdict, every block's state and result, for gfx950.
//
// Reference: nghttp2_http_on_header and the two block-end functions
// (lib/nghttp2_http.c:405-511, stated once in hd_http.h), called by the session
// on every field an inflater hands over (lib/nghttp2_session.c:3588).  The
// results are nghttp2_amd_hd_inflate_blocks_http's for the same fields; the
// input is what nghttp2_amd_hd_dev_inflate_blocks (hd_replay.hip) left in
// device memory: nghttp2_amd_hd_nv records and the arena of name, NUL, value,
// NUL per field.
//
// nghttp2_amd_hd_dev_fields_http, up to six launches, n known on the host from
// nva_cap and nblocks, the counts read on the device:
//   k_field_views    one lane per field slot: three string views of the arena
//                    in the batch layout (byte pool + offsets + lengths) -- all
//                    strings interleaved, the names, the values -- and the
//                    call's totals word.  A slot past the field count is a
//                    string that is not examined (hd_string_walk.h).
//   k_check_fields   (hd_check.hip, unchanged) on the interleaved view
//   k_name_tokens<true>  (hd_names.hip, unchanged, no hash) on the names
//   k_field_publish  one lane per field slot: the masks and tokens of the
//                    slots below the field count go to the caller's arrays
//   k_http_facts     (hd_http.hip, unchanged) on the values
//   k_http_blocks    one lane per block, 64 blocks per one-wave workgroup: the
//                    lane runs its block's fields in order through
//                    hdhttp::BlockRun, the host inflater's driver.
// The three batch kernels write every slot they are launched for, the slots
// past the count included (INVALID), so they write into the workspace and
// k_field_publish copies what the caller may see.
// k_http_blocks is a chain per block, a latency like k_replay's: what a field's
// step reads -- token, the two masks, facts, number, the nv record -- is loaded
// together, two fields ahead of the step, and the name's first byte one field
// ahead (it needs the record's offset); the rest of a name is read only when
// NAME_LOWER is clear.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nghttp2_amd_hd.h"
#include "hd_field_classes.h"
#include "hd_host.h"
#include "hd_http.h"

namespace {

constexpr uint32_t FV_WG = 256;  // k_field_views, k_field_publish: a lane per field slot
constexpr uint32_t HB_WG = 64;   // k_http_blocks: one wave, 64 blocks

__constant__ hdcls::Table kNameTable = hdcls::kTable;

// The workspace (the header's layout): the totals word, the three views, the
// masks and tokens of every slot, the values' facts and numbers.
struct Ws {
  uint32_t *totals;                // [4]
  uint32_t *all_off;               // [2 cap + 1]
  int32_t *all_len;                // [2 cap]
  uint32_t *name_off, *value_off;  // [cap + 1] each
  int32_t *name_len, *value_len;   // [cap] each
  uint8_t *masks;                  // [2 cap]
  int32_t *tokens;                 // [cap]
  uint32_t *facts;                 // [cap]
  int64_t *numbers;                // [cap]
  size_t total;
};
__host__ Ws ws_layout(void *base, size_t cap) {
  Ws w;
  hdhost::Carve c{base};
  w.totals = c.take<uint32_t>(4);
  w.all_off = c.take<uint32_t>(2 * cap + 1);
  w.all_len = c.take<int32_t>(2 * cap);
  w.name_off = c.take<uint32_t>(cap + 1);
  w.name_len = c.take<int32_t>(cap);
  w.value_off = c.take<uint32_t>(cap + 1);
  w.value_len = c.take<int32_t>(cap);
  w.numbers = c.take<int64_t>(cap);
  w.facts = c.take<uint32_t>(cap);
  w.tokens = c.take<int32_t>(cap);
  w.masks = c.take<uint8_t>(2 * cap);
  w.total = c.total();
  return w;
}

// Slot k's strings as the three views see them; slot cap is the views' end.
// Every offset is at most T, the arena bytes the replay wrote, so whatever a
// record holds (a block no connection listed leaves its slots unwritten), no
// view reaches past T: a string is examined only when its length fits between
// its offset and the next one (hdwalk::string_range).
__global__ __launch_bounds__(FV_WG) void k_field_views(const nghttp2_amd_hd_nv *__restrict__ nva, uint32_t cap,
                                                       uint64_t arena_bytes,
                                                       const uint32_t *__restrict__ out_totals,
                                                       uint32_t *__restrict__ totals, uint32_t *__restrict__ all_off,
                                                       int32_t *__restrict__ all_len, uint32_t *__restrict__ name_off,
                                                       int32_t *__restrict__ name_len,
                                                       uint32_t *__restrict__ value_off,
                                                       int32_t *__restrict__ value_len) {
  const uint32_t k = blockIdx.x * FV_WG + threadIdx.x;
  if (k > cap) return;
  // the call's own test, made here and left in the totals word for the
  // kernels behind: no field when the replay wrote none (an overflow bit), and
  // none when the arena is not readable to the pool rule's end
  uint32_t nf = min(out_totals[0], cap), T = out_totals[1], bits = 0;
  if (out_totals[2]) bits |= NGHTTP2_AMD_HD_DEV_FIELDS_NOT_REPLAYED;
  if (!bits && nf && arena_bytes < (((uint64_t)T + 15u) & ~15ull) + 16u) bits |= NGHTTP2_AMD_HD_DEV_FIELDS_ARENA_SHORT;
  if (bits) nf = 0, T = 0;
  if (k == 0) {
    totals[0] = nf;
    totals[1] = T;
    totals[2] = bits;
    totals[3] = 0u;
  }
  uint32_t no = T, vo = T;
  int32_t nl = -1, vl = -1;
  if (k < nf) {
    const nghttp2_amd_hd_nv nv = nva[k];
    no = min(nv.name_off, T);
    vo = min(nv.value_off, T);
    nl = (int32_t)min(nv.name_len, 0x7FFFFFFFu);
    vl = (int32_t)min(nv.value_len, 0x7FFFFFFFu);
  }
  name_off[k] = no;
  value_off[k] = vo;
  if (k == cap) {
    all_off[2u * k] = T;
    return;
  }
  *reinterpret_cast<uint2 *>(all_off + 2u * k) = make_uint2(no, vo);
  *reinterpret_cast<int2 *>(all_len + 2u * k) = make_int2(nl, vl);
  name_len[k] = nl;
  value_len[k] = vl;
}

__global__ __launch_bounds__(FV_WG) void k_field_publish(const uint32_t *__restrict__ totals, uint32_t cap,
                                                         const uint8_t *__restrict__ masks,
                                                         const int32_t *__restrict__ tokens,
                                                         uint8_t *__restrict__ nv_checks,
                                                         int32_t *__restrict__ nv_tokens) {
  const uint32_t k = blockIdx.x * FV_WG + threadIdx.x;
  if (k >= cap || k >= totals[0]) return;
  if (nv_checks) {
    const uint32_t m = reinterpret_cast<const uint16_t *>(masks)[k];
    nv_checks[2u * k] = (uint8_t)m;
    nv_checks[2u * k + 1u] = (uint8_t)(m >> 8);
  }
  if (nv_tokens) nv_tokens[k] = tokens[k];
}

// What one field's step reads, but for the name's bytes.
struct Rec {
  uint32_t name_off, name_len, value_len, masks, facts;
  int32_t token;
  int64_t number;
};
__device__ __forceinline__ Rec load_rec(const nghttp2_amd_hd_nv *nva, const uint8_t *masks, const int32_t *tokens,
                                        const uint32_t *facts, const int64_t *numbers, uint32_t k) {
  Rec r;
  r.name_off = nva[k].name_off;
  r.name_len = nva[k].name_len;
  r.value_len = nva[k].value_len;
  r.masks = reinterpret_cast<const uint16_t *>(masks)[k];
  r.token = tokens[k];
  r.facts = facts[k];
  r.number = numbers[k];
  return r;
}

__global__ __launch_bounds__(HB_WG) void k_http_blocks(
    const uint32_t *__restrict__ totals, const nghttp2_amd_hd_nv *__restrict__ nva, const uint8_t *__restrict__ arena,
    const uint32_t *__restrict__ block_nv_off, const int32_t *__restrict__ out_status, uint32_t nblocks,
    const uint8_t *__restrict__ masks, const int32_t *__restrict__ tokens, const uint32_t *__restrict__ facts,
    const int64_t *__restrict__ numbers, const uint8_t *__restrict__ block_modes,
    nghttp2_amd_hd_http_state *__restrict__ block_state, int32_t *__restrict__ nv_verdicts,
    int32_t *__restrict__ block_http) {
  const uint32_t i = blockIdx.x * HB_WG + threadIdx.x;
  if (i >= nblocks) return;
  const uint32_t nf = totals[0], T = totals[1], skip = totals[2];
  uint32_t f0 = block_nv_off[i], f1 = block_nv_off[i + 1];
  const uint32_t mode = block_modes[i];
  const int32_t status = out_status[i];
  hdhttp::BlockRun run = {block_state[i], mode};
  if (skip) return;  // no field was written, or none may be read: nothing changes
  f0 = min(f0, nf);
  f1 = max(min(f1, nf), f0);
  // a name the arena does not hold (a record nothing wrote) is an empty one
  auto fit = [T](Rec &r) {
    if (r.name_off >= T || r.name_len > T - r.name_off) r.name_len = 0u;
  };
  const Rec none = {};
  Rec r0 = none, r1 = none;
  uint32_t b0 = 0u;
  if (f0 < f1) r0 = load_rec(nva, masks, tokens, facts, numbers, f0);
  if (f0 + 1u < f1) r1 = load_rec(nva, masks, tokens, facts, numbers, f0 + 1u);
  fit(r0);
  if (r0.name_len) b0 = arena[r0.name_off];
  uint32_t k = f0;
  for (; k < f1; ++k) {
    Rec r2 = none;
    uint32_t b1 = 0u;
    // (a record is looked at one field after its loads were issued, not at once)
    if (k + 2u < f1) r2 = load_rec(nva, masks, tokens, facts, numbers, k + 2u);
    fit(r1);
    if (r1.name_len) b1 = arena[r1.name_off];
    const hdhttp::Field f = {arena + r0.name_off, r0.name_len,       r0.value_len, r0.token, r0.masks & 0xFFu,
                             r0.masks >> 8,       r0.facts,          r0.number,    (int32_t)b0};
    const int rv = run.step(f, kNameTable.cls);
    if (nv_verdicts) nv_verdicts[k] = rv;
    if (run.stopped) break;
    r0 = r1;
    b0 = b1;
    r1 = r2;
  }
  // behind the block's first stream error a step answers NOT_EXAMINED: stored, not asked for
  if (nv_verdicts)
    for (++k; k < f1; ++k) nv_verdicts[k] = NGHTTP2_AMD_HTTP_NOT_EXAMINED;
  run.finish(status);
  block_state[i] = run.st;
  if (block_http) block_http[i] = run.result;
}

constexpr size_t kMaxSlots = 0x7FFFFFFFu;  // 2 * nva_cap strings are one batch of the check

}  // namespace

extern "C" {

size_t nghttp2_amd_hd_dev_fields_http_workspace_size(size_t nva_cap, uint32_t nblocks) {
  (void)nblocks;  // (nothing is kept per block)
  return ws_layout(nullptr, nva_cap > kMaxSlots ? kMaxSlots : nva_cap).total;
}

int nghttp2_amd_hd_dev_fields_http(const nghttp2_amd_hd_nv *nva, size_t nva_cap, const uint8_t *arena,
                                   size_t arena_bytes, const uint32_t *block_nv_off, const int32_t *out_status,
                                   const uint32_t *out_totals, uint32_t nblocks, uint8_t *nv_checks,
                                   int32_t *nv_tokens, const uint8_t *block_modes,
                                   nghttp2_amd_hd_http_state *block_state, int32_t *nv_verdicts, int32_t *block_http,
                                   void *workspace, size_t ws_bytes, void *stream) {
  if (nblocks == 0) return 0;
  const bool http = block_modes || block_state || nv_verdicts || block_http;
  if (http && (!block_modes || !block_state)) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  if ((nva_cap && (!nva || !arena)) || nva_cap > kMaxSlots || ((uintptr_t)arena & 15u) || !block_nv_off || !out_status ||
      !out_totals || !workspace || ((uintptr_t)workspace & 15u))
    return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  const uint32_t cap = (uint32_t)nva_cap;
  const Ws w = ws_layout(workspace, cap);
  if (ws_bytes < w.total) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  if (!http && !nv_checks && !nv_tokens) return 0;  // nothing is asked for
  hipStream_t st = (hipStream_t)stream;
  const bool checks = http || nv_checks, tokens = http || nv_tokens;
  hipLaunchKernelGGL(k_field_views, dim3(cap / FV_WG + 1u), dim3(FV_WG), 0, st, nva, cap, (uint64_t)arena_bytes,
                     out_totals, w.totals, w.all_off, w.all_len, w.name_off, w.name_len, w.value_off, w.value_len);
  int rv = hdhost::hip_rv(hipGetLastError());
  if (!rv && checks) rv = nghttp2_amd_hd_check_fields_batch(arena, w.all_off, w.all_len, 2u * cap, w.masks, stream);
  if (!rv && tokens)
    rv = nghttp2_amd_hd_name_tokens_len_batch(arena, w.name_off, w.name_len, cap, w.tokens, nullptr, stream);
  if (!rv && cap && (nv_checks || nv_tokens)) {
    hipLaunchKernelGGL(k_field_publish, dim3((cap + FV_WG - 1u) / FV_WG), dim3(FV_WG), 0, st,
                       (const uint32_t *)w.totals, cap, (const uint8_t *)w.masks, (const int32_t *)w.tokens,
                       nv_checks, nv_tokens);
    rv = hdhost::hip_rv(hipGetLastError());
  }
  if (rv || !http) return rv;
  rv = nghttp2_amd_hd_http_facts_batch(arena, w.value_off, w.value_len, cap, w.facts, w.numbers, stream);
  if (rv) return rv;
  hipLaunchKernelGGL(k_http_blocks, dim3((nblocks + HB_WG - 1u) / HB_WG), dim3(HB_WG), 0, st,
                     (const uint32_t *)w.totals, nva, arena, block_nv_off, out_status, nblocks,
                     (const uint8_t *)w.masks, (const int32_t *)w.tokens, (const uint32_t *)w.facts,
                     (const int64_t *)w.numbers, block_modes, block_state, nv_verdicts, block_http);
  return hdhost::hip_rv(hipGetLastError());
}

int nghttp2_amd_hd_dev_fields_http_totals(const void *workspace, uint32_t *totals, void *stream) {
  if (!workspace || !totals) return NGHTTP2_AMD_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(totals, workspace, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return hdhost::hip_rv(e);
}

}  // extern "C"
