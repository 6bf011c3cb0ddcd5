/*
 * nghttp2_amd_hd.h -- C ABI of the MI355X-native HPACK Huffman engine.
 *
 * This is the drop-in boundary for nghttp2's HPACK Huffman hot path
 * (lib/nghttp2_hd_huffman.c + lib/nghttp2_hd_huffman_data.c in the
 * reference).  Plain C: pointers, sizes and ints only.  HIP streams are
 * passed as `void *` (a hipStream_t; NULL = the default stream).
 *
 * Two groups of entry points:
 *
 *  1. Batched, device-resident API (nghttp2_amd_hd_huff_*_batch).  N
 *     independent header strings in SoA form: one contiguous byte pool plus
 *     uint32 offsets[N+1] (string i = pool[off[i] .. off[i+1])).  All
 *     pointers are device pointers (hipMalloc'd or HBM-resident torch
 *     storage).  Calls are asynchronous on `stream`.  This is what the
 *     batched drivers (replacing src/deflatehd.cc / src/inflatehd.cc) and
 *     an integration under emit_string / hd_inflate_read_huff bind.
 *
 *  2. Link-level replacements of the reference's internal Huffman API
 *     (lib/nghttp2_hd.h:394-440) -- see nghttp2_amd_hd_huffman_compat.h.
 *
 * Pool requirements (device API): pool base pointers 16-byte aligned; the
 * source pool readable up to align_up(off[N], 16) + 16 bytes (kernels load
 * aligned 16-byte words and unaligned 4-byte windows).  src_off[0] may be
 * any value; only the source bytes from `src_off[0] & ~15` on are read.
 * Offsets are uint32, so one batch's pool is
 * < 4 GiB; shard larger sets (multi-GPU).
 *
 * Error convention: 0 on success or a negative nghttp2_error code
 * (lib/includes/nghttp2/nghttp2.h:278-459).  Per-string decode results are
 * reported in a status array, never by the return value.
 */
#ifndef NGHTTP2_AMD_HD_H
#define NGHTTP2_AMD_HD_H

#include <stddef.h>
#include <stdint.h>

#ifndef NGHTTP2_AMD_EXTERN
#define NGHTTP2_AMD_EXTERN __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* nghttp2_error values used on this path (lib/includes/nghttp2/nghttp2.h) */
#define NGHTTP2_AMD_ERR_INVALID_ARGUMENT (-501) /* nghttp2.h:278 */
#define NGHTTP2_AMD_ERR_BUFFER_ERROR (-502)     /* nghttp2.h:282 */
#define NGHTTP2_AMD_ERR_INVALID_STATE (-519)    /* nghttp2.h:366 */
#define NGHTTP2_AMD_ERR_HEADER_COMP (-523)      /* nghttp2.h:378 */
#define NGHTTP2_AMD_ERR_INSUFF_BUFSIZE (-525)   /* nghttp2.h:386 */
#define NGHTTP2_AMD_ERR_FATAL (-900)            /* nghttp2.h:451 (HIP error) */
#define NGHTTP2_AMD_ERR_NOMEM (-901)            /* nghttp2.h:455 */

/* dst_off[n] after nghttp2_amd_hd_huff_encode_batch when the batch's encoded
 * total does not fit min(dst_cap, 0xFFFFFFFE): offsets are uint32, so such a
 * batch must be split (no offset of it is valid, no byte was written at or
 * past dst_cap). */
#define NGHTTP2_AMD_OFF_OVERFLOW 0xFFFFFFFFu

/* Decode-context flag bits (lib/nghttp2_hd_huffman.h:35-37). */
#define NGHTTP2_AMD_HUFF_ACCEPTED 0x01u
#define NGHTTP2_AMD_HUFF_SYM 0x02u
/* Failure (EOS decoded) state id (lib/nghttp2_hd_huffman.h:44-48). */
#define NGHTTP2_AMD_HUFF_FAIL_STATE 0x100u

/* Library version string, e.g. "nghttp2_amd_hd 0.1.0 gfx950". */
NGHTTP2_AMD_EXTERN const char *nghttp2_amd_hd_version(void);

/* Copies the engine's Huffman tables out in the reference's struct layouts
 * so a caller can check them against lib/nghttp2_hd_huffman_data.c without a
 * GPU: sym_out receives huff_sym_table (257 x {u32 nbits, u32 code} = 2056
 * bytes, lib/nghttp2_hd_huffman_data.c:29-94), dec_out receives
 * huff_decode_table (257 x 16 x {u16 fstate, u8 flags, u8 sym} = 16448 bytes,
 * :96-4980).  Either pointer may be NULL.  Returns 0. */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_tables(void *sym_out, void *dec_out);

/* ------------------------------------------------------------------ */
/* Sizing helpers (host-only, no GPU needed)                           */
/* ------------------------------------------------------------------ */

/* Upper bound of the encoded pool for `raw_bytes` bytes in `n` strings:
 * every symbol is at most 30 bits (RFC 7541 App. B), plus one padding byte
 * per string, rounded up to 16. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_huff_encode_bound(uint64_t raw_bytes, uint32_t n);

/* Size of the decode output pool nghttp2_amd_hd_huff_decode_batch_auto needs
 * for an encoded pool of `enc_bytes` bytes in `n` strings:
 * floor(8 * enc_bytes / 5) + 4 * n, rounded up. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_huff_decode_bound(uint64_t enc_bytes, uint32_t n);

/* Bytes of device workspace nghttp2_amd_hd_huff_encode_batch and
 * nghttp2_amd_hd_huff_decode_slots need for `n` strings. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_huff_workspace_size(uint32_t n);

/* A workspace size for nghttp2_amd_hd_huff_encode_batch that is also valid
 * for earlier versions of the library, which kept per-piece bit counts for
 * `raw_bytes` raw bytes in `n` strings.  Any size >=
 * nghttp2_amd_hd_huff_workspace_size(n) is valid; the current kernels use
 * only that much. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_huff_encode_workspace_size(uint64_t raw_bytes, uint32_t n);

/* ------------------------------------------------------------------ */
/* Batched device-resident API                                          */
/* ------------------------------------------------------------------ */

/*
 * Encode N strings.  Replaces, for a whole batch, emit_string's
 * nghttp2_hd_huff_encode_count + nghttp2_hd_huff_encode pair
 * (lib/nghttp2_hd.c:1009, :1037; lib/nghttp2_hd_huffman.c:34-104).
 *
 *   src, src_off[n+1] : raw strings (device)
 *   dst               : encoded pool (device), >= dst_cap bytes
 *   dst_off[n+1]      : OUT: encoded string i = dst[dst_off[i]..dst_off[i+1]);
 *                       dst_off[i+1]-dst_off[i] == nghttp2_hd_huff_encode_count
 *   workspace         : device scratch, >= nghttp2_amd_hd_huff_workspace_size(n)
 *
 * Output bytes equal lib/nghttp2_hd_huffman.c's, including the EOS-prefix
 * (all ones) padding of the last byte.  Size dst_cap by
 * nghttp2_amd_hd_huff_encode_bound(src_off[n]-src_off[0], n); the kernels
 * never write past dst_cap.  Offsets are uint32: when the encoded total
 * would pass min(dst_cap, 0xFFFFFFFE), dst_off[n] = NGHTTP2_AMD_OFF_OVERFLOW
 * (check it after the stream synchronises) and the batch must be split: the
 * tiles of 256 strings that fit may already be written, nothing at or past
 * dst_cap is, and no offset of the batch is valid.  A batch holding a
 * string longer than NGHTTP2_AMD_ENCODE_MAX_STRING raw bytes (its code bits
 * would not fit the kernels' 32-bit counts), or a tile of 256 consecutive
 * strings (256 k .. 256 k + 255) whose encoded output may reach
 * NGHTTP2_AMD_ENCODE_MAX_TILE bytes (a wave places its output bits in 32-bit
 * positions), is marked the same way.  The tile test is conservative: it
 * sums each string's output rounded down to 64 KiB units and marks the tile
 * when that sum comes within 256 units of 2^13 (2^29 bytes), so a tile whose
 * output is between 2^29 - 16 MiB and 2^29 bytes may be marked too.  Header
 * strings are far below both (nghttp2 caps a field at 64 KiB,
 * NGHTTP2_HD_MAX_NV).
 */
#define NGHTTP2_AMD_ENCODE_MAX_STRING (0xFFFFFFFFu / 30u)
#define NGHTTP2_AMD_ENCODE_MAX_TILE (1u << 29)
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_encode_batch(const uint8_t *src, const uint32_t *src_off,
                                     uint32_t n, uint8_t *dst, size_t dst_cap,
                                     uint32_t *dst_off, void *workspace,
                                     size_t workspace_size, void *stream);

/*
 * HPACK string literals, batched: emit_string (lib/nghttp2_hd.c:1001-1044)
 * for N strings.  Literal i = dst[dst_off[i]..dst_off[i+1]) is
 *   H | length    the H bit (0x80) iff the Huffman form is strictly shorter
 *                 than the raw string (:1011), and the payload length as a
 *                 7-bit-prefix integer (count_encoded_length / encode_length,
 *                 :823-863, RFC 7541 5.1);
 *   payload       the Huffman bytes (nghttp2_hd_huff_encode) or the raw ones.
 * The literals are back to back in string order, ready to be spliced into
 * header blocks in wire order.  Two launches: the encode count (code bits
 * per string, tile sums of the literal lengths) and the encode pack, which
 * writes every literal -- prefix and payload -- straight into dst (no
 * intermediate Huffman pool); a batch of at most 256 strings takes one
 * launch that does both (the workspace is then not touched).
 *
 *   raw_bytes : src_off[n] - src_off[0] (sizes the bounds below)
 *   dst_cap   : >= nghttp2_amd_hd_emit_strings_bound(raw_bytes, n)
 *   workspace : device scratch (the tile sums),
 *               >= nghttp2_amd_hd_emit_strings_workspace_size(raw_bytes, n)
 */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_emit_strings_bound(uint64_t raw_bytes, uint32_t n);
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_emit_strings_workspace_size(uint64_t raw_bytes, uint32_t n);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_emit_strings_batch(const uint8_t *src, const uint32_t *src_off,
                                      uint32_t n, uint64_t raw_bytes, uint8_t *dst,
                                      size_t dst_cap, uint32_t *dst_off, void *workspace,
                                      size_t workspace_size, void *stream);

/*
 * Encoded lengths only: enc_len[i] = nghttp2_hd_huff_encode_count(string i)
 * (lib/nghttp2_hd_huffman.c:34-43).
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_encode_count_batch(const uint8_t *src,
                                           const uint32_t *src_off, uint32_t n,
                                           uint32_t *enc_len, void *stream);

/*
 * Output slots for a decode batch: dst_off[i+1]-dst_off[i] =
 * floor(8*E_i/5)+1, the reference's allocation for a Huffman literal
 * (nghttp2_huff_estimate_decode_length, lib/nghttp2_hd_huffman.h:76-78,
 * used at lib/nghttp2_hd.c:2080-2082 / :2166-2168).  dst_off[n] is the
 * pool size to allocate.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_decode_slots(const uint32_t *src_off, uint32_t n,
                                     uint32_t *dst_off, void *workspace,
                                     size_t workspace_size, void *stream);

/*
 * Decode N whole Huffman strings (each call is final, fin=1).  Replaces,
 * for a batch, hd_inflate_read_huff's nghttp2_hd_huff_decode_context_init +
 * nghttp2_hd_huff_decode(..., fin=1) + nghttp2_hd_huff_decode_failure_state
 * (lib/nghttp2_hd.c:1728-1751, :2076, :2162;
 * lib/nghttp2_hd_huffman.c:106-147).
 *
 *   src, src_off[n+1] : encoded strings (device)
 *   dst, dst_off[n+1] : output slots (device); string i's decoded bytes are
 *                       written to dst[dst_off[i] ...]
 *   status[n]         : OUT: decoded length (>= 0), or
 *                       NGHTTP2_AMD_ERR_HEADER_COMP (-523) exactly when the
 *                       reference returns it (non-accepting end state,
 *                       including EOS decoded), or
 *                       NGHTTP2_AMD_ERR_BUFFER_ERROR (-502) when the slot is
 *                       smaller than the decoded length.
 *   fstate[n], flags[n] : OUT, optional (NULL to skip): the final
 *                       nghttp2_hd_huff_decode_context {fstate, flags}
 *                       (lib/nghttp2_hd_huffman.h:56-60) after the string;
 *                       fstate == 0x100 <=> failure_state().
 *
 * On -523 the bytes decoded before the failure are still written (as the
 * reference leaves them in buf), so dst matches the reference byte for byte.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_decode_batch(const uint8_t *src, const uint32_t *src_off,
                                     uint32_t n, uint8_t *dst,
                                     const uint32_t *dst_off, int32_t *status,
                                     uint16_t *fstate, uint8_t *flags,
                                     void *stream);

/*
 * Same as nghttp2_amd_hd_huff_decode_batch, with the engine placing the
 * output in the same launch, densely: the batch is cut into tasks of 64
 * consecutive strings (t0 = 64 k), a task possibly split into two tasks of
 * 32 (t0 = 64 k, 64 k + 32: the engine splits the last tasks of each
 * workgroup's share so that its waves finish together), and the strings of
 * each task are back to back from the task's base
 *   base(t0) = 4 * (ceil(floor(8 x_t0 / 5) / 4) + t0),  x_t0 = src_off[t0] - src_off[0],
 * so dst_off[i] (OUT, n+1 entries) = base(t0) + the decoded bytes of the
 * task's strings before i, and dst_off[n] = the end of the last string
 * (dst_off is authoritative; which tasks were split is not specified).
 * Every string keeps the reference's allocation inside its task's span
 * (base(t1) - base(t0) >= the sum of floor(8 E_i / 5) + 1 over the task
 * [t0, t1)), so no
 * string can overflow; bytes between the end of a task's output and the
 * next task's base are unspecified.  dst (16-byte aligned) must hold
 * nghttp2_amd_hd_huff_decode_bound(E_total, n) bytes.  String i gets -502
 * when 4 * (ceil(floor(8 x_{i+1} / 5) / 4) + i + 1) > dst_cap (a pool
 * smaller than the bound); no byte at or past dst_cap is written and dst_off
 * entries saturate at dst_cap.  src_off must be non-decreasing: a task
 * holding a descending pair reports NGHTTP2_AMD_ERR_INVALID_ARGUMENT for its
 * strings and writes nothing for them.  Offsets
 * are uint32: dst_cap > 0xFFFFFFFF returns NGHTTP2_AMD_ERR_INVALID_ARGUMENT
 * (split a batch whose decode_bound passes 4 GiB).
 *
 * enc_bytes is the batch's encoded size, src_off[n] - src_off[0] (the value
 * that sized dst by nghttp2_amd_hd_huff_decode_bound).  It only picks the
 * kernel instance: a mean of at most 48 bytes per string (header-sized
 * strings) decodes whole strings as 64-byte items, a larger one cuts strings
 * into 40-byte pieces.  Both are exact for any input, so a wrong value costs
 * time, never correctness.  dst_cap does not enter the pick.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_decode_batch_auto(const uint8_t *src, const uint32_t *src_off,
                                          uint32_t n, uint64_t enc_bytes, uint8_t *dst,
                                          size_t dst_cap, uint32_t *dst_off, int32_t *status,
                                          uint16_t *fstate, uint8_t *flags, void *stream);

/*
 * The reference's nibble-stepped FSM itself (lib/nghttp2_hd_huffman.c:111-143
 * over huff_decode_table, :122-133), batched: an exact cross-check of the
 * canonical decoder and the path for chunked (streaming) input.  Each string
 * i starts from the decode context {init_fstate[i], init_flags[i]} (both
 * NULL: nghttp2_hd_huff_decode_context_init, :106-109), the final context is
 * written to fstate/flags (optional), and `final` is the reference's fin
 * flag: when nonzero a non-accepting end state gives -523, else status is
 * the number of bytes written (the reference returns srclen then; the
 * caller checks fstate == 0x100 for failure_state, :145-147).
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_huff_decode_fsm_batch(const uint8_t *src, const uint32_t *src_off,
                                         uint32_t n, uint8_t *dst, const uint32_t *dst_off,
                                         int32_t *status, uint16_t *fstate, uint8_t *flags,
                                         const uint16_t *init_fstate,
                                         const uint8_t *init_flags, int final,
                                         void *stream);

/* ------------------------------------------------------------------ */
/* Header-name tokens and name hash              */
/* ------------------------------------------------------------------ */
/*
 * Replaces lookup_token (lib/nghttp2_hd.c:137-520) and name_hash
 * (lib/nghttp2_hd.c:536-547), both static in the reference and called per
 * header field by deflate_nv (:1388-1393) and the inflater (:1811).
 *
 * nghttp2_amd_hd_name_tokens_batch: N names in the batch layout (device pool
 * + uint32 offsets[N+1], pool readable to align_up(off[N], 16) + 16);
 * token[i] = lookup_token(name i) (-1, or NGHTTP2_TOKEN_* of
 * lib/nghttp2_hd.h:56-116: the first static-table index of a static name,
 * 61..67 for te, connection, keep-alive, proxy-connection, upgrade,
 * :protocol, priority); hash[i] = 32-bit FNV-1a of name i (equal to the
 * reference's static_table[token].hash for a static name).  Device pointers,
 * asynchronous on `stream`.
 *
 * nghttp2_amd_hd_name_tokens_len_batch: the same over strings with a length
 * array, as nghttp2_amd_hd_check_fields_batch takes them.  len == NULL:
 * string i = pool[off[i] .. off[i+1]).  len given: string i = pool[off[i] ..
 * off[i] + len[i]) -- nghttp2_amd_hd_huff_decode_batch_auto's (dst, dst_off,
 * status), tokenised in the decode's stream with no repacking.  off (n + 1
 * entries) must be non-decreasing; the pool is 16-byte aligned and readable
 * to align_up(off[n], 16) + 16.  A string gets NGHTTP2_AMD_TOKEN_INVALID and
 * hash 0, and none of its bytes is read, when len[i] < 0 (a failed decode's
 * status), off[i] + len[i] > off[i+1] (compared without wrapping) or off[i] >
 * off[i+1]; NGHTTP2_AMD_TOKEN_NONE is lookup_token's -1: examined, not a
 * token name.  Bytes outside a string never reach its token or hash.  hash
 * may be NULL: only tokens are written, and a string longer than the longest
 * token name gets NGHTTP2_AMD_TOKEN_NONE with none of its bytes read (with
 * hash given every examined string is hashed in full).  Device pointers,
 * asynchronous on `stream`; n == 0 returns 0, a NULL pool, off or token
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 *
 * nghttp2_amd_hd_lookup_token / nghttp2_amd_hd_name_hash: the same for one
 * host name (what a single deflate_nv call binds).
 */
#define NGHTTP2_AMD_TOKEN_NONE (-1)
#define NGHTTP2_AMD_TOKEN_INVALID (-2)
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_name_tokens_batch(const uint8_t *names,
                                                        const uint32_t *name_off, uint32_t n,
                                                        int32_t *token, uint32_t *hash,
                                                        void *stream);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_name_tokens_len_batch(const uint8_t *pool, const uint32_t *off,
                                                            const int32_t *len, uint32_t n,
                                                            int32_t *token, uint32_t *hash,
                                                            void *stream);
NGHTTP2_AMD_EXTERN int32_t nghttp2_amd_hd_lookup_token(const uint8_t *name, size_t namelen);
NGHTTP2_AMD_EXTERN uint32_t nghttp2_amd_hd_name_hash(const uint8_t *name, size_t namelen);

/* ------------------------------------------------------------------ */
/* Header-field validation (nghttp2_check_*)                            */
/* ------------------------------------------------------------------ */
/*
 * Replaces the per-byte table scans nghttp2_http_on_header
 * (lib/nghttp2_http.c:405-447) runs on every name and value the inflater
 * hands over: nghttp2_check_header_name, _header_value,
 * _header_value_rfc9113, _method, _path, _authority (nghttp2.h) and the
 * internal nghttp2_check_nonempty_header_name (lib/nghttp2_helper.h), all in
 * lib/nghttp2_helper.c:346-558.  One pass over a string answers all of them:
 * the result is a uint8 mask, a bit set exactly when the reference function
 * returns 1 for the string.
 *
 * NAME_LOWER says whether nghttp2_check_nonempty_header_name returns 1; its
 * 0-versus-2 result for a refused name (which bad byte comes first) is told
 * apart by nghttp2_amd_hd_http_on_header below, and the authority table
 * without '@' that is private to lib/nghttp2_http.c is
 * NGHTTP2_AMD_HTTP_FACT_AUTHORITY (AUTHORITY here is the public
 * nghttp2_check_authority, which allows '@').
 */
#define NGHTTP2_AMD_CHECK_NAME 0x01u          /* nghttp2_check_header_name: empty 0, a leading ':' skipped, ":" 0 */
#define NGHTTP2_AMD_CHECK_VALUE 0x02u         /* nghttp2_check_header_value: empty 1 */
#define NGHTTP2_AMD_CHECK_VALUE_RFC9113 0x04u /* nghttp2_check_header_value_rfc9113: and no SP / HT at either end */
#define NGHTTP2_AMD_CHECK_METHOD 0x08u        /* nghttp2_check_method: empty 0 */
#define NGHTTP2_AMD_CHECK_PATH 0x10u          /* nghttp2_check_path: empty 1 */
#define NGHTTP2_AMD_CHECK_AUTHORITY 0x20u     /* nghttp2_check_authority: empty 1 */
#define NGHTTP2_AMD_CHECK_NAME_LOWER 0x40u    /* nghttp2_check_nonempty_header_name(...) == 1: no ':' exemption, empty 1 */
#define NGHTTP2_AMD_CHECK_INVALID 0x80u       /* the string was not examined; every other bit is 0 */

/* The mask of one host string (no GPU). */
NGHTTP2_AMD_EXTERN uint8_t nghttp2_amd_hd_check_field(const uint8_t *s, size_t len);

/*
 * The masks of N strings: mask[i] (OUT, n bytes) for string i of the pool
 * (batch layout: 16-byte aligned, readable to align_up(off[n], 16) + 16).
 * len == NULL: string i = pool[off[i] .. off[i+1]).  len given: string i =
 * pool[off[i] .. off[i] + len[i]) -- what nghttp2_amd_hd_huff_decode_batch_auto
 * leaves behind as (dst, dst_off, status), dense per task with unspecified
 * bytes between tasks, so a decode's output is validated in the same stream
 * with no host round trip and no repacking.  off (n + 1 entries) must be
 * non-decreasing.  A string gets NGHTTP2_AMD_CHECK_INVALID, and none of its
 * bytes is read, when len[i] < 0 (a failed decode's status), off[i] + len[i]
 * > off[i+1], or off[i] > off[i+1].  Bytes outside a string never influence
 * its mask.  Device pointers, asynchronous on `stream`; n == 0 returns 0, a
 * NULL pool, off or mask NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_check_fields_batch(const uint8_t *pool, const uint32_t *off,
                                                         const int32_t *len, uint32_t n, uint8_t *mask,
                                                         void *stream);

/* ------------------------------------------------------------------ */
/* HTTP message validation (nghttp2_http_on_header)                     */
/* ------------------------------------------------------------------ */
/*
 * Replaces nghttp2_http_on_header (lib/nghttp2_http.c:405-447, called from
 * lib/nghttp2_session.c:3588 on every field an inflater hands over) and the
 * two block-end functions (:449-511).  The reference function switches on
 * nv.token, runs byte checks on the value and keeps the stream's http_flags,
 * content_length and status_code.  Here the byte work is split off: the
 * NGHTTP2_AMD_CHECK_* masks above, the name token, and the value facts below
 * are computed once per string (on the GPU for a batch), and the per-field
 * step is a pure host function of those that reads no value byte.
 *
 * Value facts: one uint32 per string, a bit set exactly when the reference's
 * test passes for the string, and one int64, parse_uint's value.
 * parse_status_code (:56-63) needs no bytes beyond them: it is UINT && len
 * == 3 && number >= 100; the "0" test of :357 is len == 1 && number == 0.
 */
#define NGHTTP2_AMD_HTTP_FACT_AUTHORITY 0x001u     /* check_authority (:168-176): no '@'; empty 1 */
#define NGHTTP2_AMD_HTTP_FACT_SCHEME 0x002u        /* check_scheme (:118-140): empty 0 */
#define NGHTTP2_AMD_HTTP_FACT_SCHEME_HTTP 0x004u   /* memieq against "http" / "https" (:246-247) */
#define NGHTTP2_AMD_HTTP_FACT_METH_HEAD 0x008u     /* exactly "HEAD" (:204-228) */
#define NGHTTP2_AMD_HTTP_FACT_METH_CONNECT 0x010u  /* exactly "CONNECT" */
#define NGHTTP2_AMD_HTTP_FACT_METH_OPTIONS 0x020u  /* exactly "OPTIONS" */
#define NGHTTP2_AMD_HTTP_FACT_PATH_SLASH 0x040u    /* not empty, first byte '/' */
#define NGHTTP2_AMD_HTTP_FACT_PATH_ASTERISK 0x080u /* exactly "*" */
#define NGHTTP2_AMD_HTTP_FACT_TE_TRAILERS 0x100u   /* lstrieq("trailers", ...) */
#define NGHTTP2_AMD_HTTP_FACT_LWS 0x200u           /* lws() (:142-150): SP / HT only; empty 1 */
#define NGHTTP2_AMD_HTTP_FACT_UINT 0x400u          /* parse_uint (:65-89) does not return -1 */
#define NGHTTP2_AMD_HTTP_FACT_INVALID 0x80000000u  /* the string was not examined; every other bit is 0 */

/* The facts of one host string (no GPU); *number (may be NULL) = parse_uint's
 * value when UINT is set, else -1. */
NGHTTP2_AMD_EXTERN uint32_t nghttp2_amd_hd_http_facts(const uint8_t *s, size_t len, int64_t *number);

/*
 * The facts of N strings: facts[i] and number[i] (OUT, n entries each) for
 * string i, in exactly the layouts nghttp2_amd_hd_check_fields_batch takes
 * (len == NULL or given; a decode's (dst, dst_off, status) as is; the pool
 * 16-byte aligned and readable to align_up(off[n], 16) + 16).  A string gets
 * NGHTTP2_AMD_HTTP_FACT_INVALID and number -1, and none of its bytes is
 * read, when len[i] < 0, off[i] + len[i] > off[i+1] or off[i] > off[i+1].
 * Bytes outside a string never influence its facts.  Exact for a string of
 * any length: parse_uint accepts any number of leading zeros and refuses at
 * the first overflow past INT64_MAX.  Device pointers, asynchronous on
 * `stream`; n == 0 returns 0, a NULL pool, off, facts or number
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_http_facts_batch(const uint8_t *pool, const uint32_t *off,
                                                       const int32_t *len, uint32_t n, uint32_t *facts,
                                                       int64_t *number, void *stream);

/* The stream's HTTP state the reference keeps in nghttp2_stream; a fresh
 * stream is {0, -1, -1}.  http_flags are NGHTTP2_HTTP_FLAG_* of
 * lib/nghttp2_stream.h:99-138. */
typedef struct {
  uint32_t http_flags;
  int32_t status_code;
  int64_t content_length;
} nghttp2_amd_hd_http_state;

#define NGHTTP2_AMD_HTTP_FLAG__AUTHORITY 0x01u
#define NGHTTP2_AMD_HTTP_FLAG__PATH 0x02u
#define NGHTTP2_AMD_HTTP_FLAG__METHOD 0x04u
#define NGHTTP2_AMD_HTTP_FLAG__SCHEME 0x08u
#define NGHTTP2_AMD_HTTP_FLAG_HOST 0x10u
#define NGHTTP2_AMD_HTTP_FLAG__STATUS 0x20u
#define NGHTTP2_AMD_HTTP_FLAG_REQ_HEADERS \
  (NGHTTP2_AMD_HTTP_FLAG__METHOD | NGHTTP2_AMD_HTTP_FLAG__PATH | NGHTTP2_AMD_HTTP_FLAG__SCHEME)
#define NGHTTP2_AMD_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED 0x40u
#define NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT 0x80u
#define NGHTTP2_AMD_HTTP_FLAG_METH_HEAD 0x0100u
#define NGHTTP2_AMD_HTTP_FLAG_METH_OPTIONS 0x0200u
#define NGHTTP2_AMD_HTTP_FLAG_METH_UPGRADE_WORKAROUND 0x0400u
#define NGHTTP2_AMD_HTTP_FLAG_METH_ALL                                           \
  (NGHTTP2_AMD_HTTP_FLAG_METH_CONNECT | NGHTTP2_AMD_HTTP_FLAG_METH_HEAD |        \
   NGHTTP2_AMD_HTTP_FLAG_METH_OPTIONS | NGHTTP2_AMD_HTTP_FLAG_METH_UPGRADE_WORKAROUND)
#define NGHTTP2_AMD_HTTP_FLAG_PATH_REGULAR 0x0800u
#define NGHTTP2_AMD_HTTP_FLAG_PATH_ASTERISK 0x1000u
#define NGHTTP2_AMD_HTTP_FLAG_SCHEME_HTTP 0x2000u
#define NGHTTP2_AMD_HTTP_FLAG_EXPECT_FINAL_RESPONSE 0x4000u
#define NGHTTP2_AMD_HTTP_FLAG__PROTOCOL 0x8000u
#define NGHTTP2_AMD_HTTP_FLAG_PRIORITY 0x010000u /* left to the caller, see below */
#define NGHTTP2_AMD_HTTP_FLAG_BAD_PRIORITY 0x020000u

/* What the reference reads from the session, the frame and the stream id. */
#define NGHTTP2_AMD_HTTP_MODE_REQUEST 0x01u          /* session->server or a PUSH_PROMISE; clear: a response */
#define NGHTTP2_AMD_HTTP_MODE_PUSH 0x02u             /* even stream id: CONNECT refused, priority not parsed */
#define NGHTTP2_AMD_HTTP_MODE_TRAILER 0x04u          /* the block is a trailer */
#define NGHTTP2_AMD_HTTP_MODE_CONNECT_PROTOCOL 0x08u /* the extended CONNECT setting is enabled */
#define NGHTTP2_AMD_HTTP_MODE_NO_RFC9113_WS 0x10u    /* RFC 9113's leading/trailing whitespace rule is off */

#define NGHTTP2_AMD_ERR_IGN_HTTP_HEADER (-105)    /* nghttp2.h NGHTTP2_ERR_IGN_HTTP_HEADER */
#define NGHTTP2_AMD_ERR_REMOVE_HTTP_HEADER (-106) /* NGHTTP2_ERR_REMOVE_HTTP_HEADER */
#define NGHTTP2_AMD_ERR_HTTP_HEADER (-531)        /* NGHTTP2_ERR_HTTP_HEADER */
#define NGHTTP2_AMD_ERR_HTTP_MESSAGING (-532)     /* NGHTTP2_ERR_HTTP_MESSAGING */

/*
 * nghttp2_http_on_header for one field, from what the batch calls computed:
 * the name's token and NGHTTP2_AMD_CHECK_* mask, and the value's mask, facts
 * and number.  Returns 0, NGHTTP2_AMD_ERR_IGN_HTTP_HEADER,
 * NGHTTP2_AMD_ERR_REMOVE_HTTP_HEADER or NGHTTP2_AMD_ERR_HTTP_HEADER and
 * updates *state exactly as lib/nghttp2_http.c:188-447 does.  It reads no
 * value byte; of the name it reads the first byte, and the rest only when
 * NAME_LOWER is clear, to tell nghttp2_check_nonempty_header_name's 0 from
 * its 2 (lib/nghttp2_helper.c:380-392).  A NULL state is
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT (from the two block-end functions too); a
 * NULL name is an empty one.
 *
 * Out of scope: the `priority` field's structured value
 * (nghttp2_http_parse_priority) is not parsed.  The verdict does not depend
 * on the parse and stays exact; BAD_PRIORITY is set when the value check
 * fails; NGHTTP2_AMD_HTTP_FLAG_PRIORITY, BAD_PRIORITY after a failed parse
 * and http_extpri are left to the caller.  nghttp2_http_on_trailer_headers,
 * _on_remote_end_stream, _on_data_chunk and _record_request_method read
 * frame flags and DATA, not header fields, and are left out.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_http_on_header(nghttp2_amd_hd_http_state *state, uint32_t mode,
                                                     const uint8_t *name, size_t name_len,
                                                     size_t value_len, int32_t token, uint8_t name_mask,
                                                     uint8_t value_mask, uint32_t value_facts,
                                                     int64_t value_number);
/* nghttp2_http_on_request_headers (:449-484; mode's PUSH bit stands for the
 * PUSH_PROMISE frame type) and nghttp2_http_on_response_headers (:486-511):
 * 0 or -1. */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_http_on_request_headers(nghttp2_amd_hd_http_state *state,
                                                              uint32_t mode);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_http_on_response_headers(nghttp2_amd_hd_http_state *state);

/* ------------------------------------------------------------------ */
/* Header blocks into representations and Huffman literals             */
/* ------------------------------------------------------------------ */
/*
 * The representation layer of nghttp2_hd_inflate_hd_nv
 * (lib/nghttp2_hd.c:1942-1985 opcode dispatch, decode_length :882-945) for
 * complete header blocks: a block is cut into its representations -- table
 * size updates, indexed fields, literal fields with their string literals'
 * extents -- which needs no table state, so every block of a batch is parsed
 * on its own.  What the representations mean (index resolution, insertion
 * with eviction, the size update rules) is the replay's, not this layer's.
 *
 * One representation.  Offsets are positions in the wire the block was
 * parsed from (the wire pool of a batch; the block itself for
 * nghttp2_amd_hd_parse_block), lengths are the encoded lengths on the wire.
 *   kind       NGHTTP2_AMD_HD_OP_SIZE / _INDEXED / _LITERAL
 *   flags      of a LITERAL: INDEX_REQUIRED (opcode 01xxxxxx: the field enters
 *              the dynamic table), NO_INDEX (0001xxxx: NGHTTP2_NV_FLAG_NO_INDEX),
 *              NEW_NAME (the name is a string literal; clear: `value` is its
 *              index), NAME_HUFF / VALUE_HUFF (the literal's H bit)
 *   value      SIZE: the new maximum; INDEXED and a LITERAL without NEW_NAME:
 *              the index (1-based as on the wire; 0 is the replay's error)
 *   name_off, name_len    the name literal's bytes (NEW_NAME), else 0
 *   value_off, value_len  the value literal's bytes (LITERAL), else 0
 *   name_lit, value_lit   the literal's number among the Huffman literals
 *              (batch: of the whole batch; one block: of the block), or -1
 *              for a raw literal or none
 * Huffman literals are numbered in wire order: blocks in batch order,
 * representations in order within a block, a name before its value.  A block
 * that fails keeps the representations completed before the failure, and
 * their literals keep their numbers, because the reference has emitted
 * those fields by then (the replay emits them too).  A Huffman literal of
 * length 0 is a Huffman literal.
 */
typedef struct {
  uint8_t kind;
  uint8_t flags;
  uint16_t reserved; /* 0 */
  uint32_t value;
  uint32_t name_off, name_len;
  uint32_t value_off, value_len;
  int32_t name_lit, value_lit;
} nghttp2_amd_hd_op; /* 32 bytes */

#define NGHTTP2_AMD_HD_OP_SIZE 0u
#define NGHTTP2_AMD_HD_OP_INDEXED 1u
#define NGHTTP2_AMD_HD_OP_LITERAL 2u

#define NGHTTP2_AMD_HD_OP_INDEX_REQUIRED 0x01u
#define NGHTTP2_AMD_HD_OP_NO_INDEX 0x02u
#define NGHTTP2_AMD_HD_OP_NEW_NAME 0x04u
#define NGHTTP2_AMD_HD_OP_NAME_HUFF 0x08u
#define NGHTTP2_AMD_HD_OP_VALUE_HUFF 0x10u

/*
 * One block on the host (no GPU): the representations of in[0, len) go to
 * ops[0, min(*nops, ops_cap)) and their number to *nops.  The rules are
 * exactly the inflater's: prefix integers as nghttp2_amd_hd_decode_length
 * (a group at a shift of 32 or more, a carry past UINT32_MAX, or an integer
 * the block end cuts off fails), string literals of at most 65536
 * (NGHTTP2_HD_MAX_NV) bytes that the rest of the block covers.  Returns
 *   0                             the whole block is representations;
 *   NGHTTP2_AMD_ERR_HEADER_COMP   the bytes after the last completed
 *                                 representation are none; the completed
 *                                 ones are written and counted;
 *   NGHTTP2_AMD_ERR_BUFFER_ERROR  *nops > ops_cap: *nops is the count
 *                                 needed, nothing at or past ops + ops_cap
 *                                 was written (this comes before
 *                                 HEADER_COMP: call again with room);
 *   NGHTTP2_AMD_ERR_INVALID_ARGUMENT  nops is NULL, in is NULL with len > 0,
 *                                 ops is NULL with ops_cap > 0, or len >
 *                                 UINT32_MAX (the record's offsets are
 *                                 uint32).
 * The same code walks a block on the GPU (csrc/hd_parse.h).
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_parse_block(const uint8_t *in, size_t len, nghttp2_amd_hd_op *ops,
                                                  size_t ops_cap, size_t *nops);

/* totals[3] of a parse: 0, or why the batch's results are not complete */
#define NGHTTP2_AMD_HD_PARSE_OVERFLOW_OPS 0x1u  /* more representations than ops_cap */
#define NGHTTP2_AMD_HD_PARSE_OVERFLOW_U32 0x2u  /* a total does not fit the uint32 offsets */
#define NGHTTP2_AMD_HD_PARSE_OVERFLOW_LITS 0x4u /* (gather) more Huffman literals than lits_cap */
#define NGHTTP2_AMD_HD_PARSE_OVERFLOW_POOL 0x8u /* (gather) more Huffman bytes than pool_cap */

/*
 * Capacities that cannot overflow for `nblocks` blocks lying side by side
 * (non-decreasing offsets) in `wire_bytes` bytes of wire: a representation
 * takes at least one wire byte and so does a string literal, so
 * *ops_cap = *lits_cap = max(wire_bytes, 1) entries, and the Huffman bytes
 * are wire bytes: *pool_cap = align_up(wire_bytes, 16) + 16 bytes, which is
 * also what the decode needs readable behind its input.  *ws_bytes is the
 * parse's device workspace.  Any pointer may be NULL.  Returns 0, or
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT when wire_bytes > UINT32_MAX.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_parse_blocks_bound(uint64_t wire_bytes, uint32_t nblocks, size_t *ops_cap,
                                                         size_t *lits_cap, size_t *pool_cap, size_t *ws_bytes);

/*
 * The representations of a batch of blocks, on the GPU.  Block i is
 * wire[block_off[i], block_off[i+1]).
 *
 *   wire, block_off[n+1] : IN (device)
 *   op_off[n+1]       : OUT: block i's records are ops[op_off[i], op_off[i+1])
 *   ops, ops_cap      : OUT: the records, room for ops_cap of them
 *   block_status[n]   : OUT: the block's number of representations, or
 *                       NGHTTP2_AMD_ERR_HEADER_COMP when the block fails
 *                       (its completed representations are still in ops, and
 *                       op_off counts them)
 *   lit_base[n+1]     : OUT: the number of the block's first Huffman literal;
 *                       lit_base[n] is the batch's count
 *   totals[4]         : OUT: {representations, Huffman literals, Huffman
 *                       bytes, NGHTTP2_AMD_HD_PARSE_OVERFLOW_* bits}
 *   workspace         : device scratch, >= the bound's ws_bytes
 *
 * Every record equals nghttp2_amd_hd_parse_block's for the block, with the
 * offsets positions in `wire` and the literal numbers the batch's.  A block
 * with block_off[i] > block_off[i+1] is not read and gets HEADER_COMP with
 * no representation, as a string of the scan kernels gets INVALID.  Bytes
 * outside a block never influence its result, and no byte outside the
 * blocks is read.
 *
 * Three launches: the count (one lane per block walks it: representations,
 * Huffman literals, Huffman bytes), a one-workgroup scan of the three counts
 * into op_off, lit_base and totals, and the write (the same walk, storing
 * records).  Every record store is checked against ops_cap: when the batch
 * holds more, totals[3] has OVERFLOW_OPS, nothing at or past ops + ops_cap
 * is written, and the records below it are valid.  When a total passes
 * UINT32_MAX (only blocks that overlap can do that), totals[3] has
 * OVERFLOW_U32 and no record, offset or status is valid.  Size the arrays
 * by nghttp2_amd_hd_parse_blocks_bound and neither happens.
 *
 * Device pointers, asynchronous on `stream`.  n == 0 returns 0 and touches
 * nothing.  A NULL wire, block_off, op_off, ops (with ops_cap > 0),
 * block_status, lit_base, totals or workspace, or a workspace smaller than
 * the bound's, is NGHTTP2_AMD_ERR_INVALID_ARGUMENT.  A block's status is
 * int32: a block of 2^31 representations or more is out of scope.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_parse_blocks_batch(const uint8_t *wire, const uint32_t *block_off,
                                                         uint32_t nblocks, uint32_t *op_off,
                                                         nghttp2_amd_hd_op *ops, size_t ops_cap,
                                                         int32_t *block_status, uint32_t *lit_base,
                                                         uint32_t *totals, void *workspace, size_t ws_bytes,
                                                         void *stream);

/*
 * Every Huffman literal of a parsed batch, copied into one pool in the
 * decode's input layout: literal k (its number in the records) is
 * pool[lit_off[k], lit_off[k+1]), the literals back to back from 0, so
 * (pool, lit_off, totals[1] strings) goes to
 * nghttp2_amd_hd_huff_decode_batch_auto as it is.
 *
 *   wire, wire_bytes  : the wire the records point into, and its size (a
 *                       record reaching past it is not copied)
 *   ops, ops_cap      : the parse's records and their capacity
 *   totals            : the parse's totals (device): the counts are read
 *                       there, so the call follows the parse on the stream
 *                       with no host synchronisation; the gather ORs its own
 *                       OVERFLOW_* bits into totals[3]
 *   lit_off, lits_cap : OUT: lits_cap + 1 entries; [0, totals[1]] written
 *   pool, pool_cap    : OUT: the literals' bytes; 16-byte aligned.  The
 *                       decode reads its input to align_up(end, 16) + 16:
 *                       the bound's pool_cap covers that.
 *
 * Does nothing when totals[3] is not 0 on entry.  More literals than
 * lits_cap sets OVERFLOW_LITS and writes nothing; more Huffman bytes than
 * pool_cap sets OVERFLOW_POOL, lit_off is valid, and no pool byte is
 * written.  Three launches: the literals' lengths (a lane per record), a
 * one-workgroup scan into lit_off, and the copy: a wave takes 64 consecutive
 * records and copies their Huffman literals one after the other, its 64
 * lanes on consecutive bytes.
 *
 * Device pointers, asynchronous on `stream`.  A batch without Huffman
 * literals writes lit_off[0] = 0 and nothing else.  A NULL wire, ops,
 * totals, lit_off or pool is NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_gather_literals_batch(const uint8_t *wire, size_t wire_bytes,
                                                            const nghttp2_amd_hd_op *ops, size_t ops_cap,
                                                            uint32_t *totals, uint32_t *lit_off,
                                                            size_t lits_cap, uint8_t *pool, size_t pool_cap,
                                                            void *stream);

/* ------------------------------------------------------------------ */
/* Batched HPACK inflate front-end               */
/* ------------------------------------------------------------------ */
/*
 * An inflater is one connection's HPACK decoding context (dynamic table,
 * table size settings), as nghttp2_hd_inflater (lib/nghttp2_hd.h).
 * nghttp2_amd_hd_inflate_blocks decodes a batch of complete header blocks,
 * block i against inflaters[i] (blocks of one connection in order), with
 * every Huffman literal of the batch decoded in ONE GPU call.  Per block it
 * behaves as nghttp2_hd_inflate_hd3 (nghttp2.h:6623) called with in_final=1
 * until NGHTTP2_HD_INFLATE_FINAL, then nghttp2_hd_inflate_end_headers
 * (nghttp2.h:6636): the same fields, the same dynamic table evolution, the
 * same errors (NGHTTP2_ERR_HEADER_COMP, sticky per inflater).
 */
typedef struct nghttp2_amd_hd_inflater nghttp2_amd_hd_inflater;

/* One emitted header field: name and value are NUL-terminated byte strings
 * in the caller's arena; flags = NGHTTP2_NV_FLAG_NO_INDEX (1) for a
 * never-indexed literal (nghttp2.h:574-613). */
typedef struct {
  uint32_t block;
  uint32_t name_off, name_len;
  uint32_t value_off, value_len;
  uint8_t flags;
} nghttp2_amd_hd_nv;

/* nghttp2_hd_inflate_new (nghttp2.h:6277): dynamic table of 4096 bytes. */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_new(nghttp2_amd_hd_inflater **inflater_ptr);
/* nghttp2_hd_inflate_del (nghttp2.h:6302) */
NGHTTP2_AMD_EXTERN void nghttp2_amd_hd_inflate_del(nghttp2_amd_hd_inflater *inflater);
/* nghttp2_hd_inflate_change_table_size (nghttp2.h:6331): a smaller value
 * than the current maximum requires a size update at the head of the next
 * block.  After a block that failed in the middle of a representation (any
 * NGHTTP2_AMD_ERR_HEADER_COMP but that of a missing expected size update) it
 * returns NGHTTP2_AMD_ERR_INVALID_STATE and changes nothing, as the
 * reference's does for an inflater left where its block failed. */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_change_table_size(nghttp2_amd_hd_inflater *inflater,
                                             size_t settings_max_dynamic_table_size);
/* nghttp2_hd_inflate_get_num_table_entries / get_table_entry /
 * get_dynamic_table_size / get_max_dynamic_table_size (nghttp2.h:6646-6678);
 * idx is 1-based over static + dynamic table. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_inflate_get_num_table_entries(nghttp2_amd_hd_inflater *inflater);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_get_table_entry(nghttp2_amd_hd_inflater *inflater,
                                           size_t idx, const uint8_t **name, size_t *namelen,
                                           const uint8_t **value, size_t *valuelen);
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_inflate_get_dynamic_table_size(nghttp2_amd_hd_inflater *inflater);
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_inflate_get_max_dynamic_table_size(nghttp2_amd_hd_inflater *inflater);

/*
 * Inflate nblocks complete header blocks (host memory).  Fields go to
 * nva[0..*nva_used) in block order, their bytes to arena[0..*arena_used).
 * block_status[i] = fields of block i, or NGHTTP2_AMD_ERR_HEADER_COMP (the
 * fields before the error stay emitted, as the reference emits them one at
 * a time; the inflater turns bad), or NGHTTP2_AMD_ERR_BUFFER_ERROR when
 * nva / arena ran out (that block and the rest are not applied).  The GPU
 * work is asynchronous on `stream` and synchronised before return; a batch
 * without Huffman literals makes no GPU call.  The library keeps one
 * process-wide engine (pinned and device buffers, parse state) for this
 * call, so concurrent calls are serialised whole, host passes included; the
 * engine keeps its per-block buffers across calls and releases the surplus
 * when a call is far smaller than an earlier one.
 * A block is cut into its representations by the code that
 * nghttp2_amd_hd_parse_block runs (csrc/hd_parse.h).  A block_lens[i] above
 * UINT32_MAX is NGHTTP2_AMD_ERR_INVALID_ARGUMENT, as it is there, before any
 * inflater changes: the offsets of nghttp2_amd_hd_nv are uint32, so such a
 * block could not be answered.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_blocks(nghttp2_amd_hd_inflater *const *inflaters,
                                  uint32_t nblocks, const uint8_t *const *blocks,
                                  const size_t *block_lens, nghttp2_amd_hd_nv *nva,
                                  size_t nva_cap, size_t *nva_used, uint8_t *arena,
                                  size_t arena_cap, size_t *arena_used, int32_t *block_status,
                                  void *stream);

/*
 * nghttp2_amd_hd_inflate_blocks that also validates what it emits:
 * nv_checks[2 k] is the NGHTTP2_AMD_CHECK_* mask of field k's name,
 * nv_checks[2 k + 1] that of its value (2 * nva_cap bytes; the first
 * 2 * *nva_used are written, for a block that ends in
 * NGHTTP2_AMD_ERR_HEADER_COMP those of the fields emitted before the error).
 * Huffman literals are checked on the GPU right behind their decode
 * (nghttp2_amd_hd_check_fields_batch on the decode's output, one more launch
 * and one byte per literal more in the copy back), raw literals on the host
 * inside the replay, static-table entries once per process, dynamic-table
 * entries when they are inserted: an indexed field costs no byte scan.
 * nv_checks == NULL is nghttp2_amd_hd_inflate_blocks itself.  A
 * block_lens[i] above UINT32_MAX is NGHTTP2_AMD_ERR_INVALID_ARGUMENT, as there.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_blocks_checked(nghttp2_amd_hd_inflater *const *inflaters,
                                  uint32_t nblocks, const uint8_t *const *blocks,
                                  const size_t *block_lens, nghttp2_amd_hd_nv *nva,
                                  size_t nva_cap, size_t *nva_used, uint8_t *arena,
                                  size_t arena_cap, size_t *arena_used, int32_t *block_status,
                                  uint8_t *nv_checks, void *stream);

/*
 * nghttp2_amd_hd_inflate_blocks_checked that also hands every field over
 * with its name token, as nghttp2_hd_inflate_hd_nv sets nv.token
 * (lib/nghttp2_hd.c:1340, :1811): nv_tokens[k] = lookup_token of field k's
 * name (NGHTTP2_AMD_TOKEN_NONE or NGHTTP2_TOKEN_*; nva_cap entries, the first
 * *nva_used are written, for a block that ends in NGHTTP2_AMD_ERR_HEADER_COMP
 * those of the fields emitted before the error).  Huffman-coded names are
 * looked up on the GPU right behind their decode
 * (nghttp2_amd_hd_name_tokens_len_batch over the decode's output with no
 * hash: one more launch, behind the check launch when both are asked for,
 * and four bytes per literal more in the copy back), raw names on the host
 * inside the replay, static-table entries once per process; a dynamic-table
 * entry carries its name's token from insertion (or from its first tokened
 * reference, when a call without nv_tokens inserted it), so an indexed field
 * or an indexed name costs no lookup.  nv_checks and nv_tokens are
 * independent, either may be NULL: nv_tokens == NULL is
 * nghttp2_amd_hd_inflate_blocks_checked, both NULL is
 * nghttp2_amd_hd_inflate_blocks -- no token launch, no byte more in the
 * copies, no host lookup.  A block_lens[i] above UINT32_MAX is
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT, as for nghttp2_amd_hd_inflate_blocks.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_blocks_fields(nghttp2_amd_hd_inflater *const *inflaters,
                                  uint32_t nblocks, const uint8_t *const *blocks,
                                  const size_t *block_lens, nghttp2_amd_hd_nv *nva,
                                  size_t nva_cap, size_t *nva_used, uint8_t *arena,
                                  size_t arena_cap, size_t *arena_used, int32_t *block_status,
                                  uint8_t *nv_checks, int32_t *nv_tokens, void *stream);

/*
 * nghttp2_amd_hd_inflate_blocks_fields that also validates the HTTP message
 * each block carries, as the session does with nghttp2_http_on_header on
 * every field and a block-end function after the last (see "HTTP message
 * validation" above).  block_modes[i] (IN) is block i's
 * NGHTTP2_AMD_HTTP_MODE_* bits.  block_state[i] is IN-OUT: the caller puts in
 * the stream's state before the block (fresh, {0, -1, -1}, for a request; the
 * request's method flags for a response; what a 1xx block left behind for
 * the response after it) and the state after the block comes out.
 * nv_verdicts[k] (nva_cap entries, the first *nva_used written) is
 * nghttp2_amd_hd_http_on_header's result for field k, run in order on the
 * block's state.  After the first NGHTTP2_AMD_ERR_HTTP_HEADER of a block the
 * reference stops examining the stream (lib/nghttp2_session.c:3643-3664): the
 * block's later fields get NGHTTP2_AMD_HTTP_NOT_EXAMINED and the state stops
 * changing; those fields are still emitted and still enter the dynamic table.
 * block_http[i] is NGHTTP2_AMD_ERR_HTTP_HEADER if a field failed, else
 * NGHTTP2_AMD_ERR_HTTP_MESSAGING if the block-end function of the mode
 * (request or response; none for a TRAILER block) returns -1, else 0.  For a
 * block whose block_status is NGHTTP2_AMD_ERR_HEADER_COMP the fields emitted
 * before the error get verdicts and block_http[i] is
 * NGHTTP2_AMD_ERR_HEADER_COMP; a block cut off by
 * NGHTTP2_AMD_ERR_BUFFER_ERROR leaves its state untouched and gets that code
 * in block_http too.
 * The value facts come from where the masks and tokens come from: Huffman
 * literals from one nghttp2_amd_hd_http_facts_batch over the decode's output
 * (one more launch behind the check and token launches, twelve bytes per
 * literal more in the copy back), raw literals on the replay's thread,
 * static-table entries once per process; a dynamic-table entry carries its
 * value's facts from insertion, or from its first reference by an _http call
 * when another kind of call inserted it.  The call computes masks and tokens
 * internally whether or not nv_checks and nv_tokens are given.  nv_verdicts
 * and block_http may be NULL; block_modes and block_state are both needed
 * (else NGHTTP2_AMD_ERR_INVALID_ARGUMENT) unless all four are NULL, which is
 * nghttp2_amd_hd_inflate_blocks_fields itself: no launch, no byte more in
 * the copies, no host work.  A block_lens[i] above UINT32_MAX is
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT, as for nghttp2_amd_hd_inflate_blocks.
 */
#define NGHTTP2_AMD_HTTP_NOT_EXAMINED 1
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_inflate_blocks_http(nghttp2_amd_hd_inflater *const *inflaters,
                                  uint32_t nblocks, const uint8_t *const *blocks,
                                  const size_t *block_lens, nghttp2_amd_hd_nv *nva,
                                  size_t nva_cap, size_t *nva_used, uint8_t *arena,
                                  size_t arena_cap, size_t *arena_used, int32_t *block_status,
                                  uint8_t *nv_checks, int32_t *nv_tokens,
                                  const uint8_t *block_modes, nghttp2_amd_hd_http_state *block_state,
                                  int32_t *nv_verdicts, int32_t *block_http, void *stream);

/* ------------------------------------------------------------------ */
/* Device-resident inflaters: parsed blocks into fields on the GPU        */
/* ------------------------------------------------------------------ */
/*
 * The end of the chain nghttp2_amd_hd_parse_blocks_batch ->
 * nghttp2_amd_hd_gather_literals_batch -> nghttp2_amd_hd_huff_decode_batch_auto
 * for a caller whose wire lies in device memory: a set of HPACK decoding
 * contexts lives in device memory across calls, and one call turns a parsed
 * and decoded batch into nghttp2_amd_hd_nv fields and an arena in device
 * memory, with the results of nghttp2_amd_hd_inflate_blocks -- index
 * resolution against each connection's dynamic table, insertion with
 * eviction, the size update rules, the sticky bad state, the fields emitted up
 * to an error -- and advances the tables on the device.  The rules are stated
 * once, in csrc/hd_replay.h, for the kernels and for the host twin below.
 *
 * One connection's header.  The HPACK numbers are exact uint32 values
 * whatever the set's table_bytes is.
 *   max           the table limit in force (nghttp2's hd_table_bufsize_max)
 *   settings_max  the last nghttp2_hd_inflate_change_table_size value
 *   min_max       the smallest such value since the last size update
 *   size, count   the table's accounted size (32 bytes of overhead per entry)
 *                 and its entries
 *   head          the ring slot of the newest entry
 *   flags         NGHTTP2_AMD_HD_DEV_EXPECT_SIZE: the next block must open with
 *                 a size update; _BAD: a block failed, every later block
 *                 fails with no field; _MID_BLOCK: it failed outside the wait
 *                 for that size update, so a change of the table size is
 *                 NGHTTP2_AMD_ERR_INVALID_STATE
 *   cur           which of the connection's two store buffers is current
 * A ring slot is 16 bytes: {name offset, name length | 3 << 24, value offset,
 * value length | 3 << 24}, offsets into the connection's current store
 * buffer; entry i (0 the newest) is slot (head + i) mod (table_bytes / 32).
 */
typedef struct {
  uint32_t max, settings_max, min_max, size, count, head, flags, cur;
} nghttp2_amd_hd_dev_conn; /* 32 bytes */

#define NGHTTP2_AMD_HD_DEV_EXPECT_SIZE 0x1u
#define NGHTTP2_AMD_HD_DEV_BAD 0x2u
#define NGHTTP2_AMD_HD_DEV_MID_BLOCK 0x4u

/* out_totals[2] of a replay: 0, or why no field was written */
#define NGHTTP2_AMD_HD_DEV_OVERFLOW_NVA 0x1u   /* more fields than nva_cap */
#define NGHTTP2_AMD_HD_DEV_OVERFLOW_ARENA 0x2u /* more arena bytes than arena_cap */
#define NGHTTP2_AMD_HD_DEV_OVERFLOW_U32 0x4u   /* a total does not fit the uint32 offsets */

/*
 * nconn decoding contexts in device memory, each as nghttp2_hd_inflate_new
 * leaves one: maximum 4096, empty table.  Per connection the set holds the
 * header, a ring of table_bytes / 32 entry descriptors and two byte stores of
 * table_bytes (a call reads the entries that stay from one and writes the
 * table it leaves to the other).  table_bytes is a power of two, at least
 * 4096, and nconn * 2 * table_bytes at most UINT32_MAX.
 *
 * The capacity rule: table_bytes is the capacity per connection, not an HPACK
 * number.  When the HPACK maximum admits an entry whose insertion would take
 * the accounted size above table_bytes, the store cannot hold it: the block
 * ends there with NGHTTP2_AMD_ERR_NOMEM (the reference's result when its
 * allocation fails), the fields before it stay emitted, and the inflater
 * turns bad.  With table_bytes >= every settings value the peer is allowed,
 * this never happens.
 *
 * _new's initialisation is asynchronous on `stream`; _del frees the memory
 * (the caller has synchronised the streams that use the set).
 */
typedef struct nghttp2_amd_hd_dev_inflaters nghttp2_amd_hd_dev_inflaters;
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_inflaters_new(nghttp2_amd_hd_dev_inflaters **set_ptr, uint32_t nconn,
                                                        uint32_t table_bytes, void *stream);
NGHTTP2_AMD_EXTERN void nghttp2_amd_hd_dev_inflaters_del(nghttp2_amd_hd_dev_inflaters *set);

/*
 * nghttp2_hd_inflate_change_table_size for n connections: request i sets
 * connection conn[i]'s settings value to value[i] and leaves rv[i] = 0, or
 * NGHTTP2_AMD_ERR_INVALID_STATE with nothing changed when the connection
 * failed in the middle of a block, or NGHTTP2_AMD_ERR_INVALID_ARGUMENT for a
 * conn[i] >= nconn.  A value below the maximum in force lowers it, evicts,
 * and makes the next block's leading size update mandatory.  Device arrays,
 * one lane per request, asynchronous on `stream`.  Precondition: a
 * connection appears at most once in a call (two requests for one connection
 * would race; issue them in two calls).
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_inflaters_change_table_size(nghttp2_amd_hd_dev_inflaters *set,
                                                                      const uint32_t *conn, const uint32_t *value,
                                                                      int32_t *rv, uint32_t n, void *stream);

/*
 * One connection read back, for tests and debugging (synchronises `stream`):
 * *hdr is its header, bytes[table_bytes] its current store buffer, and
 * entries[4 i .. 4 i + 3] = {name offset, name length, value offset, value
 * length} into `bytes` for i < hdr->count, the newest entry first (room for
 * table_bytes / 32 entries).  Host pointers.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_inflaters_read(nghttp2_amd_hd_dev_inflaters *set, uint32_t conn,
                                                         nghttp2_amd_hd_dev_conn *hdr, uint32_t *entries,
                                                         uint8_t *bytes, void *stream);

/* The device workspace of nghttp2_amd_hd_dev_inflate_blocks: two counters per
 * block, 64 bytes and a ring of table_bytes / 32 descriptors per connection
 * (the call's insertions), and 32 bytes per record (the field references). */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_dev_inflate_workspace_size(uint32_t nconn, uint32_t table_bytes,
                                                                    size_t ops_cap, uint32_t nblocks);

/*
 * The replay of a parsed and decoded batch against the set's connections.
 *
 *   wire, wire_bytes, block_off[n+1], nblocks : the batch, as the parse got it
 *   op_off[n+1], ops, ops_cap, block_status[n], totals[4] : the parse's results
 *   dst, dst_bytes, dst_off, status, nlits : the decode's results for the
 *                       gathered literals: literal k is dst[dst_off[k],
 *                       +status[k]), failed when status[k] < 0.  dst_bytes is
 *                       dst's size (a reference past it is not read) and
 *                       nlits the number of strings the decode was run for,
 *                       that is, what dst_off and status hold: the parse's
 *                       totals[1] for a complete chain.  A literal numbered
 *                       nlits or above fails its field, so a count below
 *                       totals[1] costs fields, never a read past the
 *                       arrays.  With nlits == 0 none of the three is read.
 *   conn_blk_off[nconn+1], conn_blk[nblocks] : which blocks belong to which
 *                       connection: connection c's blocks are
 *                       conn_blk[conn_blk_off[c], conn_blk_off[c+1]) in the
 *                       order they are applied.  A block listed twice is the
 *                       caller's error (its results are undefined, no memory
 *                       outside the arrays is touched); a block not listed
 *                       emits no field and its out_status is not written.
 *   nva, nva_cap      : OUT: the fields, dense, in block order; `block` is the
 *                       block's index, the offsets are positions in arena
 *   arena, arena_cap  : OUT: name, NUL, value, NUL per field, back to back
 *   block_nv_off[n+1] : OUT: block i's fields are nva[block_nv_off[i],
 *                       block_nv_off[i+1])
 *   out_status[n]     : OUT: the block's number of fields,
 *                       NGHTTP2_AMD_ERR_HEADER_COMP (the fields before the
 *                       error are emitted and counted in block_nv_off) or
 *                       NGHTTP2_AMD_ERR_NOMEM (the capacity rule)
 *   out_totals[4]     : OUT: {fields, arena bytes,
 *                       NGHTTP2_AMD_HD_DEV_OVERFLOW_* bits, 0}
 *   workspace         : device scratch, >= the workspace size above
 *
 * Per block the results are nghttp2_amd_hd_inflate_blocks' on an inflater in
 * the same state (nghttp2_hd_inflate_hd3 with in_final, then
 * nghttp2_hd_inflate_end_headers): a block whose parse status is
 * NGHTTP2_AMD_ERR_HEADER_COMP fails behind its completed records, a literal
 * whose decode status is negative fails its field (the name is examined
 * before the value), index 0 or an index past 61 + entries fails, an entry
 * larger than the maximum empties the table and is not inserted.
 *
 * Overflow is all or nothing.  When the batch emits more fields than nva_cap
 * or more bytes than arena_cap, out_totals holds the sizes needed with the
 * bits set, nothing is written to nva or arena, and the tables are as before
 * the call: repeat it with room.  block_nv_off and out_status are valid
 * either way (not with OVERFLOW_U32).  nva_cap = ops_cap, or the parse's
 * totals[0], cannot overflow; the arena has no useful a-priori bound (an
 * indexed field of one wire byte emits its entry's bytes).
 *
 * A clear of the block counters and four launches: k_replay (one lane per
 * connection walks its blocks; no byte moves: every name and value is a
 * reference into the static table, the wire, the decode's output or the
 * connection's store), a one-workgroup scan, k_emit (a wave per 64 records:
 * the nghttp2_amd_hd_nv of each, then the strings with the lanes on
 * consecutive bytes) and k_commit (a wave per connection that had blocks
 * rewrites its table into its other store buffer).  k_emit's grid covers
 * ops_cap records, because the count is known on the device only: a workgroup
 * past the parse's totals[0] returns at once, and an ops_cap close to the
 * batch's records is cheaper than the parse's bound.  The counts are read from
 * totals on the device, so the call follows parse, gather and decode on the
 * stream with no host synchronisation; it does nothing when totals[3] is not
 * 0 on entry.
 *
 * Device pointers, asynchronous on `stream`; calls on one set are ordered by
 * the caller (one stream, or events).  nblocks == 0 returns 0 and touches
 * nothing.  A NULL set, wire, block_off, op_off, ops, block_status, totals,
 * dst, dst_off, status, conn_blk_off, conn_blk, nva (with nva_cap > 0), arena
 * (with arena_cap > 0), block_nv_off, out_status, out_totals or workspace, or
 * a workspace below the size above, is NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_inflate_blocks(
    nghttp2_amd_hd_dev_inflaters *set, const uint8_t *wire, size_t wire_bytes, const uint32_t *block_off,
    uint32_t nblocks, const uint32_t *op_off, const nghttp2_amd_hd_op *ops, size_t ops_cap,
    const int32_t *block_status, const uint32_t *totals, const uint8_t *dst, size_t dst_bytes,
    const uint32_t *dst_off, const int32_t *status, uint32_t nlits, const uint32_t *conn_blk_off,
    const uint32_t *conn_blk, nghttp2_amd_hd_nv *nva, size_t nva_cap, uint8_t *arena, size_t arena_cap, uint32_t *block_nv_off,
    int32_t *out_status, uint32_t *out_totals, void *workspace, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ */
/* Device-resident inflaters: masks, tokens and HTTP verdicts on the GPU  */
/* ------------------------------------------------------------------ */
/*
 * What nghttp2_amd_hd_inflate_blocks_http adds to nghttp2_amd_hd_inflate_blocks,
 * for the fields nghttp2_amd_hd_dev_inflate_blocks left in device memory.  The
 * call follows the replay on the stream and reads no count on the host.
 *
 *   nva, nva_cap, arena, block_nv_off[n+1], out_status[n], out_totals[4],
 *   nblocks           : IN: the replay's outputs, as it left them
 *   arena_bytes       : the arena's allocation (see the pool rule below)
 *   nv_checks         : OUT, 2 * nva_cap bytes or NULL: nv_checks[2 k] is the
 *                       NGHTTP2_AMD_CHECK_* mask of field k's name,
 *                       nv_checks[2 k + 1] that of its value
 *   nv_tokens         : OUT, nva_cap int32 or NULL: lookup_token of field k's
 *                       name (NGHTTP2_AMD_TOKEN_NONE or NGHTTP2_TOKEN_*)
 *   block_modes[n]    : IN: block i's NGHTTP2_AMD_HTTP_MODE_* bits
 *   block_state[n]    : IN-OUT: the stream's state before block i, and after
 *   nv_verdicts       : OUT, nva_cap int32 or NULL: field k's
 *                       nghttp2_amd_hd_http_on_header result, run in order on
 *                       its block's state
 *   block_http[n]     : OUT or NULL: the block's result
 *   workspace         : device scratch, 16-byte aligned, >= the size below
 *
 * The results are nghttp2_amd_hd_inflate_blocks_http's for the same fields:
 * of every array the entries of the out_totals[0] emitted fields are written
 * and no other.  After a block's first NGHTTP2_AMD_ERR_HTTP_HEADER its later
 * fields get NGHTTP2_AMD_HTTP_NOT_EXAMINED and the state stops changing.
 * block_http[i] is NGHTTP2_AMD_ERR_HTTP_HEADER if a field failed, else
 * NGHTTP2_AMD_ERR_HTTP_MESSAGING if the block-end function of the mode
 * (request or response; none for a TRAILER block) returns -1, else 0.  A block
 * whose out_status is negative (NGHTTP2_AMD_ERR_HEADER_COMP, or the capacity
 * rule's NGHTTP2_AMD_ERR_NOMEM) gets verdicts for the fields it emitted, no
 * block end, and that status in block_http.
 * The NULL rules are the host call's: nv_checks and nv_tokens are
 * independent; nv_verdicts and block_http may be NULL; block_modes and
 * block_state are both needed (else NGHTTP2_AMD_ERR_INVALID_ARGUMENT) unless
 * all four are NULL, which computes masks and/or tokens only (no facts launch,
 * no step).  An HTTP call computes masks and tokens in the workspace whether
 * or not nv_checks and nv_tokens are given.  With all six NULL nothing is
 * queued.
 *
 * Specific to the device:
 * - When out_totals[2] != 0 on entry the replay wrote no field: the call
 *   writes nothing and changes no state.  The test is made on the device.
 *   (out_totals is the replay's output: a replay that did nothing because the
 *   parse's totals[3] was set wrote none, so the caller clears out_totals, or
 *   sets out_totals[2], ahead of such a chain.)
 * - A block that no connection listed in the replay's conn_blk has undefined
 *   results (its out_status was never written); no memory outside the arrays
 *   is touched whatever the records hold.
 * - The pool rule of the three batch kernels: arena is 16-byte aligned and
 *   readable to align_up(out_totals[1], 16) + 16, and arena_bytes says how far
 *   it is readable.  When arena_bytes is smaller than that (and the batch has
 *   a field), no string is examined, nothing is written and no state changes.
 *
 * The workspace opens with a totals word, four uint32 the call's first kernel
 * writes: {the fields examined, their arena bytes, NGHTTP2_AMD_HD_DEV_FIELDS_*
 * bits, 0}; with a bit set the first two are 0.
 * nghttp2_amd_hd_dev_fields_http_totals copies it to the host (synchronises
 * `stream`).  Behind it, each part rounded up to 16 bytes, with c = nva_cap:
 *   the interleaved view   uint32[2 c + 1] offsets, int32[2 c] lengths
 *   the names view         uint32[c + 1], int32[c]
 *   the values view        uint32[c + 1], int32[c]
 *   the values' numbers    int64[c]
 *   the values' facts      uint32[c]
 *   the names' tokens      int32[c]
 *   the masks              uint8[2 c]
 * (nblocks adds nothing: no scratch is kept per block.)
 *
 * Up to six launches: k_field_views (a lane per field slot writes the three
 * views: a slot at or past the field count gets offset = arena bytes and
 * length -1, a string the batch kernels do not examine),
 * nghttp2_amd_hd_check_fields_batch on the interleaved view,
 * nghttp2_amd_hd_name_tokens_len_batch (no hash) on the names, k_field_publish
 * (the masks and tokens of the emitted fields to nv_checks and nv_tokens; the
 * batch kernels write every slot they are launched for, so they write to the
 * workspace), nghttp2_amd_hd_http_facts_batch on the values, and
 * k_http_blocks (a lane per block runs the step of csrc/hd_http.h over its
 * fields and the block end behind them).  The grids are sized from nva_cap
 * and nblocks; a workgroup past the field count does next to nothing.
 *
 * Device pointers, asynchronous on `stream`.  nblocks == 0 returns 0 and
 * touches nothing.  A NULL nva or arena (with nva_cap > 0), block_nv_off,
 * out_status, out_totals or workspace, an arena or workspace that is not
 * 16-byte aligned, an nva_cap above INT32_MAX, or a workspace below the size
 * is NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 */
#define NGHTTP2_AMD_HD_DEV_FIELDS_NOT_REPLAYED 0x1u /* out_totals[2] was set: the replay wrote no field */
#define NGHTTP2_AMD_HD_DEV_FIELDS_ARENA_SHORT 0x2u  /* arena_bytes is below the pool rule */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_dev_fields_http_workspace_size(size_t nva_cap, uint32_t nblocks);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_fields_http(
    const nghttp2_amd_hd_nv *nva, size_t nva_cap, const uint8_t *arena, size_t arena_bytes,
    const uint32_t *block_nv_off, const int32_t *out_status, const uint32_t *out_totals, uint32_t nblocks,
    uint8_t *nv_checks, int32_t *nv_tokens, const uint8_t *block_modes, nghttp2_amd_hd_http_state *block_state,
    int32_t *nv_verdicts, int32_t *block_http, void *workspace, size_t ws_bytes, void *stream);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_fields_http_totals(const void *workspace, uint32_t *totals, void *stream);

/*
 * The host twin (no GPU call): the same walk over host arrays with the same
 * layouts, for ONE connection whose blocks are the batch's, in order.  hdr is
 * the connection's header (nghttp2_amd_hd_replay_host_init makes a fresh
 * one), ring its table_bytes / 32 slots of 16 bytes, store its two buffers
 * (2 * table_bytes).  ops[op_off[i], op_off[i+1]) are block i's records with
 * offsets into wire; nlits bounds the literal numbers (dst, dst_off and
 * status may be NULL when it is 0; hdr, ring, store, wire, ops and the offset
 * and output arrays may not).  Outputs, the overflow rule and the commit
 * are the device call's.  _change_table_size is one request of the device
 * call's, returning its rv.
 */
NGHTTP2_AMD_EXTERN void nghttp2_amd_hd_replay_host_init(nghttp2_amd_hd_dev_conn *hdr);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_replay_host_change_table_size(nghttp2_amd_hd_dev_conn *hdr, const void *ring,
                                                                    uint32_t table_bytes, uint32_t value);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_replay_host(
    nghttp2_amd_hd_dev_conn *hdr, void *ring, uint8_t *store, uint32_t table_bytes, const uint8_t *wire,
    size_t wire_bytes, const uint32_t *block_off, uint32_t nblocks, const uint32_t *op_off,
    const nghttp2_amd_hd_op *ops, const int32_t *block_status, const uint8_t *dst, const uint32_t *dst_off,
    const int32_t *status, uint32_t nlits, nghttp2_amd_hd_nv *nva, size_t nva_cap, uint8_t *arena,
    size_t arena_cap, uint32_t *block_nv_off, int32_t *out_status, uint32_t *out_totals);

/* ------------------------------------------------------------------ */
/* Device-resident deflaters: header lists to wire on the GPU             */
/* ------------------------------------------------------------------ */
/*
 * The counterpart of the device-resident inflaters: a set of HPACK encoding
 * contexts lives in device memory across calls, and one call turns a batch of
 * header lists that lie in device memory -- in exactly the layout
 * nghttp2_amd_hd_dev_inflate_blocks emits -- into wire in device memory.  Per
 * block the wire, and the table after it, are nghttp2_hd_deflate_hd2's
 * (nghttp2.h:6127) on a deflater in the same state.  The rules are stated once,
 * in csrc/hd_deflate_plan.h, for the kernels and for the host twin below.
 *
 * A connection's header is the inflaters' nghttp2_amd_hd_dev_conn: max is the
 * table limit in force (hd_table_bufsize_max), settings_max the connection's
 * deflate_hd_table_bufsize_max, min_max the smallest limit since the last
 * block; size, count, head and cur as there; flags holds
 * NGHTTP2_AMD_HD_DEV_NOTIFY (notify_table_size_change: the next block opens
 * with the pending size updates).  Beside the ring of 16-byte descriptors a
 * connection keeps a parallel array of uint32 keys, the FNV-1a hash of each
 * entry's name: the search's filter (a match is always confirmed on the bytes).
 */
#define NGHTTP2_AMD_HD_DEV_NOTIFY 0x8u

/* One field's plan: the representation bytes in front of its string literals
 * (0x80 | index; 0x40 / 0x00 / 0x10 with a 6- or 4-bit name index or 0), how
 * many, and which of name and value follow as literals (emit_string's
 * framing).  block: the block the field was walked in. */
typedef struct {
  uint8_t bytes[6];
  uint8_t nbytes;
  uint8_t lits; /* NGHTTP2_AMD_HD_PLAN_LIT_* */
  uint32_t block;
  uint32_t reserved; /* 0 */
} nghttp2_amd_hd_plan_rec; /* 16 bytes */
#define NGHTTP2_AMD_HD_PLAN_LIT_NAME 0x1u
#define NGHTTP2_AMD_HD_PLAN_LIT_VALUE 0x2u
/* One block's head: the pending table size updates (at most two integers of 6
 * bytes with the 5-bit prefix and 0x20). */
typedef struct {
  uint8_t bytes[12];
  uint8_t nbytes;
  uint8_t reserved[3]; /* 0 */
} nghttp2_amd_hd_plan_head; /* 16 bytes */

/* out_totals[2] of a device deflate: 0, or why no wire was written */
#define NGHTTP2_AMD_HD_DEV_OVERFLOW_WIRE 0x1u /* more wire bytes than out_cap */
#define NGHTTP2_AMD_HD_DEV_OVERFLOW_POOL 0x2u /* more literal bytes than arena_bytes (strings that overlap) */
/* NGHTTP2_AMD_HD_DEV_OVERFLOW_U32 (0x4): a total does not fit the uint32 offsets */

/*
 * nconn encoding contexts in device memory, each as nghttp2_hd_deflate_new2
 * (lib/nghttp2_hd.c:721-748) leaves one for deflate_max[c] (a host array of
 * nconn values, or NULL for 4096 each): max = min(4096, deflate_max), an empty
 * table, and NOTIFY set when deflate_max < 4096.  table_bytes follows the
 * inflaters' rules (a power of two, at least 4096, nconn * 2 * table_bytes at
 * most UINT32_MAX) and there is no capacity error: every deflate_max[c] must be
 * at most table_bytes (else NGHTTP2_AMD_ERR_INVALID_ARGUMENT), so the store
 * holds whatever the limit admits.  _new copies the headers on `stream` and
 * waits for the copy; _del frees the memory (the caller has synchronised the
 * streams that use the set).
 */
typedef struct nghttp2_amd_hd_dev_deflaters nghttp2_amd_hd_dev_deflaters;
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_deflaters_new(nghttp2_amd_hd_dev_deflaters **set_ptr, uint32_t nconn,
                                                        uint32_t table_bytes, const uint32_t *deflate_max,
                                                        void *stream);
NGHTTP2_AMD_EXTERN void nghttp2_amd_hd_dev_deflaters_del(nghttp2_amd_hd_dev_deflaters *set);

/*
 * nghttp2_hd_deflate_change_table_size (lib/nghttp2_hd.c:1274-1288) for n
 * connections: request i sets connection conn[i]'s limit to min(value[i],
 * deflate_max), lowers min_max to it, sets NOTIFY and evicts; rv[i] = 0, or
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT for a conn[i] >= nconn.  Device arrays, one
 * lane per request, asynchronous on `stream`; a connection appears at most once
 * in a call.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_deflaters_change_table_size(nghttp2_amd_hd_dev_deflaters *set,
                                                                      const uint32_t *conn, const uint32_t *value,
                                                                      int32_t *rv, uint32_t n, void *stream);
/* One connection read back, as nghttp2_amd_hd_dev_inflaters_read (synchronises
 * `stream`; host pointers). */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_deflaters_read(nghttp2_amd_hd_dev_deflaters *set, uint32_t conn,
                                                         nghttp2_amd_hd_dev_conn *hdr, uint32_t *entries,
                                                         uint8_t *bytes, void *stream);

/* The device workspace of nghttp2_amd_hd_dev_deflate_blocks: per field slot a
 * plan record, the name view, token and hash, two literal slots and the wire
 * lengths; per block a head; per connection 64 bytes and a ring of table_bytes
 * / 32 descriptors and keys (the call's insertions); the literal pool
 * (arena_bytes and the pool rule's slack) and the framed literals
 * (nghttp2_amd_hd_emit_strings_bound(arena_bytes, 2 * nva_cap)) with
 * emit_strings' own workspace. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_dev_deflate_workspace_size(uint32_t nconn, uint32_t table_bytes,
                                                                    size_t nva_cap, size_t arena_bytes,
                                                                    uint32_t nblocks);

/*
 * A batch of header lists against the set's connections, into wire.
 *
 *   nva, nva_cap      : IN: nghttp2_amd_hd_nv records (name_off, name_len,
 *                       value_off, value_len into arena; flags & 1 is
 *                       NGHTTP2_NV_FLAG_NO_INDEX; `block` is not read), room
 *                       for nva_cap of them
 *   arena, arena_bytes: IN: the strings, and how far arena is readable
 *   block_nv_off[n+1] : IN: block i's fields are nva[block_nv_off[i],
 *                       block_nv_off[i+1]); block_nv_off[n], the field count,
 *                       is read on the device (fields at or past nva_cap are
 *                       not deflated)
 *   conn_blk_off[nconn+1], conn_blk[nblocks] : as for the inflaters: a block
 *                       listed twice is the caller's error (undefined results,
 *                       no memory outside the arrays touched); a block not
 *                       listed produces no wire and status 0
 *   out, out_cap      : OUT: the wire, the blocks back to back in block order
 *   out_off[n+1]      : OUT: block i's wire is out[out_off[i], out_off[i+1])
 *   out_status[n]     : OUT: the block's wire bytes
 *   out_totals[4]     : OUT: {wire bytes, literal pool bytes,
 *                       NGHTTP2_AMD_HD_DEV_OVERFLOW_* bits, 0}
 *   workspace         : device scratch, 16-byte aligned, >= the size above
 *
 * This is the layout nghttp2_amd_hd_dev_inflate_blocks leaves (name, NUL,
 * value, NUL per field in field order), so inflate -> (rewrite) -> deflate
 * never leaves the device.  A string must lie inside arena_bytes and be at
 * most 0xFFFFFF bytes, else it is deflated as an empty string.  The names'
 * tokens and hashes come from one nghttp2_amd_hd_name_tokens_len_batch launch
 * over the names, which examines a name when the names lie at non-decreasing
 * offsets, a field's name ends before the next field's begins, and arena is
 * 16-byte aligned and arena_bytes covers the pool rule's slack behind the last
 * name (align_up(end, 16) + 16); a name it does not examine is hashed and
 * looked up by the plan kernel itself, with the same result, only slower.
 *
 * Overflow is all or nothing, as for the inflaters: when the wire is larger
 * than out_cap (OVERFLOW_WIRE: out_totals[0] is the need), the literals are
 * more than arena_bytes (OVERFLOW_POOL, possible only with strings that
 * overlap: out_totals[1] is the need, out_totals[0] is not), or a total passes
 * uint32, nothing is written to out and every table is as before the call:
 * repeat it with room.  out_off and out_status are valid with OVERFLOW_WIRE
 * alone.  out_cap = 12 * nblocks + 12 * nva_cap + arena_bytes
 * (nghttp2_hd_deflate_bound summed) cannot overflow.  There is no bad state:
 * the reference's only deflate failures are allocation and buffer size.
 *
 * One clear and ten to twelve launches: the name view, the names' tokens and
 * hashes, k_deflate_plan (a wave per connection: the fields in order, the
 * lanes on 64 table entries at a time), the literal slots' scan and gather
 * (two slots per field slot, an unused one the empty string),
 * nghttp2_amd_hd_emit_strings_batch on them as it is, the fields' wire
 * lengths, a one-workgroup scan into out_off, k_place_wire (a wave per 64
 * fields) and k_commit (a wave per connection that had blocks).  Nothing is
 * read on the host.
 *
 * Device pointers, asynchronous on `stream`; calls on one set are ordered by
 * the caller.  nblocks == 0 returns 0 and touches nothing.  A NULL set, nva or
 * arena (with nva_cap > 0), block_nv_off, conn_blk_off, conn_blk, out (with
 * out_cap > 0), out_off, out_status, out_totals or workspace, an arena or a
 * workspace that is not 16-byte aligned, a workspace below the size above, an
 * nva_cap above 0x3FFFFFFF or an arena_bytes above UINT32_MAX is
 * NGHTTP2_AMD_ERR_INVALID_ARGUMENT.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_dev_deflate_blocks(
    nghttp2_amd_hd_dev_deflaters *set, const nghttp2_amd_hd_nv *nva, size_t nva_cap, const uint8_t *arena,
    size_t arena_bytes, const uint32_t *block_nv_off, uint32_t nblocks, const uint32_t *conn_blk_off,
    const uint32_t *conn_blk, uint8_t *out, size_t out_cap, uint32_t *out_off, int32_t *out_status,
    uint32_t *out_totals, void *workspace, size_t ws_bytes, void *stream);

/*
 * The host twin (no GPU call): the same walk over host arrays, for ONE
 * connection whose blocks are the batch's, in order.  hdr is the connection's
 * header (_init makes one as _new does), ring its table_bytes / 32 slots of 16
 * bytes, keys its table_bytes / 32 uint32, store its two buffers (2 *
 * table_bytes); deflate_max must be at most table_bytes.  recs[block_nv_off[n]]
 * and heads[n] receive the plan; the table is committed as the device call
 * commits it.  The wire of block i is heads[i]'s bytes, then per field its
 * record's bytes, the framed name when LIT_NAME is set and the framed value
 * when LIT_VALUE is.  _change_table_size is one request of the device call's.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_plan_host_init(nghttp2_amd_hd_dev_conn *hdr, uint32_t table_bytes,
                                                             uint32_t deflate_max);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_plan_host_change_table_size(nghttp2_amd_hd_dev_conn *hdr,
                                                                          const void *ring, uint32_t table_bytes,
                                                                          uint32_t value);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_plan_host(nghttp2_amd_hd_dev_conn *hdr, void *ring, uint32_t *keys,
                                                        uint8_t *store, uint32_t table_bytes,
                                                        const nghttp2_amd_hd_nv *nva, const uint8_t *arena,
                                                        size_t arena_bytes, const uint32_t *block_nv_off,
                                                        uint32_t nblocks, nghttp2_amd_hd_plan_rec *recs,
                                                        nghttp2_amd_hd_plan_head *heads);

/* ------------------------------------------------------------------ */
/* Batched HPACK deflate front-end                                      */
/* ------------------------------------------------------------------ */
/*
 * A deflater is one connection's HPACK encoding context (nghttp2_hd_deflater,
 * lib/nghttp2_hd.h).  nghttp2_amd_hd_deflate_blocks encodes a batch of
 * header lists, list i with deflaters[i] (lists of one connection in
 * order); every string literal of the batch is framed by ONE GPU call
 * (nghttp2_amd_hd_emit_strings_batch).  Block i's wire is byte-identical to
 * nghttp2_hd_deflate_hd2 (nghttp2.h:6127) on the same deflater state:
 * the same table size updates, table search, indexing decisions (never
 * index authorization, cookies shorter than 20 bytes and NO_INDEX fields;
 * no indexing for :path, age, content-length, etag, if-modified-since,
 * if-none-match, location, set-cookie and entries over 3/4 of the table)
 * and the same Huffman-or-raw literals.
 */
typedef struct nghttp2_amd_hd_deflater nghttp2_amd_hd_deflater;

/* Same layout as nghttp2_nv (nghttp2.h:574-613); flags bit 0 =
 * NGHTTP2_NV_FLAG_NO_INDEX. */
typedef struct {
  const uint8_t *name;
  const uint8_t *value;
  size_t namelen;
  size_t valuelen;
  uint8_t flags;
} nghttp2_amd_nv;

/* nghttp2_hd_deflate_new (nghttp2.h:6003) */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_new(nghttp2_amd_hd_deflater **deflater_ptr,
                               size_t max_deflate_dynamic_table_size);
/* nghttp2_hd_deflate_del (nghttp2.h:6031) */
NGHTTP2_AMD_EXTERN void nghttp2_amd_hd_deflate_del(nghttp2_amd_hd_deflater *deflater);
/* nghttp2_hd_deflate_change_table_size (nghttp2.h:6057) */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_change_table_size(nghttp2_amd_hd_deflater *deflater,
                                             size_t settings_max_dynamic_table_size);
/* nghttp2_hd_deflate_get_num_table_entries / get_table_entry /
 * get_dynamic_table_size (nghttp2.h:6221-6253); idx is 1-based. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_deflate_get_num_table_entries(nghttp2_amd_hd_deflater *deflater);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_get_table_entry(nghttp2_amd_hd_deflater *deflater,
                                           size_t idx, const uint8_t **name, size_t *namelen,
                                           const uint8_t **value, size_t *valuelen);
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_deflate_get_dynamic_table_size(nghttp2_amd_hd_deflater *deflater);
/* nghttp2_hd_deflate_get_max_dynamic_table_size (nghttp2.h:6253) */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_deflate_get_max_dynamic_table_size(nghttp2_amd_hd_deflater *deflater);
/* nghttp2_hd_deflate_bound (nghttp2.h:6209): an upper bound of one list's
 * wire; the sum over a batch bounds out_cap. */
NGHTTP2_AMD_EXTERN size_t nghttp2_amd_hd_deflate_bound(nghttp2_amd_hd_deflater *deflater,
                                    const nghttp2_amd_nv *nva, size_t nvlen);

/*
 * Deflate nblocks header lists (host memory): list i is
 * nva[block_nv_off[i]..block_nv_off[i+1]).  Block i's wire is
 * out[out_off[i]..out_off[i+1]); block_status[i] = its length, or
 * NGHTTP2_AMD_ERR_HEADER_COMP for a deflater already bad, or
 * NGHTTP2_AMD_ERR_BUFFER_ERROR when out_cap ran out (the deflater turns bad,
 * as nghttp2_hd_deflate_hd2's INSUFF_BUFSIZE does).  The GPU work is
 * asynchronous on `stream` and synchronised before return.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_deflate_blocks(nghttp2_amd_hd_deflater *const *deflaters,
                                  uint32_t nblocks, const nghttp2_amd_nv *nva,
                                  const uint32_t *block_nv_off, uint8_t *out, size_t out_cap,
                                  uint32_t *out_off, int32_t *block_status, void *stream);

/*
 * One header list into a caller buffer, as nghttp2_hd_deflate_hd2
 * (nghttp2.h:6127; lib/nghttp2_hd.c:1525-1555): the wire length, or
 * NGHTTP2_AMD_ERR_INSUFF_BUFSIZE when buflen is too small (the deflater
 * turns bad, as the reference's does), or NGHTTP2_AMD_ERR_HEADER_COMP for a
 * deflater already bad.  A batch of one list on nghttp2_amd_hd_deflate_blocks
 * (its literals framed by the GPU); host buffers, synchronous.
 */
NGHTTP2_AMD_EXTERN ptrdiff_t nghttp2_amd_hd_deflate_hd2(nghttp2_amd_hd_deflater *deflater,
                                                         uint8_t *buf, size_t buflen,
                                                         const nghttp2_amd_nv *nva, size_t nvlen,
                                                         void *stream);

/* Same layout as nghttp2_vec (nghttp2.h:5910-5919). */
typedef struct {
  uint8_t *base;
  size_t len;
} nghttp2_amd_vec;

/*
 * nghttp2_hd_deflate_hd_vec2 (nghttp2.h:6179; lib/nghttp2_hd.c:1563-1594):
 * as nghttp2_amd_hd_deflate_hd2, the wire written across the chunks
 * vec[0..veclen) in order (each filled before the next); INSUFF_BUFSIZE when
 * their total is too small, including veclen == 0 and zero-length chunks.
 * On INSUFF_BUFSIZE with several chunks, none of them is written (the
 * reference leaves the bytes it had written before it ran out).
 */
NGHTTP2_AMD_EXTERN ptrdiff_t nghttp2_amd_hd_deflate_hd_vec2(nghttp2_amd_hd_deflater *deflater,
                                                             const nghttp2_amd_vec *vec,
                                                             size_t veclen,
                                                             const nghttp2_amd_nv *nva,
                                                             size_t nvlen, void *stream);

/*
 * The HPACK prefix-integer decoder the inflate front-end parses with, as
 * nghttp2_hd_decode_length (lib/nghttp2_hd.h:416-419; lib/nghttp2_hd.c:
 * 882-945), resumable byte by byte: decode from in[0..last - in) with a
 * `prefix`-bit first byte, continuing a previous call's partial value
 * `initial` at `shift` (both 0 at the start of an integer).  Returns the
 * bytes consumed, or -1 on overflow past UINT32_MAX (a shift of 32 bits or
 * more included); *fin = 1 once the integer is complete (*res its value),
 * else *res and *shift_ptr carry the partial state to the next call.
 * Host-only.
 */
NGHTTP2_AMD_EXTERN ptrdiff_t nghttp2_amd_hd_decode_length(uint32_t *res, size_t *shift_ptr, int *fin,
                                                           uint32_t initial, size_t shift,
                                                           const uint8_t *in, const uint8_t *last,
                                                           size_t prefix);

/* ------------------------------------------------------------------ */
/* One batch over several GPUs                       */
/* ------------------------------------------------------------------ */
/*
 * Strings are independent, so a batch shards into contiguous string ranges
 * balanced by bytes, one per device, with no exchange between devices (no
 * RCCL, xGMI unused).  A sharded engine owns one host worker thread, one HIP
 * stream and its own device buffers per entry of its device list (a device
 * may repeat: several shards on one GPU); the table of each kernel is staged
 * per device.  This is nghttp2's concurrency model (one session per thread,
 * nothing shared; doc/programmers-guide.rst:35-40) with a GPU behind each
 * thread.  A sharded engine is used by one caller thread at a time; distinct
 * engines may run concurrently.
 *
 * The shard outputs are merged into one batch: shard k's output bytes follow
 * shard k-1's, and its offsets are rebased by the bytes before it.  Encode:
 * the result equals nghttp2_amd_hd_huff_encode_batch of the whole batch.
 * Decode: each shard is laid out as nghttp2_amd_hd_huff_decode_batch_auto
 * lays out a batch of its strings (dense per task, counted from the shard's
 * first string), shifted by the bytes of the shards before it; dst_off,
 * status, fstate and flags are per string as for the unsharded call.
 */
typedef struct nghttp2_amd_hd_sharded nghttp2_amd_hd_sharded;

/* Byte-balanced contiguous cut of a batch of n strings (offsets off[n+1])
 * into nshards ranges: cuts[0] = 0, cuts[nshards] = n, shard k holds the
 * strings [cuts[k], cuts[k+1]), which start at or after its 1/nshards share
 * of the bytes.  Host-only.  Returns 0 or NGHTTP2_AMD_ERR_INVALID_ARGUMENT. */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_shard_bounds(const uint32_t *off, uint32_t n, uint32_t nshards,
                                                   uint32_t *cuts);

/* A sharded engine over ndevices HIP device ids (repeats allowed).  Returns
 * 0, NGHTTP2_AMD_ERR_INVALID_ARGUMENT (no device, an id out of range) or
 * NGHTTP2_AMD_ERR_FATAL / _NOMEM (a stream or thread could not be made). */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_sharded_new(nghttp2_amd_hd_sharded **out, const int *devices,
                                                  uint32_t ndevices);
NGHTTP2_AMD_EXTERN void nghttp2_amd_hd_sharded_del(nghttp2_amd_hd_sharded *s);
NGHTTP2_AMD_EXTERN uint32_t nghttp2_amd_hd_sharded_count(const nghttp2_amd_hd_sharded *s);

/*
 * Host-resident batch (pinned memory gives the full PCIe rate; pageable
 * memory works and copies through the runtime's staging).  src must be
 * readable to align_up(src_off[n], 16) + 16 (the pool padding of every batch
 * call).  Each shard: H2D of its bytes and offsets, the engine kernels, D2H
 * of its output straight to its merged position.  Synchronous: returns when
 * every shard's output is in dst.
 *
 * encode: Huffman encode; dst_off[n+1] merged (dst_off[0] = 0).  When the
 *   merged output passes dst_cap or the uint32 offsets, nothing is written to
 *   dst, dst_off[n] = NGHTTP2_AMD_OFF_OVERFLOW and the call returns
 *   NGHTTP2_AMD_ERR_BUFFER_ERROR (split the batch).
 * decode: decode with final=1 (status per string as decode_batch_auto);
 *   dst_cap >= nghttp2_amd_hd_huff_decode_bound(E, n) + 32 * shards always
 *   suffices (E = src_off[n] - src_off[0]); a smaller pool that the merged
 *   output does not fit returns NGHTTP2_AMD_ERR_BUFFER_ERROR with nothing
 *   written to dst.  fstate and flags may both be NULL.
 */
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_sharded_encode(nghttp2_amd_hd_sharded *s, const uint8_t *src,
                                                     const uint32_t *src_off, uint32_t n, uint8_t *dst,
                                                     size_t dst_cap, uint32_t *dst_off);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_sharded_decode(nghttp2_amd_hd_sharded *s, const uint8_t *src,
                                                     const uint32_t *src_off, uint32_t n, uint8_t *dst,
                                                     size_t dst_cap, uint32_t *dst_off, int32_t *status,
                                                     uint16_t *fstate, uint8_t *flags);

/*
 * Device-resident shards: shards[k] lives on the engine's k-th device (cut
 * by the caller, e.g. with nghttp2_amd_hd_shard_bounds; its src_off may be
 * absolute or rebased -- the engine calls take them as given).  Each shard
 * runs nghttp2_amd_hd_huff_encode_batch / _decode_batch_auto on its device
 * and stream; its output stays there with shard-local offsets, and the
 * engine reports out_bytes (its dst_off[n]) and out_base (the bytes of the
 * shards before it, its position in the merged batch).  Synchronous.
 * Returns 0 or the first failing shard's error (each shard's own in rv).
 */
typedef struct {
  const uint8_t *src;        /* IN  pool on the shard's device (16-byte aligned, padded) */
  const uint32_t *src_off;   /* IN  offsets[n+1] on the shard's device */
  uint32_t n;                /* IN  strings of the shard */
  uint64_t in_bytes;         /* IN  decode: src_off[n] - src_off[0]; encode: raw bytes */
  uint8_t *dst;              /* IN  output pool on the shard's device */
  size_t dst_cap;            /* IN */
  uint32_t *dst_off;         /* IN  offsets[n+1] on the shard's device */
  int32_t *status;           /* IN  decode: status[n] on the device (encode: unused) */
  uint16_t *fstate;          /* IN  decode: optional (with flags) */
  uint8_t *flags;            /* IN  decode: optional (with fstate) */
  uint64_t out_bytes;        /* OUT the shard's output bytes (dst_off[n]) */
  uint64_t out_base;         /* OUT its first byte in the merged batch */
  int rv;                    /* OUT the shard's nghttp2_error (0) */
} nghttp2_amd_hd_shard;
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_sharded_encode_dev(nghttp2_amd_hd_sharded *s,
                                                         nghttp2_amd_hd_shard *shards);
NGHTTP2_AMD_EXTERN int nghttp2_amd_hd_sharded_decode_dev(nghttp2_amd_hd_sharded *s,
                                                         nghttp2_amd_hd_shard *shards);

#ifdef __cplusplus
}
#endif

#endif /* NGHTTP2_AMD_HD_H */
