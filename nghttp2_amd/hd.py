"""ctypes binding of include/nghttp2_amd_hd.h (the engine's C ABI).

HuffmanBatchCodec mirrors, for batches of strings, the reference's internal
Huffman API (lib/nghttp2_hd.h:385-440):

  ==========================================  ==================================
  reference (lib/nghttp2_hd_huffman.c)        batched engine call
  ==========================================  ==================================
  nghttp2_hd_huff_encode_count  :34-43        encode_count(src, src_off)
  nghttp2_hd_huff_encode        :45-104       encode(src, src_off)
  nghttp2_hd_huff_decode_context_init :106    (implicit per string)
  nghttp2_hd_huff_decode(fin=1) :111-143      decode(src, src_off) -> status
  nghttp2_hd_huff_decode_failure_state :145   fstate == 0x100
  nghttp2_huff_estimate_decode_length (.h:76) decode_slots(src_off)
  ==========================================  ==================================

Tensors are torch CUDA (HIP) tensors: uint8 pools, int32 tensors holding
uint32 offsets.  Errors follow nghttp2: negative nghttp2_error codes raise
RuntimeError; per-string decode status is an int32 tensor.
"""
import collections
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libnghttp2_amd_hd.so"

NGHTTP2_ERR_INVALID_ARGUMENT = -501
NGHTTP2_ERR_BUFFER_ERROR = -502
NGHTTP2_ERR_INVALID_STATE = -519
NGHTTP2_ERR_HEADER_COMP = -523
NGHTTP2_ERR_INSUFF_BUFSIZE = -525
NGHTTP2_ERR_FATAL = -900

# check_field / check_fields / inflate_blocks(checks=True): a bit is set
# exactly when the reference's nghttp2_check_* function returns 1
CHECK_NAME = 0x01             # nghttp2_check_header_name
CHECK_VALUE = 0x02            # nghttp2_check_header_value
CHECK_VALUE_RFC9113 = 0x04    # nghttp2_check_header_value_rfc9113
CHECK_METHOD = 0x08           # nghttp2_check_method
CHECK_PATH = 0x10             # nghttp2_check_path
CHECK_AUTHORITY = 0x20        # nghttp2_check_authority
CHECK_NAME_LOWER = 0x40       # nghttp2_check_nonempty_header_name(...) == 1
CHECK_INVALID = 0x80          # the string was not examined

# name_tokens / inflate_blocks(tokens=True): lookup_token's result, or
TOKEN_NONE = -1               # examined, not a token name (lookup_token's -1)
TOKEN_INVALID = -2            # the string was not examined

# http_facts / http_facts_batch / inflate_blocks(http=...): the value facts of
# nghttp2_http_on_header (lib/nghttp2_http.c), a bit set exactly when the
# reference's test passes
HTTP_FACT_AUTHORITY = 0x001      # check_authority (no '@')
HTTP_FACT_SCHEME = 0x002         # check_scheme
HTTP_FACT_SCHEME_HTTP = 0x004    # "http" / "https", any case
HTTP_FACT_METH_HEAD = 0x008
HTTP_FACT_METH_CONNECT = 0x010
HTTP_FACT_METH_OPTIONS = 0x020
HTTP_FACT_PATH_SLASH = 0x040     # first byte '/'
HTTP_FACT_PATH_ASTERISK = 0x080  # "*"
HTTP_FACT_TE_TRAILERS = 0x100    # "trailers", any case
HTTP_FACT_LWS = 0x200            # SP / HT only
HTTP_FACT_UINT = 0x400           # parse_uint succeeds
HTTP_FACT_INVALID = 0x80000000   # the string was not examined

HTTP_MODE_REQUEST = 0x01           # session->server or a PUSH_PROMISE; clear: a response
HTTP_MODE_PUSH = 0x02              # even stream id
HTTP_MODE_TRAILER = 0x04
HTTP_MODE_CONNECT_PROTOCOL = 0x08  # the extended CONNECT setting is enabled
HTTP_MODE_NO_RFC9113_WS = 0x10

NGHTTP2_ERR_IGN_HTTP_HEADER = -105
NGHTTP2_ERR_REMOVE_HTTP_HEADER = -106
NGHTTP2_ERR_HTTP_HEADER = -531
NGHTTP2_ERR_HTTP_MESSAGING = -532
HTTP_NOT_EXAMINED = 1            # a field after the block's first NGHTTP2_ERR_HTTP_HEADER


class HttpState(ctypes.Structure):
    """nghttp2_amd_hd_http_state: the stream's http_flags, status_code and
    content_length; a fresh stream is HttpState(0, -1, -1)."""
    _fields_ = [("http_flags", ctypes.c_uint32), ("status_code", ctypes.c_int32),
                ("content_length", ctypes.c_int64)]


_HTTP_STATE_DTYPE = np.dtype([("http_flags", "<u4"), ("status_code", "<i4"),
                              ("content_length", "<i8")])
assert _HTTP_STATE_DTYPE.itemsize == ctypes.sizeof(HttpState)

# parse_block / parse_blocks: one representation of a header block
# (nghttp2_amd_hd_op, 32 bytes).  Offsets are positions in the wire the block
# was parsed from, lengths the encoded lengths; name_lit / value_lit number the
# Huffman literals (-1: a raw literal or none).
OP_SIZE, OP_INDEXED, OP_LITERAL = 0, 1, 2
OP_INDEX_REQUIRED = 0x01
OP_NO_INDEX = 0x02
OP_NEW_NAME = 0x04
OP_NAME_HUFF = 0x08
OP_VALUE_HUFF = 0x10
OP_DTYPE = np.dtype([("kind", "u1"), ("flags", "u1"), ("reserved", "<u2"), ("value", "<u4"),
                     ("name_off", "<u4"), ("name_len", "<u4"), ("value_off", "<u4"),
                     ("value_len", "<u4"), ("name_lit", "<i4"), ("value_lit", "<i4")])
assert OP_DTYPE.itemsize == 32
# totals[3] of parse_blocks / gather_huffman_literals
PARSE_OVERFLOW_OPS = 0x1
PARSE_OVERFLOW_U32 = 0x2
PARSE_OVERFLOW_LITS = 0x4
PARSE_OVERFLOW_POOL = 0x8

_lib = None


def lib_path():
    return os.path.join(HERE, "lib", LIB_NAME)


def lib():
    """Load the HIP library; raises if it was not built (no fallback)."""
    global _lib
    if _lib is None:
        # NGHTTP2_AMD_LIB: an ablation build of the same library (tools/diag)
        path = os.environ.get("NGHTTP2_AMD_LIB") or lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                "nghttp2_amd: HIP library %s is missing -- run "
                "`python -c 'import __graft_entry__ as g; g.build()'`" % path)
        # torch first: its HIP runtime (torch/lib/libamdhip64.so, soname
        # libamdhip64.so.7) then also serves this library, so the process
        # holds ONE runtime and torch's streams are valid here.  Loaded the
        # other way round, torch brings a second runtime copy.
        import torch  # noqa: F401
        L = ctypes.CDLL(path)
        vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
        L.nghttp2_amd_hd_version.restype = ctypes.c_char_p
        L.nghttp2_amd_hd_huff_tables.argtypes = [vp, vp]
        L.nghttp2_amd_hd_huff_encode_bound.restype = sz
        L.nghttp2_amd_hd_huff_encode_bound.argtypes = [ctypes.c_uint64, u32]
        L.nghttp2_amd_hd_huff_workspace_size.restype = sz
        L.nghttp2_amd_hd_huff_workspace_size.argtypes = [u32]
        L.nghttp2_amd_hd_huff_encode_workspace_size.restype = sz
        L.nghttp2_amd_hd_huff_encode_workspace_size.argtypes = [ctypes.c_uint64, u32]
        L.nghttp2_amd_hd_huff_encode_batch.argtypes = [vp, vp, u32, vp, sz, vp, vp, sz, vp]
        L.nghttp2_amd_hd_huff_encode_count_batch.argtypes = [vp, vp, u32, vp, vp]
        L.nghttp2_amd_hd_huff_decode_slots.argtypes = [vp, u32, vp, vp, sz, vp]
        L.nghttp2_amd_hd_huff_decode_batch.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.nghttp2_amd_hd_huff_decode_bound.restype = sz
        L.nghttp2_amd_hd_huff_decode_bound.argtypes = [ctypes.c_uint64, u32]
        u64 = ctypes.c_uint64
        L.nghttp2_amd_hd_huff_decode_batch_auto.argtypes = [vp, vp, u32, u64, vp, sz, vp, vp,
                                                            vp, vp, vp]
        L.nghttp2_amd_hd_huff_decode_fsm_batch.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp,
                                                           vp, vp, ctypes.c_int, vp]
        L.nghttp2_amd_hd_emit_strings_bound.restype = sz
        L.nghttp2_amd_hd_emit_strings_bound.argtypes = [u64, u32]
        L.nghttp2_amd_hd_emit_strings_workspace_size.restype = sz
        L.nghttp2_amd_hd_emit_strings_workspace_size.argtypes = [u64, u32]
        L.nghttp2_amd_hd_emit_strings_batch.argtypes = [vp, vp, u32, u64, vp, sz, vp, vp, sz, vp]
        L.nghttp2_amd_hd_name_tokens_batch.argtypes = [vp, vp, u32, vp, vp, vp]
        L.nghttp2_amd_hd_name_tokens_len_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        L.nghttp2_amd_hd_lookup_token.argtypes = [ctypes.c_char_p, sz]
        L.nghttp2_amd_hd_lookup_token.restype = ctypes.c_int32
        L.nghttp2_amd_hd_name_hash.argtypes = [ctypes.c_char_p, sz]
        L.nghttp2_amd_hd_name_hash.restype = ctypes.c_uint32
        L.nghttp2_amd_hd_check_field.argtypes = [ctypes.c_char_p, sz]
        L.nghttp2_amd_hd_check_field.restype = ctypes.c_uint8
        L.nghttp2_amd_hd_check_fields_batch.argtypes = [vp, vp, vp, u32, vp, vp]
        L.nghttp2_amd_hd_http_facts.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int64)]
        L.nghttp2_amd_hd_http_facts.restype = ctypes.c_uint32
        L.nghttp2_amd_hd_http_facts_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        L.nghttp2_amd_hd_http_on_header.argtypes = [
            ctypes.POINTER(HttpState), u32, ctypes.c_char_p, sz, sz, ctypes.c_int32, ctypes.c_uint8,
            ctypes.c_uint8, u32, ctypes.c_int64]
        L.nghttp2_amd_hd_http_on_request_headers.argtypes = [ctypes.POINTER(HttpState), u32]
        L.nghttp2_amd_hd_http_on_response_headers.argtypes = [ctypes.POINTER(HttpState)]
        L.nghttp2_amd_hd_parse_block.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz)]
        L.nghttp2_amd_hd_parse_blocks_bound.argtypes = [u64, u32] + [ctypes.POINTER(sz)] * 4
        L.nghttp2_amd_hd_parse_blocks_batch.argtypes = [vp, vp, u32, vp, vp, sz, vp, vp, vp, vp, sz, vp]
        L.nghttp2_amd_hd_gather_literals_batch.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp, sz, vp]
        _lib = L
    return _lib


def lookup_token(name):
    """Host lookup_token (lib/nghttp2_hd.c:137): -1 or NGHTTP2_TOKEN_*."""
    name = bytes(name)
    return lib().nghttp2_amd_hd_lookup_token(name, len(name))


def name_hash(name):
    """Host FNV-1a name hash (lib/nghttp2_hd.c:536-547)."""
    name = bytes(name)
    return lib().nghttp2_amd_hd_name_hash(name, len(name))


def check_field(s):
    """Host nghttp2_check_* of one string (lib/nghttp2_helper.c:346-558): the
    CHECK_* mask."""
    s = bytes(s)
    return lib().nghttp2_amd_hd_check_field(s, len(s))


def http_facts(s):
    """Host value facts of one string (lib/nghttp2_http.c's check_authority,
    check_scheme, lws, parse_uint and literal comparisons): (HTTP_FACT_* bits,
    parse_uint's value or -1)."""
    s = bytes(s)
    num = ctypes.c_int64()
    f = lib().nghttp2_amd_hd_http_facts(s, len(s), ctypes.byref(num))
    return f, num.value


def http_on_header(state, mode, name, value_len, token, name_mask, value_mask, value_facts,
                   value_number):
    """nghttp2_http_on_header for one field from its token, masks and facts;
    updates state (an HttpState) and returns the verdict."""
    name = bytes(name)
    return lib().nghttp2_amd_hd_http_on_header(ctypes.byref(state), mode, name, len(name), value_len,
                                               token, name_mask, value_mask, value_facts,
                                               value_number)


def http_on_request_headers(state, mode):
    return lib().nghttp2_amd_hd_http_on_request_headers(ctypes.byref(state), mode)


def http_on_response_headers(state):
    return lib().nghttp2_amd_hd_http_on_response_headers(ctypes.byref(state))


def parse_block(block, ops_cap=None):
    """The representations of one complete header block, on the host
    (nghttp2_amd_hd_parse_block; no GPU): (rv, ops).  rv is 0,
    NGHTTP2_ERR_HEADER_COMP (ops holds the representations completed before
    the failure) or, with an ops_cap too small, NGHTTP2_ERR_BUFFER_ERROR (ops
    is then the count needed).  ops is a numpy array of OP_DTYPE; offsets are
    positions in `block`, Huffman literals are numbered from 0."""
    block = bytes(block)
    buf = np.frombuffer(block + b"\0", dtype=np.uint8)
    cap = len(block) if ops_cap is None else int(ops_cap)
    ops = np.zeros(max(1, cap), dtype=OP_DTYPE)
    nops = ctypes.c_size_t()
    rv = lib().nghttp2_amd_hd_parse_block(buf.ctypes.data, len(block), ops.ctypes.data, cap,
                                          ctypes.byref(nops))
    if rv == NGHTTP2_ERR_BUFFER_ERROR:
        return rv, nops.value
    if rv not in (0, NGHTTP2_ERR_HEADER_COMP):
        _check(rv, "parse_block")
    return rv, ops[:nops.value]


def parse_blocks_bound(wire_bytes, nblocks):
    """Capacities that cannot overflow for nblocks blocks side by side in
    wire_bytes bytes: (ops_cap, lits_cap, pool_cap, ws_bytes)."""
    out = [ctypes.c_size_t() for _ in range(4)]
    _check(lib().nghttp2_amd_hd_parse_blocks_bound(int(wire_bytes), int(nblocks),
                                                   *[ctypes.byref(o) for o in out]),
           "parse_blocks_bound")
    return tuple(o.value for o in out)


# What HuffmanBatchCodec.parse_blocks returns: device tensors.  ops is int32
# [ops_cap, 8], one 32-byte record per row (ops_to_numpy gives the structured
# view); op_off / lit_base are int32[n+1] holding uint32; block_status is
# int32[n]; totals is int32[4] = {representations, Huffman literals, Huffman
# bytes, PARSE_OVERFLOW_* bits}.  wire_bytes is the wire's size on the host.
ParsedBlocks = collections.namedtuple("ParsedBlocks", "ops op_off block_status lit_base totals wire_bytes")


def ops_to_numpy(ops, count=None):
    """A parse's records (ParsedBlocks.ops, or its first `count` rows) on the
    host as a numpy array of OP_DTYPE (synchronises)."""
    if count is not None:
        ops = ops[:count]
    return ops.contiguous().cpu().numpy().view(OP_DTYPE).reshape(-1)


def tables_ref_layout():
    """The engine's tables in the reference struct layouts (host-only)."""
    sym = ctypes.create_string_buffer(257 * 8)
    dec = ctypes.create_string_buffer(257 * 16 * 4)
    lib().nghttp2_amd_hd_huff_tables(sym, dec)
    return sym.raw, dec.raw


def _check(rv, what):
    if rv != 0:
        raise RuntimeError("nghttp2_amd: %s failed with nghttp2 error %d" % (what, rv))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


class HuffmanBatchCodec:
    """Batched HPACK Huffman codec on one device.

    All calls are asynchronous on the given (default: current) torch stream.
    A codec may be used from several streams: each stream gets its own device
    workspaces (tile sums, the framing pool), allocated on that stream and
    grown there, so calls on different streams never share scratch and a
    regrown block is only reused in the order of its own stream.  Calls on one
    stream run in issue order, as any work on a stream does.
    """

    _SCRATCH_KEEP = 16  # per-stream workspaces kept (two kinds per stream)

    def __init__(self, device=None):
        import torch
        self.torch = torch
        self.device = torch.device(device if device is not None else "cuda")
        self.L = lib()
        # (stream handle, kind) -> uint8 tensor allocated on that stream; the
        # least recently used entries past _SCRATCH_KEEP are dropped, so
        # short-lived streams do not pin device workspace (a dropped block
        # returns to the caching allocator on the stream it was allocated on)
        self._scratch = collections.OrderedDict()

    def _on(self, stream):
        return stream if stream is not None else self.torch.cuda.current_stream(self.device)

    def _scratch_for(self, kind, need, stream):
        s = self._on(stream)
        key = (s.cuda_stream, kind)
        t = self._scratch.get(key)
        if t is not None:
            self._scratch.move_to_end(key)
        if t is None or t.numel() < need:
            # Uninitialised on purpose: the kernels write every scratch word
            # they read (a zero fill would be one more kernel).  Allocated
            # under the call's own stream, so the caching allocator ties the
            # block to it.
            with self.torch.cuda.stream(s):
                t = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
            self._scratch[key] = t
            while len(self._scratch) > self._SCRATCH_KEEP:
                self._scratch.popitem(last=False)
        return t

    def _empty(self, n, dtype, stream):
        """An output tensor allocated under the call's stream (so the caching
        allocator never hands its block to another stream while the call's
        kernels may still write it)."""
        with self.torch.cuda.stream(self._on(stream)):
            return self.torch.empty(n, dtype=dtype, device=self.device)

    def _workspace(self, n, raw_bytes=None, stream=None):
        return self._scratch_for("ws", self.L.nghttp2_amd_hd_huff_workspace_size(n), stream)

    def encode_bound(self, raw_bytes, n):
        return self.L.nghttp2_amd_hd_huff_encode_bound(int(raw_bytes), int(n))

    def encode(self, src, src_off, raw_bytes=None, dst=None, dst_off=None, stream=None):
        """Encode strings; returns (dst pool, dst_off int32[n+1])."""
        torch = self.torch
        n = src_off.numel() - 1
        if raw_bytes is None:
            raw_bytes = src.numel()
        cap = self.encode_bound(raw_bytes, n)
        if dst is None:
            dst = self._empty(cap, torch.uint8, stream)
        if dst_off is None:
            dst_off = self._empty(n + 1, torch.int32, stream)
        ws = self._workspace(n, raw_bytes, stream)
        rv = self.L.nghttp2_amd_hd_huff_encode_batch(
            _p(src), _p(src_off), n, _p(dst), dst.numel(), _p(dst_off), _p(ws),
            ws.numel(), _stream(stream))
        _check(rv, "encode_batch")
        return dst, dst_off

    def encode_count(self, src, src_off, enc_len=None, stream=None):
        n = src_off.numel() - 1
        if enc_len is None:
            enc_len = self._empty(max(1, n), self.torch.int32, stream)
        rv = self.L.nghttp2_amd_hd_huff_encode_count_batch(
            _p(src), _p(src_off), n, _p(enc_len), _stream(stream))
        _check(rv, "encode_count_batch")
        return enc_len[:n]

    def name_tokens(self, names, name_off, token=None, hash=None, stream=None, len=None,
                    want_hash=True):
        """lookup_token + name_hash (lib/nghttp2_hd.c:137, :536) for every
        name of the batch: returns (token int32[n], hash int32[n] holding the
        uint32 FNV-1a bits).  With len (int32[n], e.g. decode_auto's status
        next to its dst and dst_off) name i is names[off[i]:off[i]+len[i]]; a
        name with a negative or overrunning len gets TOKEN_INVALID and hash 0.
        With want_hash=False only the tokens are computed and returned, and a
        string longer than every token name is not read.  Either of the two
        goes through nghttp2_amd_hd_name_tokens_len_batch."""
        torch = self.torch
        n = name_off.numel() - 1
        if token is None:
            token = self._empty(max(1, n), torch.int32, stream)
        if len is not None or not want_hash:
            if want_hash and hash is None:
                hash = self._empty(max(1, n), torch.int32, stream)
            rv = self.L.nghttp2_amd_hd_name_tokens_len_batch(
                _p(names), _p(name_off), _p(len), n, _p(token), _p(hash if want_hash else None),
                _stream(stream))
            _check(rv, "name_tokens_len_batch")
            return (token[:n], hash[:n]) if want_hash else token[:n]
        if hash is None:
            hash = self._empty(max(1, n), torch.int32, stream)
        rv = self.L.nghttp2_amd_hd_name_tokens_batch(
            _p(names), _p(name_off), n, _p(token), _p(hash), _stream(stream))
        _check(rv, "name_tokens_batch")
        return token[:n], hash[:n]

    def check_fields(self, pool, off, len=None, mask=None, stream=None):
        """nghttp2_check_* (lib/nghttp2_helper.c:346-558) for every string of
        the batch: returns mask uint8[n] of CHECK_* bits.  String i is
        pool[off[i]:off[i+1]], or with len (int32[n], e.g. decode_auto's
        status next to its dst and dst_off) pool[off[i]:off[i]+len[i]]; a
        string with a negative or overrunning len gets CHECK_INVALID."""
        n = off.numel() - 1
        if mask is None:
            mask = self._empty(max(1, n), self.torch.uint8, stream)
        rv = self.L.nghttp2_amd_hd_check_fields_batch(
            _p(pool), _p(off), _p(len), n, _p(mask), _stream(stream))
        _check(rv, "check_fields_batch")
        return mask[:n]

    def http_facts_batch(self, pool, off, len=None, facts=None, number=None, stream=None):
        """The value facts of nghttp2_http_on_header for every string of the
        batch, in check_fields' layouts: returns (facts int32[n] holding the
        uint32 HTTP_FACT_* bits, number int64[n] = parse_uint's value or -1).
        A string with a negative or overrunning len gets HTTP_FACT_INVALID."""
        n = off.numel() - 1
        if facts is None:
            facts = self._empty(max(1, n), self.torch.int32, stream)
        if number is None:
            number = self._empty(max(1, n), self.torch.int64, stream)
        rv = self.L.nghttp2_amd_hd_http_facts_batch(
            _p(pool), _p(off), _p(len), n, _p(facts), _p(number), _stream(stream))
        _check(rv, "http_facts_batch")
        return facts[:n], number[:n]

    def parse_blocks(self, wire, block_off, wire_bytes=None, ops_cap=None, stream=None):
        """The representations of every block of a batch
        (nghttp2_amd_hd_parse_blocks_batch): block i is
        wire[block_off[i]:block_off[i+1]] (uint8 pool, int32[n+1] holding
        uint32).  Returns a ParsedBlocks of device tensors; nothing is read
        back.  ops_cap defaults to the bound for wire_bytes (default
        wire.numel()), which cannot overflow for blocks side by side; with a
        smaller one, totals[3] reports PARSE_OVERFLOW_OPS."""
        torch = self.torch
        n = block_off.numel() - 1
        if wire_bytes is None:
            wire_bytes = wire.numel()
        if wire.numel() == 0:  # an all-empty batch: a pointer the library accepts (never read)
            wire = self._empty(16, torch.uint8, stream)
        cap, _, _, need = parse_blocks_bound(wire_bytes, n)
        if ops_cap is not None:
            cap = int(ops_cap)
        ops = self._empty((max(1, cap), 8), torch.int32, stream)
        op_off = self._empty(n + 1, torch.int32, stream)
        lit_base = self._empty(n + 1, torch.int32, stream)
        status = self._empty(max(1, n), torch.int32, stream)
        totals = self._empty(4, torch.int32, stream)
        if n == 0:
            with torch.cuda.stream(self._on(stream)):
                op_off.zero_(), lit_base.zero_(), totals.zero_()
        ws = self._scratch_for("pws", need, stream)
        rv = self.L.nghttp2_amd_hd_parse_blocks_batch(
            _p(wire), _p(block_off), n, _p(op_off), _p(ops), cap, _p(status), _p(lit_base),
            _p(totals), _p(ws), ws.numel(), _stream(stream))
        _check(rv, "parse_blocks_batch")
        return ParsedBlocks(ops[:cap], op_off, status[:n], lit_base, totals, int(wire_bytes))

    def gather_huffman_literals(self, wire, parsed, lits_cap=None, pool_cap=None, stream=None):
        """Every Huffman literal of a parsed batch in one pool, in decode_auto's
        input layout (nghttp2_amd_hd_gather_literals_batch): returns (pool
        uint8, lit_off int32[lits_cap + 1]); literal k is
        pool[lit_off[k]:lit_off[k+1]] for k < parsed.totals[1], and
        decode_auto(pool, lit_off[:T + 1], enc_bytes=parsed.totals[2]) decodes
        them.  The counts are read from parsed.totals on the device.  The caps
        default to the bound; a pool_cap is the number of bytes that may be
        written (the pool tensor keeps the decode's readable tail behind it)."""
        torch = self.torch
        if wire.numel() == 0:
            wire = self._empty(16, torch.uint8, stream)
        _, lcap, pcap, _ = parse_blocks_bound(parsed.wire_bytes, 0)
        if lits_cap is not None:
            lcap = int(lits_cap)
        if pool_cap is not None:
            pcap = int(pool_cap)
        lit_off = self._empty(lcap + 1, torch.int32, stream)
        pool = self._empty(((pcap + 15) // 16) * 16 + 16, torch.uint8, stream)
        rv = self.L.nghttp2_amd_hd_gather_literals_batch(
            _p(wire), parsed.wire_bytes, _p(parsed.ops), parsed.ops.shape[0], _p(parsed.totals),
            _p(lit_off), lcap, _p(pool), pcap, _stream(stream))
        _check(rv, "gather_literals_batch")
        return pool, lit_off

    def emit_strings(self, src, src_off, raw_bytes=None, dst=None, dst_off=None, stream=None):
        """HPACK string literals (emit_string, lib/nghttp2_hd.c:1001-1044) for
        every string: returns (dst pool, dst_off int32[n+1]); literal i is
        dst[dst_off[i]:dst_off[i+1]]."""
        torch = self.torch
        n = src_off.numel() - 1
        if raw_bytes is None:
            raw_bytes = src.numel()
        cap = self.L.nghttp2_amd_hd_emit_strings_bound(int(raw_bytes), n)
        if dst is None:
            dst = self._empty(cap, torch.uint8, stream)
        if dst_off is None:
            dst_off = self._empty(n + 1, torch.int32, stream)
        need = self.L.nghttp2_amd_hd_emit_strings_workspace_size(int(raw_bytes), n)
        ews = self._scratch_for("ews", need, stream)
        rv = self.L.nghttp2_amd_hd_emit_strings_batch(
            _p(src), _p(src_off), n, int(raw_bytes), _p(dst), dst.numel(), _p(dst_off),
            _p(ews), ews.numel(), _stream(stream))
        _check(rv, "emit_strings_batch")
        return dst, dst_off

    def decode_slots(self, src_off, dst_off=None, stream=None):
        n = src_off.numel() - 1
        if dst_off is None:
            dst_off = self._empty(n + 1, self.torch.int32, stream)
        ws = self._workspace(n, stream=stream)
        rv = self.L.nghttp2_amd_hd_huff_decode_slots(
            _p(src_off), n, _p(dst_off), _p(ws), ws.numel(), _stream(stream))
        _check(rv, "decode_slots")
        return dst_off

    def decode_bound(self, enc_bytes, n):
        return self.L.nghttp2_amd_hd_huff_decode_bound(int(enc_bytes), int(n))

    def decode_auto(self, src, src_off, enc_bytes=None, dst=None, dst_off=None, status=None,
                    want_ctx=False, stream=None, pick=None):
        """Decode into a dense pool (one launch): the strings of each task of
        64 consecutive strings (or of a task split into two of 32) back to
        back from the task's base auto_slot(x_t0, t0).  enc_bytes = src_off[n] - src_off[0] sizes dst and
        picks the kernel instance by the mean string length; when it is not
        given it is read from src_off on the call's stream (a host
        synchronisation of that stream: pass it to keep the call
        asynchronous).  pick = "items64" (the short-string instance: whole
        strings of up to 96 bytes as one item since round 6) / "pieces40" forces one instance
        through that same argument (tests).  Returns
        (dst, dst_off, status[, fstate, flags])."""
        torch = self.torch
        n = src_off.numel() - 1
        if enc_bytes is None:
            with torch.cuda.stream(self._on(stream)):
                ends = src_off[[0, n]].cpu().numpy().view("uint32").astype("int64")
            enc_bytes = int(ends[1] - ends[0])
        sel = {None: int(enc_bytes), "items64": 0, "pieces40": 49 * max(1, n)}[pick]
        if dst is None:
            dst = self._empty(self.decode_bound(enc_bytes, n), torch.uint8, stream)
        if dst_off is None:
            dst_off = self._empty(n + 1, torch.int32, stream)
        if status is None:
            status = self._empty(max(1, n), torch.int32, stream)
        fstate = flags = None
        if want_ctx:
            fstate = self._empty(max(1, n), torch.int16, stream)
            flags = self._empty(max(1, n), torch.uint8, stream)
        rv = self.L.nghttp2_amd_hd_huff_decode_batch_auto(
            _p(src), _p(src_off), n, sel, _p(dst), dst.numel(), _p(dst_off), _p(status),
            _p(fstate), _p(flags), _stream(stream))
        _check(rv, "decode_batch_auto")
        if want_ctx:
            return dst, dst_off, status[:n], fstate[:n], flags[:n]
        return dst, dst_off, status[:n]

    def decode_fsm(self, src, src_off, dst_off, dst, init_fstate=None, init_flags=None,
                   final=True, stream=None):
        """The reference nibble FSM, batched (streaming-capable).  Returns
        (status, fstate, flags)."""
        torch = self.torch
        n = src_off.numel() - 1
        status = self._empty(max(1, n), torch.int32, stream)
        fstate = self._empty(max(1, n), torch.int16, stream)
        flags = self._empty(max(1, n), torch.uint8, stream)
        rv = self.L.nghttp2_amd_hd_huff_decode_fsm_batch(
            _p(src), _p(src_off), n, _p(dst), _p(dst_off), _p(status), _p(fstate),
            _p(flags), _p(init_fstate), _p(init_flags), 1 if final else 0, _stream(stream))
        _check(rv, "decode_fsm_batch")
        return status[:n], fstate[:n], flags[:n]

    def decode(self, src, src_off, dst_off=None, dst=None, dst_cap=None, status=None,
               want_ctx=False, stream=None):
        """Decode strings (fin=1 each).  Returns (dst, dst_off, status[, fstate, flags]).

        dst_off defaults to the reference's floor(8E/5)+1 slots; dst_cap must
        then be given (or is derived from src size: 8*E_total/5 + n + 16).
        """
        torch = self.torch
        n = src_off.numel() - 1
        if dst_off is None:
            dst_off = self.decode_slots(src_off, stream=stream)
            if dst_cap is None:
                dst_cap = (src.numel() * 8) // 5 + n + 16
        if dst is None:
            if dst_cap is None:
                dst_cap = int(dst_off[-1].item()) + 16
            dst = self._empty(dst_cap, torch.uint8, stream)
        if status is None:
            status = self._empty(max(1, n), torch.int32, stream)
        fstate = flags = None
        if want_ctx:
            fstate = self._empty(max(1, n), torch.int16, stream)
            flags = self._empty(max(1, n), torch.uint8, stream)
        rv = self.L.nghttp2_amd_hd_huff_decode_batch(
            _p(src), _p(src_off), n, _p(dst), _p(dst_off), _p(status), _p(fstate),
            _p(flags), _stream(stream))
        _check(rv, "decode_batch")
        if want_ctx:
            return dst, dst_off, status[:n], fstate[:n], flags[:n]
        return dst, dst_off, status[:n]


# ---------------------------------------------------------------------------
# Batched HPACK inflate front-end (nghttp2_amd_hd_inflate_*)
# ---------------------------------------------------------------------------
class _Nv(ctypes.Structure):
    _fields_ = [("block", ctypes.c_uint32), ("name_off", ctypes.c_uint32),
                ("name_len", ctypes.c_uint32), ("value_off", ctypes.c_uint32),
                ("value_len", ctypes.c_uint32), ("flags", ctypes.c_uint8)]


def _inflate_lib():
    L = lib()
    if not getattr(L, "_inflate_bound", False):
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.nghttp2_amd_hd_inflate_new.argtypes = [ctypes.POINTER(vp)]
        L.nghttp2_amd_hd_inflate_del.argtypes = [vp]
        L.nghttp2_amd_hd_inflate_del.restype = None
        L.nghttp2_amd_hd_inflate_change_table_size.argtypes = [vp, sz]
        L.nghttp2_amd_hd_inflate_get_num_table_entries.argtypes = [vp]
        L.nghttp2_amd_hd_inflate_get_num_table_entries.restype = sz
        L.nghttp2_amd_hd_inflate_get_table_entry.argtypes = [
            vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz)]
        L.nghttp2_amd_hd_inflate_get_dynamic_table_size.argtypes = [vp]
        L.nghttp2_amd_hd_inflate_get_dynamic_table_size.restype = sz
        L.nghttp2_amd_hd_inflate_get_max_dynamic_table_size.argtypes = [vp]
        L.nghttp2_amd_hd_inflate_get_max_dynamic_table_size.restype = sz
        L.nghttp2_amd_hd_inflate_blocks.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, sz,
                                                    ctypes.POINTER(sz), vp, sz,
                                                    ctypes.POINTER(sz), vp, vp]
        L.nghttp2_amd_hd_inflate_blocks_checked.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, sz,
                                                            ctypes.POINTER(sz), vp, sz,
                                                            ctypes.POINTER(sz), vp, vp, vp]
        L.nghttp2_amd_hd_inflate_blocks_fields.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, sz,
                                                           ctypes.POINTER(sz), vp, sz,
                                                           ctypes.POINTER(sz), vp, vp, vp, vp]
        L.nghttp2_amd_hd_inflate_blocks_http.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, sz,
                                                         ctypes.POINTER(sz), vp, sz,
                                                         ctypes.POINTER(sz), vp, vp, vp, vp, vp, vp,
                                                         vp, vp]
        L._inflate_bound = True
    return L


class HpackInflater:
    """One connection's HPACK decoding context (nghttp2_hd_inflater)."""

    def __init__(self):
        self.L = _inflate_lib()
        p = ctypes.c_void_p()
        _check(self.L.nghttp2_amd_hd_inflate_new(ctypes.byref(p)), "inflate_new")
        self.p = p

    def __del__(self):
        if getattr(self, "p", None):
            self.L.nghttp2_amd_hd_inflate_del(self.p)
            self.p = None

    def change_table_size(self, settings_max):
        """nghttp2_hd_inflate_change_table_size: returns 0, or
        NGHTTP2_ERR_INVALID_STATE (nothing changed) after a block that failed
        in the middle of a representation."""
        rv = self.L.nghttp2_amd_hd_inflate_change_table_size(self.p, settings_max)
        if rv != NGHTTP2_ERR_INVALID_STATE:
            _check(rv, "inflate_change_table_size")
        return rv

    def dynamic_table(self):
        """[(name, value)] of the dynamic table, most recent first."""
        out = []
        n = self.L.nghttp2_amd_hd_inflate_get_num_table_entries(self.p)
        for idx in range(62, n + 1):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            la, lb = ctypes.c_size_t(), ctypes.c_size_t()
            _check(self.L.nghttp2_amd_hd_inflate_get_table_entry(
                self.p, idx, ctypes.byref(a), ctypes.byref(la), ctypes.byref(b),
                ctypes.byref(lb)), "inflate_get_table_entry")
            out.append((ctypes.string_at(a, la.value) if la.value else b"",
                        ctypes.string_at(b, lb.value) if lb.value else b""))
        return out

    def dynamic_table_size(self):
        return self.L.nghttp2_amd_hd_inflate_get_dynamic_table_size(self.p)

    def max_dynamic_table_size(self):
        """nghttp2_hd_inflate_get_max_dynamic_table_size: the table limit in
        force (the reference's ctx.hd_table_bufsize_max)."""
        return self.L.nghttp2_amd_hd_inflate_get_max_dynamic_table_size(self.p)

    def num_table_entries(self):
        """nghttp2_hd_inflate_get_num_table_entries: static (61) + dynamic."""
        return self.L.nghttp2_amd_hd_inflate_get_num_table_entries(self.p)


_NV_DTYPE = np.dtype([("block", "<u4"), ("name_off", "<u4"), ("name_len", "<u4"),
                      ("value_off", "<u4"), ("value_len", "<u4"), ("flags", "u1")], align=True)
assert _NV_DTYPE.itemsize == ctypes.sizeof(_Nv)


def inflate_blocks(inflaters, blocks, stream=None, nva_cap=None, arena_cap=None, retry=True,
                   checks=False, tokens=False, http=None, http_state=None):
    """Inflate complete header blocks, block i against inflaters[i], with
    every Huffman literal decoded in one GPU batch.  Returns
    (status[i], fields[i] = [(name, value, flags)]).  A batch that outgrows
    the field/arena buffers is cut at the first block that does not fit
    (status NGHTTP2_ERR_BUFFER_ERROR from there on, those blocks not
    applied); with retry the rest is resubmitted with buffers twice the size.
    With checks the call is equivalent to nghttp2_amd_hd_inflate_blocks_checked and a third
    result follows: a uint8 array (nfields, 2) of the CHECK_* masks of every
    emitted field's name and value, in the order of the fields.
    With tokens the call is equivalent to nghttp2_amd_hd_inflate_blocks_fields and one more
    result follows (after the masks when both are asked for): an int32 array
    (nfields,) of lookup_token of every emitted field's name, as
    nghttp2_hd_inflate_hd_nv sets nv.token.
    With http (one HTTP_MODE_* value per block) the call is equivalent to
    nghttp2_amd_hd_inflate_blocks_http and three more results follow: an int32
    array (nfields,) of nghttp2_http_on_header's verdict for every emitted
    field (HTTP_NOT_EXAMINED after a block's first stream error), a structured
    array (nblocks,) of the streams' states after their blocks (http_flags,
    status_code, content_length), and a list of the blocks' results (0,
    NGHTTP2_ERR_HTTP_HEADER, NGHTTP2_ERR_HTTP_MESSAGING or
    NGHTTP2_ERR_HEADER_COMP).  http_state gives the states before the blocks,
    one (http_flags, status_code, content_length) per block; None is a fresh
    stream, (0, -1, -1), for every block.
    Every call goes through nghttp2_amd_hd_inflate_blocks_http, with NULL for
    the arrays not asked for (the other three entry points are that, in C).
    The blocks go in as one joined buffer and the fields come out of
    uninitialised numpy buffers (no per-block ctypes objects, no zero fill)."""
    L = _inflate_lib()
    nb = len(blocks)
    modes_all = states_all = bhttp_all = None  # (without http, all four HTTP arguments are NULL)
    if http is not None:
        modes_all = np.fromiter((int(m) for m in http), dtype=np.uint8, count=nb)
        states_all = np.empty(nb, dtype=_HTTP_STATE_DTYPE)
        if http_state is None:
            states_all[:] = (0, -1, -1)
        else:
            for i, t in enumerate(http_state):
                states_all[i] = tuple(t)
        bhttp_all = np.full(nb, NGHTTP2_ERR_BUFFER_ERROR, dtype=np.int32)
    joined = b"".join(bytes(b) for b in blocks)
    total = len(joined)
    lens_all = np.fromiter((len(b) for b in blocks), dtype=np.uint64, count=nb)
    starts = np.zeros(nb, dtype=np.uint64)
    if nb > 1:
        np.cumsum(lens_all[:-1], out=starts[1:])
    pool = np.frombuffer(joined, dtype=np.uint8) if total else np.zeros(1, dtype=np.uint8)
    ptrs_all = starts + np.uint64(pool.ctypes.data)
    infs_all = np.fromiter((i.p.value for i in inflaters), dtype=np.uint64, count=nb)
    nva_cap = total + 16 if nva_cap is None else nva_cap
    arena_cap = 8 * total + 64 * (total + 16) + 4096 if arena_cap is None else arena_cap
    s = None
    if stream is not None:
        s = ctypes.c_void_p(stream.cuda_stream)
    else:
        try:
            import torch
            if torch.cuda.is_available():
                s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        except Exception:  # pragma: no cover - torch is part of the image
            s = None
    status = [NGHTTP2_ERR_BUFFER_ERROR] * nb
    fields = [[] for _ in range(nb)]
    masks, toks, verds = [], [], []
    first = 0

    def ptr(a):  # an array's address, NULL for one not asked for
        return None if a is None else ctypes.c_void_p(a.ctypes.data)
    while first < nb:
        m = nb - first
        ptrs = np.ascontiguousarray(ptrs_all[first:])
        lens = np.ascontiguousarray(lens_all[first:])
        infs = np.ascontiguousarray(infs_all[first:])
        nva = np.empty(max(1, nva_cap), dtype=_NV_DTYPE)
        arena = np.empty(max(1, arena_cap), dtype=np.uint8)
        st = np.empty(m, dtype=np.int32)
        nv_used, ar_used = ctypes.c_size_t(), ctypes.c_size_t()
        chk = np.empty((max(1, nva_cap), 2), dtype=np.uint8) if checks else None
        tk = np.empty(max(1, nva_cap), dtype=np.int32) if tokens else None
        vd = np.empty(max(1, nva_cap), dtype=np.int32) if http is not None else None
        # (views of the callers' slices: the states are updated in place)
        modes, states, bhttp = (a if a is None else a[first:] for a in (modes_all, states_all, bhttp_all))
        rv = L.nghttp2_amd_hd_inflate_blocks_http(
            ptr(infs), m, ptr(ptrs), ptr(lens), ptr(nva), nva_cap, ctypes.byref(nv_used), ptr(arena),
            arena_cap, ctypes.byref(ar_used), ptr(st), ptr(chk), ptr(tk), ptr(modes), ptr(states),
            ptr(vd), ptr(bhttp), s)
        if rv != NGHTTP2_ERR_BUFFER_ERROR:
            _check(rv, "inflate_blocks")
        raw = arena[:ar_used.value].tobytes()
        nv = nva[:nv_used.value]
        if checks:
            masks.append(chk[:nv_used.value].copy())
        if tokens:
            toks.append(tk[:nv_used.value].copy())
        if http is not None:
            verds.append(vd[:nv_used.value].copy())
        for b, no, nl, vo, vl, fl in zip((nv["block"] + first).tolist(), nv["name_off"].tolist(),
                                         nv["name_len"].tolist(), nv["value_off"].tolist(),
                                         nv["value_len"].tolist(), nv["flags"].tolist()):
            fields[b].append((raw[no:no + nl], raw[vo:vo + vl], fl))
        stl = st.tolist()
        done = 0
        while done < m and stl[done] != NGHTTP2_ERR_BUFFER_ERROR:
            status[first + done] = stl[done]
            done += 1
        first += done
        if done < m:
            if not retry:
                break
            if done == 0:
                nva_cap, arena_cap = 2 * nva_cap + 16, 2 * arena_cap + 4096
    res = (status, fields)
    if checks:
        res += (np.concatenate(masks) if masks else np.zeros((0, 2), np.uint8),)
    if tokens:
        res += (np.concatenate(toks) if toks else np.zeros(0, np.int32),)
    if http is not None:
        res += (np.concatenate(verds) if verds else np.zeros(0, np.int32), states_all,
                bhttp_all.tolist())
    return res


# ---------------------------------------------------------------------------
# Device-resident inflaters (nghttp2_amd_hd_dev_*, nghttp2_amd_hd_replay_host)
# ---------------------------------------------------------------------------
NGHTTP2_ERR_NOMEM = -901
DEV_EXPECT_SIZE, DEV_BAD, DEV_MID_BLOCK = 0x1, 0x2, 0x4
DEV_OVERFLOW_NVA, DEV_OVERFLOW_ARENA, DEV_OVERFLOW_U32 = 0x1, 0x2, 0x4
DEV_CONN_DTYPE = np.dtype([(f, "<u4") for f in ("max", "settings_max", "min_max", "size", "count", "head",
                                                "flags", "cur")])
assert DEV_CONN_DTYPE.itemsize == 32


def _replay_lib():
    L = lib()
    if not getattr(L, "_replay_bound", False):
        vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        L.nghttp2_amd_hd_dev_inflaters_new.argtypes = [ctypes.POINTER(vp), u32, u32, vp]
        L.nghttp2_amd_hd_dev_inflaters_del.argtypes = [vp]
        L.nghttp2_amd_hd_dev_inflaters_del.restype = None
        L.nghttp2_amd_hd_dev_inflaters_change_table_size.argtypes = [vp, vp, vp, vp, u32, vp]
        L.nghttp2_amd_hd_dev_inflaters_read.argtypes = [vp, u32, vp, vp, vp, vp]
        L.nghttp2_amd_hd_dev_inflate_workspace_size.argtypes = [u32, u32, sz, u32]
        L.nghttp2_amd_hd_dev_inflate_workspace_size.restype = sz
        L.nghttp2_amd_hd_dev_inflate_blocks.argtypes = [vp, vp, sz, vp, u32, vp, vp, sz, vp, vp, vp, sz, vp, vp,
                                                        u32, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp]
        L.nghttp2_amd_hd_dev_fields_http_workspace_size.argtypes = [sz, u32]
        L.nghttp2_amd_hd_dev_fields_http_workspace_size.restype = sz
        L.nghttp2_amd_hd_dev_fields_http.argtypes = [vp, sz, vp, sz, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, sz,
                                                     vp]
        L.nghttp2_amd_hd_dev_fields_http_totals.argtypes = [vp, vp, vp]
        L.nghttp2_amd_hd_replay_host_init.argtypes = [vp]
        L.nghttp2_amd_hd_replay_host_init.restype = None
        L.nghttp2_amd_hd_replay_host_change_table_size.argtypes = [vp, vp, u32, u32]
        L.nghttp2_amd_hd_replay_host.argtypes = [vp, vp, vp, u32, vp, sz, vp, u32, vp, vp, vp, vp, vp, vp, u32,
                                                 vp, sz, vp, sz, vp, vp, vp]
        L._replay_bound = True
    return L


def replay_fields(nva, arena, block_nv_off, out_status):
    """A replay's results (host arrays, or the device tensors of a
    ReplayedBlocks: synchronises) as inflate_blocks returns them:
    (status[i], fields[i] = [(name, value, flags)])."""
    def host(a):
        return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    off = host(block_nv_off).view(np.uint32).tolist()
    status = host(out_status).view(np.int32).tolist()
    nv = host(nva).reshape(-1).view(np.uint8)[:_NV_DTYPE.itemsize * off[-1]].view(_NV_DTYPE)
    raw = host(arena).tobytes()
    flat = [(raw[no:no + nl], raw[vo:vo + vl], fl)
            for no, nl, vo, vl, fl in zip(nv["name_off"].tolist(), nv["name_len"].tolist(),
                                          nv["value_off"].tolist(), nv["value_len"].tolist(),
                                          nv["flags"].tolist())]
    return status, [flat[off[i]:off[i + 1]] for i in range(len(status))]


def replay_annotated(r):
    """A ReplayedBlocks of a call with checks, tokens or http, read back
    (synchronises) in inflate_blocks' result order: (status, fields), then the
    (nfields, 2) masks, the tokens, and the verdicts, the states after the
    blocks (a structured array) and the list of the blocks' results, each
    where the call was asked for it."""
    res = replay_fields(r.nva, r.arena, r.block_nv_off, r.status)
    nf = int(r.block_nv_off[-1].item()) & 0xFFFFFFFF
    if r.checks is not None:
        res += (r.checks.cpu().numpy()[:2 * nf].reshape(-1, 2),)
    if r.tokens is not None:
        res += (r.tokens.cpu().numpy()[:nf],)
    if r.block_http is not None:
        res += (r.verdicts.cpu().numpy()[:nf], r.http_state.cpu().numpy().view(_HTTP_STATE_DTYPE),
                r.block_http.cpu().tolist())
    return res


def _conn_state(hdr, entries, raw):
    e = entries[:4 * int(hdr["count"])].reshape(-1, 4).tolist()
    return [(raw[a:a + b], raw[c:c + d]) for a, b, c, d in e]


def _host_table(h, ring, store, table_bytes):
    """[(name, value)], most recent first, of a host twin's table: its header
    h, its ring (uint32 [4 * slots]) and its two store buffers."""
    slots = table_bytes // 32
    ring = ring.reshape(-1, 4)
    raw = store[int(h["cur"]) * table_bytes:][:table_bytes].tobytes()
    out = []
    for i in range(int(h["count"])):
        a, b, c, d = (int(x) for x in ring[(int(h["head"]) + i) % slots])
        out.append((raw[a:a + (b & 0xFFFFFF)], raw[c:c + (d & 0xFFFFFF)]))
    return out


class HostReplayInflater:
    """One connection of a DeviceInflaters set on the host
    (nghttp2_amd_hd_replay_host; no GPU): the same header, ring and stores,
    walked by the same code.  What the device results are compared with."""

    def __init__(self, table_bytes=4096):
        self.L = _replay_lib()
        self.table_bytes = int(table_bytes)
        self.hdr = np.zeros(1, DEV_CONN_DTYPE)
        self.ring = np.zeros(self.table_bytes // 32 * 4, np.uint32)
        self.store = np.zeros(2 * self.table_bytes, np.uint8)
        self.L.nghttp2_amd_hd_replay_host_init(self.hdr.ctypes.data)

    def change_table_size(self, value):
        rv = self.L.nghttp2_amd_hd_replay_host_change_table_size(self.hdr.ctypes.data, self.ring.ctypes.data,
                                                                 self.table_bytes, int(value))
        if rv != NGHTTP2_ERR_INVALID_STATE:
            _check(rv, "replay_host_change_table_size")
        return rv

    def replay(self, wire, block_off, op_off, ops, block_status, dst=None, dst_off=None, status=None,
               nva_cap=None, arena_cap=None):
        """The blocks wire[block_off[i]:block_off[i+1]] with the records
        ops[op_off[i]:op_off[i+1]] (OP_DTYPE, offsets into wire) and parse
        statuses block_status, in order on this connection; literal k is
        dst[dst_off[k]:+status[k]].  Returns (out_totals, nva, arena,
        block_nv_off, out_status) as numpy arrays; with an overflow bit in
        out_totals[2] nothing was emitted and the table is as before."""
        n = len(block_off) - 1
        w = np.frombuffer(bytes(wire) + b"\0", np.uint8)
        block_off = np.ascontiguousarray(block_off, np.uint32)
        op_off = np.ascontiguousarray(op_off, np.uint32)
        ops = np.ascontiguousarray(ops, OP_DTYPE) if len(ops) else np.zeros(1, OP_DTYPE)
        block_status = np.ascontiguousarray(block_status, np.int32)
        nlits = 0 if status is None else len(status)
        if nlits:
            dst = np.ascontiguousarray(dst, np.uint8) if len(dst) else np.zeros(1, np.uint8)
            dst_off = np.ascontiguousarray(dst_off, np.uint32)
            status = np.ascontiguousarray(status, np.int32)
        nva_cap = max(1, len(ops)) if nva_cap is None else int(nva_cap)
        if arena_cap is None:  # the exact need, from a run that emits nothing
            r = self.replay(wire, block_off, op_off, ops, block_status, dst, dst_off, status, nva_cap, 0)
            if not r[0][2] & DEV_OVERFLOW_ARENA:  # (no byte needed: that run was the call)
                return r
            arena_cap = int(r[0][1])
        nva = np.zeros(max(1, nva_cap), _NV_DTYPE)
        arena = np.zeros(max(1, arena_cap), np.uint8)
        nv_off = np.zeros(n + 1, np.uint32)
        out_status = np.zeros(max(1, n), np.int32)
        totals = np.zeros(4, np.uint32)

        def ptr(a):  # the decode's arrays are not read without literals
            return a.ctypes.data if nlits else None
        rv = self.L.nghttp2_amd_hd_replay_host(
            self.hdr.ctypes.data, self.ring.ctypes.data, self.store.ctypes.data, self.table_bytes, w.ctypes.data,
            len(w) - 1, block_off.ctypes.data, n, op_off.ctypes.data, ops.ctypes.data, block_status.ctypes.data,
            ptr(dst), ptr(dst_off), ptr(status), nlits,
            nva.ctypes.data, nva_cap, arena.ctypes.data, arena_cap, nv_off.ctypes.data, out_status.ctypes.data,
            totals.ctypes.data)
        _check(rv, "replay_host")
        return totals, nva, arena[:arena_cap], nv_off, out_status[:n]

    def table(self):
        """[(name, value)] of the dynamic table, most recent first."""
        return _host_table(self.hdr[0], self.ring, self.store, self.table_bytes)

    def table_size(self):
        return int(self.hdr[0]["size"])

    def table_max(self):
        return int(self.hdr[0]["max"])

    def flags(self):
        """(expect_size, bad, mid_block)"""
        f = int(self.hdr[0]["flags"])
        return bool(f & DEV_EXPECT_SIZE), bool(f & DEV_BAD), bool(f & DEV_MID_BLOCK)


# What DeviceInflaters.inflate_parsed / .inflate return: device tensors.  nva
# is uint8 [24 * nva_cap] (nghttp2_amd_hd_nv records), arena uint8, block_nv_off
# int32[n+1] holding uint32, status int32[n], totals int32[4] = {fields, arena
# bytes, DEV_OVERFLOW_* bits, 0}.  replay_fields(*r[:4]) gives the fields.
# A call with checks, tokens or http (nghttp2_amd_hd_dev_fields_http behind the
# replay) also leaves checks uint8 [2 * nva_cap], tokens int32 [nva_cap],
# verdicts int32 [nva_cap], http_state uint8 [16 * n] (_HTTP_STATE_DTYPE
# records) and block_http int32 [n]; None where not asked for.  Of the per-field
# arrays the first totals[0] entries are written.  replay_annotated(r) reads
# them back.
ReplayedBlocks = collections.namedtuple(
    "ReplayedBlocks", "nva arena block_nv_off status totals checks tokens verdicts http_state block_http",
    defaults=(None,) * 5)
DEV_FIELDS_NOT_REPLAYED, DEV_FIELDS_ARENA_SHORT = 0x1, 0x2


class _DeviceSet:
    """What the two sets of contexts in device memory share: the handle, and
    a connection's table changed in size and read back.  _PREFIX names the
    set's C functions: nghttp2_amd_hd_<_PREFIX>_new, _del, _change_table_size
    and _read."""
    _PREFIX = None

    def _call(self, name, *args):
        name = "%s_%s" % (self._PREFIX, name)
        _check(getattr(self.L, "nghttp2_amd_hd_" + name)(*args), name)

    def _new(self, L, nconn, table_bytes, device, stream, *args):
        """The set on `device`; args go between table_bytes and the stream."""
        import torch
        self.torch = torch
        self.device = torch.device(device if device is not None else "cuda")
        self.L = L
        self.nconn, self.table_bytes = int(nconn), int(table_bytes)
        p = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self._call("new", ctypes.byref(p), self.nconn, self.table_bytes, *args, _stream(stream))
        self.p = p

    def __del__(self):
        if getattr(self, "p", None):
            self.torch.cuda.synchronize(self.device)
            getattr(self.L, "nghttp2_amd_hd_%s_del" % self._PREFIX)(self.p)
            self.p = None

    def _dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype).view(np.int32)).to(self.device)

    def change_table_size(self, conns, values, stream=None):
        """nghttp2_hd_inflate_change_table_size (the inflaters) or
        nghttp2_hd_deflate_change_table_size (the deflaters) for connection
        conns[i] with values[i]; a connection appears at most once.  Returns
        the rv's as a device int32 tensor: 0, or for an inflater in the middle
        of a block NGHTTP2_ERR_INVALID_STATE."""
        conns = [int(c) for c in conns]
        if len(set(conns)) != len(conns):
            raise ValueError("change_table_size: a connection appears more than once")
        if any(c < 0 or c >= self.nconn for c in conns):
            raise ValueError("change_table_size: connection out of range")
        n = len(conns)
        rv = self.torch.zeros(max(1, n), dtype=self.torch.int32, device=self.device)
        if n:
            c = self._dev(conns, np.uint32)
            v = self._dev([int(x) for x in values], np.uint32)
            self._call("change_table_size", self.p, _p(c), _p(v), _p(rv), n, _stream(stream))
        return rv[:n]

    def _read(self, c, stream=None):
        hdr = np.zeros(1, DEV_CONN_DTYPE)
        ent = np.zeros(self.table_bytes // 32 * 4, np.uint32)
        raw = np.zeros(self.table_bytes, np.uint8)
        self._call("read", self.p, int(c), hdr.ctypes.data, ent.ctypes.data, raw.ctypes.data, _stream(stream))
        return hdr[0], ent, raw.tobytes()

    def table(self, c, stream=None):
        """[(name, value)] of connection c's dynamic table, most recent first
        (synchronises the stream)."""
        return _conn_state(*self._read(c, stream))

    def table_size(self, c, stream=None):
        return int(self._read(c, stream)[0]["size"])

    def table_max(self, c, stream=None):
        return int(self._read(c, stream)[0]["max"])

    def csr(self, conn_of_block):
        """conn_blk_off[nconn+1], conn_blk[n] (device int32 tensors) from the
        connection of every block: a stable sort, so a connection's blocks
        stay in batch order."""
        conn = np.asarray(conn_of_block, np.int64)
        if len(conn) and (conn.min() < 0 or conn.max() >= self.nconn):
            raise ValueError("conn_of_block: connection out of range")
        order = np.argsort(conn, kind="stable").astype(np.uint32)
        off = np.zeros(self.nconn + 1, np.uint32)
        np.cumsum(np.bincount(conn, minlength=self.nconn), out=off[1:])
        return self._dev(off, np.uint32), self._dev(order if len(order) else [0], np.uint32)


class DeviceInflaters(_DeviceSet):
    """nconn HPACK decoding contexts in device memory
    (nghttp2_amd_hd_dev_inflaters): the end of the chain parse -> gather ->
    decode_auto for wire that lies on the device.  table_bytes is the
    capacity per connection (a power of two >= 4096): an insertion the HPACK
    maximum admits and the store cannot hold ends its block with
    NGHTTP2_ERR_NOMEM.  Calls on one set are ordered by their stream."""

    _PREFIX = "dev_inflaters"

    def __init__(self, nconn, table_bytes=4096, device=None, stream=None):
        self._ws = self._fields_ws = None
        self._new(_replay_lib(), nconn, table_bytes, device, stream)

    def state(self, c, stream=None):
        """(table, size, max, (expect_size, bad, mid_block)) in one read."""
        h, ent, raw = self._read(c, stream)
        f = int(h["flags"])
        return (_conn_state(h, ent, raw), int(h["size"]), int(h["max"]),
                (bool(f & DEV_EXPECT_SIZE), bool(f & DEV_BAD), bool(f & DEV_MID_BLOCK)))

    def fields_totals(self, stream=None):
        """The totals word of the last call with checks, tokens or http
        (synchronises the stream): [fields examined, their arena bytes,
        DEV_FIELDS_* bits, 0]."""
        t = np.zeros(4, np.uint32)
        if self._fields_ws is not None:
            _check(self.L.nghttp2_amd_hd_dev_fields_http_totals(_p(self._fields_ws), t.ctypes.data, _stream(stream)),
                   "dev_fields_http_totals")
        return t.tolist()

    def _annotate(self, r, nva_cap, n, checks, tokens, http, http_state, s):
        """nghttp2_amd_hd_dev_fields_http behind a replay, on stream s."""
        torch = self.torch
        need = self.L.nghttp2_amd_hd_dev_fields_http_workspace_size(nva_cap, n)
        chk = tok = modes = states = verd = bhttp = None
        with torch.cuda.stream(s):
            if self._fields_ws is None or self._fields_ws.numel() < need:
                self._fields_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            if checks:
                chk = torch.empty(2 * max(1, nva_cap), dtype=torch.uint8, device=self.device)
            if tokens:
                tok = torch.empty(max(1, nva_cap), dtype=torch.int32, device=self.device)
            if http is not None:
                if hasattr(http, "device"):
                    modes = http.to(device=self.device, dtype=torch.uint8)
                else:
                    modes = torch.from_numpy(np.fromiter((int(m) for m in http), np.uint8, count=n)).to(self.device)
                if modes.numel() != n:
                    raise ValueError("http: one mode per block")
                if http_state is None:  # fresh streams: {0, -1, -1}
                    states = torch.full((n, 4), -1, dtype=torch.int32, device=self.device)
                    states[:, 0] = 0
                    states = states.view(torch.uint8).reshape(-1)
                else:  # (a copy: the caller's states stay as they are)
                    states = http_state.to(self.device).contiguous().view(torch.uint8).reshape(-1).clone()
                if states.numel() != n * _HTTP_STATE_DTYPE.itemsize:
                    raise ValueError("http_state: one 16-byte state per block")
                verd = torch.empty(max(1, nva_cap), dtype=torch.int32, device=self.device)
                bhttp = torch.empty(n, dtype=torch.int32, device=self.device)
        rv = self.L.nghttp2_amd_hd_dev_fields_http(
            _p(r.nva), nva_cap, _p(r.arena), r.arena.untyped_storage().nbytes(), _p(r.block_nv_off), _p(r.status),
            _p(r.totals), n, _p(chk), _p(tok), _p(modes), _p(states), _p(verd), _p(bhttp), _p(self._fields_ws),
            self._fields_ws.numel(), ctypes.c_void_p(s.cuda_stream))
        _check(rv, "dev_fields_http")
        return r._replace(checks=chk, tokens=tok, verdicts=verd, http_state=states, block_http=bhttp)

    def inflate_parsed(self, wire, block_off, parsed, dst, dst_off, status, conn_blk_off, conn_blk,
                       nva_cap=None, arena_cap=None, stream=None, checks=False, tokens=False, http=None,
                       http_state=None):
        """nghttp2_amd_hd_dev_inflate_blocks on tensors: the parse's results
        (a ParsedBlocks), the decode's (dst, dst_off, status; None for a batch
        without Huffman literals) and the CSR of csr().  nva_cap defaults to
        the parse's ops_cap, which cannot overflow.  Nothing is read back:
        returns a ReplayedBlocks.
        checks, tokens, http and http_state are inflate_blocks' and queue
        nghttp2_amd_hd_dev_fields_http behind the replay: http is a device
        uint8 tensor or a host sequence of HTTP_MODE_* values, one per block,
        http_state a device tensor of 16-byte _HTTP_STATE_DTYPE records (any
        dtype; it is copied, not changed) or None for fresh streams.  A host
        sequence is uploaded, which waits for the stream.  The arena is
        allocated with the slack the batch kernels' pool rule asks for."""
        torch = self.torch
        n = block_off.numel() - 1
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        ops_cap = parsed.ops.shape[0]
        nva_cap = ops_cap if nva_cap is None else int(nva_cap)
        arena_cap = 4 * parsed.wire_bytes + 4096 if arena_cap is None else int(arena_cap)
        need = self.L.nghttp2_amd_hd_dev_inflate_workspace_size(self.nconn, self.table_bytes, ops_cap, n)
        with torch.cuda.stream(s):
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            nva = torch.empty(max(1, nva_cap) * _NV_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
            # (readable to align_up(arena bytes, 16) + 16: the pool rule)
            arena = torch.empty((max(1, arena_cap) + 15) // 16 * 16 + 16, dtype=torch.uint8, device=self.device)
            nv_off = torch.zeros(n + 1, dtype=torch.int32, device=self.device)
            out_status = torch.empty(max(1, n), dtype=torch.int32, device=self.device)
            totals = torch.zeros(4, dtype=torch.int32, device=self.device)
            if wire.numel() == 0:
                wire = torch.empty(16, dtype=torch.uint8, device=self.device)
            nlits = 0 if dst is None else status.numel()
            if dst is None:  # never read: the call is told there is no literal
                dst = torch.empty(16, dtype=torch.uint8, device=self.device)
                dst_off = status = torch.zeros(4, dtype=torch.int32, device=self.device)
        rv = self.L.nghttp2_amd_hd_dev_inflate_blocks(
            self.p, _p(wire), parsed.wire_bytes, _p(block_off), n, _p(parsed.op_off), _p(parsed.ops), ops_cap,
            _p(parsed.block_status), _p(parsed.totals), _p(dst), dst.numel(), _p(dst_off), _p(status), nlits,
            _p(conn_blk_off), _p(conn_blk), _p(nva), nva_cap, _p(arena), arena_cap, _p(nv_off), _p(out_status),
            _p(totals), _p(self._ws), self._ws.numel(), ctypes.c_void_p(s.cuda_stream))
        _check(rv, "dev_inflate_blocks")
        r = ReplayedBlocks(nva, arena[:arena_cap], nv_off, out_status[:n], totals)
        if checks or tokens or http is not None:
            r = self._annotate(r, nva_cap, n, checks, tokens, http, http_state, s)
        return r

    def inflate(self, codec, wire, block_off, conn_of_block, wire_bytes=None, nlits=None, enc_bytes=None,
                arena_cap=None, stream=None, csr=None, checks=False, tokens=False, http=None, http_state=None):
        """parse -> gather -> decode_auto -> replay of a batch on the device:
        block i is wire[block_off[i]:block_off[i+1]] and belongs to
        connection conn_of_block[i] (a host sequence).  Returns a
        ReplayedBlocks of device tensors.  Two things make the host wait for
        the stream, and both can be avoided.  The CSR is built from
        conn_of_block on the host and uploaded, which waits for the work
        queued before it: pass csr=self.csr(conn_of_block), built ahead (then
        conn_of_block is not read and may be None).  And the chain keeps one
        host read, the decode's string count (the parse's totals[1], read with
        totals[2]): pass nlits (and enc_bytes, else the wire's size bounds
        it); a count below the batch's fails the fields of the literals past
        it.  With csr, nlits and an arena_cap, calls queue on the stream with
        no host synchronisation between them.  Without an arena_cap the call starts from four times the wire,
        reads out_totals and repeats the replay with the reported need when
        the arena was too small; with one, nothing is read and an overflow
        is the caller's to see in totals[2].
        checks, tokens, http and http_state: see inflate_parsed; the repeated
        replay repeats them (an overflowed call wrote none and changed no
        state)."""
        torch = self.torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        off, blk = csr if csr is not None else self.csr(conn_of_block)
        pb = codec.parse_blocks(wire, block_off, wire_bytes=wire_bytes, stream=s)
        pool, lit_off = codec.gather_huffman_literals(wire, pb, stream=s)
        if nlits is None:
            with torch.cuda.stream(s):
                t = pb.totals.cpu().numpy().view(np.uint32)
            if t[3]:
                raise RuntimeError("nghttp2_amd: the parse overflowed (totals[3] = %d)" % t[3])
            nlits, enc_bytes = int(t[1]), int(t[2])
        elif enc_bytes is None:
            enc_bytes = pb.wire_bytes
        dec = (None, None, None)
        if nlits:
            dec = codec.decode_auto(pool, lit_off[:nlits + 1], enc_bytes=enc_bytes, stream=s)
        ann = dict(checks=checks, tokens=tokens, http=http, http_state=http_state)
        r = self.inflate_parsed(wire, block_off, pb, dec[0], dec[1], dec[2], off, blk, arena_cap=arena_cap,
                                stream=s, **ann)
        if arena_cap is None:
            with torch.cuda.stream(s):
                t = r.totals.cpu().numpy().view(np.uint32)
            if t[2] & DEV_OVERFLOW_ARENA and not t[2] & DEV_OVERFLOW_U32:
                r = self.inflate_parsed(wire, block_off, pb, dec[0], dec[1], dec[2], off, blk,
                                        arena_cap=int(t[1]), stream=s, **ann)
        return r


# ---------------------------------------------------------------------------
# Batched HPACK deflate front-end (nghttp2_amd_hd_deflate_*)
# ---------------------------------------------------------------------------
class _NvIn(ctypes.Structure):
    _fields_ = [("name", ctypes.c_void_p), ("value", ctypes.c_void_p),
                ("namelen", ctypes.c_size_t), ("valuelen", ctypes.c_size_t),
                ("flags", ctypes.c_uint8)]


_NVIN_DTYPE = np.dtype([("name", "<u8"), ("value", "<u8"), ("namelen", "<u8"),
                        ("valuelen", "<u8"), ("flags", "u1")], align=True)
assert _NVIN_DTYPE.itemsize == ctypes.sizeof(_NvIn)


def _deflate_lib():
    L = _inflate_lib()
    if not getattr(L, "_deflate_bound", False):
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.nghttp2_amd_hd_deflate_new.argtypes = [ctypes.POINTER(vp), sz]
        L.nghttp2_amd_hd_deflate_del.argtypes = [vp]
        L.nghttp2_amd_hd_deflate_del.restype = None
        L.nghttp2_amd_hd_deflate_change_table_size.argtypes = [vp, sz]
        L.nghttp2_amd_hd_deflate_get_num_table_entries.argtypes = [vp]
        L.nghttp2_amd_hd_deflate_get_num_table_entries.restype = sz
        L.nghttp2_amd_hd_deflate_get_table_entry.argtypes = [
            vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz)]
        L.nghttp2_amd_hd_deflate_get_dynamic_table_size.argtypes = [vp]
        L.nghttp2_amd_hd_deflate_get_dynamic_table_size.restype = sz
        L.nghttp2_amd_hd_deflate_blocks.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, sz, vp, vp, vp]
        L.nghttp2_amd_hd_deflate_get_max_dynamic_table_size.argtypes = [vp]
        L.nghttp2_amd_hd_deflate_get_max_dynamic_table_size.restype = sz
        L.nghttp2_amd_hd_deflate_bound.argtypes = [vp, vp, sz]
        L.nghttp2_amd_hd_deflate_bound.restype = sz
        L.nghttp2_amd_hd_deflate_hd2.argtypes = [vp, vp, sz, vp, sz, vp]
        L.nghttp2_amd_hd_deflate_hd2.restype = ctypes.c_ssize_t
        L.nghttp2_amd_hd_deflate_hd_vec2.argtypes = [vp, vp, sz, vp, sz, vp]
        L.nghttp2_amd_hd_deflate_hd_vec2.restype = ctypes.c_ssize_t
        L.nghttp2_amd_hd_decode_length.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(sz),
                                                   ctypes.POINTER(ctypes.c_int), ctypes.c_uint32, sz,
                                                   vp, vp, sz]
        L.nghttp2_amd_hd_decode_length.restype = ctypes.c_ssize_t
        L._deflate_bound = True
    return L


class HpackDeflater:
    """One connection's HPACK encoding context (nghttp2_hd_deflater)."""

    def __init__(self, max_deflate_table_size=4096):
        self.L = _deflate_lib()
        p = ctypes.c_void_p()
        _check(self.L.nghttp2_amd_hd_deflate_new(ctypes.byref(p), max_deflate_table_size),
               "deflate_new")
        self.p = p

    def __del__(self):
        if getattr(self, "p", None):
            self.L.nghttp2_amd_hd_deflate_del(self.p)
            self.p = None

    def change_table_size(self, settings_max):
        _check(self.L.nghttp2_amd_hd_deflate_change_table_size(self.p, settings_max),
               "deflate_change_table_size")

    def dynamic_table(self):
        out = []
        n = self.L.nghttp2_amd_hd_deflate_get_num_table_entries(self.p)
        for idx in range(62, n + 1):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            la, lb = ctypes.c_size_t(), ctypes.c_size_t()
            _check(self.L.nghttp2_amd_hd_deflate_get_table_entry(
                self.p, idx, ctypes.byref(a), ctypes.byref(la), ctypes.byref(b),
                ctypes.byref(lb)), "deflate_get_table_entry")
            out.append((ctypes.string_at(a, la.value) if la.value else b"",
                        ctypes.string_at(b, lb.value) if lb.value else b""))
        return out

    def dynamic_table_size(self):
        return self.L.nghttp2_amd_hd_deflate_get_dynamic_table_size(self.p)

    def max_dynamic_table_size(self):
        """nghttp2_hd_deflate_get_max_dynamic_table_size (the reference's
        ctx.hd_table_bufsize_max)."""
        return self.L.nghttp2_amd_hd_deflate_get_max_dynamic_table_size(self.p)

    def num_table_entries(self):
        return self.L.nghttp2_amd_hd_deflate_get_num_table_entries(self.p)

    def bound(self, header_list):
        """nghttp2_hd_deflate_bound of one list."""
        nva, keep = _nv_array(header_list)
        return self.L.nghttp2_amd_hd_deflate_bound(self.p, nva.ctypes.data, len(header_list))

    def deflate_hd2(self, header_list, buflen, stream=None):
        """nghttp2_hd_deflate_hd2 into a buffer of buflen bytes: (rv, wire);
        rv is the length or NGHTTP2_ERR_INSUFF_BUFSIZE / HEADER_COMP."""
        nva, keep = _nv_array(header_list)
        buf = np.zeros(max(1, buflen), dtype=np.uint8)
        rv = self.L.nghttp2_amd_hd_deflate_hd2(self.p, buf.ctypes.data, buflen, nva.ctypes.data,
                                               len(header_list), _cur_stream(stream))
        return rv, (buf[:rv].tobytes() if rv >= 0 else b"")

    def deflate_hd_vec2(self, header_list, chunk_lens, stream=None):
        """nghttp2_hd_deflate_hd_vec2 over chunks of the given lengths (None:
        a NULL vector of length 0): (rv, [chunk bytes])."""
        nva, keep = _nv_array(header_list)
        if chunk_lens is None:
            rv = self.L.nghttp2_amd_hd_deflate_hd_vec2(self.p, None, 0, nva.ctypes.data,
                                                       len(header_list), _cur_stream(stream))
            return rv, []
        bufs = [np.zeros(max(1, n), dtype=np.uint8) for n in chunk_lens]
        vec = (_Vec * max(1, len(chunk_lens)))()
        for k, (b, n) in enumerate(zip(bufs, chunk_lens)):
            vec[k].base = b.ctypes.data if n else None
            vec[k].len = n
        rv = self.L.nghttp2_amd_hd_deflate_hd_vec2(self.p, vec, len(chunk_lens), nva.ctypes.data,
                                                   len(header_list), _cur_stream(stream))
        return rv, [b[:n].tobytes() for b, n in zip(bufs, chunk_lens)]


class _Vec(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_size_t)]


def _cur_stream(stream):
    if stream is not None:
        return ctypes.c_void_p(stream.cuda_stream)
    import torch
    if torch.cuda.is_available():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None


def _nv_array(header_list):
    """An nghttp2_nv-layout array over one list's (name, value[, flags]);
    returns (array, buffers kept alive)."""
    nva = np.zeros(max(1, len(header_list)), dtype=_NVIN_DTYPE)
    keep = []
    for k, h in enumerate(header_list):
        n, v = np.frombuffer(bytes(h[0]) + b"\0", np.uint8), np.frombuffer(bytes(h[1]) + b"\0", np.uint8)
        keep += [n, v]
        nva[k] = (n.ctypes.data, v.ctypes.data, len(h[0]), len(h[1]), h[2] if len(h) > 2 else 0)
    return nva, keep


def decode_length(data, prefix, initial=0, shift=0):
    """nghttp2_hd_decode_length over bytes `data`: (rv, value, shift, fin)."""
    L = _deflate_lib()
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    res, sh, fin = ctypes.c_uint32(), ctypes.c_size_t(), ctypes.c_int()
    base = buf.ctypes.data
    rv = L.nghttp2_amd_hd_decode_length(ctypes.byref(res), ctypes.byref(sh), ctypes.byref(fin),
                                        initial, shift, base, base + len(data), prefix)
    return rv, res.value, sh.value, fin.value


def deflate_blocks(deflaters, header_lists, stream=None, out_cap=None):
    """Encode header lists (each [(name, value[, flags])]), list i with
    deflaters[i]; every literal framed in one GPU batch.  Returns
    (status[i], wire[i]).  out_cap (default: room for every list) limits the
    output: a list that does not fit gets NGHTTP2_ERR_BUFFER_ERROR and its
    deflater turns bad."""
    L = _deflate_lib()
    nb = len(header_lists)
    flat = [(bytes(h[0]), bytes(h[1]), (h[2] if len(h) > 2 else 0))
            for hl in header_lists for h in hl]
    nf = len(flat)
    # every name and value in one joined buffer; the nv array (nghttp2_nv
    # layout) points into it -- no ctypes object per field
    parts = [x for n_, v_, _ in flat for x in (n_, v_)]
    joined = b"".join(parts)
    plen = np.fromiter((len(x) for x in parts), dtype=np.uint64, count=2 * nf)
    pstart = np.zeros(2 * nf, dtype=np.uint64)
    if nf:
        np.cumsum(plen[:-1], out=pstart[1:])
    pool = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, dtype=np.uint8)
    nva = np.zeros(max(1, nf), dtype=_NVIN_DTYPE)
    if nf:
        base = np.uint64(pool.ctypes.data)
        nva["name"][:nf] = pstart[0::2] + base
        nva["value"][:nf] = pstart[1::2] + base
        nva["namelen"][:nf] = plen[0::2]
        nva["valuelen"][:nf] = plen[1::2]
        nva["flags"][:nf] = np.fromiter((f for _, _, f in flat), dtype=np.uint8, count=nf)
    offs = np.zeros(nb + 1, dtype=np.uint32)
    if nb:
        np.cumsum(np.fromiter((len(hl) for hl in header_lists), dtype=np.uint32, count=nb),
                  out=offs[1:])
    cap = int(plen.sum()) + 16 * nf + 16 * nb + 64 if out_cap is None else out_cap
    out = np.empty(max(1, cap), dtype=np.uint8)
    out_off = np.zeros(nb + 1, dtype=np.uint32)
    st = np.zeros(max(1, nb), dtype=np.int32)
    defl = np.fromiter((d.p.value for d in deflaters), dtype=np.uint64, count=nb) if nb \
        else np.zeros(1, dtype=np.uint64)
    s = None
    if stream is not None:
        s = ctypes.c_void_p(stream.cuda_stream)
    else:
        import torch
        if torch.cuda.is_available():
            s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = ctypes.c_void_p
    rv = L.nghttp2_amd_hd_deflate_blocks(vp(defl.ctypes.data), nb, vp(nva.ctypes.data),
                                         vp(offs.ctypes.data), vp(out.ctypes.data), cap,
                                         vp(out_off.ctypes.data), vp(st.ctypes.data), s)
    if rv not in (0, NGHTTP2_ERR_BUFFER_ERROR):
        _check(rv, "deflate_blocks")
    oo = out_off.tolist()
    raw = out[:oo[nb]].tobytes()
    return st[:nb].tolist(), [raw[oo[i]:oo[i + 1]] for i in range(nb)]


# ---------------------------------------------------------------------------
# Device-resident deflaters (nghttp2_amd_hd_dev_deflate*, nghttp2_amd_hd_deflate_plan_host)
# ---------------------------------------------------------------------------
DEV_NOTIFY = 0x8
DEV_OVERFLOW_WIRE, DEV_OVERFLOW_POOL = 0x1, 0x2  # (DEV_OVERFLOW_U32 is the inflaters')
PLAN_LIT_NAME, PLAN_LIT_VALUE = 0x1, 0x2
PLAN_REC_DTYPE = np.dtype([("bytes", "u1", (6,)), ("nbytes", "u1"), ("lits", "u1"), ("block", "<u4"),
                           ("reserved", "<u4")])
PLAN_HEAD_DTYPE = np.dtype([("bytes", "u1", (12,)), ("nbytes", "u1"), ("reserved", "u1", (3,))])
assert PLAN_REC_DTYPE.itemsize == 16 and PLAN_HEAD_DTYPE.itemsize == 16


def _dev_deflate_lib():
    L = _replay_lib()
    if not getattr(L, "_dev_deflate_bound", False):
        vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        L.nghttp2_amd_hd_dev_deflaters_new.argtypes = [ctypes.POINTER(vp), u32, u32, vp, vp]
        L.nghttp2_amd_hd_dev_deflaters_del.argtypes = [vp]
        L.nghttp2_amd_hd_dev_deflaters_del.restype = None
        L.nghttp2_amd_hd_dev_deflaters_change_table_size.argtypes = [vp, vp, vp, vp, u32, vp]
        L.nghttp2_amd_hd_dev_deflaters_read.argtypes = [vp, u32, vp, vp, vp, vp]
        L.nghttp2_amd_hd_dev_deflate_workspace_size.argtypes = [u32, u32, sz, sz, u32]
        L.nghttp2_amd_hd_dev_deflate_workspace_size.restype = sz
        L.nghttp2_amd_hd_dev_deflate_blocks.argtypes = [vp, vp, sz, vp, sz, vp, u32, vp, vp, vp, sz, vp, vp, vp, vp,
                                                        sz, vp]
        L.nghttp2_amd_hd_deflate_plan_host_init.argtypes = [vp, u32, u32]
        L.nghttp2_amd_hd_deflate_plan_host_change_table_size.argtypes = [vp, vp, u32, u32]
        L.nghttp2_amd_hd_deflate_plan_host.argtypes = [vp, vp, vp, vp, u32, vp, vp, sz, vp, u32, vp, vp]
        L._dev_deflate_bound = True
    return L


def pack_header_lists(header_lists):
    """Host header lists (each [(name, value[, flags])]) in the layout
    nghttp2_amd_hd_dev_inflate_blocks emits and the device deflaters take:
    (nva, arena, block_nv_off) numpy arrays -- _NV_DTYPE records, the arena of
    name, NUL, value, NUL per field with the pool rule's slack behind it
    (zeros), and uint32 offsets."""
    flat = [(bytes(h[0]), bytes(h[1]), h[2] if len(h) > 2 else 0, b)
            for b, hl in enumerate(header_lists) for h in hl]
    nva = np.zeros(max(1, len(flat)), _NV_DTYPE)
    parts, at = [], 0
    for k, (n, v, fl, b) in enumerate(flat):
        nva[k] = (b, at, len(n), at + len(n) + 1, len(v), fl)
        parts += [n, b"\0", v, b"\0"]
        at += len(n) + len(v) + 2
    arena = np.zeros((at + 15) // 16 * 16 + 32, np.uint8)
    arena[:at] = np.frombuffer(b"".join(parts), np.uint8)
    off = np.zeros(len(header_lists) + 1, np.uint32)
    np.cumsum([len(hl) for hl in header_lists], out=off[1:])
    return nva[:len(flat)], arena, off


class HostDeflatePlanner:
    """One connection of a DeviceDeflaters set on the host
    (nghttp2_amd_hd_deflate_plan_host; no GPU): the same header, ring, keys
    and stores, walked by the same code.  What the device results are
    compared with."""

    def __init__(self, table_bytes=4096, deflate_max=4096):
        self.L = _dev_deflate_lib()
        self.table_bytes = int(table_bytes)
        self.hdr = np.zeros(1, DEV_CONN_DTYPE)
        self.ring = np.zeros(self.table_bytes // 32 * 4, np.uint32)
        self.keys = np.zeros(self.table_bytes // 32, np.uint32)
        self.store = np.zeros(2 * self.table_bytes, np.uint8)
        _check(self.L.nghttp2_amd_hd_deflate_plan_host_init(self.hdr.ctypes.data, self.table_bytes, int(deflate_max)),
               "deflate_plan_host_init")

    def change_table_size(self, value):
        _check(self.L.nghttp2_amd_hd_deflate_plan_host_change_table_size(
            self.hdr.ctypes.data, self.ring.ctypes.data, self.table_bytes, int(value)),
            "deflate_plan_host_change_table_size")
        return 0

    def plan_packed(self, nva, arena, block_nv_off):
        """The plan of packed lists (pack_header_lists' arrays), every block
        on this connection in order: (recs, heads) as PLAN_REC_DTYPE /
        PLAN_HEAD_DTYPE arrays."""
        n = len(block_nv_off) - 1
        nva = np.ascontiguousarray(nva, _NV_DTYPE)
        block_nv_off = np.ascontiguousarray(block_nv_off, np.uint32)
        recs = np.zeros(max(1, len(nva)), PLAN_REC_DTYPE)
        heads = np.zeros(max(1, n), PLAN_HEAD_DTYPE)
        _check(self.L.nghttp2_amd_hd_deflate_plan_host(
            self.hdr.ctypes.data, self.ring.ctypes.data, self.keys.ctypes.data, self.store.ctypes.data,
            self.table_bytes, nva.ctypes.data if len(nva) else None, arena.ctypes.data, len(arena),
            block_nv_off.ctypes.data, n, recs.ctypes.data, heads.ctypes.data), "deflate_plan_host")
        return recs[:len(nva)], heads[:n]

    def plan(self, header_lists):
        """plan_packed of host header lists; also returns the packed arrays:
        (recs, heads, nva, arena, block_nv_off)."""
        nva, arena, off = pack_header_lists(header_lists)
        return self.plan_packed(nva, arena, off) + (nva, arena, off)

    def table(self):
        """[(name, value)] of the dynamic table, most recent first."""
        return _host_table(self.hdr[0], self.ring, self.store, self.table_bytes)

    def table_size(self):
        return int(self.hdr[0]["size"])

    def table_max(self):
        return int(self.hdr[0]["max"])

    def state(self):
        return self.table(), self.table_size(), self.table_max()


class DeviceDeflaters(_DeviceSet):
    """nconn HPACK encoding contexts in device memory
    (nghttp2_amd_hd_dev_deflaters): header lists that lie on the device --
    a ReplayedBlocks of DeviceInflaters, or packed (nva, arena, block_nv_off)
    tensors -- into wire on the device.  deflate_max is one value for every
    connection, a sequence of nconn, or None for 4096; each at most
    table_bytes.  Calls on one set are ordered by their stream."""

    _PREFIX = "dev_deflaters"

    def __init__(self, nconn, table_bytes=4096, deflate_max=None, device=None, stream=None):
        self._ws = None
        dm = None
        if deflate_max is not None:
            dm = np.full(int(nconn), deflate_max, np.uint32) if np.isscalar(deflate_max) else \
                np.ascontiguousarray(deflate_max, np.uint32)
            if len(dm) != int(nconn):
                raise ValueError("deflate_max: one value per connection")
        self._new(_dev_deflate_lib(), nconn, table_bytes, device, stream, dm.ctypes.data if dm is not None else None)

    def state(self, c, stream=None):
        """(table, size, max) in one read."""
        h, ent, raw = self._read(c, stream)
        return _conn_state(h, ent, raw), int(h["size"]), int(h["max"])

    def upload(self, header_lists):
        """pack_header_lists' arrays as device tensors (nva, arena,
        block_nv_off), for deflate."""
        nva, arena, off = pack_header_lists(header_lists)
        t = self.torch
        nv = np.ascontiguousarray(nva).view(np.uint8) if len(nva) else np.zeros(_NV_DTYPE.itemsize, np.uint8)
        return (t.from_numpy(nv.copy()).to(self.device), t.from_numpy(arena).to(self.device),
                t.from_numpy(off.view(np.int32)).to(self.device))

    @staticmethod
    def bound(nblocks, nva_cap, arena_bytes):
        """An out_cap that cannot overflow: nghttp2_hd_deflate_bound summed."""
        return 12 * nblocks + 12 * nva_cap + arena_bytes

    def deflate(self, fields, conn_blk_off, conn_blk, out_cap=None, stream=None, out=None):
        """nghttp2_amd_hd_dev_deflate_blocks: fields is a ReplayedBlocks or
        (nva, arena, block_nv_off) device tensors, conn_blk_off / conn_blk
        the CSR of csr().  Returns (out, out_off, out_status, totals) device
        tensors: block i's wire is out[out_off[i]:out_off[i+1]], totals =
        {wire bytes, literal pool bytes, DEV_OVERFLOW_* bits, 0}.  Nothing is
        read back; without an out_cap the bound that cannot overflow is used,
        with one an overflow is the caller's to see in totals[2] (no wire, no
        table changed: repeat with room).  out: a uint8 device tensor to
        write the wire to (its size is the out_cap when none is given)."""
        torch = self.torch
        if isinstance(fields, ReplayedBlocks):
            nva, arena, nv_off = fields.nva, fields.arena, fields.block_nv_off
        else:
            nva, arena, nv_off = fields
        n = nv_off.numel() - 1
        nva_cap = nva.numel() * nva.element_size() // _NV_DTYPE.itemsize
        # how far the arena is readable: to the end of its allocation
        arena_bytes = arena.untyped_storage().nbytes() - arena.storage_offset() * arena.element_size()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if out is not None and out_cap is None:
            out_cap = out.numel()
        cap = self.bound(n, nva_cap, arena_bytes) if out_cap is None else int(out_cap)
        if out is not None and (out.numel() < cap or out.dtype != torch.uint8):
            raise ValueError("out: a uint8 tensor of at least out_cap bytes")
        need = self.L.nghttp2_amd_hd_dev_deflate_workspace_size(self.nconn, self.table_bytes, nva_cap, arena_bytes, n)
        with torch.cuda.stream(s):
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            if out is None:
                out = torch.empty(max(1, cap), dtype=torch.uint8, device=self.device)
            out_off = torch.zeros(n + 1, dtype=torch.int32, device=self.device)
            out_status = torch.zeros(max(1, n), dtype=torch.int32, device=self.device)
            totals = torch.zeros(4, dtype=torch.int32, device=self.device)
        rv = self.L.nghttp2_amd_hd_dev_deflate_blocks(
            self.p, _p(nva), nva_cap, _p(arena), arena_bytes, _p(nv_off), n, _p(conn_blk_off), _p(conn_blk),
            _p(out), cap, _p(out_off), _p(out_status), _p(totals), _p(self._ws), self._ws.numel(),
            ctypes.c_void_p(s.cuda_stream))
        _check(rv, "dev_deflate_blocks")
        return out[:cap], out_off, out_status[:n], totals


def deflated_wire(out, out_off, totals=None):
    """A device deflate's wire read back (synchronises): [bytes] per block.
    With the call's totals, a call that overflowed (totals[2] != 0: out was
    not written) raises instead of returning what out happened to hold."""
    if totals is not None:
        t = totals.cpu().numpy().view(np.uint32).tolist()
        if t[2]:
            raise RuntimeError("nghttp2_amd: the deflate overflowed (totals = %r): no wire was written" % (t,))
    off = out_off.cpu().numpy().view(np.uint32).tolist()
    raw = out[:off[-1]].cpu().numpy().tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
