"""nghttp2_amd -- MI355X-native HPACK Huffman engine (host side).

The product is the HIP/C shared library nghttp2_amd/lib/libnghttp2_amd_hd.so
(sources in nghttp2_amd/csrc, C ABI in include/nghttp2_amd_hd.h).  This
package is the thin Python binding over that C ABI used by bench.py, the
batched drivers and the tests: torch is only the device-memory / stream
plumbing.  There is no CPU fallback: every compute call goes to the HIP
library and raises if it is missing.
"""
from .hd import (  # noqa: F401
    CHECK_AUTHORITY,
    CHECK_INVALID,
    CHECK_METHOD,
    CHECK_NAME,
    CHECK_NAME_LOWER,
    CHECK_PATH,
    CHECK_VALUE,
    CHECK_VALUE_RFC9113,
    DeviceDeflaters,
    DeviceInflaters,
    HostDeflatePlanner,
    HostReplayInflater,
    HpackDeflater,
    HpackInflater,
    HuffmanBatchCodec,
    NGHTTP2_ERR_BUFFER_ERROR,
    NGHTTP2_ERR_HEADER_COMP,
    NGHTTP2_ERR_INVALID_STATE,
    NGHTTP2_ERR_INSUFF_BUFSIZE,
    NGHTTP2_ERR_INVALID_ARGUMENT,
    NGHTTP2_ERR_NOMEM,
    TOKEN_INVALID,
    TOKEN_NONE,
    check_field,
    decode_length,
    lib,
    pack_header_lists,
    parse_block,
    replay_annotated,
    replay_fields,
    lib_path,
    deflate_blocks,
    inflate_blocks,
    tables_ref_layout,
)

__version__ = "0.1.0"
