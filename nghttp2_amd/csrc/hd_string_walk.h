// hd_string_walk.h -- which bytes a string of the batch layout owns (byte pool
// + uint32 offsets[n+1], optionally a length per string): the one statement of
// the rule for k_check_fields (hd_check.hip), k_http_facts (hd_http.hip) and
// k_name_tokens<true> (hd_names.hip).  The wave walk of the first two is still
// written out in each of them: behind a forced-inline template the same
// statements compiled to another instruction order that measured slower on
// short strings.
#pragma once

#include "hd_wave.h"

namespace hdwalk {

// String s of (off, len): its bytes [a, b) when it is examined, else the
// empty [0, 0), which reads nothing.  o0 <= o1 first, so o1 - o0 cannot wrap;
// a length is compared with that room, never added to an offset before it is
// known to fit.  `len` is optional: without it the string ends at off[s + 1].
// (The offsets are loaded ahead of the length, as k_check_fields always did;
// the length first, as the length form of the name kernel once had it, measured
// no faster there and slower in the check: DESIGN.md 2.10.)
struct Range {
  uint32_t a, b;
  bool valid;
};
__device__ __forceinline__ Range string_range(const uint32_t *off, const int32_t *len, uint32_t s) {
  const uint32_t o0 = off[s], o1 = off[s + 1];
  uint32_t l = o1 - o0;
  bool valid = o0 <= o1;
  if (len) {
    const int32_t li = len[s];
    valid = valid && li >= 0 && (uint32_t)li <= l;
    l = (uint32_t)li;
  }
  Range r = {0u, 0u, valid};
  if (valid) {
    r.a = o0;
    r.b = o0 + l;
  }
  return r;
}

}  // namespace hdwalk
