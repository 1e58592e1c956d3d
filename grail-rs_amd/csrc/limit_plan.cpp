// limit_plan.cpp — the host side of limit streams that needs no device: E(N) and grail_limit_stream_len, the ring's capacity,
// and the checks of the calls on limit streams (where they end as every stream's do: row_checks.h).  The contract is
// include/grail_hip.h, "levels, continued: the limiter on streams".  No HIP call, so it builds with g++ under AddressSanitizer
// and UBSan (tests/test_limit_stream_sanitize.py), as fir_plan.cpp and resample_plan.cpp do.  DESIGN.md §4.17.
#include <cstdint>

#include "../../include/grail_hip.h"
#include "limit_plan.h"
#include "row_checks.h"

namespace grail {

uint32_t limit_stream_delay(uint32_t ell) { return GRAIL_LIMIT_STREAM_DELAY(ell); }

uint64_t limit_stream_known(uint64_t fed, uint32_t ell)
{
    const uint64_t delay = limit_stream_delay(ell);
    return fed > delay ? fed - delay : 0;
}

uint32_t limit_stream_ring_capacity(uint32_t ell)
{
    // the oldest sample the next output may still need is x[N - 3 L - 19]
    const uint32_t need = 3u * (1u << ell) + 19u;
    uint32_t cap = 32;
    while (cap < need) cap <<= 1;
    return cap;
}

const char *limit_stream_open_error(uint32_t n_rows, uint32_t group, float ceiling, uint32_t ell)
{
    if (ell > GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX) return "lookahead_log2 is above 10";
    if (group == 0 || n_rows % group != 0) return "n_rows is no multiple of group";
    if (!(ceiling > 0.0f) || !(ceiling <= 3.4028234663852886e38f)) return "the ceiling is not a finite number above 0";
    if (n_rows == 0) return "n_rows is 0";
    return nullptr;
}

// (a stream has rows in whole groups: limit_stream_open_error; a call feeds a row fewer than 2^32 samples: in_len is 32 bits wide)
const char *limit_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, uint32_t group,
                                    const void *out, uint64_t out_stride, uint64_t *chunks)
{
    *chunks = 0;
    if (out_stride < in_stride) return "out_stride < in_stride (a stream never cuts outputs short)";
    const uint64_t longest = in_stride < 0xFFFFFFFFull ? in_stride : 0xFFFFFFFFull;
    return stream_next_error({in, in_stride, in_len, n_rows, out, out_stride}, longest, n_rows / group, GRAIL_LIMIT_CHUNK, chunks);
}

const char *limit_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t group, uint32_t ell,
                                      uint64_t *chunks)
{
    *chunks = 0;
    const uint32_t tail = limit_stream_delay(ell);
    if (out_stride < tail) return "out_stride is below the stream's delay, GRAIL_LIMIT_STREAM_DELAY(lookahead_log2)";
    return stream_finish_error(out, out_stride, n_rows, tail, n_rows / group, GRAIL_LIMIT_CHUNK, chunks);
}

}  // namespace grail

extern "C" {

int grail_limit_stream_len(uint64_t fed_before, uint64_t n, uint32_t lookahead_log2, int finishing, uint64_t *n_out)
{
    if (!n_out || lookahead_log2 > GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX) return GRAIL_ERR_INVALID_ARG;
    if ((finishing && n) || fed_before > UINT64_MAX - n) return GRAIL_ERR_INVALID_ARG;
    const uint64_t known = grail::limit_stream_known(fed_before, lookahead_log2);
    *n_out = finishing ? fed_before - known : grail::limit_stream_known(fed_before + n, lookahead_log2) - known;
    return GRAIL_OK;
}

}  // extern "C"
