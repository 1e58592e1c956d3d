// meter_plan.cpp — the host side of meter streams that needs no device: the hop of a rate, grail_meter_stream_hops, the stride
// rule of a call's hop sums, and the checks of open and next (where they end as every stream's do: row_checks.h).  The contract
// is include/grail_hip.h, "levels, continued: the meters on streams".  No HIP call, so it builds with g++ under AddressSanitizer
// and UBSan (tests/test_meter_stream_sanitize.py), as limit_plan.cpp does.  DESIGN.md §4.18.
#include <cstdint>

#include "../../include/grail_hip.h"
#include "meter_plan.h"
#include "row_checks.h"

namespace grail {

namespace {
constexpr uint32_t METER_CHUNK = 4096;      // METER_STREAM_CHUNK of kernels.h (which is HIP's to include)
}

uint32_t meter_stream_hop(uint32_t sample_rate)
{
    return sample_rate < GRAIL_LOUDNESS_RATE_MIN || sample_rate > GRAIL_LOUDNESS_RATE_MAX ? 0u : sample_rate / 10u;
}

uint64_t meter_stream_hops(uint64_t fed_before, uint64_t n, uint32_t hop) { return (fed_before + n) / hop - fed_before / hop; }

uint64_t meter_stream_hops_stride(uint64_t in_stride, uint32_t hop) { return in_stride / hop + (in_stride % hop != 0u); }

const char *meter_stream_open_error(uint32_t n_rows, uint32_t sample_rate, uint64_t max_hops)
{
    if (!meter_stream_hop(sample_rate)) return "sample_rate is outside GRAIL_LOUDNESS_RATE_MIN .. GRAIL_LOUDNESS_RATE_MAX";
    if (n_rows == 0) return "n_rows is 0";
    if (max_hops == 0) return "max_hops is 0";
    if (max_hops > (SIZE_MAX / 8u) / n_rows) return "n_rows x max_hops x 8 bytes of ledger do not fit size_t";
    return nullptr;
}

// (a call feeds a row fewer than 2^32 samples: in_len is 32 bits wide)
const char *meter_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *hop_sumsq,
                                    uint64_t hops_stride, uint32_t hop, uint64_t *chunks)
{
    *chunks = 0;
    if (!in_len || (in_stride && !in)) return ROWS_NULL;
    if (in_stride == 0) return nullptr;
    if (!rows_span_fits(in_stride, n_rows)) return ROWS_SPAN;
    if (hop_sumsq) {
        if (hops_stride < meter_stream_hops_stride(in_stride, hop)) return "hops_stride < (in_stride + H - 1) / H, the most hops a call can complete";
        if (!rows_span_fits(hops_stride, n_rows)) return ROWS_SPAN;
    }
    *chunks = stream_chunks(in_stride, METER_CHUNK);
    return (uint64_t)n_rows * *chunks > 0x7FFFFFFFull ? STREAM_CHUNKS : nullptr;
}

}  // namespace grail

extern "C" {

int grail_meter_stream_hops(uint64_t fed_before, uint64_t n, uint32_t sample_rate, uint64_t *n_hops)
{
    const uint32_t hop = grail::meter_stream_hop(sample_rate);
    if (!n_hops || !hop || fed_before > UINT64_MAX - n) return GRAIL_ERR_INVALID_ARG;
    *n_hops = grail::meter_stream_hops(fed_before, n, hop);
    return GRAIL_OK;
}

}  // extern "C"
