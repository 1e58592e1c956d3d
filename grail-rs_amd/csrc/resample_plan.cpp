// resample_plan.cpp — the host side of sample-rate conversion that needs no device: grail_resample_ratio (a pair of rates
// -> up, down, taps), grail_resample_coefficients (the Kaiser-windowed sinc as integers over 2^26) and grail_resample_len.
// The contract is include/grail_hip.h, "levels, continued: sample-rate conversion".  No HIP call, so it builds with g++
// under AddressSanitizer and UBSan (tests/test_resample_sanitize.py), as mix_plan.cpp and level_gains.cpp do.
// DESIGN.md §4.13.  Also grail_resample_stream_len, the ring's capacity and the checks of the calls on resample streams
// (tests/test_resample_stream_sanitize.py; §4.16; where they end as every stream's do: row_checks.h).
#include <cmath>
#include <cstdint>

#include "../../include/grail_hip.h"
#include "fir_plan.h"
#include "resample_plan.h"
#include "row_checks.h"

namespace grail {

// I0 by its power series: the terms ((y / 2)^k / k!)^2 ascending until one no longer changes the sum
double bessel_i0(double y)
{
    double sum = 1.0, t = 1.0;
    for (uint32_t k = 1;; ++k) {
        t = t * (y / 2.0) / (double)k;
        const double next = sum + t * t;
        if (next == sum) return sum;
        sum = next;
    }
}

// sin(pi a) / (pi a), 1 at 0
double sinc_pi(double a)
{
    constexpr double PI = 3.14159265358979323846;
    return a == 0.0 ? 1.0 : std::sin(PI * a) / (PI * a);
}

}  // namespace grail

namespace {

using grail::bessel_i0;

constexpr double RESAMPLE_BETA = 8.0;

uint32_t gcd32(uint32_t a, uint32_t b)
{
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// U, D, P of a pair, or false: a rate of 0, equal rates, more than GRAIL_RESAMPLE_TABLE_MAX entries
bool ratio(uint32_t rate_in, uint32_t rate_out, uint32_t *U, uint32_t *D, uint32_t *P)
{
    if (rate_in == 0 || rate_out == 0 || rate_in == rate_out) return false;
    const uint32_t g = gcd32(rate_in, rate_out);
    const uint64_t u = rate_out / g, d = rate_in / g, longer = u > d ? u : d;
    const uint64_t half = (GRAIL_RESAMPLE_ZERO_CROSSINGS * longer + u - 1) / u;      // < 2^37
    if (u * 2 * half > GRAIL_RESAMPLE_TABLE_MAX) return false;                       // (u < 2^32, half < 2^37: no overflow)
    *U = (uint32_t)u, *D = (uint32_t)d, *P = (uint32_t)(2 * half);
    return true;
}

// N(j) = llrint(H(|j|) * 2^26): |j| makes the table even by construction
int32_t numerator(int64_t j, uint32_t U, double f, double W, double i0_beta)
{
    const double x = (double)(j < 0 ? -j : j) / (double)U;
    const double a = f * x;
    const double sinc = grail::sinc_pi(a);
    const double r = x / W;
    const double under = 1.0 - r * r;
    const double window = bessel_i0(RESAMPLE_BETA * std::sqrt(under > 0.0 ? under : 0.0)) / i0_beta;
    return (int32_t)std::llrint(f * sinc * window * 67108864.0);
}

// E(N): the outputs known after N samples, 0 for N <= h, else ceil((N - h) U / D)
unsigned __int128 known_outputs(uint64_t N, uint32_t U, uint32_t D, uint32_t P)
{
    const uint64_t h = P / 2;
    return N <= h ? 0 : ((unsigned __int128)(N - h) * U + (D - 1u)) / D;
}

}  // namespace

namespace grail {

uint32_t resample_stream_ring_capacity(uint32_t taps)
{
    uint32_t cap = 1;
    while (cap < taps - 1u && cap < GRAIL_RESAMPLE_TABLE_MAX) cap <<= 1;        // (taps >= 2; U taps <= the table's limit)
    return cap;
}

unsigned __int128 resample_stream_most(uint64_t n, uint32_t U, uint32_t D) { return ((unsigned __int128)n * U + (D - 1u)) / D; }

uint64_t resample_stream_tail(uint32_t U, uint32_t D, uint32_t taps) { return (uint64_t)resample_stream_most(taps / 2u, U, D); }

const char *resample_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, const void *out,
                                       uint64_t out_stride, uint32_t U, uint32_t D, uint64_t *chunks)
{
    *chunks = 0;
    if ((unsigned __int128)out_stride < resample_stream_most(in_stride, U, D))
        return "out_stride < ceil(in_stride * up / down) (a stream never cuts outputs short)";
    // (a stream has rows: grail_resample_stream_open; a call feeds a row fewer than 2^32 samples: in_len is 32 bits wide)
    const uint64_t longest = (uint64_t)resample_stream_most(in_stride < 0xFFFFFFFFull ? in_stride : 0xFFFFFFFFull, U, D);
    return stream_next_error({in, in_stride, in_len, n_rows, out, out_stride}, longest, n_rows, RESAMPLE_STREAM_CHUNK, chunks);
}

const char *resample_stream_finish_error(const void *out, uint64_t out_stride, uint32_t n_rows, uint32_t U, uint32_t D, uint32_t taps,
                                         uint64_t *chunks)
{
    *chunks = 0;
    const uint64_t tail = resample_stream_tail(U, D, taps);         // at least 1
    if (out_stride < tail) return "out_stride < ceil((taps / 2) * up / down), the longest tail";
    return stream_finish_error(out, out_stride, n_rows, tail, n_rows, RESAMPLE_STREAM_CHUNK, chunks);
}

}  // namespace grail

extern "C" {

int grail_resample_stream_len(uint64_t fed_before, uint64_t n, uint32_t rate_in, uint32_t rate_out, int finishing, uint64_t *n_out)
{
    uint32_t U, D, P;
    if (!n_out || !ratio(rate_in, rate_out, &U, &D, &P)) return GRAIL_ERR_INVALID_ARG;
    if ((finishing && n) || fed_before > UINT64_MAX - n) return GRAIL_ERR_INVALID_ARG;
    const unsigned __int128 before = known_outputs(fed_before, U, D, P);
    const unsigned __int128 count = finishing ? grail::resample_stream_most(fed_before, U, D) - before
                                              : known_outputs(fed_before + n, U, D, P) - before;
    if (count > (unsigned __int128)UINT64_MAX) return GRAIL_ERR_INVALID_ARG;
    *n_out = (uint64_t)count;
    return GRAIL_OK;
}

int grail_resample_ratio(uint32_t rate_in, uint32_t rate_out, uint32_t *up, uint32_t *down, uint32_t *taps)
{
    uint32_t U, D, P;
    if (!ratio(rate_in, rate_out, &U, &D, &P)) return GRAIL_ERR_INVALID_ARG;
    if (up) *up = U;
    if (down) *down = D;
    if (taps) *taps = P;
    return GRAIL_OK;
}

int grail_resample_coefficients(uint32_t rate_in, uint32_t rate_out, int32_t *num, uint32_t cap)
{
    uint32_t U, D, P;
    if (!num || !ratio(rate_in, rate_out, &U, &D, &P) || cap < U * P) return GRAIL_ERR_INVALID_ARG;
    const double f = U < D ? 0.9 * ((double)U / (double)D) : 0.9;
    const double W = (double)(P / 2), i0_beta = bessel_i0(RESAMPLE_BETA);
    for (uint32_t p = 0; p < U; ++p)
        for (uint32_t k = 0; k < P; ++k)
            num[(size_t)p * P + k] = numerator(((int64_t)k - (int64_t)(P / 2)) * (int64_t)U + (int64_t)p, U, f, W, i0_beta);
    return GRAIL_OK;
}

int grail_resample_len(uint64_t n, uint32_t rate_in, uint32_t rate_out, uint64_t *n_out)
{
    uint32_t U, D, P;
    if (!n_out || !ratio(rate_in, rate_out, &U, &D, &P)) return GRAIL_ERR_INVALID_ARG;
    const unsigned __int128 out = ((unsigned __int128)n * U + (D - 1u)) / D;
    if (out > (unsigned __int128)UINT64_MAX) return GRAIL_ERR_INVALID_ARG;
    *n_out = (uint64_t)out;
    return GRAIL_OK;
}

}  // extern "C"
