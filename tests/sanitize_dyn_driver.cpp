// Drives the pure-host side of dynamics (csrc/dyn_plan.cpp: grail_dyn_design, grail_dyn_ballistics, lev[k], the lookup's index
// arithmetic, a set's checks and image, the checks of grail_dyn_async and of the stream calls) under AddressSanitizer and UBSan
// (tests/test_dyn_sanitize.py builds and runs it): every array lives on the heap at exactly the size the call is entitled to,
// so that a read or write one element past it is caught, and the lookup is walked at every edge of its table.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/dyn_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize dyn driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

using namespace grail;

static bool says(const char *why, const char *word) { return why && std::strstr(why, word); }

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint32_t P = GRAIL_DYN_POINTS;
    CHECK(P == 641 && DYN_POINTS == P);

    // the designer into exactly 641 doubles, both kinds and detectors; the refusals write nothing
    std::unique_ptr<double[]> gain(new double[P]);
    for (int kind : {GRAIL_DYN_COMPRESS, GRAIL_DYN_EXPAND})
        for (int det : {GRAIL_DYN_PEAK, GRAIL_DYN_SQUARE}) {
            for (uint32_t k = 0; k < P; ++k) gain[k] = -77.0;
            CHECK(grail_dyn_design(kind, det, -24.0, 4.0, 6.0, 40.0, 3.0, gain.get()) == GRAIL_OK);
            for (uint32_t k = 0; k < P; ++k) CHECK(std::isfinite(gain[k]) && gain[k] > 0.0);
            CHECK(grail_dyn_design(kind, det, -24.0, 1e9, 0.0, 200.0, 0.0, gain.get()) == GRAIL_OK);
            for (uint32_t k = 0; k < P; ++k) CHECK(std::isfinite(gain[k]) && gain[k] >= 0.0 && gain[k] <= 1.0);
        }
    for (uint32_t k = 0; k < P; ++k) gain[k] = -77.0;
    CHECK(grail_dyn_design(2, 0, -24.0, 4.0, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_dyn_design(-1, 0, -24.0, 4.0, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_dyn_design(0, 2, -24.0, 4.0, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_dyn_design(0, -1, -24.0, 4.0, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_dyn_design(0, 0, nan, 4.0, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_dyn_design(0, 0, inf, 4.0, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    for (double ratio : {0.999, 0.0, -2.0, nan, inf}) CHECK(grail_dyn_design(0, 0, -24.0, ratio, 6.0, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    for (double neg : {-1e-9, nan, inf, -inf}) {
        CHECK(grail_dyn_design(0, 0, -24.0, 4.0, neg, 0.0, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_dyn_design(1, 0, -24.0, 4.0, 6.0, neg, 0.0, gain.get()) == GRAIL_ERR_INVALID_ARG);
    }
    for (double makeup : {nan, inf, -inf, 1e5}) CHECK(grail_dyn_design(0, 0, -24.0, 4.0, 6.0, 0.0, makeup, gain.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_dyn_design(0, 0, -24.0, 4.0, 6.0, 0.0, 0.0, nullptr) == GRAIL_ERR_INVALID_ARG);
    for (uint32_t k = 0; k < P; ++k) CHECK(gain[k] == -77.0);

    // the ballistics into exactly two doubles
    std::unique_ptr<double[]> alpha(new double[2]);
    alpha[0] = alpha[1] = -77.0;
    CHECK(grail_dyn_ballistics(0, 1.0, 1.0, alpha.get()) == GRAIL_ERR_INVALID_ARG && grail_dyn_ballistics(48000, 1.0, 1.0, nullptr) == GRAIL_ERR_INVALID_ARG);
    for (double ms : {-1.0, nan, inf, 1e300})
        CHECK(grail_dyn_ballistics(48000, ms, 1.0, alpha.get()) == GRAIL_ERR_INVALID_ARG && grail_dyn_ballistics(48000, 1.0, ms, alpha.get()) == GRAIL_ERR_INVALID_ARG);
    CHECK(alpha[0] == -77.0 && alpha[1] == -77.0);
    CHECK(grail_dyn_ballistics(48000, 0.0, 120.0, alpha.get()) == GRAIL_OK && alpha[0] == 0.0 && !std::signbit(alpha[0]) && alpha[1] > 0.99 && alpha[1] < 1.0);
    CHECK(grail_dyn_ballistics(0xFFFFFFFFu, 5e-324, 1e6, alpha.get()) == GRAIL_OK && alpha[0] == 0.0 && alpha[1] < 1.0);

    // the lookup's index arithmetic on a table of exactly 641 doubles, G[k] = k: curve(lev[k]) = k, and just below it k - 2^-48
    std::unique_ptr<double[]> stairs(new double[P]);
    for (uint32_t k = 0; k < P; ++k) stairs[k] = (double)k;
    uint32_t k;
    double f;
    bool inside;
    const double lo = std::ldexp(1.0, GRAIL_DYN_LOG2_LO), hi = std::ldexp(1.0, GRAIL_DYN_LOG2_HI);
    CHECK(dyn_level(0) == lo && dyn_level(P - 1) == hi && dyn_level(16) == 2.0 * lo && dyn_level(17) == 2.0 * lo * 1.0625);
    for (double e : {0.0, 5e-324, 2.2250738585072014e-308, std::nextafter(lo, 0.0)}) {
        dyn_index(e, &k, &f, &inside);
        CHECK(k == 0 && !inside && f == 0.0 && dyn_lookup(stairs.get(), e) == 0.0);
    }
    dyn_index(lo, &k, &f, &inside);
    CHECK(k == 0 && inside && f == 0.0 && dyn_lookup(stairs.get(), lo) == 0.0);
    dyn_index(std::nextafter(lo, 1.0), &k, &f, &inside);
    CHECK(k == 0 && inside && f == std::ldexp(1.0, -48));       // (one unit of the mantissa is 2^-48 of a step)
    for (uint32_t j = 0; j < P; ++j) {
        const double lev = dyn_level(j);
        dyn_index(lev, &k, &f, &inside);
        CHECK(k == j && f == 0.0 && inside == (j + 1 < P));
        CHECK(dyn_lookup(stairs.get(), lev) == (double)j);
        if (j == 0) continue;
        const double below = std::nextafter(lev, 0.0);
        dyn_index(below, &k, &f, &inside);
        CHECK(k == j - 1 && inside && f == 1.0 - std::ldexp(1.0, -48));
        CHECK(dyn_lookup(stairs.get(), below) == (double)(j - 1) + f);
    }
    for (double e : {hi, std::nextafter(hi, inf), 1e300, std::numeric_limits<double>::max()}) {
        dyn_index(e, &k, &f, &inside);
        CHECK(k == P - 1 && !inside && f == 0.0 && dyn_lookup(stairs.get(), e) == (double)(P - 1));
    }
    dyn_index(std::nextafter(hi, 0.0), &k, &f, &inside);
    CHECK(k == P - 2 && inside);

    // a set: the checks read exactly n_curves curves, the image is exactly [n_curves][641] pairs
    for (uint32_t C : {1u, 3u, 16u}) {
        std::unique_ptr<double[]> g(new double[(size_t)C * P]), a(new double[2 * C]);
        std::unique_ptr<uint32_t[]> d(new uint32_t[C]);
        for (uint32_t i = 0; i < C * P; ++i) g[i] = (double)(i % 97) / 64.0;
        for (uint32_t i = 0; i < 2 * C; ++i) a[i] = (double)i / (2.0 * C);
        for (uint32_t i = 0; i < C; ++i) d[i] = i & 1u;
        CHECK(dyn_set_error(g.get(), a.get(), d.get(), C) == nullptr);
        std::vector<double> image;
        dyn_set_image(g.get(), C, image);
        CHECK(image.size() == (size_t)C * DYN_IMAGE_DOUBLES);
        for (uint32_t c = 0; c < C; ++c)
            for (uint32_t j = 0; j < P; ++j) {
                const double *pair = image.data() + (size_t)c * DYN_IMAGE_DOUBLES + 2 * j;
                CHECK(pair[0] == g[c * P + j] && pair[1] == (j + 1 < P ? g[c * P + j + 1] - g[c * P + j] : 0.0));
            }
        g[(size_t)C * P - 1] = nan;
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), C), "not finite"));
        g[(size_t)C * P - 1] = -0.5;
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), C), "negative"));
        g[(size_t)C * P - 1] = 0.0;
        a[2 * C - 1] = 1.0;
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), C), "alpha"));
        a[2 * C - 1] = nan;
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), C), "alpha"));
        a[2 * C - 1] = 0.5, a[0] = -1e-300;
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), C), "alpha"));
        a[0] = 0.0, d[C - 1] = 2;
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), C), "detector"));
        d[C - 1] = 1;
        CHECK(dyn_set_error(g.get(), a.get(), d.get(), C) == nullptr);
        CHECK(says(dyn_set_error(nullptr, a.get(), d.get(), C), "NULL") && says(dyn_set_error(g.get(), nullptr, d.get(), C), "NULL") &&
              says(dyn_set_error(g.get(), a.get(), nullptr, C), "NULL"));
        CHECK(says(dyn_set_error(g.get(), a.get(), d.get(), 0), "outside") && says(dyn_set_error(g.get(), a.get(), d.get(), 17), "outside"));
    }

    // the calls: addresses are compared, never looked behind
    const char *a = (const char *)0x10000000, *b = (const char *)0x20000000, *key = (const char *)0x30000000, *ln = (const char *)0x40000000;
    CHECK(dyn_call_error(a, 64, ln, 2, nullptr, 0, 0, nullptr, b, 64) == nullptr);
    CHECK(dyn_call_error(nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0) == nullptr);
    CHECK(dyn_call_error(a, 64, ln, 2, nullptr, 0, 0, nullptr, nullptr, 0) == nullptr);                 // (the results only)
    CHECK(says(dyn_call_error(a, 64, nullptr, 2, nullptr, 0, 0, nullptr, b, 64), "NULL buffer"));
    CHECK(says(dyn_call_error(nullptr, 64, ln, 2, nullptr, 0, 0, nullptr, b, 64), "NULL buffer"));
    CHECK(says(dyn_call_error(a, 64, ln, 2, nullptr, 0, 0, nullptr, nullptr, 64), "NULL buffer"));
    CHECK(says(dyn_call_error(a, 64, ln, 2, nullptr, 0, 0, nullptr, a + 4 * 127, 64), "overlaps rows_dev"));
    CHECK(dyn_call_error(a, 64, ln, 2, nullptr, 0, 0, nullptr, a + 4 * 128, 64) == nullptr);
    CHECK(says(dyn_call_error(a, 1ull << 59, ln, 4, nullptr, 0, 0, nullptr, b, 64), "2^60"));
    CHECK(says(dyn_call_error(a, 1ull << 32, ln, 1, nullptr, 0, 0, nullptr, (const char *)(1ull << 50), 1ull << 32), "2^32"));
    CHECK(dyn_call_error(a, 1ull << 32, ln, 1, nullptr, 0, 0, nullptr, (const char *)(1ull << 50), 0xFFFFFFFFull) == nullptr);
    CHECK(dyn_call_error(a, 64, ln, 2, key, 64, 2, nullptr, b, 64) == nullptr && dyn_call_error(a, 64, ln, 2, key, 64, 1, ln, b, 64) == nullptr);
    CHECK(dyn_call_error(a, 64, ln, 2, a, 64, 2, nullptr, b, 64) == nullptr);                            // (a row may be its own key)
    CHECK(dyn_call_error(a, 64, ln, 2, key, 0, 2, nullptr, b, 64) == nullptr);                           // (keys of no samples)
    CHECK(says(dyn_call_error(a, 64, ln, 2, key, 64, 0, nullptr, b, 64), "n_keys = 0"));
    CHECK(says(dyn_call_error(a, 64, ln, 2, key, 64, 1, nullptr, b, 64), "n_keys < n_rows"));
    CHECK(says(dyn_call_error(a, 64, ln, 2, key, 1ull << 59, 4, nullptr, b, 64), "2^60"));
    CHECK(says(dyn_call_error(a, 64, ln, 2, b + 4 * 127, 64, 2, nullptr, b, 64), "overlaps key_dev"));
    CHECK(says(dyn_call_error(a, 64, ln, 2, b - 4 * 640 + 4, 64, 10, ln, b, 64), "overlaps key_dev"));
    CHECK(dyn_call_error(a, 64, ln, 2, b - 4 * 640, 64, 10, ln, b, 64) == nullptr);
    CHECK(dyn_call_error(a, 64, ln, 2, b, 64, 2, nullptr, nullptr, 0) == nullptr);                       // (nothing written: nothing to overlap)

    // streams: the open's host arrays are read to exactly n_rows
    for (uint32_t R : {1u, 5u, 70u}) {
        std::unique_ptr<uint32_t[]> curve(new uint32_t[R]), kr(new uint32_t[R]);
        for (uint32_t u = 0; u < R; ++u) curve[u] = u % 3, kr[u] = u % 2;
        CHECK(dyn_stream_open_error(curve.get(), R, 3, 0, nullptr) == nullptr && dyn_stream_open_error(nullptr, R, 1, 0, kr.get()) == nullptr);
        CHECK(dyn_stream_open_error(curve.get(), R, 3, 2, kr.get()) == nullptr && dyn_stream_open_error(curve.get(), R, 3, R, nullptr) == nullptr);
        CHECK(R < 3 || says(dyn_stream_open_error(curve.get(), R, 2, 0, nullptr), "curve index"));
        CHECK(R < 2 || says(dyn_stream_open_error(curve.get(), R, 3, 1, kr.get()), "key index"));
        CHECK(R < 2 || says(dyn_stream_open_error(curve.get(), R, 3, R - 1, nullptr), "n_keys < n_rows"));
        curve[R - 1] = 3;
        CHECK(says(dyn_stream_open_error(curve.get(), R, 3, 0, nullptr), "curve index"));
        curve[R - 1] = 0, kr[R - 1] = 0xFFFFFFFFu;
        CHECK(says(dyn_stream_open_error(curve.get(), R, 3, 2, kr.get()), "key index"));
    }
    CHECK(says(dyn_stream_open_error(nullptr, 0, 1, 0, nullptr), "n_rows is 0"));
    CHECK(dyn_stream_next_error(a, 64, ln, 2, false, 0, nullptr, 0, b, 64) == nullptr && dyn_stream_next_error(a, 64, ln, 2, true, 2, key, 64, b, 80) == nullptr);
    CHECK(dyn_stream_next_error(nullptr, 0, ln, 2, true, 2, nullptr, 0, nullptr, 0) == nullptr);       // (a call of no samples)
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, false, 0, nullptr, 0, b, 63), "out_stride < in_stride"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, true, 2, nullptr, 64, b, 64), "needs key_dev"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, false, 0, key, 64, b, 64), "takes no key_dev"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, true, 2, key, 63, b, 64), "key_stride < in_stride"));
    CHECK(says(dyn_stream_next_error(a, 64, nullptr, 2, false, 0, nullptr, 0, b, 64), "NULL buffer"));
    CHECK(says(dyn_stream_next_error(nullptr, 64, ln, 2, false, 0, nullptr, 0, b, 64), "NULL buffer"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, false, 0, nullptr, 0, nullptr, 64), "NULL buffer"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, false, 0, nullptr, 0, a + 4 * 127, 64), "overlaps in_dev"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, true, 2, b + 4 * 127, 64, b, 64), "overlaps key_dev"));
    CHECK(says(dyn_stream_next_error(a, 64, ln, 2, true, 4, key, 1ull << 59, b, 64), "2^60"));
    std::printf("sanitize dyn driver: ok\n");
    return 0;
}
