// Drives the pure-host IIR functions of csrc/iir_plan.cpp under AddressSanitizer and UBSan (tests/test_iir_sanitize.py
// builds and runs it): every array lives on the heap at exactly the size the call is entitled to, so that a read or write
// one element past it is caught.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../include/grail_hip.h"
#include "../grail-rs_amd/csrc/iir_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize iir driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // designs into exactly five doubles: finite, and a1, a2 those of a stable pole pair (|a2| < 1, |a1| < 1 + a2)
    for (int kind = GRAIL_IIR_LOWPASS; kind <= GRAIL_IIR_HIGHSHELF; ++kind)
        for (uint32_t rate : {8000u, 44100u, 48000u, 192000u})
            for (double f0 : {20.0, 1000.0, 3999.0})
                for (double q : {0.3, 0.7071067811865476, 8.0})
                    for (double g : {-24.0, -0.0, 0.0, 12.0}) {
                        std::unique_ptr<double[]> c(new double[5]);
                        CHECK(grail_iir_design(kind, rate, f0, q, g, c.get()) == GRAIL_OK);
                        for (int k = 0; k < 5; ++k) CHECK(std::isfinite(c[k]));
                        CHECK(std::fabs(c[4]) < 1.0 && std::fabs(c[3]) < 1.0 + c[4]);
                    }
    {
        std::unique_ptr<double[]> c(new double[5]);
        for (int k = 0; k < 5; ++k) c[k] = 77.0;
        for (int kind : {-1, 7, 1 << 30, -(1 << 30)}) CHECK(grail_iir_design(kind, 48000, 1000.0, 1.0, 0.0, c.get()) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_iir_design(GRAIL_IIR_PEAK, 0, 1000.0, 1.0, 0.0, c.get()) == GRAIL_ERR_INVALID_ARG);
        for (double f0 : {0.0, -0.0, -1.0, 24000.0, 24000.5, 1e300, nan, inf, -inf})
            CHECK(grail_iir_design(GRAIL_IIR_PEAK, 48000, f0, 1.0, 0.0, c.get()) == GRAIL_ERR_INVALID_ARG);
        for (double q : {0.0, -0.0, -1.0, nan, inf, -inf}) CHECK(grail_iir_design(GRAIL_IIR_PEAK, 48000, 1000.0, q, 0.0, c.get()) == GRAIL_ERR_INVALID_ARG);
        for (double g : {nan, inf, -inf}) CHECK(grail_iir_design(GRAIL_IIR_LOWPASS, 48000, 1000.0, 1.0, g, c.get()) == GRAIL_ERR_INVALID_ARG);
        CHECK(grail_iir_design(GRAIL_IIR_HIGHSHELF, 48000, 1000.0, 1.0, 1e5, c.get()) == GRAIL_ERR_INVALID_ARG);     // 10^5000
        CHECK(grail_iir_design(GRAIL_IIR_PEAK, 48000, 1000.0, 1.0, 0.0, nullptr) == GRAIL_ERR_INVALID_ARG);
        for (int k = 0; k < 5; ++k) CHECK(c[k] == 77.0);
    }

    // set images: every filter's sections at a pitch of 40 doubles, +0.0 past its own; S = 1, 7, 8 and F = 1, 64
    for (uint32_t F : {1u, 3u, 64u}) {
        std::unique_ptr<uint32_t[]> S(new uint32_t[F]);
        uint32_t total = 0, most = 0;
        for (uint32_t f = 0; f < F; ++f) {
            S[f] = F == 1 ? 1u : (f % 3 == 0 ? 1u : f % 3 == 1 ? 7u : 8u);
            total += 5 * S[f];
            most = S[f] > most ? S[f] : most;
        }
        std::unique_ptr<double[]> coef(new double[total]);
        for (uint32_t i = 0; i < total; ++i) coef[i] = (double)(i % 17) - 8.25;
        CHECK(grail::iir_set_error(coef.get(), S.get(), F) == nullptr);
        std::vector<double> image;
        std::vector<uint32_t> sections;
        uint32_t bound = 77;
        grail::iir_set_image(coef.get(), S.get(), F, image, sections, &bound);
        CHECK(image.size() == (size_t)F * grail::IIR_IMAGE_DOUBLES && sections.size() == F && bound == (most == 1 ? 1u : 8u));
        size_t from = 0;
        for (uint32_t f = 0; f < F; ++f) {
            CHECK(sections[f] == S[f]);
            for (uint32_t k = 0; k < grail::IIR_IMAGE_DOUBLES; ++k) {
                const double got = image[(size_t)f * grail::IIR_IMAGE_DOUBLES + k];
                CHECK(k < 5 * S[f] ? got == coef[from + k] : (got == 0.0 && !std::signbit(got)));
            }
            from += 5 * S[f];
        }
        // a coefficient that is not finite: the set's last, and (not looked at: the array ends there) none past it
        coef[total - 1] = inf;
        CHECK(grail::iir_set_error(coef.get(), S.get(), F) != nullptr);
        coef[total - 1] = 1.0, coef[0] = nan;
        CHECK(grail::iir_set_error(coef.get(), S.get(), F) != nullptr);
        coef[0] = 1.0;
        CHECK(grail::iir_set_error(coef.get(), S.get(), F) == nullptr);
    }
    for (uint32_t most : {1u, 2u, 3u, 4u, 5u, 8u}) {     // the bound: the largest S rounded up to 1, 2, 4, 8
        std::unique_ptr<uint32_t[]> S(new uint32_t[2]);
        S[0] = 1, S[1] = most;
        std::unique_ptr<double[]> coef(new double[5 * (1 + most)]);
        for (uint32_t i = 0; i < 5 * (1 + most); ++i) coef[i] = 0.5;
        std::vector<double> image;
        std::vector<uint32_t> sections;
        uint32_t bound = 77;
        grail::iir_set_image(coef.get(), S.get(), 2, image, sections, &bound);
        CHECK(bound == (most <= 2 ? most : most <= 4 ? 4u : 8u));
    }
    {   // every refused set
        std::unique_ptr<double[]> coef(new double[5 * 8 * 65]);
        std::unique_ptr<uint32_t[]> S(new uint32_t[65]);
        for (uint32_t i = 0; i < 5 * 8 * 65; ++i) coef[i] = 0.25;
        for (uint32_t f = 0; f < 65; ++f) S[f] = 8;
        CHECK(grail::iir_set_error(coef.get(), S.get(), 64) == nullptr);
        CHECK(grail::iir_set_error(coef.get(), S.get(), 65) != nullptr && grail::iir_set_error(coef.get(), S.get(), 0) != nullptr);
        CHECK(grail::iir_set_error(nullptr, S.get(), 1) != nullptr && grail::iir_set_error(coef.get(), nullptr, 1) != nullptr);
        for (uint32_t bad : {0u, 9u, 0xFFFFFFFFu}) {
            S[1] = bad;
            CHECK(grail::iir_set_error(coef.get(), S.get(), 2) != nullptr && grail::iir_set_error(coef.get(), S.get(), 1) == nullptr);
        }
    }

    // lengths
    CHECK(grail::iir_len(0, 9, 100) == 0 && grail::iir_len(10, 9, 100) == 19 && grail::iir_len(10, 9, 15) == 15 && grail::iir_len(10, 9, 0) == 0);
    CHECK(grail::iir_len(UINT64_MAX, 0xFFFFFFFFu, UINT64_MAX) == UINT64_MAX && grail::iir_len(1, 0, 7) == 1);
    uint64_t n_out = 77;
    CHECK(grail_iir_stream_len(0, 0, 5, 0, &n_out) == GRAIL_OK && n_out == 0);
    CHECK(grail_iir_stream_len(7, 100, 5, 0, &n_out) == GRAIL_OK && n_out == 100);
    CHECK(grail_iir_stream_len(7, 0, 5, 1, &n_out) == GRAIL_OK && n_out == 5);
    CHECK(grail_iir_stream_len(0, 0, 5, 1, &n_out) == GRAIL_OK && n_out == 0);
    CHECK(grail_iir_stream_len((1ull << 63) - 2, 1, 0xFFFFFFFFu, 0, &n_out) == GRAIL_OK && n_out == 1);
    n_out = 77;
    CHECK(grail_iir_stream_len((1ull << 63) - 1, 1, 5, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_iir_stream_len(1ull << 63, 0, 5, 0, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_iir_stream_len(0, UINT64_MAX, 5, 0, &n_out) == GRAIL_ERR_INVALID_ARG && grail_iir_stream_len(3, 1, 5, 1, &n_out) == GRAIL_ERR_INVALID_ARG);
    CHECK(grail_iir_stream_len(3, 1, 5, 0, nullptr) == GRAIL_ERR_INVALID_ARG && n_out == 77);

    // the checks of the calls on streams (addresses are compared, never looked behind)
    {
        std::unique_ptr<uint32_t[]> which(new uint32_t[4]);
        for (uint32_t u = 0; u < 4; ++u) which[u] = u;
        CHECK(grail::iir_stream_open_error(which.get(), 4, 4) == nullptr && grail::iir_stream_open_error(nullptr, 4, 1) == nullptr);
        CHECK(grail::iir_stream_open_error(which.get(), 4, 3) != nullptr && grail::iir_stream_open_error(which.get(), 0, 4) != nullptr);
        const void *a = (const void *)0x10000000, *b = (const void *)0x20000000, *len = (const void *)0x30000000;
        CHECK(grail::iir_stream_next_error(a, 64, len, 4, b, 64) == nullptr && grail::iir_stream_next_error(nullptr, 0, len, 4, nullptr, 0) == nullptr);
        CHECK(grail::iir_stream_next_error(a, 64, len, 4, b, 63) != nullptr && grail::iir_stream_next_error(a, 64, nullptr, 4, b, 64) != nullptr);
        CHECK(grail::iir_stream_next_error(nullptr, 64, len, 4, b, 64) != nullptr && grail::iir_stream_next_error(a, 64, len, 4, nullptr, 64) != nullptr);
        CHECK(grail::iir_stream_next_error(a, 64, len, 4, (const char *)a + 4 * 255, 64) != nullptr);
        CHECK(grail::iir_stream_next_error(a, 64, len, 4, (const char *)a + 4 * 256, 64) == nullptr);
        CHECK(grail::iir_stream_next_error(a, 1ull << 59, len, 4, b, 1ull << 59) != nullptr);
        CHECK(grail::iir_stream_finish_error(b, 64, 4, 64) == nullptr && grail::iir_stream_finish_error(b, 63, 4, 64) != nullptr);
        CHECK(grail::iir_stream_finish_error(nullptr, 64, 4, 1) != nullptr && grail::iir_stream_finish_error(nullptr, 0, 4, 0) == nullptr);
        CHECK(grail::iir_stream_finish_error(b, 1ull << 59, 4, 1) != nullptr);
    }
    std::printf("sanitize iir driver: ok\n");
    return 0;
}
