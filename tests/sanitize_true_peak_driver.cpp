// Drives the pure-host true-peak functions of csrc/level_gains.cpp under AddressSanitizer and UBSan
// (tests/test_true_peak_host.py builds and runs it): every array lives on the heap at exactly the documented size, so
// that a read or write one element past it is caught.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "../include/grail_hip.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "sanitize true peak driver: %s failed (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    {       // the table: exactly 48 doubles
        std::unique_ptr<double[]> coef(new double[GRAIL_TRUE_PEAK_PHASES * GRAIL_TRUE_PEAK_TAPS]);
        CHECK(grail_true_peak_coefficients(coef.get()) == GRAIL_OK);
        CHECK(coef[6] == 7964.0 / 8192.0 && coef[12] == -239.0 / 8192.0 && coef[47] == 14.0 / 8192.0);
        for (int k = 0; k < 12; ++k) CHECK(coef[24 + k] == coef[12 + 11 - k] && coef[36 + k] == coef[11 - k]);
        CHECK(grail_true_peak_coefficients(nullptr) == GRAIL_ERR_INVALID_ARG);
    }
    CHECK(grail_true_peak_db(1.0) == 0.0 && grail_true_peak_db(0.0) == -HUGE_VAL && std::isnan(grail_true_peak_db(NAN)) &&
          std::isnan(grail_true_peak_db(-1.0)));
    CHECK(std::isfinite(grail_true_peak_db(5e-324)) && std::isfinite(grail_true_peak_db(1e308)));
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    const auto next = [&]() {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return seed;
    };
    for (uint32_t n_rows : {0u, 1u, 7u, 300u}) {
        for (uint32_t n_items : {0u, 1u, 64u, 1000u}) {
            if (n_rows == 0 && n_items) continue;
            std::unique_ptr<double[]> tp(new double[n_rows]);
            std::unique_ptr<uint32_t[]> rows(new uint32_t[n_items]);
            std::unique_ptr<float[]> gains(new float[n_items]), before(new float[n_items]);
            for (uint32_t r = 0; r < n_rows; ++r) {
                const uint64_t v = next();
                // zeros, denormals, audio-sized values, the largest a row of FLT_MAX samples can read
                tp[r] = v % 7 == 0 ? 0.0 : v % 7 == 1 ? 5e-324 : v % 7 == 2 ? 2.02 * 3.4028234663852886e38 : (double)(v % 100000) / 50000.0;
            }
            for (uint32_t i = 0; i < n_items; ++i) {
                const uint64_t v = next();
                rows[i] = (uint32_t)(v % n_rows);
                gains[i] = v % 11 == 0 ? 3.4028234663852886e38f : v % 11 == 1 ? -1e-45f : v % 11 == 2 ? 0.0f
                           : v % 11 == 3 ? std::numeric_limits<float>::infinity() : v % 11 == 4 ? NAN
                           : ((v >> 8) % 2 ? -1.0f : 1.0f) * (float)((v >> 16) % 1000) / 100.0f;
                before[i] = gains[i];
            }
            for (float ceiling : {-1.0f, 0.0f, 200.0f, -200.0f, 770.0f, -770.0f}) {
                for (uint32_t i = 0; i < n_items; ++i) gains[i] = before[i];
                uint32_t limited = 0xFFFFFFFFu;
                CHECK(grail_true_peak_limit_gains(tp.get(), n_rows, rows.get(), n_items, ceiling, gains.get(), &limited) == GRAIL_OK);
                CHECK(limited <= n_items);
                const double c = std::pow(10.0, (double)ceiling / 20.0);
                for (uint32_t i = 0; i < n_items; ++i) {
                    const double t = tp[rows[i]];
                    if (t > 0.0 && !std::isnan(gains[i])) CHECK((double)std::fabs(gains[i]) * t <= c);
                    CHECK(std::isnan(gains[i]) == std::isnan(before[i]) && (std::isnan(gains[i]) || std::signbit(gains[i]) == std::signbit(before[i])));
                    if (!(t > 0.0)) CHECK(std::isnan(before[i]) || gains[i] == before[i]);
                }
                CHECK(grail_true_peak_limit_gains(tp.get(), n_rows, rows.get(), n_items, ceiling, gains.get(), nullptr) == GRAIL_OK);
            }
            if (n_items) {
                rows[n_items - 1] = n_rows;         // one past the rows: refused before anything is written
                uint32_t limited = 77;
                CHECK(grail_true_peak_limit_gains(tp.get(), n_rows, rows.get(), n_items, 0.0f, gains.get(), &limited) == GRAIL_ERR_INVALID_ARG);
                CHECK(limited == 77);
                rows[n_items - 1] = 0;
                CHECK(grail_true_peak_limit_gains(tp.get(), n_rows, rows.get(), n_items, NAN, gains.get(), &limited) == GRAIL_ERR_INVALID_ARG);
                CHECK(grail_true_peak_limit_gains(nullptr, n_rows, rows.get(), n_items, 0.0f, gains.get(), &limited) == GRAIL_ERR_INVALID_ARG);
                CHECK(limited == 77);
            }
        }
    }
    std::printf("sanitize true peak driver: ok\n");
    return 0;
}
