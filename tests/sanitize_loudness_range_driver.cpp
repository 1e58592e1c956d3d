// sanitize_loudness_range_driver.cpp — drives grail_loudness_window_max and grail_loudness_range (csrc/level_gains.cpp)
// under AddressSanitizer + UBSan (tests/test_loudness_segmented_host.py): arrays of exactly n_hops entries (an overread is
// ASan's to find) around every length at which the functions take another path — fewer hops than a window, exactly one
// block, many —, with rows that are loud, under the absolute gate, loud and quiet in stretches, or zero but for one hop.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/grail_hip.h"

static int failures = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);         \
            ++failures;                                                     \
            return;                                                         \
        }                                                                   \
    } while (0)

static void meter_case(std::mt19937 &rng, uint32_t n_hops, uint32_t hop, int kind)
{
    std::vector<double> h(n_hops);          // exactly n_hops entries
    std::uniform_real_distribution<double> u(0.0, 1.0);
    double largest = 0.0;
    for (uint32_t i = 0; i < n_hops; ++i) {
        double ms = 0.0;
        if (kind == 0) ms = 0.1 + u(rng);                                       // all loud, within 20 LU of each other
        else if (kind == 1) ms = GRAIL_LOUDNESS_ABS_GATE * 0.9 * u(rng);        // all under the absolute gate
        else if (kind == 2) ms = u(rng) < 0.5 ? u(rng) : 1e-9 * u(rng);         // loud and quiet stretches
        else ms = i + 1 == n_hops ? 1.0 : 0.0;                                  // zero but for the last hop
        h[i] = ms * hop;
        largest = std::max(largest, ms);
    }
    for (const uint32_t window : {0u, 1u, 4u, 30u, n_hops, n_hops + 1u}) {
        const double m = grail_loudness_window_max(h.data(), n_hops, hop, window);
        CHECK(std::isfinite(m) && m >= 0.0);
        if (window == 0 || window > n_hops) CHECK(m == 0.0);
        else CHECK(m <= largest * (1.0 + 1e-12));
        if (window == 1 && n_hops) CHECK(m == largest * hop / ((double)hop) || std::fabs(m - largest) <= 1e-12 * largest);
        CHECK(grail_loudness_window_max(h.data(), n_hops, 0, window) == 0.0);
    }
    if (kind == 3 && n_hops >= 30) CHECK(grail_loudness_window_max(h.data(), n_hops, hop, 30) == 1.0 * hop / (30.0 * hop));
    const double lra = grail_loudness_range(h.data(), n_hops, hop);
    CHECK(std::isfinite(lra) && lra >= 0.0);
    if (n_hops <= 30 || kind == 1 || kind == 3) CHECK(lra == 0.0);     // no block, one block, or every kept block the same
    if (kind == 0) CHECK(lra <= 10.0 * std::log10(1.1 / 0.1) + 1e-9);
    CHECK(lra <= 20.0 + 10.0 * std::log10(30.0) + 1e-9);               // nothing kept lies 20 LU below the mean of the kept
    CHECK(grail_loudness_range(h.data(), n_hops, 0) == 0.0);
}

int main()
{
    std::mt19937 rng(20240921u);
    for (const uint32_t n : {0u, 1u, 3u, 4u, 5u, 29u, 30u, 31u, 32u, 59u, 60u, 61u, 400u})
        for (int kind = 0; kind < 4; ++kind) meter_case(rng, n, 4800u, kind);
    for (int k = 0; k < 300; ++k) meter_case(rng, rng() % 300u, 256u + rng() % 20000u, k % 4);
    if (grail_loudness_window_max(nullptr, 40, 4800, 4) != 0.0 || grail_loudness_range(nullptr, 40, 4800) != 0.0) ++failures;
    if (failures) {
        std::printf("sanitize loudness range driver: %d failures\n", failures);
        return 1;
    }
    std::printf("sanitize loudness range driver: ok\n");
    return 0;
}
