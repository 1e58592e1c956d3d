// sanitize_loudness_driver.cpp — drives the loudness half of csrc/level_gains.cpp under AddressSanitizer + UBSan
// (tests/test_loudness_host.py): grail_kweighting over the whole range of rates and outside it, grail_gated_mean_square
// over arrays of exactly n_hops entries (an overread is ASan's to find) with every kind of row — too short, under the
// absolute gate, one block over it, loud and quiet stretches —, the two formulas, and grail_level_gains in
// GRAIL_LEVEL_LOUDNESS with only the arrays that mode needs.
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

static void kweighting_case(uint32_t rate)
{
    double coef[10];
    for (double &c : coef) c = -77.0;
    const int rc = grail_kweighting(rate, coef);
    if (rate < GRAIL_LOUDNESS_RATE_MIN || rate > GRAIL_LOUDNESS_RATE_MAX) {
        CHECK(rc == GRAIL_ERR_INVALID_ARG);
        for (const double c : coef) CHECK(c == -77.0);
        return;
    }
    CHECK(rc == GRAIL_OK);
    for (const double c : coef) CHECK(std::isfinite(c));
    CHECK(coef[5] == 1.0 && coef[6] == -2.0 && coef[7] == 1.0);
    // (below 2 x 1682 Hz the shelf's corner lies above half the rate: ten finite numbers, but no K-weighting)
    if (rate < 4000u) return;
    // both sections are stable: |a2| < 1 and |a1| < 1 + a2
    CHECK(std::fabs(coef[4]) < 1.0 && std::fabs(coef[3]) < 1.0 + coef[4]);
    CHECK(std::fabs(coef[9]) < 1.0 && std::fabs(coef[8]) < 1.0 + coef[9]);
    // the shelf passes DC unchanged and lifts the top by 4 dB: gains (b0+b1+b2)/(1+a1+a2) and (b0-b1+b2)/(1-a1+a2)
    CHECK(std::fabs((coef[0] + coef[1] + coef[2]) / (1.0 + coef[3] + coef[4]) - 1.0) < 1e-6);
    CHECK(std::fabs(20.0 * std::log10((coef[0] - coef[1] + coef[2]) / (1.0 - coef[3] + coef[4])) - 3.999843853973347) < 1e-6);
}

static void gate_case(std::mt19937 &rng, uint32_t n_hops, uint32_t hop, int kind)
{
    std::vector<double> h(n_hops);          // exactly n_hops entries
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double per = 4.0 * hop;
    double largest = 0.0;
    for (uint32_t i = 0; i < n_hops; ++i) {
        double ms = 0.0;
        if (kind == 0) ms = u(rng);                                             // all loud
        else if (kind == 1) ms = GRAIL_LOUDNESS_ABS_GATE * 0.9 * u(rng);        // all under the absolute gate
        else if (kind == 2) ms = u(rng) < 0.5 ? u(rng) : 1e-9 * u(rng);         // loud and quiet stretches
        else ms = i + 1 == n_hops ? 1.0 : 0.0;                                  // one block over the gate
        h[i] = ms * hop;
        if (ms > largest) largest = ms;
    }
    const double g = grail_gated_mean_square(h.data(), n_hops, hop);
    CHECK(std::isfinite(g) && g >= 0.0);
    if (n_hops < 4 || kind == 1) CHECK(g == 0.0);
    else {
        CHECK(g <= largest * (1.0 + 1e-12));
        if (kind == 0) CHECK(g > GRAIL_LOUDNESS_ABS_GATE);
        if (kind == 3) CHECK(g == (((0.0 + 0.0) + 0.0) + 1.0 * hop) / per);
    }
    CHECK(grail_gated_mean_square(h.data(), n_hops, 0) == 0.0);
}

static void gains_case(std::mt19937 &rng, uint32_t n_rows, uint32_t n_items)
{
    std::uniform_real_distribution<double> ms(1e-7, 1.0);
    std::uniform_real_distribution<float> lufs(-40.0f, -10.0f);
    std::vector<double> level(n_rows);
    std::vector<uint32_t> bad(n_rows, 0u);
    for (uint32_t r = 0; r < n_rows; ++r) level[r] = grail_loudness_level(ms(rng));
    if (n_rows >= 2) {
        level[0] = grail_loudness_level(0.0);       // a row shorter than 400 ms
        bad[1] = 1;
    }
    std::vector<uint32_t> rows(n_items);
    std::vector<float> target(n_items), g(n_items, -1.0f);
    uint32_t expect_out = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        rows[i] = rng() % n_rows;
        target[i] = lufs(rng);
        if (n_rows >= 2 && rows[i] < 2) ++expect_out;
    }
    uint32_t out = 0xFFFFFFFFu;
    CHECK(grail_level_gains(GRAIL_LEVEL_LOUDNESS, nullptr, nullptr, bad.data(), nullptr, level.data(), n_rows, rows.data(),
                            target.data(), n_items, g.data(), &out) == GRAIL_OK);
    CHECK(out == expect_out);
    for (uint32_t i = 0; i < n_items; ++i) {
        if (n_rows >= 2 && rows[i] < 2) CHECK(g[i] == 0.0f);
        else CHECK(g[i] == (float)(std::pow(10.0, (double)target[i] / 20.0) / level[rows[i]]));
    }
    if (n_items) {      // the mode's array missing: refused, nothing written
        std::vector<float> keep(n_items, -1.0f);
        CHECK(grail_level_gains(GRAIL_LEVEL_LOUDNESS, nullptr, nullptr, bad.data(), nullptr, nullptr, n_rows, rows.data(),
                                target.data(), n_items, keep.data(), &out) == GRAIL_ERR_INVALID_ARG);
        for (const float v : keep) CHECK(v == -1.0f);
    }
}

int main()
{
    std::mt19937 rng(20240913u);
    for (const uint32_t rate : {0u, 1u, 2559u, 2560u, 8000u, 16000u, 22050u, 44100u, 48000u, 96000u, 192000u, 1048576u,
                                1048577u, 0xFFFFFFFFu})
        kweighting_case(rate);
    for (int k = 0; k < 300; ++k) kweighting_case(2560u + rng() % (1048576u - 2560u));
    for (int k = 0; k < 400; ++k) gate_case(rng, rng() % 200u, 256u + rng() % 20000u, k % 4);
    for (const uint32_t n : {0u, 1u, 3u, 4u, 5u})
        for (int kind = 0; kind < 4; ++kind) gate_case(rng, n, 4800u, kind);
    if (grail_gated_mean_square(nullptr, 10, 4800) != 0.0) ++failures;
    for (int k = 0; k < 100; ++k) gains_case(rng, 1u + rng() % 50u, rng() % 200u);
    gains_case(rng, 2, 0);
    if (grail_loudness_lufs(0.0) != -HUGE_VAL || grail_loudness_level(0.0) != 0.0) ++failures;
    if (std::fabs(grail_loudness_lufs(GRAIL_LOUDNESS_ABS_GATE) + 70.0) > 1e-9) ++failures;
    if (std::fabs(20.0 * std::log10(grail_loudness_level(0.01)) - grail_loudness_lufs(0.01)) > 1e-9) ++failures;
    if (failures) {
        std::printf("sanitize loudness driver: %d failures\n", failures);
        return 1;
    }
    std::printf("sanitize loudness driver: ok\n");
    return 0;
}
