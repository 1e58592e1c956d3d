// mix_plan.cpp — the host side of mixing that needs no device: grail_mix_async's plan (which items each list tile of each
// track accumulates, in which order; how long a workgroup's span is) and grail_mix_place_sequential.  No HIP call, so it
// builds with g++ under AddressSanitizer and UBSan (tests/test_mix_host.py), as the launch planner does.  DESIGN.md §4.8.
#include "mix_plan.h"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "../../include/grail_hip.h"

namespace grail {
namespace mix {

namespace {

constexpr uint64_t LANES = 256;                 // threads of a mix workgroup
constexpr double MAX_WORKGROUPS = 4194304.0;    // a launch's grid (x 256 threads stays below 2^32)
constexpr uint64_t MAX_ENTRIES = 1ull << 26;    // (item, list tile) pairs: 256 MB of indices at most

uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// the items in accumulation order: ascending row, ties in the order given
std::vector<uint32_t> accumulation_order(const uint32_t *item_rows, uint32_t n_items)
{
    std::vector<uint32_t> order(n_items);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [item_rows](uint32_t a, uint32_t b) { return item_rows[a] < item_rows[b]; });
    return order;
}

}  // namespace

int build_plan(const uint32_t *row_len, uint32_t n_rows, uint64_t row_stride, const uint32_t *item_rows,
               const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_gains, uint32_t n_items,
               uint32_t n_tracks, uint64_t track_len, uint64_t track_stride, uint32_t compute_units, Plan &plan,
               std::string *why)
{
    auto bad = [why](const char *msg) {
        if (why) *why = msg;
        return (int)GRAIL_ERR_INVALID_ARG;
    };
    if (n_items && (!item_rows || !item_offsets)) return bad("item_rows or item_offsets is NULL");
    if (n_rows && !row_len) return bad("row_len is NULL");
    if (track_len > track_stride) return bad("track_len > track_stride");
    if (track_len && (double)n_tracks > MAX_WORKGROUPS) return bad("more than 4 194 304 tracks");
    for (uint32_t r = 0; r < n_rows; ++r)
        if (row_len[r] > row_stride) return bad("a row_len exceeds row_stride");
    for (uint32_t i = 0; i < n_items; ++i) {
        if (item_rows[i] >= n_rows) return bad("an item's row is >= n_rows");
        if ((item_tracks ? item_tracks[i] : 0u) >= n_tracks) return bad("an item's track is >= n_tracks");
    }
    plan.items.clear();
    plan.covered = 0;
    std::vector<uint32_t> track_of;
    for (const uint32_t i : accumulation_order(item_rows, n_items)) {
        const uint64_t off = item_offsets[i], n = row_len[item_rows[i]];
        if (n == 0 || off >= track_len) continue;                       // adds nothing
        MixItem m;
        m.base = (int64_t)((uint64_t)item_rows[i] * row_stride - off);  // (mod 2^64: base + s is the row's sample for covered s)
        m.lo = off;
        m.hi = off + std::min(n, track_len - off);
        m.gain = item_gains ? item_gains[i] : 1.0f;
        m.item = i;
        plan.items.push_back(m);
        track_of.push_back(item_tracks ? item_tracks[i] : 0u);
        plan.covered += m.hi - m.lo;
    }
    // Spans.  A long mix (at least four one-pass workgroups of 2 048 samples per compute unit) takes 8 samples per lane and
    // pass, a short one — a few tracks with thousands of items stacked on them — one, so that the grid still spreads over the
    // device: a track has only track_len lanes of parallelism.  Up to 8 passes per workgroup while that leaves about 8
    // workgroups per compute unit.
    const double S = (double)n_tracks * (double)track_len, cus = (double)std::max(compute_units, 1u);
    plan.samples_per_lane = S >= 2048.0 * 4.0 * cus ? 8u : 1u;
    const uint64_t pass = LANES * plan.samples_per_lane;
    const double passes = std::floor(S / ((double)pass * 8.0 * cus));
    plan.wg_samples = pass * (uint64_t)std::min(8.0, std::max(1.0, passes));
    while (plan.wg_samples < track_len && (double)n_tracks * (double)ceil_div(track_len, plan.wg_samples) > MAX_WORKGROUPS)
        plan.wg_samples *= 2;
    plan.wgs_per_track = track_len ? ceil_div(track_len, plan.wg_samples) : 0;
    // List tiles: up to 64 spans, a quarter of the items' mean length at most — an item sits in a few lists, and the items of
    // a list that miss a workgroup's span (skipped by a scalar test) stay few.  Longer while the lists would pass MAX_ENTRIES.
    uint64_t spans = 1;
    if (!plan.items.empty()) {
        const double mean = (double)plan.covered / (double)plan.items.size();
        while (spans < 64 && (double)(plan.wg_samples * spans * 2) * 4.0 <= mean) spans *= 2;
    }
    plan.tile_samples = plan.wg_samples * spans;
    auto entries_for = [&plan](uint64_t tile) {
        uint64_t e = 0;
        for (const MixItem &m : plan.items) e += (m.hi - 1) / tile - m.lo / tile + 1;
        return e;
    };
    while (plan.tile_samples < track_len && entries_for(plan.tile_samples) > MAX_ENTRIES) plan.tile_samples *= 2;
    plan.tiles_per_track = track_len ? ceil_div(track_len, plan.tile_samples) : 0;
    // the lists: counted, then filled in accumulation order (CSR)
    const size_t n_tiles = (size_t)n_tracks * plan.tiles_per_track;
    plan.tile_start.assign(n_tiles + 1, 0u);
    for (size_t k = 0; k < plan.items.size(); ++k) {
        const MixItem &m = plan.items[k];
        const size_t t0 = (size_t)track_of[k] * plan.tiles_per_track;
        for (uint64_t tl = m.lo / plan.tile_samples; tl <= (m.hi - 1) / plan.tile_samples; ++tl) ++plan.tile_start[t0 + tl + 1];
    }
    for (size_t k = 0; k < n_tiles; ++k) plan.tile_start[k + 1] += plan.tile_start[k];
    plan.tile_items.assign(plan.tile_start[n_tiles], 0u);
    std::vector<uint32_t> fill(plan.tile_start.begin(), plan.tile_start.end() - 1);
    for (size_t k = 0; k < plan.items.size(); ++k) {
        const MixItem &m = plan.items[k];
        const size_t t0 = (size_t)track_of[k] * plan.tiles_per_track;
        for (uint64_t tl = m.lo / plan.tile_samples; tl <= (m.hi - 1) / plan.tile_samples; ++tl)
            plan.tile_items[fill[t0 + tl]++] = (uint32_t)k;
    }
    return GRAIL_OK;
}

}  // namespace mix
}  // namespace grail

extern "C" {

int grail_mix_place_sequential(const uint32_t *row_len, uint32_t n_rows, const uint32_t *item_rows,
                               const uint32_t *item_tracks, const int64_t *gaps, uint32_t n_items,
                               uint32_t n_tracks, uint64_t *item_offsets, uint64_t *track_len)
{
    if (n_tracks && !track_len) return GRAIL_ERR_INVALID_ARG;
    if (n_items && (!row_len || !item_rows || !item_offsets)) return GRAIL_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_rows[i] >= n_rows || (item_tracks ? item_tracks[i] : 0u) >= n_tracks) return GRAIL_ERR_INVALID_ARG;
    std::vector<uint64_t> cursor(n_tracks, 0), furthest(n_tracks, 0), offs(n_items, 0);
    for (const uint32_t i : grail::mix::accumulation_order(item_rows, n_items)) {
        const uint32_t t = item_tracks ? item_tracks[i] : 0u;
        const int64_t g = gaps ? gaps[i] : 0;
        const uint64_t mag = g < 0 ? 0ull - (uint64_t)g : (uint64_t)g;
        if (g < 0 && mag > cursor[t]) return GRAIL_ERR_INVALID_ARG;          // a start below 0
        if (g >= 0 && mag > UINT64_MAX - cursor[t] - row_len[item_rows[i]]) return GRAIL_ERR_INVALID_ARG;
        const uint64_t start = g < 0 ? cursor[t] - mag : cursor[t] + mag;
        offs[i] = start;
        cursor[t] = start + row_len[item_rows[i]];
        furthest[t] = std::max(furthest[t], cursor[t]);
    }
    for (uint32_t i = 0; i < n_items; ++i) item_offsets[i] = offs[i];
    for (uint32_t t = 0; t < n_tracks; ++t) track_len[t] = furthest[t];
    return GRAIL_OK;
}

}  // extern "C"
