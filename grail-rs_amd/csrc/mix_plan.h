// mix_plan.h — the host plan of a mix (grail_mix_async; internal).  No HIP: mix_plan.cpp builds with g++ under the
// sanitizers (tests/test_mix_host.py), the kernel unit (mix_kernels.hip) reads MixItem as laid out here.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace grail {
namespace mix {

// One item as the kernel reads it: 32 B, one scalar load per item (the descriptors are wave-uniform).
struct MixItem {
    int64_t base;     // track sample s reads rows[base + s] (mod 2^64): row * row_stride - offset
    uint64_t lo, hi;  // the track samples the item covers, [lo, hi): lo < hi <= track_len
    float gain;
    uint32_t item;    // the caller's index of the item
};
static_assert(sizeof(MixItem) == 32, "MixItem is one 32-byte scalar load");

// The work of one mix.  Every track is cut into WORKGROUP SPANS of wg_samples (one 256-thread workgroup each; a lane owns
// samples span0 + p * 256 * J + j * 256 + lane, J = samples_per_lane, p = the pass) and into LIST TILES of tile_samples (a
// multiple of wg_samples): tile_items[tile_start[k] .. tile_start[k + 1]) are the items that intersect list tile k
// (k = track * tiles_per_track + tile of the track), in accumulation order, as indices into `items`.
struct Plan {
    uint32_t samples_per_lane = 1;   // J: 1 (short spans: thousands of items stacked on few tracks) or 8 (long spans)
    uint64_t wg_samples = 256;       // a multiple of 256 * J
    uint64_t tile_samples = 256;     // a multiple of wg_samples
    uint64_t wgs_per_track = 0;      // ceil(track_len / wg_samples)
    uint64_t tiles_per_track = 0;    // ceil(track_len / tile_samples)
    std::vector<MixItem> items;      // the items that cover something, stable-sorted by row (= accumulation order)
    std::vector<uint32_t> tile_start;   // [n_tracks * tiles_per_track + 1]
    std::vector<uint32_t> tile_items;
    uint64_t covered = 0;            // samples the items cover (each read once)
};

// Checks the items (rows < n_rows, tracks < n_tracks, track_len <= track_stride, every row_len <= row_stride) and lays
// out the plan.  GRAIL_OK or GRAIL_ERR_INVALID_ARG with the reason in *why.  compute_units: what the launch policy plans
// for (the spans spread a mix over about 8 workgroups per compute unit where the tracks are long enough).
int build_plan(const uint32_t *row_len, uint32_t n_rows, uint64_t row_stride, const uint32_t *item_rows,
               const uint32_t *item_tracks, const uint64_t *item_offsets, const float *item_gains, uint32_t n_items,
               uint32_t n_tracks, uint64_t track_len, uint64_t track_stride, uint32_t compute_units, Plan &plan,
               std::string *why);

}  // namespace mix
}  // namespace grail
