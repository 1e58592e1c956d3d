// mix_kernels.hip — rendered rows -> tracks (grail_mix_async) and tracks -> interleaved i16 frames
// (grail_pcm16_frames_async).  The contract (include/grail_hip.h, "mixing"): every track sample is the left fold, in
// ascending row order, of gain * x over the items that cover it — one v_mul_f32 and one v_add_f32 per item (the library
// is built with -ffp-contract=off), no atomics, nothing but plain vector loads and stores.  DESIGN.md §4.8.
#include "kernels.h"
#include "mix_plan.h"
#include "pcm16.h"

namespace grail {

namespace {

// One workgroup = one span of one track (mix_plan.h).  Lane `l` owns samples c0 + j * 256 + l of every pass of 256 * J
// samples, so each wave-instruction's load and store covers 64 consecutive samples whatever an item's offset.  The items
// of the span's list tile come in accumulation order; their descriptors are wave-uniform (scalar loads).  U of them are
// taken per step and all their U x J loads issued before the first add: J = 1, U = 8 (short spans, many items stacked) or
// J = 8, U = 4 (long spans) — at least 8 loads per lane in flight either way.  Within a pass everything is a 32-bit offset
// o = j * 256 + l: an item covers [a, b) of it; a lane outside that loads the item's nearest covered sample (in bounds, no
// per-lane branch around the load) and skips the add, so an uncovered -0.0 stays -0.0.
template <int J, int U, bool ACC>
__global__ __launch_bounds__(256) void mix_kernel(const float *__restrict__ rows, const mix::MixItem *__restrict__ items,
                                                  const uint32_t *__restrict__ tile_start,
                                                  const uint32_t *__restrict__ tile_items, float *__restrict__ tracks,
                                                  uint64_t track_stride, uint64_t track_len, uint64_t wg_samples,
                                                  uint32_t wgs_per_track, uint32_t wgs_per_tile, uint32_t tiles_per_track)
{
    const uint32_t t = blockIdx.x / wgs_per_track;
    const uint32_t w = blockIdx.x - t * wgs_per_track;
    const uint64_t span0 = (uint64_t)w * wg_samples;
    const uint64_t span1 = span0 + wg_samples < track_len ? span0 + wg_samples : track_len;
    const uint32_t tile = t * tiles_per_track + w / wgs_per_tile;
    const uint32_t first = tile_start[tile], last = tile_start[tile + 1];
    float *trk = tracks + (uint64_t)t * track_stride;
    const uint32_t lane = threadIdx.x;
    for (uint64_t c0 = span0; c0 < span1; c0 += 256u * J) {
        const uint32_t n_valid = (uint32_t)(span1 - c0 < 256u * J ? span1 - c0 : 256u * J);
        const uint64_t c1 = c0 + n_valid;
        float acc[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const uint32_t o = (uint32_t)j * 256u + lane;
            acc[j] = 0.0f;
            if (ACC && o < n_valid) acc[j] = trk[c0 + o];
        }
        for (uint32_t k = first; k < last; k += U) {
            float x[U][J] = {};
            float g[U];
            uint32_t a[U], len[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a[u] = 0u;
                len[u] = 0u;                            // (an empty slot covers nothing)
                g[u] = 0.0f;
                if (k + u < last) {
                    const mix::MixItem it = items[tile_items[k + u]];
                    if (it.lo < c1 && it.hi > c0) {
                        const uint32_t lo = it.lo > c0 ? (uint32_t)(it.lo - c0) : 0u;
                        const uint32_t hi = it.hi < c1 ? (uint32_t)(it.hi - c0) : n_valid;
                        a[u] = lo;
                        len[u] = hi - lo;
                        g[u] = it.gain;
                        const float *src = rows + (uint64_t)(it.base + (int64_t)(c0 + lo));   // the first covered sample
#pragma unroll
                        for (int j = 0; j < J; ++j) {
                            const int32_t d = (int32_t)((uint32_t)j * 256u + lane - lo);
                            const int32_t c = d < 0 ? 0 : (d >= (int32_t)(hi - lo) ? (int32_t)(hi - lo) - 1 : d);
                            x[u][j] = src[c];
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const uint32_t o = (uint32_t)j * 256u + lane;
                    if (o - a[u] < len[u]) acc[j] = acc[j] + g[u] * x[u][j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const uint32_t o = (uint32_t)j * 256u + lane;
            if (o < n_valid) trk[c0 + o] = acc[j];
        }
    }
}

// tracks [n_tracks][track_stride] -> frames[f * n_tracks + t] (examples/cli.rs:49, pcm16.h)
__global__ __launch_bounds__(256) void pcm16_frames_kernel(const float *__restrict__ tracks, uint64_t track_stride,
                                                           uint32_t n_tracks, uint64_t n_frames,
                                                           int16_t *__restrict__ frames)
{
    const uint64_t total = n_frames * n_tracks;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256u) {
        const uint64_t f = e / n_tracks;
        const uint32_t t = (uint32_t)(e - f * n_tracks);
        frames[e] = (int16_t)pcm16_from_f32(tracks[(uint64_t)t * track_stride + f]);
    }
}

}  // namespace

hipError_t launch_mix(const MixArgs &a, hipStream_t stream)
{
    if (a.n_workgroups == 0) return hipSuccess;
#define GRAIL_MIX_LAUNCH(J, U, ACC)                                                                                    \
    hipLaunchKernelGGL((mix_kernel<J, U, ACC>), dim3(a.n_workgroups), dim3(256), 0, stream, a.rows, a.items,          \
                       a.tile_start, a.tile_items, a.tracks, a.track_stride, a.track_len, a.wg_samples,               \
                       a.wgs_per_track, a.wgs_per_tile, a.tiles_per_track)
    if (a.samples_per_lane == 8) {
        if (a.accumulate) GRAIL_MIX_LAUNCH(8, 4, true);
        else GRAIL_MIX_LAUNCH(8, 4, false);
    } else {
        if (a.accumulate) GRAIL_MIX_LAUNCH(1, 8, true);
        else GRAIL_MIX_LAUNCH(1, 8, false);
    }
#undef GRAIL_MIX_LAUNCH
    return hipGetLastError();
}

hipError_t launch_pcm16_frames(const float *tracks, uint64_t track_stride, uint32_t n_tracks, uint64_t n_frames,
                               int16_t *frames, hipStream_t stream)
{
    const uint64_t total = n_frames * n_tracks;
    if (total == 0) return hipSuccess;
    const uint64_t groups = (total + 255u) / 256u;
    hipLaunchKernelGGL(pcm16_frames_kernel, dim3((uint32_t)(groups < 65536u ? groups : 65536u)), dim3(256), 0, stream,
                       tracks, track_stride, n_tracks, n_frames, frames);
    return hipGetLastError();
}

}  // namespace grail
