// loudness_segment_kernels.hip — the K-weighting of few long rows, parallel in time (grail_loudness_segmented_async).
// The contract (include/grail_hip.h, "levels, continued": the segmented form): hop h of a row is the serial recurrence
// started from a zero state GRAIL_LOUDNESS_WARMUP_HOPS hops before the hop's first sample, so a hop is a pure function
// of (P + 1) H samples and the parallelism is across hops: one lane per (row, hop), a wave = 64 consecutive hops of one
// row.  The staging is loudness_kernels.hip's with "row r of the tile" meaning "segment r": the segment of hop h is the
// samples [(h - P) H, (h + 1) H), and what lies before the row's first sample enters as +0.0.  No atomics, every store a
// plain vector store.  DESIGN.md §4.10, "segmented form".
#include "kernels.h"
#include "loudness_common.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

using namespace loud;

namespace {

constexpr uint32_t P = GRAIL_LOUDNESS_WARMUP_HOPS;

// One tile's loads: wave-instruction i reads steps [s0, s0 + 64) of the segments 4i .. 4i + 3 of the wave, lane l the four
// samples from step s0 + 4 (l mod 16) on of segment 4i + l / 16.  Step s of segment r is the row's sample
// t = (h0 + r - P) H + s, a signed number: t < 0 lies before the row and gives +0.0 (the load reads sample 0), t past the
// row's stride reads the row's last group (a single sample: the row's last).  Every load lies inside row[row_stride] and
// none sits behind a branch.  VEC needs H % 4 == 0 besides the base and the stride: t is then a multiple of 4 and a group
// of four lies wholly on one side of 0.
template <bool VEC>
__device__ __forceinline__ void seg_load(const float *__restrict__ row, uint64_t row_stride, int64_t t_first, uint32_t H,
                                         uint32_t s0, uint32_t lane, float (&x)[LOUD_LOADS][4])
{
    const int64_t col = t_first + (int64_t)(s0 + 4u * (lane & 15u));       // of segment 0; segment r lies r H further on
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        const int64_t t = col + (int64_t)(4u * i + (lane >> 4)) * (int64_t)H;
        if (VEC) {
            const uint64_t o = t < 0 ? 0u : ((uint64_t)t < row_stride ? (uint64_t)t : row_stride - 4u);
            const float4 v = *reinterpret_cast<const float4 *>(row + o);
            x[i][0] = t < 0 ? 0.0f : v.x;
            x[i][1] = t < 0 ? 0.0f : v.y;
            x[i][2] = t < 0 ? 0.0f : v.z;
            x[i][3] = t < 0 ? 0.0f : v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const int64_t tk = t + (int64_t)k;
                const uint64_t o = tk < 0 ? 0u : ((uint64_t)tk < row_stride ? (uint64_t)tk : row_stride - 1u);
                const float v = row[o];
                x[i][k] = tk < 0 ? 0.0f : v;
            }
        }
    }
}

// One wave = the hops h0 .. h0 + 63 of one row, lane r = hop h0 + r, block (row, w) at blockIdx.x = row * waves + w.
// Every lane walks (P + 1) H steps: P H of warm-up, then its hop; the boundary between the two is wave-uniform, so the
// tile is walked in runs that end at the tile's end or at the boundary, where acc starts again from +0.0.  Only the hop's
// own samples t < n are counted.  A hop h < P starts before the row: it is fed +0.0 until t = 0, and a zero state fed
// zeros stays zero (up to the sign of zero, which no later nonzero value and no z*z depends on), so it is the
// recurrence started at sample 0.  The lane of the first hop that is not whole counts the row's tail and stores no hop;
// a wave wholly past the row's samples returns at once (n is one number for the wave).
template <bool VEC>
__global__ __launch_bounds__(64) void loudness_segments_kernel(const float *__restrict__ rows, uint64_t row_stride,
                                                               const uint32_t *__restrict__ len, uint32_t waves, uint32_t H,
                                                               LoudCoef coef, double *__restrict__ hops, uint64_t hops_stride,
                                                               uint32_t *__restrict__ hop_bad, uint64_t lanes)
{
    __shared__ float tile[LOUD_ROWS * LOUD_PITCH];
    const uint32_t lane = threadIdx.x;
    const uint32_t u = blockIdx.x / waves;
    const uint64_t h0 = (uint64_t)(blockIdx.x % waves) * LOUD_ROWS;
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;          // (never past the row, whatever len holds)
    if (h0 * H >= n) return;                                               // (so row_stride >= 1 from here on)
    const float *row = rows + (uint64_t)u * row_stride;
    const uint64_t h = h0 + lane;
    const int64_t t_first = ((int64_t)h0 - (int64_t)P) * (int64_t)H;       // segment 0's first sample
    const int64_t t_mine = t_first + (int64_t)lane * (int64_t)H;
    const uint32_t own = P * H, steps = (P + 1u) * H;
    KState k = {0.0, 0.0, 0.0, 0.0, 0.0, 0u};
    const float *mine_lds = tile + lane * LOUD_PITCH;
    float x[LOUD_LOADS][4];
    seg_load<VEC>(row, row_stride, t_first, H, 0, lane, x);
    loud_stash(tile, lane, x);
    __syncthreads();
    for (uint32_t s0 = 0; s0 < steps; s0 += LOUD_T) {
        const bool more = s0 + LOUD_T < steps;
        if (more) seg_load<VEC>(row, row_stride, t_first, H, s0 + LOUD_T, lane, x);
        const uint32_t lim = steps - s0 < LOUD_T ? steps - s0 : LOUD_T;
        uint32_t i = 0;
        while (i < lim) {
            const bool in_hop = s0 + i >= own;
            const uint32_t left = (in_hop ? steps : own) - (s0 + i);
            const uint32_t run = left < lim - i ? left : lim - i;
            const int64_t t = t_mine + (int64_t)(s0 + i);
            uint32_t j = 0;
            for (; j + 8u <= run; j += 8u) {
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q)
                    loud_sample(mine_lds[i + j + q], in_hop && t + (int64_t)(j + q) < (int64_t)n, coef.c, k);
            }
            for (; j < run; ++j) loud_sample(mine_lds[i + j], in_hop && t + (int64_t)j < (int64_t)n, coef.c, k);
            i += run;
            if (s0 + i == own) k.acc = 0.0;
        }
        __syncthreads();                                // every lane has read the tile
        if (more) loud_stash(tile, lane, x);
        __syncthreads();
    }
    if ((h + 1u) * H <= n) hops[(uint64_t)u * hops_stride + h] = k.acc;
    if (hop_bad && h < lanes) hop_bad[(uint64_t)u * lanes + h] = k.bad;
}

// A row's non-finite count from its hops' counts, one lane per row: an integer sum, so no order to fix.  The hops that
// hold a sample t < n are exactly those of the waves that did not return early.
__global__ __launch_bounds__(256) void loudness_counts_kernel(const uint32_t *__restrict__ len, uint64_t row_stride,
                                                              uint32_t n_rows, uint32_t H, const uint32_t *__restrict__ hop_bad,
                                                              uint64_t lanes, uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;
    const uint64_t held = n / H + (n % H != 0);
    const uint32_t *b = hop_bad + u * lanes;
    uint32_t sum = 0;
    for (uint64_t h = 0; h < held; ++h) sum += b[h];
    nonfinite[u] = sum;
}

}  // namespace

uint64_t loudness_segment_lanes(uint64_t row_stride, uint32_t hop) { return row_stride / hop + (row_stride % hop != 0); }

uint64_t loudness_segment_waves(uint64_t row_stride, uint32_t hop)
{
    return (loudness_segment_lanes(row_stride, hop) + LOUD_ROWS - 1u) / LOUD_ROWS;
}

hipError_t launch_loudness_segments(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows, uint32_t hop,
                                    const double *coef, double *hops, uint64_t hops_stride, uint32_t *hop_bad,
                                    uint32_t *nonfinite, hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    const uint64_t lanes = loudness_segment_lanes(row_stride, hop);
    const uint64_t waves = loudness_segment_waves(row_stride, hop);
    // blockIdx.x = row * waves + wave (grid.y ends at 65 535 rows); a launch holds fewer than 2^32 threads
    if (waves > LOUD_SEGMENT_WAVES_MAX || (uint64_t)n_rows * waves > LOUD_SEGMENT_WAVES_MAX) return hipErrorInvalidValue;
    if (waves) {
        LoudCoef c;
        for (int i = 0; i < 10; ++i) c.c[i] = coef[i];
        const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && (row_stride & 3u) == 0 && (hop & 3u) == 0;
        const dim3 grid((uint32_t)(n_rows * waves));
        if (vec)
            hipLaunchKernelGGL(loudness_segments_kernel<true>, grid, dim3(64), 0, stream, rows, row_stride, len, (uint32_t)waves,
                               hop, c, hops, hops_stride, hop_bad, lanes);
        else
            hipLaunchKernelGGL(loudness_segments_kernel<false>, grid, dim3(64), 0, stream, rows, row_stride, len, (uint32_t)waves,
                               hop, c, hops, hops_stride, hop_bad, lanes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (nonfinite)
        hipLaunchKernelGGL(loudness_counts_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, stream, len, row_stride, n_rows,
                           hop, hop_bad, lanes, nonfinite);
    return hipGetLastError();
}

}  // namespace grail
