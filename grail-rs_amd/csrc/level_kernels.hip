// level_kernels.hip — how loud rendered rows are, measured where they lie (grail_levels_async,
// grail_frame_levels_async).  The contract (include/grail_hip.h, "levels"): per frame of F samples the largest finite
// |x|, the count of non-finite samples, and a binary64 sum of squares over 256 partials p[t mod 256] folded in ascending
// t and then halved 128, 64, ..., 1; a row's sum is the left fold of its frames' sums.  No atomics, every store a plain
// vector store: the bits depend on the samples and F alone.  DESIGN.md §4.9.
#include "kernels.h"

namespace grail {

namespace {

constexpr int LEVEL_CHUNKS = 8;     // 256-sample chunks whose loads a wave issues before the first use (8 x 16 B per lane)

// U chunks of one frame, from chunk c on: all their loads, then the fold.  A slot past the frame's last chunk reads that
// last chunk again and holds nothing (lo = hi = 0); a lane past the chunk's end reads the chunk's last covered sample:
// every load is in bounds and none sits behind a branch, so all of a step's loads are issued before the first use.
template <bool VEC, int U>
__device__ __forceinline__ void level_step(const float *__restrict__ row, uint64_t c, uint64_t c1, uint64_t start,
                                           uint64_t end, uint32_t lane, double (&p)[4], uint32_t &peak, uint32_t &bad)
{
    float x[U][4];
    uint32_t lo[U], hi[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const bool live = c + i < c1;
        const uint64_t base = (live ? c + i : c1 - 1u) << 8;
        const uint32_t top = end - base < 256u ? (uint32_t)(end - base) : 256u;     // 1 .. 256 samples of the chunk lie below end
        lo[i] = live && start > base ? (uint32_t)(start - base) : 0u;
        hi[i] = live ? top : 0u;
        const float *src = row + base;
        if (VEC) {
            // the last covered sample's group of four starts below n <= row_stride, a multiple of 4: inside the row
            const uint32_t o = 4u * lane < top ? 4u * lane : ((top - 1u) & ~3u);
            const float4 v = *reinterpret_cast<const float4 *>(src + o);
            x[i][0] = v.x;
            x[i][1] = v.y;
            x[i][2] = v.z;
            x[i][3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t o = 4u * lane + k < top ? 4u * lane + k : top - 1u;
                x[i][k] = src[o];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = __builtin_fabsf(x[i][k]);
            const bool inside = 4u * lane + k - lo[i] < hi[i] - lo[i];
            const bool finite = a <= 3.4028234663852886e38f;        // false for NaN and Inf
            bad += (inside && !finite) ? 1u : 0u;
            const float s = (inside && finite) ? a : 0.0f;
            const uint32_t sb = __float_as_uint(s);
            peak = sb > peak ? sb : peak;
            p[k] = __builtin_fma((double)s, (double)s, p[k]);
        }
    }
}

// One wave = one (row, frame).  The frame is walked in the row's aligned chunks of 256 samples (t counted from the row's
// first sample, so a frame whose F is no multiple of 256 starts and ends inside a chunk); lane l holds samples 4l .. 4l+3
// of every chunk, i.e. the four partials p[4l .. 4l+3], and one wave-instruction reads 64 x 16 B = the whole chunk.
// A sample outside [lo, hi) of its chunk, or not finite, enters as +0.0f: a partial is never negative, so adding +0.0
// leaves its bits alone (the contract's "skipped").  The square of a binary32 is exact in binary64, so the fma below is
// the contract's multiply and add.  VEC = false is the same mapping with four 4-byte loads per lane, for rows whose base
// is not 16-byte aligned.  The peak is kept as the bit pattern of |x| (finite non-negative floats order as integers).
template <bool VEC>
__global__ __launch_bounds__(256) void level_frames_kernel(const float *__restrict__ rows, uint64_t row_stride,
                                                           const uint32_t *__restrict__ len, uint32_t n_rows, uint32_t F,
                                                           uint32_t grid_frames, double *__restrict__ fsum,
                                                           float *__restrict__ fpeak, uint32_t *__restrict__ fbad,
                                                           uint64_t frames_stride)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * 4u + wave;
    const uint64_t u = w / grid_frames;
    if (u >= n_rows) return;
    const uint32_t f = (uint32_t)(w - u * grid_frames);
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;       // (never past the row, whatever len holds)
    const uint64_t start = (uint64_t)f * F;
    if (start >= n) return;                                             // frames past the row's last: nothing written
    const uint64_t end = start + F < n ? start + F : n;
    const float *row = rows + u * row_stride;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t peak = 0u, bad = 0u;
    const uint64_t c1 = (end + 255u) >> 8;
    uint64_t c = start >> 8;
    for (; c + LEVEL_CHUNKS <= c1; c += LEVEL_CHUNKS) level_step<VEC, LEVEL_CHUNKS>(row, c, c1, start, end, lane, p, peak, bad);
    // what is left (a short frame is all of it: 2 or 3 chunks at F = 480) in a step of its own size
    if (c1 - c > 4u) level_step<VEC, 8>(row, c, c1, start, end, lane, p, peak, bad);
    else if (c1 - c > 2u) level_step<VEC, 4>(row, c, c1, start, end, lane, p, peak, bad);
    else if (c1 > c) level_step<VEC, 2>(row, c, c1, start, end, lane, p, peak, bad);
    // the halving tree: w = 128 ... 4 pair lanes 32, 16, ..., 1 apart (lane 0 ends with the contract's p[0 .. 3]),
    // then w = 2 and w = 1 inside the lane
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = p[k] + __shfl_xor(p[k], d, 64);
        const uint32_t op = (uint32_t)__shfl_xor((int)peak, d, 64);
        peak = op > peak ? op : peak;
        bad += (uint32_t)__shfl_xor((int)bad, d, 64);
    }
    if (lane == 0u) {
        const double q0 = p[0] + p[2], q1 = p[1] + p[3];
        const uint64_t at = u * frames_stride + f;
        if (fsum) fsum[at] = q0 + q1;
        if (fpeak) fpeak[at] = __uint_as_float(peak);
        if (fbad) fbad[at] = bad;
    }
}

// A row's totals from its frames, one lane per row: the sums folded in ascending frame order from +0.0.
__global__ __launch_bounds__(256) void level_totals_kernel(const uint32_t *__restrict__ len, uint64_t row_stride,
                                                           uint32_t n_rows, uint32_t F, const double *__restrict__ fsum,
                                                           const float *__restrict__ fpeak,
                                                           const uint32_t *__restrict__ fbad, uint64_t frames_stride,
                                                           double *__restrict__ sumsq, float *__restrict__ peak,
                                                           uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;
    const uint64_t frames = (n + F - 1u) / F;
    const uint64_t at = u * frames_stride;
    double s = 0.0;
    uint32_t m = 0u, b = 0u;
    for (uint64_t f = 0; f < frames; ++f) {
        s = s + fsum[at + f];
        const uint32_t pb = __float_as_uint(fpeak[at + f]);
        m = pb > m ? pb : m;
        b += fbad[at + f];
    }
    if (sumsq) sumsq[u] = s;
    if (peak) peak[u] = __uint_as_float(m);
    if (nonfinite) nonfinite[u] = b;
}

}  // namespace

hipError_t launch_level_frames(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows,
                               uint32_t frame, uint32_t grid_frames, double *fsum, float *fpeak, uint32_t *fbad,
                               uint64_t frames_stride, hipStream_t stream)
{
    const uint64_t waves = (uint64_t)n_rows * grid_frames;
    if (waves == 0) return hipSuccess;
    const uint64_t groups = (waves + 3u) / 4u;
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && (row_stride & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(level_frames_kernel<true>, dim3((uint32_t)groups), dim3(256), 0, stream, rows, row_stride, len,
                           n_rows, frame, grid_frames, fsum, fpeak, fbad, frames_stride);
    else
        hipLaunchKernelGGL(level_frames_kernel<false>, dim3((uint32_t)groups), dim3(256), 0, stream, rows, row_stride, len,
                           n_rows, frame, grid_frames, fsum, fpeak, fbad, frames_stride);
    return hipGetLastError();
}

hipError_t launch_level_totals(const uint32_t *len, uint64_t row_stride, uint32_t n_rows, uint32_t frame,
                               const double *fsum, const float *fpeak, const uint32_t *fbad, uint64_t frames_stride,
                               double *sumsq, float *peak, uint32_t *nonfinite, hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(level_totals_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, stream, len, row_stride, n_rows,
                       frame, fsum, fpeak, fbad, frames_stride, sumsq, peak, nonfinite);
    return hipGetLastError();
}

}  // namespace grail
