// true_peak_kernels.hip — the true peak of rendered rows (grail_true_peak_async).  The contract (include/grail_hip.h,
// "levels, continued: true peak"): every sample through the 4-phase x 12-tap filter of BS.1770-4 Annex 2 in binary64,
// each output the left fold acc = acc + C[p][k] * v[t - k] over ascending k from +0.0, a row's number the largest |y|
// over its n + 11 output times and four phases.  The filter is FIR and a maximum has no order, so time is parallel: one
// wave per (row, chunk of output times), and a lone long row fills the device.  No atomics, every store a plain vector
// store.  DESIGN.md §4.11.
#include "kernels.h"
#include "row_kernel_common.h"
#include "true_peak_taps.h"

namespace grail {

namespace {

constexpr uint32_t TP_CHUNK = 4096;     // output times of one wave (not part of the contract: a maximum has no order)
constexpr int TP_STEPS = 4;             // 256-output steps whose loads a wave issues before the first use (16 x 16 B per lane)
constexpr uint32_t TP_TAIL = 11;        // the outputs after a row's last sample: the filter rings on for taps - 1 samples

// TP_STEPS steps of one chunk, from step s0 on: all their loads, then the filter.  Everything is counted from the
// chunk's origin o = (its first output time) - 12, a multiple of 4: lane l of step s owns the outputs at r0 + 12 .. r0 + 15
// with r0 = 256 s + 4 l and needs the samples r0 + 1 .. r0 + 15, which it takes with four overlapping 16-byte loads of
// the groups r0 / 4 .. r0 / 4 + 3 (three of them were or will be another lane's own group: hits in the vector cache, no
// cross-lane traffic and no carry from step to step).  A sample lies in the row when lo <= r < hi; a group index is
// clamped to the row's first and last group and a 4-byte load to the row's first and last sample, so every load is in
// bounds and none sits behind a branch; what a clamped load brings is outside [lo, hi) and enters as +0.0, as does a
// sample that is not finite.  An output past the row's n + 11 has no sample in [lo, hi) and reads +0.0: it needs no mask.
template <bool VEC>
__device__ __forceinline__ void true_peak_steps(const float *__restrict__ row, int64_t o, uint32_t s0, uint32_t lo,
                                                uint32_t hi, uint32_t lane, double &best, uint32_t &bad)
{
    float x[TP_STEPS][16];
#pragma unroll
    for (int i = 0; i < TP_STEPS; ++i) {
        const uint32_t r0 = (s0 + i) * 256u + 4u * lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (VEC) {
                // the row's last group starts below n <= row_stride, a multiple of 4: inside the row
                const uint32_t g_lo = (lo + 3u) >> 2, g_hi = (hi - 1u) >> 2;
                uint32_t g = (r0 >> 2) + q;
                g = g < g_lo ? g_lo : g;
                g = g > g_hi ? g_hi : g;
                const float4 v = *reinterpret_cast<const float4 *>(row + (o + (int64_t)(4u * g)));
                x[i][4 * q + 0] = v.x;
                x[i][4 * q + 1] = v.y;
                x[i][4 * q + 2] = v.z;
                x[i][4 * q + 3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t r = r0 + 4u * q + k;
                    r = r < lo ? lo : r;
                    r = r > hi - 1u ? hi - 1u : r;
                    x[i][4 * q + k] = row[o + (int64_t)r];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TP_STEPS; ++i) {
        const uint32_t r0 = (s0 + i) * 256u + 4u * lane;
        double v[16];
#pragma unroll
        for (int j = 1; j < 16; ++j) {
            const bool inside = r0 + j - lo < hi - lo;
            const bool finite = finite_f32(x[i][j]);
            if (j >= 12) bad += (inside && !finite) ? 1u : 0u;                           // (the lane's own four: counted once)
            v[j] = (double)((inside && finite) ? x[i][j] : 0.0f);
        }
        // 16 independent chains of 12: C * v is exact (a 13-bit numerator times a 24-bit significand), so the fused
        // multiply-add is the contract's multiply and add
        double peak[4];
#pragma unroll
        for (int out = 0; out < 4; ++out) {
            double y[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 12; ++k) acc = __builtin_fma(true_peak_tap(p, k), v[12 + out - k], acc);
                y[p] = __builtin_fabs(acc);
            }
            peak[out] = __builtin_fmax(__builtin_fmax(y[0], y[1]), __builtin_fmax(y[2], y[3]));
        }
        // (no NaN reaches here and nothing is negative: the maximum is exact and has no order)
        best = __builtin_fmax(best, __builtin_fmax(__builtin_fmax(peak[0], peak[1]), __builtin_fmax(peak[2], peak[3])));
    }
}

// One wave = one (row, chunk of TP_CHUNK output times); the row's output times are 0 .. n + 10.  VEC = false is the same
// mapping with 4-byte loads, for rows whose base is not 16-byte aligned or whose stride is no multiple of 4.
template <bool VEC>
__global__ __launch_bounds__(256) void true_peak_frames_kernel(const float *__restrict__ rows, uint64_t row_stride,
                                                               const uint32_t *__restrict__ len, uint32_t n_rows,
                                                               uint32_t grid_chunks, double *__restrict__ cmax,
                                                               uint32_t *__restrict__ cbad)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * 4u + wave;
    const uint64_t u = w / grid_chunks;
    if (u >= n_rows) return;
    const uint32_t c = (uint32_t)(w - u * grid_chunks);
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;       // (never past the row, whatever len holds)
    const uint64_t outputs = n ? n + TP_TAIL : 0u;
    const uint64_t start = (uint64_t)c * TP_CHUNK;
    if (start >= outputs) return;                                       // chunks past the row's last: nothing written
    const uint64_t left = outputs - start;
    const uint32_t steps = left < TP_CHUNK ? (uint32_t)((left + 255u) >> 8) : TP_CHUNK / 256u;
    const int64_t o = (int64_t)start - 12;
    const uint32_t lo = c ? 0u : 12u;                                   // the row's first sample, counted from o
    const int64_t span = (int64_t)n - o;                                // ... and its end: >= lo + 1, since start <= n + 10
    const uint32_t hi = span < 8192 ? (uint32_t)span : 8192u;           // (a chunk looks at 0 .. 4 107 only)
    const float *row = rows + u * row_stride;
    double best = 0.0;
    uint32_t bad = 0u;
    // (a slot past `steps` stays inside the chunk, 16 = 4 x TP_STEPS, and holds outputs past the row's last: +0.0)
    for (uint32_t s = 0; s < steps; s += TP_STEPS) true_peak_steps<VEC>(row, o, s, lo, hi, lane, best, bad);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        best = __builtin_fmax(best, __shfl_xor(best, d, 64));
        bad += (uint32_t)__shfl_xor((int)bad, d, 64);
    }
    if (lane == 0u) {
        const uint64_t at = u * grid_chunks + c;
        cmax[at] = best;
        cbad[at] = bad;
    }
}

// A row's numbers from its chunks, one lane per row.
__global__ __launch_bounds__(256) void true_peak_totals_kernel(const uint32_t *__restrict__ len, uint64_t row_stride,
                                                               uint32_t n_rows, const double *__restrict__ cmax,
                                                               const uint32_t *__restrict__ cbad, uint32_t grid_chunks,
                                                               double *__restrict__ true_peak,
                                                               uint32_t *__restrict__ nonfinite)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;
    const uint64_t chunks = n ? (n + TP_TAIL + TP_CHUNK - 1u) / TP_CHUNK : 0u;
    const uint64_t at = u * grid_chunks;
    double m = 0.0;
    uint32_t b = 0u;
    for (uint64_t c = 0; c < chunks; ++c) {
        m = __builtin_fmax(m, cmax[at + c]);
        b += cbad[at + c];
    }
    if (true_peak) true_peak[u] = m;
    if (nonfinite) nonfinite[u] = b;
}

}  // namespace

uint64_t true_peak_grid_chunks(uint64_t row_stride)
{
    return row_stride ? (row_stride + TP_TAIL + TP_CHUNK - 1u) / TP_CHUNK : 0u;
}

hipError_t launch_true_peak_frames(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows,
                                   uint32_t grid_chunks, double *cmax, uint32_t *cbad, hipStream_t stream)
{
    const uint64_t waves = (uint64_t)n_rows * grid_chunks;
    if (waves == 0) return hipSuccess;
    const uint64_t groups = (waves + 3u) / 4u;
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && (row_stride & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(true_peak_frames_kernel<true>, dim3((uint32_t)groups), dim3(256), 0, stream, rows, row_stride,
                           len, n_rows, grid_chunks, cmax, cbad);
    else
        hipLaunchKernelGGL(true_peak_frames_kernel<false>, dim3((uint32_t)groups), dim3(256), 0, stream, rows, row_stride,
                           len, n_rows, grid_chunks, cmax, cbad);
    return hipGetLastError();
}

hipError_t launch_true_peak_totals(const uint32_t *len, uint64_t row_stride, uint32_t n_rows, const double *cmax,
                                   const uint32_t *cbad, uint32_t grid_chunks, double *true_peak, uint32_t *nonfinite,
                                   hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(true_peak_totals_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, stream, len, row_stride, n_rows,
                       cmax, cbad, grid_chunks, true_peak, nonfinite);
    return hipGetLastError();
}

}  // namespace grail
