// spectrum_kernels.hip — short-time spectra of rows (grail_spectrum_async).  The contract (include/grail_spectrum.h, "levels,
// continued: short-time spectra"): frames of W windowed samples every H, a radix-2 decimation-in-time transform of N = 2^p
// complex numbers whose twiddles come from the host's table, the power of the bins 0 .. N/2 and left folds of it over bands;
// binary64, every operation rounded by itself, one rounding to binary32 at each store.  One workgroup of 256 lanes takes
// SPECTRUM_CHUNK_FRAMES consecutive frames of one row: N >= 512 a frame at a time, all four waves on it; N <= 256 four frames
// at a time, a wave each.  A frame lives in LDS as N complex doubles, the twiddles staged once a workgroup beside it.  The
// full flow graph is computed (DESIGN.md §4.25 says why not half of it), two stages to a pass over LDS: a lane holds the four
// numbers that two consecutive stages combine, so the operations and their order are the contract's and the passes half as
// many.  No atomics, every store a plain vector store.
#include "kernels.h"
#include "row_kernel_common.h"
#include "spectrum_plan.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

namespace {

constexpr uint32_t SPECTRUM_THREADS = 256;

// the lanes on one frame and the frames a workgroup works on side by side
__host__ __device__ constexpr uint32_t spectrum_lanes(uint32_t P) { return P <= 8u ? 64u : SPECTRUM_THREADS; }
__host__ __device__ constexpr uint32_t spectrum_side(uint32_t P) { return SPECTRUM_THREADS / spectrum_lanes(P); }

// one butterfly of the contract: t = v * w, four products, a difference and a sum; then u + t and u - t
__device__ __forceinline__ void butterfly(double2 &u, double2 &v, const double2 w)
{
    const double tr = (v.x * w.x) - (v.y * w.y);
    const double ti = (v.x * w.y) + (v.y * w.x);
    const double2 a = u;
    u.x = a.x + tr, u.y = a.y + ti;
    v.x = a.x - tr, v.y = a.y - ti;
}

// Stages s = 1 .. P on the frame at A, by the LANES lanes whose index among them is l.  P odd: stage 1 alone first.  Then
// stages (s, s + 1) together: with h = 2^(s-1), a lane takes g + k + {0, h, 2h, 3h}, g a multiple of 4h and k < h: stage s
// pairs the first with the second and the third with the fourth on T[k N / 2h], stage s + 1 the first with the third on
// T[k N / 4h] and the second with the fourth on T[(k + h) N / 4h].  Every lane of the workgroup comes here (barriers).
template <uint32_t P, uint32_t LANES>
__device__ __forceinline__ void spectrum_stages(double2 *A, const double2 *T, uint32_t l, bool live)
{
    constexpr uint32_t N = 1u << P;
    uint32_t s = 1;
    if (P & 1u) {
        if (live) {
            const double2 w = T[0];
            for (uint32_t i = l; i < N / 2u; i += LANES) {
                double2 u = A[2u * i], v = A[2u * i + 1u];
                butterfly(u, v, w);
                A[2u * i] = u, A[2u * i + 1u] = v;
            }
        }
        __syncthreads();
        s = 2;
    }
#pragma unroll
    for (; s < P; s += 2u) {
        if (live) {
            const uint32_t h = 1u << (s - 1u);
            for (uint32_t q = l; q < N / 4u; q += LANES) {
                const uint32_t k = q & (h - 1u);
                const uint32_t i0 = ((q >> (s - 1u)) << (s + 1u)) + k;
                double2 x0 = A[i0], x1 = A[i0 + h], x2 = A[i0 + 2u * h], x3 = A[i0 + 3u * h];
                const double2 w = T[k << (P - s)];
                butterfly(x0, x1, w);
                butterfly(x2, x3, w);
                butterfly(x0, x2, T[k << (P - s - 1u)]);
                butterfly(x1, x3, T[(k + h) << (P - s - 1u)]);
                A[i0] = x0, A[i0 + h] = x1, A[i0 + 2u * h] = x2, A[i0 + 3u * h] = x3;
            }
        }
        __syncthreads();
    }
}

// a sample of the row as it enters a frame: +0.0 outside [0, n) and where it is not finite
__device__ __forceinline__ double spectrum_sample(float x, bool inside)
{
    return (inside && finite_f32(x)) ? (double)x : 0.0;
}

// Frame f of the row into A: A[rev(j)] = ((double)w[j] * v[f H - pad + j], +0.0) for j < W, (+0.0, +0.0) from W on.  VEC: the
// row starts on 16 bytes and t0 is a multiple of 4, so four samples [t0, t0 + 4) inside [0, n) are one 16-byte load; the groups
// that straddle 0 or n go sample by sample.  Nothing at or past n is read.
template <uint32_t P, uint32_t LANES, bool VEC>
__device__ __forceinline__ void spectrum_stage_frame(double2 *A, const float *__restrict__ row, uint64_t n, int64_t start,
                                                     const float *__restrict__ window, uint32_t W, uint32_t l)
{
    constexpr uint32_t N = 1u << P;
    if (VEC) {
        const int64_t a0 = start & ~(int64_t)3;
        const uint32_t groups = (uint32_t)((start + (int64_t)W - a0 + 3) >> 2);
        for (uint32_t g = l; g < groups; g += LANES) {
            const int64_t t0 = a0 + 4 * (int64_t)g;
            float x[4];
            if (t0 >= 0 && (uint64_t)t0 + 4u <= n) {
                const float4 v = *reinterpret_cast<const float4 *>(row + t0);
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = (t0 + e >= 0 && (uint64_t)(t0 + e) < n) ? row[t0 + e] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t t = t0 + e, j = t - start;
                if (j < 0 || j >= (int64_t)W) continue;
                const double a = (double)window[j] * spectrum_sample(x[e], t >= 0 && (uint64_t)t < n);
                A[__brev((uint32_t)j) >> (32u - P)] = make_double2(a, 0.0);
            }
        }
    } else {
        for (uint32_t j = l; j < W; j += LANES) {
            const int64_t t = start + (int64_t)j;
            const bool inside = t >= 0 && (uint64_t)t < n;
            const float x = inside ? row[t] : 0.0f;
            const double a = (double)window[j] * spectrum_sample(x, inside);
            A[__brev(j) >> (32u - P)] = make_double2(a, 0.0);
        }
    }
    for (uint32_t j = W + l; j < N; j += LANES) A[__brev(j) >> (32u - P)] = make_double2(0.0, 0.0);
}

// One workgroup = (row u, chunk c): frames [8 c, 8 c + 8) of the row, as many as it has.  The chunk owns the samples of its
// frames' hops, [8 c H, min((8 c + 8) H, n)): it counts the non-finite ones among them (each sample of a row has one owner,
// however the frames overlap).  That pass is the first to touch the chunk's samples; that the frames' loads behind it then find
// them in the caches, so that a sample comes from HBM once, is the supposition (FETCH_SIZE was not collected: DESIGN.md §4.25).
template <uint32_t P, bool VEC>
__global__ __launch_bounds__(SPECTRUM_THREADS) void spectrum_kernel(SpectrumArgs a)
{
    constexpr uint32_t N = 1u << P, LANES = spectrum_lanes(P), SIDE = spectrum_side(P), BINS = N / 2u + 1u;
    __shared__ double2 frame[SIDE * N];
    __shared__ double2 T[N / 2u];
    __shared__ uint32_t red[4];
    const uint32_t tid = threadIdx.x;
    uint64_t u;
    uint32_t c;
    chunk_of_block(a.grid_chunks, u, c);
    const uint64_t n = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;       // (never past the row, whatever len holds)
    const uint64_t n_frames = (n + a.hop - 1u) / a.hop;                         // (n < 2^32)
    const uint64_t f_begin = (uint64_t)c * SPECTRUM_CHUNK_FRAMES;
    if (f_begin >= n_frames) return;                                            // (the whole workgroup)
    const uint64_t f_end = f_begin + SPECTRUM_CHUNK_FRAMES < n_frames ? f_begin + SPECTRUM_CHUNK_FRAMES : n_frames;
    const float *row = a.rows + u * a.row_stride;
    for (uint32_t i = tid; i < N / 2u; i += SPECTRUM_THREADS) T[i] = reinterpret_cast<const double2 *>(a.twiddles)[i];
    if (a.cbad) {
        const uint64_t lo = f_begin * a.hop, hi = f_end * a.hop < n ? f_end * a.hop : n;
        uint32_t bad = 0;
        for (uint64_t t = lo + tid; t < hi; t += SPECTRUM_THREADS) bad += finite_f32(row[t]) ? 0u : 1u;
        block_count_store(bad, red, tid, a.cbad, u, a.grid_chunks, c);
    }
    const uint32_t l = tid % LANES, slot = tid / LANES;
    double2 *A = frame + slot * N;
    double *Pd = reinterpret_cast<double *>(A + BINS);          // P[0 .. N/2] over A[N/2 + 1 ..], which the power no longer reads
    for (uint64_t f0 = f_begin; f0 < f_end; f0 += SIDE) {
        const uint64_t f = f0 + slot;
        const bool live = f < f_end;
        if (live) spectrum_stage_frame<P, LANES, VEC>(A, row, n, (int64_t)(f * a.hop) - (int64_t)a.pad, a.window, a.n_window, l);
        __syncthreads();                                        // the frame and (the first time) the twiddles are there
        spectrum_stages<P, LANES>(A, T, l, live);
        const uint64_t at = u * a.frames_stride + f;
        if (live) {
            for (uint32_t k = l; k < BINS; k += LANES) {
                const double2 z = A[k];
                const double p = (z.x * z.x) + (z.y * z.y);
                if (a.bands) Pd[k] = p;
                if (a.power) a.power[at * BINS + k] = (float)p;
            }
        }
        __syncthreads();                                        // every P[k] is there
        if (live && a.bands) {
            for (uint32_t b = l; b < a.n_bands; b += LANES) {
                const uint32_t *d = a.band_desc + b * SPECTRUM_BAND_WORDS;
                const uint32_t first = d[0], count = d[1];
                const float *wt = a.band_weights + d[2];
                double e = 0.0;
                for (uint32_t k = 0; k < count; ++k) e = e + ((double)wt[k] * Pd[first + k]);
                a.bands[at * a.n_bands + b] = (float)e;
            }
        }
        __syncthreads();                                        // ... and read, before the next frame lands on it
    }
}

__global__ __launch_bounds__(256) void spectrum_totals_kernel(SpectrumArgs a)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= a.n_rows) return;
    const uint64_t n = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;
    const uint64_t n_frames = (n + a.hop - 1u) / a.hop;
    if (a.n_frames) a.n_frames[u] = (uint32_t)n_frames;
    if (a.nonfinite) a.nonfinite[u] = sum_chunks(a.cbad, u, a.grid_chunks, (n_frames + SPECTRUM_CHUNK_FRAMES - 1u) / SPECTRUM_CHUNK_FRAMES);
}

template <uint32_t P>
void spectrum_launch_vec(const SpectrumArgs &a, bool vec, uint32_t workgroups, hipStream_t stream)
{
    if (vec)
        hipLaunchKernelGGL((spectrum_kernel<P, true>), dim3(workgroups), dim3(SPECTRUM_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((spectrum_kernel<P, false>), dim3(workgroups), dim3(SPECTRUM_THREADS), 0, stream, a);
}

}  // namespace

hipError_t launch_spectrum(const SpectrumArgs &args, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)args.n_rows * args.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    const bool vec = aligned16(args.rows, args.row_stride);
    switch (args.log2n) {
    case 6: spectrum_launch_vec<6>(args, vec, (uint32_t)workgroups, stream); break;
    case 7: spectrum_launch_vec<7>(args, vec, (uint32_t)workgroups, stream); break;
    case 8: spectrum_launch_vec<8>(args, vec, (uint32_t)workgroups, stream); break;
    case 9: spectrum_launch_vec<9>(args, vec, (uint32_t)workgroups, stream); break;
    case 10: spectrum_launch_vec<10>(args, vec, (uint32_t)workgroups, stream); break;
    case 11: spectrum_launch_vec<11>(args, vec, (uint32_t)workgroups, stream); break;
    case 12: spectrum_launch_vec<12>(args, vec, (uint32_t)workgroups, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_spectrum_totals(const SpectrumArgs &args, hipStream_t stream)
{
    if (args.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(spectrum_totals_kernel, dim3((args.n_rows + 255u) / 256u), dim3(256), 0, stream, args);
    return hipGetLastError();
}

}  // namespace grail
