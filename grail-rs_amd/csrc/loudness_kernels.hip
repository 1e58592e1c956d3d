// loudness_kernels.hip — K-weighted, gated loudness of rendered rows (grail_loudness_async).  The contract
// (include/grail_hip.h, "levels, continued"): two biquads in transposed direct form II along each row, binary64, every
// operation rounded by itself, z*z folded per hop of H samples; then the BS.1770 gate over a row's hops.  The recurrence
// is serial along a row in exact arithmetic, so the parallelism is across rows: one lane per row, 64 rows per wave.
// No atomics, every store a plain vector store.  DESIGN.md §4.10.
#include "kernels.h"
#include "loudness_common.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

using namespace loud;

namespace {

// One tile's loads: wave-instruction i reads samples [t0, t0 + 64) of the rows 4i .. 4i + 3 of the wave, lane l the four
// samples from 4 (l mod 16) on of row 4i + l / 16: whole 256-byte pieces of rows, 16 loads in flight before the first use.
// A row past the launch's last reads the last row; a group of four past the row's stride reads the row's last group (a
// single sample: the row's last): every load lies inside rows[n_rows][row_stride] and none sits behind a branch.  What
// such a slot holds belongs to no row's samples t < n and is never counted.
template <bool VEC>
__device__ __forceinline__ void loud_load(const float *__restrict__ rows, uint64_t row_stride, uint32_t n_rows,
                                          uint64_t row0, uint64_t t0, uint32_t lane, float (&x)[LOUD_LOADS][4])
{
    const uint64_t col = t0 + 4u * (lane & 15u);
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        uint64_t r = row0 + 4u * i + (lane >> 4);
        r = r < n_rows ? r : n_rows - 1u;
        const float *src = rows + r * row_stride;
        if (VEC) {
            const uint64_t o = col < row_stride ? col : row_stride - 4u;        // (row_stride is a multiple of 4 and >= 4)
            const float4 v = *reinterpret_cast<const float4 *>(src + o);
            x[i][0] = v.x;
            x[i][1] = v.y;
            x[i][2] = v.z;
            x[i][3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint64_t o = col + k < row_stride ? col + k : row_stride - 1u;
                x[i][k] = src[o];
            }
        }
    }
}

// One wave = 64 rows, lane r = row row0 + r, from the rows' first sample to the longest row's last in tiles of 64
// samples.  The next tile's loads are issued before the current tile is filtered and land in LDS after it, so they are
// in flight for the whole of a tile's arithmetic.  A lane past its row's end goes on filtering what the tile holds (its
// state is never read again): only the count and the hop stores look at n.  H is one number for the launch, so a hop's
// end is wave-uniform: the tile is walked in runs that end at the tile's or the hop's end, and a hop's sum is one store
// per lane between two runs.
template <bool VEC>
__global__ __launch_bounds__(64) void loudness_hops_kernel(const float *__restrict__ rows, uint64_t row_stride,
                                                           const uint32_t *__restrict__ len, uint32_t n_rows, uint32_t H,
                                                           LoudCoef coef, double *__restrict__ hops, uint64_t hops_stride,
                                                           uint32_t *__restrict__ nonfinite)
{
    __shared__ float tile[LOUD_ROWS * LOUD_PITCH];
    const uint32_t lane = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * LOUD_ROWS;
    const uint64_t u = row0 + lane;
    const bool mine = u < n_rows;
    uint64_t n = 0;
    if (mine) n = len[u] < row_stride ? len[u] : row_stride;               // (never past the row, whatever len holds)
    // the wave's longest row
    uint64_t longest = n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)longest, d, 64);
        longest = o > longest ? o : longest;
    }
    longest = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(longest >> 32)) << 32) |
              __builtin_amdgcn_readfirstlane((uint32_t)longest);
    const uint64_t whole = n / H * H;                   // the samples of the row's whole hops
    double *const my_hops = hops + u * hops_stride;
    KState k = {0.0, 0.0, 0.0, 0.0, 0.0, 0u};
    const float *mine_lds = tile + lane * LOUD_PITCH;
    float x[LOUD_LOADS][4];
    if (longest) {
        loud_load<VEC>(rows, row_stride, n_rows, row0, 0, lane, x);
        loud_stash(tile, lane, x);
    }
    __syncthreads();
    uint64_t hop_end = H;                               // the end of the hop the next sample lies in (uniform)
    uint64_t hop = 0;
    for (uint64_t t0 = 0; t0 < longest; t0 += LOUD_T) {
        const bool more = t0 + LOUD_T < longest;
        if (more) loud_load<VEC>(rows, row_stride, n_rows, row0, t0 + LOUD_T, lane, x);
        uint32_t i = 0;
        while (i < LOUD_T) {
            const uint64_t left = hop_end - (t0 + i);
            const uint32_t run = left < LOUD_T - i ? (uint32_t)left : LOUD_T - i;
            uint32_t j = 0;
            for (; j + 8u <= run; j += 8u) {
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) loud_sample(mine_lds[i + j + q], t0 + i + j + q < n, coef.c, k);
            }
            for (; j < run; ++j) loud_sample(mine_lds[i + j], t0 + i + j < n, coef.c, k);
            i += run;
            if (t0 + i == hop_end) {
                if (hop_end <= whole) my_hops[hop] = k.acc;
                k.acc = 0.0;
                hop_end += H;
                ++hop;
            }
        }
        __syncthreads();                                // every lane has read the tile
        if (more) loud_stash(tile, lane, x);
        __syncthreads();
    }
    if (mine && nonfinite) nonfinite[u] = k.bad;
}

// The gate over a row's hops, one lane per row (as level_totals_kernel folds a row's frames).
__global__ __launch_bounds__(256) void loudness_gate_kernel(const uint32_t *__restrict__ len, uint64_t row_stride,
                                                            uint32_t n_rows, uint32_t H, const double *__restrict__ hops,
                                                            uint64_t hops_stride, double *__restrict__ gated)
{
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= n_rows) return;
    const uint64_t n = len[u] < row_stride ? len[u] : row_stride;
    const uint64_t n_hops = n / H;
    if (n_hops < 4u) {
        gated[u] = 0.0;
        return;
    }
    const double *h = hops + u * hops_stride;
    const uint64_t blocks = n_hops - 3u;
    const double per = 4.0 * (double)H;
    double sum = 0.0;
    uint32_t count = 0;
    for (uint64_t j = 0; j < blocks; ++j) {
        const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / per;
        if (z > GRAIL_LOUDNESS_ABS_GATE) {
            sum = sum + z;
            ++count;
        }
    }
    if (count == 0u) {
        gated[u] = 0.0;
        return;
    }
    const double r = 0.1 * (sum / (double)count);
    sum = 0.0;
    count = 0;
    for (uint64_t j = 0; j < blocks; ++j) {
        const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / per;
        if (z > GRAIL_LOUDNESS_ABS_GATE && z > r) {
            sum = sum + z;
            ++count;
        }
    }
    gated[u] = count ? sum / (double)count : 0.0;
}

}  // namespace

hipError_t launch_loudness_hops(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_rows, uint32_t hop,
                                const double *coef, double *hops, uint64_t hops_stride, uint32_t *nonfinite,
                                hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    LoudCoef c;
    for (int i = 0; i < 10; ++i) c.c[i] = coef[i];
    const uint32_t groups = (n_rows + LOUD_ROWS - 1u) / LOUD_ROWS;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0 && (row_stride & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(loudness_hops_kernel<true>, dim3(groups), dim3(64), 0, stream, rows, row_stride, len, n_rows, hop,
                           c, hops, hops_stride, nonfinite);
    else
        hipLaunchKernelGGL(loudness_hops_kernel<false>, dim3(groups), dim3(64), 0, stream, rows, row_stride, len, n_rows, hop,
                           c, hops, hops_stride, nonfinite);
    return hipGetLastError();
}

hipError_t launch_loudness_gate(const uint32_t *len, uint64_t row_stride, uint32_t n_rows, uint32_t hop, const double *hops,
                                uint64_t hops_stride, double *gated, hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(loudness_gate_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, stream, len, row_stride, n_rows,
                       hop, hops, hops_stride, gated);
    return hipGetLastError();
}

}  // namespace grail
