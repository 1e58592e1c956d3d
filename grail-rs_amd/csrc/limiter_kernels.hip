// limiter_kernels.hip — the look-ahead limiter of finished tracks (grail_limit_async).  The contract (include/grail_hip.h,
// "levels, continued: limiter"): per sample the detector d[t] = max(|v[t]|, e[t] .. e[t + 11]) over the true-peak filter's
// outputs, the required gain as an integer q[t] = min(Q, floor(c Q / d[t])) of Q = 2^24, its minimum over the next L
// samples, the sum of L of those minima, one rounding to binary32 and the product.  Integers have no order to fix and
// the filter is FIR, so time is parallel: one workgroup per (group of rows, chunk of LIMIT_CHUNK samples), which works
// out the q it needs (its samples and L - 1 either side) in LDS from the rows themselves.  x -> min(Q, floor(c Q / x)) does
// not rise with x, so the q of a maximum is the minimum of the q's: the kernel quantises every |v| and e by itself (in
// binary64, the contract's division) and takes minima of integers from there on, across the twelve outputs and across the
// members of a group alike.  No atomics, every store a plain vector store.  DESIGN.md §4.12.
#include "kernels.h"
#include "true_peak_taps.h"

namespace grail {

namespace {

constexpr uint32_t LIMIT_Q = 1u << 24;
constexpr uint32_t LIMIT_LMAX = 1u << 10;
constexpr uint32_t LIMIT_TAPS_AFTER = 11;                           // the outputs a sample feeds after its own
// the q's of a chunk: its samples and L - 1 either side; the e's reach eleven further; + 3 for the rounding to a group of 4
constexpr uint32_t LIMIT_CELLS = (LIMIT_CHUNK + 2u * LIMIT_LMAX - 2u + LIMIT_TAPS_AFTER + 3u + 3u) & ~3u;
constexpr uint32_t LIMIT_SUM_LOG2 = 7;                              // 2^7 deficits of at most 2^24 each stay below 2^32

struct LimitChunk {
    uint64_t maxdef;        // the largest L Q - S[t] of the chunk
    uint32_t limited, bad;
};

// One wave's 256 output times of one member row, as true_peak_kernels.hip takes them: everything is counted from
// o = (the first output time wanted, rounded down to a multiple of 4) - 12; lane l of block b owns the outputs at
// r0 + 12 .. r0 + 15 with r0 = 256 b + 4 l and needs the samples r0 + 1 .. r0 + 15, taken with four overlapping 16-byte
// loads.  A sample lies in the row when lo <= r < hi (lo a multiple of 4, lo < hi); group and sample indices are clamped
// to the row, so every load is in bounds and none sits behind a branch; what a clamped load brings enters as +0.0, as
// does a sample that is not finite.  The lane's four |v| and four e = max_p |y[p]| are quantised and stored (the first
// member) or folded in by minimum (the others: same lane, same cells) at cell r0 + k - sh.
template <bool VEC>
__device__ __forceinline__ void limit_detect(const float *__restrict__ row, int64_t o, uint32_t blk, uint32_t lo, uint32_t hi,
                                             uint32_t lane, double cd, double cq, uint32_t own_lo, uint32_t own_hi, bool first,
                                             uint32_t sh, uint32_t n_q, uint32_t *qv, uint32_t *qe, uint32_t &bad, bool &hot)
{
    float x[16];
    const uint32_t r0 = blk * 256u + 4u * lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (VEC) {
            const uint32_t g_lo = lo >> 2, g_hi = (hi - 1u) >> 2;
            uint32_t g = (r0 >> 2) + q;
            g = g < g_lo ? g_lo : g;
            g = g > g_hi ? g_hi : g;
            const float4 v = *reinterpret_cast<const float4 *>(row + (o + (int64_t)(4u * g)));
            x[4 * q + 0] = v.x;
            x[4 * q + 1] = v.y;
            x[4 * q + 2] = v.z;
            x[4 * q + 3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t r = r0 + 4u * q + k;
                r = r < lo ? lo : r;
                r = r > hi - 1u ? hi - 1u : r;
                x[4 * q + k] = row[o + (int64_t)r];
            }
        }
    }
    double v[16];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const bool inside = r0 + j - lo < hi - lo;
        const bool finite = __builtin_fabsf(x[j]) <= 3.4028234663852886e38f;            // false for NaN and Inf
        // (the lane's own four, and only in the chunk's own samples: a sample is counted once)
        if (j >= 12) bad += (inside && !finite && r0 + j - own_lo < own_hi - own_lo) ? 1u : 0u;
        v[j] = (double)((inside && finite) ? x[j] : 0.0f);
    }
    double d[8];
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
        d[out] = __builtin_fmax(__builtin_fmax(y[0], y[1]), __builtin_fmax(y[2], y[3]));
        d[4 + out] = __builtin_fabs(v[12 + out]);
    }
    // the division only in a wave that holds a number above the ceiling (speech at -23 LUFS: hardly any)
    bool above = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) above = above || d[i] > cd;
    uint32_t q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = LIMIT_Q;
    if (__builtin_amdgcn_ballot_w64(above) != 0ull) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool over = d[i] > cd;
            const double ratio = cq / (over ? d[i] : cq);                               // correctly rounded; <= 2^24 (1 + 2^-52)
            const uint32_t f = (uint32_t)ratio;                                         // (>= 0: the floor)
            q[i] = over ? (f < LIMIT_Q ? f : LIMIT_Q) : LIMIT_Q;
        }
    }
    hot = hot || above;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t cell = r0 + k - sh;                                              // (wraps below 0: fails both tests)
        if (cell < n_q + LIMIT_TAPS_AFTER) qe[cell] = first ? q[k] : (qe[cell] < q[k] ? qe[cell] : q[k]);
        if (cell < n_q) qv[cell] = first ? q[4 + k] : (qv[cell] < q[4 + k] ? qv[cell] : q[4 + k]);
    }
}

// the length all members of a group share, or false
__device__ __forceinline__ bool limit_group_len(const uint32_t *__restrict__ len, uint64_t row_stride, uint64_t first_row,
                                                uint32_t group, uint64_t &n)
{
    n = len[first_row] < row_stride ? len[first_row] : row_stride;
    bool same = true;
    for (uint32_t j = 1; j < group; ++j) {
        const uint64_t nj = len[first_row + j] < row_stride ? len[first_row + j] : row_stride;
        same = same && nj == n;
    }
    return same;
}

// One workgroup = one (group, chunk of LIMIT_CHUNK samples).  VEC = false is the same mapping with 4-byte loads and
// stores, for bases that are not 16-byte aligned or strides that are no multiple of 4.
template <bool VEC>
__global__ __launch_bounds__(256) void limit_frames_kernel(const float *__restrict__ rows, uint64_t row_stride,
                                                           const uint32_t *__restrict__ len, uint32_t n_groups, uint32_t group,
                                                           float ceiling, uint32_t ell, uint32_t grid_chunks,
                                                           float *__restrict__ out, uint64_t out_stride,
                                                           LimitChunk *__restrict__ cstat)
{
    __shared__ uint32_t cells_a[LIMIT_CELLS];
    __shared__ uint32_t cells_b[LIMIT_CELLS];
    __shared__ LimitChunk red[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane = tid & 63u;
    const uint32_t grp = blockIdx.x / grid_chunks;
    const uint32_t chunk = blockIdx.x - grp * grid_chunks;
    if (grp >= n_groups) return;
    const uint64_t first_row = (uint64_t)grp * group;
    uint64_t n;
    if (!limit_group_len(len, row_stride, first_row, group, n)) return;      // refused: nothing written (the totals say so)
    const uint64_t t0 = (uint64_t)chunk * LIMIT_CHUNK;
    if (t0 >= n) return;                                                     // chunks past the group's last: nothing written
    const uint32_t L = 1u << ell;
    const uint32_t count = n - t0 < LIMIT_CHUNK ? (uint32_t)(n - t0) : LIMIT_CHUNK;     // the chunk's samples
    const uint32_t n_m = count + L - 1u;                                     // the minima m[s], s = t0 - (L - 1) .. t0 + count - 1
    const uint32_t n_q = n_m + L - 1u;                                       // the q[s] under them, s from a = t0 - (L - 1) on
    const int64_t a = (int64_t)t0 - (int64_t)(L - 1u);
    const uint32_t sh = (uint32_t)(a & 3);                                   // a - (a rounded down to a multiple of 4)
    const int64_t o = a - (int64_t)sh - 12;
    const uint32_t lo = o < 0 ? (uint32_t)(-o) : 0u;                         // the row's first sample, counted from o
    const int64_t span = (int64_t)n - o;                                     // ... and its end: > t0 - o >= lo
    const uint32_t hi = span < 16384 ? (uint32_t)span : 16384u;              // (a chunk looks at fewer than 6 200 samples)
    const uint32_t own_lo = (uint32_t)((int64_t)t0 - o), own_hi = own_lo + count;
    const uint32_t blocks = (n_q + LIMIT_TAPS_AFTER + sh + 255u) >> 8;
    const double cd = (double)ceiling, cq = cd * 16777216.0;                 // (exact)

    // 1, 2: every member's |v| and e, quantised; the group's by minimum
    uint32_t bad = 0u;
    bool hot = false;
    for (uint32_t j = 0; j < group; ++j) {
        const float *row = rows + (first_row + j) * row_stride;
        for (uint32_t blk = wave; blk < blocks; blk += 4u)
            limit_detect<VEC>(row, o, blk, lo, hi, lane, cd, cq, own_lo, own_hi, j == 0u, sh, n_q, cells_a, cells_b, bad, hot);
    }
    // nothing above the ceiling in reach: every q is Q, every sum L Q and every gain 1.0f; the rest is skipped, same bits
    const bool work = __syncthreads_or(hot ? 1 : 0) != 0;
    uint32_t *src = cells_a, *dst = cells_b;
    uint32_t sum_log2 = 0;
    if (work) {
        // q[s] = min(|v|'s q, the twelve e's q's) inside the row, Q outside (cells_a, in place: a cell has one reader)
        for (uint32_t i = tid; i < n_q; i += 256u) {
            uint32_t q = cells_a[i];
#pragma unroll
            for (uint32_t k = 0; k <= LIMIT_TAPS_AFTER; ++k) q = cells_b[i + k] < q ? cells_b[i + k] : q;
            const int64_t s = a + (int64_t)i;
            cells_a[i] = (s >= 0 && s < (int64_t)n) ? q : LIMIT_Q;
        }
        __syncthreads();
        // 3: the minimum over L = 2^ell by doubling; a window of 2 w exists for n_q - 2 w + 1 starts
        for (uint32_t w = 1; w < L; w <<= 1) {
            const uint32_t starts = n_q - 2u * w + 1u;
            for (uint32_t i = tid; i < starts; i += 256u) dst[i] = src[i] < src[i + w] ? src[i] : src[i + w];
            __syncthreads();
            uint32_t *t = src;
            src = dst;
            dst = t;
        }
        // 4: deficits Q - m, summed by doubling while 32 bits hold them; the apply adds the blocks that are left
        for (uint32_t i = tid; i < n_m; i += 256u) src[i] = LIMIT_Q - src[i];
        __syncthreads();
        sum_log2 = ell < LIMIT_SUM_LOG2 ? ell : LIMIT_SUM_LOG2;
        for (uint32_t w = 1; w < (1u << sum_log2); w <<= 1) {
            const uint32_t starts = n_m - 2u * w + 1u;
            for (uint32_t i = tid; i < starts; i += 256u) dst[i] = src[i] + src[i + w];
            __syncthreads();
            uint32_t *t = src;
            src = dst;
            dst = t;
        }
    }
    // 5: S[t] = L Q - the deficits of m[t - L + 1 .. t], cells (t - t0) + j 2^sum_log2; g; the product; the clamp
    const uint32_t pieces = L >> sum_log2, piece = 1u << sum_log2;
    const uint64_t full = (uint64_t)L << 24;
    const double scale = __builtin_ldexp(1.0, -(int)(24u + ell));
    uint64_t maxdef = 0;
    uint32_t limited = 0u;
    for (uint32_t at = 4u * tid; at < count; at += 1024u) {
        float g[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            uint64_t def = 0;
            if (work && at + k < count)
                for (uint32_t j = 0; j < pieces; ++j) def += src[at + k + j * piece];
            maxdef = def > maxdef ? def : maxdef;
            limited += def ? 1u : 0u;
            g[k] = (float)((double)(full - def) * scale);
        }
        const bool whole = at + 4u <= count;
        for (uint32_t j = 0; j < group; ++j) {
            const float *row = rows + (first_row + j) * row_stride + t0 + at;
            float *to = out + (first_row + j) * out_stride + t0 + at;
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (VEC && whole) {
                const float4 v = *reinterpret_cast<const float4 *>(row);
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (at + k < count) x[k] = row[k];
            }
            float z[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const bool finite = __builtin_fabsf(x[k]) <= 3.4028234663852886e38f;
                float p = g[k] * x[k];
                p = p < -ceiling ? -ceiling : p;
                p = p > ceiling ? ceiling : p;
                z[k] = finite ? p : 0.0f;
            }
            if (VEC && whole) {
                *reinterpret_cast<float4 *>(to) = make_float4(z[0], z[1], z[2], z[3]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (at + k < count) to[k] = z[k];
            }
        }
    }
    // the chunk's numbers: integers, so any order
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t other = __shfl_xor((unsigned long long)maxdef, s, 64);
        maxdef = other > maxdef ? other : maxdef;
        limited += (uint32_t)__shfl_xor((int)limited, s, 64);
        bad += (uint32_t)__shfl_xor((int)bad, s, 64);
    }
    if (lane == 0u) {
        red[wave].maxdef = maxdef;
        red[wave].limited = limited;
        red[wave].bad = bad;
    }
    __syncthreads();
    if (tid == 0u) {
        LimitChunk c = red[0];
        for (int w = 1; w < 4; ++w) {
            c.maxdef = red[w].maxdef > c.maxdef ? red[w].maxdef : c.maxdef;
            c.limited += red[w].limited;
            c.bad += red[w].bad;
        }
        cstat[(uint64_t)grp * grid_chunks + chunk] = c;
    }
}

// A group's numbers from its chunks, one lane per group; a refused group says so in all three.
__global__ __launch_bounds__(256) void limit_totals_kernel(const uint32_t *__restrict__ len, uint64_t row_stride,
                                                           uint32_t n_groups, uint32_t group, uint32_t ell,
                                                           const LimitChunk *__restrict__ cstat, uint32_t grid_chunks,
                                                           float *__restrict__ min_gain, uint32_t *__restrict__ n_limited,
                                                           uint32_t *__restrict__ nonfinite)
{
    const uint64_t grp = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (grp >= n_groups) return;
    uint64_t n;
    if (!limit_group_len(len, row_stride, grp * group, group, n)) {
        if (min_gain) min_gain[grp] = __uint_as_float(0x7FC00000u);
        if (n_limited) n_limited[grp] = 0xFFFFFFFFu;
        if (nonfinite) nonfinite[grp] = 0u;
        return;
    }
    const uint64_t chunks = (n + LIMIT_CHUNK - 1u) / LIMIT_CHUNK;
    uint64_t maxdef = 0;
    uint32_t limited = 0u, bad = 0u;
    for (uint64_t c = 0; c < chunks; ++c) {
        const LimitChunk s = cstat[grp * grid_chunks + c];
        maxdef = s.maxdef > maxdef ? s.maxdef : maxdef;
        limited += s.limited;
        bad += s.bad;
    }
    const uint64_t full = (uint64_t)1 << (24u + ell);
    if (min_gain) min_gain[grp] = (float)((double)(full - maxdef) * __builtin_ldexp(1.0, -(int)(24u + ell)));
    if (n_limited) n_limited[grp] = limited;
    if (nonfinite) nonfinite[grp] = bad;
}

}  // namespace

uint64_t limit_grid_chunks(uint64_t row_stride) { return (row_stride + LIMIT_CHUNK - 1u) / LIMIT_CHUNK; }

size_t limit_chunk_bytes() { return sizeof(LimitChunk); }

hipError_t launch_limit_frames(const float *rows, uint64_t row_stride, const uint32_t *len, uint32_t n_groups, uint32_t group,
                               float ceiling, uint32_t lookahead_log2, uint32_t grid_chunks, float *out, uint64_t out_stride,
                               void *cstat, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)n_groups * grid_chunks;
    if (workgroups == 0) return hipSuccess;
    if (workgroups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const bool vec = ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0 &&
                     ((row_stride | out_stride) & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(limit_frames_kernel<true>, dim3((uint32_t)workgroups), dim3(256), 0, stream, rows, row_stride, len,
                           n_groups, group, ceiling, lookahead_log2, grid_chunks, out, out_stride, (LimitChunk *)cstat);
    else
        hipLaunchKernelGGL(limit_frames_kernel<false>, dim3((uint32_t)workgroups), dim3(256), 0, stream, rows, row_stride, len,
                           n_groups, group, ceiling, lookahead_log2, grid_chunks, out, out_stride, (LimitChunk *)cstat);
    return hipGetLastError();
}

hipError_t launch_limit_totals(const uint32_t *len, uint64_t row_stride, uint32_t n_groups, uint32_t group,
                               uint32_t lookahead_log2, const void *cstat, uint32_t grid_chunks, float *min_gain,
                               uint32_t *n_limited, uint32_t *nonfinite, hipStream_t stream)
{
    if (n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(limit_totals_kernel, dim3((n_groups + 255u) / 256u), dim3(256), 0, stream, len, row_stride, n_groups,
                       group, lookahead_log2, (const LimitChunk *)cstat, grid_chunks, min_gain, n_limited, nonfinite);
    return hipGetLastError();
}

}  // namespace grail
