// limiter_kernels.hip — the look-ahead limiter of finished tracks (grail_limit_async).  The contract (include/grail_hip.h,
// "levels, continued: limiter"): per sample the detector d[t] = max(|v[t]|, e[t] .. e[t + 11]) over the true-peak filter's
// outputs, the required gain as an integer q[t] = min(Q, floor(c Q / d[t])) of Q = 2^24, its minimum over the next L
// samples, the sum of L of those minima, one rounding to binary32 and the product.  Integers have no order to fix and
// the filter is FIR, so time is parallel: one workgroup per (group of rows, chunk of LIMIT_CHUNK samples), which works
// out the q it needs (its samples and L - 1 either side) in LDS from the rows themselves.  x -> min(Q, floor(c Q / x)) does
// not rise with x, so the q of a maximum is the minimum of the q's: the kernel quantises every |v| and e by itself (in
// binary64, the contract's division) and takes minima of integers from there on, across the twelve outputs and across the
// members of a group alike.  No atomics, every store a plain vector store.  DESIGN.md §4.12.  The passes after the detector
// are written once for rows and streams (limit_window_sums, limit_gains, limit_wave_fold, limit_chunk_store); the finite test,
// the state word and the ring are row_kernel_common.h's (§4.21).
#include "kernels.h"
#include "row_kernel_common.h"
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
        const bool finite = finite_f32(x[j]);
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

// Steps 2 to 4 of a chunk of `count` outputs, alike for a row and for a stream: from the quantised |v| (cells_a) and e (cells_b)
// of the n_q samples from time a on (the row ends at `end`) to the deficits Q - m of the n_m window minima, summed in blocks of
// 2^sum_log2; `src` is the array that holds them.  It takes the few uniforms both kernels hold anyway and works out n_m and
// n_q again: limit_frames_kernel has no scalar register to spare (passing them, or folding the wave inside
// limit_chunk_store, moved its count).  Every lane of the workgroup comes here (there are barriers inside).
__device__ __forceinline__ void limit_window_sums(uint32_t *cells_a, uint32_t *cells_b, uint32_t tid, uint32_t count, int64_t a,
                                                  int64_t end, uint32_t ell, uint32_t *&src, uint32_t &sum_log2)
{
    const uint32_t L = 1u << ell, n_m = count + L - 1u, n_q = n_m + L - 1u;
    uint32_t *dst = cells_b;
    src = cells_a;
    // q[s] = min(|v|'s q, the twelve e's q's) inside the row, Q outside (cells_a, in place: a cell has one reader)
    for (uint32_t i = tid; i < n_q; i += 256u) {
        uint32_t q = cells_a[i];
#pragma unroll
        for (uint32_t k = 0; k <= LIMIT_TAPS_AFTER; ++k) q = cells_b[i + k] < q ? cells_b[i + k] : q;
        const int64_t s = a + (int64_t)i;
        cells_a[i] = (s >= 0 && s < end) ? q : LIMIT_Q;
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

// Step 5's gains of the four outputs from `at` on: S[t] = L Q - the deficits of m[t - L + 1 .. t], the pieces left to add
__device__ __forceinline__ void limit_gains(const uint32_t *src, bool work, uint32_t at, uint32_t count, uint32_t pieces, uint32_t piece,
                                            uint64_t full, double scale, float (&g)[4], uint64_t &maxdef, uint32_t &limited)
{
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        uint64_t def = 0;
        if (work && at + k < count)
            for (uint32_t j = 0; j < pieces; ++j) def += src[at + k + j * piece];
        maxdef = def > maxdef ? def : maxdef;
        limited += def ? 1u : 0u;
        g[k] = (float)((double)(full - def) * scale);
    }
}

// a chunk's three numbers across a wave: integers, so any order
__device__ __forceinline__ void limit_wave_fold(uint64_t &maxdef, uint32_t &limited, uint32_t &bad)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t other = __shfl_xor((unsigned long long)maxdef, s, 64);
        maxdef = other > maxdef ? other : maxdef;
        limited += (uint32_t)__shfl_xor((int)limited, s, 64);
        bad += (uint32_t)__shfl_xor((int)bad, s, 64);
    }
}

// ... and, folded so, across the workgroup's four waves into the chunk's slot; red: LDS.  Every lane comes here (a barrier).
__device__ __forceinline__ void limit_chunk_store(uint64_t maxdef, uint32_t limited, uint32_t bad, LimitChunk *red, uint32_t wave,
                                                  uint32_t lane, uint32_t tid, LimitChunk *slot)
{
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
        *slot = c;
    }
}

// the smallest gain of a group from its largest deficit
__device__ __forceinline__ float limit_min_gain(uint64_t maxdef, uint32_t ell)
{
    const uint64_t full = (uint64_t)1 << (24u + ell);
    return (float)((double)(full - maxdef) * __builtin_ldexp(1.0, -(int)(24u + ell)));
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
    uint32_t *src = cells_a;
    uint32_t sum_log2 = 0;
    if (work) limit_window_sums(cells_a, cells_b, tid, count, a, (int64_t)n, ell, src, sum_log2);
    // 5: S[t] = L Q - the deficits of m[t - L + 1 .. t], cells (t - t0) + j 2^sum_log2; g; the product; the clamp
    const uint32_t pieces = L >> sum_log2, piece = 1u << sum_log2;
    const uint64_t full = (uint64_t)L << 24;
    const double scale = __builtin_ldexp(1.0, -(int)(24u + ell));
    uint64_t maxdef = 0;
    uint32_t limited = 0u;
    for (uint32_t at = 4u * tid; at < count; at += 1024u) {
        float g[4];
        limit_gains(src, work, at, count, pieces, piece, full, scale, g, maxdef, limited);
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
                const bool finite = finite_f32(x[k]);
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
    limit_wave_fold(maxdef, limited, bad);
    limit_chunk_store(maxdef, limited, bad, red, wave, lane, tid, cstat + ((uint64_t)grp * grid_chunks + chunk));
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
        refuse_counts(n_limited, nonfinite, grp);
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
    if (min_gain) min_gain[grp] = limit_min_gain(maxdef, ell);
    if (n_limited) n_limited[grp] = limited;
    if (nonfinite) nonfinite[grp] = bad;
}

// ---- streams (grail_limit_stream_*): groups fed chunk by chunk, DESIGN.md §4.17 ---------------------------------------------
// A group's state is the state word of row_kernel_common.h, N counting the samples fed to each member; every member row has
// a ring (there too) of at least 3 L + 19 samples.  Times are absolute (counted from the group's first sample): after N samples the outputs below E(N) =
// max(0, N - (L + 10)) are final, a call that feeds n writes E(N) .. E(N + n) - 1, a finishing call E(N) .. N - 1.  Either
// way the outputs are those of the one-shot kernel for a row of N + n samples: the last one a feeding call writes needs
// q up to N + n - 12 and so samples up to N + n - 1, and a finishing call is the one-shot row's end.
struct LimitStreamGroup {
    uint64_t fed, first;    // N; E(N), the first output this call writes
    uint32_t n, count;      // the samples this call feeds each member, the outputs it writes
    bool takes, refused;    // the call changes the group's state; the members differ in n, or the group has ended and is fed
};
__device__ __forceinline__ LimitStreamGroup limit_stream_group(const uint64_t *__restrict__ state, const uint32_t *__restrict__ in_len,
                                                               uint64_t in_stride, const uint8_t *__restrict__ mark, bool finishing,
                                                               uint64_t grp, uint32_t group, uint32_t L)
{
    LimitStreamGroup r;
    const uint64_t w = state[grp];
    const bool ended = (w & STREAM_ENDED) != 0;
    const uint64_t delay = L + 10u;
    r.fed = w & ~STREAM_ENDED;
    r.first = r.fed > delay ? r.fed - delay : 0u;
    if (finishing) {
        r.n = 0u;
        r.refused = false;
        r.takes = !ended && (!mark || mark[grp]);
        r.count = r.takes ? (uint32_t)(r.fed - r.first) : 0u;              // the tail: min(N, L + 10) outputs
    } else {
        uint64_t n;
        const bool same = limit_group_len(in_len, in_stride, grp * group, group, n);
        r.n = (uint32_t)n;
        r.refused = !same || (ended && n);
        r.takes = !ended && same;
        const uint64_t to = r.fed + n;
        r.count = r.takes ? (uint32_t)((to > delay ? to - delay : 0u) - r.first) : 0u;      // E(N + n) - E(N): at most n
    }
    return r;
}

// A wave-uniform value kept in a vector register from here on.  limit_frames_kernel fills the scalar file (105 of 106, the
// detector's 48 taps among them) and the stream kernel has a dozen uniforms more; with three waves a SIMD there are vector
// registers to spare, and what is only compared against lane values loses nothing there.
template <typename T>
__device__ __forceinline__ T limit_in_vgpr(T x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// limit_detect for a stream (its own copy: limit_frames_kernel pays nothing for it).  Everything is counted from o as there.
// A sample at r lies in the group when lo <= r < hi; below `split` (= N - o, or 0 when o is past N) it comes from the ring,
// from there on from `row` at r - split: row points at the call's sample at max(o, N), n of them follow.  The ring is read in groups of four at (o + r0) mod ring_cap (o, r0 and ring_cap are multiples
// of 4: always inside, always 16-byte aligned); the call's samples by 16-byte loads when VEC and in_vec (N a multiple of 4, so a group
// of four lies on one side of the seam) and by 4-byte loads otherwise, every index clamped into the n samples; no load sits
// behind a divergent branch (n != 0 and in_vec are the group's).
template <bool VEC>
__device__ __forceinline__ void limit_stream_detect(const float *__restrict__ hist, uint32_t o_ring, uint32_t ring_mask,
                                                    const float *__restrict__ row, uint32_t n, bool in_vec, uint32_t blk, uint32_t lo,
                                                    uint32_t hi, uint32_t split, uint32_t lane, double cd, double cq,
                                                    uint32_t own_lo, uint32_t own_hi, bool first, uint32_t sh, uint32_t n_q,
                                                    uint32_t *qv, uint32_t *qe, uint32_t &bad, bool &hot)
{
    const uint32_t r0 = blk * 256u + 4u * lane;
    // all the loads of the block first (the two branches are the group's), then the choice
    float4 old[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) old[q] = *reinterpret_cast<const float4 *>(hist + ((o_ring + r0 + 4u * q) & ring_mask));
    float now[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) now[j] = 0.0f;
    if (n) {
        if (VEC && in_vec) {
            const int32_t last = (int32_t)((n - 1u) & ~3u);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int32_t at = (int32_t)(r0 + 4u * q) - (int32_t)split;
                at = at < 0 ? 0 : at;
                at = at > last ? last : at;
                const float4 v = *reinterpret_cast<const float4 *>(row + at);
                now[4 * q + 0] = v.x, now[4 * q + 1] = v.y, now[4 * q + 2] = v.z, now[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                int32_t at = (int32_t)(r0 + j) - (int32_t)split;
                at = at < 0 ? 0 : at;
                at = at > (int32_t)(n - 1u) ? (int32_t)(n - 1u) : at;
                now[j] = row[at];
            }
        }
    }
    float x[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x[4 * q + 0] = r0 + 4u * q + 0u < split ? old[q].x : now[4 * q + 0];
        x[4 * q + 1] = r0 + 4u * q + 1u < split ? old[q].y : now[4 * q + 1];
        x[4 * q + 2] = r0 + 4u * q + 2u < split ? old[q].z : now[4 * q + 2];
        x[4 * q + 3] = r0 + 4u * q + 3u < split ? old[q].w : now[4 * q + 3];
    }
    double v[16];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const bool inside = r0 + j - lo < hi - lo;
        const bool finite = finite_f32(x[j]);
        // (the lane's own four, and only among the chunk's share of the call's samples: a sample is counted once; what the
        // ring holds is finite)
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
    // the division only in a wave that holds a number above the ceiling
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

// limit_frames_kernel with the group's state in place of the rows' lengths: one workgroup = one (group, chunk of LIMIT_CHUNK of
// this call's outputs).  Reads the state and the rings, writes neither (limit_stream_advance_kernel, queued behind it, is
// their only writer).  Chunk c also counts the non-finite samples among this call's inputs [c LIMIT_CHUNK, (c + 1) LIMIT_CHUNK),
// the last chunk to the end of them; chunk 0 of a group that is fed runs even when the call writes it no output.  VEC: in
// and out are 16-byte aligned and their strides multiples of 4.
template <bool VEC>
__global__ __launch_bounds__(256) void limit_stream_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                           const uint32_t *__restrict__ in_len, uint32_t n_groups, uint32_t group,
                                                           float ceiling, uint32_t ell, const uint64_t *__restrict__ state,
                                                           const float *__restrict__ ring, uint32_t ring_cap,
                                                           const uint8_t *__restrict__ mark, uint32_t finishing, uint32_t grid_chunks,
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
    const uint32_t L = 1u << ell;
    const LimitStreamGroup sg = limit_stream_group(state, in_len, in_stride, mark, finishing != 0u, grp, group, L);
    const uint32_t n = sg.n;
    const uint64_t m0 = (uint64_t)chunk * LIMIT_CHUNK;                       // the chunk's first output, counted in this call's
    // a refused group and one with neither samples nor outputs have no chunk; chunk 0 of any other runs even with no output to
    // write: it counts
    if (sg.refused || (n == 0u && sg.count == 0u) || (m0 >= sg.count && chunk != 0u)) return;
    const bool last = m0 + LIMIT_CHUNK >= sg.count;
    const uint32_t count = m0 >= sg.count ? 0u : (last ? (uint32_t)(sg.count - m0) : LIMIT_CHUNK);
    const uint64_t first_row = (uint64_t)grp * group;
    const uint32_t ring_mask = ring_cap - 1u;

    // the chunk's share of the call's samples, [own_lo, own_hi) of them: the detector counts the non-finite ones among them
    // (its reach ends L + 10 past the chunk's last output: at own_hi); a call that writes no output counts them here
    uint32_t bad = 0u;
    const uint32_t own_lo = m0 < n ? (uint32_t)m0 : n;
    const uint32_t own_hi = last || m0 + LIMIT_CHUNK > n ? n : (uint32_t)(m0 + LIMIT_CHUNK);
    if (count == 0u) {
        for (uint32_t j = 0; j < group; ++j) {
            const float *row = in + (first_row + j) * in_stride;
            for (uint32_t t = own_lo + tid; t < own_hi; t += 256u) bad += finite_f32(row[t]) ? 0u : 1u;
        }
    }

    const uint64_t total = limit_in_vgpr(sg.fed + n);                        // the row as the one-shot kernel would see it
    const uint64_t t0 = limit_in_vgpr(sg.first + m0);
    const uint64_t fed = limit_in_vgpr(sg.fed);
    const uint32_t n_m = count + L - 1u;
    const uint32_t n_q = n_m + L - 1u;
    const int64_t a = (int64_t)t0 - (int64_t)(L - 1u);
    const uint32_t sh = (uint32_t)(a & 3);
    const int64_t o = a - (int64_t)sh - 12;
    bool hot = false;
    if (count) {
        // the group's first sample, or the oldest its rings still hold (no cell that counts reaches below either), from o
        const int64_t oldest = sg.fed > ring_cap ? (int64_t)(sg.fed - ring_cap) : 0;
        const uint32_t lo = limit_in_vgpr(oldest > o ? (uint32_t)(oldest - o) : 0u);        // (oldest < t0 <= o + 16384)
        const int64_t span = (int64_t)total - o;                             // > t0 - o >= lo
        const uint32_t hi = limit_in_vgpr(span < 16384 ? (uint32_t)span : 16384u);
        // the seam between ring and call: sample N lies at N - o, at most 2 L + 24 above o (o >= t0 - L - 14, t0 >= N - L - 10)
        // or, in a later chunk of a long call, below it; then the call's samples are counted from o - N (< n - L - 10)
        const int64_t seam = (int64_t)sg.fed - o;
        const uint32_t split = limit_in_vgpr(seam > 0 ? (uint32_t)seam : 0u);
        const uint64_t skip = seam < 0 ? (uint64_t)(-seam) : 0u;              // (a multiple of 4 when N is)
        const uint32_t n_win = n ? n - (uint32_t)skip : 0u;
        // the chunk's share of the call's samples, counted from o like everything else (N + own_lo - o >= 0: a <= N + m0)
        const uint32_t c_lo = limit_in_vgpr((uint32_t)((int64_t)(sg.fed + own_lo) - o)), c_hi = limit_in_vgpr(c_lo + (own_hi - own_lo));
        const uint32_t o_ring = (uint32_t)((uint64_t)o & ring_mask);
        const uint32_t blocks = (n_q + LIMIT_TAPS_AFTER + sh + 255u) >> 8;
        const double cd = (double)ceiling, cq = cd * 16777216.0;             // (exact)
        const bool in_vec = VEC && (sg.fed & 3u) == 0u;
        // 1, 2: every member's |v| and e, quantised; the group's by minimum
        for (uint32_t j = 0; j < group; ++j) {
            const float *hist = ring + (first_row + j) * ring_cap;
            const float *row = in + (first_row + j) * in_stride + skip;      // (not read when n = 0)
            for (uint32_t blk = wave; blk < blocks; blk += 4u)
                limit_stream_detect<VEC>(hist, o_ring, ring_mask, row, n_win, in_vec, blk, lo, hi, split, lane, cd, cq, c_lo, c_hi, j == 0u, sh,
                                         n_q, cells_a, cells_b, bad, hot);
        }
    }
    // nothing above the ceiling in reach: every q is Q, every sum L Q and every gain 1.0f; the rest is skipped, same bits
    const bool work = __syncthreads_or(hot ? 1 : 0) != 0;
    uint32_t *src = cells_a;
    uint32_t sum_log2 = 0;
    if (work) limit_window_sums(cells_a, cells_b, tid, count, a, (int64_t)total, ell, src, sum_log2);
    // 5: S[t], g, the product, the clamp.  Output t0 + i goes to out[m0 + i]: the stores are 16-byte aligned when VEC; the
    // sample itself comes from the ring (already +0.0 where it was not finite: g * +0.0 is the +0.0 the contract writes) or
    // from the call's samples by 4-byte loads, the seam and the outputs' own offset in time being anywhere.
    const uint32_t pieces = L >> sum_log2, piece = 1u << sum_log2;
    const uint64_t full = (uint64_t)L << 24;
    const double scale = __builtin_ldexp(1.0, -(int)(24u + ell));
    uint64_t maxdef = 0;
    uint32_t limited = 0u;
    for (uint32_t at = 4u * tid; at < count; at += 1024u) {
        float g[4];
        limit_gains(src, work, at, count, pieces, piece, full, scale, g, maxdef, limited);
        const bool whole = at + 4u <= count;
        for (uint32_t j = 0; j < group; ++j) {
            const float *hist = ring + (first_row + j) * ring_cap;
            const float *row = in + (first_row + j) * in_stride;
            float *to = out + (first_row + j) * out_stride + m0 + at;
            float z[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint64_t s = t0 + at + k;
                const float old = hist[(uint32_t)s & ring_mask];
                float now = 0.0f;
                if (n) {
                    int64_t i = (int64_t)s - (int64_t)fed;
                    i = i < 0 ? 0 : i;
                    i = i > (int64_t)(n - 1u) ? (int64_t)(n - 1u) : i;
                    now = row[i];
                }
                const float x = s < fed ? old : now;
                float p = g[k] * x;
                p = p < -ceiling ? -ceiling : p;
                p = p > ceiling ? ceiling : p;
                z[k] = finite_f32(x) ? p : 0.0f;
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
    limit_wave_fold(maxdef, limited, bad);
    limit_chunk_store(maxdef, limited, bad, red, wave, lane, tid, cstat + ((uint64_t)grp * grid_chunks + chunk));
}

// Behind limit_stream_kernel on the stream, one wave per group, the only writer of a stream's state: the group's numbers from
// its chunks, every member's last samples of the call into its ring (ring_keep), then N + n (a finishing call: the group
// ended).  A refused group: refuse_counts and NaN, 0 beside them, its state as it was.  No LDS.
__global__ __launch_bounds__(256) void limit_stream_advance_kernel(const float *__restrict__ in, uint64_t in_stride,
                                                                   const uint32_t *__restrict__ in_len, uint32_t n_groups,
                                                                   uint32_t group, uint32_t ell, uint64_t *__restrict__ state,
                                                                   float *__restrict__ ring, uint32_t ring_cap,
                                                                   const uint8_t *__restrict__ mark, uint32_t finishing,
                                                                   const LimitChunk *__restrict__ cstat, uint32_t grid_chunks,
                                                                   uint32_t *__restrict__ out_len, float *__restrict__ min_gain,
                                                                   uint32_t *__restrict__ n_limited, uint32_t *__restrict__ nonfinite)
{
    const uint64_t grp = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (grp >= n_groups) return;
    const LimitStreamGroup sg = limit_stream_group(state, in_len, in_stride, mark, finishing != 0u, grp, group, 1u << ell);
    if (sg.refused) {
        if (lane == 0u) {
            refuse_counts(out_len, nonfinite, grp);
            if (min_gain) min_gain[grp] = __uint_as_float(0x7FC00000u);
            if (n_limited) n_limited[grp] = 0u;
        }
        return;
    }
    uint64_t maxdef = 0;
    uint32_t limited = 0u, bad = 0u;
    if (sg.takes && (sg.n || sg.count)) {
        const uint32_t chunks = sg.count ? (sg.count + LIMIT_CHUNK - 1u) / LIMIT_CHUNK : 1u;
        for (uint32_t c = lane; c < chunks; c += 64u) {
            const LimitChunk s = cstat[grp * grid_chunks + c];
            maxdef = s.maxdef > maxdef ? s.maxdef : maxdef;
            limited += s.limited;
            bad += s.bad;
        }
        for (uint32_t j = 0; j < group; ++j)
            ring_keep(in + (grp * group + j) * in_stride, sg.n, (uint32_t)sg.fed, ring + (grp * group + j) * ring_cap, ring_cap, ring_cap, lane);
    }
    limit_wave_fold(maxdef, limited, bad);
    if (lane != 0u) return;
    if (out_len) out_len[grp] = sg.count;
    if (min_gain) min_gain[grp] = limit_min_gain(maxdef, ell);
    if (n_limited) n_limited[grp] = limited;
    if (nonfinite) nonfinite[grp] = bad;
    if (sg.takes) state[grp] = finishing ? (sg.fed | STREAM_ENDED) : sg.fed + sg.n;
}

}  // namespace

uint64_t limit_grid_chunks(uint64_t row_stride) { return (row_stride + LIMIT_CHUNK - 1u) / LIMIT_CHUNK; }

size_t limit_chunk_bytes() { return sizeof(LimitChunk); }

hipError_t launch_limit_frames(const LimitArgs &a, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_groups * a.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    launch_either(aligned16(a.rows, a.row_stride, a.out, a.out_stride), limit_frames_kernel<true>, limit_frames_kernel<false>,
                  dim3((uint32_t)workgroups), dim3(256), 0, stream, a.rows, a.row_stride, a.len, a.n_groups, a.group, a.ceiling,
                  a.ell, a.grid_chunks, a.out, a.out_stride, (LimitChunk *)a.cstat);
    return hipGetLastError();
}

hipError_t launch_limit_totals(const LimitArgs &a, hipStream_t stream)
{
    if (a.n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(limit_totals_kernel, dim3((a.n_groups + 255u) / 256u), dim3(256), 0, stream, a.len, a.row_stride, a.n_groups,
                       a.group, a.ell, (const LimitChunk *)a.cstat, a.grid_chunks, a.min_gain, a.n_limited, a.nonfinite);
    return hipGetLastError();
}

hipError_t launch_limit_stream(const LimitArgs &a, hipStream_t stream)
{
    const uint64_t workgroups = (uint64_t)a.n_groups * a.grid_chunks;
    hipError_t e;
    if (!grid_fits(workgroups, &e)) return e;
    launch_either(aligned16(a.rows, a.row_stride, a.out, a.out_stride), limit_stream_kernel<true>, limit_stream_kernel<false>,
                  dim3((uint32_t)workgroups), dim3(256), 0, stream, a.rows, a.row_stride, a.len, a.n_groups, a.group, a.ceiling,
                  a.ell, a.state, a.ring, a.ring_cap, a.mark, a.finishing ? 1u : 0u, a.grid_chunks, a.out, a.out_stride,
                  (LimitChunk *)a.cstat);
    return hipGetLastError();
}

hipError_t launch_limit_stream_advance(const LimitArgs &a, hipStream_t stream)
{
    if (a.n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(limit_stream_advance_kernel, dim3(a.n_groups / 4u + (a.n_groups % 4u != 0u)), dim3(256), 0, stream, a.rows,
                       a.row_stride, a.len, a.n_groups, a.group, a.ell, a.state, a.ring, a.ring_cap, a.mark, a.finishing ? 1u : 0u,
                       (const LimitChunk *)a.cstat, a.grid_chunks, a.out_len, a.min_gain, a.n_limited, a.nonfinite);
    return hipGetLastError();
}

}  // namespace grail
