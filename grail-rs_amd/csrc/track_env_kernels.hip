// track_env_kernels.hip — dynamics of the few long tracks of a mix (grail_track_dyn_async): a workgroup a row.  The contract is
// grail_dyn_async's (include/grail_hip.h, "levels, continued: dynamics", ROW) and so is every bit: each operation of
// dyn_sample (dyn_kernels.hip) is here, in its order, rounded by itself.  What differs is who does it.  Of a sample's work
// only alpha = a > e ? attack : release; e = a + alpha * (e - a) needs the sample before it.  So a row is walked in tiles of
// TRACK_TILE samples, and a tile passes three stages:
//   before the chain: TRACK_WORKERS lanes, four samples each: load, finite test and count, v, w, a = |w| or w * w -> LDS;
//   the chain:        one lane of wave 0, sample after sample: e[t] written over a[t];
//   after the chain:  the same lanes and samples as before it: the index from the bits of e[t], the pair gathered from
//                     global memory, f, the gain, the lane's smallest gain and its time, (float)(g * v) stored.
// Step k does tile k before the chain, tile k - 1 in it and tile k - 2 after it, one barrier a step.  A worker reads e of
// tile k - 2 where it then writes a of tile k, so two tile buffers do.  v waits in the worker's registers for two steps.
// No atomics, no private segment, every store a plain vector store.  DESIGN.md §4.24.
#include "kernels.h"
#include "dyn_plan.h"
#include "row_kernel_common.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

namespace {

// Four samples from column col of a row of `stride` floats.  A group past the stride reads the row's last group, a sample
// past it the row's last sample: every load lies inside the row and none sits behind a per-lane branch.  What such a slot
// holds enters nothing.
template <bool VEC>
__device__ __forceinline__ void track_load(const float *__restrict__ row, uint64_t stride, uint64_t col, float (&x)[4])
{
    if (VEC) {
        const uint64_t o = col < stride ? col : stride - 4u;                    // (stride is a multiple of 4 and >= 4)
        const float4 v = *reinterpret_cast<const float4 *>(row + o);
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t o = col + k < stride ? col + k : stride - 1u;        // (stride >= 1)
            x[k] = row[o];
        }
    }
}

// The chain over the first `run` samples of a tile: a[t] in, e[t] out in its place.  One lane.  Sixteen samples a turn in two
// halves: a half's a[t] are read while the other half is worked through, so no read waits on the chain and the chain on no
// read but the first.  (The second half's look-ahead wraps at the tile's end and reads what nobody uses.)
__device__ __forceinline__ double track_chain(double *buf, uint32_t run, double e, double attack, double release)
{
    constexpr uint32_t H = 8;
    double lo[H], hi[H];
    uint32_t i = 0;
#pragma unroll
    for (uint32_t q = 0; q < H; ++q) lo[q] = buf[q];
    for (; i + 2u * H <= run; i += 2u * H) {
#pragma unroll
        for (uint32_t q = 0; q < H; ++q) hi[q] = buf[i + H + q];
#pragma unroll
        for (uint32_t q = 0; q < H; ++q) {
            const double a = lo[q];
            const double alpha = a > e ? attack : release;
            e = a + alpha * (e - a);
            buf[i + q] = e;
        }
#pragma unroll
        for (uint32_t q = 0; q < H; ++q) lo[q] = buf[(i + 2u * H + q) & (TRACK_TILE - 1u)];
#pragma unroll
        for (uint32_t q = 0; q < H; ++q) {
            const double a = hi[q];
            const double alpha = a > e ? attack : release;
            e = a + alpha * (e - a);
            buf[i + H + q] = e;
        }
    }
#pragma unroll 1
    for (; i < run; ++i) {
        const double a = buf[i];
        const double alpha = a > e ? attack : release;
        e = a + alpha * (e - a);
        buf[i] = e;
    }
    return e;
}

// of two (gain, first time) pairs the smaller gain, and of gains that compare equal the earlier time: the winner's bits
__device__ __forceinline__ void track_smaller(double &g, uint32_t &t, double og, uint32_t ot)
{
    const bool take = og < g || (og == g && ot < t);
    g = take ? og : g;
    t = take ? ot : t;
}

template <bool VEC, bool KEYED>
__global__ __launch_bounds__(TRACK_THREADS) void track_env_kernel(DynArgs a)
{
    __shared__ double buf[2][TRACK_TILE];
    __shared__ double red_gain[TRACK_WORKERS];
    __shared__ uint32_t red_time[TRACK_WORKERS];
    __shared__ uint32_t red_bad[TRACK_WORKERS];
    const uint32_t tid = threadIdx.x;
    const bool worker = tid >= 64u;
    const uint32_t col = worker ? 4u * (tid - 64u) : 0u;        // the worker's four samples of every tile
    const uint64_t u = blockIdx.x;
    // the row: the same for every lane
    const uint32_t cu = a.curve ? a.curve[u] : 0u;
    bool refused = cu >= a.n_curves;
    uint32_t kr = 0;
    if (KEYED) {
        kr = a.key_row ? a.key_row[u] : (uint32_t)u;
        refused = refused || kr >= a.n_keys;
    }
    uint64_t n = 0, nk = 0;
    if (!refused) n = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;           // (never past the row, whatever len holds)
    const uint64_t n_out = n < a.out_stride ? n : a.out_stride;
    if (KEYED && !refused) {
        const uint64_t kl = a.key_len ? a.key_len[kr] : a.key_stride;
        nk = kl < a.key_stride ? kl : a.key_stride;
    }
    // the row's curve (an index outside the set reads curve 0 and works on nothing)
    const uint32_t cc = cu < a.n_curves ? cu : 0u;
    const double2 *const table = reinterpret_cast<const double2 *>(a.image) + (uint64_t)cc * DYN_POINTS;
    const double attack = a.alpha[2u * cc];
    const double release = a.alpha[2u * cc + 1u];
    const bool square = a.detector[cc] == GRAIL_DYN_SQUARE;
    const float *const row = a.rows + u * a.row_stride;
    const float *const key = KEYED ? a.key + (uint64_t)(kr < a.n_keys ? kr : 0u) * a.key_stride : nullptr;    // (n_keys >= 1: the host)
    const bool key_loads = KEYED && a.key_stride != 0u;         // (keys of no samples: every w is +0.0, nothing is read)
    float *const out_row = a.out + u * a.out_stride;            // (formed into an address that is used for n_out > 0 only)

    const uint64_t tiles = (n + TRACK_TILE - 1u) / TRACK_TILE;
    double e = 0.0;                                             // the chain lane's
    double mg = __builtin_huge_val();                           // a worker's smallest gain (below every gain) ...
    uint32_t mt = 0xFFFFFFFFu;                                  // ... and when it first saw it
    uint32_t bad = 0;
    float v_cur[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v_prev[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint64_t steps = tiles ? tiles + 2u : 0u;
    for (uint64_t k = 0; k < steps; ++k) {
        double *const mine = buf[k & 1u];                       // tile k - 2 leaves it, tile k enters it
        if (worker) {
            const bool before = k < tiles, after = k >= 2u;
            const uint64_t t_in = k * TRACK_TILE + col;
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, kx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (before) {
                track_load<VEC>(row, a.row_stride, t_in, x);
                if constexpr (KEYED) {
                    if (key_loads) track_load<VEC>(key, a.key_stride, t_in, kx);
                }
            }
            if (after) {
                // dyn_sample from the bits of e on: dyn_index of dyn_plan.cpp on the bits alone, the median holds the index
                // inside the table whatever e is (a slot past the row's end holds its a, and counts for nothing)
                const uint64_t t_out = (k - 2u) * TRACK_TILE + col;
                float y[4];
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint64_t bits = (uint64_t)__double_as_longlong(mine[col + q]);
                    const int32_t raw = (int32_t)(uint32_t)(bits >> 48) - (int32_t)DYN_KEY_LO;
                    const int32_t last = (int32_t)DYN_POINTS - 1;
                    const int32_t ki = raw < 0 ? 0 : (raw > last ? last : raw);
                    const double2 pair = table[ki];             // {G[k], G[k+1] - G[k]}
                    const double f = __longlong_as_double((long long)(0x3FF0000000000000ull | ((bits & 0xFFFFFFFFFFFFull) << 4))) - 1.0;
                    const double gi = pair.x + f * pair.y;
                    const double g = (uint32_t)raw < (uint32_t)last ? gi : pair.x;
                    const bool smaller = t_out + q < n && g < mg;
                    mg = smaller ? g : mg;
                    mt = smaller ? (uint32_t)(t_out + q) : mt;  // (t < n < 2^32: len is 32 bits wide)
                    y[q] = (float)(g * (double)v_prev[q]);
                }
                if (t_out < n_out) {
                    float *dst = out_row + t_out;
                    if (VEC && t_out + 4u <= n_out) {
                        float4 o;
                        o.x = y[0];
                        o.y = y[1];
                        o.z = y[2];
                        o.w = y[3];
                        *reinterpret_cast<float4 *>(dst) = o;
                    } else {
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q)
                            if (t_out + q < n_out) dst[q] = y[q];
                    }
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) v_prev[q] = v_cur[q];
            if (before) {
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const bool live = t_in + q < n;
                    const bool finite = finite_f32(x[q]);
                    bad += (live && !finite) ? 1u : 0u;
                    v_cur[q] = (live && finite) ? x[q] : 0.0f;  // (v = (double)v_cur, exact, when the gain is there)
                    double w = (double)v_cur[q];
                    if (KEYED) w = (t_in + q < nk && finite_f32(kx[q])) ? (double)kx[q] : 0.0;
                    mine[col + q] = square ? w * w : __builtin_fabs(w);
                }
            }
        } else if (tid == 0u && k >= 1u && k <= tiles) {
            const uint64_t t0 = (k - 1u) * TRACK_TILE;
            const uint32_t run = n - t0 < TRACK_TILE ? (uint32_t)(n - t0) : TRACK_TILE;
            e = track_chain(buf[(k - 1u) & 1u], run, e, attack, release);
        }
        __syncthreads();
    }
    // the row's end: the workers' counts and pairs through LDS to wave 0
    if (worker) {
        red_gain[tid - 64u] = mg;
        red_time[tid - 64u] = mt;
        red_bad[tid - 64u] = bad;
    }
    __syncthreads();
    if (tid >= 64u) return;
    mg = red_gain[tid], mt = red_time[tid], bad = red_bad[tid];
#pragma unroll
    for (uint32_t j = 64u; j < TRACK_WORKERS; j += 64u) {
        track_smaller(mg, mt, red_gain[tid + j], red_time[tid + j]);
        bad += red_bad[tid + j];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double og = __longlong_as_double(__shfl_xor(__double_as_longlong(mg), d, 64));
        const uint32_t ot = (uint32_t)__shfl_xor((int)mt, d, 64);
        track_smaller(mg, mt, og, ot);
    }
    bad = wave_sum(bad);
    if (tid != 0u) return;
    if (a.out_len) a.out_len[u] = refused ? GRAIL_LIMIT_REFUSED : (uint32_t)n_out;
    if (a.nonfinite) a.nonfinite[u] = bad;
    if (a.min_gain) a.min_gain[u] = refused ? __longlong_as_double(0x7FF8000000000000ll) : (n ? mg : 1.0);
}

template <bool KEYED>
void track_launch_vec(const DynArgs &a, bool vec, hipStream_t stream)
{
    if (vec)
        hipLaunchKernelGGL((track_env_kernel<true, KEYED>), dim3(a.n_rows), dim3(TRACK_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((track_env_kernel<false, KEYED>), dim3(a.n_rows), dim3(TRACK_THREADS), 0, stream, a);
}

}  // namespace

hipError_t launch_track_dyn(const DynArgs &args, hipStream_t stream)
{
    hipError_t e;
    if (!grid_fits(args.n_rows, &e)) return e;
    const bool vec = aligned16(args.rows, args.row_stride, args.out, args.out_stride) && (!args.key || aligned16(args.key, args.key_stride));
    if (args.key)
        track_launch_vec<true>(args, vec, stream);
    else
        track_launch_vec<false>(args, vec, stream);
    return hipGetLastError();
}

}  // namespace grail
