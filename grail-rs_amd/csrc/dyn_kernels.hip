// dyn_kernels.hip — dynamics of rows (grail_dyn_async) and of streams (grail_dyn_stream_*).  The contract (include/grail_hip.h,
// "levels, continued: dynamics"): an envelope e that follows |w| or w*w with one alpha on the way up and another on the way
// down, a gain read off the row's curve at e by the bits of e, the sample times the gain; binary64, every operation rounded by
// itself, one rounding to binary32 at the end; no log, exp or pow on the device.  The shape is iir_kernels.hip's: one lane per
// row, 64 rows per wave, tiles of 64 samples in through LDS and out through LDS the other way, and a second tile for the key of
// a keyed call.  The load, the store and the tile are that unit's, copied (DESIGN.md §4.21 says why copies); the table is
// gathered from global memory, a pair of doubles a sample (§4.23 says why not from LDS).  No atomics, every store a plain
// vector store.  DESIGN.md §4.23.
#include "kernels.h"
#include "dyn_plan.h"
#include "loudness_common.h"
#include "row_kernel_common.h"

#include "../../include/grail_hip.h"

#pragma clang fp contract(off)

namespace grail {

using namespace loud;

namespace {

// iir_load of iir_kernels.hip: wave-instruction i reads samples [t0, t0 + 64) of four rows of the wave, lane l the four samples
// from 4 (l mod 16) on of the wave's row 4i + l / 16: whole 256-byte pieces of rows.  MAPPED = false: the wave's row j is row
// row0 + j of rows[n_rows][stride], a row past the last reads the last.  MAPPED = true (the keys): the wave's row j is row
// map[j] of rows, map in LDS and every entry below n_rows.  A group of four past the stride reads the row's last group: every
// load lies inside rows[n_rows][stride] and none sits behind a per-lane branch.  What such a slot holds enters nothing.
// FRESH: the lane index is made opaque at entry, so that the sixteen row addresses are worked out again at every tile and not
// kept in registers from tile to tile (two registers a load and a store: 96 of a keyed kernel's, which took it past 256).
template <bool VEC, bool MAPPED, bool FRESH>
__device__ __forceinline__ void dyn_load(const float *__restrict__ rows, uint64_t stride, uint32_t n_rows, uint64_t row0,
                                         const uint32_t *map, uint64_t t0, uint32_t lane, float (&x)[LOUD_LOADS][4])
{
    if (FRESH) asm volatile("" : "+v"(lane));
    const uint64_t col = t0 + 4u * (lane & 15u);
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        uint64_t r;
        if (MAPPED) {
            r = map[4u * i + (lane >> 4)];
        } else {
            r = row0 + 4u * i + (lane >> 4);
            r = r < n_rows ? r : n_rows - 1u;
        }
        const float *src = rows + r * stride;
        if (VEC) {
            const uint64_t o = col < stride ? col : stride - 4u;                // (stride is a multiple of 4 and >= 4)
            const float4 v = *reinterpret_cast<const float4 *>(src + o);
            x[i][0] = v.x;
            x[i][1] = v.y;
            x[i][2] = v.z;
            x[i][3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint64_t o = col + k < stride ? col + k : stride - 1u;    // (stride >= 1)
                x[i][k] = src[o];
            }
        }
    }
}

// iir_store of iir_kernels.hip: the tile holds the outputs [t0, t0 + 64) of the wave's rows where it held their samples, and
// leaves in the pieces it came in.  row_out[r] is row r's n_out (0 for a row past the launch's last, a refused one and one the
// call writes nothing for): an output at or past it is not stored, so every store lies inside [0, n_out) of a row of the launch.
template <bool VEC, bool FRESH>
__device__ __forceinline__ void dyn_store(const float *tile, const uint32_t *row_out, float *__restrict__ out, uint64_t out_stride,
                                          uint64_t row0, uint64_t t0, uint32_t lane)
{
    if (FRESH) asm volatile("" : "+v"(lane));
    const uint64_t col = t0 + 4u * (lane & 15u);
#pragma unroll
    for (uint32_t i = 0; i < LOUD_LOADS; ++i) {
        const uint32_t rl = 4u * i + (lane >> 4);
        const uint64_t n_out = row_out[rl];
        if (col >= n_out) continue;
        const float *src = tile + rl * LOUD_PITCH + 4u * (lane & 15u);
        float *dst = out + (row0 + rl) * out_stride + col;
        if (VEC && col + 4u <= n_out) {
            float4 v;
            v.x = src[0];
            v.y = src[1];
            v.z = src[2];
            v.w = src[3];
            *reinterpret_cast<float4 *>(dst) = v;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (col + k < n_out) dst[k] = src[k];
        }
    }
}

// what a lane carries along its row
struct DynLane {
    double e;               // the envelope
    double min_gain;
    uint32_t bad;
};

// what a lane reads of its curve: the pairs {G[k], G[k+1] - G[k]}, its two alphas, its detector
struct DynCurve {
    const double2 *table;
    double attack, release;
    bool square;
};

// One sample in the contract's order.  live: t < n (the sample is the row's own); klive: t is inside the row's key.  The
// chain from sample to sample is the compare, the select and e = a + alpha * (e - a); the lookup and the product hang off it.
// A lane past its row's end keeps e and min_gain as they were (a stream's state is the row's, not the wave's).
template <bool KEYED>
__device__ __forceinline__ float dyn_sample(float xf, float kf, bool live, bool klive, const DynCurve &c, DynLane &s)
{
    const bool finite = finite_f32(xf);
    s.bad += (live && !finite) ? 1u : 0u;
    const double v = (live && finite) ? (double)xf : 0.0;
    double w = v;
    if (KEYED) w = (klive && finite_f32(kf)) ? (double)kf : 0.0;
    const double a = c.square ? w * w : __builtin_fabs(w);
    const double alpha = a > s.e ? c.attack : c.release;
    const double e = a + alpha * (s.e - a);
    s.e = live ? e : s.e;
    // curve(e): dyn_index of dyn_plan.cpp on the bits alone.  e is finite and >= +0.0, so its bits order as it does: the
    // exponent field and the mantissa's top four bits, less those of 2^LO, are below 0 for e < 2^LO, 0 .. 639 inside and 640
    // or more from 2^HI on.  The median holds the index inside the table whatever e is.
    const uint64_t bits = (uint64_t)__double_as_longlong(e);
    const int32_t raw = (int32_t)(uint32_t)(bits >> 48) - (int32_t)DYN_KEY_LO;
    const int32_t last = (int32_t)DYN_POINTS - 1;
    const int32_t k = raw < 0 ? 0 : (raw > last ? last : raw);
    const double2 pair = c.table[k];                    // {G[k], G[k+1] - G[k]}
    // m's low 48 bits as the top of a mantissa under the exponent of 1.0: 1 + f, and the subtraction is exact
    const double f = __longlong_as_double((long long)(0x3FF0000000000000ull | ((bits & 0xFFFFFFFFFFFFull) << 4))) - 1.0;
    const double gi = pair.x + f * pair.y;
    const double g = (uint32_t)raw < (uint32_t)last ? gi : pair.x;
    s.min_gain = (live && g < s.min_gain) ? g : s.min_gain;
    return (float)(g * v);
}

// One wave = 64 rows, lane r = row row0 + r, from the rows' first sample to the wave's longest row's last in tiles of 64.  The
// next tile's loads (the key's too) are issued before the current tile is worked through and land in LDS after its outputs
// have left, so they are in flight for the whole of a tile's arithmetic.  A lane's outputs overwrite its own samples in the
// tile, and the tile is stored as it was loaded.  STREAM: e comes from HBM and goes back there.
// The keyed instantiations hold two tiles' loads in flight (128 registers) and work their addresses out afresh at every tile
// (FRESH above); the others keep them from tile to tile as iir_kernel does.  All stay under 256 registers a lane.
template <bool VEC, bool KEYED, bool STREAM>
__global__ __launch_bounds__(64) void dyn_kernel(DynArgs a)
{
    __shared__ float tile[LOUD_ROWS * LOUD_PITCH];
    __shared__ float ktile[KEYED ? LOUD_ROWS * LOUD_PITCH : 1];
    __shared__ uint32_t row_out[LOUD_ROWS];
    __shared__ uint32_t key_of[KEYED ? LOUD_ROWS : 1];
    const uint32_t lane = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * LOUD_ROWS;
    const uint64_t u = row0 + lane;
    const bool mine = u < a.n_rows;
    uint64_t n = 0, n_out = 0, nk = 0, fed = 0;
    uint32_t cu = 0, kr = 0;
    bool refused = false;
    DynLane s = {0.0, __builtin_huge_val(), 0u};        // (min_gain: below every gain; a row of no samples reads 1.0)
    uint64_t *const w = a.state + u * DYN_STREAM_STATE_WORDS;       // (formed into an address that is used by streams only)
    if (mine) {
        cu = a.curve ? a.curve[u] : 0u;
        refused = cu >= a.n_curves;
        if (KEYED) {
            kr = a.key_row ? a.key_row[u] : (uint32_t)u;
            refused = refused || kr >= a.n_keys;
        }
        if (!refused) n = a.len[u] < a.row_stride ? a.len[u] : a.row_stride;       // (never past the row, whatever len holds)
        n_out = n < a.out_stride ? n : a.out_stride;
        if (KEYED && !refused) {
            if (STREAM) {
                nk = n;                                                             // (key_stride >= in_stride: the host)
            } else {
                const uint64_t kl = a.key_len ? a.key_len[kr] : a.key_stride;
                nk = kl < a.key_stride ? kl : a.key_stride;
            }
        }
        if (STREAM) {
            fed = w[0];
            s.e = __longlong_as_double((long long)w[1]);
        }
    }
    // the lane's curve (an index outside the set reads curve 0 and works on nothing)
    const uint32_t cc = cu < a.n_curves ? cu : 0u;
    DynCurve c;
    c.table = reinterpret_cast<const double2 *>(a.image) + (uint64_t)cc * DYN_POINTS;
    c.attack = a.alpha[2u * cc];
    c.release = a.alpha[2u * cc + 1u];
    c.square = a.detector[cc] == GRAIL_DYN_SQUARE;
    row_out[lane] = (uint32_t)n_out;                    // (n_out < 2^32: len is 32 bits wide)
    if (KEYED) key_of[lane] = kr < a.n_keys ? kr : 0u;  // (n_keys >= 1: the host)
    uint64_t longest = n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)longest, d, 64);
        longest = o > longest ? o : longest;
    }
    longest = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(longest >> 32)) << 32) |
              __builtin_amdgcn_readfirstlane((uint32_t)longest);
    const bool key_loads = KEYED && a.key_stride != 0u;         // (uniform; keys of no samples: every w is +0.0, nothing is read)
    float *mine_lds = tile + lane * LOUD_PITCH;
    const float *mine_key = ktile + (KEYED ? lane * LOUD_PITCH : 0u);
    float x[LOUD_LOADS][4];
    float kx[KEYED ? LOUD_LOADS : 1][4];
    __syncthreads();                                    // key_of is there
    if (longest) {
        dyn_load<VEC, false, KEYED>(a.rows, a.row_stride, a.n_rows, row0, nullptr, 0, lane, x);
        loud_stash(tile, lane, x);
        if constexpr (KEYED) {
            if (key_loads) {
                dyn_load<VEC, true, KEYED>(a.key, a.key_stride, a.n_keys, 0, key_of, 0, lane, kx);
                loud_stash(ktile, lane, kx);
            }
        }
    }
    __syncthreads();
    for (uint64_t t0 = 0; t0 < longest; t0 += LOUD_T) {
        const bool more = t0 + LOUD_T < longest;
        if (more) {
            dyn_load<VEC, false, KEYED>(a.rows, a.row_stride, a.n_rows, row0, nullptr, t0 + LOUD_T, lane, x);
            if constexpr (KEYED) {
                if (key_loads) dyn_load<VEC, true, KEYED>(a.key, a.key_stride, a.n_keys, 0, key_of, t0 + LOUD_T, lane, kx);
            }
        }
        const uint32_t run = longest - t0 < LOUD_T ? (uint32_t)(longest - t0) : LOUD_T;       // of the longest row
        constexpr uint32_t UNROLL = 4u;
        uint32_t i = 0;
        for (; i + UNROLL <= run; i += UNROLL) {
            float xs[UNROLL], ks[UNROLL];
#pragma unroll
            for (uint32_t q = 0; q < UNROLL; ++q) {
                xs[q] = mine_lds[i + q];
                ks[q] = KEYED ? mine_key[i + q] : 0.0f;
            }
#pragma unroll
            for (uint32_t q = 0; q < UNROLL; ++q) {
                const uint64_t t = t0 + i + q;
                xs[q] = dyn_sample<KEYED>(xs[q], ks[q], t < n, t < nk, c, s);
            }
#pragma unroll
            for (uint32_t q = 0; q < UNROLL; ++q) mine_lds[i + q] = xs[q];
        }
#pragma unroll 1
        for (; i < run; ++i) {
            const uint64_t t = t0 + i;
            mine_lds[i] = dyn_sample<KEYED>(mine_lds[i], KEYED ? mine_key[i] : 0.0f, t < n, t < nk, c, s);
        }
        __syncthreads();                                // every lane's outputs are in the tile
        dyn_store<VEC, KEYED>(tile, row_out, a.out, a.out_stride, row0, t0, lane);
        __syncthreads();                                // ... and have left it
        if (more) {
            loud_stash(tile, lane, x);
            if constexpr (KEYED) {
                if (key_loads) loud_stash(ktile, lane, kx);
            }
        }
        __syncthreads();
    }
    if (!mine) return;
    if (STREAM) {
        w[1] = (uint64_t)__double_as_longlong(s.e);
        w[0] = fed + n;
    }
    if (a.out_len) a.out_len[u] = refused ? GRAIL_LIMIT_REFUSED : (uint32_t)n_out;
    if (a.nonfinite) a.nonfinite[u] = s.bad;
    if (a.min_gain) a.min_gain[u] = refused ? __longlong_as_double(0x7FF8000000000000ll) : (n ? s.min_gain : 1.0);
}

template <bool KEYED, bool STREAM>
void dyn_launch_vec(const DynArgs &a, bool vec, uint32_t groups, hipStream_t stream)
{
    if (vec)
        hipLaunchKernelGGL((dyn_kernel<true, KEYED, STREAM>), dim3(groups), dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((dyn_kernel<false, KEYED, STREAM>), dim3(groups), dim3(64), 0, stream, a);
}

template <bool STREAM>
void dyn_launch_keyed(const DynArgs &a, bool vec, uint32_t groups, hipStream_t stream)
{
    if (a.key)
        dyn_launch_vec<true, STREAM>(a, vec, groups, stream);
    else
        dyn_launch_vec<false, STREAM>(a, vec, groups, stream);
}

}  // namespace

hipError_t launch_dyn(const DynArgs &args, hipStream_t stream)
{
    if (args.n_rows == 0) return hipSuccess;
    const uint32_t groups = (args.n_rows + LOUD_ROWS - 1u) / LOUD_ROWS;
    const bool vec = aligned16(args.rows, args.row_stride, args.out, args.out_stride) && (!args.key || aligned16(args.key, args.key_stride));
    if (args.state)
        dyn_launch_keyed<true>(args, vec, groups, stream);
    else
        dyn_launch_keyed<false>(args, vec, groups, stream);
    return hipGetLastError();
}

}  // namespace grail
