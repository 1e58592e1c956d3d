// dyn_plan.h — what the pure-host side of dynamics (dyn_plan.cpp) shares with transforms.cpp, transform_streams.cpp and
// dyn_kernels.hip.  No HIP type: it builds with g++ (tests/test_dyn_sanitize.py).
#pragma once

#include <cstdint>
#include <vector>

namespace grail {

constexpr uint32_t DYN_POINTS = 641;        // == GRAIL_DYN_POINTS
constexpr uint32_t DYN_STEPS = 16;          // == GRAIL_DYN_STEPS_PER_OCTAVE
constexpr int32_t DYN_LOG2_LO = -32;        // == GRAIL_DYN_LOG2_LO
constexpr int32_t DYN_LOG2_HI = 8;          // == GRAIL_DYN_LOG2_HI
// One curve of a set as the kernel reads it: DYN_POINTS pairs {G[k], G[k+1] - G[k]} (the last pair's difference +0.0), so that
// the two table words of a sample are one 16-byte gather.  The difference is the contract's own subtraction, rounded once,
// whoever does it.
constexpr uint32_t DYN_IMAGE_DOUBLES = 2 * DYN_POINTS;
// (bits of e) >> 48 of e = 2^LO: the exponent field times 16 plus the mantissa's top four bits; k = that of e minus this
constexpr uint32_t DYN_KEY_LO = (uint32_t)(1023 + DYN_LOG2_LO) * DYN_STEPS;
// a stream's state words a row: N, then e as its bits
constexpr uint32_t DYN_STREAM_STATE_WORDS = 2;
// grail_track_dyn_async (track_env_kernels.hip): a workgroup walks its row in tiles of TRACK_TILE samples, a power of two.  Not
// part of the contract: no number depends on it.  One wave runs the envelope's chain; each of the TRACK_TILE / 4 other lanes
// takes four samples of a tile on either side of the chain.
constexpr uint32_t TRACK_TILE = 1024;
constexpr uint32_t TRACK_WORKERS = TRACK_TILE / 4;
constexpr uint32_t TRACK_THREADS = 64 + TRACK_WORKERS;

// lev[k] = 2^(LO + k div 16) * (1 + (k mod 16) / 16), exact; k < DYN_POINTS
double dyn_level(uint32_t k);
// The lookup's index arithmetic for e finite and >= +0.0: *k in 0 .. 640 and *f in [0, 1), with *inside false where e is
// below 2^LO (k = 0) or at or above 2^HI (k = 640) and the result is G[k] alone.  The kernel gets the same three cases
// from the bits alone (dyn_kernels.hip).
void dyn_index(double e, uint32_t *k, double *f, bool *inside);
// curve(e) of the contract on one curve G[DYN_POINTS]
double dyn_lookup(const double *gain, double e);

// NULL when (gain, alpha, detector, n_curves) is a set grail_dyn_create takes, else what is wrong with it
const char *dyn_set_error(const double *gain, const double *alpha, const uint32_t *detector, uint32_t n_curves);
// the device image of a checked set: image[DYN_IMAGE_DOUBLES * c ..]: curve c
void dyn_set_image(const double *gain, uint32_t n_curves, std::vector<double> &image);

// NULL when a call of grail_dyn_async may be queued, else what is wrong with its arguments (addresses are compared, never
// looked behind)
const char *dyn_call_error(const void *rows, uint64_t row_stride, const void *len, uint32_t n_rows, const void *key,
                           uint64_t key_stride, uint32_t n_keys, const void *key_row, const void *out, uint64_t out_stride);

// Streams (grail_dyn_stream_*).  NULL when curve (host [n_rows], or NULL = curve 0) and key_row (host [n_rows], or NULL = row u
// to key u; not read for n_keys = 0) bind n_rows >= 1 rows to curves of a set of n_curves and to keys below n_keys
const char *dyn_stream_open_error(const uint32_t *curve, uint32_t n_rows, uint32_t n_curves, uint32_t n_keys, const uint32_t *key_row);
// NULL when a call of grail_dyn_stream_next_async may be queued on a stream that is keyed or not (n_keys; 0: self-keyed)
const char *dyn_stream_next_error(const void *in, uint64_t in_stride, const void *in_len, uint32_t n_rows, bool keyed,
                                  uint32_t n_keys, const void *key, uint64_t key_stride, const void *out, uint64_t out_stride);

}  // namespace grail
