/* grail_spectrum.h — short-time spectra of rows on the device: the grail_spectrum_* family and grail_mel_design.
 * A header of its own, which grail_hip.h includes at its end: a program that includes grail_hip.h has all of it.  It is apart
 * because the Python binding's top-level names and its table of grail_hip.h's functions are a recorded listing
 * (tests/golden/binding_surface.txt) that a new family does not move: the family's binding is the module grail_hip.spectrum,
 * its Rust declarations grail-hip-sys/src/spectrum.rs, and tests/test_spectrum_host.py holds both to this file name by name and
 * signature by signature, as tests/test_abi.py holds the rest to grail_hip.h.  Types, statuses and the conventions of every call
 * (what is device memory, what comes before GRAIL_ERR_NO_DEVICE) are grail_hip.h's. */
#ifndef GRAIL_SPECTRUM_H
#define GRAIL_SPECTRUM_H

#include "grail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- levels, continued: short-time spectra ------------------------------------------------------------------------------------------
 * Every stage above works in the time domain.  The first thing a user of rendered rows does with them is turn them into
 * frames of spectral features: a spectrogram to look at, mel energies for a recogniser or a vocoder.  This section does
 * that where the rows lie: windowed frames, a radix-2 transform written down one operation at a time, the power of the
 * bins 0 .. N/2 and weighted sums of it over bands.  A library FFT has no order of additions that a page of numpy could
 * state; this transform has (tests/spectrum_model.py is the page).
 * ARITHMETIC.  All of it IEEE binary64, every operation rounded by itself (no fused multiply-add anywhere), evaluated in
 * the order written; denormals are not flushed.  A row's numbers are a pure function of its samples and the set: not of
 * the strides, alignment, the rows around it, the device or the launch.  No float atomics.
 * SET.  A set holds: the transform size N = 2^p, GRAIL_SPECTRUM_LOG2_MIN = 6 <= p <= GRAIL_SPECTRUM_LOG2_MAX = 12; a window
 * w[0 .. W-1] of binary32 numbers, every one finite, 1 <= W <= N; a hop H >= 1; a lead `pad` of zeros in front of the
 * first sample, 0 <= pad < W; 0 <= B <= GRAIL_SPECTRUM_BANDS_MAX = 256 bands.
 * TWIDDLES.  T[0 .. N/2 - 1], pairs (re, im), as grail_spectrum_twiddles returns them.  With Q = N / 4:
 *   - for j = 0 .. Q: (c, s) = (1, 0) at j = 0, (0, 1) at j = Q, otherwise (cos(2 pi j / N), sin(2 pi j / N)) of the C
 *     library, the argument being ((2 pi) * j) / N with pi the binary64 nearest to it;
 *   - T[j] = (c, 0.0 - s) for 0 <= j <= Q;      T[N/2 - j] = (0.0 - c, 0.0 - s) for 1 <= j < Q.
 * The table as the function returns it is the contract, as with grail_kweighting.  The mirror is deliberate: T[N/2 - j] =
 * -conj(T[j]) exactly, and with it the transform of real input has conjugate symmetry bit for bit (X[N - k] = conj(X[k])
 * up to the sign of a zero, which the power never sees).
 * FRAMES.  For a row of n = min(len[u], row_stride) samples:
 *   - v[t] = (double)x[t] for 0 <= t < n and +0.0 outside; a sample that is not finite (|x| > FLT_MAX or NaN) is counted
 *     once in nonfinite[u] and enters as +0.0; memory between n and row_stride is never read, whatever it holds.
 *   - frame f exists when f * H < n: n_frames[u] = ceil(n / H), 0 for a row of no samples (grail_spectrum_frames).
 *   - a[j] = (double)w[j] * v[f * H - pad + j] for j < W (the product of two binary32 numbers is exact in binary64), and
 *     a[j] = +0.0 for W <= j < N.
 * TRANSFORM.  Radix 2, decimation in time, in place on N complex numbers:
 *   - A[rev_p(j)] = (a[j], +0.0), rev_p the reversal of the p bits of j.
 *   - for s = 1 .. p, with M = 2^s and h = M / 2: for every g a multiple of M below N and every k < h, with w = T[k * N / M],
 *     u = A[g + k], v = A[g + k + h]:
 *         t = ( (v.re * w.re) - (v.im * w.im),  (v.re * w.im) + (v.im * w.re) )
 *         A[g + k] = u + t;      A[g + k + h] = u - t            (component by component)
 * POWER.  P[k] = (A[k].re * A[k].re) + (A[k].im * A[k].im) for k = 0 .. N/2.  power[u][f][k] = (float)P[k], one rounding;
 * it may be infinite and is not counted.
 * BANDS.  Band b has a first bin first[b], a count count[b] and that many binary32 weights, every one finite; first[b] +
 * count[b] <= N/2 + 1 (a count of 0 is an empty band); the counts of one set come to at most GRAIL_SPECTRUM_WEIGHTS_MAX =
 * 65 536.  e = +0.0; for k = 0 .. count[b] - 1 ascending e = e + ((double)wt[b][k] * P[first[b] + k]) (the product rounded,
 * then the sum); bands[u][f][b] = (float)e, one rounding.  The bands read the binary64 P, not the rounded power.
 * All values are finite in binary64 (|a[j]| < 2^256, so P < 2^540), so no NaN is ever produced: every output bit is
 * promised.  Frames at and past n_frames[u] are never written.
 * NO LOGARITHM ON THE DEVICE, as in the dynamics section: the caller has the energies in HBM and takes the logarithm
 * there, with the floor and the base of their own front end.
 * WINDOWS.  grail_spectrum_window: w[j] = (float)(a - (1 - a) * cos(((2 pi) * j) / W)) for j = 0 .. W - 1, the periodic
 * form, a = 0.5 (GRAIL_SPECTRUM_HANN) or 0.54 (GRAIL_SPECTRUM_HAMMING); 1.0f for GRAIL_SPECTRUM_RECT.  The bits of cos are
 * the C library's: the table as returned is the contract.
 * MEL.  grail_mel_design makes B = n_bands triangles on the HTK scale mel(f) = 2595 * log10(1 + f / 700), f(m) = 700 *
 * (pow(10, m / 2595) - 1): with m_lo = mel(lo_hz), m_hi = mel(hi_hz), the B + 2 points p[i] = f(m_lo + ((m_hi - m_lo) * i) /
 * (B + 1)), i = 0 .. B + 1.  Band b has l = p[b], c = p[b + 1], r = p[b + 2]; at the centre f = (k * rate) / N of bin k =
 * 0 .. N/2 its weight is (float)max(0, min((f - l) / (c - l), (r - f) / (r - c))).  first[b] and count[b] delimit the bins
 * whose weight is above 0 (count 0, first 0 for a band that catches no bin); the weights of the bands lie one after another.
 * No area normalisation.  The bits of log10 and pow are the C library's: the tables as returned are the contract.
 * NOT here: the Slaney scale and its area normalisation; reflect padding (pad leads with zeros); phase or complex output; a
 * logarithm; a stream form (frames that straddle two calls). */
#define GRAIL_SPECTRUM_LOG2_MIN 6
#define GRAIL_SPECTRUM_LOG2_MAX 12
#define GRAIL_SPECTRUM_BANDS_MAX 256
#define GRAIL_SPECTRUM_WEIGHTS_MAX 65536
#define GRAIL_SPECTRUM_RECT    0
#define GRAIL_SPECTRUM_HANN    1
#define GRAIL_SPECTRUM_HAMMING 2
/* The frames of one workgroup's stretch of a row.  Not part of the contract (no number depends on it): it is here so that
 * tests can aim at the seams. */
#define GRAIL_SPECTRUM_CHUNK_FRAMES 8
typedef struct grail_spectrum grail_spectrum; /* a transform size, window, hop, lead and bands, resident in HBM */

/* Pure host: re_im[2 j], re_im[2 j + 1] = T[j] of TWIDDLES above, j = 0 .. 2^log2n / 2 - 1.  GRAIL_ERR_INVALID_ARG, nothing
 * written: log2n outside 6 .. 12, re_im NULL. */
int grail_spectrum_twiddles(uint32_t log2n, double *re_im);
/* Pure host: *n_frames = ceil(n / hop), the frames of a row of n samples.  GRAIL_ERR_INVALID_ARG, nothing written: hop 0,
 * n_frames NULL. */
int grail_spectrum_frames(uint64_t n, uint32_t hop, uint64_t *n_frames);
/* Pure host: w[0 .. n_window - 1] of WINDOWS above.  GRAIL_ERR_INVALID_ARG, nothing written: an unknown kind, n_window
 * outside 1 .. 4096, w NULL. */
int grail_spectrum_window(int kind, uint32_t n_window, float *w);
/* Pure host: the triangles of MEL above for a transform of 2^log2n points at sample_rate: first [n_bands], count [n_bands],
 * weights [cap]; *n_weights = the sum of the counts.  GRAIL_ERR_INVALID_ARG, nothing written: a NULL argument, sample_rate
 * 0, log2n outside 6 .. 12, n_bands outside 1 .. 256, not 0 <= lo_hz < hi_hz <= sample_rate / 2, a band so narrow that two
 * of the B + 2 points coincide.  GRAIL_ERR_BUFFER_TOO_SMALL, only *n_weights written: cap below the sum of the counts
 * (weights may then be NULL: the way to ask for the size). */
int grail_mel_design(uint32_t sample_rate, uint32_t log2n, uint32_t n_bands, double lo_hz, double hi_hz, uint32_t *first,
                     uint32_t *count, float *weights, uint32_t cap, uint32_t *n_weights);

/* A set on ctx's device: window [n_window]; band_first, band_count [n_bands]; band_weights: the bands' weights one after
 * another (NULL is fine where there are none).  The set keeps its own copy with its twiddles, uploaded on ctx's stream; the
 * arrays may be reused at once.  GRAIL_ERR_INVALID_ARG, nothing created: out or window NULL; log2n outside 6 .. 12;
 * n_window outside 1 .. 2^log2n; hop 0; pad >= n_window; n_bands above 256; bands without band_first or band_count, weights
 * without band_weights; a band that leaves 0 .. N/2; more than 65 536 weights; a window number or a weight that is not
 * finite.  These come first; without a usable device: GRAIL_ERR_NO_DEVICE. */
int grail_spectrum_create(grail_ctx *ctx, uint32_t log2n, const float *window, uint32_t n_window, uint32_t hop, uint32_t pad,
                          uint32_t n_bands, const uint32_t *band_first, const uint32_t *band_count,
                          const float *band_weights, grail_spectrum **out);
/* Releases a set once everything queued on ctx's stream is through; sets still alive at grail_destroy go with the
 * context.  NULL is a no-op.  GRAIL_ERR_INVALID_ARG: a pointer that is not a live set of this context (another context's, or
 * one freed before: sets are looked up, not looked into). */
int grail_spectrum_free(grail_ctx *ctx, grail_spectrum *set);
/* FRAMES to BANDS above, queued on ctx's stream like grail_fir_async: rows_dev: device [n_rows][row_stride]; len_dev:
 * device [n_rows]; power_dev and bands_dev as below, either may be NULL, not both.  Results are DEVICE arrays [n_rows],
 * either may be NULL: n_frames, nonfinite.  frames_stride must be at least ceil(row_stride / H), the rule of
 * grail_frame_levels_async; frames past a row's last are left unwritten.  Neither output may overlap rows_dev.  16-byte
 * loads where the rows' base is 16-byte aligned and row_stride a multiple of 4, 4-byte ones otherwise: same bits.  One
 * workgroup takes GRAIL_SPECTRUM_CHUNK_FRAMES frames of one row, so a lone long track fills the device.  The scratch (4
 * bytes per row and 8 frames) stays with the context, grown and never shrunk, until grail_destroy.
 * GRAIL_ERR_INVALID_ARG, nothing queued: set NULL or of another context; both outputs NULL; bands_dev with a set of no
 * bands; a NULL buffer with samples to read; frames_stride below ceil(row_stride / H); rows or outputs that span more than
 * 2^60 numbers; output ranges that overlap the rows; more than 2^31 - 1 workgroups.  These come first; without a usable
 * device: GRAIL_ERR_NO_DEVICE.  n_rows = 0 is a success that queues nothing. */
int grail_spectrum_async(grail_ctx *ctx, const grail_spectrum *set, const float *rows_dev, uint64_t row_stride,
                         const uint32_t *len_dev, uint32_t n_rows,
                         float *power_dev,  /* device [n_rows][frames_stride][N/2 + 1] or NULL */
                         float *bands_dev,  /* device [n_rows][frames_stride][B]       or NULL */
                         uint64_t frames_stride, uint32_t *n_frames_dev, uint32_t *nonfinite_dev);

#ifdef __cplusplus
}
#endif
#endif /* GRAIL_SPECTRUM_H */
