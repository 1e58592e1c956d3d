"""Short-time spectra of rendered rows at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2
GB) rendered once, then in one process on the same buffer
  grail_spectrum_async    N = 1 024 (Hann), H = 256, a lead of 512, 80 mel bands, bands only (7.9 GB written),
  grail_true_peak_async   (§4.11: 48 binary64 multiply-adds a sample, nothing written),
  grail_fir_async         with K = 144 (§4.14: 144 multiply-adds an output),
then a lone row of 10^7 samples through grail_spectrum_async.  Wall clock around each call and its sync, best of --reps after
a warm-up.  Binary64 operations a second of the transform: 10 per butterfly of the graph actually computed, which is the full
one: N / 2 * log2 N butterflies a frame.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python
tools/spectrum_bench.py`.  Prints one line per case and a JSON summary.

--breakdown: where the time goes, instead of the above.  --utts rows (8 192 is what DESIGN.md §4.25 quotes) of noise, 96 006
samples at a stride of 96 008, the same set; the call with the mel bands, with 80 empty bands and with 80 bands of one bin in
their place, each with and without the non-finite count; power only; then the other shapes of the kernel, N = 64, 256 and
4 096 at H = N / 4 with one band of one bin."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grail-rs_amd"))

import grail_hip as G                      # noqa: E402
from grail_hip import spectrum as S        # noqa: E402
from grail_hip import workload as W        # noqa: E402

LOG2N, HOP, PAD, BANDS, K_FIR = 10, 256, 512, 80, 144


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def breakdown(ctx, n, reps):
    stride, length = 96008, 96006
    x = (np.random.default_rng(1).standard_normal(n * stride) * 0.1).astype(np.float32)
    d_rows, d_len = ctx.device_alloc(x.nbytes), ctx.device_alloc(n * 4)
    ctx.h2d(d_rows, x, x.nbytes)
    ctx.h2d(d_len, np.full(n, length, np.uint32), n * 4)
    N, bins = 1 << LOG2N, (1 << LOG2N) // 2 + 1
    frames_stride = S.frames(stride, HOP)
    d_bands, d_power = ctx.device_alloc(n * frames_stride * BANDS * 4), ctx.device_alloc(n * frames_stride * bins * 4)
    d_nf, d_bad = ctx.device_alloc(n * 4), ctx.device_alloc(n * 4)
    win = S.window(S.HANN, N)
    mel = S.mel_design(48000, LOG2N, BANDS, 0.0, 24000.0)
    empty = (np.zeros(BANDS, np.uint32), np.zeros(BANDS, np.uint32), np.zeros(0, np.float32))
    one = (np.arange(BANDS, dtype=np.uint32), np.ones(BANDS, np.uint32), np.ones(BANDS, np.float32))
    out = {"rows": n, "samples_per_row": length, "mel_weights": int(mel[1].sum()), "mel_widest_band": int(mel[1].max()), "cases": {}}
    print(f"{n} rows x {length} samples of noise; the mel bands hold {out['mel_weights']} weights, the widest {out['mel_widest_band']} bins")
    for name, bands in (("mel bands", mel), ("80 empty bands", empty), ("80 bands of one bin", one)):
        st = S.create(ctx, LOG2N, win, HOP, PAD, bands)

        def call(count):
            S.transform_async(ctx, st, d_rows, stride, d_len, n, None, d_bands, frames_stride, d_nf, d_bad if count else None)
            ctx.sync()

        with_count, without = best(lambda: call(True), reps)[0], best(lambda: call(False), reps)[0]
        out["cases"][name] = {"ms": with_count, "ms_without_count": without}
        print(f"{name}: bands only {with_count:.2f} ms; without the count {without:.2f} ms")
        S.free(ctx, st)
    st = S.create(ctx, LOG2N, win, HOP, PAD)

    def power_only():
        S.transform_async(ctx, st, d_rows, stride, d_len, n, d_power, None, frames_stride, d_nf, d_bad)
        ctx.sync()

    out["cases"]["power only"] = {"ms": best(power_only, reps)[0]}
    print(f"power only: {out['cases']['power only']['ms']:.2f} ms")
    S.free(ctx, st)
    for p in (6, 8, 12):
        M = 1 << p
        st = S.create(ctx, p, S.window(S.HANN, M), M // 4, M // 2, (np.zeros(1, np.uint32), np.ones(1, np.uint32), np.ones(1, np.float32)))
        fs = S.frames(stride, M // 4)
        rows = min(n, (n * frames_stride * BANDS) // fs)         # (as many as the bands' buffer holds at one number a frame)

        def sized():
            S.transform_async(ctx, st, d_rows, stride, d_len, rows, None, d_bands, fs, d_nf, None)
            ctx.sync()

        ms = best(sized, reps)[0]
        ops = rows * S.frames(length, M // 4) * 10 * (M // 2) * p
        out["cases"][f"p = {p}"] = {"rows": rows, "ms": ms, "binary64_ops_per_s": ops / (ms * 1e-3)}
        print(f"p = {p}, H = N / 4, one band, {rows} rows: {ms:.2f} ms = {ops / (ms * 1e-3) / 1e12:.2f} T binary64 operations a second")
        S.free(ctx, st)
    for ptr in (d_rows, d_len, d_bands, d_power, d_nf, d_bad):
        ctx.device_free(ptr)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lone", type=int, default=10_000_000, help="samples of the lone row (0: skip it)")
    ap.add_argument("--only-spectrum", action="store_true", help="render, then grail_spectrum_async alone (for a counter run)")
    ap.add_argument("--breakdown", action="store_true", help="where the time goes, on --utts rows of noise (see the docstring)")
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("spectrum_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    if args.breakdown:
        breakdown(ctx, args.utts, args.reps)
        ctx.close()
        return
    ctx.set_voices(W.single_voice())
    rate = int(W.SAMPLE_RATE)
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    N = 1 << LOG2N
    frames_stride = S.frames(stride, HOP)
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(max(n, 1) * 4)
    d_bands = ctx.device_alloc(n * frames_stride * BANDS * 4)
    b.synthesize_async(d_rows, stride, d_len)
    ctx.sync()
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    samples = float(lens.astype(np.float64).sum())
    frames = float(np.sum((lens.astype(np.int64) + HOP - 1) // HOP))
    flops_a_frame = 10 * (N // 2) * LOG2N
    print(f"{n} rows x {int(lens.max())} samples = {samples * 4 / 1e9:.2f} GB; {frames:.0f} frames of N = {N} every {HOP}, "
          f"{BANDS} mel bands = {frames * BANDS * 4 / 1e9:.2f} GB written")
    out = {"rows": n, "samples_per_row": int(lens.max()), "samples": samples, "frames": frames, "log2n": LOG2N, "hop": HOP, "bands": BANDS,
           "flops_a_frame": flops_a_frame, "graph": "full", "cases": {}}
    d_nf, d_bad, d_tp = ctx.device_alloc(max(n, 1) * 4), ctx.device_alloc(max(n, 1) * 4), ctx.device_alloc(max(n, 1) * 8)
    mel = S.mel_design(rate, LOG2N, BANDS, 0.0, rate / 2.0)
    spectrum_set = S.create(ctx, LOG2N, S.window(S.HANN, N), HOP, PAD, mel)

    def spectrum():
        S.transform_async(ctx, spectrum_set, d_rows, stride, d_len, n, None, d_bands, frames_stride, d_nf, d_bad)
        ctx.sync()

    ms, ms_all = best(spectrum, args.reps)
    out["cases"]["grail_spectrum_async"] = {"ms": ms, "ms_all": ms_all, "binary64_ops_per_s": frames * flops_a_frame / (ms * 1e-3),
                                            "bytes_read_per_s": samples * 4 / (ms * 1e-3)}
    print(f"grail_spectrum_async, bands only: {ms:.2f} ms (call + sync; all {', '.join('%.2f' % v for v in ms_all)}); "
          f"{frames * flops_a_frame / (ms * 1e-3) / 1e12:.2f} T binary64 operations a second (10 a butterfly, the full graph), "
          f"{samples * 4 / (ms * 1e-3) / 1e12:.2f} TB/s of the rows' bytes")
    if not args.only_spectrum:
        def true_peak():
            ctx.true_peak_async(d_rows, stride, d_len, n, d_tp, d_bad)
            ctx.sync()

        tms, tms_all = best(true_peak, args.reps)
        out["cases"]["grail_true_peak_async"] = {"ms": tms, "ms_all": tms_all}
        print(f"grail_true_peak_async: {tms:.2f} ms; the spectrum call is {ms / tms:.2f} x")
        out_stride = (stride + K_FIR + 63) // 64 * 64
        d_out = ctx.device_alloc(n * out_stride * 4)
        taps = np.concatenate([G.fir_design(rate, 300.0, 3400.0, K_FIR - 1), np.zeros(1, np.float32)])
        fir_set = ctx.fir_create([(taps, (K_FIR - 2) // 2)])

        def fir():
            ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_out, out_stride, d_nf, d_bad)
            ctx.sync()

        fms, fms_all = best(fir, args.reps)
        out["cases"]["grail_fir_async_K144"] = {"ms": fms, "ms_all": fms_all}
        print(f"grail_fir_async K = {K_FIR}: {fms:.2f} ms; the spectrum call is {ms / fms:.2f} x")
        ctx.fir_free(fir_set)
        ctx.device_free(d_out)
    if args.lone:
        long_n = args.lone
        for p in (d_rows, d_bands):
            ctx.device_free(p)
        long_frames = S.frames(long_n, HOP)
        d_rows, d_bands = ctx.device_alloc(long_n * 4), ctx.device_alloc(long_frames * BANDS * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)

        def lone():
            S.transform_async(ctx, spectrum_set, d_rows, long_n, d_len, 1, None, d_bands, long_frames, d_nf, d_bad)
            ctx.sync()

        lms, lms_all = best(lone, args.reps)
        out["lone_row"] = {"samples": long_n, "frames": long_frames, "ms": lms, "ms_all": lms_all,
                           "binary64_ops_per_s": long_frames * flops_a_frame / (lms * 1e-3)}
        print(f"a lone row of {long_n} samples, {long_frames} frames: {lms:.2f} ms = {1e6 * lms / long_n:.2f} ns a sample; "
              f"{long_frames * flops_a_frame / (lms * 1e-3) / 1e12:.2f} T binary64 operations a second")
    S.free(ctx, spectrum_set)
    for p in (d_rows, d_bands, d_len, d_nf, d_bad, d_tp):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
