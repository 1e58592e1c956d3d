"""Dynamics of rendered rows at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB)
rendered once, then in one process on the same buffers
  grail_iir_async   with a filter of S = 2 sections (the yardstick: the same shape of kernel, about the same arithmetic),
  grail_dyn_async   self-keyed (8 B a sample) with a soft-knee compressor on the peak detector,
  grail_dyn_async   keyed (12 B a sample): row u listens to row u + n / 2 of the same buffer, key_len_dev the rows' lengths,
beside the time HBM needs for 8 B a sample at the 6.29 TB/s a float4 copy reaches on an MI355X; then a sweep of row counts (1,
8, 64, 512, 4 096, 65 536 of those rows) through grail_dyn_async (a lane a row) and grail_track_dyn_async (a workgroup a row,
DESIGN.md §4.24) to find where the two cross; then a lone row of 10^7 samples through both (the one-lane figure is the yardstick
of the workgroup form, taken in this same run) beside grail_iir_async S = 2 on the same row, and eight such rows through both.
Wall clock around each call and its sync, best of --reps after a warm-up, with the spread (max - min)
/ min of the repeats.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/dyn_bench.py`.  Prints one
line per case and a JSON summary."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grail-rs_amd"))

import grail_hip as G                      # noqa: E402
from grail_hip import workload as W        # noqa: E402

HBM_BYTES_PER_S = 6.29e12                  # a float4 copy on an MI355X (8.0 TB/s on paper)


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def butterworth(kind, rate, f0, sections):
    return np.array([G.iir_design(kind, rate, f0, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * sections))))
                     for k in range(sections)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lone-reps", type=int, default=None, help="repeats of the rows of --lone samples (default: --reps)")
    ap.add_argument("--no-sweep", action="store_true", help="skip the sweep of row counts")
    ap.add_argument("--lone", type=int, default=10_000_000, help="samples of the lone row (0: skip it)")
    args = ap.parse_args()
    lone_reps = args.reps if args.lone_reps is None else args.lone_reps
    if G.device_count() < 1:
        raise SystemExit("dyn_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    ctx.set_voices(W.single_voice())
    rate = int(W.SAMPLE_RATE)
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(max(n, 8) * 4)       # (eight long rows later)
    d_out = ctx.device_alloc(n * stride * 4)
    b.synthesize_async(d_rows, stride, d_len)
    ctx.sync()
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    samples = float(lens.astype(np.float64).sum())
    hbm_ms = 1e3 * samples * 8 / HBM_BYTES_PER_S
    print(f"{n} rows x {int(lens.max())} samples = {samples * 4 / 1e9:.2f} GB; 8 B a sample at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {hbm_ms:.2f} ms")
    out = {"rows": n, "samples_per_row": int(lens.max()), "samples": samples, "hbm_ms_8B_a_sample": hbm_ms, "cases": {}}
    d_g, d_b, d_n = ctx.device_alloc(max(n, 8) * 8), ctx.device_alloc(max(n, 8) * 4), ctx.device_alloc(max(n, 8) * 4)
    d_key_row = ctx.device_alloc(n * 4)
    ctx.h2d(d_key_row, ((np.arange(n, dtype=np.uint32) + n // 2) % max(n, 1)).astype(np.uint32), n * 4)
    iir_set = ctx.iir_create([butterworth(G.IIR_HIGHPASS, rate, 100.0, 2)])
    curve = (G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -24.0, 3.0, 6.0), G.dyn_ballistics(rate, 5.0, 120.0), G.DYN_PEAK)
    dyn_set = ctx.dyn_create([curve])

    def iir():
        ctx.iir_async(iir_set, d_rows, stride, d_len, n, None, 0, d_out, stride, d_n, d_b)
        ctx.sync()

    def dyn():
        ctx.dyn_async(dyn_set, d_rows, stride, d_len, n, None, d_out, stride, d_n, d_b, d_g)
        ctx.sync()

    def dyn_keyed():
        ctx.dyn_async(dyn_set, d_rows, stride, d_len, n, None, d_out, stride, d_n, d_b, d_g, key_dev=d_rows, key_stride=stride,
                      key_len_dev=d_len, n_keys=n, key_row_dev=d_key_row)
        ctx.sync()

    iir_ms, iir_all = best(iir, args.reps)
    out["cases"]["grail_iir_async_S2"] = {"ms": iir_ms, "ms_all": iir_all, "spread": (max(iir_all) - iir_ms) / iir_ms, "over_hbm": iir_ms / hbm_ms}
    print(f"grail_iir_async S = 2: {iir_ms:.2f} ms (call + sync), spread {100 * (max(iir_all) - iir_ms) / iir_ms:.1f} %; "
          f"{iir_ms / hbm_ms:.2f} x the HBM time of 8 B a sample")
    for name, fn, bytes_a_sample in (("grail_dyn_async", dyn, 8), ("grail_dyn_async_keyed", dyn_keyed, 12)):
        ms, ms_all = best(fn, args.reps)
        spread = (max(ms_all) - ms) / ms
        gains = np.zeros(n, np.float64)
        ctx.d2h(gains, d_g, n * 8)
        out["cases"][name] = {"ms": ms, "ms_all": ms_all, "spread": spread, "over_iir_S2": ms / iir_ms,
                              "over_hbm": ms / (hbm_ms * bytes_a_sample / 8), "smallest_min_gain": float(gains.min())}
        print(f"{name}: {ms:.2f} ms (call + sync), spread {100 * spread:.1f} %; {ms / iir_ms:.2f} x grail_iir_async S = 2, "
              f"{ms / (hbm_ms * bytes_a_sample / 8):.2f} x the HBM time of {bytes_a_sample} B a sample; the smallest min_gain "
              f"{20 * math.log10(max(float(gains.min()), 1e-300)):.2f} dB")
    if not args.no_sweep:
        # the first k of the same rows through both calls: where a lane a row overtakes a workgroup a row
        out["sweep"] = []
        for k in sorted({min(k, n) for k in (1, 8, 64, 512, 4096, 65536)}):
            def lanes():
                ctx.dyn_async(dyn_set, d_rows, stride, d_len, k, None, d_out, stride, d_n, d_b, d_g)
                ctx.sync()

            def groups():
                ctx.track_dyn_async(dyn_set, d_rows, stride, d_len, k, None, d_out, stride, d_n, d_b, d_g)
                ctx.sync()

            lms, lms_all = best(lanes, args.reps)
            gms, gms_all = best(groups, args.reps)
            out["sweep"].append({"rows": k, "dyn_ms": lms, "dyn_ms_all": lms_all, "track_dyn_ms": gms, "track_dyn_ms_all": gms_all})
            print(f"{k} rows: grail_dyn_async {lms:.3f} ms (spread {100 * (max(lms_all) - lms) / lms:.1f} %), grail_track_dyn_async "
                  f"{gms:.3f} ms (spread {100 * (max(gms_all) - gms) / gms:.1f} %): {lms / gms:.2f} x")
    if args.lone:
        long_n = args.lone
        for p in (d_rows, d_out):
            ctx.device_free(p)
        eight = 8
        d_rows, d_out = ctx.device_alloc(eight * long_n * 4), ctx.device_alloc(eight * long_n * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        for r in range(eight):      # (row 0 is the lone row; the others are the same track turned down a little each)
            ctx.h2d(C.c_void_p(d_rows.value + r * long_n * 4), x * np.float32(1.0 - r / 16.0), long_n * 4)
        ctx.h2d(d_len, np.full(eight, long_n, np.uint32), 4 * eight)

        def lone_iir():
            ctx.iir_async(iir_set, d_rows, long_n, d_len, 1, None, 0, d_out, long_n, d_n, d_b)
            ctx.sync()

        def long_dyn(call, rows):
            def run():
                call(dyn_set, d_rows, long_n, d_len, rows, None, d_out, long_n, d_n, d_b, d_g)
                ctx.sync()
            return run

        ims, ims_all = best(lone_iir, lone_reps)
        dms, dms_all = best(long_dyn(ctx.dyn_async, 1), lone_reps)
        tms, tms_all = best(long_dyn(ctx.track_dyn_async, 1), lone_reps)
        d_spread, t_spread = (max(dms_all) - dms) / dms, (max(tms_all) - tms) / tms
        out["lone_row"] = {"samples": long_n, "iir_S2_ms": ims, "iir_S2_ms_all": ims_all, "dyn_ms": dms, "dyn_ms_all": dms_all,
                           "track_dyn_ms": tms, "track_dyn_ms_all": tms_all, "dyn_over_track_dyn": dms / tms}
        print(f"a lone row of {long_n} samples: grail_dyn_async {dms:.1f} ms = {1e6 * dms / long_n:.1f} ns a sample, "
              f"grail_iir_async S = 2 {ims:.1f} ms = {1e6 * ims / long_n:.1f} ns a sample")
        print(f"a lone row of {long_n} samples: grail_track_dyn_async {tms:.1f} ms = {1e6 * tms / long_n:.1f} ns a sample (spread "
              f"{100 * t_spread:.1f} %), grail_dyn_async in this run {dms:.1f} ms (spread {100 * d_spread:.1f} %): {dms / tms:.2f} x")
        d8, d8_all = best(long_dyn(ctx.dyn_async, eight), lone_reps)
        t8, t8_all = best(long_dyn(ctx.track_dyn_async, eight), lone_reps)
        out["eight_rows"] = {"samples": long_n, "dyn_ms": d8, "dyn_ms_all": d8_all, "track_dyn_ms": t8, "track_dyn_ms_all": t8_all}
        print(f"eight rows of {long_n} samples: grail_track_dyn_async {t8:.1f} ms (spread {100 * (max(t8_all) - t8) / t8:.1f} %), "
              f"grail_dyn_async {d8:.1f} ms (spread {100 * (max(d8_all) - d8) / d8:.1f} %): {d8 / t8:.2f} x")
    ctx.dyn_free(dyn_set)
    ctx.iir_free(iir_set)
    for p in (d_g, d_b, d_n, d_key_row, d_rows, d_out, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
