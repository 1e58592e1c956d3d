"""FIR filtering at full size, one step per process:
  --step rows   the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB) rendered once, then on the same buffer
                  grail_fir_async with K = 144 (as many multiply-adds per output as 48 000 -> 16 000 resampling has),
                  grail_resample_async 48 000 -> 16 000 (§4.13: one LDS read per multiply-add, coefficients wave-uniform),
                  grail_true_peak_async (§4.11: 48 multiply-adds a sample, nothing written),
                  a plain device-to-device copy of the rows' buffer (what reading and writing the bytes costs);
  --step lone   a lone track of 10^7 samples through K = 32, 255, 1023 and 4096 (time is parallel: it fills the device);
  --step fir    render, then grail_fir_async K = 144 alone (for a counter run);
  --step stream the config-3 rows through a filter stream in chunks of 4 800 samples (100 ms), K = 144,
                  against grail_fir_async on the same samples in the same process: every chunk is first copied into a
                  buffer of its own (outside the clock: a live stream's pull writes it there), then
                  grail_filter_stream_next_async + sync is timed; the tail by grail_filter_stream_finish_async.  The streamed
                  output is compared with the one-shot output on the device (grail_batch_compare: no row differs).
Wall clock around each call and its sync, best of --reps after a warm-up.  Each step is a process of its own so that each
runs under a time limit of its own and a failure ends the chain:
    timeout -k 10 600 python tools/fir_bench.py --step rows && timeout -k 10 300 python tools/fir_bench.py --step lone
Kernel times: the same chain with `rocprofv3 --kernel-trace --stats -- ` before each `python`; bytes fetched and written:
`rocprofv3 --pmc FETCH_SIZE -- python tools/fir_bench.py --step fir` and the same with WRITE_SIZE (a run of its own each,
no tracing beside them).  Prints one line per case and a JSON summary."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grail-rs_amd"))

import grail_hip as G                      # noqa: E402
from grail_hip import workload as W        # noqa: E402

K_ROWS = 144                               # 48 000 -> 16 000 has P = 144 taps per output
LONE_TAPS = [32, 255, 1023, 4096]


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def taps_of(K):
    """a linear-phase low-pass where K allows one (odd), its even-length neighbour's taps otherwise: the time does not depend
    on the values"""
    h = G.fir_design(48000, 0.0, 8000.0, K if K % 2 else K - 1)
    return (np.r_[h, np.float32(0.0)] if len(h) < K else h), (K - 1) // 2


def rows_step(ctx, args, out, only_fir):
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    out_stride = (stride + K_ROWS + 63) // 64 * 64
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len, d_out = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * out_stride * 4)
    render = []
    for _ in range(3):
        b.synthesize_async(d_rows, stride, d_len)
        ctx.sync()
        render.append(ctx.last_kernel_ms())
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    samples = float(lens.astype(np.float64).sum())
    nbytes = samples * 4
    print(f"render: {n} rows x {int(lens.max())} samples = {nbytes / 1e9:.2f} GB, kernel {min(render[1:]):.2f} ms")
    out.update({"rows": n, "samples_per_row": int(lens.max()), "bytes": nbytes, "render_kernel_ms": min(render[1:])})
    d_ol, d_b, d_tp = ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)

    def report(name, ms, ms_all, extra=""):
        out["cases"][name] = {"ms": ms, "ms_all": ms_all}
        print(f"{name}: {ms:.2f} ms (call + sync), {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s of the rows' bytes{extra}")

    h, origin = taps_of(K_ROWS)
    fir_set = ctx.fir_create([(h, origin)])

    def fir():
        ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_out, out_stride, d_ol, d_b)
        ctx.sync()

    ms, ms_all = best(fir, args.reps)
    fir_fma = (samples + n * (K_ROWS - 1 - origin)) * K_ROWS
    report(f"grail_fir_async K = {K_ROWS}", ms, ms_all, f"; {fir_fma / (ms * 1e-3) / 1e12:.2f} T multiply-adds a second")
    out["fir_fma_per_s"] = fir_fma / (ms * 1e-3)
    if not only_fir:
        def resample():
            ctx.resample_async(d_rows, stride, d_len, n, 48000, 16000, d_out, out_stride, d_ol, d_b)
            ctx.sync()

        ms, ms_all = best(resample, args.reps)
        rs_fma = samples / 3.0 * 144
        report("grail_resample_async 48000->16000", ms, ms_all, f"; {rs_fma / (ms * 1e-3) / 1e12:.2f} T multiply-adds a second")
        out["resample_fma_per_s"] = rs_fma / (ms * 1e-3)

        def true_peak():
            ctx.true_peak_async(d_rows, stride, d_len, n, d_tp, d_b)
            ctx.sync()

        ms, ms_all = best(true_peak, args.reps)
        report("grail_true_peak_async", ms, ms_all, f"; {samples * 48 / (ms * 1e-3) / 1e12:.2f} T multiply-adds a second")
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipDeviceSynchronize.argtypes = []

        def copy():
            rc = hip.hipMemcpy(d_out, d_rows, n * stride * 4, 3)             # hipMemcpyDeviceToDevice
            rc = rc or hip.hipDeviceSynchronize()
            if rc:
                raise SystemExit(f"hipMemcpy failed: {rc}")

        report("device copy", *best(copy, args.reps))
        cases = out["cases"]
        name = f"grail_fir_async K = {K_ROWS}"
        print(f"{name}: {cases[name]['ms'] / cases['grail_resample_async 48000->16000']['ms']:.2f} x the resampler (3 x the outputs), "
              f"{cases[name]['ms'] / cases['grail_true_peak_async']['ms']:.2f} x grail_true_peak_async, "
              f"{cases[name]['ms'] / cases['device copy']['ms']:.2f} x the copy; multiply-adds a second: "
              f"{out['fir_fma_per_s'] / out['resample_fma_per_s']:.2f} x the resampler's")
    ctx.fir_free(fir_set)
    for p in (d_ol, d_b, d_tp, d_rows, d_out, d_len):
        ctx.device_free(p)
    b.free()


def stream_step(ctx, args, out):
    chunk = 4800
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    out_stride = (stride + K_ROWS + 63) // 64 * 64
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4)
    d_out, d_sout = ctx.device_alloc(n * out_stride * 4), ctx.device_alloc(n * out_stride * 4)
    b.synthesize_async(d_rows, stride, d_len)
    ctx.sync()
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    if lens.min() != lens.max():
        raise SystemExit("the stream step wants rows of one length (the aligned corpus): every row's chunk lands at the same offset")
    length = int(lens[0])
    h, origin = taps_of(K_ROWS)
    fir_set = ctx.fir_create([(h, origin)])
    d_ol, d_b, d_sol = ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 4)

    def fir():
        ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_out, out_stride, d_ol, d_b)
        ctx.sync()

    one_shot, one_shot_all = best(fir, args.reps)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    d_chunk, d_clen = ctx.device_alloc(n * chunk * 4), ctx.device_alloc(n * 4)
    calls = -(-length // chunk)
    runs = []
    for _ in range(2):                                   # (the first run warms up)
        fs = ctx.fir_stream_open(fir_set, n)
        ms, written = [], 0
        for c in range(calls):
            k = min(chunk, length - c * chunk)
            rc = hip.hipMemcpy2D(d_chunk, chunk * 4, C.c_void_p(d_rows.value + 4 * c * chunk), stride * 4, k * 4, n, 3)
            if rc:
                raise SystemExit(f"hipMemcpy2D failed: {rc}")
            ctx.h2d(d_clen, np.full(n, k, np.uint32), n * 4)
            t0 = time.perf_counter()
            ctx.fir_stream_next_async(fs, d_chunk, chunk, d_clen, C.c_void_p(d_sout.value + 4 * written), out_stride, d_sol, None)
            ctx.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
            written += G.fir_stream_len(c * chunk, k, K_ROWS, origin)
        t0 = time.perf_counter()
        ctx.fir_stream_finish(fs, n, C.c_void_p(d_sout.value + 4 * written), out_stride, None, d_sol)
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
        ctx.fir_stream_close(fs)
        runs.append(ms)
    max_diff, _, mismatches = ctx.compare(d_sout, d_out, out_stride, d_ol, d_ol, n)
    ms = runs[-1]
    out.update({"rows": n, "samples_per_row": length, "chunk": chunk, "calls": calls, "one_shot_ms": one_shot, "one_shot_ms_all": one_shot_all,
                "stream_ms": sum(ms), "stream_ms_runs": [sum(r) for r in runs], "stream_next_ms_median": float(np.median(ms[:-1])), "stream_finish_ms": ms[-1],
                "mismatches": int(np.count_nonzero((max_diff != 0) | (mismatches != 0)))})
    print(f"grail_fir_async K = {K_ROWS}: {one_shot:.2f} ms; the same rows through a filter stream in {calls} calls of {chunk} samples: "
          f"{sum(ms):.2f} ms = {sum(ms) / one_shot:.2f} x (a call {np.median(ms[:-1]):.3f} ms, finish {ms[-1]:.3f} ms); "
          f"rows that differ from the one-shot output: {out['mismatches']}")
    ctx.fir_free(fir_set)
    for p in (d_ol, d_b, d_sol, d_chunk, d_clen, d_rows, d_out, d_sout, d_len):
        ctx.device_free(p)
    b.free()


def lone_step(ctx, args, out):
    long_n = 10_000_000
    long_out = (long_n + 4096 + 63) // 64 * 64
    d_rows, d_out, d_len = ctx.device_alloc(long_n * 4), ctx.device_alloc(long_out * 4), ctx.device_alloc(4)
    d_ol, d_b = ctx.device_alloc(4), ctx.device_alloc(4)
    x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
    ctx.h2d(d_rows, x, long_n * 4)
    ctx.h2d(d_len, np.array([long_n], np.uint32), 4)
    for K in LONE_TAPS:
        h, origin = taps_of(K)
        fir_set = ctx.fir_create([(h, origin)])

        def fir():
            ctx.fir_async(fir_set, d_rows, long_n, d_len, 1, None, d_out, long_out, d_ol, d_b)
            ctx.sync()

        ms, _ = best(fir, args.reps)
        ctx.fir_free(fir_set)
        fma = (long_n + K - 1 - origin) * K
        out[f"lone_track_1e7_K{K}_ms"] = ms
        print(f"a lone track of {long_n} samples, K = {K}: {ms:.3f} ms = {1e6 * ms / long_n:.3f} ns a sample, "
              f"{fma / (ms * 1e-3) / 1e12:.2f} T multiply-adds a second")
    for p in (d_rows, d_out, d_len, d_ol, d_b):
        ctx.device_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["rows", "lone", "fir", "stream"], required=True)
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("fir_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    out = {"step": args.step, "cases": {}}
    if args.step == "lone":
        lone_step(ctx, args, out)
    elif args.step == "stream":
        stream_step(ctx, args, out)
    else:
        rows_step(ctx, args, out, only_fir=args.step == "fir")
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
