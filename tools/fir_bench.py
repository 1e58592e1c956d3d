"""FIR filtering at full size, one step per process:
  --step rows   the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB) rendered once, then on the same buffer
                  grail_fir_async with K = 144 (as many multiply-adds per output as 48 000 -> 16 000 resampling has),
                  grail_resample_async 48 000 -> 16 000 (§4.13: one LDS read per multiply-add, coefficients wave-uniform),
                  grail_true_peak_async (§4.11: 48 multiply-adds a sample, nothing written),
                  a plain device-to-device copy of the rows' buffer (what reading and writing the bytes costs);
  --step lone   a lone track of 10^7 samples through K = 32, 255, 1023 and 4096 (time is parallel: it fills the device);
  --step fir    render, then grail_fir_async K = 144 alone (for a counter run).
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
    ap.add_argument("--step", choices=["rows", "lone", "fir"], required=True)
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("fir_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    out = {"step": args.step, "cases": {}}
    if args.step == "lone":
        lone_step(ctx, args, out)
    else:
        rows_step(ctx, args, out, only_fir=args.step == "fir")
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
