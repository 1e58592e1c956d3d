"""The look-ahead limiter at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB) rendered
once, then on the same buffer, in the same process,
  grail_limit_async           (one workgroup per row and chunk of 4 096 samples: detection, look-ahead, smoothing, apply),
                              at L = 256 with a ceiling nothing reaches (every chunk takes the copy path), with the ceiling
                              at half the median sample peak (most chunks do the whole work), and at L = 1 and L = 1024,
  grail_true_peak_async       (§4.11: the same 48 multiply-adds a sample, no second pass and nothing written),
  a plain device-to-device copy of the rows' buffer (hipMemcpy: what reading and writing the bytes costs),
and a lone track of 10^7 samples (time is parallel: it fills the device).  Wall clock around each call and its sync, best of
--reps after a warm-up.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/limiter_bench.py`; bytes
fetched and written: under `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -- python tools/limiter_bench.py --only-limit` (a run of
its own).  Prints one line per case and a JSON summary.
  --step stream   the same rows through a limit stream in calls of 4 800 samples (100 ms), then finish,
                  beside grail_limit_async on the same rows at the hot ceiling, at L = 256 and L = 1024: the stream's calls
                  summed as a multiple of the one-shot call, the outputs compared on the device."""
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


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def stream_step(ctx, args):
    chunk = 4800
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4)
    d_out, d_sout = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * stride * 4)
    b.synthesize_async(d_rows, stride, d_len)
    ctx.sync()
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    if lens.min() != lens.max():
        raise SystemExit("the stream step wants rows of one length (the aligned corpus): every row's chunk lands at the same offset")
    length = int(lens[0])
    _, peak, _ = ctx.levels(d_rows, stride, d_len, n)
    hot_c = np.float32(np.median(peak[peak > 0]) / 2.0)
    d_g, d_l, d_b, d_sol = (ctx.device_alloc(n * 4) for _ in range(4))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    chunk_out = (max(chunk, G.limit_stream_delay(10)) + 63) // 64 * 64
    d_chunk, d_clen, d_cout = ctx.device_alloc(n * chunk * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * chunk_out * 4)
    calls = -(-length // chunk)
    out = {"step": "stream", "rows": n, "samples_per_row": length, "chunk": chunk, "calls": calls, "ceiling": float(hot_c), "cases": {}}

    def copy2d(dst, dst_pitch, src, src_pitch, width):
        if width:
            # (a copy between device buffers may return before it is through, and the context's stream does not wait for it)
            rc = hip.hipMemcpy2D(dst, dst_pitch * 4, src, src_pitch * 4, width * 4, n, 3)      # hipMemcpyDeviceToDevice
            rc = rc or hip.hipDeviceSynchronize()
            if rc:
                raise SystemExit(f"hipMemcpy2D failed: {rc}")

    for ell in (8, 10):
        def one_shot_call():
            ctx.limit_async(d_rows, stride, d_len, n, hot_c, ell, d_out, stride, 1, d_g, d_l, d_b)
            ctx.sync()

        one_shot, one_shot_all = best(one_shot_call, args.reps)
        runs = []
        for _ in range(2):                                   # (the first run warms up)
            ls = ctx.limit_stream_open(n, hot_c, ell)
            ms, written = [], 0
            for c in range(calls):
                k = min(chunk, length - c * chunk)
                copy2d(d_chunk, chunk, C.c_void_p(d_rows.value + 4 * c * chunk), stride, k)
                ctx.h2d(d_clen, np.full(n, k, np.uint32), n * 4)
                t0 = time.perf_counter()
                ls.next_async(d_chunk, chunk, d_clen, d_cout, chunk_out, d_sol)
                ctx.sync()
                ms.append(1e3 * (time.perf_counter() - t0))
                # (untimed: the call's outputs behind those of the calls before, as a consumer would put them)
                count = G.limit_stream_len(c * chunk, k, ell)
                copy2d(C.c_void_p(d_sout.value + 4 * written), stride, d_cout, chunk_out, count)
                written += count
            t0 = time.perf_counter()
            ls.finish_async(d_cout, chunk_out, None, d_sol)
            ctx.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
            count = G.limit_stream_len(length, 0, ell, finishing=True)
            copy2d(C.c_void_p(d_sout.value + 4 * written), stride, d_cout, chunk_out, count)
            written += count
            ls.close()
            runs.append(ms)
        if written != length:
            raise SystemExit(f"the stream wrote {written} outputs a row, the one-shot call {length}")
        max_diff, _, mismatches = ctx.compare(d_sout, d_out, stride, d_len, d_len, n)
        differ = int(np.count_nonzero((max_diff != 0) | (mismatches != 0)))
        ms = runs[-1]
        name = f"L={1 << ell}"
        out["cases"][name] = {"one_shot_ms": one_shot, "one_shot_ms_all": one_shot_all, "stream_ms": sum(ms),
                              "stream_ms_runs": [sum(r) for r in runs], "stream_next_ms_median": float(np.median(ms[:-1])),
                              "stream_finish_ms": ms[-1], "ratio": sum(ms) / one_shot, "mismatches": differ}
        print(f"grail_limit_async {name} hot: {one_shot:.2f} ms; the same rows through a limit stream in {calls} calls of {chunk} samples: "
              f"{sum(ms):.2f} ms = {sum(ms) / one_shot:.2f} x (a call {np.median(ms[:-1]):.3f} ms, finish {ms[-1]:.3f} ms); "
              f"rows that differ from the one-shot output: {differ}")
        assert differ == 0, f"{name}: {differ} rows of the stream differ from the one-shot output"
    for p in (d_g, d_l, d_b, d_sol, d_chunk, d_clen, d_cout, d_rows, d_out, d_sout, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-limit", action="store_true", help="render, then the hot grail_limit_async case alone (for a counter run)")
    ap.add_argument("--step", choices=["rows", "stream"], default="rows", help="rows: the one-shot call at full size (the default); "
                    "stream: the same rows through a limit stream, chunk by chunk")
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("limiter_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    if args.step == "stream":
        return stream_step(ctx, args)
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len, d_out = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * stride * 4)
    render = []
    for _ in range(3):
        b.synthesize_async(d_rows, stride, d_len)
        ctx.sync()
        render.append(ctx.last_kernel_ms())
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    nbytes = float(lens.astype(np.float64).sum()) * 4
    _, peak, _ = ctx.levels(d_rows, stride, d_len, n)
    hot_c = np.float32(np.median(peak[peak > 0]) / 2.0)
    calm_c = np.float32(4.0 * peak.max())
    print(f"render: {n} rows x {int(lens.max())} samples = {nbytes / 1e9:.2f} GB, kernel {min(render[1:]):.2f} ms; sample peaks up to "
          f"{peak.max():.4f}, median {np.median(peak[peak > 0]):.4f}")
    out = {"rows": n, "samples_per_row": int(lens.max()), "bytes": nbytes, "render_kernel_ms": min(render[1:]), "cases": {}}

    def report(name, ms, ms_all, extra=""):
        out["cases"][name] = {"ms": ms, "ms_all": ms_all}
        print(f"{name}: {ms:.2f} ms (call + sync), {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s of the rows' bytes{extra}")

    d_g, d_l, d_b, d_tp = ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)

    def limit(c, ell):
        def run():
            ctx.limit_async(d_rows, stride, d_len, n, c, ell, d_out, stride, 1, d_g, d_l, d_b)
            ctx.sync()
        return run

    def limited_share():
        counts = np.zeros(n, np.uint32)
        ctx.d2h(counts, d_l, n * 4)
        return f"; {np.count_nonzero(counts)} rows limited, {100.0 * counts.astype(np.float64).sum() * 4 / nbytes:.2f} % of the samples"

    ms, ms_all = best(limit(hot_c, 8), args.reps)
    report("grail_limit_async L=256 hot", ms, ms_all, limited_share())
    if not args.only_limit:
        ms, ms_all = best(limit(calm_c, 8), args.reps)
        report("grail_limit_async L=256 calm", ms, ms_all, limited_share())
        for ell in (0, 10):
            ms, ms_all = best(limit(hot_c, ell), args.reps)
            report(f"grail_limit_async L={1 << ell} hot", ms, ms_all, limited_share())

        def true_peak():
            ctx.true_peak_async(d_rows, stride, d_len, n, d_tp, d_b)
            ctx.sync()

        report("grail_true_peak_async", *best(true_peak, args.reps))
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
        for name in ("grail_limit_async L=256 hot", "grail_limit_async L=256 calm"):
            print(f"{name}: {cases[name]['ms'] / cases['grail_true_peak_async']['ms']:.2f} x grail_true_peak_async, "
                  f"{cases[name]['ms'] / cases['device copy']['ms']:.2f} x the copy")
        # a lone long track: time is parallel, so it fills the device
        long_n = 10_000_000
        for p in (d_rows, d_out):
            ctx.device_free(p)
        d_rows, d_out = ctx.device_alloc(long_n * 4), ctx.device_alloc(long_n * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)
        for name, c in (("hot", np.float32(0.2)), ("calm", np.float32(4.0))):
            def lone():
                ctx.limit_async(d_rows, long_n, d_len, 1, c, 8, d_out, long_n, 1, d_g, d_l, d_b)
                ctx.sync()

            ms, _ = best(lone, 5)
            out[f"lone_track_1e7_{name}_ms"] = ms
            print(f"a lone track of {long_n} samples, L = 256, {name}: {ms:.3f} ms = {1e6 * ms / long_n:.3f} ns a sample")
    for p in (d_g, d_l, d_b, d_tp, d_rows, d_out, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
