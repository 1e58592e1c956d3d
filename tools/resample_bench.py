"""Sample-rate conversion at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB) rendered
once, then on the same buffer, in the same process,
  grail_resample_async        (one workgroup per row and chunk of 1 024 outputs, one lane per output, P multiply-adds each)
                              for 48 000 -> 16 000 (one phase: the coefficients are wave-uniform), 48 000 -> 44 100 and
                              44 100 -> 48 000 (a phase per lane),
  grail_true_peak_async       (§4.11: 48 multiply-adds a sample, as many as 48 000 -> 16 000 has, nothing written),
  a plain device-to-device copy of the rows' buffer (hipMemcpy: what reading and writing the bytes costs),
and a lone track of 10^7 samples through the same three pairs (time is parallel: it fills the device).  Wall clock around each
call and its sync, best of --reps after a warm-up.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python
tools/resample_bench.py`; bytes fetched and written: under `rocprofv3 --pmc FETCH_SIZE -- python tools/resample_bench.py
--only-resample` and the same with WRITE_SIZE (a run of its own each: the two do not fit one pass).  Prints one line per
case and a JSON summary.
  --step stream   the config-3 rows through a resample stream in 21 calls of 4 800 samples (100 ms), then
                  the tail, for 48 000 -> 16 000 and 44 100 -> 48 000: wall clock around each call and its sync, summed, beside
                  grail_resample_async on the same samples in the same process; the two outputs must be equal in every bit."""
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

PAIRS = [(48000, 16000), (48000, 44100), (44100, 48000)]


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


STREAM_PAIRS = [(48000, 16000), (44100, 48000)]


def stream_step(ctx, args, out):
    chunk = 4800
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    out_stride = (max(G.resample_len(stride, *pair) for pair in STREAM_PAIRS) + 63) // 64 * 64
    chunk_out = (max(max(G.resample_len(chunk, *pair), G.resample_stream_len(2 ** 20, 0, *pair, finishing=True)) for pair in STREAM_PAIRS) + 63) // 64 * 64
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
    d_ol, d_b, d_sol = ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 4)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    d_chunk, d_clen, d_cout = ctx.device_alloc(n * chunk * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * chunk_out * 4)
    calls = -(-length // chunk)
    out.update({"rows": n, "samples_per_row": length, "chunk": chunk, "calls": calls})

    def copy2d(dst, dst_pitch, src, src_pitch, width):
        if width:
            # (a copy between device buffers may return before it is through, and the context's stream does not wait for it)
            rc = hip.hipMemcpy2D(dst, dst_pitch * 4, src, src_pitch * 4, width * 4, n, 3)      # hipMemcpyDeviceToDevice
            rc = rc or hip.hipDeviceSynchronize()
            if rc:
                raise SystemExit(f"hipMemcpy2D failed: {rc}")

    for pair in STREAM_PAIRS:
        def one_shot_call():
            ctx.resample_async(d_rows, stride, d_len, n, pair[0], pair[1], d_out, out_stride, d_ol, d_b)
            ctx.sync()

        one_shot, one_shot_all = best(one_shot_call, args.reps)
        runs = []
        for _ in range(2):                                   # (the first run warms up)
            rs = ctx.resample_stream_open(pair[0], pair[1], n)
            ms, written = [], 0
            for c in range(calls):
                k = min(chunk, length - c * chunk)
                copy2d(d_chunk, chunk, C.c_void_p(d_rows.value + 4 * c * chunk), stride, k)
                ctx.h2d(d_clen, np.full(n, k, np.uint32), n * 4)
                t0 = time.perf_counter()
                ctx.resample_stream_next_async(rs, d_chunk, chunk, d_clen, d_cout, chunk_out, d_sol, None)
                ctx.sync()
                ms.append(1e3 * (time.perf_counter() - t0))
                # (untimed: the call's outputs behind those of the calls before, as a consumer would put them)
                count = G.resample_stream_len(c * chunk, k, *pair)
                copy2d(C.c_void_p(d_sout.value + 4 * written), out_stride, d_cout, chunk_out, count)
                written += count
            t0 = time.perf_counter()
            ctx.resample_stream_finish(rs, n, d_cout, chunk_out, None, d_sol)
            ctx.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
            count = G.resample_stream_len(length, 0, *pair, finishing=True)
            copy2d(C.c_void_p(d_sout.value + 4 * written), out_stride, d_cout, chunk_out, count)
            written += count
            ctx.resample_stream_close(rs)
            runs.append(ms)
        if written != G.resample_len(length, *pair):
            raise SystemExit(f"the stream wrote {written} outputs a row, the one-shot call {G.resample_len(length, *pair)}")
        max_diff, _, mismatches = ctx.compare(d_sout, d_out, out_stride, d_ol, d_ol, n)
        differ = int(np.count_nonzero((max_diff != 0) | (mismatches != 0)))
        ms = runs[-1]
        name = f"{pair[0]}->{pair[1]}"
        out["cases"][name] = {"one_shot_ms": one_shot, "one_shot_ms_all": one_shot_all, "stream_ms": sum(ms),
                              "stream_ms_runs": [sum(r) for r in runs], "stream_next_ms_median": float(np.median(ms[:-1])),
                              "stream_finish_ms": ms[-1], "ratio": sum(ms) / one_shot, "mismatches": differ}
        print(f"grail_resample_async {name}: {one_shot:.2f} ms; the same rows through a resample stream in {calls} calls of {chunk} samples: "
              f"{sum(ms):.2f} ms = {sum(ms) / one_shot:.2f} x (a call {np.median(ms[:-1]):.3f} ms, finish {ms[-1]:.3f} ms); "
              f"rows that differ from the one-shot output: {differ}")
        if differ:
            u = int(np.flatnonzero((max_diff != 0) | (mismatches != 0))[0])
            a, b_ = np.zeros(written, np.float32), np.zeros(written, np.float32)
            ctx.d2h(a, C.c_void_p(d_sout.value + 4 * u * out_stride), written * 4)
            ctx.d2h(b_, C.c_void_p(d_out.value + 4 * u * out_stride), written * 4)
            at = np.flatnonzero(a.view(np.uint32) != b_.view(np.uint32))
            print(f"row {u}: {len(at)} of {written} outputs differ, the first at {at[:8]}: {a[at[:4]]} for {b_[at[:4]]}")
        assert differ == 0, f"{name}: {differ} rows of the stream differ from the one-shot output"
    for p in (d_ol, d_b, d_sol, d_chunk, d_clen, d_cout, d_rows, d_out, d_sout, d_len):
        ctx.device_free(p)
    b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["rows", "stream"], default="rows", help="rows: the one-shot call at full size (the default); "
                    "stream: the same rows through a resample stream, chunk by chunk")
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-resample", action="store_true", help="render, then grail_resample_async 48 000 -> 16 000 alone (for a counter run)")
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("resample_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    if args.step == "stream":
        out = {"step": "stream", "cases": {}}
        stream_step(ctx, args, out)
        ctx.close()
        print(json.dumps(out))
        return
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    out_stride = (max(G.resample_len(stride, *pair) for pair in PAIRS) + 63) // 64 * 64
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
    out = {"rows": n, "samples_per_row": int(lens.max()), "bytes": nbytes, "render_kernel_ms": min(render[1:]), "cases": {}}
    d_ol, d_b, d_tp = ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)

    def report(name, ms, ms_all, extra=""):
        out["cases"][name] = {"ms": ms, "ms_all": ms_all}
        print(f"{name}: {ms:.2f} ms (call + sync), {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s of the rows' bytes{extra}")

    def resample(pair, rows, row_stride, length, n_rows, to, to_stride):
        def run():
            ctx.resample_async(rows, row_stride, length, n_rows, pair[0], pair[1], to, to_stride, d_ol, d_b)
            ctx.sync()
        return run

    def work(pair, n_in):
        U, D, P = G.resample_ratio(*pair)
        fma = n_in * U / D * P
        return U, D, P, fma

    for pair in PAIRS[:1] if args.only_resample else PAIRS:
        ms, ms_all = best(resample(pair, d_rows, stride, d_len, n, d_out, out_stride), args.reps)
        U, D, P, fma = work(pair, samples)
        report(f"grail_resample_async {pair[0]}->{pair[1]}", ms, ms_all,
               f"; U = {U}, D = {D}, P = {P}: {fma / (ms * 1e-3) / 1e12:.2f} T multiply-adds a second")
    if not args.only_resample:
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
        for pair in PAIRS:
            name = f"grail_resample_async {pair[0]}->{pair[1]}"
            print(f"{name}: {cases[name]['ms'] / cases['grail_true_peak_async']['ms']:.2f} x grail_true_peak_async, "
                  f"{cases[name]['ms'] / cases['device copy']['ms']:.2f} x the copy")
        # a lone long track: time is parallel, so it fills the device
        long_n = 10_000_000
        for p in (d_rows, d_out):
            ctx.device_free(p)
        long_out = (max(G.resample_len(long_n, *pair) for pair in PAIRS) + 63) // 64 * 64
        d_rows, d_out = ctx.device_alloc(long_n * 4), ctx.device_alloc(long_out * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)
        for pair in PAIRS:
            ms, _ = best(resample(pair, d_rows, long_n, d_len, 1, d_out, long_out), 5)
            _, _, P, fma = work(pair, long_n)
            out[f"lone_track_1e7_{pair[0]}_{pair[1]}_ms"] = ms
            print(f"a lone track of {long_n} samples, {pair[0]}->{pair[1]}: {ms:.3f} ms = {1e6 * ms / long_n:.3f} ns an input sample, "
                  f"{fma / (ms * 1e-3) / 1e12:.2f} T multiply-adds a second")

        def lone_true_peak():
            ctx.true_peak_async(d_rows, long_n, d_len, 1, d_tp, d_b)
            ctx.sync()

        ms, _ = best(lone_true_peak, 5)
        out["lone_track_1e7_true_peak_ms"] = ms
        print(f"a lone track of {long_n} samples, grail_true_peak_async: {ms:.3f} ms")
    for p in (d_ol, d_b, d_tp, d_rows, d_out, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
