"""Short-time spectra of rows (include/grail_spectrum.h, the part of the C ABI that has a header of its own): the header's
constants, the signature of every function it declares (SIGNATURES, which tests/test_spectrum_host.py holds to the header as
tests/test_abi.py holds _abi's table to grail_hip.h), the pure-host designers, and the calls on a Context.

A module of its own, reached as grail_hip.spectrum: the package's top-level names, Context's methods and the EXPORTS table are a
recorded listing (tests/golden/binding_surface.txt), and this family adds to none of them.  So what would have been
Context.spectrum_create(...) is spectrum.create(ctx, ...), and so on:

    from grail_hip import spectrum as S
    mel = S.mel_design(48000, 10, 80, 0.0, 24000.0)
    st = S.create(ctx, 10, S.window(S.HANN, 1024), 256, pad=512, bands=mel)
    n_frames, nonfinite = S.transform(ctx, st, rows_dev, stride, len_dev, n_rows, None, bands_dev, frames_stride)
    S.free(ctx, st)
"""
import ctypes as C

import numpy as np

from ._abi import ERR_BUFFER_TOO_SMALL, OK, _also_declares, _arr, _check, _ptr, _sig, load
from .device import _per, _waited

LOG2_MIN, LOG2_MAX = 6, 12       # GRAIL_SPECTRUM_LOG2_MIN / _MAX: a transform has 2^6 .. 2^12 points
BANDS_MAX = 256                  # GRAIL_SPECTRUM_BANDS_MAX: the bands of one set
WEIGHTS_MAX = 65536              # GRAIL_SPECTRUM_WEIGHTS_MAX: the weights of one set's bands together
RECT, HANN, HAMMING = 0, 1, 2    # GRAIL_SPECTRUM_RECT / _HANN / _HAMMING: the kinds grail_spectrum_window knows
CHUNK_FRAMES = 8                 # GRAIL_SPECTRUM_CHUNK_FRAMES: one workgroup's frames (no number depends on it)


def _signatures():
    vp, i32, u32, u64, f64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
    return {
        "grail_spectrum_twiddles": _sig(u32, vp),
        "grail_spectrum_frames": _sig(u64, u32, vp),
        "grail_spectrum_window": _sig(i32, u32, vp),
        "grail_mel_design": _sig(u32, u32, u32, f64, f64, vp, vp, vp, u32, vp),
        "grail_spectrum_create": _sig(vp, u32, vp, u32, u32, u32, u32, vp, vp, vp, vp),
        "grail_spectrum_free": _sig(vp, vp),
        "grail_spectrum_async": _sig(vp, vp, vp, u64, vp, u32, vp, vp, u64, vp, vp),
    }


# function name -> (restype, argtypes) of every symbol include/grail_spectrum.h declares; load() sets them with grail_hip.h's
SIGNATURES = _signatures()
_also_declares(SIGNATURES)


# ---- pure host ------------------------------------------------------------------------------------------------------------------
def twiddles(log2n):
    """grail_spectrum_twiddles (pure host): float64 [N/2][2] = (re, im), the table the transform of N = 2^log2n points reads."""
    table = np.zeros(((1 << int(log2n)) // 2 if 0 <= int(log2n) <= LOG2_MAX else 1, 2), dtype=np.float64)
    _check(load().grail_spectrum_twiddles(log2n, table.ctypes.data))
    return table


def frames(n, hop):
    """grail_spectrum_frames (pure host): ceil(n / hop), the frames of a row of n samples."""
    out = C.c_uint64(0)
    _check(load().grail_spectrum_frames(n, hop, C.addressof(out)))
    return out.value


def window(kind, n_window):
    """grail_spectrum_window (pure host): float32[n_window], the periodic Hann (HANN) or Hamming (HAMMING) window, or ones
    (RECT)."""
    w = np.zeros(max(int(n_window), 1), dtype=np.float32)
    _check(load().grail_spectrum_window(kind, n_window, w.ctypes.data))
    return w


def mel_design(sample_rate, log2n, n_bands, lo_hz, hi_hz):
    """grail_mel_design (pure host): (first uint32[n_bands], count uint32[n_bands], weights float32[sum of the counts]), HTK mel
    triangles over the bins 0 .. N/2 of a transform of N = 2^log2n points at sample_rate, as create takes them."""
    first = np.zeros(max(int(n_bands), 1), dtype=np.uint32)
    count = np.zeros(max(int(n_bands), 1), dtype=np.uint32)
    total = C.c_uint32(0)
    status = load().grail_mel_design(sample_rate, log2n, n_bands, lo_hz, hi_hz, first.ctypes.data, count.ctypes.data, None, 0,
                                    C.addressof(total))
    if status not in (OK, ERR_BUFFER_TOO_SMALL):
        _check(status)
    weights = np.zeros(max(total.value, 1), dtype=np.float32)
    _check(load().grail_mel_design(sample_rate, log2n, n_bands, lo_hz, hi_hz, first.ctypes.data, count.ctypes.data,
                                  weights.ctypes.data, total.value, C.addressof(total)))
    return first[:n_bands], count[:n_bands], weights[:total.value]


# ---- on a Context ---------------------------------------------------------------------------------------------------------------
def create(ctx, log2n, window, hop, pad=0, bands=None):
    """grail_spectrum_create: a set for short-time spectra on ctx's device: a transform of 2^log2n points, a window (float32[W],
    as window() returns it or the caller's own), a hop, a lead of `pad` zeros in front of the first sample, and bands = (first
    uint32[B], count uint32[B], weights float32[sum of the counts]) as mel_design returns them, or None for no bands.  Returns
    the set's handle, for transform / transform_async / free; sets still alive go with the context."""
    win = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
    first, count, weights = (None, None, None) if bands is None else (_arr(bands[0], np.uint32), _arr(bands[1], np.uint32),
                                                                      _arr(bands[2], np.float32))
    n_bands = 0 if first is None else len(first)
    assert count is None or len(count) == n_bands
    out = C.c_void_p(None)
    _check(load().grail_spectrum_create(ctx.handle, log2n, win.ctypes.data, len(win), hop, pad, n_bands, _ptr(first), _ptr(count),
                                       _ptr(weights), C.addressof(out)))
    return out


def free(ctx, spectrum_set):
    """grail_spectrum_free: waits for the context's stream, then releases the set."""
    _check(load().grail_spectrum_free(ctx.handle, spectrum_set))


def transform_async(ctx, spectrum_set, rows_dev, row_stride, len_dev, n_rows, power_dev, bands_dev, frames_stride, n_frames_dev=None,
                    nonfinite_dev=None):
    """grail_spectrum_async: the rows' frames transformed; power_dev: DEVICE float32 [n_rows][frames_stride][N/2 + 1], bands_dev:
    DEVICE float32 [n_rows][frames_stride][B] (either may be None, not both; neither may overlap rows_dev); frames_stride at
    least ceil(row_stride / hop).  Results are DEVICE arrays [n_rows] (either may be None), queued on the context's stream.
    Frames past a row's last are left unwritten."""
    _check(load().grail_spectrum_async(ctx.handle, spectrum_set, rows_dev, row_stride, len_dev, n_rows, power_dev, bands_dev,
                                      frames_stride, n_frames_dev, nonfinite_dev))


def transform(ctx, spectrum_set, rows_dev, row_stride, len_dev, n_rows, power_dev, bands_dev, frames_stride):
    """transform_async, waited for, the results copied back: (n_frames uint32, nonfinite uint32), one per row."""
    return _waited(ctx, _per(n_rows, np.uint32, np.uint32),
                   lambda *d: transform_async(ctx, spectrum_set, rows_dev, row_stride, len_dev, n_rows, power_dev, bands_dev,
                                              frames_stride, *d))
