//! Raw mirror of `include/grail_spectrum.h`: short-time spectra of rows (`grail_spectrum_*`, `grail_mel_design`).  A module
//! of its own as the header is a header of its own; `tests/test_spectrum_host.py` holds it to the header name by name and
//! signature by signature, as `tests/test_abi.py` holds `lib.rs` to `grail_hip.h`.
#![allow(non_camel_case_types)]
use super::grail_ctx;
use std::os::raw::c_int;

#[repr(C)]
pub struct grail_spectrum {
    _private: [u8; 0],
}

/// The transform sizes 2^6 .. 2^12, the most bands and weights of one set (`grail_spectrum_create`), the windows
/// `grail_spectrum_window` knows, and the frames of one workgroup's stretch of a row (no number depends on it).
pub const GRAIL_SPECTRUM_LOG2_MIN: u32 = 6;
pub const GRAIL_SPECTRUM_LOG2_MAX: u32 = 12;
pub const GRAIL_SPECTRUM_BANDS_MAX: u32 = 256;
pub const GRAIL_SPECTRUM_WEIGHTS_MAX: u32 = 65536;
pub const GRAIL_SPECTRUM_RECT: c_int = 0;
pub const GRAIL_SPECTRUM_HANN: c_int = 1;
pub const GRAIL_SPECTRUM_HAMMING: c_int = 2;
pub const GRAIL_SPECTRUM_CHUNK_FRAMES: u32 = 8;

extern "C" {
    pub fn grail_spectrum_twiddles(log2n: u32, re_im: *mut f64) -> c_int;
    pub fn grail_spectrum_frames(n: u64, hop: u32, n_frames: *mut u64) -> c_int;
    pub fn grail_spectrum_window(kind: c_int, n_window: u32, w: *mut f32) -> c_int;
    pub fn grail_mel_design(sample_rate: u32, log2n: u32, n_bands: u32, lo_hz: f64, hi_hz: f64, first: *mut u32,
        count: *mut u32, weights: *mut f32, cap: u32, n_weights: *mut u32) -> c_int;
    pub fn grail_spectrum_create(ctx: *mut grail_ctx, log2n: u32, window: *const f32, n_window: u32, hop: u32, pad: u32,
        n_bands: u32, band_first: *const u32, band_count: *const u32, band_weights: *const f32,
        out: *mut *mut grail_spectrum) -> c_int;
    pub fn grail_spectrum_free(ctx: *mut grail_ctx, set: *mut grail_spectrum) -> c_int;
    pub fn grail_spectrum_async(ctx: *mut grail_ctx, set: *const grail_spectrum, rows_dev: *const f32, row_stride: u64,
        len_dev: *const u32, n_rows: u32, power_dev: *mut f32, bands_dev: *mut f32, frames_stride: u64,
        n_frames_dev: *mut u32, nonfinite_dev: *mut u32) -> c_int;
}
