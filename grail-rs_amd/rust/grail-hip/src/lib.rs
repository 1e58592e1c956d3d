//! `utterances.synthesize_batch(&gpu)` / `utterances.synthesize_batch(&node)` — the batched counterpart of grail-rs's
//! `.select(v).sequence(v).jitter(seed, v).synthesize()` (reference src/lib.rs:1013, 941, 786,
//! 587; trait pattern of `IntoSynthesize`, src/lib.rs:582-600).  Per-utterance results are
//! bit-identical to the CPU iterator chain.  SOURCE ONLY: not compiled in the build image.
use grail_hip_sys as sys;
use grail_rs::{PhonemeElem, Voice};
use std::ffi::CStr;

#[derive(Debug)]
pub struct Error {
    pub status: i32,
    pub message: String,
}

fn check(status: i32) -> Result<(), Error> {
    if status == sys::GRAIL_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(sys::grail_last_error()) }.to_string_lossy().into_owned();
    Err(Error { status, message })
}

/// One GPU + a voice table (grail_ctx).
pub struct Gpu {
    ctx: *mut sys::grail_ctx,
}

// grail-rs keeps its struct layouts private to Rust; convert field by field.  `Array` needs a
// `pub fn to_array(self) -> [f32; NUM_FORMANTS]` accessor in grail-rs (one line).
fn elem_to_c(e: &grail_rs::SynthesisElem) -> sys::grail_synthesis_elem {
    sys::grail_synthesis_elem {
        frequency: e.frequency,
        formant_freq: e.formant_freq.to_array(),
        formant_bw: e.formant_bw.to_array(),
        formant_smooth: e.formant_smooth.to_array(),
        formant_breath: e.formant_breath.to_array(),
        formant_turb: e.formant_turb.to_array(),
        formant_amp: e.formant_amp.to_array(),
    }
}

fn voice_to_c(v: &Voice) -> sys::grail_voice {
    sys::grail_voice {
        sample_rate: v.sample_rate,
        phonemes: [elem_to_c(&v.phonemes.a), elem_to_c(&v.phonemes.e)],
        center_frequency: v.center_frequency,
        jitter_frequency: v.jitter_frequency,
        jitter_delta_frequency: v.jitter_delta_frequency,
        jitter_delta_formant_frequency: v.jitter_delta_formant_frequency,
        jitter_delta_amplitude: v.jitter_delta_amplitude,
    }
}

impl Gpu {
    pub fn new(device: i32, voices: &[Voice]) -> Result<Self, Error> {
        // the library on the loader's path may be older or newer than the header this crate mirrors
        let have = unsafe { sys::grail_abi_version() };
        if have != sys::GRAIL_ABI_VERSION {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG,
                               message: format!("libgrail_hip.so has ABI version {have}, grail-hip-sys mirrors {}", sys::GRAIL_ABI_VERSION) });
        }
        let mut ctx = std::ptr::null_mut();
        check(unsafe { sys::grail_create(device, &mut ctx) })?;
        let gpu = Gpu { ctx };
        let table: Vec<_> = voices.iter().map(voice_to_c).collect();
        check(unsafe { sys::grail_set_voices(gpu.ctx, table.as_ptr(), table.len() as u32) })?;
        Ok(gpu)
    }
}

impl Drop for Gpu {
    fn drop(&mut self) {
        unsafe { sys::grail_destroy(self.ctx) };
    }
}

pub struct Utterance {
    pub phonemes: Vec<PhonemeElem>,
    pub voice: u32,
    pub jitter_seed: u32,
}

/// A batch in the flat form the C ABI takes (`grail_synthesize_batch`): utterance u is
/// `segs[offs[u]..offs[u + 1]]` with voice `vids[u]` and jitter seed `seeds[u]`.
pub struct FlatBatch {
    segs: Vec<sys::grail_phoneme_elem>,
    offs: Vec<u32>,
    vids: Vec<u32>,
    seeds: Vec<u32>,
}

impl FlatBatch {
    fn new<I: IntoIterator<Item = Utterance>>(utterances: I) -> Self {
        let mut b = FlatBatch { segs: vec![], offs: vec![0u32], vids: vec![], seeds: vec![] };
        for u in utterances {
            b.segs.extend(u.phonemes.iter().map(|p| sys::grail_phoneme_elem {
                phoneme: p.phoneme as i32, // Silence=0 Stop=1 Glide=2 A=3 E=4 (src/lib.rs:632-649)
                length: p.length,
                blend_length: p.blend_length,
                frequency: p.frequency,
            }));
            b.offs.push(b.segs.len() as u32);
            b.vids.push(u.voice);
            b.seeds.push(u.jitter_seed);
        }
        b
    }

    pub fn len(&self) -> u32 {
        self.vids.len() as u32
    }
}

/// What a batch can be rendered on: one GPU ([`Gpu`]) or every GPU of the node ([`Node`]).
pub trait SynthesisTarget {
    fn render(&self, batch: &FlatBatch) -> Result<Vec<Vec<f32>>, Error>;
}

/// `utterances.synthesize_batch(&gpu)` / `utterances.synthesize_batch(&node)`: the batched counterpart of
/// `IntoSynthesize` (src/lib.rs:582-600).
pub trait IntoSynthesizeBatch {
    fn synthesize_batch<T: SynthesisTarget>(self, target: &T) -> Result<Vec<Vec<f32>>, Error>;
}

impl<I: IntoIterator<Item = Utterance>> IntoSynthesizeBatch for I {
    fn synthesize_batch<T: SynthesisTarget>(self, target: &T) -> Result<Vec<Vec<f32>>, Error> {
        target.render(&FlatBatch::new(self))
    }
}

fn rows_of(out: &[f32], stride: usize, lens: &[u32]) -> Vec<Vec<f32>> {
    lens.iter().enumerate().map(|(u, &l)| out[u * stride..][..l as usize].to_vec()).collect()
}

impl SynthesisTarget for Gpu {
    fn render(&self, b: &FlatBatch) -> Result<Vec<Vec<f32>>, Error> {
        let gpu = self;
        let n = b.len();
        let mut lens = vec![0u32; n as usize];
        unsafe {
            let mut h = std::ptr::null_mut();
            check(sys::grail_batch_upload(gpu.ctx, b.segs.as_ptr(), b.offs.as_ptr(), b.vids.as_ptr(),
                                          b.seeds.as_ptr(), n, &mut h))?;
            let r = check(sys::grail_batch_lengths(gpu.ctx, h, u32::MAX, lens.as_mut_ptr()));
            sys::grail_batch_free(gpu.ctx, h);
            r?;
        }
        let stride = (*lens.iter().max().unwrap_or(&0) as u64 + 63) / 64 * 64;
        // Results of up to PINNED_LIMIT bytes land in PINNED host memory: grail_synthesize_batch renders rows in
        // blocks of up to 4096 utterances and copies each block out on a second stream while the next one
        // renders; a pinned destination receives those copies directly (measured 53 GB/s end to end = 93 %
        // of a plain pinned hipMemcpy, profiles/r04_host_output.txt; the hipHostMalloc / hipHostFree of the
        // block itself is not in that figure and costs about a second per 10 GB).  Larger results, and hosts
        // that refuse the pinned allocation (locked-memory limit, little free RAM), take a plain Vec — the
        // library then feeds it through its own ring of pinned staging buffers and copier threads (~49 GB/s).
        const PINNED_LIMIT: usize = 2 << 30;
        let floats = n as usize * stride as usize;
        let mut pinned: *mut std::ffi::c_void = std::ptr::null_mut();
        let have_pinned = floats * 4 <= PINNED_LIMIT
            && unsafe { sys::grail_host_alloc(gpu.ctx, floats * 4, &mut pinned) } == 0
            && !pinned.is_null();
        let mut pageable: Vec<f32> = if have_pinned { Vec::new() } else { vec![0f32; floats] };
        let dst = if have_pinned { pinned as *mut f32 } else { pageable.as_mut_ptr() };
        let r = check(unsafe {
            sys::grail_synthesize_batch(gpu.ctx, b.segs.as_ptr(), b.offs.as_ptr(), b.vids.as_ptr(),
                                        b.seeds.as_ptr(), n, dst, stride,
                                        lens.as_mut_ptr(), sys::GRAIL_OUT_HOST)
        });
        let result = r.map(|_| rows_of(unsafe { std::slice::from_raw_parts(dst as *const f32, floats) }, stride as usize, &lens));
        if have_pinned {
            unsafe { sys::grail_host_free(gpu.ctx, pinned) };
        }
        drop(pageable);
        result
    }
}

/// Every GPU of the node behind the same call (grail_node_*): one context and one host thread per device inside the
/// library, the voice table carried to the other GPUs' HBM by one ncclBroadcast over xGMI, the batch cut into contiguous
/// shards (`grail_shard_range`) that render concurrently into slices of one host buffer — the reference's single call
/// (`examples/cli.rs:175-184`) for a host that holds 524 288 utterances and eight MI355X.  No data-path collective:
/// per-utterance state is self-contained (src/lib.rs:470-488, 724-748, 839-854).
pub struct Node {
    node: *mut sys::grail_node,
}

impl Node {
    /// `Node::new(&[0, 1, 2, 3, 4, 5, 6, 7], &[voice])`
    pub fn new(devices: &[i32], voices: &[Voice]) -> Result<Self, Error> {
        let have = unsafe { sys::grail_abi_version() };
        if have != sys::GRAIL_ABI_VERSION {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG,
                               message: format!("libgrail_hip.so has ABI version {have}, grail-hip-sys mirrors {}", sys::GRAIL_ABI_VERSION) });
        }
        let mut node = std::ptr::null_mut();
        check(unsafe { sys::grail_node_create(devices.as_ptr(), devices.len() as u32, &mut node) })?;
        let n = Node { node };
        let table: Vec<_> = voices.iter().map(voice_to_c).collect();
        check(unsafe { sys::grail_node_set_voices(n.node, table.as_ptr(), table.len() as u32) })?;
        Ok(n)
    }

    pub fn devices(&self) -> u32 {
        unsafe { sys::grail_node_size(self.node) }
    }

    /// What RCCL itself reports for the node's communicator (`ncclCommCount`): the number of GPUs that met.
    pub fn rccl_ranks(&self) -> Result<u32, Error> {
        let mut v = 0i64;
        check(unsafe { sys::grail_node_get_option(self.node, b"node_rccl_ranks\0".as_ptr() as *const _, &mut v) })?;
        Ok(v as u32)
    }

    pub fn set_arithmetic(&self, a: Arithmetic) -> Result<(), Error> {
        let v = match a { Arithmetic::Exact => 0, Arithmetic::Fast => 1 };
        check(unsafe { sys::grail_node_set_option(self.node, b"arithmetic\0".as_ptr() as *const _, v) })
    }
}

impl Drop for Node {
    fn drop(&mut self) {
        unsafe { sys::grail_node_destroy(self.node) };
    }
}

/// `utterances.synthesize_batch(&node)`: the same result as the `Gpu` form, rows in the caller's order.
impl SynthesisTarget for Node {
    fn render(&self, b: &FlatBatch) -> Result<Vec<Vec<f32>>, Error> {
        let node = self;
        let n = b.len();
        let mut lens = vec![0u32; n as usize];
        // the Sequencer clock pre-pass (src/lib.rs:861-888), sharded like the synthesis: sizes the rows
        check(unsafe { sys::grail_node_lengths(node.node, b.segs.as_ptr(), b.offs.as_ptr(), b.vids.as_ptr(), n, u32::MAX,
                                               lens.as_mut_ptr()) })?;
        let stride = (*lens.iter().max().unwrap_or(&0) as u64 + 63) / 64 * 64;
        let floats = n as usize * stride as usize;
        // pinned memory every device can copy into (hipHostMallocPortable) while it fits; else a plain Vec, fed through
        // each context's ring of pinned staging buffers
        const PINNED_LIMIT: usize = 16 << 30;
        let mut pinned: *mut std::ffi::c_void = std::ptr::null_mut();
        let have_pinned = floats * 4 <= PINNED_LIMIT
            && unsafe { sys::grail_node_host_alloc(node.node, floats * 4, &mut pinned) } == 0
            && !pinned.is_null();
        let mut pageable: Vec<f32> = if have_pinned { Vec::new() } else { vec![0f32; floats] };
        let dst = if have_pinned { pinned as *mut f32 } else { pageable.as_mut_ptr() };
        let r = check(unsafe {
            sys::grail_node_synthesize_batch(node.node, b.segs.as_ptr(), b.offs.as_ptr(), b.vids.as_ptr(),
                                             b.seeds.as_ptr(), n, dst, stride, lens.as_mut_ptr(), sys::GRAIL_OUT_HOST)
        });
        let result = r.map(|_| rows_of(unsafe { std::slice::from_raw_parts(dst as *const f32, floats) }, stride as usize, &lens));
        if have_pinned {
            unsafe { sys::grail_node_host_free(node.node, pinned) };
        }
        drop(pageable);
        result
    }
}

/// Arithmetic of the synthesis kernels: `Exact` (default) is bit-identical to the CPU iterator chain;
/// `Fast` is the stated-tolerance mode (|fast - exact| <= GRAIL_FAST_TOLERANCE = 64 * 2^-23 of full
/// scale, measured 18 * 2^-23; clock, phases, wraps and noise generators stay exact): 2.3x the
/// throughput on large batches, 2x on batches of a few thousand utterances (time-split kernels), 5x on batches
/// of a few hundred (time-parallel scan kernel).
pub enum Arithmetic { Exact, Fast }

impl Gpu {
    pub fn set_arithmetic(&self, a: Arithmetic) -> Result<(), Error> {
        let v = match a { Arithmetic::Exact => 0, Arithmetic::Fast => 1 };
        check(unsafe { sys::grail_set_option(self.ctx, b"arithmetic\0".as_ptr() as *const _, v) })
    }

    /// Whether `Arithmetic::Fast` is served for the current voice table (see [`fast_sharpness`]); sharper
    /// tables are rendered by the exact kernels whatever `set_arithmetic` says.
    pub fn fast_arithmetic_served(&self) -> Result<bool, Error> {
        let mut v = 0i64;
        check(unsafe { sys::grail_get_option(self.ctx, b"fast_arithmetic_served\0".as_ptr() as *const _, &mut v) })?;
        Ok(v != 0)
    }
}

/// Where an utterance goes in a mix ([`Gpu::mix`]): utterance `utterance` of the call, added into track `track` from
/// track sample `offset` on, scaled by `gain`.
#[derive(Copy, Clone, Debug)]
pub struct Placement {
    pub utterance: u32,
    pub track: u32,
    pub offset: u64,
    pub gain: f32,
}

impl Gpu {
    /// Renders `utterances` and mixes them into `n_tracks` tracks of `track_len` samples on the device
    /// (`grail_batch_mix`: every track sample is the left fold, in utterance order, of gain * sample over the placements
    /// that cover it — the bits of that CPU loop over the rows of `synthesize_batch`, `Arithmetic::Exact`); only the
    /// finished tracks cross PCIe.
    pub fn mix<I: IntoIterator<Item = Utterance>>(&self, utterances: I, placements: &[Placement], n_tracks: u32,
                                                 track_len: u64) -> Result<Vec<Vec<f32>>, Error> {
        let b = FlatBatch::new(utterances);
        let rows: Vec<u32> = placements.iter().map(|p| p.utterance).collect();
        let tracks: Vec<u32> = placements.iter().map(|p| p.track).collect();
        let offsets: Vec<u64> = placements.iter().map(|p| p.offset).collect();
        let gains: Vec<f32> = placements.iter().map(|p| p.gain).collect();
        let stride = ((track_len + 63) / 64 * 64).max(64);
        let floats = n_tracks as usize * stride as usize;
        let mut host = vec![0f32; floats];
        unsafe {
            let mut h = std::ptr::null_mut();
            check(sys::grail_batch_upload(self.ctx, b.segs.as_ptr(), b.offs.as_ptr(), b.vids.as_ptr(), b.seeds.as_ptr(),
                                          b.len(), &mut h))?;
            let mut d: *mut std::ffi::c_void = std::ptr::null_mut();
            let mut r = check(sys::grail_device_alloc(self.ctx, floats * 4 + 4, &mut d));
            if r.is_ok() {
                r = check(sys::grail_batch_mix(self.ctx, h, rows.as_ptr(), tracks.as_ptr(), offsets.as_ptr(), gains.as_ptr(),
                                               rows.len() as u32, d as *mut f32, stride, n_tracks, track_len,
                                               std::ptr::null_mut(), 0));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, host.as_mut_ptr() as *mut std::ffi::c_void, d, floats * 4));
            }
            if !d.is_null() {
                sys::grail_device_free(self.ctx, d);
            }
            sys::grail_batch_free(self.ctx, h);
            r?;
        }
        Ok(host.chunks(stride as usize).map(|t| t[..track_len as usize].to_vec()).collect())
    }

    /// [`Gpu::mix`] with a level per placement instead of a gain (`grail_batch_mix_leveled`): placement `i`'s utterance is
    /// brought to `level_db[i]` decibels (0 dB = level 1.0) of `mode`; `Placement::gain` is not read.  The rows are
    /// measured on the device between rendering and mixing.  Returns the tracks, the gains that were used and the number
    /// of placements that got gain 0 (an empty or silent utterance, or one holding a non-finite sample).
    pub fn mix_leveled<I: IntoIterator<Item = Utterance>>(&self, utterances: I, placements: &[Placement], level_db: &[f32],
                                                         mode: LevelMode, n_tracks: u32, track_len: u64)
                                                         -> Result<(Vec<Vec<f32>>, Vec<f32>, u32), Error> {
        let (tracks, gains, unleveled, _) = self.mix_leveled_with(utterances, placements, level_db, mode, None, n_tracks,
                                                                  track_len)?;
        Ok((tracks, gains, unleveled))
    }

    /// [`Gpu::mix_leveled`] under a true-peak ceiling in dBTP (`grail_batch_mix_leveled_limited`): every utterance's true
    /// peak is measured on the device as well, and a gain that would bring it above the ceiling is cut back to it.  The
    /// ceiling binds each placement; placements that overlap on a track can still sum above it ([`Gpu::true_peak`] of the
    /// finished tracks tells).  Returns the tracks, the gains that were used, the placements that got gain 0 and the
    /// placements that the ceiling changed.
    pub fn mix_leveled_limited<I: IntoIterator<Item = Utterance>>(&self, utterances: I, placements: &[Placement],
                                                                 level_db: &[f32], mode: LevelMode, ceiling_db: f32,
                                                                 n_tracks: u32, track_len: u64)
                                                                 -> Result<(Vec<Vec<f32>>, Vec<f32>, u32, u32), Error> {
        self.mix_leveled_with(utterances, placements, level_db, mode, Some(ceiling_db), n_tracks, track_len)
    }

    fn mix_leveled_with<I: IntoIterator<Item = Utterance>>(&self, utterances: I, placements: &[Placement], level_db: &[f32],
                                                          mode: LevelMode, ceiling_db: Option<f32>, n_tracks: u32,
                                                          track_len: u64)
                                                          -> Result<(Vec<Vec<f32>>, Vec<f32>, u32, u32), Error> {
        assert_eq!(level_db.len(), placements.len());
        let b = FlatBatch::new(utterances);
        let rows: Vec<u32> = placements.iter().map(|p| p.utterance).collect();
        let tracks: Vec<u32> = placements.iter().map(|p| p.track).collect();
        let offsets: Vec<u64> = placements.iter().map(|p| p.offset).collect();
        let stride = ((track_len + 63) / 64 * 64).max(64);
        let floats = n_tracks as usize * stride as usize;
        let mut host = vec![0f32; floats];
        let mut gains = vec![0f32; rows.len().max(1)];
        let mut unleveled = 0u32;
        let mut limited = 0u32;
        unsafe {
            let mut h = std::ptr::null_mut();
            check(sys::grail_batch_upload(self.ctx, b.segs.as_ptr(), b.offs.as_ptr(), b.vids.as_ptr(), b.seeds.as_ptr(),
                                          b.len(), &mut h))?;
            let mut d: *mut std::ffi::c_void = std::ptr::null_mut();
            let mut r = check(sys::grail_device_alloc(self.ctx, floats * 4 + 4, &mut d));
            if r.is_ok() {
                r = check(match ceiling_db {
                    None => sys::grail_batch_mix_leveled(self.ctx, h, rows.as_ptr(), tracks.as_ptr(), offsets.as_ptr(),
                                                         level_db.as_ptr(), mode as std::os::raw::c_int, rows.len() as u32,
                                                         d as *mut f32, stride, n_tracks, track_len, std::ptr::null_mut(),
                                                         gains.as_mut_ptr(), &mut unleveled, 0),
                    Some(c) => sys::grail_batch_mix_leveled_limited(self.ctx, h, rows.as_ptr(), tracks.as_ptr(),
                                                                    offsets.as_ptr(), level_db.as_ptr(),
                                                                    mode as std::os::raw::c_int, rows.len() as u32,
                                                                    d as *mut f32, stride, n_tracks, track_len,
                                                                    std::ptr::null_mut(), gains.as_mut_ptr(), &mut unleveled,
                                                                    c, &mut limited, 0),
                });
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, host.as_mut_ptr() as *mut std::ffi::c_void, d, floats * 4));
            }
            if !d.is_null() {
                sys::grail_device_free(self.ctx, d);
            }
            sys::grail_batch_free(self.ctx, h);
            r?;
        }
        gains.truncate(rows.len());
        Ok((host.chunks(stride as usize).map(|t| t[..track_len as usize].to_vec()).collect(), gains, unleveled, limited))
    }

    /// True peak of rows of samples, measured on the device (`grail_true_peak_async`; the contract is the header's section
    /// "levels, continued: true peak"): per row the largest magnitude of the row oversampled four times by the filter of
    /// BS.1770-4 Annex 2 (see [`true_peak_db`]) and the count of non-finite samples.  Time is parallel: one long row fills
    /// the device.
    pub fn true_peak(&self, rows: &[Vec<f32>]) -> Result<(Vec<f64>, Vec<u32>), Error> {
        let n = rows.len();
        let mut peaks = vec![0f64; n];
        let mut bad = vec![0u32; n];
        if n == 0 {
            return Ok((peaks, bad));
        }
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 4] = [std::ptr::null_mut(); 4];
            let sizes = [n * stride * 4, n * 4, n * 8, n * 4];
            let mut r = Ok(());
            for k in 0..4 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[1], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_true_peak_async(self.ctx, d[0] as *const f32, stride as u64, d[1] as *const u32, n as u32,
                                                     d[2] as *mut f64, d[3] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, peaks.as_mut_ptr() as *mut std::ffi::c_void, d[2], n * 8));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((peaks, bad))
    }

    /// The look-ahead limiter over rows of samples, `group` consecutive rows sharing one gain curve (finished tracks as one
    /// linked group: `group = rows.len()`), on the device (`grail_limit_async`; the contract is the header's section "levels,
    /// continued: limiter").  `ceiling` is linear (see [`limit_ceiling`]), the look-ahead `2^lookahead_log2` samples.
    /// Returns the limited rows and, per group, the smallest gain, the count of limited samples and the count of
    /// non-finite ones; a group whose rows differ in length is refused: its rows come back empty, its numbers are NaN,
    /// [`LIMIT_REFUSED`] and 0.  Afterwards `|sample| <= ceiling` holds exactly; the true peak follows to within the header's
    /// bound: measure it with [`Gpu::true_peak`].
    pub fn limit(&self, rows: &[Vec<f32>], ceiling: f32, lookahead_log2: u32, group: u32)
                 -> Result<(Vec<Vec<f32>>, Vec<f32>, Vec<u32>, Vec<u32>), Error> {
        let n = rows.len();
        if group == 0 || n % group as usize != 0 {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "limit: the number of rows is no multiple of group".into() });
        }
        let groups = n / group as usize;
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut min_gain = vec![0f32; groups];
        let mut limited = vec![0u32; groups];
        let mut bad = vec![0u32; groups];
        if n == 0 {
            return Ok((out, min_gain, limited, bad));
        }
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 6] = [std::ptr::null_mut(); 6];
            let sizes = [n * stride * 4, n * stride * 4, n * 4, groups * 4, groups * 4, groups * 4];
            let mut r = Ok(());
            for k in 0..6 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_limit_async(self.ctx, d[0] as *const f32, stride as u64, d[2] as *const u32, n as u32, group,
                                                 ceiling, lookahead_log2, d[1] as *mut f32, stride as u64, d[3] as *mut f32,
                                                 d[4] as *mut u32, d[5] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, min_gain.as_mut_ptr() as *mut std::ffi::c_void, d[3], groups * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, limited.as_mut_ptr() as *mut std::ffi::c_void, d[4], groups * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[5], groups * 4));
            }
            for i in 0..n {
                if r.is_ok() && lens[i] != 0 && limited[i / group as usize] != LIMIT_REFUSED {
                    out[i] = vec![0f32; lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(self.ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * stride) as *const std::ffi::c_void, lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((out, min_gain, limited, bad))
    }

    /// Rows of samples at `rate_in` resampled to `rate_out` on the device (`grail_resample_async`; the contract is the header's
    /// section "levels, continued: sample-rate conversion"): output `m` of a row sits at input time `m * rate_in / rate_out`,
    /// a row of `n` samples gives `ceil(n * rate_out / rate_in)`.  Returns the resampled rows and, per row, the count of
    /// non-finite input samples (they enter as +0.0).  The filter overshoots: limit or measure after resampling.
    pub fn resample(&self, rows: &[Vec<f32>], rate_in: u32, rate_out: u32) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        let n = rows.len();
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let longest_out = resample_len(longest as u64, rate_in, rate_out)? as usize;
        if n == 0 {
            return Ok((out, bad));
        }
        let stride = ((longest + 63) / 64 * 64).max(64);
        let out_stride = ((longest_out + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let sizes = [n * stride * 4, n * out_stride * 4, n * 4, n * 4, n * 4];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_resample_async(self.ctx, d[0] as *const f32, stride as u64, d[2] as *const u32, n as u32, rate_in,
                                                    rate_out, d[1] as *mut f32, out_stride as u64, d[3] as *mut u32, d[4] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(self.ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad))
    }

    /// A set of FIR filters on this device (`grail_fir_create`), for [`Gpu::fir`]: `(taps, origin)` per filter, `origin` the tap
    /// that sits at time zero (0: causal; `(taps.len() - 1) / 2`: linear phase, zero delay).  Released when dropped.
    pub fn fir_set(&self, filters: &[(Vec<f32>, u32)]) -> Result<FirSet<'_>, Error> {
        let taps: Vec<f32> = filters.iter().flat_map(|(t, _)| t.iter().copied()).collect();
        let n_taps: Vec<u32> = filters.iter().map(|(t, _)| t.len() as u32).collect();
        let origin: Vec<u32> = filters.iter().map(|(_, o)| *o).collect();
        let tail = filters.iter().map(|(t, o)| (t.len() as u64).saturating_sub(1 + *o as u64)).max().unwrap_or(0);
        let mut set: *mut sys::grail_fir = std::ptr::null_mut();
        check(unsafe {
            sys::grail_fir_create(self.ctx, taps.as_ptr(), n_taps.as_ptr(), origin.as_ptr(), filters.len() as u32, &mut set)
        })?;
        let longest = n_taps.iter().copied().max().unwrap_or(1);
        Ok(FirSet { gpu: self, set, tail, longest })
    }

    /// Rows of samples filtered on the device (`grail_fir_async`; the contract is the header's section "levels, continued: FIR
    /// filtering"), row `i` with filter `which[i]` of the set (`None`: filter 0 for every row).  A row of `n` samples gives
    /// `n + taps - 1 - origin`: the tail rings out.  Returns the filtered rows and, per row, the count of non-finite input
    /// samples (they enter as +0.0); a row whose index is outside the set comes back empty.  A filter overshoots: limit or
    /// measure after filtering.
    pub fn fir(&self, set: &FirSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        let n = rows.len();
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        if n == 0 {
            return Ok((out, bad));
        }
        if which.map_or(false, |w| w.len() != n) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "fir: one filter index per row".to_string() });
        }
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let out_stride = ((longest + set.tail as usize + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 6] = [std::ptr::null_mut(); 6];
            let sizes = [n * stride * 4, n * out_stride * 4, n * 4, n * 4, n * 4, n * 4];
            let mut r = Ok(());
            for k in 0..6 {
                if r.is_ok() && (k < 5 || which.is_some()) {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if let (true, Some(w)) = (r.is_ok(), which) {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[5], w.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_fir_async(self.ctx, set.set, d[0] as *const f32, stride as u64, d[2] as *const u32, n as u32,
                                               d[5] as *const u32, d[1] as *mut f32, out_stride as u64, d[3] as *mut u32,
                                               d[4] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 && out_lens[i] != LIMIT_REFUSED {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(self.ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad))
    }

    /// A stream of `n_rows` rows filtered chunk by chunk (`grail_filter_stream_open`; the contract is the header's section
    /// "levels, continued: FIR filtering of streams"), row `i` bound to filter `which[i]` of the set (`None`: filter 0).  The
    /// chunks' outputs put end to end, then the tail of [`FirStream::finish`], are the bits [`Gpu::fir`] gives for the whole
    /// rows.  Closed when dropped; the borrow keeps the set alive for as long.
    pub fn fir_stream<'a>(&'a self, set: &'a FirSet<'a>, n_rows: u32, which: Option<&[u32]>) -> Result<FirStream<'a>, Error> {
        if which.map_or(false, |w| w.len() != n_rows as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "fir_stream: one filter index per row".to_string() });
        }
        let mut fs: *mut sys::grail_filter_stream = std::ptr::null_mut();
        check(unsafe {
            sys::grail_filter_stream_open(self.ctx, set.set, n_rows, which.map_or(std::ptr::null(), |w| w.as_ptr()), &mut fs)
        })?;
        Ok(FirStream { gpu: self, fs, n_rows, tail: set.longest.saturating_sub(1), _set: set })
    }

    /// A set of recursive filters on this device (`grail_iir_create`), for [`Gpu::iir`] and [`Gpu::iir_stream`]: per filter its
    /// biquad sections `[b0, b1, b2, a1, a2]`, one to eight of them ([`iir_design`] makes one).  Released when dropped.
    pub fn iir_set(&self, filters: &[Vec<[f64; 5]>]) -> Result<IirSet<'_>, Error> {
        let coef: Vec<f64> = filters.iter().flat_map(|f| f.iter().flat_map(|s| s.iter().copied())).collect();
        let n_sections: Vec<u32> = filters.iter().map(|f| f.len() as u32).collect();
        let mut set: *mut sys::grail_iir = std::ptr::null_mut();
        check(unsafe { sys::grail_iir_create(self.ctx, coef.as_ptr(), n_sections.as_ptr(), filters.len() as u32, &mut set) })?;
        Ok(IirSet { gpu: self, set })
    }

    /// Rows of samples filtered recursively on the device (`grail_iir_async`; the contract is the header's section "levels,
    /// continued: recursive filtering"), row `i` with filter `which[i]` of the set (`None`: filter 0 for every row).  A row of
    /// `n` samples gives `n + tail`: the filter rings out on +0.0 input.  Returns the filtered rows and, per row, the count of
    /// non-finite input samples (they enter as +0.0); a row whose index is outside the set comes back empty.  A filter
    /// overshoots: limit or measure after filtering.
    pub fn iir(&self, set: &IirSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>, tail: u32) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        self.iir_rows(set, rows, which, tail, false)
    }

    /// [`Gpu::iir`] parallel in time (`grail_biquad_blocked_async`; the contract is the header's section "levels, continued:
    /// recursive filtering, parallel in time"): a row's steps in blocks of 1024, a lane each.  The call for a few long rows
    /// (the tracks of a mix); [`Gpu::iir`] is the one for many rows.  Bit for bit [`Gpu::iir`] up to a row's 1024th output, a
    /// contract of its own from there on (the two differ by some 1e-11 of the row's peak before the rounding to `f32`).
    pub fn iir_blocked(&self, set: &IirSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>, tail: u32) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        self.iir_rows(set, rows, which, tail, true)
    }

    fn iir_rows(&self, set: &IirSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>, tail: u32, blocked: bool) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        let n = rows.len();
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        if n == 0 {
            return Ok((out, bad));
        }
        if which.map_or(false, |w| w.len() != n) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "iir: one filter index per row".to_string() });
        }
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let out_stride = ((longest + tail as usize + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 6] = [std::ptr::null_mut(); 6];
            let sizes = [n * stride * 4, n * out_stride * 4, n * 4, n * 4, n * 4, n * 4];
            let mut r = Ok(());
            for k in 0..6 {
                if r.is_ok() && (k < 5 || which.is_some()) {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if let (true, Some(w)) = (r.is_ok(), which) {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[5], w.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                let call = if blocked { sys::grail_biquad_blocked_async } else { sys::grail_iir_async };
                r = check(call(self.ctx, set.set, d[0] as *const f32, stride as u64, d[2] as *const u32, n as u32,
                               d[5] as *const u32, tail, d[1] as *mut f32, out_stride as u64, d[3] as *mut u32, d[4] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 && out_lens[i] != LIMIT_REFUSED {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(self.ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad))
    }

    /// A stream of `n_rows` rows filtered recursively chunk by chunk (`grail_iir_stream_open`; the contract is the header's
    /// section "levels, continued: recursive filtering of streams"), row `i` bound to filter `which[i]` of the set (`None`:
    /// filter 0), every row ringing out over `tail` outputs at its finish.  The chunks' outputs put end to end, then the tail of
    /// [`IirStream::finish`], are the bits [`Gpu::iir`] gives for the whole rows with the same tail.  Closed when dropped; the
    /// borrow keeps the set alive for as long.
    pub fn iir_stream<'a>(&'a self, set: &'a IirSet<'a>, n_rows: u32, which: Option<&[u32]>, tail: u32) -> Result<IirStream<'a>, Error> {
        if which.map_or(false, |w| w.len() != n_rows as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "iir_stream: one filter index per row".to_string() });
        }
        let mut is: *mut sys::grail_iir_stream = std::ptr::null_mut();
        check(unsafe {
            sys::grail_iir_stream_open(self.ctx, set.set, n_rows, which.map_or(std::ptr::null(), |w| w.as_ptr()), tail, &mut is)
        })?;
        Ok(IirStream { gpu: self, is, n_rows, tail, _set: set })
    }

    /// A set of gain curves on this device (`grail_dyn_create`), for [`Gpu::dynamics`] and [`Gpu::dyn_stream`]: one to sixteen
    /// curves, each a table of [`DYN_POINTS`] gains ([`dyn_design`] makes one), its two alphas ([`dyn_ballistics`]) and its
    /// detector (`sys::GRAIL_DYN_PEAK` or `sys::GRAIL_DYN_SQUARE`).  Released when dropped.
    pub fn dyn_set(&self, curves: &[DynCurve]) -> Result<DynSet<'_>, Error> {
        if curves.iter().any(|c| c.gain.len() != DYN_POINTS) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "dyn_set: a curve has DYN_POINTS gains".to_string() });
        }
        let gain: Vec<f64> = curves.iter().flat_map(|c| c.gain.iter().copied()).collect();
        let alpha: Vec<f64> = curves.iter().flat_map(|c| c.alpha.iter().copied()).collect();
        let detector: Vec<u32> = curves.iter().map(|c| c.detector as u32).collect();
        let mut set: *mut sys::grail_dyn = std::ptr::null_mut();
        check(unsafe { sys::grail_dyn_create(self.ctx, gain.as_ptr(), alpha.as_ptr(), detector.as_ptr(), curves.len() as u32, &mut set) })?;
        Ok(DynSet { gpu: self, set })
    }

    /// Rows of samples compressed, expanded or ducked on the device (`grail_dyn_async`; the contract is the header's section
    /// "levels, continued: dynamics"), row `i` on curve `which[i]` of the set (`None`: curve 0 for every row).  `keys`: `None`,
    /// and every row follows itself; or the key rows and, per row, the index of the key it follows (ducking: the bed's rows keyed
    /// by the voice's track).  Returns the rows, per row the count of non-finite input samples (they enter as +0.0) and the
    /// smallest gain it was given (1.0 for an empty row); a row whose curve or key index is outside comes back empty with a NaN.
    pub fn dynamics(&self, set: &DynSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>, keys: Option<(&[Vec<f32>], &[u32])>)
                    -> Result<(Vec<Vec<f32>>, Vec<u32>, Vec<f64>), Error> {
        self.dynamics_rows(set, rows, which, keys, false)
    }

    /// [`Gpu::dynamics`] with a workgroup a row (`grail_track_dyn_async`; the header's section "levels, continued: dynamics, a
    /// workgroup a row"): the call for the few long tracks of a mix, [`Gpu::dynamics`] the one for many rows.  Bit for bit
    /// [`Gpu::dynamics`] in every result: only the envelope's chain stays serial, the rest of a sample's work does not.
    pub fn track_dynamics(&self, set: &DynSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>, keys: Option<(&[Vec<f32>], &[u32])>)
                          -> Result<(Vec<Vec<f32>>, Vec<u32>, Vec<f64>), Error> {
        self.dynamics_rows(set, rows, which, keys, true)
    }

    fn dynamics_rows(&self, set: &DynSet<'_>, rows: &[Vec<f32>], which: Option<&[u32]>, keys: Option<(&[Vec<f32>], &[u32])>, tracks: bool)
                     -> Result<(Vec<Vec<f32>>, Vec<u32>, Vec<f64>), Error> {
        let n = rows.len();
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        let mut min_gain = vec![1f64; n];
        if n == 0 {
            return Ok((out, bad, min_gain));
        }
        if which.map_or(false, |w| w.len() != n) || keys.map_or(false, |(k, r)| r.len() != n || k.is_empty()) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "dynamics: one curve index and one key index per row".to_string() });
        }
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        let n_keys = keys.map_or(0, |(k, _)| k.len());
        let key_stride = keys.map_or(0, |(k, _)| ((k.iter().map(|r| r.len()).max().unwrap_or(0) + 63) / 64 * 64).max(64));
        let key_lens: Vec<u32> = keys.map_or(Vec::new(), |(k, _)| k.iter().map(|r| r.len() as u32).collect());
        unsafe {
            // rows, out, len, out_len, nonfinite, min_gain, curve, key, key_len, key_row
            let mut d: [*mut std::ffi::c_void; 10] = [std::ptr::null_mut(); 10];
            let sizes = [n * stride * 4, n * stride * 4, n * 4, n * 4, n * 4, n * 8, n * 4, n_keys * key_stride * 4, n_keys * 4, n * 4];
            let mut r = Ok(());
            for k in 0..10 {
                if r.is_ok() && (k < 6 || (k == 6 && which.is_some()) || (k > 6 && keys.is_some())) {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if let (true, Some(w)) = (r.is_ok(), which) {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[6], w.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if let Some((k, key_row)) = keys {
                for (i, row) in k.iter().enumerate() {
                    if r.is_ok() && !row.is_empty() {
                        r = check(sys::grail_memcpy_h2d(self.ctx, (d[7] as *mut f32).add(i * key_stride) as *mut std::ffi::c_void,
                                                        row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                    }
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, d[8], key_lens.as_ptr() as *const std::ffi::c_void, n_keys * 4));
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, d[9], key_row.as_ptr() as *const std::ffi::c_void, n * 4));
                }
            }
            if r.is_ok() {
                let call = if tracks { sys::grail_track_dyn_async } else { sys::grail_dyn_async };
                r = check(call(self.ctx, set.set, d[0] as *const f32, stride as u64, d[2] as *const u32, n as u32,
                               d[6] as *const u32, d[7] as *const f32, key_stride as u64, d[8] as *const u32,
                               n_keys as u32, d[9] as *const u32, d[1] as *mut f32, stride as u64, d[3] as *mut u32,
                               d[4] as *mut u32, d[5] as *mut f64));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, min_gain.as_mut_ptr() as *mut std::ffi::c_void, d[5], n * 8));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 && out_lens[i] != LIMIT_REFUSED {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(self.ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad, min_gain))
    }

    /// A stream of `n_rows` self-keyed rows compressed chunk by chunk (`grail_dyn_stream_open`; the contract is the header's
    /// section "levels, continued: dynamics of streams"), row `i` bound to curve `which[i]` of the set (`None`: curve 0).  The
    /// chunks' outputs put end to end are the bits [`Gpu::dynamics`] gives for the whole rows.  Closed when dropped; the borrow
    /// keeps the set alive for as long.  (Keyed streams are reached through the `-sys` crate.)
    pub fn dyn_stream<'a>(&'a self, set: &'a DynSet<'a>, n_rows: u32, which: Option<&[u32]>) -> Result<DynStream<'a>, Error> {
        if which.map_or(false, |w| w.len() != n_rows as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "dyn_stream: one curve index per row".to_string() });
        }
        let mut ds: *mut sys::grail_dyn_stream = std::ptr::null_mut();
        check(unsafe {
            sys::grail_dyn_stream_open(self.ctx, set.set, n_rows, which.map_or(std::ptr::null(), |w| w.as_ptr()), 0, std::ptr::null(), &mut ds)
        })?;
        Ok(DynStream { gpu: self, ds, n_rows, _set: set })
    }

    /// A stream of `n_rows` rows resampled chunk by chunk from `rate_in` to `rate_out` (`grail_resample_stream_open`; the
    /// contract is the header's section "levels, continued: sample-rate conversion of streams").  The chunks' outputs put
    /// end to end, then the tail of [`ResampleStream::finish`], are the bits [`Gpu::resample`] gives for the whole rows.
    /// Closed when dropped.
    pub fn resample_stream(&self, rate_in: u32, rate_out: u32, n_rows: u32) -> Result<ResampleStream<'_>, Error> {
        let (up, down, taps) = resample_ratio(rate_in, rate_out)?;
        let mut rs: *mut sys::grail_resample_stream = std::ptr::null_mut();
        check(unsafe { sys::grail_resample_stream_open(self.ctx, rate_in, rate_out, n_rows, &mut rs) })?;
        Ok(ResampleStream { gpu: self, rs, n_rows, up, down, taps })
    }

    /// A stream of `n_rows` rows in groups of `group`, limited chunk by chunk under `ceiling` (linear) with a look-ahead of
    /// 2^`lookahead_log2` samples (`grail_limit_stream_open`; the contract is the header's section "levels, continued: the
    /// limiter on streams").  The chunks' outputs put end to end, then the tail of [`LimitStream::finish`], are the bits
    /// [`Gpu::limit`] gives for the whole rows, 2^`lookahead_log2` + 10 samples late.  Closed when dropped.
    pub fn limit_stream(&self, n_rows: u32, group: u32, ceiling: f32, lookahead_log2: u32) -> Result<LimitStream<'_>, Error> {
        let mut ls: *mut sys::grail_limit_stream = std::ptr::null_mut();
        check(unsafe { sys::grail_limit_stream_open(self.ctx, n_rows, group, ceiling, lookahead_log2, &mut ls) })?;
        Ok(LimitStream { gpu: self, ls, n_rows, group, delay: (1u32 << lookahead_log2) + 10 })
    }

    /// A stream of `n_rows` rows metered chunk by chunk at `sample_rate` with grail_kweighting's coefficients, each row's
    /// ledger holding `max_hops` hops of 100 ms (`grail_meter_stream_open`; the contract is the header's section "levels,
    /// continued: the meters on streams").  The chunks' hop sums put end to end are the bits [`Gpu::loudness`]'s kernels give
    /// for the whole rows, the largest of the chunks' true peaks is [`Gpu::true_peak`]'s.  Closed when dropped.
    pub fn meter_stream(&self, n_rows: u32, sample_rate: u32, max_hops: u64) -> Result<MeterStream<'_>, Error> {
        let mut ms: *mut sys::grail_meter_stream = std::ptr::null_mut();
        check(unsafe { sys::grail_meter_stream_open(self.ctx, n_rows, sample_rate, std::ptr::null(), max_hops, &mut ms) })?;
        Ok(MeterStream { gpu: self, ms, n_rows, hop: sample_rate / 10 })
    }

    /// K-weighted gated loudness of rows of samples, measured on the device (`grail_loudness_async`; the contract is the
    /// header's section "levels, continued"): per row the gated mean square (see [`loudness_lufs`]) and the count of
    /// non-finite samples.  One lane filters one row: many rows fill the device.
    pub fn loudness(&self, rows: &[Vec<f32>], sample_rate: u32) -> Result<(Vec<f64>, Vec<u32>), Error> {
        let n = rows.len();
        let mut gated = vec![0f64; n];
        let mut bad = vec![0u32; n];
        if n == 0 {
            return Ok((gated, bad));
        }
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 4] = [std::ptr::null_mut(); 4];
            let sizes = [n * stride * 4, n * 4, n * 8, n * 4];
            let mut r = Ok(());
            for k in 0..4 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[1], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_loudness_async(self.ctx, d[0] as *const f32, stride as u64, d[1] as *const u32, n as u32,
                                                    sample_rate, std::ptr::null(), d[2] as *mut f64, std::ptr::null_mut(), 0,
                                                    d[3] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, gated.as_mut_ptr() as *mut std::ffi::c_void, d[2], n * 8));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        Ok((gated, bad))
    }

    /// The same of few long rows (finished tracks), parallel in time (`grail_loudness_segmented_async`: every hop of
    /// 100 ms filtered from a zero state three hops before it, one lane per hop): per row the gated mean square, the
    /// count of non-finite samples and the row's hop sums, from which [`loudness_range`] and [`loudness_window_max`]
    /// follow on the host.
    pub fn track_loudness(&self, rows: &[Vec<f32>], sample_rate: u32) -> Result<(Vec<f64>, Vec<u32>, Vec<Vec<f64>>), Error> {
        let n = rows.len();
        let mut gated = vec![0f64; n];
        let mut bad = vec![0u32; n];
        if n == 0 {
            return Ok((gated, bad, Vec::new()));
        }
        let hop = (sample_rate / 10) as usize;
        let longest = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let hs = if hop > 0 { (stride / hop).max(1) } else { 1 };
        let mut hops = vec![0f64; n * hs];
        let lens: Vec<u32> = rows.iter().map(|r| r.len() as u32).collect();
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let sizes = [n * stride * 4, n * 4, n * 8, n * 4, n * hs * 8];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(self.ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in rows.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(self.ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(self.ctx, d[1], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_loudness_segmented_async(self.ctx, d[0] as *const f32, stride as u64, d[1] as *const u32,
                                                              n as u32, sample_rate, std::ptr::null(), d[2] as *mut f64,
                                                              d[4] as *mut f64, hs as u64, d[3] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, gated.as_mut_ptr() as *mut std::ffi::c_void, d[2], n * 8));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(self.ctx, hops.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * hs * 8));
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(self.ctx, p);
                }
            }
            r?;
        }
        // (hops past a row's last were never written)
        let per_row = rows.iter().enumerate().map(|(i, row)| hops[i * hs..i * hs + row.len() / hop].to_vec()).collect();
        Ok((gated, bad, per_row))
    }
}

/// The ten K-weighting coefficients for a sample rate (`grail_kweighting`; pure host, no GPU).
pub fn kweighting(sample_rate: u32) -> Result<[f64; 10], Error> {
    let mut coef = [0f64; 10];
    check(unsafe { sys::grail_kweighting(sample_rate, coef.as_mut_ptr()) })?;
    Ok(coef)
}

/// The BS.1770 gate over one row's hop sums, `hop` = sample rate / 10 (`grail_gated_mean_square`; pure host).
pub fn gated_mean_square(hop_sumsq: &[f64], hop: u32) -> f64 {
    unsafe { sys::grail_gated_mean_square(hop_sumsq.as_ptr(), hop_sumsq.len() as u32, hop) }
}

/// Loudness in LUFS of a gated mean square (`grail_loudness_lufs`): negative infinity for 0.
pub fn loudness_lufs(gated_ms: f64) -> f64 {
    unsafe { sys::grail_loudness_lufs(gated_ms) }
}

/// The level whose 20 log10 is the loudness in LUFS (`grail_loudness_level`).
pub fn loudness_level(gated_ms: f64) -> f64 {
    unsafe { sys::grail_loudness_level(gated_ms) }
}

/// The largest mean square over windows of `window_hops` hops of one row's hop sums, one window every hop
/// (`grail_loudness_window_max`; pure host): 4 hops = momentary, 30 = short-term; [`loudness_lufs`] gives its LUFS.
pub fn loudness_window_max(hop_sumsq: &[f64], hop: u32, window_hops: u32) -> f64 {
    unsafe { sys::grail_loudness_window_max(hop_sumsq.as_ptr(), hop_sumsq.len() as u32, hop, window_hops) }
}

/// The loudness range in LU of one row's hop sums after EBU Tech 3342 (`grail_loudness_range`; pure host).
pub fn loudness_range(hop_sumsq: &[f64], hop: u32) -> f64 {
    unsafe { sys::grail_loudness_range(hop_sumsq.as_ptr(), hop_sumsq.len() as u32, hop) }
}

/// The 4 x 12 taps of the true-peak filter, `[phase][tap]` (`grail_true_peak_coefficients`; pure host, no GPU).
pub fn true_peak_coefficients() -> Result<[[f64; 12]; 4], Error> {
    let mut coef = [[0f64; 12]; 4];
    check(unsafe { sys::grail_true_peak_coefficients(coef.as_mut_ptr() as *mut f64) })?;
    Ok(coef)
}

/// A true peak in dBTP (`grail_true_peak_db`): 20 log10, negative infinity for 0.
pub fn true_peak_db(true_peak: f64) -> f64 {
    unsafe { sys::grail_true_peak_db(true_peak) }
}

/// `n_limited` of a group that [`Gpu::limit`] refused (`GRAIL_LIMIT_REFUSED`).
pub const LIMIT_REFUSED: u32 = 0xFFFF_FFFF;
/// The largest `lookahead_log2` of [`Gpu::limit`] (`GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX`).
pub const LIMIT_LOOKAHEAD_LOG2_MAX: u32 = 10;

/// `(up, down, taps)` of a pair of whole-numbered sample rates (`grail_resample_ratio`; pure host); an error for a pair
/// that [`Gpu::resample`] does not take: a rate of 0, equal rates, more than 32 768 table entries.
pub fn resample_ratio(rate_in: u32, rate_out: u32) -> Result<(u32, u32, u32), Error> {
    let (mut up, mut down, mut taps) = (0u32, 0u32, 0u32);
    check(unsafe { sys::grail_resample_ratio(rate_in, rate_out, &mut up, &mut down, &mut taps) })?;
    Ok((up, down, taps))
}

/// The length of a row of `n` samples resampled: `ceil(n * up / down)` (`grail_resample_len`; pure host).
pub fn resample_len(n: u64, rate_in: u32, rate_out: u32) -> Result<u64, Error> {
    let mut n_out = 0u64;
    check(unsafe { sys::grail_resample_len(n, rate_in, rate_out, &mut n_out) })?;
    Ok(n_out)
}

/// A set of FIR filters resident on a [`Gpu`]'s device ([`Gpu::fir_set`]); `grail_fir_free` when dropped.
pub struct FirSet<'a> {
    gpu: &'a Gpu,
    set: *mut sys::grail_fir,
    tail: u64,
    longest: u32,
}

impl Drop for FirSet<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_fir_free(self.gpu.ctx, self.set);
        }
    }
}

/// Rows filtered chunk by chunk on a [`Gpu`]'s device ([`Gpu::fir_stream`]), their history resident in HBM between calls;
/// `grail_filter_stream_close` when dropped.
pub struct FirStream<'a> {
    gpu: &'a Gpu,
    fs: *mut sys::grail_filter_stream,
    n_rows: u32,
    tail: u32,
    _set: &'a FirSet<'a>,
}

impl FirStream<'_> {
    // one call on the stream: `chunks` fed (None: the rows marked in `which` finish); the outputs and the counts per row
    fn call(&mut self, chunks: Option<&[Vec<f32>]>, which: Option<&[u8]>) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        let n = self.n_rows as usize;
        let longest = chunks.map_or(0, |c| c.iter().map(|r| r.len()).max().unwrap_or(0));
        let stride = (longest + 63) / 64 * 64;
        let out_stride = (longest.max(self.tail as usize) + 63) / 64 * 64;
        let lens: Vec<u32> = chunks.map_or(vec![0u32; n], |c| c.iter().map(|r| r.len() as u32).collect());
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let sizes = [n * stride.max(1) * 4, n * out_stride.max(1) * 4, n * 4, n * 4, n * 4];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, sizes[k], &mut d[k]));
                }
            }
            if let Some(c) = chunks {
                for (i, row) in c.iter().enumerate() {
                    if r.is_ok() && !row.is_empty() {
                        r = check(sys::grail_memcpy_h2d(ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                        row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                    }
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_h2d(ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
                }
                if r.is_ok() {
                    r = check(sys::grail_filter_stream_next_async(ctx, self.fs, d[0] as *const f32, stride as u64, d[2] as *const u32,
                                                                  d[1] as *mut f32, out_stride as u64, d[3] as *mut u32,
                                                                  d[4] as *mut u32));
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_d2h(ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
                }
            } else if r.is_ok() {
                r = check(sys::grail_filter_stream_finish_async(ctx, self.fs, which.map_or(std::ptr::null(), |w| w.as_ptr()),
                                                                d[1] as *mut f32, out_stride as u64, d[3] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 && out_lens[i] != LIMIT_REFUSED {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad))
    }

    /// Feeds row `i` the samples `chunks[i]` (an empty chunk: the row pauses) and returns, per row, the outputs that became
    /// known and the count of non-finite samples among those fed (`grail_filter_stream_next_async`).  A row that has ended
    /// and is fed comes back empty, its state untouched.
    pub fn next(&mut self, chunks: &[Vec<f32>]) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        if chunks.len() != self.n_rows as usize {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "FirStream::next: one chunk per row".to_string() });
        }
        self.call(Some(chunks), None)
    }

    /// Ends the rows marked in `which` (`None`: every row) and returns their tails: what the filter still rings out with
    /// +0.0 to come (`grail_filter_stream_finish_async`); empty for rows not marked and rows ended before.
    pub fn finish(&mut self, which: Option<&[bool]>) -> Result<Vec<Vec<f32>>, Error> {
        if which.map_or(false, |w| w.len() != self.n_rows as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "FirStream::finish: one mark per row".to_string() });
        }
        let marks: Option<Vec<u8>> = which.map(|w| w.iter().map(|&m| m as u8).collect());
        Ok(self.call(None, marks.as_deref())?.0)
    }
}

impl Drop for FirStream<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_filter_stream_close(self.gpu.ctx, self.fs);
        }
    }
}

/// A set of recursive filters resident on a [`Gpu`]'s device ([`Gpu::iir_set`]); `grail_iir_free` when dropped.
pub struct IirSet<'a> {
    gpu: &'a Gpu,
    set: *mut sys::grail_iir,
}

impl Drop for IirSet<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_iir_free(self.gpu.ctx, self.set);
        }
    }
}

/// Rows filtered recursively chunk by chunk on a [`Gpu`]'s device ([`Gpu::iir_stream`]), their filters' state resident in HBM
/// between calls; `grail_iir_stream_close` when dropped.
pub struct IirStream<'a> {
    gpu: &'a Gpu,
    is: *mut sys::grail_iir_stream,
    n_rows: u32,
    tail: u32,
    _set: &'a IirSet<'a>,
}

impl IirStream<'_> {
    // one call on the stream: `chunks` fed (None: the rows marked in `which` finish); the outputs and the counts per row
    fn call(&mut self, chunks: Option<&[Vec<f32>]>, which: Option<&[u8]>) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        let n = self.n_rows as usize;
        let longest = chunks.map_or(0, |c| c.iter().map(|r| r.len()).max().unwrap_or(0));
        let stride = (longest + 63) / 64 * 64;
        let out_stride = (longest.max(self.tail as usize) + 63) / 64 * 64;
        let lens: Vec<u32> = chunks.map_or(vec![0u32; n], |c| c.iter().map(|r| r.len() as u32).collect());
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let sizes = [n * stride.max(1) * 4, n * out_stride.max(1) * 4, n * 4, n * 4, n * 4];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, sizes[k], &mut d[k]));
                }
            }
            if let Some(c) = chunks {
                for (i, row) in c.iter().enumerate() {
                    if r.is_ok() && !row.is_empty() {
                        r = check(sys::grail_memcpy_h2d(ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                        row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                    }
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_h2d(ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
                }
                if r.is_ok() {
                    r = check(sys::grail_iir_stream_next_async(ctx, self.is, d[0] as *const f32, stride as u64, d[2] as *const u32,
                                                               d[1] as *mut f32, out_stride as u64, d[3] as *mut u32,
                                                               d[4] as *mut u32));
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_d2h(ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
                }
            } else if r.is_ok() {
                r = check(sys::grail_iir_stream_finish_async(ctx, self.is, which.map_or(std::ptr::null(), |w| w.as_ptr()),
                                                             d[1] as *mut f32, out_stride as u64, d[3] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 && out_lens[i] != LIMIT_REFUSED {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad))
    }

    /// Feeds row `i` the samples `chunks[i]` (an empty chunk: the row pauses) and returns, per row, as many outputs and the
    /// count of non-finite samples among those fed (`grail_iir_stream_next_async`).  A row that has ended and is fed comes
    /// back empty, its state untouched.
    pub fn next(&mut self, chunks: &[Vec<f32>]) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        if chunks.len() != self.n_rows as usize {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "IirStream::next: one chunk per row".to_string() });
        }
        self.call(Some(chunks), None)
    }

    /// Ends the rows marked in `which` (`None`: every row) and returns their tails: what the filter still rings out over the
    /// stream's `tail` outputs with +0.0 to come (`grail_iir_stream_finish_async`); empty for rows not marked, rows ended
    /// before and rows that were fed nothing.
    pub fn finish(&mut self, which: Option<&[bool]>) -> Result<Vec<Vec<f32>>, Error> {
        if which.map_or(false, |w| w.len() != self.n_rows as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "IirStream::finish: one mark per row".to_string() });
        }
        let marks: Option<Vec<u8>> = which.map(|w| w.iter().map(|&m| m as u8).collect());
        Ok(self.call(None, marks.as_deref())?.0)
    }
}

impl Drop for IirStream<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_iir_stream_close(self.gpu.ctx, self.is);
        }
    }
}

/// One gain curve of a [`DynSet`]: [`DYN_POINTS`] gains over the levels of the envelope, `[alpha_attack, alpha_release]`, and the
/// detector (`sys::GRAIL_DYN_PEAK` or `sys::GRAIL_DYN_SQUARE`).
#[derive(Clone, Debug)]
pub struct DynCurve {
    pub gain: Vec<f64>,
    pub alpha: [f64; 2],
    pub detector: i32,
}

/// A set of gain curves resident on a [`Gpu`]'s device ([`Gpu::dyn_set`]); `grail_dyn_free` when dropped.
pub struct DynSet<'a> {
    gpu: &'a Gpu,
    set: *mut sys::grail_dyn,
}

impl Drop for DynSet<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_dyn_free(self.gpu.ctx, self.set);
        }
    }
}

/// Self-keyed rows compressed chunk by chunk on a [`Gpu`]'s device ([`Gpu::dyn_stream`]), their envelopes resident in HBM
/// between calls; `grail_dyn_stream_close` when dropped.
pub struct DynStream<'a> {
    gpu: &'a Gpu,
    ds: *mut sys::grail_dyn_stream,
    n_rows: u32,
    _set: &'a DynSet<'a>,
}

impl DynStream<'_> {
    /// Feeds row `i` the samples `chunks[i]` (an empty chunk: the row pauses) and returns, per row, as many outputs, the count
    /// of non-finite samples among those fed and the smallest gain of the call (1.0 for an empty chunk)
    /// (`grail_dyn_stream_next_async`).
    pub fn next(&mut self, chunks: &[Vec<f32>]) -> Result<(Vec<Vec<f32>>, Vec<u32>, Vec<f64>), Error> {
        let n = self.n_rows as usize;
        if chunks.len() != n {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "DynStream::next: one chunk per row".to_string() });
        }
        let longest = chunks.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = (longest + 63) / 64 * 64;
        let lens: Vec<u32> = chunks.iter().map(|r| r.len() as u32).collect();
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut bad = vec![0u32; n];
        let mut min_gain = vec![1f64; n];
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let sizes = [n * stride.max(1) * 4, n * stride.max(1) * 4, n * 4, n * 4, n * 8];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in chunks.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_dyn_stream_next_async(ctx, self.ds, d[0] as *const f32, stride as u64, d[2] as *const u32,
                                                           std::ptr::null(), 0, d[1] as *mut f32, stride as u64, std::ptr::null_mut(),
                                                           d[3] as *mut u32, d[4] as *mut f64));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, min_gain.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 8));
            }
            for i in 0..n {
                if r.is_ok() && lens[i] != 0 {          // (a dynamics stream writes as many outputs as it is fed samples)
                    out[i] = vec![0f32; lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * stride) as *const std::ffi::c_void, lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad, min_gain))
    }
}

impl Drop for DynStream<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_dyn_stream_close(self.gpu.ctx, self.ds);
        }
    }
}

/// Rows resampled chunk by chunk on a [`Gpu`]'s device ([`Gpu::resample_stream`]), their history and their place between
/// two output samples resident in HBM between calls; `grail_resample_stream_close` when dropped.
pub struct ResampleStream<'a> {
    gpu: &'a Gpu,
    rs: *mut sys::grail_resample_stream,
    n_rows: u32,
    up: u32,
    down: u32,
    taps: u32,
}

impl ResampleStream<'_> {
    // the most outputs of a call that feeds `n` samples: ceil(n up / down)
    fn most(&self, n: usize) -> usize {
        ((n as u128 * self.up as u128 + (self.down as u128 - 1)) / self.down as u128) as usize
    }

    // one call on the stream: `chunks` fed (None: the rows marked in `which` finish); the outputs and the counts per row
    fn call(&mut self, chunks: Option<&[Vec<f32>]>, which: Option<&[u8]>) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        let n = self.n_rows as usize;
        let longest = chunks.map_or(0, |c| c.iter().map(|r| r.len()).max().unwrap_or(0));
        let stride = (longest + 63) / 64 * 64;
        let out_stride = (self.most(stride).max(self.most(self.taps as usize / 2)) + 63) / 64 * 64;
        let lens: Vec<u32> = chunks.map_or(vec![0u32; n], |c| c.iter().map(|r| r.len() as u32).collect());
        let mut out: Vec<Vec<f32>> = vec![Vec::new(); n];
        let mut out_lens = vec![0u32; n];
        let mut bad = vec![0u32; n];
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let sizes = [n * stride.max(1) * 4, n * out_stride.max(1) * 4, n * 4, n * 4, n * 4];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, sizes[k], &mut d[k]));
                }
            }
            if let Some(c) = chunks {
                for (i, row) in c.iter().enumerate() {
                    if r.is_ok() && !row.is_empty() {
                        r = check(sys::grail_memcpy_h2d(ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                        row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                    }
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_h2d(ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
                }
                if r.is_ok() {
                    r = check(sys::grail_resample_stream_next_async(ctx, self.rs, d[0] as *const f32, stride as u64, d[2] as *const u32,
                                                                    d[1] as *mut f32, out_stride as u64, d[3] as *mut u32,
                                                                    d[4] as *mut u32));
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_d2h(ctx, bad.as_mut_ptr() as *mut std::ffi::c_void, d[4], n * 4));
                }
            } else if r.is_ok() {
                r = check(sys::grail_resample_stream_finish_async(ctx, self.rs, which.map_or(std::ptr::null(), |w| w.as_ptr()),
                                                                  d[1] as *mut f32, out_stride as u64, d[3] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], n * 4));
            }
            for i in 0..n {
                if r.is_ok() && out_lens[i] != 0 && out_lens[i] != LIMIT_REFUSED {
                    out[i] = vec![0f32; out_lens[i] as usize];
                    r = check(sys::grail_memcpy_d2h(ctx, out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    out_lens[i] as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
        }
        Ok((out, bad))
    }

    /// Feeds row `i` the samples `chunks[i]` (an empty chunk: the row pauses) and returns, per row, the outputs that became
    /// known and the count of non-finite samples among those fed (`grail_resample_stream_next_async`).  A row that has
    /// ended and is fed comes back empty, its state untouched.
    pub fn next(&mut self, chunks: &[Vec<f32>]) -> Result<(Vec<Vec<f32>>, Vec<u32>), Error> {
        if chunks.len() != self.n_rows as usize {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "ResampleStream::next: one chunk per row".to_string() });
        }
        self.call(Some(chunks), None)
    }

    /// Ends the rows marked in `which` (`None`: every row) and returns their tails: the outputs that still read samples
    /// fed, with +0.0 to come (`grail_resample_stream_finish_async`); empty for rows not marked and rows ended before.
    pub fn finish(&mut self, which: Option<&[bool]>) -> Result<Vec<Vec<f32>>, Error> {
        if which.map_or(false, |w| w.len() != self.n_rows as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "ResampleStream::finish: one mark per row".to_string() });
        }
        let marks: Option<Vec<u8>> = which.map(|w| w.iter().map(|&m| m as u8).collect());
        Ok(self.call(None, marks.as_deref())?.0)
    }
}

impl Drop for ResampleStream<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_resample_stream_close(self.gpu.ctx, self.rs);
        }
    }
}

/// What one call on a [`LimitStream`] gives: per row the outputs that became known (empty for the rows of a refused
/// group), per group the smallest gain and the count of limited samples among them and the count of non-finite samples
/// among those fed.
pub struct LimitChunk {
    pub out: Vec<Vec<f32>>,
    pub min_gain: Vec<f32>,
    pub n_limited: Vec<u32>,
    pub nonfinite: Vec<u32>,
}

/// Groups of rows limited chunk by chunk on a [`Gpu`]'s device ([`Gpu::limit_stream`]), their look-ahead resident in HBM
/// between calls; `grail_limit_stream_close` when dropped.
pub struct LimitStream<'a> {
    gpu: &'a Gpu,
    ls: *mut sys::grail_limit_stream,
    n_rows: u32,
    group: u32,
    delay: u32,
}

impl LimitStream<'_> {
    /// The samples the output lags the input by: `GRAIL_LIMIT_STREAM_DELAY`.
    pub fn delay(&self) -> u32 {
        self.delay
    }

    // one call on the stream: `chunks` fed (None: the groups marked in `which` finish)
    fn call(&mut self, chunks: Option<&[Vec<f32>]>, which: Option<&[u8]>) -> Result<LimitChunk, Error> {
        let n = self.n_rows as usize;
        let groups = (self.n_rows / self.group) as usize;
        let longest = chunks.map_or(0, |c| c.iter().map(|r| r.len()).max().unwrap_or(0));
        let stride = (longest + 63) / 64 * 64;
        let out_stride = (stride.max(self.delay as usize) + 63) / 64 * 64;
        let lens: Vec<u32> = chunks.map_or(vec![0u32; n], |c| c.iter().map(|r| r.len() as u32).collect());
        let mut res = LimitChunk { out: vec![Vec::new(); n], min_gain: vec![1f32; groups], n_limited: vec![0u32; groups],
                                   nonfinite: vec![0u32; groups] };
        let mut out_lens = vec![0u32; groups];
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: [*mut std::ffi::c_void; 7] = [std::ptr::null_mut(); 7];
            let sizes = [n * stride.max(1) * 4, n * out_stride * 4, n * 4, groups * 4, groups * 4, groups * 4, groups * 4];
            let mut r = Ok(());
            for k in 0..7 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, sizes[k], &mut d[k]));
                }
            }
            if let Some(c) = chunks {
                for (i, row) in c.iter().enumerate() {
                    if r.is_ok() && !row.is_empty() {
                        r = check(sys::grail_memcpy_h2d(ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                        row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                    }
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_h2d(ctx, d[2], lens.as_ptr() as *const std::ffi::c_void, n * 4));
                }
                if r.is_ok() {
                    r = check(sys::grail_limit_stream_next_async(ctx, self.ls, d[0] as *const f32, stride as u64, d[2] as *const u32,
                                                                 d[1] as *mut f32, out_stride as u64, d[3] as *mut u32,
                                                                 d[4] as *mut f32, d[5] as *mut u32, d[6] as *mut u32));
                }
                if r.is_ok() {
                    r = check(sys::grail_memcpy_d2h(ctx, res.nonfinite.as_mut_ptr() as *mut std::ffi::c_void, d[6], groups * 4));
                }
            } else if r.is_ok() {
                r = check(sys::grail_limit_stream_finish_async(ctx, self.ls, which.map_or(std::ptr::null(), |w| w.as_ptr()),
                                                               d[1] as *mut f32, out_stride as u64, d[3] as *mut u32,
                                                               d[4] as *mut f32, d[5] as *mut u32));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, out_lens.as_mut_ptr() as *mut std::ffi::c_void, d[3], groups * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, res.min_gain.as_mut_ptr() as *mut std::ffi::c_void, d[4], groups * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_d2h(ctx, res.n_limited.as_mut_ptr() as *mut std::ffi::c_void, d[5], groups * 4));
            }
            for i in 0..n {
                let len = out_lens[i / self.group as usize];
                if r.is_ok() && len != 0 && len != LIMIT_REFUSED {
                    res.out[i] = vec![0f32; len as usize];
                    r = check(sys::grail_memcpy_d2h(ctx, res.out[i].as_mut_ptr() as *mut std::ffi::c_void,
                                                    (d[1] as *const f32).add(i * out_stride) as *const std::ffi::c_void,
                                                    len as usize * 4));
                }
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
        }
        Ok(res)
    }

    /// Feeds row `i` the samples `chunks[i]` (empty chunks: the group pauses) and returns what became known
    /// (`grail_limit_stream_next_async`).  A group whose members are fed different lengths, or that has ended and is fed,
    /// is refused for the call: its rows come back empty, its `min_gain` NaN, its state untouched.
    pub fn next(&mut self, chunks: &[Vec<f32>]) -> Result<LimitChunk, Error> {
        if chunks.len() != self.n_rows as usize {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "LimitStream::next: one chunk per row".to_string() });
        }
        self.call(Some(chunks), None)
    }

    /// Ends the groups marked in `which` (`None`: every group) and returns their tails, the last `delay()` outputs at most
    /// (`grail_limit_stream_finish_async`); empty for groups not marked and groups ended before.
    pub fn finish(&mut self, which: Option<&[bool]>) -> Result<LimitChunk, Error> {
        if which.map_or(false, |w| w.len() != (self.n_rows / self.group) as usize) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "LimitStream::finish: one mark per group".to_string() });
        }
        let marks: Option<Vec<u8>> = which.map(|w| w.iter().map(|&m| m as u8).collect());
        self.call(None, marks.as_deref())
    }
}

impl Drop for LimitStream<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_limit_stream_close(self.gpu.ctx, self.ls);
        }
    }
}

/// The outputs a call on a [`LimitStream`] writes for a group that was fed `fed_before` samples before it: a `next` call
/// that feeds `n` samples, or (`finishing`, `n` = 0) the tail (`grail_limit_stream_len`; pure host).
pub fn limit_stream_len(fed_before: u64, n: u64, lookahead_log2: u32, finishing: bool) -> Result<u64, Error> {
    let mut n_out = 0u64;
    check(unsafe { sys::grail_limit_stream_len(fed_before, n, lookahead_log2, finishing as i32, &mut n_out) })?;
    Ok(n_out)
}

/// What one call on a [`MeterStream`] gives, per row: the hop sums the call completed, the largest true-peak output among
/// the call's own, the count of non-finite samples fed.  A refused row: no hops, a NaN peak, `refused[i]` set.
pub struct MeterChunk {
    pub hop_sumsq: Vec<Vec<f64>>,
    pub true_peak: Vec<f64>,
    pub nonfinite: Vec<u32>,
    pub refused: Vec<bool>,
}

/// What a [`MeterStream`] shows of its rows at one moment (`grail_meter_stream_read_async`): mean squares (see
/// [`loudness_lufs`]), the running true peak and the hops completed.
pub struct MeterReading {
    pub integrated_ms: Vec<f64>,
    pub momentary_ms: Vec<f64>,
    pub short_term_ms: Vec<f64>,
    pub true_peak: Vec<f64>,
    pub hops: Vec<u64>,
}

/// Rows metered chunk by chunk on a [`Gpu`]'s device ([`Gpu::meter_stream`]), the filter's state, the running peak and the
/// ledger of hop sums resident in HBM between calls; `grail_meter_stream_close` when dropped.
pub struct MeterStream<'a> {
    gpu: &'a Gpu,
    ms: *mut sys::grail_meter_stream,
    n_rows: u32,
    hop: u32,
}

impl MeterStream<'_> {
    // `count` elements of `T` from device memory
    unsafe fn down<T: Clone + Default>(&self, src: *const std::ffi::c_void, count: usize) -> Result<Vec<T>, Error> {
        let mut v = vec![T::default(); count];
        check(sys::grail_memcpy_d2h(self.gpu.ctx, v.as_mut_ptr() as *mut std::ffi::c_void, src, count * std::mem::size_of::<T>()))?;
        Ok(v)
    }

    /// Feeds row `i` the samples `chunks[i]` (an empty chunk: the row pauses; `grail_meter_stream_next_async`).
    pub fn next(&mut self, chunks: &[Vec<f32>]) -> Result<MeterChunk, Error> {
        let n = self.n_rows as usize;
        if chunks.len() != n {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "MeterStream::next: one chunk per row".to_string() });
        }
        let longest = chunks.iter().map(|r| r.len()).max().unwrap_or(0);
        let stride = ((longest + 63) / 64 * 64).max(64);
        let hops_stride = (stride + self.hop as usize - 1) / self.hop as usize;
        let lens: Vec<u32> = chunks.iter().map(|r| r.len() as u32).collect();
        let ctx = self.gpu.ctx;
        let mut res = MeterChunk { hop_sumsq: vec![Vec::new(); n], true_peak: Vec::new(), nonfinite: Vec::new(), refused: vec![false; n] };
        unsafe {
            let mut d: [*mut std::ffi::c_void; 6] = [std::ptr::null_mut(); 6];
            let sizes = [n * stride * 4, n * 4, n * hops_stride * 8, n * 4, n * 8, n * 4];
            let mut r = Ok(());
            for k in 0..6 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, sizes[k], &mut d[k]));
                }
            }
            for (i, row) in chunks.iter().enumerate() {
                if r.is_ok() && !row.is_empty() {
                    r = check(sys::grail_memcpy_h2d(ctx, (d[0] as *mut f32).add(i * stride) as *mut std::ffi::c_void,
                                                    row.as_ptr() as *const std::ffi::c_void, row.len() * 4));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_memcpy_h2d(ctx, d[1], lens.as_ptr() as *const std::ffi::c_void, n * 4));
            }
            if r.is_ok() {
                r = check(sys::grail_meter_stream_next_async(ctx, self.ms, d[0] as *const f32, stride as u64, d[1] as *const u32,
                                                             d[2] as *mut f64, hops_stride as u64, d[3] as *mut u32,
                                                             d[4] as *mut f64, d[5] as *mut u32));
            }
            let mut got = Ok(());
            if r.is_ok() {
                got = (|| {
                    let n_hops: Vec<u32> = self.down(d[3], n)?;
                    res.true_peak = self.down(d[4], n)?;
                    res.nonfinite = self.down(d[5], n)?;
                    for i in 0..n {
                        res.refused[i] = n_hops[i] == LIMIT_REFUSED;
                        if !res.refused[i] && n_hops[i] != 0 {
                            res.hop_sumsq[i] = self.down((d[2] as *const f64).add(i * hops_stride) as *const std::ffi::c_void,
                                                         n_hops[i] as usize)?;
                        }
                    }
                    Ok(())
                })();
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
            got?;
        }
        Ok(res)
    }

    /// What the meter shows of every row now (`grail_meter_stream_read_async`); changes no state.
    pub fn read(&self) -> Result<MeterReading, Error> {
        let n = self.n_rows as usize;
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: [*mut std::ffi::c_void; 5] = [std::ptr::null_mut(); 5];
            let mut r = Ok(());
            for k in 0..5 {
                if r.is_ok() {
                    r = check(sys::grail_device_alloc(ctx, n * 8, &mut d[k]));
                }
            }
            if r.is_ok() {
                r = check(sys::grail_meter_stream_read_async(ctx, self.ms, d[0] as *mut f64, d[1] as *mut f64, d[2] as *mut f64,
                                                             d[3] as *mut f64, d[4] as *mut u64));
            }
            let mut got = Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: String::new() });
            if r.is_ok() {
                got = (|| {
                    Ok(MeterReading { integrated_ms: self.down(d[0], n)?, momentary_ms: self.down(d[1], n)?,
                                      short_term_ms: self.down(d[2], n)?, true_peak: self.down(d[3], n)?, hops: self.down(d[4], n)? })
                })();
            }
            for p in d {
                if !p.is_null() {
                    sys::grail_device_free(ctx, p);
                }
            }
            r?;
            got
        }
    }

    /// Row `row`'s hop sums so far, copied from the ledger (`grail_meter_stream_ledger`): what [`loudness_range`] and
    /// [`loudness_window_max`] take.
    pub fn ledger(&self, row: u32) -> Result<Vec<f64>, Error> {
        if row >= self.n_rows {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "MeterStream::ledger: no such row".to_string() });
        }
        let hops = self.read()?.hops[row as usize] as usize;
        let mut base: *const f64 = std::ptr::null();
        let mut stride = 0u64;
        check(unsafe { sys::grail_meter_stream_ledger(self.gpu.ctx, self.ms, &mut base, &mut stride) })?;
        unsafe { self.down(base.add(row as usize * stride as usize) as *const std::ffi::c_void, hops) }
    }

    /// Ends the rows marked in `which` (`None`: every row) and returns, per row, the largest of the eleven true-peak
    /// outputs after its last sample (`grail_meter_stream_finish_async`); 0 for rows not marked and rows ended before.
    pub fn finish(&mut self, which: Option<&[bool]>) -> Result<Vec<f64>, Error> {
        let n = self.n_rows as usize;
        if which.map_or(false, |w| w.len() != n) {
            return Err(Error { status: sys::GRAIL_ERR_INVALID_ARG, message: "MeterStream::finish: one mark per row".to_string() });
        }
        let marks: Option<Vec<u8>> = which.map(|w| w.iter().map(|&m| m as u8).collect());
        let ctx = self.gpu.ctx;
        unsafe {
            let mut d: *mut std::ffi::c_void = std::ptr::null_mut();
            check(sys::grail_device_alloc(ctx, n * 8, &mut d))?;
            let mut r = check(sys::grail_meter_stream_finish_async(ctx, self.ms, marks.as_deref().map_or(std::ptr::null(), |w| w.as_ptr()),
                                                                   d as *mut f64));
            let mut peaks = Vec::new();
            if r.is_ok() {
                match self.down::<f64>(d, n) {
                    Ok(v) => peaks = v,
                    Err(e) => r = Err(e),
                }
            }
            sys::grail_device_free(ctx, d);
            r?;
            Ok(peaks)
        }
    }
}

impl Drop for MeterStream<'_> {
    fn drop(&mut self) {
        unsafe {
            sys::grail_meter_stream_close(self.gpu.ctx, self.ms);
        }
    }
}

/// The hops a call on a [`MeterStream`] completes for a row that was fed `fed_before` samples before it and is fed `n`
/// (`grail_meter_stream_hops`; pure host).
pub fn meter_stream_hops(fed_before: u64, n: u64, sample_rate: u32) -> Result<u64, Error> {
    let mut n_hops = 0u64;
    check(unsafe { sys::grail_meter_stream_hops(fed_before, n, sample_rate, &mut n_hops) })?;
    Ok(n_hops)
}

/// The outputs a call on a [`ResampleStream`] writes for a row that was fed `fed_before` samples before it: a `next` call
/// that feeds `n` samples, or (`finishing`, `n` = 0) the tail (`grail_resample_stream_len`; pure host).
pub fn resample_stream_len(fed_before: u64, n: u64, rate_in: u32, rate_out: u32, finishing: bool) -> Result<u64, Error> {
    let mut n_out = 0u64;
    check(unsafe { sys::grail_resample_stream_len(fed_before, n, rate_in, rate_out, finishing as i32, &mut n_out) })?;
    Ok(n_out)
}

/// The outputs a call on a [`FirStream`] writes for a row that was fed `fed_before` samples before it: a `next` call that
/// feeds `n` samples, or (`finishing`, `n` = 0) the tail (`grail_filter_stream_len`; pure host).
pub fn fir_stream_len(fed_before: u64, n: u64, n_taps: u32, origin: u32, finishing: bool) -> Result<u64, Error> {
    let mut n_out = 0u64;
    check(unsafe { sys::grail_filter_stream_len(fed_before, n, n_taps, origin, finishing as i32, &mut n_out) })?;
    Ok(n_out)
}

/// The most taps of a filter, the most filters of a set (`GRAIL_FIR_TAPS_MAX`, `GRAIL_FIR_FILTERS_MAX`).
pub const FIR_TAPS_MAX: u32 = sys::GRAIL_FIR_TAPS_MAX;
pub const FIR_FILTERS_MAX: u32 = sys::GRAIL_FIR_FILTERS_MAX;

/// One biquad section `[b0, b1, b2, a1, a2]` of `kind` (`sys::GRAIL_IIR_LOWPASS` ... `sys::GRAIL_IIR_HIGHSHELF`) at `f0_hz`
/// with quality `q`; `gain_db` is read by the shelves and the peak (`grail_iir_design`; pure host).
pub fn iir_design(kind: i32, sample_rate: u32, f0_hz: f64, q: f64, gain_db: f64) -> Result<[f64; 5], Error> {
    let mut coef = [0f64; 5];
    check(unsafe { sys::grail_iir_design(kind, sample_rate, f0_hz, q, gain_db, coef.as_mut_ptr()) })?;
    Ok(coef)
}

/// The gains of one curve, and the most curves of a set (`GRAIL_DYN_POINTS`, `GRAIL_DYN_CURVES_MAX`).
pub const DYN_POINTS: usize = sys::GRAIL_DYN_POINTS as usize;
pub const DYN_CURVES_MAX: u32 = sys::GRAIL_DYN_CURVES_MAX;

/// The gain curve of a soft-knee compressor (`sys::GRAIL_DYN_COMPRESS`) or of its mirror below the threshold, a downward
/// expander held at `range_db` (`sys::GRAIL_DYN_EXPAND`), over the levels of `detector`'s envelope: [`DYN_POINTS`] gains
/// (`grail_dyn_design`; pure host).
pub fn dyn_design(kind: i32, detector: i32, threshold_db: f64, ratio: f64, knee_db: f64, range_db: f64, makeup_db: f64) -> Result<Vec<f64>, Error> {
    let mut gain = vec![0f64; DYN_POINTS];
    check(unsafe { sys::grail_dyn_design(kind, detector, threshold_db, ratio, knee_db, range_db, makeup_db, gain.as_mut_ptr()) })?;
    Ok(gain)
}

/// `[alpha_attack, alpha_release]` of an envelope that covers 1 - 1/e of a step in `attack_ms` on the way up and `release_ms`
/// on the way down, 0.0 for a time of 0 (`grail_dyn_ballistics`; pure host).
pub fn dyn_ballistics(sample_rate: u32, attack_ms: f64, release_ms: f64) -> Result<[f64; 2], Error> {
    let mut alpha = [0f64; 2];
    check(unsafe { sys::grail_dyn_ballistics(sample_rate, attack_ms, release_ms, alpha.as_mut_ptr()) })?;
    Ok(alpha)
}

/// The block transition matrix of one filter, `[2 S][2 S]` row-major: state `i` (`s1[0] s2[0] s1[1] ...`) after 1024 steps on
/// +0.0 input from the unit state `c`, at `i * 2 S + c` (`grail_biquad_block_matrix`; pure host).  It is what
/// [`Gpu::iir_blocked`] carries a row's state from block to block with.
pub fn iir_block_matrix(sections: &[[f64; 5]]) -> Result<Vec<f64>, Error> {
    let coef: Vec<f64> = sections.iter().flat_map(|s| s.iter().copied()).collect();
    let mut matrix = vec![0f64; 4 * sections.len() * sections.len()];
    check(unsafe { sys::grail_biquad_block_matrix(coef.as_ptr(), sections.len() as u32, matrix.as_mut_ptr()) })?;
    Ok(matrix)
}

/// The outputs a call on an [`IirStream`] writes for a row that was fed `fed_before` samples before it: a `next` call that
/// feeds `n` samples, or (`finishing`, `n` = 0) the finish (`grail_iir_stream_len`; pure host).
pub fn iir_stream_len(fed_before: u64, n: u64, tail: u32, finishing: bool) -> Result<u64, Error> {
    let mut n_out = 0u64;
    check(unsafe { sys::grail_iir_stream_len(fed_before, n, tail, finishing as i32, &mut n_out) })?;
    Ok(n_out)
}

/// The length of a row of `n` samples filtered: 0 for `n` = 0, else `n + n_taps - 1 - origin` (`grail_fir_len`; pure host).
pub fn fir_len(n: u64, n_taps: u32, origin: u32) -> Result<u64, Error> {
    let mut n_out = 0u64;
    check(unsafe { sys::grail_fir_len(n, n_taps, origin, &mut n_out) })?;
    Ok(n_out)
}

/// The Kaiser-windowed band-pass `lo_hz .. hi_hz` at `sample_rate`, `n_taps` odd (`grail_fir_design`; pure host): the taps and
/// the origin, `(n_taps - 1) / 2`, that gives the filter zero delay.  `lo_hz` = 0: a low-pass; `hi_hz` = `sample_rate / 2`: a
/// high-pass.
pub fn fir_design(sample_rate: u32, lo_hz: f64, hi_hz: f64, n_taps: u32) -> Result<(Vec<f32>, u32), Error> {
    let mut taps = vec![0f32; n_taps.max(1) as usize];
    check(unsafe { sys::grail_fir_design(sample_rate, lo_hz, hi_hz, n_taps, taps.as_mut_ptr()) })?;
    Ok((taps, (n_taps - 1) / 2))
}

/// The `f32` that a ceiling in dBTP is to [`Gpu::limit`] (`grail_limit_ceiling`; pure host).
pub fn limit_ceiling(ceiling_db: f32) -> f32 {
    unsafe { sys::grail_limit_ceiling(ceiling_db) }
}

/// Caps `gains` so that no item's row exceeds `ceiling_db` dBTP (`grail_true_peak_limit_gains`; pure host): item `i`
/// plays row `item_rows[i]`.  Returns the number of gains that were changed.
pub fn true_peak_limit_gains(true_peak: &[f64], item_rows: &[u32], ceiling_db: f32, gains: &mut [f32]) -> Result<u32, Error> {
    assert_eq!(item_rows.len(), gains.len());
    let mut limited = 0u32;
    check(unsafe {
        sys::grail_true_peak_limit_gains(true_peak.as_ptr(), true_peak.len() as u32, item_rows.as_ptr(),
                                         item_rows.len() as u32, ceiling_db, gains.as_mut_ptr(), &mut limited)
    })?;
    Ok(limited)
}

/// What "level" means to [`Gpu::mix_leveled`] (GRAIL_LEVEL_PEAK / _RMS / _ACTIVE / _LOUDNESS: targets then in LUFS).
#[derive(Copy, Clone, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum LevelMode {
    Peak = 0,
    Rms = 1,
    Active = 2,
    Loudness = 4,
}

/// The "active" level of one row from its frames' sums of squares (`grail_active_level`; pure host, no GPU).
pub fn active_level(frame_sumsq: &[f64], row_len: u32, frame: u32, floor_db: f32) -> f64 {
    assert!(frame > 0 && frame_sumsq.len() as u64 >= (row_len as u64 + frame as u64 - 1) / frame as u64);
    unsafe { sys::grail_active_level(frame_sumsq.as_ptr(), row_len, frame, floor_db) }
}

/// Predicted |fast - reference| of `voice` in units of 2^-23 of max(1, peak) (grail_fast_sharpness): narrow and
/// high formants amplify rounding-level differences of the filter coefficients.  Fast arithmetic is served up to
/// GRAIL_FAST_SHARPNESS_LIMIT = 28 (`voices::generic()`: 24).  Pure host function, no GPU.
pub fn fast_sharpness(voice: &Voice) -> f32 {
    unsafe { sys::grail_fast_sharpness(&voice_to_c(voice)) }
}

/// Warm-up length of `voice` for the time-split fast kernels in samples (0: the voice does not qualify).
pub fn time_split_warmup(voice: &Voice) -> u32 {
    unsafe { sys::grail_time_split_warmup(&voice_to_c(voice)) }
}

/// The lazy source of `examples/interactive.rs:31-48` on the GPU: ONE chain for a whole session.  Segments are
/// appended while samples are pulled; a Sequencer that needs a segment which has not been appended yet pauses
/// (`src/lib.rs:866-888` pulls `iter.next()` on demand) and `next` comes back short — the front end then feeds it, a
/// `Phoneme::Silence` when no text is waiting, as the reference's `repeat_with(|| receiver.try_recv().unwrap_or(' '))`
/// does.  Carrier phase, noise seed, jitter and filter state carry across everything appended: the samples are those
/// of the CPU iterator chain over the concatenated list, bit for bit.
pub struct LiveStream<'a> {
    gpu: &'a Gpu,
    stream: *mut sys::grail_stream,
    d_out: *mut std::ffi::c_void,
    d_len: *mut std::ffi::c_void,
    chunk: u32,
    stride: u64,
}

impl<'a> LiveStream<'a> {
    /// `.sequence(voice).jitter(jitter_seed, voice).synthesize()` over a source that is still being written.
    pub fn new(gpu: &'a Gpu, chunk: u32, voice: u32, jitter_seed: u32) -> Result<Self, Error> {
        let stride = (chunk as u64 + 63) / 64 * 64;
        let mut s = LiveStream { gpu, stream: std::ptr::null_mut(), d_out: std::ptr::null_mut(),
                                 d_len: std::ptr::null_mut(), chunk, stride };
        unsafe {
            check(sys::grail_stream_open_live(gpu.ctx, 1, &voice, &jitter_seed, 0, 0, &mut s.stream))?;
            check(sys::grail_device_alloc(gpu.ctx, stride as usize * 4, &mut s.d_out))?;
            check(sys::grail_device_alloc(gpu.ctx, 4, &mut s.d_len))?;
        }
        Ok(s)
    }

    /// The source delivers: these segments follow what the chain already has.
    pub fn append(&mut self, phonemes: &[PhonemeElem]) -> Result<(), Error> {
        let segs: Vec<_> = phonemes.iter().map(|p| sys::grail_phoneme_elem {
            phoneme: p.phoneme as i32, length: p.length, blend_length: p.blend_length, frequency: p.frequency,
        }).collect();
        let offs = [0u32, segs.len() as u32];
        check(unsafe { sys::grail_stream_append(self.gpu.ctx, self.stream, segs.as_ptr(), offs.as_ptr()) })
    }

    /// The source has ended: what is pending is spoken, the last segment fades out, `next` then returns nothing.
    pub fn finish(&mut self) -> Result<(), Error> {
        check(unsafe { sys::grail_stream_finish(self.gpu.ctx, self.stream, std::ptr::null()) })
    }

    /// Segments appended that the Sequencer has not pulled yet.
    pub fn pending(&mut self) -> Result<u32, Error> {
        let mut n = 0u32;
        check(unsafe { sys::grail_stream_pending(self.gpu.ctx, self.stream, &mut n) })?;
        Ok(n)
    }

    /// `Iterator::next`, up to `chunk` samples at a time: fewer when the Sequencer waits for its source (or the
    /// chain has ended).
    pub fn next(&mut self) -> Result<Vec<f32>, Error> {
        let mut n = 0u32;
        unsafe {
            check(sys::grail_stream_next_async(self.gpu.ctx, self.stream, self.chunk, self.d_out as *mut f32,
                                               self.stride, self.d_len as *mut u32))?;
            check(sys::grail_sync(self.gpu.ctx))?;
            check(sys::grail_memcpy_d2h(self.gpu.ctx, &mut n as *mut u32 as *mut _, self.d_len, 4))?;
            let mut out = vec![0f32; n as usize];
            if n > 0 {
                check(sys::grail_memcpy_d2h(self.gpu.ctx, out.as_mut_ptr() as *mut _, self.d_out, n as usize * 4))?;
            }
            Ok(out)
        }
    }
}

impl Drop for LiveStream<'_> {
    fn drop(&mut self) {
        unsafe {
            if !self.stream.is_null() { sys::grail_stream_close(self.gpu.ctx, self.stream); }
            if !self.d_out.is_null() { sys::grail_device_free(self.gpu.ctx, self.d_out); }
            if !self.d_len.is_null() { sys::grail_device_free(self.gpu.ctx, self.d_len); }
        }
    }
}
