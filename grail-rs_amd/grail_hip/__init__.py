"""ctypes binding of libgrail_hip.so — the C ABI declared in include/grail_hip.h.

This is plumbing for tests and bench.py (the reference's own host language,
Rust, is not in this image; INTEGRATION.md has the Rust binding).  It holds no
arithmetic: every sample comes from the HIP kernels behind the C ABI, and
anything that needs the GPU raises GrailError when the library or a device is
missing — there is no CPU fallback.

Reference API mirrored (reference file:line):
  Voice src/lib.rs:696, SynthesisElem :316, PhonemeElem :961, SequenceElem :814,
  Phoneme :632, voices::generic() src/voices/generic.rs:5,
  .select().sequence().jitter().synthesize() src/lib.rs:1013/941/786/587.
"""
import ctypes as C
import os

import numpy as np

NUM_FORMANTS = 8
DEFAULT_SAMPLE_RATE = 44100.0

PH_SILENCE, PH_STOP, PH_GLIDE, PH_A, PH_E = range(5)
PH_COUNT = 5
NUM_VOICED = 2

OK = 0
ERR_INVALID_ARG = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_BUFFER_TOO_SMALL = -4
ERR_OUT_OF_MEMORY = -5
ERR_RCCL = -6
ERR_NO_VOICES = -7

OUT_HOST = 0
OUT_DEVICE = 1
# "arithmetic" = 1 (fast mode): GRAIL_FAST_TOLERANCE of include/grail_hip.h
FAST_TOLERANCE_ULPS = 64
FAST_TOLERANCE = FAST_TOLERANCE_ULPS * 2.0 ** -23
FAST_SHARPNESS_LIMIT = 28.0      # GRAIL_FAST_SHARPNESS_LIMIT
FAST_TOLERANCE_NOTE = (f"fast mode: max |fast - exact| <= {FAST_TOLERANCE_ULPS} * 2^-23 = {FAST_TOLERANCE:.3g} of "
                       "full scale vs the oracle (tests/test_fast_gpu.py asserts it on configs 2, 3, 4 "
                       "and a fuzz corpus); clock, phases, wraps and LCGs stay exact")
UNIQUE_ID_BYTES = 128
ABI_VERSION = 4                  # GRAIL_ABI_VERSION of the header this binding mirrors

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GRAIL_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib",
                                                         "libgrail_hip.so")

# every symbol include/grail_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "grail_abi_version", "grail_status_string", "grail_last_error",
    "grail_elem_silent", "grail_elem_new_phoneme", "grail_elem_new", "grail_elem_resample",
    "grail_elem_blend", "grail_voice_generic", "grail_voice_generic_at", "grail_voice_get",
    "grail_create", "grail_destroy", "grail_device_count", "grail_device_pci_bus_id", "grail_time_split_warmup", "grail_length_bound",
    "grail_time_split_grid", "grail_fast_sharpness", "grail_plan_blocks", "grail_plan_ragged_blocks", "grail_dispatch_model",
    "grail_packed_launch_order", "grail_set_voices",
    "grail_get_voices", "grail_set_option", "grail_get_option",
    "grail_batch_upload", "grail_batch_upload_elems", "grail_batch_free", "grail_batch_size",
    "grail_batch_lengths", "grail_batch_synthesize_async", "grail_sync",
    "grail_last_kernel_ms", "grail_last_kernel_name", "grail_synthesize_batch", "grail_synthesize_batch_elems",
    "grail_stream_open", "grail_stream_next_async", "grail_stream_close",
    "grail_stream_open_live", "grail_stream_append", "grail_stream_append_elems", "grail_stream_finish", "grail_stream_pending",
    "grail_language_generic", "grail_transcribe", "grail_intonate", "grail_text_to_phoneme_elems",
    "grail_synthesize_batch_pcm16", "grail_batch_synthesize_pcm16_async", "grail_stream_next_pcm16_async", "grail_say_batch", "grail_pcm16_async", "grail_batch_digest", "grail_batch_compare", "grail_wav_write_i16",
    "grail_device_alloc", "grail_device_free", "grail_host_alloc", "grail_host_free", "grail_memcpy_d2h", "grail_memcpy_h2d",
    "grail_memset_d", "grail_shard_range", "grail_comm_unique_id", "grail_comm_init",
    "grail_broadcast_voices", "grail_comm_info", "grail_comm_destroy",
    "grail_node_create", "grail_node_destroy", "grail_node_size", "grail_node_context", "grail_node_set_voices",
    "grail_node_set_option", "grail_node_get_option", "grail_node_shard_of", "grail_node_synthesize_batch",
    "grail_node_synthesize_batch_elems", "grail_node_synthesize_batch_pcm16", "grail_node_synthesize_batch_device",
    "grail_node_say_batch",
    "grail_node_lengths", "grail_node_last_shard_ms", "grail_node_host_alloc", "grail_node_host_free",
    "grail_mix_async", "grail_batch_mix", "grail_mix_place_sequential", "grail_pcm16_frames_async",
    "grail_wav_write_i16_frames",
    "grail_levels_async", "grail_frame_levels_async", "grail_level_gains", "grail_active_level", "grail_batch_mix_leveled",
    "grail_kweighting", "grail_loudness_async", "grail_gated_mean_square", "grail_loudness_lufs", "grail_loudness_level",
    "grail_loudness_segmented_async", "grail_loudness_window_max", "grail_loudness_range",
    "grail_true_peak_coefficients", "grail_true_peak_async", "grail_true_peak_db", "grail_true_peak_limit_gains",
    "grail_batch_mix_leveled_limited",
    "grail_limit_ceiling", "grail_limit_async",
    "grail_resample_ratio", "grail_resample_coefficients", "grail_resample_len", "grail_resample_async",
    "grail_fir_len", "grail_fir_design", "grail_fir_create", "grail_fir_free", "grail_fir_async",
    "grail_filter_stream_len", "grail_filter_stream_open", "grail_filter_stream_next_async", "grail_filter_stream_finish_async",
    "grail_filter_stream_close",
    "grail_resample_stream_len", "grail_resample_stream_open", "grail_resample_stream_next_async",
    "grail_resample_stream_finish_async", "grail_resample_stream_close",
    "grail_limit_stream_len", "grail_limit_stream_open", "grail_limit_stream_next_async", "grail_limit_stream_finish_async",
    "grail_limit_stream_close",
    "grail_meter_stream_hops", "grail_meter_stream_open", "grail_meter_stream_next_async", "grail_meter_stream_read_async",
    "grail_meter_stream_ledger", "grail_meter_stream_finish_async", "grail_meter_stream_close",
    "grail_iir_design", "grail_iir_create", "grail_iir_free", "grail_iir_async",
    "grail_biquad_blocked_async", "grail_biquad_block_matrix",
    "grail_iir_stream_len", "grail_iir_stream_open", "grail_iir_stream_next_async", "grail_iir_stream_finish_async",
    "grail_iir_stream_close",
    "grail_dyn_design", "grail_dyn_ballistics", "grail_dyn_create", "grail_dyn_free", "grail_dyn_async",
    "grail_track_dyn_async",
    "grail_dyn_stream_open", "grail_dyn_stream_next_async", "grail_dyn_stream_close",
]
MIX_ACCUMULATE = 1               # GRAIL_MIX_ACCUMULATE
LEVEL_PEAK, LEVEL_RMS, LEVEL_ACTIVE = 0, 1, 2    # GRAIL_LEVEL_*: what "level" means to level_gains / mix_leveled
LEVEL_FRAME = 4096               # GRAIL_LEVEL_FRAME: the frame length of the row totals
LEVEL_ACTIVE_FLOOR_DB = 40.0     # GRAIL_LEVEL_ACTIVE_FLOOR_DB
LEVEL_LOUDNESS = 4               # GRAIL_LEVEL_LOUDNESS: level = loudness_level(gated mean square), targets in LUFS
LOUDNESS_ABS_GATE = 1.1724653045822981e-07      # GRAIL_LOUDNESS_ABS_GATE: the mean square of -70 LUFS
LOUDNESS_LEVEL_SCALE = 0.8529037030705663       # GRAIL_LOUDNESS_LEVEL_SCALE: 10^(-0.691 / 10)
LOUDNESS_RATE_MIN, LOUDNESS_RATE_MAX = 2560, 1048576
LOUDNESS_WARMUP_HOPS = 3                        # GRAIL_LOUDNESS_WARMUP_HOPS: loudness_segmented starts a hop's filter 3 hops early
TRUE_PEAK_PHASES, TRUE_PEAK_TAPS = 4, 12        # GRAIL_TRUE_PEAK_*: the 4x oversampling filter of BS.1770-4 Annex 2
LIMIT_LOOKAHEAD_LOG2_MAX = 10                   # GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX: the look-ahead is 2^0 .. 2^10 samples
LIMIT_REFUSED = 0xFFFFFFFF                      # GRAIL_LIMIT_REFUSED: n_limited of a group whose members differ in length
LIMIT_CHUNK = 4096                              # GRAIL_LIMIT_CHUNK: one workgroup's samples (no number depends on it)


def limit_stream_delay(lookahead_log2):
    """GRAIL_LIMIT_STREAM_DELAY: the samples a limit stream's output lags its input by, 2^lookahead_log2 + 10"""
    return (1 << lookahead_log2) + 10


RESAMPLE_ZERO_CROSSINGS = 24                    # GRAIL_RESAMPLE_ZERO_CROSSINGS: per side, at the lower of the two rates
RESAMPLE_TABLE_MAX = 32768                      # GRAIL_RESAMPLE_TABLE_MAX: up * taps of a supported pair of rates
RESAMPLE_CHUNK = 1024                           # GRAIL_RESAMPLE_CHUNK: one workgroup's outputs (no number depends on it)
FIR_TAPS_MAX = 4096                             # GRAIL_FIR_TAPS_MAX: the taps of one filter
FIR_FILTERS_MAX = 64                            # GRAIL_FIR_FILTERS_MAX: the filters of one set
FIR_CHUNK = 2048                                # GRAIL_FIR_CHUNK: one workgroup's outputs (no number depends on it)
IIR_SECTIONS_MAX = 8                            # GRAIL_IIR_SECTIONS_MAX: the biquad sections of one recursive filter
IIR_FILTERS_MAX = 64                            # GRAIL_IIR_FILTERS_MAX: the filters of one set
IIR_BLOCK = 1024                                # GRAIL_BIQUAD_BLOCK: the steps of a block of grail_biquad_blocked_async
# GRAIL_IIR_*: the kinds grail_iir_design knows
IIR_LOWPASS, IIR_HIGHPASS, IIR_BANDPASS, IIR_NOTCH, IIR_PEAK, IIR_LOWSHELF, IIR_HIGHSHELF = range(7)
DYN_STEPS_PER_OCTAVE = 16                       # GRAIL_DYN_STEPS_PER_OCTAVE: the points of a gain curve an octave of the envelope
DYN_LOG2_LO, DYN_LOG2_HI = -32, 8               # GRAIL_DYN_LOG2_LO / _HI: the curve spans 2^-32 .. 2^8
DYN_POINTS = 641                                # GRAIL_DYN_POINTS: the gains of one curve
DYN_CURVES_MAX = 16                             # GRAIL_DYN_CURVES_MAX: the curves of one set
DYN_PEAK, DYN_SQUARE = 0, 1                     # GRAIL_DYN_PEAK / _SQUARE: what the envelope follows, |w| or w * w
DYN_COMPRESS, DYN_EXPAND = 0, 1                 # GRAIL_DYN_COMPRESS / _EXPAND: the kinds grail_dyn_design knows


class GrailError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"grail_hip status {status}: {message}")
        self.status = status


class SynthesisElem(C.Structure):
    _fields_ = [
        ("frequency", C.c_float),
        ("formant_freq", C.c_float * NUM_FORMANTS),
        ("formant_bw", C.c_float * NUM_FORMANTS),
        ("formant_smooth", C.c_float * NUM_FORMANTS),
        ("formant_breath", C.c_float * NUM_FORMANTS),
        ("formant_turb", C.c_float * NUM_FORMANTS),
        ("formant_amp", C.c_float * NUM_FORMANTS),
    ]

    def as_np(self):
        return np.frombuffer(bytes(self), dtype=np.float32).copy()

    @classmethod
    def from_np(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.size == 49
        return cls.from_buffer_copy(a.tobytes())


class Voice(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_float),
        ("phonemes", SynthesisElem * NUM_VOICED),
        ("center_frequency", C.c_float),
        ("jitter_frequency", C.c_float),
        ("jitter_delta_frequency", C.c_float),
        ("jitter_delta_formant_frequency", C.c_float),
        ("jitter_delta_amplitude", C.c_float),
    ]

    def copy(self):
        return Voice.from_buffer_copy(bytes(self))


class PhonemeElem(C.Structure):
    _fields_ = [
        ("phoneme", C.c_int32),
        ("length", C.c_float),
        ("blend_length", C.c_float),
        ("frequency", C.c_float),
    ]


class SequenceElem(C.Structure):
    _fields_ = [
        ("has_elem", C.c_int32),
        ("elem", SynthesisElem),
        ("length", C.c_float),
        ("blend_length", C.c_float),
    ]


class PlanBlock(C.Structure):
    """grail_plan_block: one kernel launch of a batch's plan (grail_plan_blocks)."""
    _fields_ = [
        ("rows", C.c_uint32),
        ("lanes_per_utterance", C.c_uint32),
        ("pipelined", C.c_uint32),
        ("chunks", C.c_uint32),
        ("scan", C.c_uint32),
        ("fast", C.c_uint32),
        ("formants", C.c_uint32),
        ("model_ms", C.c_float),
    ]

    def family(self):
        if self.scan:
            return f"scan{self.scan + 1}"
        if self.chunks:
            return f"split{self.chunks}"
        if self.pipelined:
            return f"pipe{self.formants}r{16 * self.pipelined}"
        return ("fast" if self.fast else "exact") + f"L{self.lanes_per_utterance}"


class NodeShard(C.Structure):
    """grail_node_shard: the rows and segments one device of a node renders (grail_node_shard_of)."""
    _fields_ = [
        ("first_row", C.c_uint64),
        ("rows", C.c_uint64),
        ("first_seg", C.c_uint32),
        ("n_segs", C.c_uint32),
    ]


class Rule(C.Structure):
    _fields_ = [
        ("string", C.POINTER(C.c_uint32)),
        ("string_len", C.c_uint32),
        ("phonemes", C.POINTER(C.c_int32)),
        ("n_phonemes", C.c_uint32),
    ]


PHONEME_DTYPE = np.dtype(
    [("phoneme", "<i4"), ("length", "<f4"), ("blend_length", "<f4"), ("frequency", "<f4")]
)

_lib = None


def lib_exists():
    return os.path.exists(LIB_PATH)


def load():
    """Load libgrail_hip.so; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GrailError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() "
                                        "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, u32p, u64 = C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64
    L.grail_abi_version.restype = C.c_int
    if L.grail_abi_version() != ABI_VERSION:     # before any other symbol is touched
        raise GrailError(ERR_INVALID_ARG, f"{LIB_PATH} has ABI version {L.grail_abi_version()}, this binding "
                                          f"mirrors version {ABI_VERSION} of include/grail_hip.h: rebuild the library")
    L.grail_status_string.restype = C.c_char_p
    L.grail_status_string.argtypes = [C.c_int]
    L.grail_last_error.restype = C.c_char_p
    L.grail_elem_silent.restype = None
    L.grail_elem_silent.argtypes = [C.POINTER(SynthesisElem)]
    fp = C.POINTER(C.c_float)
    L.grail_elem_new_phoneme.restype = None
    L.grail_elem_new_phoneme.argtypes = [C.POINTER(SynthesisElem)] + [fp] * 6
    L.grail_elem_new.restype = None
    L.grail_elem_new.argtypes = [C.POINTER(SynthesisElem), C.c_float, C.c_float] + [fp] * 6
    L.grail_elem_resample.restype = None
    L.grail_elem_resample.argtypes = [C.POINTER(SynthesisElem), C.c_float, C.c_float]
    L.grail_elem_blend.restype = None
    L.grail_elem_blend.argtypes = [C.POINTER(SynthesisElem)] * 3 + [C.c_float]
    L.grail_voice_generic.restype = None
    L.grail_voice_generic.argtypes = [C.POINTER(Voice)]
    L.grail_voice_generic_at.restype = None
    L.grail_voice_generic_at.argtypes = [C.POINTER(Voice), C.c_float]
    L.grail_voice_get.argtypes = [C.POINTER(Voice), C.c_int32, C.POINTER(SynthesisElem)]
    L.grail_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.grail_destroy.argtypes = [vp]
    L.grail_device_count.argtypes = [C.POINTER(C.c_int)]
    L.grail_device_pci_bus_id.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.grail_length_bound.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_float]
    L.grail_length_bound.restype = C.c_uint64
    L.grail_time_split_warmup.argtypes = [C.POINTER(Voice)]
    L.grail_time_split_warmup.restype = C.c_uint32
    L.grail_fast_sharpness.argtypes = [C.POINTER(Voice)]
    L.grail_fast_sharpness.restype = C.c_float
    L.grail_time_split_grid.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.grail_plan_blocks.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.POINTER(PlanBlock), C.c_uint32, u32p]
    L.grail_plan_ragged_blocks.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, u32p, u32p, u32p,
                                           C.POINTER(PlanBlock), C.c_uint32, u32p]
    L.grail_dispatch_model.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), u32p, C.c_uint32, C.POINTER(C.c_double)]
    L.grail_packed_launch_order.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, u32p]
    L.grail_set_voices.argtypes = [vp, vp, C.c_uint32]
    L.grail_get_voices.argtypes = [vp, vp, C.c_uint32, u32p]
    L.grail_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.grail_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.grail_batch_upload.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(vp)]
    L.grail_batch_upload_elems.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(vp)]
    L.grail_batch_free.argtypes = [vp, vp]
    L.grail_batch_size.restype = C.c_uint32
    L.grail_batch_size.argtypes = [vp]
    L.grail_batch_lengths.argtypes = [vp, vp, C.c_uint32, vp]
    L.grail_batch_synthesize_async.argtypes = [vp, vp, vp, u64, vp]
    L.grail_sync.argtypes = [vp]
    L.grail_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.grail_last_kernel_name.restype = C.c_char_p
    L.grail_last_kernel_name.argtypes = [vp]
    L.grail_synthesize_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, u64, vp, C.c_uint32]
    L.grail_synthesize_batch_elems.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, u64, vp,
                                               C.c_uint32]
    L.grail_stream_open.argtypes = [vp, vp, C.POINTER(vp)]
    L.grail_stream_next_async.argtypes = [vp, vp, C.c_uint32, vp, u64, vp]
    L.grail_stream_next_pcm16_async.argtypes = [vp, vp, C.c_uint32, vp, u64, vp]
    L.grail_stream_close.argtypes = [vp, vp]
    L.grail_stream_open_live.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.grail_stream_append.argtypes = [vp, vp, vp, vp]
    L.grail_stream_append_elems.argtypes = [vp, vp, vp, vp]
    L.grail_stream_finish.argtypes = [vp, vp, vp]
    L.grail_stream_pending.argtypes = [vp, vp, vp]
    L.grail_language_generic.restype = C.c_uint32
    L.grail_language_generic.argtypes = [C.POINTER(C.POINTER(Rule)), C.POINTER(C.c_int)]
    L.grail_transcribe.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Rule), C.c_uint32,
                                   C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_uint32, u32p]
    L.grail_intonate.argtypes = [C.POINTER(Voice), C.POINTER(C.c_int32), C.c_uint32, vp]
    L.grail_text_to_phoneme_elems.argtypes = [C.POINTER(Voice), C.c_char_p, vp, C.c_uint32, u32p]
    L.grail_say_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32, vp, vp, vp, u64, vp,
                                  C.c_uint32]
    L.grail_pcm16_async.argtypes = [vp, vp, u64, vp, C.c_uint32, C.c_uint32, vp, u64]
    L.grail_synthesize_batch_pcm16.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, u64, vp,
                                               C.c_uint32]
    L.grail_batch_synthesize_pcm16_async.argtypes = [vp, vp, vp, u64, vp]
    L.grail_batch_digest.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp, vp]
    L.grail_batch_compare.argtypes = [vp, vp, vp, u64, vp, vp, C.c_uint32, vp, vp, vp]
    L.grail_wav_write_i16.argtypes = [C.c_char_p, vp, C.c_uint32, C.c_uint32]
    L.grail_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.grail_device_free.argtypes = [vp, vp]
    L.grail_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.grail_host_free.argtypes = [vp, vp]
    L.grail_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.grail_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.grail_memset_d.argtypes = [vp, vp, C.c_int, C.c_size_t]
    L.grail_shard_range.restype = None
    L.grail_shard_range.argtypes = [u64, C.c_uint32, C.c_uint32, C.POINTER(u64), C.POINTER(u64)]
    L.grail_comm_unique_id.argtypes = [vp]
    L.grail_comm_init.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.grail_broadcast_voices.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.grail_comm_info.argtypes = [vp, u32p, u32p]
    L.grail_comm_destroy.argtypes = [vp]
    L.grail_node_create.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(vp)]
    L.grail_node_destroy.argtypes = [vp]
    L.grail_node_size.restype = C.c_uint32
    L.grail_node_size.argtypes = [vp]
    L.grail_node_context.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.grail_node_set_voices.argtypes = [vp, vp, C.c_uint32]
    L.grail_node_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.grail_node_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.grail_node_shard_of.argtypes = [u32p, u64, C.c_uint32, C.c_uint32, C.POINTER(NodeShard), u32p, u64]
    L.grail_node_synthesize_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, u64, vp, C.c_uint32]
    L.grail_node_synthesize_batch_elems.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, u64, vp, C.c_uint32]
    L.grail_node_synthesize_batch_pcm16.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, u64, vp, C.c_uint32]
    L.grail_node_synthesize_batch_device.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(vp), u64, vp]
    L.grail_node_say_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32, vp, vp, vp, u64, vp, C.c_uint32]
    L.grail_node_lengths.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    L.grail_node_last_shard_ms.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32]
    L.grail_node_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.grail_node_host_free.argtypes = [vp, vp]
    L.grail_mix_async.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, u64, C.c_uint32, u64,
                                  C.c_uint32]
    L.grail_batch_mix.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, u64, C.c_uint32, u64, vp, C.c_uint32]
    L.grail_mix_place_sequential.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.grail_pcm16_frames_async.argtypes = [vp, vp, u64, C.c_uint32, u64, vp]
    L.grail_wav_write_i16_frames.argtypes = [C.c_char_p, vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.grail_levels_async.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp, vp]
    L.grail_frame_levels_async.argtypes = [vp, vp, u64, vp, C.c_uint32, C.c_uint32, vp, vp, u64]
    L.grail_level_gains.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp]
    L.grail_active_level.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float]
    L.grail_active_level.restype = C.c_double
    L.grail_batch_mix_leveled.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint32, vp, u64, C.c_uint32, u64, vp, vp,
                                          vp, C.c_uint32]
    L.grail_kweighting.argtypes = [C.c_uint32, vp]
    L.grail_loudness_async.argtypes = [vp, vp, u64, vp, C.c_uint32, C.c_uint32, vp, vp, vp, u64, vp]
    L.grail_gated_mean_square.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.grail_gated_mean_square.restype = C.c_double
    L.grail_loudness_lufs.argtypes = [C.c_double]
    L.grail_loudness_lufs.restype = C.c_double
    L.grail_loudness_level.argtypes = [C.c_double]
    L.grail_loudness_level.restype = C.c_double
    L.grail_loudness_segmented_async.argtypes = [vp, vp, u64, vp, C.c_uint32, C.c_uint32, vp, vp, vp, u64, vp]
    L.grail_loudness_window_max.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.grail_loudness_window_max.restype = C.c_double
    L.grail_loudness_range.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.grail_loudness_range.restype = C.c_double
    L.grail_true_peak_coefficients.argtypes = [vp]
    L.grail_true_peak_async.argtypes = [vp, vp, u64, vp, C.c_uint32, vp, vp]
    L.grail_true_peak_db.argtypes = [C.c_double]
    L.grail_true_peak_db.restype = C.c_double
    L.grail_true_peak_limit_gains.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_float, vp, vp]
    L.grail_limit_ceiling.argtypes = [C.c_float]
    L.grail_limit_ceiling.restype = C.c_float
    L.grail_limit_async.argtypes = [vp, vp, u64, vp, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp, u64, vp, vp, vp]
    L.grail_resample_ratio.argtypes = [C.c_uint32, C.c_uint32, vp, vp, vp]
    L.grail_resample_coefficients.argtypes = [C.c_uint32, C.c_uint32, vp, C.c_uint32]
    L.grail_resample_len.argtypes = [u64, C.c_uint32, C.c_uint32, vp]
    L.grail_resample_async.argtypes = [vp, vp, u64, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64, vp, vp]
    L.grail_fir_len.argtypes = [u64, C.c_uint32, C.c_uint32, vp]
    L.grail_fir_design.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_uint32, vp]
    L.grail_fir_create.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    L.grail_fir_free.argtypes = [vp, vp]
    L.grail_fir_async.argtypes = [vp, vp, vp, u64, vp, C.c_uint32, vp, vp, u64, vp, vp]
    L.grail_filter_stream_len.argtypes = [u64, u64, C.c_uint32, C.c_uint32, C.c_int, vp]
    L.grail_filter_stream_open.argtypes = [vp, vp, C.c_uint32, vp, vp]
    L.grail_filter_stream_next_async.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp]
    L.grail_filter_stream_finish_async.argtypes = [vp, vp, vp, vp, u64, vp]
    L.grail_filter_stream_close.argtypes = [vp, vp]
    L.grail_resample_stream_len.argtypes = [u64, u64, C.c_uint32, C.c_uint32, C.c_int, vp]
    L.grail_resample_stream_open.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.grail_resample_stream_next_async.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp]
    L.grail_resample_stream_finish_async.argtypes = [vp, vp, vp, vp, u64, vp]
    L.grail_resample_stream_close.argtypes = [vp, vp]
    L.grail_limit_stream_len.argtypes = [u64, u64, C.c_uint32, C.c_int, vp]
    L.grail_limit_stream_open.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp]
    L.grail_limit_stream_next_async.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
    L.grail_limit_stream_finish_async.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp]
    L.grail_limit_stream_close.argtypes = [vp, vp]
    L.grail_meter_stream_hops.argtypes = [u64, u64, C.c_uint32, vp]
    L.grail_meter_stream_open.argtypes = [vp, C.c_uint32, C.c_uint32, vp, u64, vp]
    L.grail_meter_stream_next_async.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp]
    L.grail_meter_stream_read_async.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.grail_meter_stream_ledger.argtypes = [vp, vp, vp, vp]
    L.grail_meter_stream_finish_async.argtypes = [vp, vp, vp, vp]
    L.grail_meter_stream_close.argtypes = [vp, vp]
    L.grail_iir_design.argtypes = [C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_double, vp]
    L.grail_iir_create.argtypes = [vp, vp, vp, C.c_uint32, vp]
    L.grail_iir_free.argtypes = [vp, vp]
    L.grail_iir_async.argtypes = [vp, vp, vp, u64, vp, C.c_uint32, vp, C.c_uint32, vp, u64, vp, vp]
    L.grail_biquad_blocked_async.argtypes = [vp, vp, vp, u64, vp, C.c_uint32, vp, C.c_uint32, vp, u64, vp, vp]
    L.grail_biquad_block_matrix.argtypes = [vp, C.c_uint32, vp]
    L.grail_iir_stream_len.argtypes = [u64, u64, C.c_uint32, C.c_int, vp]
    L.grail_iir_stream_open.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp]
    L.grail_iir_stream_next_async.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp]
    L.grail_iir_stream_finish_async.argtypes = [vp, vp, vp, vp, u64, vp]
    L.grail_iir_stream_close.argtypes = [vp, vp]
    L.grail_dyn_design.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp]
    L.grail_dyn_ballistics.argtypes = [C.c_uint32, C.c_double, C.c_double, vp]
    L.grail_dyn_create.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
    L.grail_dyn_free.argtypes = [vp, vp]
    L.grail_dyn_async.argtypes = [vp, vp, vp, u64, vp, C.c_uint32, vp, vp, u64, vp, C.c_uint32, vp, vp, u64, vp, vp, vp]
    L.grail_track_dyn_async.argtypes = list(L.grail_dyn_async.argtypes)
    L.grail_dyn_stream_open.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.grail_dyn_stream_next_async.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp]
    L.grail_dyn_stream_close.argtypes = [vp, vp]
    L.grail_batch_mix_leveled_limited.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_uint32, vp, u64, C.c_uint32, u64, vp,
                                                  vp, vp, C.c_float, vp, C.c_uint32]
    _lib = L
    return L


def _check(status):
    if status != OK:
        raise GrailError(status, load().grail_last_error().decode() or
                         load().grail_status_string(status).decode())


# ---- host-side parameter algebra -------------------------------------------
def voice_generic(sample_rate=None):
    """voices::generic() (src/voices/generic.rs:5); sample_rate != None gives the
    resampled variant of SURVEY.md §8d."""
    v = Voice()
    if sample_rate is None:
        load().grail_voice_generic(C.byref(v))
    else:
        load().grail_voice_generic_at(C.byref(v), C.c_float(sample_rate))
    return v


def elem_new_phoneme(freq, bw, smooth, turb, breath, amp):
    """SynthesisElem::new_phoneme == MKPHON (src/lib.rs:381, src/voices/mod.rs:7)."""
    e = SynthesisElem()
    arrs = [(C.c_float * NUM_FORMANTS)(*[float(x) for x in a])
            for a in (freq, bw, smooth, turb, breath, amp)]
    load().grail_elem_new_phoneme(C.byref(e), *arrs)
    return e


def elem_resample(elem, old_rate, new_rate):
    e = SynthesisElem.from_buffer_copy(bytes(elem))
    load().grail_elem_resample(C.byref(e), C.c_float(old_rate), C.c_float(new_rate))
    return e


def elem_silent():
    e = SynthesisElem()
    load().grail_elem_silent(C.byref(e))
    return e


def elem_blend(a, b, alpha):
    e = SynthesisElem()
    load().grail_elem_blend(C.byref(e), C.byref(a), C.byref(b), C.c_float(alpha))
    return e


def shard_range(n_utt, rank, world):
    b, e = C.c_uint64(), C.c_uint64()
    load().grail_shard_range(n_utt, rank, world, C.byref(b), C.byref(e))
    return b.value, e.value


def node_shard_of(seg_offsets, index, n_devices):
    """(NodeShard, rebased seg_offsets) of device slot `index` out of n_devices: the view a node call hands to that
    device's grail_synthesize_batch (grail_node_shard_of; pure host arithmetic, no GPU)."""
    offs = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
    n_utt = len(offs) - 1
    u32p = C.POINTER(C.c_uint32)
    sh = NodeShard()
    _check(load().grail_node_shard_of(offs.ctypes.data_as(u32p), n_utt, index, n_devices, C.byref(sh), None, 0))
    rebased = np.zeros(sh.rows + 1, dtype=np.uint32)
    _check(load().grail_node_shard_of(offs.ctypes.data_as(u32p), n_utt, index, n_devices, C.byref(sh),
                                      rebased.ctypes.data_as(u32p), len(rebased)))
    return sh, rebased


def voices_blob(voices):
    """The broadcast payload: the raw grail_voice[] bytes."""
    return b"".join(bytes(v) for v in voices)


def voices_from_blob(blob):
    n = len(blob) // C.sizeof(Voice)
    assert n * C.sizeof(Voice) == len(blob)
    return [Voice.from_buffer_copy(blob[i * C.sizeof(Voice):(i + 1) * C.sizeof(Voice)])
            for i in range(n)]


def segments(seq):
    a = np.zeros(len(seq), dtype=PHONEME_DTYPE)
    for i, s in enumerate(seq):
        a[i] = tuple(s)
    return a


# ---- text front half ---------------------------------------------------------
def make_rules(rule_list):
    """[(string, [phonemes...]), ...] -> (Rule array, keepalive list)."""
    keep = []
    arr = (Rule * len(rule_list))()
    for i, (st, ph) in enumerate(rule_list):
        cps = (C.c_uint32 * max(len(st), 1))(*[ord(ch) for ch in st])
        pp = (C.c_int32 * max(len(ph), 1))(*ph)
        keep += [cps, pp]
        arr[i].string = C.cast(cps, C.POINTER(C.c_uint32))
        arr[i].string_len = len(st)
        arr[i].phonemes = C.cast(pp, C.POINTER(C.c_int32))
        arr[i].n_phonemes = len(ph)
    return arr, keep


def transcribe(text, rule_list, case_sensitive=False, leading_silence=False):
    """Transcriber (src/lib.rs:1116); leading_silence=True is .transcribe() (:1201)."""
    arr, keep = make_rules(rule_list)
    cps = (C.c_uint32 * max(len(text), 1))(*[ord(ch) for ch in text])
    cap = 4 * len(text) + 8
    out = (C.c_int32 * cap)()
    n = C.c_uint32()
    _check(load().grail_transcribe(cps, len(text), arr, len(rule_list), int(case_sensitive),
                                   int(leading_silence), out, cap, C.byref(n)))
    return list(out[: n.value])


def language_generic():
    """languages::generic() as [(string, [phonemes])], case_sensitive."""
    rules = C.POINTER(Rule)()
    cs = C.c_int()
    n = load().grail_language_generic(C.byref(rules), C.byref(cs))
    out = []
    for i in range(n):
        r = rules[i]
        out.append(("".join(chr(r.string[k]) for k in range(r.string_len)),
                    [r.phonemes[k] for k in range(r.n_phonemes)]))
    return out, bool(cs.value)


def text_to_phoneme_elems(voice, text):
    n = C.c_uint32()
    _check(load().grail_text_to_phoneme_elems(C.byref(voice), text.encode("utf-8"), None, 0,
                                              C.byref(n)))
    a = np.zeros(max(n.value, 1), dtype=PHONEME_DTYPE)
    _check(load().grail_text_to_phoneme_elems(C.byref(voice), text.encode("utf-8"), a.ctypes.data,
                                              n.value, C.byref(n)))
    return a[: n.value]


def wav_write_i16(path, pcm, sample_rate):
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    _check(load().grail_wav_write_i16(path.encode(), pcm.ctypes.data, len(pcm), int(sample_rate)))


def wav_write_i16_frames(path, frames, sample_rate):
    """A multichannel WAV: frames[n_frames, n_channels] int16 (1-D: mono), grail_wav_write_i16_frames."""
    frames = np.ascontiguousarray(frames, dtype=np.int16)
    if frames.ndim == 1:
        frames = frames.reshape(-1, 1)
    _check(load().grail_wav_write_i16_frames(path.encode(), frames.ctypes.data, frames.shape[0], frames.shape[1],
                                             int(sample_rate)))


def _mix_items(item_rows, item_offsets, item_tracks, item_gains):
    """The parallel item arrays of the mixing calls (None: all on track 0 / gain 1.0)."""
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    offs = np.ascontiguousarray(item_offsets, dtype=np.uint64)
    tracks = None if item_tracks is None else np.ascontiguousarray(item_tracks, dtype=np.uint32)
    gains = None if item_gains is None else np.ascontiguousarray(item_gains, dtype=np.float32)
    assert len(offs) == len(rows) and (tracks is None or len(tracks) == len(rows)) and (gains is None or len(gains) == len(rows))
    return rows, offs, tracks, gains


def mix_place_sequential(row_len, item_rows, item_tracks=None, gaps=None, n_tracks=1):
    """Items laid end to end per track in accumulation order, gaps[i] samples after the previous item on its track
    (grail_mix_place_sequential; pure host).  Returns (item_offsets uint64[n_items], track_len uint64[n_tracks])."""
    row_len = np.ascontiguousarray(row_len, dtype=np.uint32)
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    tracks = None if item_tracks is None else np.ascontiguousarray(item_tracks, dtype=np.uint32)
    gaps = None if gaps is None else np.ascontiguousarray(gaps, dtype=np.int64)
    offs = np.zeros(max(len(rows), 1), dtype=np.uint64)
    track_len = np.zeros(max(n_tracks, 1), dtype=np.uint64)
    _check(load().grail_mix_place_sequential(row_len.ctypes.data, len(row_len), rows.ctypes.data, _ptr(tracks), _ptr(gaps),
                                             len(rows), n_tracks, offs.ctypes.data, track_len.ctypes.data))
    return offs[:len(rows)], track_len[:n_tracks]


def length_bound(segment_lengths, sample_rate):
    """An upper bound of an utterance's length in samples (grail_length_bound); None: no bound."""
    a = np.ascontiguousarray(segment_lengths, dtype=np.float32)
    v = int(load().grail_length_bound(a.ctypes.data_as(C.POINTER(C.c_float)), len(a), float(sample_rate)))
    return None if v == 2 ** 64 - 1 else v


def time_split_warmup(voice):
    """Warm-up length of `voice` for the time-split fast kernels, in samples (0: does not qualify)."""
    return int(load().grail_time_split_warmup(C.byref(voice)))


def fast_sharpness(voice):
    """Predicted bound on |fast - reference| for `voice`, units of 2^-23 (served up to FAST_SHARPNESS_LIMIT)."""
    return float(load().grail_fast_sharpness(C.byref(voice)))


def time_split_grid(span_samples, warmup, chunks, ff_cost_permille=165):
    """Chunk starts of a time-split launch (GrailError when so many chunks do not fit)."""
    out = (C.c_uint32 * max(int(chunks), 1))()
    _check(load().grail_time_split_grid(span_samples, warmup, chunks, ff_cost_permille, out))
    return [int(x) for x in out]


def plan_blocks(rows, span_samples, arithmetic=0, live_formants=4, warmup=3904, compute_units=256):
    """How a batch of `rows` utterances (longest: span_samples) is cut into kernel launches: [PlanBlock]."""
    arr = (PlanBlock * 16)()
    n = C.c_uint32()
    _check(load().grail_plan_blocks(compute_units, arithmetic, live_formants, warmup, rows, span_samples, arr, 16,
                                    C.byref(n)))
    return [PlanBlock.from_buffer_copy(bytes(arr[i])) for i in range(min(n.value, 16))]


def plan_ragged_blocks(row_samples, row_segments=None, row_kinks=None, arithmetic=0, live_formants=4, warmup=3904,
                       compute_units=256):
    """... of a batch whose utterances differ in length: row_samples descending (launch order), the rows' segments and
    kinks of alpha (option "ragged_plan"): [PlanBlock]."""
    def u32(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
    rs, sg, kk = u32(row_samples), u32(row_segments), u32(row_kinks)
    u32p = C.POINTER(C.c_uint32)
    arr = (PlanBlock * 16)()
    n = C.c_uint32()
    _check(load().grail_plan_ragged_blocks(compute_units, arithmetic, live_formants, warmup, len(rs),
                                           rs.ctypes.data_as(u32p), None if sg is None else sg.ctypes.data_as(u32p),
                                           None if kk is None else kk.ctypes.data_as(u32p), arr, 16, C.byref(n)))
    return [PlanBlock.from_buffer_copy(bytes(arr[i])) for i in range(min(n.value, 16))]


def dispatch_model(workgroup_ms, order=None, compute_units=256, waves_per_workgroup=1):
    """The makespan of workgroups that take workgroup_ms[b], launched in `order`, by the library's model of the workgroup
    dispatcher (grail_dispatch_model; pure host arithmetic)."""
    c = np.ascontiguousarray(workgroup_ms, dtype=np.float64)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    out = C.c_double()
    _check(load().grail_dispatch_model(compute_units, waves_per_workgroup, c.ctypes.data_as(C.POINTER(C.c_double)),
                                       None if o is None else o.ctypes.data_as(C.POINTER(C.c_uint32)), len(c), C.byref(out)))
    return out.value


def packed_launch_order(workgroup_ms, compute_units=256, waves_per_workgroup=1):
    """order[position] = workgroup: what option "packed_launch_order" launches such workgroups in (grail_packed_launch_order)."""
    c = np.ascontiguousarray(workgroup_ms, dtype=np.float64)
    o = np.zeros(len(c), dtype=np.uint32)
    _check(load().grail_packed_launch_order(compute_units, waves_per_workgroup, c.ctypes.data_as(C.POINTER(C.c_double)), len(c),
                                            o.ctypes.data_as(C.POINTER(C.c_uint32))))
    return o


def device_count():
    n = C.c_int(0)
    st = load().grail_device_count(C.byref(n))
    return n.value if st == OK else 0


def _ptr(a):
    return None if a is None else a.ctypes.data


def level_gains(mode, item_rows, item_level_db, sumsq=None, peak=None, nonfinite=None, row_len=None, active_level=None,
                n_rows=None):
    """grail_level_gains (pure host): the gain that brings each item's row to item_level_db[i] dB, from the rows' numbers
    (LEVEL_PEAK: peak; LEVEL_RMS: sumsq and row_len; LEVEL_ACTIVE: active_level).  Returns (gains float32[n_items],
    n_unleveled: the items that got gain 0 because their row's level is 0 or it holds a non-finite sample)."""
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    sumsq, peak, nonfinite = arr(sumsq, np.float64), arr(peak, np.float32), arr(nonfinite, np.uint32)
    row_len, active_level = arr(row_len, np.uint32), arr(active_level, np.float64)
    given = [len(a) for a in (sumsq, peak, nonfinite, row_len, active_level) if a is not None]
    if n_rows is None:
        n_rows = min(given) if given else 0
    assert all(g >= n_rows for g in given)
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    db = np.ascontiguousarray(item_level_db, dtype=np.float32)
    assert len(db) == len(rows)
    gains = np.full(max(len(rows), 1), np.nan, dtype=np.float32)
    n_unleveled = C.c_uint32(0xFFFFFFFF)
    _check(load().grail_level_gains(int(mode), _ptr(sumsq), _ptr(peak), _ptr(nonfinite), _ptr(row_len), _ptr(active_level),
                                    n_rows, rows.ctypes.data, db.ctypes.data, len(rows), gains.ctypes.data,
                                    C.addressof(n_unleveled)))
    return gains[:len(rows)], n_unleveled.value


def active_level(frame_sumsq, row_len, frame=LEVEL_FRAME, floor_db=LEVEL_ACTIVE_FLOOR_DB):
    """grail_active_level (pure host): sqrt(mean square) over the frames within floor_db of the loudest frame."""
    fs = np.ascontiguousarray(frame_sumsq, dtype=np.float64)
    assert len(fs) >= -(-int(row_len) // int(frame))
    return float(load().grail_active_level(fs.ctypes.data, int(row_len), int(frame), float(floor_db)))


def kweighting(sample_rate):
    """grail_kweighting (pure host): the ten K-weighting coefficients for a sample rate, float64[10]: b0 b1 b2 a1 a2 of the
    shelf, then of the high-pass."""
    coef = np.full(10, np.nan, dtype=np.float64)
    _check(load().grail_kweighting(int(sample_rate), coef.ctypes.data))
    return coef


def gated_mean_square(hop_sumsq, hop):
    """grail_gated_mean_square (pure host): the BS.1770 gate over one row's hop sums; hop = sample_rate // 10."""
    hs = np.ascontiguousarray(hop_sumsq, dtype=np.float64)
    return float(load().grail_gated_mean_square(hs.ctypes.data if len(hs) else None, len(hs), int(hop)))


def loudness_lufs(gated_ms):
    """grail_loudness_lufs: -0.691 + 10 log10(gated mean square); -inf for 0."""
    return float(load().grail_loudness_lufs(float(gated_ms)))


def loudness_level(gated_ms):
    """grail_loudness_level: the level whose 20 log10 is the loudness in LUFS."""
    return float(load().grail_loudness_level(float(gated_ms)))


def loudness_window_max(hop_sumsq, hop, window_hops):
    """grail_loudness_window_max (pure host): the largest mean square over windows of window_hops hops, one every hop:
    4 = momentary, 30 = short-term; loudness_lufs() gives its LUFS.  0 for fewer hops than the window."""
    hs = np.ascontiguousarray(hop_sumsq, dtype=np.float64)
    return float(load().grail_loudness_window_max(hs.ctypes.data if len(hs) else None, len(hs), int(hop), int(window_hops)))


def loudness_range(hop_sumsq, hop):
    """grail_loudness_range (pure host): the loudness range in LU (EBU Tech 3342) of one row's hop sums; 0 for fewer than
    30 hops or nothing above the absolute gate."""
    hs = np.ascontiguousarray(hop_sumsq, dtype=np.float64)
    return float(load().grail_loudness_range(hs.ctypes.data if len(hs) else None, len(hs), int(hop)))


def true_peak_coefficients():
    """grail_true_peak_coefficients (pure host): the 4 x 12 taps of the BS.1770-4 Annex 2 filter, float64[4, 12]."""
    coef = np.full((TRUE_PEAK_PHASES, TRUE_PEAK_TAPS), np.nan, dtype=np.float64)
    _check(load().grail_true_peak_coefficients(coef.ctypes.data))
    return coef


def true_peak_db(true_peak):
    """grail_true_peak_db: 20 log10(true peak) in dBTP; -inf for 0."""
    return float(load().grail_true_peak_db(float(true_peak)))


def limit_ceiling(ceiling_db):
    """grail_limit_ceiling (pure host): the float32 that a ceiling in dBTP is to grail_limit_async."""
    return np.float32(load().grail_limit_ceiling(float(np.float32(ceiling_db))))


def limit_stream_len(fed_before, n, lookahead_log2, finishing=False):
    """grail_limit_stream_len (pure host): the outputs a call on a limit stream writes for a group that was fed fed_before
    samples before it: a `next` call that feeds n samples, or (finishing, n = 0) the tail of `finish`."""
    out = C.c_uint64(0)
    _check(load().grail_limit_stream_len(fed_before, n, lookahead_log2, 1 if finishing else 0, C.addressof(out)))
    return out.value


def resample_ratio(rate_in, rate_out):
    """grail_resample_ratio (pure host): (up, down, taps) of a pair of whole-numbered rates; GrailError for a pair that is
    not supported (a rate of 0, equal rates, more than RESAMPLE_TABLE_MAX table entries)."""
    u, d, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _check(load().grail_resample_ratio(rate_in, rate_out, C.addressof(u), C.addressof(d), C.addressof(p)))
    return u.value, d.value, p.value


def resample_coefficients(rate_in, rate_out):
    """grail_resample_coefficients (pure host): the numerators N of 2^26 of the pair's table, int32[up, taps]."""
    u, _, p = resample_ratio(rate_in, rate_out)
    num = np.zeros((u, p), dtype=np.int32)
    _check(load().grail_resample_coefficients(rate_in, rate_out, num.ctypes.data, u * p))
    return num


def resample_len(n, rate_in, rate_out):
    """grail_resample_len (pure host): ceil(n * up / down), the length of a row of n samples resampled."""
    out = C.c_uint64(0)
    _check(load().grail_resample_len(n, rate_in, rate_out, C.addressof(out)))
    return out.value


def resample_stream_len(fed_before, n, rate_in, rate_out, finishing=False):
    """grail_resample_stream_len (pure host): the outputs a call on a resample stream writes for a row that was fed
    fed_before samples before it: a `next` call that feeds n samples, or (finishing, n = 0) the tail of `finish`."""
    out = C.c_uint64(0)
    _check(load().grail_resample_stream_len(fed_before, n, rate_in, rate_out, 1 if finishing else 0, C.addressof(out)))
    return out.value


def fir_len(n, n_taps, origin):
    """grail_fir_len (pure host): 0 for n = 0, else n + n_taps - 1 - origin, the length of a row of n samples filtered."""
    out = C.c_uint64(0)
    _check(load().grail_fir_len(n, n_taps, origin, C.addressof(out)))
    return out.value


def fir_stream_len(fed_before, n, n_taps, origin, finishing=False):
    """grail_filter_stream_len (pure host): the outputs a call on a filter stream writes for a row that was fed fed_before
    samples before it: a `next` call that feeds n samples, or (finishing, n = 0) the tail of `finish`."""
    out = C.c_uint64(0)
    _check(load().grail_filter_stream_len(fed_before, n, n_taps, origin, 1 if finishing else 0, C.addressof(out)))
    return out.value


def fir_design(sample_rate, lo_hz, hi_hz, n_taps):
    """grail_fir_design (pure host): float32[n_taps] of the Kaiser-windowed band-pass lo_hz .. hi_hz at sample_rate (n_taps
    odd; lo_hz = 0: a low-pass, hi_hz = sample_rate / 2: a high-pass).  The origin to use is (n_taps - 1) // 2."""
    taps = np.zeros(max(int(n_taps), 1), dtype=np.float32)
    _check(load().grail_fir_design(sample_rate, lo_hz, hi_hz, n_taps, taps.ctypes.data))
    return taps


def iir_design(kind, sample_rate, f0_hz, q, gain_db=0.0):
    """grail_iir_design (pure host): float64[5] = b0 b1 b2 a1 a2 of one biquad section of `kind` (IIR_LOWPASS ... IIR_HIGHSHELF)
    at f0_hz with quality q; gain_db is read by the shelves and the peak."""
    coef = np.zeros(5, dtype=np.float64)
    _check(load().grail_iir_design(kind, sample_rate, f0_hz, q, gain_db, coef.ctypes.data))
    return coef


def iir_block_matrix(coef):
    """grail_biquad_block_matrix (pure host): float64 [2 S][2 S], the block transition matrix of one filter (float64 [S][5] or
    flat [5 S]): state i (s1[0] s2[0] s1[1] ...) after IIR_BLOCK steps on +0.0 from the unit state c, at [i][c]."""
    flat = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
    assert len(flat) % 5 == 0
    S = len(flat) // 5
    matrix = np.zeros((2 * S, 2 * S), dtype=np.float64)
    _check(load().grail_biquad_block_matrix(flat.ctypes.data, S, matrix.ctypes.data))
    return matrix


def iir_stream_len(fed_before, n, tail, finishing=False):
    """grail_iir_stream_len (pure host): the outputs a call on an IIR stream writes for a row that was fed fed_before samples
    before it: n for a `next` call that feeds n; for `finish` (n must be 0) the tail, or 0 for a row that was fed nothing."""
    out = C.c_uint64(0)
    _check(load().grail_iir_stream_len(fed_before, n, tail, 1 if finishing else 0, C.addressof(out)))
    return out.value


def dyn_design(kind, detector, threshold_db, ratio, knee_db=0.0, range_db=0.0, makeup_db=0.0):
    """grail_dyn_design (pure host): float64[DYN_POINTS], the gain curve of a compressor (DYN_COMPRESS) or a downward expander
    (DYN_EXPAND; range_db: the most it takes away) over the levels of the detector's envelope (DYN_PEAK or DYN_SQUARE)."""
    gain = np.zeros(DYN_POINTS, dtype=np.float64)
    _check(load().grail_dyn_design(kind, detector, threshold_db, ratio, knee_db, range_db, makeup_db, gain.ctypes.data))
    return gain


def dyn_ballistics(sample_rate, attack_ms, release_ms):
    """grail_dyn_ballistics (pure host): float64[2] = alpha_attack, alpha_release of an envelope that covers 1 - 1/e of a step
    in attack_ms on the way up and release_ms on the way down; 0.0 for a time of 0."""
    alpha = np.zeros(2, dtype=np.float64)
    _check(load().grail_dyn_ballistics(sample_rate, attack_ms, release_ms, alpha.ctypes.data))
    return alpha


def true_peak_limit_gains(true_peak, item_rows, item_gains, ceiling_db, n_rows=None):
    """grail_true_peak_limit_gains (pure host): the gains capped so that |gain| * true_peak[row] <= 10^(ceiling_db / 20).
    Returns (gains float32[n_items], a copy; n_limited: the items that were changed)."""
    tp = np.ascontiguousarray(true_peak, dtype=np.float64)
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    gains = np.array(item_gains, dtype=np.float32, ndmin=1)
    assert len(gains) == len(rows)
    n_limited = C.c_uint32(0xFFFFFFFF)
    _check(load().grail_true_peak_limit_gains(tp.ctypes.data, len(tp) if n_rows is None else n_rows, rows.ctypes.data,
                                              len(rows), float(ceiling_db), gains.ctypes.data, C.addressof(n_limited)))
    return gains, n_limited.value


class Batch:
    def __init__(self, ctx, handle, n_utt):
        self.ctx, self.handle, self.n_utt = ctx, handle, n_utt

    def lengths(self, max_len=0xFFFFFFFF):
        out = np.zeros(max(self.n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_lengths(self.ctx.handle, self.handle, max_len, out.ctypes.data))
        return out[: self.n_utt]

    def synthesize_async(self, out_dev, out_stride, out_len_dev=None):
        _check(load().grail_batch_synthesize_async(self.ctx.handle, self.handle, out_dev,
                                                   out_stride, out_len_dev))

    def synthesize_pcm16_async(self, out_dev, out_stride, out_len_dev=None):
        """Rows of i16 PCM: the WAV sink's conversion fused into the kernel's store."""
        _check(load().grail_batch_synthesize_pcm16_async(self.ctx.handle, self.handle, out_dev,
                                                         out_stride, out_len_dev))

    def mix(self, item_rows, item_offsets, tracks_dev, track_stride, n_tracks, track_len, item_tracks=None,
            item_gains=None, accumulate=False):
        """grail_batch_mix: the batch rendered in blocks of rows and mixed into tracks_dev [n_tracks][track_stride]
        (synchronous).  Returns the rows' lengths."""
        rows, offs, tracks, gains = _mix_items(item_rows, item_offsets, item_tracks, item_gains)
        out_len = np.zeros(max(self.n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_mix(self.ctx.handle, self.handle, rows.ctypes.data, _ptr(tracks), offs.ctypes.data,
                                      _ptr(gains), len(rows), tracks_dev, track_stride, n_tracks, track_len,
                                      out_len.ctypes.data, MIX_ACCUMULATE if accumulate else 0))
        return out_len[:self.n_utt]

    def mix_leveled(self, item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                    item_tracks=None, mode=LEVEL_RMS, accumulate=False):
        """grail_batch_mix_leveled: mix() with a level in dB per item instead of a gain; every block's rows are measured on
        the device between rendering and mixing.  Returns (the rows' lengths, the gains used, n_unleveled)."""
        return self._mix_leveled(item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                                 item_tracks, mode, accumulate, None)[:3]

    def mix_leveled_limited(self, item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                            ceiling_db, item_tracks=None, mode=LEVEL_RMS, accumulate=False):
        """grail_batch_mix_leveled_limited: mix_leveled() under a true-peak ceiling in dBTP; the rows' true peaks are
        measured too and cap the gains.  Returns (the rows' lengths, the gains used, n_unleveled, n_limited)."""
        return self._mix_leveled(item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                                 item_tracks, mode, accumulate, float(ceiling_db))

    def _mix_leveled(self, item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len, item_tracks,
                     mode, accumulate, ceiling_db):
        rows, offs, tracks, _ = _mix_items(item_rows, item_offsets, item_tracks, None)
        db = np.ascontiguousarray(item_level_db, dtype=np.float32)
        assert len(db) == len(rows)
        out_len = np.zeros(max(self.n_utt, 1), dtype=np.uint32)
        gains = np.zeros(max(len(rows), 1), dtype=np.float32)
        n_unleveled, n_limited = C.c_uint32(0), C.c_uint32(0)
        flags = MIX_ACCUMULATE if accumulate else 0
        if ceiling_db is None:
            _check(load().grail_batch_mix_leveled(self.ctx.handle, self.handle, rows.ctypes.data, _ptr(tracks), offs.ctypes.data,
                                                  db.ctypes.data, int(mode), len(rows), tracks_dev, track_stride, n_tracks,
                                                  track_len, out_len.ctypes.data, gains.ctypes.data, C.addressof(n_unleveled),
                                                  flags))
        else:
            _check(load().grail_batch_mix_leveled_limited(
                self.ctx.handle, self.handle, rows.ctypes.data, _ptr(tracks), offs.ctypes.data, db.ctypes.data, int(mode),
                len(rows), tracks_dev, track_stride, n_tracks, track_len, out_len.ctypes.data, gains.ctypes.data,
                C.addressof(n_unleveled), ceiling_db, C.addressof(n_limited), flags))
        return out_len[:self.n_utt], gains[:len(rows)], n_unleveled.value, n_limited.value

    def free(self):
        if self.handle:
            load().grail_batch_free(self.ctx.handle, self.handle)
            self.handle = None


class Stream:
    """grail_stream: resumable synthesis of a Batch (chunks of samples per call)."""

    def __init__(self, batch):
        self.batch, self.ctx = batch, batch.ctx
        h = C.c_void_p()
        _check(load().grail_stream_open(self.ctx.handle, batch.handle, C.byref(h)))
        self.handle = h

    def next_async(self, max_samples, out_dev, out_stride, out_len_dev=None):
        _check(load().grail_stream_next_async(self.ctx.handle, self.handle, max_samples, out_dev,
                                              out_stride, out_len_dev))

    def next_pcm16_async(self, max_samples, out_dev, out_stride, out_len_dev=None):
        _check(load().grail_stream_next_pcm16_async(self.ctx.handle, self.handle, max_samples,
                                                    out_dev, out_stride, out_len_dev))

    def close(self):
        if self.handle:
            load().grail_stream_close(self.ctx.handle, self.handle)
            self.handle = None


class LiveStream(Stream):
    """grail_stream_open_live: n_utt chains whose sources deliver while they run (examples/interactive.rs:31-48)."""

    def __init__(self, ctx, n_utt, voice_ids=None, jitter_seeds=None, ring_segments=0, elems=False):
        self.ctx, self.n_utt, self.elems, self.batch = ctx, n_utt, elems, None
        if voice_ids is not None:
            voice_ids = np.ascontiguousarray(voice_ids, dtype=np.uint32)
            assert len(voice_ids) == n_utt
        if jitter_seeds is not None:
            jitter_seeds = np.ascontiguousarray(jitter_seeds, dtype=np.uint32)
            assert len(jitter_seeds) == n_utt
        h = C.c_void_p()
        _check(load().grail_stream_open_live(ctx.handle, n_utt, _ptr(voice_ids), _ptr(jitter_seeds), ring_segments,
                                             1 if elems else 0, C.byref(h)))
        self.handle = h

    def append(self, segs, seg_offsets):
        """Utterance u receives segs[seg_offsets[u]:seg_offsets[u + 1]] behind what it already has."""
        seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        assert len(seg_offsets) == self.n_utt + 1
        if self.elems:
            arr = (SequenceElem * max(len(segs), 1))(*segs)
            _check(load().grail_stream_append_elems(self.ctx.handle, self.handle, C.cast(arr, C.c_void_p),
                                                    seg_offsets.ctypes.data))
        else:
            segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
            _check(load().grail_stream_append(self.ctx.handle, self.handle, segs.ctypes.data, seg_offsets.ctypes.data))

    def finish(self, which=None):
        if which is not None:
            which = np.ascontiguousarray(which, dtype=np.uint8)
            assert len(which) == self.n_utt
        _check(load().grail_stream_finish(self.ctx.handle, self.handle, _ptr(which)))

    def pending(self):
        out = np.zeros(self.n_utt, dtype=np.uint32)
        _check(load().grail_stream_pending(self.ctx.handle, self.handle, out.ctypes.data))
        return out


def _waited(ctx, n, types, call):
    """The waited-for form of a call whose results are device arrays: n words of each of `types` in device memory, call(*them),
    the results copied back; the wait and the release whatever happened.  A tuple of arrays, one per type."""
    res = [np.zeros(n, dtype=t) for t in types]
    d = [ctx.device_alloc(n * 4) for _ in res]
    try:
        call(*d)
        for dst, src in zip(res, d):
            ctx.d2h(dst, src, n * 4)
    finally:
        ctx.sync()
        for p in d:
            ctx.device_free(p)
    return tuple(res)


def _waited_sized(ctx, n, types, call):
    """_waited for results of 4 or 8 bytes each"""
    res = [np.zeros(n, dtype=t) for t in types]
    d = [ctx.device_alloc(max(r.nbytes, 8)) for r in res]
    try:
        call(*d)
        for dst, src in zip(res, d):
            if dst.nbytes:
                ctx.d2h(dst, src, dst.nbytes)
    finally:
        ctx.sync()
        for p in d:
            ctx.device_free(p)
    return tuple(res)


class LimitStream:
    """A limit stream of a Context (Context.limit_stream_open), beside the fir_stream_* and resample_stream_* helpers: the
    handle with what the waited-for forms need to size their results, one per group."""

    def __init__(self, ctx, handle, n_rows, group, lookahead_log2):
        self.ctx, self.handle, self.n_rows, self.group, self.lookahead_log2 = ctx, handle, n_rows, group, lookahead_log2
        self.n_groups = n_rows // group
        self.delay = limit_stream_delay(lookahead_log2)

    def next_async(self, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, min_gain_dev=None,
                   n_limited_dev=None, nonfinite_dev=None):
        """grail_limit_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the outputs that
        became known go to out_dev + u * out_stride.  Results are DEVICE arrays [n_groups] (any may be None), queued on the
        context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_limit_stream_next_async(self.ctx.handle, self.handle, in_dev, in_stride, in_len_dev, out_dev, out_stride,
                                                    out_len_dev, min_gain_dev, n_limited_dev, nonfinite_dev))

    def _waited(self, types, call):
        return _waited(self.ctx, self.n_groups, types, call)

    def next(self, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """next_async, waited for, the results copied back: (out_len uint32, min_gain float32, n_limited uint32, nonfinite
        uint32), one per group; a refused group reads (LIMIT_REFUSED, NaN, 0, 0)."""
        return self._waited((np.uint32, np.float32, np.uint32, np.uint32),
                            lambda *d: self.next_async(in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def finish_async(self, out_dev, out_stride, which=None, out_len_dev=None, min_gain_dev=None, n_limited_dev=None):
        """grail_limit_stream_finish_async: the groups marked in which (a host sequence, non-zero = marked; None: every group)
        that have not ended write their tails (at most `delay` samples a row) and end."""
        marks = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        assert marks is None or len(marks) == self.n_groups
        _check(load().grail_limit_stream_finish_async(self.ctx.handle, self.handle, None if marks is None else marks.ctypes.data,
                                                      out_dev, out_stride, out_len_dev, min_gain_dev, n_limited_dev))

    def finish(self, out_dev, out_stride, which=None):
        """finish_async, waited for: (out_len uint32, min_gain float32, n_limited uint32), one per group; (0, 1.0, 0) for
        groups not marked or ended before."""
        return self._waited((np.uint32, np.float32, np.uint32), lambda *d: self.finish_async(out_dev, out_stride, which, *d))

    def close(self):
        """grail_limit_stream_close: waits for the context's stream, then releases the stream."""
        if self.handle is not None:
            _check(load().grail_limit_stream_close(self.ctx.handle, self.handle))
            self.handle = None


def meter_stream_hops(fed_before, n, sample_rate):
    """grail_meter_stream_hops (pure host): the hops a `next` call on a meter stream completes for a row that was fed fed_before
    samples before it and is fed n: (fed_before + n) // H - fed_before // H, H = sample_rate // 10."""
    out = C.c_uint64()
    _check(load().grail_meter_stream_hops(fed_before, n, sample_rate, C.addressof(out)))
    return out.value


class MeterStream:
    """A meter stream of a Context (Context.meter_stream_open), in the style of LimitStream: the handle with what the waited-for
    forms need to size their results, one per row."""

    def __init__(self, ctx, handle, n_rows, sample_rate, max_hops):
        self.ctx, self.handle, self.n_rows, self.sample_rate, self.max_hops = ctx, handle, n_rows, sample_rate, max_hops
        self.hop = sample_rate // 10

    def hops_stride(self, in_stride):
        """the least hops_stride of a call that feeds rows of in_stride: the most hops a row can complete in it"""
        return (in_stride + self.hop - 1) // self.hop

    def next_async(self, in_dev, in_stride, in_len_dev, hop_sumsq_dev=None, hops_stride=0, n_hops_dev=None, true_peak_dev=None,
                   nonfinite_dev=None):
        """grail_meter_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the hops the call
        completes go to hop_sumsq_dev + u * hops_stride (float64).  Results are DEVICE arrays [n_rows] (uint32, float64,
        uint32; any may be None), queued on the context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_meter_stream_next_async(self.ctx.handle, self.handle, in_dev, in_stride, in_len_dev, hop_sumsq_dev,
                                                    hops_stride, n_hops_dev, true_peak_dev, nonfinite_dev))

    def _waited(self, types, call):
        """_waited for results of 4 or 8 bytes each"""
        res = [np.zeros(self.n_rows, dtype=t) for t in types]
        d = [self.ctx.device_alloc(r.nbytes) for r in res]
        try:
            call(*d)
            for dst, src in zip(res, d):
                self.ctx.d2h(dst, src, dst.nbytes)
        finally:
            self.ctx.sync()
            for p in d:
                self.ctx.device_free(p)
        return tuple(res)

    def next(self, in_dev, in_stride, in_len_dev, hop_sumsq_dev=None, hops_stride=0):
        """next_async, waited for, the results copied back: (n_hops uint32, true_peak float64, nonfinite uint32), one per
        row; a refused row reads (LIMIT_REFUSED, NaN, 0)."""
        return self._waited((np.uint32, np.float64, np.uint32),
                            lambda *d: self.next_async(in_dev, in_stride, in_len_dev, hop_sumsq_dev, hops_stride, *d))

    def read_async(self, integrated_ms_dev=None, momentary_ms_dev=None, short_term_ms_dev=None, true_peak_dev=None, hops_dev=None):
        """grail_meter_stream_read_async: what the meter shows of every row now, DEVICE arrays [n_rows] of float64 (hops_dev:
        uint64), any may be None; changes no state."""
        _check(load().grail_meter_stream_read_async(self.ctx.handle, self.handle, integrated_ms_dev, momentary_ms_dev,
                                                    short_term_ms_dev, true_peak_dev, hops_dev))

    def read(self):
        """read_async, waited for: (integrated_ms, momentary_ms, short_term_ms, true_peak float64, hops uint64), one per row."""
        return self._waited((np.float64, np.float64, np.float64, np.float64, np.uint64), self.read_async)

    def ledger(self):
        """grail_meter_stream_ledger: (the ledger's device address, its stride in float64); row u's hop sums lie at
        address + 8 * (u * stride + h), h below the row's hops."""
        base, stride = C.c_void_p(), C.c_uint64()
        _check(load().grail_meter_stream_ledger(self.ctx.handle, self.handle, C.addressof(base), C.addressof(stride)))
        return base, stride.value

    def ledger_rows(self):
        """the rows' hop sums so far, copied from the ledger: a list of float64 arrays, one per row"""
        hops = self.read()[4]
        base, stride = self.ledger()
        rows = []
        for u, h in enumerate(hops):
            row = np.zeros(int(h), dtype=np.float64)
            if h:
                self.ctx.d2h(row, C.c_void_p(base.value + 8 * u * stride), row.nbytes)
            rows.append(row)
        return rows

    def finish_async(self, which=None, true_peak_dev=None):
        """grail_meter_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row) that
        have not ended ring out over the eleven outputs after their last sample and end."""
        marks = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        assert marks is None or len(marks) == self.n_rows
        _check(load().grail_meter_stream_finish_async(self.ctx.handle, self.handle, None if marks is None else marks.ctypes.data,
                                                      true_peak_dev))

    def finish(self, which=None):
        """finish_async, waited for: the largest of each row's eleven last outputs, float64; +0.0 for rows not marked or ended
        before."""
        return self._waited((np.float64,), lambda d: self.finish_async(which, d))[0]

    def close(self):
        """grail_meter_stream_close: waits for the context's stream, then releases the stream."""
        if self.handle is not None:
            _check(load().grail_meter_stream_close(self.ctx.handle, self.handle))
            self.handle = None


class Context:
    """grail_ctx: one per (process, GPU)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(load().grail_create(device, C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            load().grail_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_voices(self, voices):
        arr = (Voice * len(voices))(*[v.copy() for v in voices])
        _check(load().grail_set_voices(self.handle, C.cast(arr, C.c_void_p), len(voices)))

    def get_voices(self):
        n = C.c_uint32()
        _check(load().grail_get_voices(self.handle, None, 0, C.byref(n)))
        arr = (Voice * max(n.value, 1))()
        _check(load().grail_get_voices(self.handle, C.cast(arr, C.c_void_p), n.value, C.byref(n)))
        return [arr[i].copy() for i in range(n.value)]

    def pci_bus_id(self):
        buf = C.create_string_buffer(32)
        _check(load().grail_device_pci_bus_id(self.handle, buf, 32))
        return buf.value.decode()

    def set_option(self, name, value):
        _check(load().grail_set_option(self.handle, name.encode(), value))

    def get_option(self, name):
        v = C.c_int64()
        _check(load().grail_get_option(self.handle, name.encode(), C.byref(v)))
        return v.value

    @staticmethod
    def _prep(segs_dtype, segs, seg_offsets, voice_ids, jitter_seeds):
        seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        n_utt = len(seg_offsets) - 1
        if voice_ids is not None:
            voice_ids = np.ascontiguousarray(voice_ids, dtype=np.uint32)
            assert len(voice_ids) == n_utt
        if jitter_seeds is not None:
            jitter_seeds = np.ascontiguousarray(jitter_seeds, dtype=np.uint32)
            assert len(jitter_seeds) == n_utt
        return seg_offsets, n_utt, voice_ids, jitter_seeds

    def upload(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None):
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        h = C.c_void_p()
        _check(load().grail_batch_upload(self.handle, segs.ctypes.data, seg_offsets.ctypes.data,
                                         _ptr(voice_ids), _ptr(jitter_seeds), n_utt, C.byref(h)))
        return Batch(self, h, n_utt)

    def upload_elems(self, seq_elems, seg_offsets, voice_ids=None, jitter_seeds=None):
        arr = (SequenceElem * max(len(seq_elems), 1))(*seq_elems)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, None, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        h = C.c_void_p()
        _check(load().grail_batch_upload_elems(self.handle, C.cast(arr, C.c_void_p),
                                               seg_offsets.ctypes.data, _ptr(voice_ids),
                                               _ptr(jitter_seeds), n_utt, C.byref(h)))
        return Batch(self, h, n_utt)

    def synthesize(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=None,
                   allow_truncation=False):
        """One-call form over host buffers.  Returns (out[n_utt, out_stride], out_len)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        if out_stride is None:
            b = self.upload(segs, seg_offsets, voice_ids, jitter_seeds)
            try:
                lens = b.lengths()
            finally:
                b.free()
            out_stride = int((max(int(lens.max()) if n_utt else 0, 1) + 3) // 4 * 4)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        st = load().grail_synthesize_batch(self.handle, segs.ctypes.data, seg_offsets.ctypes.data,
                                           _ptr(voice_ids), _ptr(jitter_seeds), n_utt,
                                           out.ctypes.data, out_stride, out_len.ctypes.data,
                                           OUT_HOST)
        if not (allow_truncation and st == ERR_BUFFER_TOO_SMALL):
            _check(st)
        return out[:n_utt], out_len[:n_utt]

    def synthesize_pcm16(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=4096):
        """One-call form with i16 PCM rows (examples/cli.rs:49 on the device)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.int16)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_synthesize_batch_pcm16(
            self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids),
            _ptr(jitter_seeds), n_utt, out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n_utt], out_len[:n_utt]

    def synthesize_elems(self, seq_elems, seg_offsets, voice_ids=None, jitter_seeds=None,
                         out_stride=4096):
        arr = (SequenceElem * max(len(seq_elems), 1))(*seq_elems)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, None, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_synthesize_batch_elems(
            self.handle, C.cast(arr, C.c_void_p), seg_offsets.ctypes.data, _ptr(voice_ids),
            _ptr(jitter_seeds), n_utt, out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n_utt], out_len[:n_utt]

    def say(self, texts, voice_ids=None, jitter_seeds=None, out_stride=None, seconds_per_char=1.6):
        """examples/cli.rs:175-184 for a list of texts. Returns (out[n, stride], out_len)."""
        n = len(texts)
        arr = (C.c_char_p * max(n, 1))(*[t.encode("utf-8") for t in texts])
        if voice_ids is not None:
            voice_ids = np.ascontiguousarray(voice_ids, dtype=np.uint32)
        if jitter_seeds is not None:
            jitter_seeds = np.ascontiguousarray(jitter_seeds, dtype=np.uint32)
        if out_stride is None:
            rate = max(v.sample_rate for v in self.get_voices())
            longest = max([len(t) for t in texts] + [1])
            out_stride = (int((longest * seconds_per_char + 1.0) * rate) + 63) // 64 * 64
        out = np.zeros((max(n, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n, 1), dtype=np.uint32)
        _check(load().grail_say_batch(self.handle, arr, n, _ptr(voice_ids), _ptr(jitter_seeds),
                                      out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n], out_len[:n]

    def pcm16(self, in_dev, in_stride, len_dev, n_utt, max_len, out_dev, out_stride):
        _check(load().grail_pcm16_async(self.handle, in_dev, in_stride, len_dev, n_utt, max_len,
                                        out_dev, out_stride))

    def mix_async(self, rows_dev, row_stride, row_len, item_rows, item_offsets, tracks_dev, track_stride, n_tracks,
                  track_len, item_tracks=None, item_gains=None, accumulate=False):
        """grail_mix_async: rows_dev [n_rows][row_stride] (row_len: host, one per row) mixed into tracks_dev
        [n_tracks][track_stride], queued on the context's stream."""
        row_len = np.ascontiguousarray(row_len, dtype=np.uint32)
        rows, offs, tracks, gains = _mix_items(item_rows, item_offsets, item_tracks, item_gains)
        _check(load().grail_mix_async(self.handle, rows_dev, row_stride, row_len.ctypes.data, len(row_len),
                                      rows.ctypes.data, _ptr(tracks), offs.ctypes.data, _ptr(gains), len(rows),
                                      tracks_dev, track_stride, n_tracks, track_len,
                                      MIX_ACCUMULATE if accumulate else 0))

    def pcm16_frames_async(self, tracks_dev, track_stride, n_tracks, n_frames, frames_dev):
        """grail_pcm16_frames_async: tracks -> interleaved i16 frames (frames_dev[f * n_tracks + t])."""
        _check(load().grail_pcm16_frames_async(self.handle, tracks_dev, track_stride, n_tracks, n_frames, frames_dev))

    def levels_async(self, rows_dev, row_stride, len_dev, n_rows, sumsq_dev=None, peak_dev=None, nonfinite_dev=None):
        """grail_levels_async: per row the binary64 sum of squares, the largest finite |x| and the count of non-finite
        samples, into DEVICE arrays [n_rows] (any may be None), queued on the context's stream."""
        _check(load().grail_levels_async(self.handle, rows_dev, row_stride, len_dev, n_rows, sumsq_dev, peak_dev,
                                         nonfinite_dev))

    def levels(self, rows_dev, row_stride, len_dev, n_rows):
        """levels_async, waited for and copied back: (sumsq float64, peak float32, nonfinite uint32), one per row."""
        sumsq = np.zeros(max(n_rows, 1), dtype=np.float64)
        peak = np.zeros(max(n_rows, 1), dtype=np.float32)
        bad = np.zeros(max(n_rows, 1), dtype=np.uint32)
        d = [self.device_alloc(max(n_rows, 1) * k) for k in (8, 4, 4)]
        try:
            self.levels_async(rows_dev, row_stride, len_dev, n_rows, *d)
            for dst, src in zip((sumsq, peak, bad), d):
                self.d2h(dst, src, n_rows * dst.itemsize)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return sumsq[:n_rows], peak[:n_rows], bad[:n_rows]

    def frame_levels_async(self, rows_dev, row_stride, len_dev, n_rows, frame, frame_sumsq_dev, frame_peak_dev,
                           frames_stride):
        """grail_frame_levels_async: per frame of `frame` samples, into DEVICE arrays [n_rows][frames_stride]."""
        _check(load().grail_frame_levels_async(self.handle, rows_dev, row_stride, len_dev, n_rows, frame, frame_sumsq_dev,
                                               frame_peak_dev, frames_stride))

    def frame_levels(self, rows_dev, row_stride, len_dev, n_rows, frame, fill=None):
        """frame_levels_async, waited for and copied back: (sumsq float64 [n_rows, frames], peak float32 [n_rows, frames])
        with frames = ceil(row_stride / frame).  Frames past a row's end hold `fill` (default NaN): the call leaves them
        unwritten."""
        frames = max(-(-int(row_stride) // int(frame)), 1)
        sumsq = np.full((max(n_rows, 1), frames), np.nan if fill is None else fill, dtype=np.float64)
        peak = np.full((max(n_rows, 1), frames), np.nan if fill is None else fill, dtype=np.float32)
        d = [self.device_alloc(sumsq.nbytes), self.device_alloc(peak.nbytes)]
        try:
            self.h2d(d[0], sumsq, sumsq.nbytes)
            self.h2d(d[1], peak, peak.nbytes)
            self.frame_levels_async(rows_dev, row_stride, len_dev, n_rows, frame, d[0], d[1], frames)
            self.d2h(sumsq, d[0], sumsq.nbytes)
            self.d2h(peak, d[1], peak.nbytes)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return sumsq[:n_rows], peak[:n_rows]

    def loudness_async(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, gated_ms_dev=None,
                       hop_sumsq_dev=None, hops_stride=0, nonfinite_dev=None):
        """grail_loudness_async: per row the K-weighted gated mean square, the hop sums [n_rows][hops_stride] and the count
        of non-finite samples, into DEVICE arrays (any may be None), queued on the context's stream.  coef: ten float64 or
        None = kweighting(sample_rate)."""
        c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
        assert c is None or c.shape == (10,)
        _check(load().grail_loudness_async(self.handle, rows_dev, row_stride, len_dev, n_rows, int(sample_rate), _ptr(c),
                                           gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev))

    def loudness_segmented_async(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, gated_ms_dev=None,
                                 hop_sumsq_dev=None, hops_stride=0, nonfinite_dev=None):
        """grail_loudness_segmented_async: loudness_async's arguments and outputs, every hop filtered from a zero state
        LOUDNESS_WARMUP_HOPS hops before it, one lane per hop: for few long rows (a finished track)."""
        c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
        assert c is None or c.shape == (10,)
        _check(load().grail_loudness_segmented_async(self.handle, rows_dev, row_stride, len_dev, n_rows, int(sample_rate),
                                                     _ptr(c), gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev))

    def loudness_segmented(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, hops=True, fill=None):
        """loudness_segmented_async, waited for and copied back: what loudness() returns."""
        return self._loudness_sync(self.loudness_segmented_async, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, hops,
                                   fill)

    def loudness(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, hops=True, fill=None):
        """loudness_async, waited for and copied back: (gated_ms float64 [n_rows], hop_sumsq float64 [n_rows, row_stride //
        hop] or None, nonfinite uint32 [n_rows]).  Hops past a row's last hold `fill` (default NaN): the call leaves them
        unwritten."""
        return self._loudness_sync(self.loudness_async, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, hops, fill)

    def _loudness_sync(self, call, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, hops, fill):
        hop = int(sample_rate) // 10
        hs = max(int(row_stride) // hop, 1) if hop else 1
        gated = np.zeros(max(n_rows, 1), dtype=np.float64)
        bad = np.zeros(max(n_rows, 1), dtype=np.uint32)
        hop_sumsq = np.full((max(n_rows, 1), hs), np.nan if fill is None else fill, dtype=np.float64) if hops else None
        d = [self.device_alloc(gated.nbytes), self.device_alloc(bad.nbytes)]
        if hops:
            d.append(self.device_alloc(hop_sumsq.nbytes))
        try:
            if hops:
                self.h2d(d[2], hop_sumsq, hop_sumsq.nbytes)
            call(rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, d[0], d[2] if hops else None,
                 hs if hops else 0, d[1])
            self.d2h(gated, d[0], gated.nbytes)
            self.d2h(bad, d[1], bad.nbytes)
            if hops:
                self.d2h(hop_sumsq, d[2], hop_sumsq.nbytes)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return gated[:n_rows], (hop_sumsq[:n_rows] if hops else None), bad[:n_rows]

    def true_peak_async(self, rows_dev, row_stride, len_dev, n_rows, true_peak_dev=None, nonfinite_dev=None):
        """grail_true_peak_async: per row the true peak (4x oversampled, BS.1770-4 Annex 2) and the count of non-finite
        samples, into DEVICE arrays [n_rows] (either may be None), queued on the context's stream."""
        _check(load().grail_true_peak_async(self.handle, rows_dev, row_stride, len_dev, n_rows, true_peak_dev,
                                            nonfinite_dev))

    def true_peak(self, rows_dev, row_stride, len_dev, n_rows):
        """true_peak_async, waited for and copied back: (true_peak float64, nonfinite uint32), one per row."""
        tp = np.zeros(max(n_rows, 1), dtype=np.float64)
        bad = np.zeros(max(n_rows, 1), dtype=np.uint32)
        d = [self.device_alloc(max(n_rows, 1) * k) for k in (8, 4)]
        try:
            self.true_peak_async(rows_dev, row_stride, len_dev, n_rows, *d)
            for dst, src in zip((tp, bad), d):
                self.d2h(dst, src, n_rows * dst.itemsize)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return tp[:n_rows], bad[:n_rows]

    def limit_async(self, rows_dev, row_stride, len_dev, n_rows, ceiling, lookahead_log2, out_dev, out_stride=None, group=1,
                    min_gain_dev=None, n_limited_dev=None, nonfinite_dev=None):
        """grail_limit_async: the look-ahead limiter over groups of `group` consecutive rows, into out_dev (must not overlap
        rows_dev); ceiling is linear (limit_ceiling gives it from dBTP), the look-ahead 2^lookahead_log2 samples.  Results
        are DEVICE arrays [n_rows // group] (any may be None), queued on the context's stream."""
        _check(load().grail_limit_async(self.handle, rows_dev, row_stride, len_dev, n_rows, group, float(np.float32(ceiling)),
                                        lookahead_log2, out_dev, row_stride if out_stride is None else out_stride,
                                        min_gain_dev, n_limited_dev, nonfinite_dev))

    def limit(self, rows_dev, row_stride, len_dev, n_rows, ceiling, lookahead_log2, out_dev, out_stride=None, group=1):
        """limit_async, waited for, the results copied back: (min_gain float32, n_limited uint32, nonfinite uint32), one per
        group; a refused group reads (NaN, LIMIT_REFUSED, 0)."""
        n_groups = n_rows // group if group else 0
        res = [np.zeros(max(n_groups, 1), dtype=t) for t in (np.float32, np.uint32, np.uint32)]
        d = [self.device_alloc(max(n_groups, 1) * 4) for _ in res]
        try:
            self.limit_async(rows_dev, row_stride, len_dev, n_rows, ceiling, lookahead_log2, out_dev, out_stride, group, *d)
            for dst, src in zip(res, d):
                self.d2h(dst, src, n_groups * 4)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return tuple(r[:n_groups] for r in res)

    def resample_async(self, rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev, out_stride, out_len_dev=None,
                       nonfinite_dev=None):
        """grail_resample_async: the rows at rate_in resampled to rate_out into out_dev (must not overlap rows_dev), output m
        at input time m * down / up.  Results are DEVICE arrays [n_rows] (either may be None), queued on the context's
        stream."""
        _check(load().grail_resample_async(self.handle, rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev,
                                           out_stride, out_len_dev, nonfinite_dev))

    def resample(self, rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev, out_stride):
        """resample_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row."""
        res = [np.zeros(max(n_rows, 1), dtype=np.uint32) for _ in range(2)]
        d = [self.device_alloc(max(n_rows, 1) * 4) for _ in res]
        try:
            self.resample_async(rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev, out_stride, *d)
            for dst, src in zip(res, d):
                self.d2h(dst, src, n_rows * 4)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return tuple(r[:n_rows] for r in res)

    def fir_create(self, filters):
        """grail_fir_create: a set of filters on this context's device.  filters: a list of (taps float32[K], origin), one per
        filter.  Returns the set's handle, for fir / fir_async / fir_free; sets still alive go with the context."""
        taps = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t, _ in filters]
        flat = np.concatenate(taps) if taps else np.zeros(0, np.float32)
        n_taps = np.array([len(t) for t in taps], dtype=np.uint32)
        origin = np.array([o for _, o in filters], dtype=np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_fir_create(self.handle, flat.ctypes.data, n_taps.ctypes.data, origin.ctypes.data, len(filters),
                                       C.addressof(out)))
        return out

    def fir_free(self, fir_set):
        """grail_fir_free: waits for the context's stream, then releases the set."""
        _check(load().grail_fir_free(self.handle, fir_set))

    def fir_async(self, fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride, out_len_dev=None,
                  nonfinite_dev=None):
        """grail_fir_async: the rows filtered into out_dev (must not overlap rows_dev), row u with filter filter_dev[u] of the
        set (a DEVICE array of uint32; None: filter 0 for every row).  Results are DEVICE arrays [n_rows] (either may be
        None), queued on the context's stream."""
        _check(load().grail_fir_async(self.handle, fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride,
                                      out_len_dev, nonfinite_dev))

    def fir(self, fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride):
        """fir_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row whose
        filter index is outside the set: (LIMIT_REFUSED, 0)."""
        res = [np.zeros(max(n_rows, 1), dtype=np.uint32) for _ in range(2)]
        d = [self.device_alloc(max(n_rows, 1) * 4) for _ in res]
        try:
            self.fir_async(fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride, *d)
            for dst, src in zip(res, d):
                self.d2h(dst, src, n_rows * 4)
        finally:
            self.sync()
            for p in d:
                self.device_free(p)
        return tuple(r[:n_rows] for r in res)

    def fir_stream_open(self, fir_set, n_rows, filters=None):
        """grail_filter_stream_open: a stream of n_rows rows filtered call by call, row u bound to filter filters[u] of the set
        (a host sequence; None: filter 0 for every row).  Returns the stream's handle, for fir_stream_next / _finish /
        _close; streams still open go with the context, and their set cannot be freed before them."""
        which = None if filters is None else np.ascontiguousarray(filters, dtype=np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_filter_stream_open(self.handle, fir_set, n_rows, None if which is None else which.ctypes.data,
                                               C.addressof(out)))
        return out

    def fir_stream_next_async(self, fs, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, nonfinite_dev=None):
        """grail_filter_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the outputs that
        became known go to out_dev + u * out_stride.  Results are DEVICE arrays [n_rows] (either may be None), queued on the
        context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_filter_stream_next_async(self.handle, fs, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev,
                                                     nonfinite_dev))

    def fir_stream_next(self, fs, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """fir_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row
        that had ended and was fed: (LIMIT_REFUSED, 0)."""
        return _waited(self, n_rows, (np.uint32, np.uint32),
                       lambda *d: self.fir_stream_next_async(fs, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def fir_stream_finish(self, fs, n_rows, out_dev, out_stride, which=None, out_len_dev=None):
        """grail_filter_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row)
        that have not ended write their tails and end.  out_len_dev None: waited for, and the tails' lengths (uint32, one
        per row; 0 for rows not marked or ended before) returned."""
        marks = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        assert marks is None or len(marks) == n_rows

        def finish(out_len):
            _check(load().grail_filter_stream_finish_async(self.handle, fs, None if marks is None else marks.ctypes.data, out_dev,
                                                          out_stride, out_len))
        return finish(out_len_dev) if out_len_dev is not None else _waited(self, n_rows, (np.uint32,), finish)[0]

    def fir_stream_close(self, fs):
        """grail_filter_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_filter_stream_close(self.handle, fs))

    def iir_create(self, filters):
        """grail_iir_create: a set of recursive filters on this context's device.  filters: a list of float64 arrays [S][5]
        (or flat [5 S]), the sections b0 b1 b2 a1 a2 of one filter each.  Returns the set's handle, for iir / iir_async /
        iir_free / iir_stream_open; sets still alive go with the context."""
        secs = [np.ascontiguousarray(f, dtype=np.float64).reshape(-1) for f in filters]
        flat = np.concatenate(secs) if secs else np.zeros(0, np.float64)
        n_sections = np.array([len(f) // 5 for f in secs], dtype=np.uint32)
        assert all(len(f) % 5 == 0 for f in secs)
        out = C.c_void_p(None)
        _check(load().grail_iir_create(self.handle, flat.ctypes.data, n_sections.ctypes.data, len(filters), C.addressof(out)))
        return out

    def iir_free(self, iir_set):
        """grail_iir_free: waits for the context's stream, then releases the set (refused while it has open streams)."""
        _check(load().grail_iir_free(self.handle, iir_set))

    def iir_async(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride, out_len_dev=None,
                  nonfinite_dev=None):
        """grail_iir_async: the rows filtered into out_dev (must not overlap rows_dev), row u with filter filter_dev[u] of the
        set (a DEVICE array of uint32; None: filter 0 for every row), ringing out over `tail` outputs past its last sample.
        Results are DEVICE arrays [n_rows] (either may be None), queued on the context's stream."""
        _check(load().grail_iir_async(self.handle, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev,
                                      out_stride, out_len_dev, nonfinite_dev))

    def iir(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride):
        """iir_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row whose
        filter index is outside the set: (LIMIT_REFUSED, 0)."""
        return _waited(self, n_rows, (np.uint32, np.uint32),
                       lambda *d: self.iir_async(iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev,
                                                 out_stride, *d))

    def iir_blocked_async(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride,
                          out_len_dev=None, nonfinite_dev=None):
        """grail_biquad_blocked_async: iir_async's arguments and results, parallel in time: a row's steps in blocks of IIR_BLOCK,
        a lane each.  The call for a few long rows; bit for bit iir_async's up to a row's IIR_BLOCK-th output, its own
        contract from there on."""
        _check(load().grail_biquad_blocked_async(self.handle, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail,
                                              out_dev, out_stride, out_len_dev, nonfinite_dev))

    def iir_blocked(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride):
        """iir_blocked_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row
        whose filter index is outside the set: (LIMIT_REFUSED, 0)."""
        return _waited(self, n_rows, (np.uint32, np.uint32),
                       lambda *d: self.iir_blocked_async(iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail,
                                                         out_dev, out_stride, *d))

    def iir_stream_open(self, iir_set, n_rows, filters=None, tail=0):
        """grail_iir_stream_open: a stream of n_rows rows filtered recursively call by call, row u bound to filter filters[u]
        of the set (a host sequence; None: filter 0 for every row), every row ringing out over `tail` outputs at its finish.
        Returns the stream's handle, for iir_stream_next / _finish / _close."""
        which = None if filters is None else np.ascontiguousarray(filters, dtype=np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_iir_stream_open(self.handle, iir_set, n_rows, None if which is None else which.ctypes.data, tail,
                                            C.addressof(out)))
        return out

    def iir_stream_next_async(self, st, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, nonfinite_dev=None):
        """grail_iir_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples and writes as many
        outputs to out_dev + u * out_stride.  Results are DEVICE arrays [n_rows] (either may be None)."""
        _check(load().grail_iir_stream_next_async(self.handle, st, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev,
                                                  nonfinite_dev))

    def iir_stream_next(self, st, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """iir_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row
        that had ended and was fed: (LIMIT_REFUSED, 0)."""
        return _waited(self, n_rows, (np.uint32, np.uint32),
                       lambda *d: self.iir_stream_next_async(st, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def iir_stream_finish(self, st, n_rows, out_dev, out_stride, which=None, out_len_dev=None):
        """grail_iir_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row) that
        have not ended write their tails and end.  out_len_dev None: waited for, and the tails' lengths (uint32, one per row;
        0 for rows not marked, ended before or fed nothing) returned."""
        marks = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        assert marks is None or len(marks) == n_rows

        def finish(out_len):
            _check(load().grail_iir_stream_finish_async(self.handle, st, None if marks is None else marks.ctypes.data, out_dev,
                                                       out_stride, out_len))
        return finish(out_len_dev) if out_len_dev is not None else _waited(self, n_rows, (np.uint32,), finish)[0]

    def iir_stream_close(self, st):
        """grail_iir_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_iir_stream_close(self.handle, st))

    def dyn_create(self, curves):
        """grail_dyn_create: a set of gain curves on this context's device.  curves: a list of (gain float64[DYN_POINTS], (alpha_attack,
        alpha_release), detector), as dyn_design and dyn_ballistics return them or the caller's own.  Returns the set's handle, for
        dyn / dyn_async / dyn_free / dyn_stream_open; sets still alive go with the context."""
        gain = np.ascontiguousarray([np.asarray(c[0], dtype=np.float64) for c in curves], dtype=np.float64).reshape(-1)
        assert len(gain) == DYN_POINTS * len(curves)
        alpha = np.ascontiguousarray([c[1] for c in curves], dtype=np.float64).reshape(-1)
        detector = np.array([c[2] for c in curves], dtype=np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_dyn_create(self.handle, gain.ctypes.data, alpha.ctypes.data, detector.ctypes.data, len(curves),
                                       C.addressof(out)))
        return out

    def dyn_free(self, dyn_set):
        """grail_dyn_free: waits for the context's stream, then releases the set (refused while it has open streams)."""
        _check(load().grail_dyn_free(self.handle, dyn_set))

    def dyn_async(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, out_len_dev=None,
                  nonfinite_dev=None, min_gain_dev=None, key_dev=None, key_stride=0, key_len_dev=None, n_keys=0, key_row_dev=None):
        """grail_dyn_async: the rows times the gain their curve (curve_dev: a DEVICE array of uint32; None: curve 0 for every row)
        gives at their envelope, into out_dev (must overlap neither rows_dev nor the keys).  key_dev None: every row follows
        itself; else row u follows key key_row_dev[u] (None: key u) of the n_keys rows at key_dev.  Results are DEVICE arrays
        [n_rows] (each may be None; min_gain is float64), queued on the context's stream."""
        _check(load().grail_dyn_async(self.handle, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, key_dev, key_stride,
                                      key_len_dev, n_keys, key_row_dev, out_dev, out_stride, out_len_dev, nonfinite_dev, min_gain_dev))

    def dyn(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, key_dev=None, key_stride=0,
            key_len_dev=None, n_keys=0, key_row_dev=None):
        """dyn_async, waited for, the results copied back: (out_len uint32, nonfinite uint32, min_gain float64), one per row; a
        row whose curve or key index is outside: (LIMIT_REFUSED, 0, NaN)."""
        return _waited_sized(self, n_rows, (np.uint32, np.uint32, np.float64),
                             lambda *d: self.dyn_async(dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride,
                                                       *d, key_dev=key_dev, key_stride=key_stride, key_len_dev=key_len_dev,
                                                       n_keys=n_keys, key_row_dev=key_row_dev))

    def track_dyn_async(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, out_len_dev=None,
                        nonfinite_dev=None, min_gain_dev=None, key_dev=None, key_stride=0, key_len_dev=None, n_keys=0, key_row_dev=None):
        """grail_track_dyn_async: dyn_async's arguments, results and bits with a workgroup a row, for the few long tracks of a
        mix (the header's WHICH CALL FOR WHAT says below how many rows)."""
        _check(load().grail_track_dyn_async(self.handle, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, key_dev, key_stride,
                                            key_len_dev, n_keys, key_row_dev, out_dev, out_stride, out_len_dev, nonfinite_dev,
                                            min_gain_dev))

    def track_dyn(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, key_dev=None, key_stride=0,
                  key_len_dev=None, n_keys=0, key_row_dev=None):
        """track_dyn_async, waited for, the results copied back as dyn does: (out_len uint32, nonfinite uint32, min_gain
        float64), one per row."""
        return _waited_sized(self, n_rows, (np.uint32, np.uint32, np.float64),
                             lambda *d: self.track_dyn_async(dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev,
                                                             out_stride, *d, key_dev=key_dev, key_stride=key_stride,
                                                             key_len_dev=key_len_dev, n_keys=n_keys, key_row_dev=key_row_dev))

    def dyn_stream_open(self, dyn_set, n_rows, curves=None, n_keys=0, key_rows=None):
        """grail_dyn_stream_open: a stream of n_rows rows compressed call by call, row u bound to curve curves[u] of the set (a
        host sequence; None: curve 0 for every row).  n_keys = 0: every row follows itself; else row u follows key key_rows[u]
        (a host sequence; None: key u) of the n_keys key rows each call brings.  Returns the stream's handle, for
        dyn_stream_next / _close."""
        which = None if curves is None else np.ascontiguousarray(curves, dtype=np.uint32)
        keys = None if key_rows is None else np.ascontiguousarray(key_rows, dtype=np.uint32)
        assert (which is None or len(which) == n_rows) and (keys is None or len(keys) == n_rows)
        out = C.c_void_p(None)
        _check(load().grail_dyn_stream_open(self.handle, dyn_set, n_rows, None if which is None else which.ctypes.data, n_keys,
                                            None if keys is None else keys.ctypes.data, C.addressof(out)))
        return out

    def dyn_stream_next_async(self, st, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, nonfinite_dev=None,
                              min_gain_dev=None, key_dev=None, key_stride=0):
        """grail_dyn_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples (and, keyed, reads as many
        of its key at key_dev) and writes as many outputs to out_dev + u * out_stride.  Results are DEVICE arrays [n_rows] (each
        may be None; min_gain is float64)."""
        _check(load().grail_dyn_stream_next_async(self.handle, st, in_dev, in_stride, in_len_dev, key_dev, key_stride, out_dev,
                                                  out_stride, out_len_dev, nonfinite_dev, min_gain_dev))

    def dyn_stream_next(self, st, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride, key_dev=None, key_stride=0):
        """dyn_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32, min_gain float64), one
        per row."""
        return _waited_sized(self, n_rows, (np.uint32, np.uint32, np.float64),
                             lambda *d: self.dyn_stream_next_async(st, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d,
                                                                   key_dev=key_dev, key_stride=key_stride))

    def dyn_stream_close(self, st):
        """grail_dyn_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_dyn_stream_close(self.handle, st))

    def resample_stream_open(self, rate_in, rate_out, n_rows):
        """grail_resample_stream_open: a stream of n_rows rows resampled call by call from rate_in to rate_out.  Returns the
        stream's handle, for resample_stream_next / _finish / _close; streams still open go with the context."""
        out = C.c_void_p(None)
        _check(load().grail_resample_stream_open(self.handle, rate_in, rate_out, n_rows, C.addressof(out)))
        return out

    def resample_stream_next_async(self, rs, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None,
                                   nonfinite_dev=None):
        """grail_resample_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the outputs that
        became known go to out_dev + u * out_stride (out_stride >= resample_len(in_stride)).  Results are DEVICE arrays
        [n_rows] (either may be None), queued on the context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_resample_stream_next_async(self.handle, rs, in_dev, in_stride, in_len_dev, out_dev, out_stride,
                                                       out_len_dev, nonfinite_dev))

    def resample_stream_next(self, rs, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """resample_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a
        row that had ended and was fed: (LIMIT_REFUSED, 0)."""
        return _waited(self, n_rows, (np.uint32, np.uint32),
                       lambda *d: self.resample_stream_next_async(rs, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def resample_stream_finish(self, rs, n_rows, out_dev, out_stride, which=None, out_len_dev=None):
        """grail_resample_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row)
        that have not ended write their tails and end.  out_len_dev None: waited for, and the tails' lengths (uint32, one
        per row; 0 for rows not marked or ended before) returned."""
        marks = None if which is None else np.ascontiguousarray(which, dtype=np.uint8)
        assert marks is None or len(marks) == n_rows

        def finish(out_len):
            _check(load().grail_resample_stream_finish_async(self.handle, rs, None if marks is None else marks.ctypes.data, out_dev,
                                                            out_stride, out_len))
        return finish(out_len_dev) if out_len_dev is not None else _waited(self, n_rows, (np.uint32,), finish)[0]

    def resample_stream_close(self, rs):
        """grail_resample_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_resample_stream_close(self.handle, rs))

    def limit_stream_open(self, n_rows, ceiling, lookahead_log2, group=1):
        """grail_limit_stream_open: a stream of n_rows rows in groups of `group`, limited call by call under `ceiling` (linear)
        with a look-ahead of 2^lookahead_log2 samples.  Returns a LimitStream; streams still open go with the context."""
        out = C.c_void_p(None)
        _check(load().grail_limit_stream_open(self.handle, n_rows, group, float(np.float32(ceiling)), lookahead_log2, C.addressof(out)))
        return LimitStream(self, out, n_rows, group, lookahead_log2)

    def meter_stream_open(self, n_rows, sample_rate, max_hops, coef=None):
        """grail_meter_stream_open: a stream of n_rows rows metered call by call at sample_rate (coef: float64 [10], None:
        kweighting(sample_rate)), each row's ledger holding max_hops hops.  Returns a MeterStream; streams still open go
        with the context."""
        out = C.c_void_p()
        c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
        assert c is None or c.shape == (10,)
        _check(load().grail_meter_stream_open(self.handle, n_rows, int(sample_rate), _ptr(c), int(max_hops), C.addressof(out)))
        return MeterStream(self, out, n_rows, int(sample_rate), int(max_hops))

    def digest(self, in_dev, in_stride, len_dev, n_utt):
        """(bit-pattern sums mod 2^64, max finite |x|, non-finite counts) per row, computed on the device (every length
        at most the stride).  A sum is blind to samples permuted within a row: use compare beside it."""
        sums = np.zeros(max(n_utt, 1), dtype=np.uint64)
        maxabs = np.zeros(max(n_utt, 1), dtype=np.float32)
        bad = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_digest(self.handle, in_dev, in_stride, len_dev, n_utt,
                                         sums.ctypes.data, maxabs.ctypes.data, bad.ctypes.data))
        return sums[:n_utt], maxabs[:n_utt], bad[:n_utt]

    def compare(self, a_dev, b_dev, stride, len_a_dev, len_b_dev, n_utt):
        """(max |a-b|, sum (a-b)^2, structural mismatches) per row of two device renderings, over the first len_a samples
        (every length at most the stride).  A sample whose |a-b| is not finite enters neither number and is a mismatch
        unless both sides carry the same bits or both are NaN; +1 where the lengths differ; -0.0 equals +0.0."""
        md = np.zeros(max(n_utt, 1), dtype=np.float32)
        sq = np.zeros(max(n_utt, 1), dtype=np.float64)
        bad = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_compare(self.handle, a_dev, b_dev, stride, len_a_dev, len_b_dev, n_utt,
                                          md.ctypes.data, sq.ctypes.data, bad.ctypes.data))
        return md[:n_utt], sq[:n_utt], bad[:n_utt]

    def h2d(self, dst_dev, src, nbytes):
        _check(load().grail_memcpy_h2d(self.handle, dst_dev, src.ctypes.data, nbytes))

    def sync(self):
        _check(load().grail_sync(self.handle))

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(load().grail_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value

    def last_kernel_name(self):
        return load().grail_last_kernel_name(self.handle).decode()

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        _check(load().grail_device_alloc(self.handle, nbytes, C.byref(p)))
        return p

    def device_free(self, p):
        _check(load().grail_device_free(self.handle, p))

    def host_alloc(self, shape, dtype):
        """A numpy array in pinned host memory (grail_host_alloc); free it with host_free(array)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        _check(load().grail_host_alloc(self.handle, n, C.byref(p)))
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        _check(load().grail_host_free(self.handle, p))

    def synthesize_into(self, out, out_len, segs, seg_offsets, voice_ids=None, jitter_seeds=None):
        """One-call form into a caller-owned host array out[n_utt, out_stride] (f32 or i16)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets, voice_ids,
                                                                 jitter_seeds)
        assert out.shape[0] >= n_utt and out.flags.c_contiguous
        fn = load().grail_synthesize_batch if out.dtype == np.float32 else load().grail_synthesize_batch_pcm16
        _check(fn(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids), _ptr(jitter_seeds),
                  n_utt, out.ctypes.data, out.shape[1], out_len.ctypes.data, OUT_HOST))

    def d2h(self, dst, src_dev, nbytes, offset=0):
        src = C.c_void_p(src_dev.value + offset)
        _check(load().grail_memcpy_d2h(self.handle, dst.ctypes.data, src, nbytes))

    def memset(self, dst_dev, value, nbytes):
        _check(load().grail_memset_d(self.handle, dst_dev, value, nbytes))

    # RCCL
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        _check(load().grail_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        _check(load().grail_comm_init(self.handle, buf, rank, world))

    def broadcast_voices(self, n_voices, root=0):
        _check(load().grail_broadcast_voices(self.handle, n_voices, root))

    def comm_info(self):
        """(ncclCommCount, ncclCommUserRank) of this context's communicator; (0, 0) without one."""
        n, r = C.c_uint32(), C.c_uint32()
        _check(load().grail_comm_info(self.handle, C.byref(n), C.byref(r)))
        return n.value, r.value


class _BorrowedContext(Context):
    """A node's context (grail_node_context): owned by the node, never destroyed from here."""

    def __init__(self, handle, device):       # noqa: super().__init__ would create a context
        self.handle, self.device = handle, device

    def close(self):
        self.handle = None


class Node:
    """grail_node: one process, several GPUs — a context and a host thread per device; one call renders a batch over all
    of them (contiguous shards, no data-path collective; the voice table travels by one ncclBroadcast)."""

    def __init__(self, devices, voices_without_rccl=False):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check(load().grail_node_create(arr, len(self.devices), C.byref(h)))
        self.handle = h
        if voices_without_rccl:
            self.set_option("node_voices_without_rccl", 1)

    def close(self):
        if self.handle:
            load().grail_node_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def size(self):
        return int(load().grail_node_size(self.handle))

    def context(self, index):
        h = C.c_void_p()
        _check(load().grail_node_context(self.handle, index, C.byref(h)))
        return _BorrowedContext(h, self.devices[index])

    def set_voices(self, voices):
        arr = (Voice * len(voices))(*[v.copy() for v in voices])
        _check(load().grail_node_set_voices(self.handle, C.cast(arr, C.c_void_p), len(voices)))

    def set_option(self, name, value):
        _check(load().grail_node_set_option(self.handle, name.encode(), value))

    def get_option(self, name):
        v = C.c_int64()
        _check(load().grail_node_get_option(self.handle, name.encode(), C.byref(v)))
        return v.value

    def lengths(self, segs, seg_offsets, voice_ids=None, max_len=0xFFFFFFFF):
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, _ = Context._prep(None, segs, seg_offsets, voice_ids, None)
        out = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_node_lengths(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids), n_utt,
                                         max_len, out.ctypes.data))
        return out[:n_utt]

    def synthesize(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=None, out=None,
                   allow_truncation=False, pcm16=False):
        """grail_node_synthesize_batch(_pcm16) over host buffers.  Returns (out[n_utt, out_stride], out_len)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = Context._prep(None, segs, seg_offsets, voice_ids, jitter_seeds)
        if out is not None:
            out_stride = out.shape[1]
            assert out.shape[0] >= n_utt and out.flags.c_contiguous
            pcm16 = out.dtype == np.int16
        elif out_stride is None:
            lens = self.lengths(segs, seg_offsets, voice_ids)
            out_stride = int((max(int(lens.max()) if n_utt else 0, 1) + 63) // 64 * 64)
        if out is None:
            out = np.zeros((max(n_utt, 1), out_stride), dtype=np.int16 if pcm16 else np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        fn = load().grail_node_synthesize_batch_pcm16 if pcm16 else load().grail_node_synthesize_batch
        st = fn(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids), _ptr(jitter_seeds), n_utt,
                out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST)
        if not (allow_truncation and st == ERR_BUFFER_TOO_SMALL):
            _check(st)
        return out[:n_utt], out_len[:n_utt]

    def synthesize_device(self, segs, seg_offsets, voice_ids, jitter_seeds, out_dev, out_stride):
        """grail_node_synthesize_batch_device: slot i's shard into out_dev[i] (device memory of its GPU).  Returns out_len."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = Context._prep(None, segs, seg_offsets, voice_ids, jitter_seeds)
        ptrs = (C.c_void_p * self.size())(*[p if p is None or isinstance(p, C.c_void_p) else C.c_void_p(p) for p in out_dev])
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_node_synthesize_batch_device(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids),
                                                         _ptr(jitter_seeds), n_utt, ptrs, out_stride, out_len.ctypes.data))
        return out_len[:n_utt]

    def synthesize_elems(self, seq_elems, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=4096):
        arr = (SequenceElem * max(len(seq_elems), 1))(*seq_elems)
        seg_offsets, n_utt, voice_ids, jitter_seeds = Context._prep(None, None, seg_offsets, voice_ids, jitter_seeds)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_node_synthesize_batch_elems(
            self.handle, C.cast(arr, C.c_void_p), seg_offsets.ctypes.data, _ptr(voice_ids), _ptr(jitter_seeds), n_utt,
            out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n_utt], out_len[:n_utt]

    def say(self, texts, voice_ids=None, jitter_seeds=None, out_stride=4096):
        n = len(texts)
        arr = (C.c_char_p * max(n, 1))(*[t.encode("utf-8") for t in texts])
        if voice_ids is not None:
            voice_ids = np.ascontiguousarray(voice_ids, dtype=np.uint32)
        if jitter_seeds is not None:
            jitter_seeds = np.ascontiguousarray(jitter_seeds, dtype=np.uint32)
        out = np.zeros((max(n, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n, 1), dtype=np.uint32)
        _check(load().grail_node_say_batch(self.handle, arr, n, _ptr(voice_ids), _ptr(jitter_seeds), out.ctypes.data,
                                           out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n], out_len[:n]

    def last_shard_ms(self):
        ms = (C.c_float * self.size())()
        _check(load().grail_node_last_shard_ms(self.handle, ms, self.size()))
        return [float(x) for x in ms]

    def host_alloc(self, shape, dtype):
        """A numpy array in pinned host memory every device of the node can copy into; free it with host_free(array)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        _check(load().grail_node_host_alloc(self.handle, n, C.byref(p)))
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        _check(load().grail_node_host_free(self.handle, p))
