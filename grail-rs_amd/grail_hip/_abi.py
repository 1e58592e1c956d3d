"""The C ABI as ctypes sees it: the constants and structures of include/grail_hip.h, the signature of every function it
declares (_SIGNATURES, which tests/test_abi.py holds to the header), and load()."""
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


def _sig(*argtypes, ret=C.c_int):
    """One row of _SIGNATURES: (restype, argtypes); most functions return a status."""
    return ret, list(argtypes)


def _signatures():
    P = C.POINTER
    vp, cp, usz = C.c_void_p, C.c_char_p, C.c_size_t
    i32, i64, u32, u64, f32, f64 = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double
    vpp, i32p, u32p, f32p, f64p = P(vp), P(i32), P(u32), P(f32), P(f64)
    elem, voice, rule, blocks = P(SynthesisElem), P(Voice), P(Rule), P(PlanBlock)
    return {
        "grail_abi_version": _sig(),
        "grail_status_string": _sig(i32, ret=cp),
        "grail_last_error": _sig(ret=cp),
        "grail_elem_silent": _sig(elem, ret=None),
        "grail_elem_new_phoneme": _sig(elem, f32p, f32p, f32p, f32p, f32p, f32p, ret=None),
        "grail_elem_new": _sig(elem, f32, f32, f32p, f32p, f32p, f32p, f32p, f32p, ret=None),
        "grail_elem_resample": _sig(elem, f32, f32, ret=None),
        "grail_elem_blend": _sig(elem, elem, elem, f32, ret=None),
        "grail_voice_generic": _sig(voice, ret=None),
        "grail_voice_generic_at": _sig(voice, f32, ret=None),
        "grail_voice_get": _sig(voice, i32, elem),
        "grail_create": _sig(i32, vpp),
        "grail_destroy": _sig(vp),
        "grail_device_count": _sig(i32p),
        "grail_device_pci_bus_id": _sig(vp, cp, usz),
        "grail_time_split_warmup": _sig(voice, ret=u32),
        "grail_length_bound": _sig(f32p, u32, f32, ret=u64),
        "grail_time_split_grid": _sig(u32, u32, u32, u32, u32p),
        "grail_fast_sharpness": _sig(voice, ret=f32),
        "grail_plan_blocks": _sig(u32, i32, i32, u32, u32, u32, blocks, u32, u32p),
        "grail_plan_ragged_blocks": _sig(u32, i32, i32, u32, u32, u32p, u32p, u32p, blocks, u32, u32p),
        "grail_dispatch_model": _sig(u32, u32, f64p, u32p, u32, f64p),
        "grail_packed_launch_order": _sig(u32, u32, f64p, u32, u32p),
        "grail_set_voices": _sig(vp, vp, u32),
        "grail_get_voices": _sig(vp, vp, u32, u32p),
        "grail_set_option": _sig(vp, cp, i64),
        "grail_get_option": _sig(vp, cp, P(i64)),
        "grail_batch_upload": _sig(vp, vp, vp, vp, vp, u32, vpp),
        "grail_batch_upload_elems": _sig(vp, vp, vp, vp, vp, u32, vpp),
        "grail_batch_free": _sig(vp, vp),
        "grail_batch_size": _sig(vp, ret=u32),
        "grail_batch_lengths": _sig(vp, vp, u32, vp),
        "grail_batch_synthesize_async": _sig(vp, vp, vp, u64, vp),
        "grail_sync": _sig(vp),
        "grail_last_kernel_ms": _sig(vp, f32p),
        "grail_last_kernel_name": _sig(vp, ret=cp),
        "grail_synthesize_batch": _sig(vp, vp, vp, vp, vp, u32, vp, u64, vp, u32),
        "grail_synthesize_batch_elems": _sig(vp, vp, vp, vp, vp, u32, vp, u64, vp, u32),
        "grail_stream_open": _sig(vp, vp, vpp),
        "grail_stream_next_async": _sig(vp, vp, u32, vp, u64, vp),
        "grail_stream_close": _sig(vp, vp),
        "grail_stream_open_live": _sig(vp, u32, vp, vp, u32, i32, vpp),
        "grail_stream_append": _sig(vp, vp, vp, vp),
        "grail_stream_append_elems": _sig(vp, vp, vp, vp),
        "grail_stream_finish": _sig(vp, vp, vp),
        "grail_stream_pending": _sig(vp, vp, vp),
        "grail_language_generic": _sig(P(rule), i32p, ret=u32),
        "grail_transcribe": _sig(u32p, u32, rule, u32, i32, i32, i32p, u32, u32p),
        "grail_intonate": _sig(voice, i32p, u32, vp),
        "grail_text_to_phoneme_elems": _sig(voice, cp, vp, u32, u32p),
        "grail_synthesize_batch_pcm16": _sig(vp, vp, vp, vp, vp, u32, vp, u64, vp, u32),
        "grail_batch_synthesize_pcm16_async": _sig(vp, vp, vp, u64, vp),
        "grail_stream_next_pcm16_async": _sig(vp, vp, u32, vp, u64, vp),
        "grail_say_batch": _sig(vp, P(cp), u32, vp, vp, vp, u64, vp, u32),
        "grail_pcm16_async": _sig(vp, vp, u64, vp, u32, u32, vp, u64),
        "grail_batch_digest": _sig(vp, vp, u64, vp, u32, vp, vp, vp),
        "grail_batch_compare": _sig(vp, vp, vp, u64, vp, vp, u32, vp, vp, vp),
        "grail_wav_write_i16": _sig(cp, vp, u32, u32),
        "grail_device_alloc": _sig(vp, usz, vpp),
        "grail_device_free": _sig(vp, vp),
        "grail_host_alloc": _sig(vp, usz, vpp),
        "grail_host_free": _sig(vp, vp),
        "grail_memcpy_d2h": _sig(vp, vp, vp, usz),
        "grail_memcpy_h2d": _sig(vp, vp, vp, usz),
        "grail_memset_d": _sig(vp, vp, i32, usz),
        "grail_shard_range": _sig(u64, u32, u32, P(u64), P(u64), ret=None),
        "grail_comm_unique_id": _sig(vp),
        "grail_comm_init": _sig(vp, vp, u32, u32),
        "grail_broadcast_voices": _sig(vp, u32, u32),
        "grail_comm_info": _sig(vp, u32p, u32p),
        "grail_comm_destroy": _sig(vp),
        "grail_node_create": _sig(i32p, u32, vpp),
        "grail_node_destroy": _sig(vp),
        "grail_node_size": _sig(vp, ret=u32),
        "grail_node_context": _sig(vp, u32, vpp),
        "grail_node_set_voices": _sig(vp, vp, u32),
        "grail_node_set_option": _sig(vp, cp, i64),
        "grail_node_get_option": _sig(vp, cp, P(i64)),
        "grail_node_shard_of": _sig(u32p, u64, u32, u32, P(NodeShard), u32p, u64),
        "grail_node_synthesize_batch": _sig(vp, vp, vp, vp, vp, u32, vp, u64, vp, u32),
        "grail_node_synthesize_batch_elems": _sig(vp, vp, vp, vp, vp, u32, vp, u64, vp, u32),
        "grail_node_synthesize_batch_pcm16": _sig(vp, vp, vp, vp, vp, u32, vp, u64, vp, u32),
        "grail_node_synthesize_batch_device": _sig(vp, vp, vp, vp, vp, u32, vpp, u64, vp),
        "grail_node_say_batch": _sig(vp, P(cp), u32, vp, vp, vp, u64, vp, u32),
        "grail_node_lengths": _sig(vp, vp, vp, vp, u32, u32, vp),
        "grail_node_last_shard_ms": _sig(vp, f32p, u32),
        "grail_node_host_alloc": _sig(vp, usz, vpp),
        "grail_node_host_free": _sig(vp, vp),
        "grail_mix_async": _sig(vp, vp, u64, vp, u32, vp, vp, vp, vp, u32, vp, u64, u32, u64, u32),
        "grail_batch_mix": _sig(vp, vp, vp, vp, vp, vp, u32, vp, u64, u32, u64, vp, u32),
        "grail_mix_place_sequential": _sig(vp, u32, vp, vp, vp, u32, u32, vp, vp),
        "grail_pcm16_frames_async": _sig(vp, vp, u64, u32, u64, vp),
        "grail_wav_write_i16_frames": _sig(cp, vp, u32, u32, u32),
        "grail_levels_async": _sig(vp, vp, u64, vp, u32, vp, vp, vp),
        "grail_frame_levels_async": _sig(vp, vp, u64, vp, u32, u32, vp, vp, u64),
        "grail_level_gains": _sig(i32, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp),
        "grail_active_level": _sig(vp, u32, u32, f32, ret=f64),
        "grail_batch_mix_leveled": _sig(vp, vp, vp, vp, vp, vp, i32, u32, vp, u64, u32, u64, vp, vp, vp, u32),
        "grail_kweighting": _sig(u32, vp),
        "grail_loudness_async": _sig(vp, vp, u64, vp, u32, u32, vp, vp, vp, u64, vp),
        "grail_gated_mean_square": _sig(vp, u32, u32, ret=f64),
        "grail_loudness_lufs": _sig(f64, ret=f64),
        "grail_loudness_level": _sig(f64, ret=f64),
        "grail_loudness_segmented_async": _sig(vp, vp, u64, vp, u32, u32, vp, vp, vp, u64, vp),
        "grail_loudness_window_max": _sig(vp, u32, u32, u32, ret=f64),
        "grail_loudness_range": _sig(vp, u32, u32, ret=f64),
        "grail_true_peak_coefficients": _sig(vp),
        "grail_true_peak_async": _sig(vp, vp, u64, vp, u32, vp, vp),
        "grail_true_peak_db": _sig(f64, ret=f64),
        "grail_true_peak_limit_gains": _sig(vp, u32, vp, u32, f32, vp, vp),
        "grail_batch_mix_leveled_limited": _sig(vp, vp, vp, vp, vp, vp, i32, u32, vp, u64, u32, u64, vp, vp, vp, f32, vp, u32),
        "grail_limit_ceiling": _sig(f32, ret=f32),
        "grail_limit_async": _sig(vp, vp, u64, vp, u32, u32, f32, u32, vp, u64, vp, vp, vp),
        "grail_resample_ratio": _sig(u32, u32, vp, vp, vp),
        "grail_resample_coefficients": _sig(u32, u32, vp, u32),
        "grail_resample_len": _sig(u64, u32, u32, vp),
        "grail_resample_async": _sig(vp, vp, u64, vp, u32, u32, u32, vp, u64, vp, vp),
        "grail_fir_len": _sig(u64, u32, u32, vp),
        "grail_fir_design": _sig(u32, f64, f64, u32, vp),
        "grail_fir_create": _sig(vp, vp, vp, vp, u32, vp),
        "grail_fir_free": _sig(vp, vp),
        "grail_fir_async": _sig(vp, vp, vp, u64, vp, u32, vp, vp, u64, vp, vp),
        "grail_filter_stream_len": _sig(u64, u64, u32, u32, i32, vp),
        "grail_filter_stream_open": _sig(vp, vp, u32, vp, vp),
        "grail_filter_stream_next_async": _sig(vp, vp, vp, u64, vp, vp, u64, vp, vp),
        "grail_filter_stream_finish_async": _sig(vp, vp, vp, vp, u64, vp),
        "grail_filter_stream_close": _sig(vp, vp),
        "grail_resample_stream_len": _sig(u64, u64, u32, u32, i32, vp),
        "grail_resample_stream_open": _sig(vp, u32, u32, u32, vp),
        "grail_resample_stream_next_async": _sig(vp, vp, vp, u64, vp, vp, u64, vp, vp),
        "grail_resample_stream_finish_async": _sig(vp, vp, vp, vp, u64, vp),
        "grail_resample_stream_close": _sig(vp, vp),
        "grail_limit_stream_len": _sig(u64, u64, u32, i32, vp),
        "grail_limit_stream_open": _sig(vp, u32, u32, f32, u32, vp),
        "grail_limit_stream_next_async": _sig(vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp),
        "grail_limit_stream_finish_async": _sig(vp, vp, vp, vp, u64, vp, vp, vp),
        "grail_limit_stream_close": _sig(vp, vp),
        "grail_meter_stream_hops": _sig(u64, u64, u32, vp),
        "grail_meter_stream_open": _sig(vp, u32, u32, vp, u64, vp),
        "grail_meter_stream_next_async": _sig(vp, vp, vp, u64, vp, vp, u64, vp, vp, vp),
        "grail_meter_stream_read_async": _sig(vp, vp, vp, vp, vp, vp, vp),
        "grail_meter_stream_ledger": _sig(vp, vp, vp, vp),
        "grail_meter_stream_finish_async": _sig(vp, vp, vp, vp),
        "grail_meter_stream_close": _sig(vp, vp),
        "grail_iir_design": _sig(i32, u32, f64, f64, f64, vp),
        "grail_iir_create": _sig(vp, vp, vp, u32, vp),
        "grail_iir_free": _sig(vp, vp),
        "grail_iir_async": _sig(vp, vp, vp, u64, vp, u32, vp, u32, vp, u64, vp, vp),
        "grail_biquad_blocked_async": _sig(vp, vp, vp, u64, vp, u32, vp, u32, vp, u64, vp, vp),
        "grail_biquad_block_matrix": _sig(vp, u32, vp),
        "grail_iir_stream_len": _sig(u64, u64, u32, i32, vp),
        "grail_iir_stream_open": _sig(vp, vp, u32, vp, u32, vp),
        "grail_iir_stream_next_async": _sig(vp, vp, vp, u64, vp, vp, u64, vp, vp),
        "grail_iir_stream_finish_async": _sig(vp, vp, vp, vp, u64, vp),
        "grail_iir_stream_close": _sig(vp, vp),
        "grail_dyn_design": _sig(i32, i32, f64, f64, f64, f64, f64, vp),
        "grail_dyn_ballistics": _sig(u32, f64, f64, vp),
        "grail_dyn_create": _sig(vp, vp, vp, vp, u32, vp),
        "grail_dyn_free": _sig(vp, vp),
        "grail_dyn_async": _sig(vp, vp, vp, u64, vp, u32, vp, vp, u64, vp, u32, vp, vp, u64, vp, vp, vp),
        "grail_track_dyn_async": _sig(vp, vp, vp, u64, vp, u32, vp, vp, u64, vp, u32, vp, vp, u64, vp, vp, vp),
        "grail_dyn_stream_open": _sig(vp, vp, u32, vp, u32, vp, vp),
        "grail_dyn_stream_next_async": _sig(vp, vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp),
        "grail_dyn_stream_close": _sig(vp, vp),
    }


# function name -> (restype, argtypes) of every symbol include/grail_hip.h declares; tests/test_abi.py holds each row to its
# prototype by kind and width
_SIGNATURES = _signatures()
EXPORTS = list(_SIGNATURES)

# ... and of every symbol a header declares that grail_hip.h includes (include/grail_spectrum.h: grail_hip.spectrum brings its table
# with _also_declares when it is imported, which the package does); load() sets these the same way, so there is one path
_INCLUDED_SIGNATURES = {}

_lib = None


def lib_exists():
    return os.path.exists(LIB_PATH)


def _declare(L, name):
    fn = getattr(L, name)
    fn.restype, fn.argtypes = _SIGNATURES[name] if name in _SIGNATURES else _INCLUDED_SIGNATURES[name]
    return fn


def _also_declares(table):
    """a module's own signature table joins what load() declares (on the library at once, if it is loaded already)"""
    assert not set(table) & set(_SIGNATURES)
    _INCLUDED_SIGNATURES.update(table)
    if _lib is not None:
        for name in table:
            _declare(_lib, name)


def load():
    """Load libgrail_hip.so; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GrailError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() "
                                        "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    version = _declare(L, "grail_abi_version")()         # before any other symbol is touched
    if version != ABI_VERSION:
        raise GrailError(ERR_INVALID_ARG, f"{LIB_PATH} has ABI version {version}, this binding "
                                          f"mirrors version {ABI_VERSION} of include/grail_hip.h: rebuild the library")
    for name in list(_SIGNATURES) + list(_INCLUDED_SIGNATURES):
        _declare(L, name)
    _lib = L
    return L


def _check(status):
    if status != OK:
        raise GrailError(status, load().grail_last_error().decode() or
                         load().grail_status_string(status).decode())


def _ptr(a):
    """the address of a host array (None stays None).  It is a plain number and keeps nothing alive: `a` must be a name that
    lives until the call that reads the address has returned, never an expression that makes the array."""
    return None if a is None else a.ctypes.data


def _arr(a, dtype):
    """an optional host sequence as a contiguous array of dtype; None stays None"""
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)
