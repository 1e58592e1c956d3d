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

The package by subject, every name of which is reachable as grail_hip.NAME:
  _abi    the header's constants and structures, the signature table behind EXPORTS, load()
  host    the pure-host calls (parameter algebra, text front half, planning, the arithmetic around measurements)
  device  Context, Batch, the streams, Node, and the one waited-for form
The star imports below have no __all__ on purpose: every public name of the three, the modules C, np and os among them,
was an attribute of this module before the split.  grail_hip.host and grail_hip.device are new attributes, the submodules.
load() reads LIB_PATH and keeps the loaded library in _abi: grail_hip.LIB_PATH is a copy and grail_hip._lib a read-only
view, so assigning to either here does not reach load() (assign to grail_hip._abi's).
"""
from . import _abi
from ._abi import *                                                         # noqa: F401,F403
from ._abi import _HERE, _arr, _check, _ptr                                 # noqa: F401
from .host import *                                                         # noqa: F401,F403
from .host import _mix_items                                                # noqa: F401
from .device import *                                                       # noqa: F401,F403
from .device import _BorrowedContext, _coef10, _marks, _per, _waited        # noqa: F401
# include/grail_spectrum.h (short-time spectra) is the submodule grail_hip.spectrum and adds no name here: see its docstring
from . import spectrum                                                      # noqa: F401


def __getattr__(name):
    if name == "_lib":                   # the library load() has loaded, or None: it lives where load() sets it
        return _abi._lib
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
