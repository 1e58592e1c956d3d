"""The sixteen launchers of the row transforms (limiter, resampler, FIR, meter streams) hand their kernels the fields of one
argument struct (csrc/kernels.h: LimitArgs, ResampleArgs, FirArgs, MeterStreamArgs).  Most of those fields are pointers and
integers of the same few types, so a launcher that passed `a.out_len` where the kernel takes `cbad` would compile; here the
sequence of fields a launcher passes is held to the parameter names of the kernel it launches, in order, from the text of
the four units.  Read from the sources only: no library, no device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grail-rs_amd", "csrc")

# unit -> its launchers -> the struct each takes (None: launch_meter_stream_read keeps a parameter list of its own)
LAUNCHERS = {
    "limiter_kernels.hip": {"launch_limit_frames": "LimitArgs", "launch_limit_totals": "LimitArgs",
                            "launch_limit_stream": "LimitArgs", "launch_limit_stream_advance": "LimitArgs"},
    "resample_kernels.hip": {"launch_resample": "ResampleArgs", "launch_resample_totals": "ResampleArgs",
                             "launch_resample_stream": "ResampleArgs", "launch_resample_stream_advance": "ResampleArgs"},
    "fir_kernels.hip": {"launch_fir": "FirArgs", "launch_fir_totals": "FirArgs", "launch_fir_stream": "FirArgs",
                        "launch_fir_stream_advance": "FirArgs"},
    "meter_stream_kernels.hip": {"launch_meter_stream_hops": "MeterStreamArgs", "launch_meter_stream_peak": "MeterStreamArgs",
                                 "launch_meter_stream_advance": "MeterStreamArgs", "launch_meter_stream_read": None},
}

# a kernel's parameter -> the struct's field, where the two names differ: a stream's kernels call the rows the call feeds `in`,
# the meter's kernels write the hop H, the resampler's the ratio U / D and the taps a phase P
ALIAS = {"in": "rows", "in_stride": "row_stride", "in_len": "len", "H": "hop", "U": "up", "D": "down", "P": "taps"}


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def balanced(text, at):
    """text[at] is '(' or '{': what stands between it and its partner"""
    pair = {"(": ")", "{": "}"}[text[at]]
    depth = 0
    for i in range(at, len(text)):
        depth += (text[i] == text[at]) - (text[i] == pair)
        if depth == 0:
            return text[at + 1:i]
    raise AssertionError("unbalanced at %d" % at)


def split_args(text):
    """the arguments of a call or the parameters of a function: split at the commas outside every parenthesis"""
    parts, depth, cur = [], 0, ""
    for ch in text:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


def kernel_parameters(text, kernel):
    m = re.search(r"__global__[^;{]*?\bvoid " + kernel + r"\(", text)
    assert m, kernel
    params = split_args(balanced(text, m.end() - 1))
    return [re.search(r"(\w+)$", p).group(1) for p in params]


def struct_fields(header, struct):
    """the names of a struct's fields, its base's first"""
    m = re.search(r"struct " + struct + r"(?: : (\w+))? \{", header)
    assert m, struct
    body = re.sub(r"//[^\n]*", "", balanced(header, m.end() - 1))
    fields = struct_fields(header, m.group(1)) if m.group(1) else []
    for decl in body.split(";"):
        fields += re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
    return fields


def launches(text, launcher):
    """(the launcher's parameters, the locals it declares, the kernel it launches, the arguments it gives the kernel)"""
    m = re.search(r"^hipError_t " + launcher + r"\(", text, re.M)
    assert m, launcher
    params = balanced(text, m.end() - 1)
    body = balanced(text, text.index("{", m.end() + len(params)))
    found = [c for c in re.finditer(r"\b(hipLaunchKernelGGL|launch_either)\(", body)]
    assert len(found) == 1, (launcher, "one launch a launcher")
    call = split_args(balanced(body, found[0].end() - 1))
    # both forms end `..., grid, block, lds, stream, <the kernel's arguments>`; the kernel stands before the grid
    at = call.index("stream")
    named = sorted(set(re.findall(r"\b(\w+_kernel)\b", ", ".join(call[:at]))))
    if not named:       # the resampler: a function picks the instantiation; it names one kernel template
        pickers = sorted(set(re.findall(r"\b(\w+_variant)\b", ", ".join(call[:at]))))
        assert len(pickers) == 1, (launcher, pickers)
        picker = re.search(r"\bauto " + pickers[0] + r"\(int tab\)\s*\{", text)
        named = sorted(set(re.findall(r"\b(\w+_kernel)\b", balanced(text, picker.end() - 1))))
    assert len(named) == 1, (launcher, named)
    local = re.findall(r"^\s*(?:const )?\w+ (\w+)(?: = [^;]*)?;", body, re.M)
    return params, local, named[0], call[at + 1:]


def passed_name(arg, struct_field_names, own_names, launcher):
    """the name an argument stands for: `a.name` a field of the struct, a bare name one the launcher itself declares; casts
    and the bool-to-word `? 1u : 0u` set aside"""
    arg = re.sub(r"^\((?:const )?\w+(?: \*)?\)", "", arg)
    arg = re.sub(r" \? 1u : 0u$", "", arg)
    m = re.fullmatch(r"a\.(\w+)", arg)
    if m:
        assert m.group(1) in struct_field_names, (launcher, arg, "no such field")
        return m.group(1)
    assert re.fullmatch(r"\w+", arg) and arg in own_names, (launcher, arg, "neither a field nor the launcher's own")
    return arg


def test_every_launcher_passes_the_fields_its_kernels_parameters_name():
    header = source("kernels.h")
    checked = []
    for unit, launchers in LAUNCHERS.items():
        text = source(unit)
        # the unit holds these launchers and no other
        assert sorted(re.findall(r"^hipError_t (launch_\w+)\(", text, re.M)) == sorted(launchers), unit
        for launcher, struct in launchers.items():
            params, local, kernel, args = launches(text, launcher)
            if struct:
                assert re.sub(r"\s+", " ", params) == "const %s &a, hipStream_t stream" % struct, (launcher, params)
                assert re.search(r"^hipError_t %s\(const %s &a, hipStream_t stream\);" % (launcher, struct), header, re.M), launcher
                fields, own = struct_fields(header, struct), local
            else:
                fields, own = [], [re.search(r"(\w+)$", p).group(1) for p in split_args(params)]
            passed = [passed_name(arg, fields, own, launcher) for arg in args]
            wanted = [ALIAS.get(p, p) for p in kernel_parameters(text, kernel)]
            assert passed == wanted, (launcher, kernel, passed, wanted)
            checked.append(launcher)
    assert len(checked) == len(set(checked)) == 16, checked


def test_the_reader_sees_a_swapped_pair():
    """the check above on a launcher's text with two of its fields exchanged: it must not pass"""
    header, text = source("kernels.h"), source("fir_kernels.hip")
    _, _, kernel, args = launches(text, "launch_fir_stream_advance")
    assert "a.cbad" in args and "a.out_len" in args
    swapped = text.replace("a.cbad, a.grid_chunks, a.out_len, a.nonfinite);", "a.out_len, a.grid_chunks, a.cbad, a.nonfinite);")
    assert swapped != text
    _, local, kernel, args = launches(swapped, "launch_fir_stream_advance")
    fields = struct_fields(header, "FirArgs")
    passed = [passed_name(arg, fields, local, "launch_fir_stream_advance") for arg in args]
    assert sorted(passed) == sorted(ALIAS.get(p, p) for p in kernel_parameters(text, kernel))
    assert passed != [ALIAS.get(p, p) for p in kernel_parameters(text, kernel)]


def test_the_structs_state_the_stream_fields_once():
    header = source("kernels.h")
    base = struct_fields(header, "RowCallArgs")
    assert base == ["rows", "row_stride", "len", "state", "ring", "ring_cap", "mark", "finishing"]
    for struct in ("LimitArgs", "ResampleArgs", "FirArgs", "MeterStreamArgs"):
        fields = struct_fields(header, struct)
        assert fields[:len(base)] == base and len(fields) == len(set(fields)), struct
