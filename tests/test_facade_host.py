"""The C++ facade (include/grail.hpp) where no device is needed, and the helpers that tests/test_facade_gpu.py shares:
tests/facade_driver.cpp is built as the Makefile's `example` target links the examples, fed raw little-endian arrays and a
small manifest, and writes every result back in the same form; all judging is done here, against the Python binding.

- the driver compiles warning-free under -Wall -Wextra -Werror with g++ and with clang++;
- group `host`: the facade's host functions give the binding's values bit for bit, detail::chunk_stride its four cases;
- without a device the device groups end with status 40 + GRAIL_ERR_NO_DEVICE and say why;
- the same `host` group once more as a stand-alone program under AddressSanitizer and UBSan;
- tests/FACADE.md names a test that exists for every public name of the header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "facade_driver.cpp")
HEADER = os.path.join(ROOT, "include", "grail.hpp")
LIBDIR = os.path.join(ROOT, "grail-rs_amd", "lib")
CLANG = "/opt/rocm/llvm/bin/clang++"
WARNINGS = ["-Wall", "-Wextra", "-Werror"]
TIMEOUT = 120
FAULT_STATUSES = (134, 139)


# ---- the driver: built, fed, run, read ----------------------------------------------------------------------------------
def build_driver(out_dir, compiler="g++", flags=("-O2",), name="facade_driver"):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call([compiler, *flags, "-std=c++17", *WARNINGS, "-I" + os.path.join(ROOT, "include"), DRIVER, "-o", exe,
                           "-L" + LIBDIR, "-lgrail_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def put(folder, name, array, dtype=None):
    a = np.ascontiguousarray(array) if dtype is None else np.ascontiguousarray(array, dtype=np.dtype(dtype).newbyteorder("<"))
    with open(os.path.join(str(folder), name), "wb") as f:
        f.write(a.tobytes())


def put_rows(folder, name, rows, dtype="f4", ext=".f32"):
    put(folder, name + ".len.u32", [len(r) for r in rows], "u4")
    put(folder, name + ext, np.concatenate([np.asarray(r, dtype) for r in rows]) if len(rows) else np.zeros(0, dtype), dtype)


def put_manifest(folder, **entries):
    with open(os.path.join(str(folder), "manifest.txt"), "w") as f:
        for key, value in entries.items():
            values = value if isinstance(value, (list, tuple)) else [value]
            f.write(key.replace("__", ".") + " " + " ".join(repr(v) if isinstance(v, float) else str(v) for v in values) + "\n")


def get(folder, name, dtype):
    with open(os.path.join(str(folder), name), "rb") as f:
        return np.frombuffer(f.read(), dtype=np.dtype(dtype).newbyteorder("<")).copy()


def get_rows(folder, name, dtype="f4", ext=".f32"):
    lens, flat = get(folder, name + ".len.u32", "u4"), get(folder, name + ext, dtype)
    assert int(lens.sum()) == len(flat), name
    ends = np.cumsum(lens)
    return [flat[int(e) - int(n):int(e)] for n, e in zip(lens, ends)]


def run_driver(exe, group, in_dir, out_dir, env=None):
    """one fresh child process -> CompletedProcess; a time limit reads as returncode None"""
    try:
        return subprocess.run([exe, group, str(in_dir), str(out_dir)], capture_output=True, text=True, timeout=TIMEOUT, env=env)
    except subprocess.TimeoutExpired as e:
        return subprocess.CompletedProcess(e.cmd, None, "", "time limit")


def bits(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b, dtype=np.float32):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a, dtype), bits(b, dtype))


# ---- group host ------------------------------------------------------------------------------------------------------------
TEXT = "aEi oui péa"
DESIGNS = [(8000, 300.0, 3400.0, 255), (48000, 0.0, 8000.0, 63), (48000, 100.0, 24000.0, 31), (16000, 50.5, 7000.25, 3)]
HOP = 256
CEILINGS_DB = [-1.0, 0.0, -0.1, -6.0206, 3.0, -120.0]
RATES = [8000.0, 44100.0, 48000.0, 22050.5]


def hop_rows():
    rng = np.random.default_rng(2024)
    rows = [np.zeros(0), rng.uniform(0.0, 3.0, 3), rng.uniform(0.0, 3.0, 4), rng.uniform(0.0, 3.0, 29), rng.uniform(0.0, 3.0, 30),
            rng.uniform(0.0, 3.0, 75) * np.repeat([1.0, 1e-3, 0.2], 25), np.full(40, 1e-9)]
    return [np.asarray(r, np.float64) for r in rows]


def write_host_inputs(folder):
    with open(os.path.join(str(folder), "text.txt"), "wb") as f:
        f.write(TEXT.encode("utf-8"))
    put_manifest(folder, fir_design=[v for d in DESIGNS for v in d], hop=HOP)
    put_rows(folder, "hops", hop_rows(), "f8", ".f64")
    put(folder, "ceiling_db.f32", CEILINGS_DB, "f4")
    put(folder, "rates.f32", RATES, "f4")


def check_host_outputs(out):
    v = G.voice_generic()
    assert get(out, "phonemes.bin", "u1").tobytes() == G.text_to_phoneme_elems(v, TEXT).tobytes()
    assert get(out, "phonemes_of_nothing.bin", "u1").tobytes() == G.text_to_phoneme_elems(v, "").tobytes()
    assert len(G.text_to_phoneme_elems(v, TEXT)) > 8
    for i, (rate, lo, hi, K) in enumerate(DESIGNS):
        assert same(get(out, f"design{i}.f32", "f4"), G.fir_design(rate, lo, hi, K)), DESIGNS[i]
    assert list(get(out, "design_origins.u32", "u4")) == [(K - 1) // 2 for *_, K in DESIGNS]
    assert same(get(out, "design_default.f32", "f4"), G.fir_design(8000, 300.0, 3400.0, 255))
    rows = hop_rows()
    got = {k: get(out, k + ".f64", "f8") for k in ("range", "window4", "window30")}
    assert same(got["range"], [G.loudness_range(h, HOP) for h in rows], np.float64)
    assert same(got["window4"], [G.loudness_window_max(h, HOP, 4) for h in rows], np.float64)
    assert same(got["window30"], [G.loudness_window_max(h, HOP, 30) for h in rows], np.float64)
    assert got["range"][5] > 1.0 and got["window30"][4] > 0 and got["window30"][3] == 0      # the cases are not all trivial
    assert same(get(out, "ceilings.f32", "f4"), [G.limit_ceiling(db) for db in CEILINGS_DB])
    at = [G.voice_generic(np.float32(r)) for r in RATES]
    assert get(out, "voices_at.bin", "u1").tobytes() == b"".join(bytes(x) for x in at)
    assert get(out, "voice_generic.bin", "u1").tobytes() == bytes(v)
    assert same(get(out, "sharpness.f32", "f4"), [np.float32(G.fast_sharpness(x)) for x in [v] + at])
    assert list(get(out, "phoneme_enum.i32", "i4")) == [G.PH_SILENCE, G.PH_STOP, G.PH_GLIDE, G.PH_A, G.PH_E]
    # no chunks (a finishing call), no rows, every chunk empty, 64, 65
    assert list(get(out, "chunk_stride.u32", "u4")) == [0, 0, 0, 64, 128]


@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("facade_driver"))


def test_the_driver_and_the_header_are_warning_free_under_both_compilers(built, tmp_path):
    for compiler in ("g++", CLANG):
        assert shutil.which(compiler), compiler
        exe = build_driver(tmp_path, compiler, name="driver_" + os.path.basename(compiler))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT)
        assert r.returncode == 2 and "usage: facade_driver GROUP IN_DIR OUT_DIR" in r.stderr


def test_host_functions_equal_the_bindings_values(driver, tmp_path):
    write_host_inputs(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    r = run_driver(driver, "host", tmp_path, out)
    assert r.returncode == 0, r.stderr
    check_host_outputs(out)


def test_a_missing_input_and_an_unknown_group_are_said(driver, tmp_path):
    r = run_driver(driver, "host", tmp_path, tmp_path)
    assert r.returncode == 3 and "manifest.txt" in r.stderr
    put_manifest(tmp_path, hop=HOP)
    r = run_driver(driver, "nothing", tmp_path, tmp_path)
    assert r.returncode == 3 and "no group nothing" in r.stderr


def test_without_a_device_the_device_groups_say_so(driver, tmp_path):
    if G.device_count() != 0:
        return                       # (with a device tests/test_facade_gpu.py runs these groups)
    put_manifest(tmp_path, hop=HOP)
    put(tmp_path, "voices.bin", np.frombuffer(bytes(G.voice_generic()), np.uint8))
    for group in ("rows", "streams", "chain"):
        r = run_driver(driver, group, tmp_path, tmp_path)
        assert r.returncode == 40 + G.ERR_NO_DEVICE, (group, r.returncode, r.stderr)
        assert "facade_driver: " + group in r.stderr and "no HIP device" in r.stderr
        assert "done" not in r.stdout


@pytest.mark.timeout(300)
def test_host_group_under_asan_ubsan(built, tmp_path):
    """The facade's host paths and the driver's own reading and writing as a stand-alone program under the sanitizers (the
    library it links is the ordinary build).  Leak detection is off: the HIP runtime that the library pulls in keeps
    allocations of its own until the process ends."""
    exe = build_driver(tmp_path, "g++", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"),
                       name="facade_driver_san")
    write_host_inputs(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = run_driver(exe, "host", tmp_path, out, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    check_host_outputs(out)


# ---- the ledger ----------------------------------------------------------------------------------------------------------------
def public_names(text):
    """{name: how many declarations} of grail.hpp: free functions as `ns::name`, classes and structs by name, their public
    methods as `Class::name` (overloads count); constructors, destructors and operators belong to the class's own line"""
    names, namespaces, cls, public = {}, [], None, True

    def add(n):
        names[n] = names.get(n, 0) + 1

    for line in text.split("\n"):
        m = re.match(r"namespace (\w+) \{", line)
        if m:
            namespaces.append(m.group(1))
            continue
        if re.match(r"\}  // namespace", line):
            namespaces.pop()
            continue
        m = re.match(r"(?:enum )?(class|struct) (\w+)\b[^;]*$", line)
        if m:
            cls, public = m.group(2), m.group(1) == "struct" or line.startswith("enum")
            add(cls)
            continue
        if line.startswith("};"):
            cls = None
            continue
        if cls and re.match(r"(public|private|protected):", line):
            public = line.startswith("public")
            continue
        m = re.match(r"    enum class (\w+)", line)
        if m and cls and public:
            add(cls + "::" + m.group(1))
            continue
        prefix = "::".join(namespaces[1:] + ([cls] if cls else []))
        decl = r"(?:inline |static |explicit )?(?:const )?[\w:]+(?:<[^()]*>)?(?: const)?[ &*]+(\w+)\("
        m = re.match(("    " if cls else "") + decl, line)
        if m and (not cls or public) and m.group(1) != cls and m.group(1) != "operator":
            add((prefix + "::" if prefix else "") + m.group(1))
    return names


def ledger_rows():
    with open(os.path.join(ROOT, "tests", "FACADE.md")) as f:
        return [line for line in f if line.startswith("|") and not re.match(r"\|\s*(-+|name)\s*\|", line)]


def test_the_header_parser_finds_what_the_header_declares():
    with open(HEADER) as f:
        names = public_names(f.read())
    for name, count in {"check": 1, "voices::generic_at": 1, "phoneme_elems": 1, "detail::chunk_stride": 1, "fir_design": 1,
                        "detail::stream_round_trip": 1, "Gpu": 1, "Gpu::fir": 1, "Gpu::set_arithmetic": 1, "LiveStream::next": 4,
                        "LimitStream::finish": 1, "LimitStream::finish_async": 1, "TrackLoudness::short_term_max": 1,
                        "Limited::refused": 1, "Stream::next": 1, "Node::rccl_ranks": 1, "FirSet::longest": 1, "Error": 1,
                        "Gpu::Arithmetic": 1, "Phoneme": 1}.items():
        assert names.get(name) == count, (name, names.get(name))
    assert not any(n.startswith("Gpu::measure_loudness") or n.startswith("Gpu::mix_leveled_with") for n in names)     # private
    assert not any(n.split("::")[-1].endswith("_") for n in names)
    assert len(names) > 90


def test_every_public_name_of_the_header_has_a_line_that_names_a_test_that_exists():
    """tests/FACADE.md: every public function, class and method of grail.hpp stands in the first column of a row (an
    overloaded name in as many rows as it has overloads), no row names what the header does not declare, and every row
    names, in its last column, test ids `file.py::name` that exist"""
    with open(HEADER) as f:
        declared = public_names(f.read())
    listed, defined = {}, {}
    for line in ledger_rows():
        cells = line.rstrip().rstrip("|").split("|")
        for name in re.findall(r"`([\w:]+)`", cells[1]):
            listed[name] = listed.get(name, 0) + 1
        ids = re.findall(r"`(test_\w+\.py)::(test_\w+)", cells[-1])
        assert ids, "a line without a test id: " + line
        for name, test in ids:
            if name not in defined:
                with open(os.path.join(ROOT, "tests", name)) as f:
                    defined[name] = set(re.findall(r"^def (test_\w+)\(", f.read(), re.M))
            assert test in defined[name], (name, test)
    missing = {n: c for n, c in declared.items() if listed.get(n, 0) < c}
    assert not missing, f"public names of grail.hpp without a line (or with fewer lines than overloads): {missing}"
    stale = sorted(set(listed) - set(declared))
    assert not stale, f"lines that name what grail.hpp does not declare: {stale}"
