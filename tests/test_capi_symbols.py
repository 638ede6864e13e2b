"""CPU-side check of the drop-in boundary: the C-ABI library builds, loads and exports every function declared in
include/srsgpu_phy.h (no compute call: there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "srsgpu_phy.h")
LIB = os.path.join(ROOT, "srsran-5g_amd", "lib", "libsrsgpu_phy.so")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srsgpu_[a-z0-9_]+)\s*\(", text)))


def header_prototypes():
    """name -> (return type, number of parameters) of every function the header declares. Its prototypes hold no nested
    parentheses and no function pointers, so the parameters are the top-level commas plus one, `void` being none."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(srsgpu_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), 0 if params == "void" else params.count(",") + 1)
    return out


# The ctypes restype of every return type the header uses (None is void).
RESTYPES = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64}


def test_header_declares_api():
    fns = declared_functions()
    assert "srsgpu_ldpc_decode" in fns and "srsgpu_context_create" in fns
    assert sorted(header_prototypes()) == fns


def test_public_names_of_the_package_are_kept():
    """Every public name the package had before it was split into one module per channel (tests/golden/
    srsgpu_public_names.txt, written from the single-file package) is still an attribute of `srsgpu`."""
    import srsgpu
    names = open(os.path.join(ROOT, "tests", "golden", "srsgpu_public_names.txt")).read().split()
    assert len(names) == 166
    missing = [n for n in names if not hasattr(srsgpu, n)]
    assert not missing, missing
    assert callable(srsgpu._dptr)


def test_prototype_table_matches_header():
    """srsgpu._abi.PROTOTYPES against include/srsgpu_phy.h, function by function: the same names, as many argtypes as
    the declaration has parameters, and the restype of the declared return type (None exactly for void)."""
    from srsgpu import _abi
    header = header_prototypes()
    assert len(header) == 106
    assert set(_abi.PROTOTYPES) == set(declared_functions()) == set(header)
    assert _abi.EXPORTED_SYMBOLS == sorted(_abi.PROTOTYPES)
    assert not set(_abi.DEBUG_PROTOTYPES) & set(header)
    for name, (ret, nof_params) in header.items():
        restype, argtypes = _abi.PROTOTYPES[name][:2]
        assert len(argtypes) == nof_params, name
        assert (restype is None) == (ret == "void"), name
        assert restype is RESTYPES[ret], (name, ret, restype)
    for row in list(_abi.PROTOTYPES.values()) + list(_abi.DEBUG_PROTOTYPES.values()):
        assert len(row) == 2 or row[2:] == (_abi.OPTIONAL,), row


def test_device_memory_is_owned_by_device_buffer_only():
    """The host layer allocates and frees device memory in one place, srsgpu::device_buffer (capi_internal.h): a plan
    that calls hipMalloc / hipFree itself escapes the live-buffer count and the lifetime tests."""
    csrc = os.path.join(ROOT, "srsran-5g_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".cpp", ".h")))
    assert "capi_internal.h" in files and "capi.cpp" in files
    users = [f for f in files
             if any(call in open(os.path.join(csrc, f)).read() for call in ("hipMalloc(", "hipFree("))]
    assert users == ["capi_internal.h"], users


@pytest.mark.skipif(not os.path.exists(LIB), reason="libsrsgpu_phy.so not built")
def test_library_exports_every_declared_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    missing = [f for f in declared_functions() if f not in exported]
    assert not missing, missing
    import torch  # noqa: F401  (share torch's HIP runtime, as the product binding does)
    lib = ctypes.CDLL(LIB)
    for f in declared_functions():
        assert hasattr(lib, f)
    assert lib.srsgpu_version() >= 100


@pytest.mark.skipif(not os.path.exists(LIB), reason="libsrsgpu_phy.so not built")
def test_python_binding_lists_header_symbols():
    import srsgpu
    assert sorted(srsgpu.EXPORTED_SYMBOLS) == declared_functions()


@pytest.mark.skipif(not os.path.exists(LIB), reason="libsrsgpu_phy.so not built")
def test_loaded_library_is_typed_by_the_table():
    """load_library() types every function of the table: the library exports every row that is not marked optional, and
    each carries the row's argtypes and restype (an untyped function would pass a device pointer as a C int)."""
    from srsgpu import _abi
    lib = _abi.load_library()
    for name, row in {**_abi.PROTOTYPES, **_abi.DEBUG_PROTOTYPES}.items():
        if not hasattr(lib, name):
            assert _abi.OPTIONAL in row[2:], name
            continue
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(row[1]), name
        assert fn.restype is row[0], name
    for name in _abi.PROTOTYPES:
        assert hasattr(lib, name), name


def test_missing_required_symbol_is_named(monkeypatch):
    """A library without a required function is refused with the function's name; the interpreter's own _ctypes
    extension stands in for such a build."""
    import _ctypes
    from srsgpu import _abi
    monkeypatch.setattr(_abi, "_loaded", None)
    with pytest.raises(_abi.SrsGpuError, match="srsgpu_version"):
        _abi.load_library(_ctypes.__file__)
    assert _abi._loaded is None


@pytest.mark.skipif(not os.path.exists(LIB), reason="libsrsgpu_phy.so not built")
def test_no_device_fails_loudly():
    import torch
    import srsgpu
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(srsgpu.SrsGpuError):
        srsgpu.Context(0)
