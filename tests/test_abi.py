"""CPU tests of the drop-in boundary: libogg_hip.so loads without a GPU and exports every symbol include/ogg_hip.h
declares; the ctypes signature table covers the header; argument errors surface with the reference's texts.  No
compute call is made here (there is no CPU compute path to call)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ogg_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ogg_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_a_reasonable_surface():
    syms = declared_symbols()
    assert len(syms) >= 40
    for must in ("ogg_grid_metrics_midas", "ogg_grid_metrics_midas_plan", "ogg_angle_x", "ogg_bipolar_cap_metrics_quad", "ogg_displaced_pole_metrics_quad",
                 "ogg_bipolar_cap_mesh", "ogg_displaced_pole_mesh", "ogg_phi_mercator", "ogg_generate_latlon_grid"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    from ocean_model_grid_generator_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libogg_hip.so is not built: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_ctypes_table_covers_the_header():
    from ocean_model_grid_generator_amd import _lib
    table = set(_lib.SIGNATURES) | set(_lib.STRING_GETTERS) | set(_lib.LONG_GETTERS)
    assert sorted(table) == declared_symbols()
    lib = _lib.load()
    assert lib.ogg_version().startswith(b"ogg_hip")


def test_math_eval_codes_match_the_header():
    """_lib.MATH restates the OGG_MATH_* codes of ogg_math_eval_dev: the same names, the same numbers."""
    from ocean_model_grid_generator_amd import _lib
    defines = dict(re.findall(r"^#define OGG_MATH_([A-Z0-9_]+)\s+(\d+)", open(HEADER).read(), flags=re.M))
    assert len(defines) >= 20
    assert {k.lower(): int(v) for k, v in defines.items()} == _lib.MATH


def test_every_struct_has_a_size_code_and_a_mirror():
    """Every struct of the header has an OGG_ABI_* code, _lib restates the codes (the same names, the same numbers) and holds a mirror of
    each struct, and every mirror has the size the compiler gives the struct: a silent mismatch would shift every pointer behind it."""
    import numpy as np
    from ocean_model_grid_generator_amd import _lib
    text = open(HEADER).read()
    structs = set(re.findall(r"^\}\s*ogg_([a-z0-9_]+);", text, flags=re.M))
    assert len(structs) == len(re.findall(r"\btypedef struct\b", text)) >= 28
    defines = {k: int(v) for k, v in re.findall(r"^#define OGG_ABI_([A-Z0-9_]+)\s+(\d+)", text, flags=re.M)}
    n = defines.pop("N")
    assert {k.lower() for k in defines} == structs
    assert sorted(defines.values()) == list(range(n))
    assert defines == _lib.ABI and set(_lib.ABI_MIRRORS) == set(_lib.ABI)
    lib = _lib.load()
    for name, code in _lib.ABI.items():
        mirror = _lib.ABI_MIRRORS[name]
        size = mirror.itemsize if isinstance(mirror, np.dtype) else ctypes.sizeof(mirror)
        assert lib.ogg_abi_sizeof(code) == size, name
    assert lib.ogg_abi_sizeof(-1) == lib.ogg_abi_sizeof(n) == -1


def exported_symbols(path):
    """The defined dynamic symbols of a shared library that begin with ogg_, or None when no tool that lists them is installed."""
    import shutil
    import subprocess
    nm = shutil.which("nm")
    readelf = shutil.which("llvm-readelf", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        names = [line.split()[-1] for line in out.splitlines() if line.split()]
    elif readelf:
        out = subprocess.run([readelf, "--dyn-syms", "-W", path], check=True, stdout=subprocess.PIPE, text=True).stdout
        names = [f[7] for f in (line.split() for line in out.splitlines()) if len(f) == 8 and f[6] != "UND"]
    else:
        return None
    return sorted({n.split("@")[0] for n in names if n.startswith("ogg_")})


def test_library_exports_nothing_the_header_does_not_declare():
    """The other direction of test_library_exports_every_declared_symbol: an entry point that left the header has left the library."""
    from ocean_model_grid_generator_amd import _lib
    exported = exported_symbols(_lib.LIB_PATH)
    if exported is None:
        pytest.skip("neither nm nor llvm-readelf is installed")
    assert exported == declared_symbols()


def test_descriptor_structs_have_the_c_layout():
    """The ctypes mirrors of the three descriptor structs must have the size the compiler gives them (a silent mismatch would
    shift every pointer), and the pass validates its arguments before any device work."""
    from ocean_model_grid_generator_amd import _lib
    lib = _lib.load()
    assert lib.ogg_abi_sizeof(0) == ctypes.sizeof(_lib.LatlonBand)
    assert lib.ogg_abi_sizeof(1) == ctypes.sizeof(_lib.BipolarBand)
    assert lib.ogg_abi_sizeof(2) == ctypes.sizeof(_lib.DpoleBand)
    assert lib.ogg_abi_sizeof(-1) == lib.ogg_abi_sizeof(len(_lib.ABI)) == -1     # len(_lib.ABI) == OGG_ABI_N, checked below
    bands = (_lib.LatlonBand * 5)()
    rc = lib.ogg_tripolar_pass_dev(5, bands, 1441, -300.0, 360.0, 6371e3, 1, None, None)     # more than 4 lat-lon bands
    assert rc == _lib.OGG_EARG and b"at most 4 bands" in lib.ogg_last_error()
    cap = _lib.BipolarBand()
    cap.Ni, cap.Nj, cap.n_pt_rows, cap.order = 1440, 10, 4, 9
    cap.x = cap.y = cap.angle = cap.dx = cap.dy = cap.area = 8     # never dereferenced: validation comes first
    rc = lib.ogg_tripolar_pass_dev(0, bands, 1441, -300.0, 360.0, 6371e3, 1, ctypes.byref(cap), None)
    assert rc == _lib.OGG_EORDER and lib.ogg_last_error() == b"Uncoded order"
    scap = _lib.DpoleBand()
    scap.Ni, scap.Nj, scap.n_pt_rows, scap.n_cell_rows, scap.order, scap.arc_form = 1440, 10, 4, 4, 3, 0
    scap.x = scap.y = scap.angle = scap.dx = scap.dy = scap.area = scap.workspace = 8
    scap.workspace_bytes = 1 << 30
    rc = lib.ogg_supergrid_pass_dev(0, bands, 1441, -300.0, 360.0, 6371e3, 1, None, ctypes.byref(scap), None, None, None)
    assert rc == _lib.OGG_EORDER and lib.ogg_last_error() == b"order not coded"        # OGG:547
    scap.order, scap.arc_form = 4, 7
    rc = lib.ogg_supergrid_pass_dev(0, bands, 1441, -300.0, 360.0, 6371e3, 1, None, ctypes.byref(scap), None, None, None)
    assert rc == _lib.OGG_EARG and b"arc_form" in lib.ogg_last_error()


def test_argument_errors_use_reference_texts():
    """Validation happens before any device work, so these run without a GPU."""
    from ocean_model_grid_generator_amd import _lib
    lib = _lib.load()
    rc = lib.ogg_bipolar_cap_metrics_quad(7, 48, 10, 64.0, -300.0, 0.2, 6371e3, None, None, None)
    assert rc == _lib.OGG_EORDER and lib.ogg_last_error() == b"Uncoded order"          # OGG:204
    rc = lib.ogg_displaced_pole_metrics_quad(3, 72, 14, -300.0, -78.0, 80.0, 0.2, 6371e3, None, None, None)
    assert rc == _lib.OGG_EORDER and lib.ogg_last_error() == b"order not coded"        # OGG:547
    with pytest.raises(Exception, match="Uncoded order"):
        _lib.check(lib.ogg_bipolar_cap_metrics_quad(1, 48, 10, 64.0, -300.0, 0.2, 6371e3, None, None, None))


def test_no_cpu_fallback_in_product_package():
    """The product package must not import the oracle (or anything under oracle/)."""
    pkg = os.path.join(ROOT, "ocean_model_grid_generator_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "ogg_oracle" not in src, f
