"""The table of the libraries (no GPU): _lib.LIBRARIES against the headers, the version scripts, the built files and what make would do.

Every operator library follows one convention -- csrc/tpg_<name>.hip, include/tripolar_hip_<name>.h, csrc/<name>.map,
libtripolar_hip_<name>.so, tpg_<name>_last_error, <NAME>_TAG and <NAME>_FLAGS -- and each check below runs over every one of them, so a new
library is covered the day it enters the registry.  The product keeps its own tests in test_abi.py."""
import functools
import inspect
import os
import re
import subprocess

import pytest

from orthogonalsphericalshellgrids.jl_amd import _lib
from test_abi import ROOT, declared_symbols, exported_symbols

CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
OPERATORS = [name for name in _lib.LIBRARIES if name != "product"]
BY_OPERATOR_LIBRARY = [name for name in OPERATORS if name != "operators"]      # the thirteen of the Makefile's list: no test build, a _TAG
# the constants a header defines, by value: each is checked in the C program below and against the Python constant of the same name
CONSTANTS = {
    "timestep": {"TPG_AB2_EULER": 1, "TPG_AB2_STORE_PREVIOUS": 2},
    "advection": {"TPG_ADVECTION_CENTERED2": 0},
    "momentum": {"TPG_MOMENTUM_ENSTROPHY_CONSERVING": 0},
    "hydrostatic": {"TPG_CORIOLIS_ENSTROPHY_CONSERVING": 0, "TPG_CORIOLIS_ENERGY_CONSERVING": 1, "TPG_TENDENCY_ADD": 0, "TPG_TENDENCY_WRITE": 1},
    "vertical_diffusion": {"TPG_KAPPA_CONSTANT": 0, "TPG_KAPPA_PROFILE": 1, "TPG_KAPPA_FIELD": 2,
                           "TPG_VDIFF_AUTO": 0, "TPG_VDIFF_ON_CHIP": 1, "TPG_VDIFF_STREAMED": 2},
}


def _path(name):
    return getattr(_lib, _lib.LIBRARIES[name].path_global)


@functools.lru_cache(maxsize=None)
def _exports(name):
    return tuple(exported_symbols(_path(name)))


def _map_text(name):
    return open(os.path.join(CSRC, _lib.LIBRARIES[name].map)).read()


def _make(*args):
    """the commands `make -n -B` prints for `args`: nothing runs, no compiler and no GPU is needed"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, *args], capture_output=True, text=True, check=True).stdout
    return [line for line in out.splitlines() if not line.startswith("make")]


def test_the_registry_is_every_library_once():
    assert len(_lib.LIBRARIES) == 15 and next(iter(_lib.LIBRARIES)) == "product" and len({_path(name) for name in _lib.LIBRARIES}) == 15
    assert set(CONSTANTS) <= set(OPERATORS)
    for name in OPERATORS:
        record = _lib.LIBRARIES[name]
        assert record.header == f"tripolar_hip_{name}.h" and record.map == f"{name}.map" and record.path_global == f"{name.upper()}_LIB_PATH"
        assert os.path.basename(_path(name)) == f"libtripolar_hip_{name}.so"
        assert record.signatures is getattr(_lib, f"{name.upper()}_SIGNATURES")
        assert record.load is getattr(_lib, f"{name}_lib") and record.check is getattr(_lib, f"check_{name}")


@pytest.mark.parametrize("name", OPERATORS)
def test_header_map_exports_and_signatures_are_one_list(name):
    record = _lib.LIBRARIES[name]
    record.load()
    names = sorted(record.signatures)
    assert f"tpg_{name}_last_error" in names and len(names) >= 2
    text = _map_text(name)
    assert "local: *;" in text
    assert sorted(declared_symbols(record.header)) == sorted(re.findall(r"\btpg_[a-z0-9_]+", text)) == sorted(_exports(name)) == names


@pytest.mark.parametrize("name", OPERATORS)
def test_exports_are_in_no_other_library(name):
    mine = set(_exports(name))
    for other in _lib.LIBRARIES:                                   # every other one, the product included
        if other != name:
            assert not mine & set(_exports(other)), f"{name} and {other} export one name"


@pytest.mark.parametrize("name", OPERATORS)
def test_library_reads_no_environment_variable(name):
    und = subprocess.run(["nm", "-D", "--undefined-only", _path(name)], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und


@pytest.mark.parametrize("name", OPERATORS)
def test_header_is_plain_c(name, tmp_path):
    """the header compiles as C99 with no C++ or HIP types, every function it declares is one, and its constants have the values the
    binding holds: a constant of another value is an array of negative size"""
    record = _lib.LIBRARIES[name]
    constants = CONSTANTS.get(name, {})
    src = tmp_path / "abi.c"
    src.write_text(f'#include "{record.header}"\ntypedef void (*fn)(void);\nstatic fn table[] = {{' + ", ".join(f"(fn){n}" for n in sorted(record.signatures))
                   + "};\n" + "".join(f"typedef char value_of_{c}[({c} == {v}) ? 1 : -1];\n" for c, v in constants.items())
                   + "int main(void) { return sizeof(table) == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for constant, value in constants.items():
        assert getattr(_lib, constant) == value, constant
    defined = re.findall(r"#define (TPG_[A-Z0-9_]+) ", open(os.path.join(ROOT, "include", record.header)).read())
    assert sorted(c for c in defined if not c.endswith("_H")) == sorted(constants)      # the table above misses none


@pytest.mark.parametrize("name", OPERATORS)
def test_missing_library_fails_loudly(name, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the binding raises, and names the path it looked at"""
    record = _lib.LIBRARIES[name]
    missing = str(tmp_path / os.path.basename(_path(name)))
    monkeypatch.setattr(_lib, f"_{name}", None)
    monkeypatch.setattr(_lib, record.path_global, missing)
    with pytest.raises(ImportError, match="only backend") as err:
        record.load()
    assert missing in str(err.value)


def test_the_registry_is_the_headers_and_the_maps_and_build_loads_it():
    headers = set(os.listdir(os.path.join(ROOT, "include"))) - {"tripolar_hip.h", "tripolar_hip_test.h"}
    assert headers == {_lib.LIBRARIES[name].header for name in OPERATORS}
    maps = {f for f in os.listdir(CSRC) if f.endswith(".map")} - {"exports.map", "operators_test.map"}
    assert maps == {_lib.LIBRARIES[name].map for name in OPERATORS}
    assert (_lib.LIBRARIES["product"].header, _lib.LIBRARIES["product"].map) == ("tripolar_hip.h", "exports.map")
    import __graft_entry__
    assert re.search(r"for \w+ in _lib\.LIBRARIES\.values\(\):[^\n]*\n\s+\w+\.load\(\)", inspect.getsource(__graft_entry__.build))


@pytest.mark.parametrize("name", BY_OPERATOR_LIBRARY)
def test_make_builds_a_tagged_variant_beside_the_library(name):
    """<NAME>_TAG and <NAME>_FLAGS, the interface profiles/*/README.md quote: the object and the library take the tag, the compile takes the
    flags, and nothing else is made"""
    prefix = name.upper()
    lines = _make(f"{prefix}_TAG=_t", f"{prefix}_FLAGS=-DTPG_X=1", f"../libtripolar_hip_{name}_t.so")
    compiles = [line for line in lines if f"-c tpg_{name}.hip" in line]
    assert len(compiles) == 1 and compiles[0].endswith(f"-c tpg_{name}.hip -o tpg_{name}_t.o")
    assert " -DTPG_X=1 " in compiles[0] and " -ffp-contract=off " in compiles[0] and " --offload-arch=gfx950 " in compiles[0]
    links = [line for line in lines if "-shared" in line]
    assert len(links) == 1 and f" -Wl,--version-script={name}.map " in links[0]
    assert links[0].endswith(f"-o ../libtripolar_hip_{name}_t.so.tmp tpg_api.o tpg_{name}_t.o")
    assert lines[-1] == f"mv -f ../libtripolar_hip_{name}_t.so.tmp ../libtripolar_hip_{name}_t.so" and lines.index(links[0]) == len(lines) - 2
    assert len(lines) == 4 and " -c tpg_api.hip -o tpg_api.o" in lines[0] + lines[1]      # its copy of the error channel, and nothing else


def test_make_links_every_library_of_the_registry():
    lines = _make()
    linked = sorted(line.split(" -o ")[1].split()[0] for line in lines if "--version-script=" in line)
    want = ["../libtripolar_hip.so.tmp"] + [f"../libtripolar_hip_{name}.so.tmp" for name in OPERATORS]
    assert linked == sorted(want + ["../../tools/libtripolar_hip_test.so.tmp", "../../tools/libtripolar_hip_operators_test.so.tmp"])
    for name in _lib.LIBRARIES:
        script = [line for line in lines if f"-o ../{os.path.basename(_path(name))}.tmp " in line]
        assert len(script) == 1 and f"--version-script={_lib.LIBRARIES[name].map} " in script[0]
        assert f"mv -f ../{os.path.basename(_path(name))}.tmp ../{os.path.basename(_path(name))}" in lines
