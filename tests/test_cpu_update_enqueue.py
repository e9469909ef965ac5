"""CPU suite for stream-ordered geometry updates (fr_update_geometry_enqueue, fr_geometry_consumed,
fr_geometry_update_status): the ABI surface, the NULL-context answers and the C++ facade, no device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

NAMES = ("fr_update_geometry_enqueue", "fr_geometry_consumed", "fr_geometry_update_status")


def test_names_are_in_the_header_and_in_the_python_mirror(fovrt_mod):
    from test_cpu_abi import header_symbols
    syms = header_symbols()
    lib = fovrt_mod.load_library()
    for name in NAMES:
        assert name in syms, name
        assert name in fovrt_mod._SIGS, name
        assert hasattr(lib, name), name
    for method in ("update_geometry_enqueue", "geometry_consumed", "geometry_update_status"):
        assert callable(getattr(fovrt_mod.PathTracer, method))


def test_null_context_is_invalid(fovrt_mod):
    lib = fovrt_mod.load_library()
    xyz = (C.c_float * 9)()
    a, r = C.c_uint64(7), C.c_uint64(7)
    assert lib.fr_update_geometry_enqueue(None, xyz, None, 1, fovrt_mod.FR_NORMALS_KEEP, None) == fovrt_mod.FR_E_INVALID
    assert lib.fr_geometry_consumed(None, None) == fovrt_mod.FR_E_INVALID
    assert lib.fr_geometry_update_status(None, C.byref(a), C.byref(r)) == fovrt_mod.FR_E_INVALID
    assert (a.value, r.value) == (7, 7)


FACADE_USER = r"""
#include "fovrt.hpp"
#include <cstdint>
// the three members exist with these signatures (never called: no device here)
using PT = fovrt::PathTracer;
void (PT::*enqueue)(const void*, const void*, size_t, int, void*) = &PT::update_geometry_enqueue;
void (PT::*consumed)(void*) = &PT::geometry_consumed;
void (PT::*status)(uint64_t*, uint64_t*) = &PT::geometry_update_status;
int main() { return enqueue && consumed && status ? 0 : 1; }
"""


def test_cpp_facade_builds_with_a_plain_host_compiler(tmp_path):
    """include/fovrt.hpp with the three new members, compiled by a host compiler that sees no HIP headers."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "user.cpp"
    src.write_text(FACADE_USER)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
