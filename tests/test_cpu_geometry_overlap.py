"""CPU suite for overlapped geometry updates (fr_set_geometry_overlap): the ABI surface, the NULL-context answer
and the C++ facade, no device."""
import os
import shutil
import subprocess

from helpers import ROOT

NAME = "fr_set_geometry_overlap"


def test_name_is_in_the_header_the_python_mirror_and_the_library(fovrt_mod):
    from test_cpu_abi import header_symbols
    assert NAME in header_symbols()
    assert NAME in fovrt_mod._SIGS
    assert hasattr(fovrt_mod.load_library(), NAME)
    assert callable(fovrt_mod.PathTracer.set_geometry_overlap)


def test_null_context_is_invalid(fovrt_mod):
    lib = fovrt_mod.load_library()
    for on in (0, 1, 2):
        assert lib.fr_set_geometry_overlap(None, on) == fovrt_mod.FR_E_INVALID


FACADE_USER = r"""
#include "fovrt.hpp"
// the member exists with this signature (never called: no device here)
using PT = fovrt::PathTracer;
void (PT::*overlap)(bool) = &PT::set_geometry_overlap;
int main() { return overlap ? 0 : 1; }
"""


def test_cpp_facade_builds_with_a_plain_host_compiler(tmp_path):
    """include/fovrt.hpp with the new member, compiled by a host compiler that sees no HIP headers."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "user.cpp"
    src.write_text(FACADE_USER)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
