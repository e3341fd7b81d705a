"""The device-free mesh BVH builder (csrc/rtp_mesh_host.cpp) under the host
AddressSanitizer + UBSan: tests/cpp/asan_mesh.cpp, a stand-alone program
linked by build.build_asan() against the host-sanitized library sources.  It
builds a tess-sized and a 65 536-quad scene generated in the program, creates
no context, and is not run where a HIP device is present."""
from __future__ import annotations

import os
import subprocess

import pytest

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def asan_mesh():
    from raytracingtherestofyourlife_amd import build

    assert "rtp_mesh_host.cpp" in build.SOURCES
    return {os.path.basename(e): e for e in build.build_asan()}["asan_mesh"]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a HIP device is present: sanitized programs do not run there")
def test_mesh_builder_sanitized_without_device(asan_mesh):
    r = subprocess.run([asan_mesh], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "OK"
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
