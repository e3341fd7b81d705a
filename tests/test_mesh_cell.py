"""The per-cell maths that the host and the device builder of a mesh scene
share (csrc/rtp_mesh_cell.hpp), as plain host C++: tests/cpp/mesh_cell_check.cpp,
a stand-alone program with its own main.  It holds next_up / next_down, the
ordered float key, half_outward (against the binary search the host builder
used before) and the pads and boxes of hand-made cells to values stated in the
program.  Built plain by build.build_mesh_cell_check() and under the host
AddressSanitizer + UBSan by build.build_asan(); neither touches a device, and
the sanitized one is not run where a HIP device is present."""
from __future__ import annotations

import os
import subprocess

import pytest

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "OK"
    return r


def test_mesh_cell_maths():
    from raytracingtherestofyourlife_amd import build

    assert "rtp_mesh_cell.hpp" in build.HEADERS and "rtp_lbvh.hpp" in build.HEADERS
    _run(build.build_mesh_cell_check())


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a HIP device is present: sanitized programs do not run there")
def test_mesh_cell_maths_sanitized_without_device():
    from raytracingtherestofyourlife_amd import build

    r = _run({os.path.basename(e): e for e in build.build_asan()}["mesh_cell_check"])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
