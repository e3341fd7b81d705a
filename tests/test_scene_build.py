"""The inline scene build (csrc/rtp_scene_host.cpp: the quads with their
prefilter tables, the sphere records and their BVH, the light constants) as
plain host C++: tests/cpp/scene_build_check.cpp, a stand-alone program with its
own main over the device-free units of the library.  It holds the four Cornell
variants, the 1000-sphere one under the host build's switches, and small
hand-made descriptors to counts, messages and structure stated in the program.
Built plain by build.build_scene_build_check() -- no HIP include path, no HIP
library, every symbol resolved, so a HIP dependency in those units fails the
build -- and under the host AddressSanitizer + UBSan by build.build_asan();
neither touches a device, and the sanitized one is not run where a HIP device
is present."""
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


def test_scene_build_without_hip():
    from raytracingtherestofyourlife_amd import build

    assert set(build.DEVICE_FREE_SOURCES) <= set(build.SOURCES) and "rtp_scene_host.cpp" in build.DEVICE_FREE_SOURCES
    assert "rtp_scene.hpp" in build.HEADERS and "rtp_host_base.hpp" in build.HEADERS
    # the device-free units name no HIP header, nor the headers that do
    for unit in build.DEVICE_FREE_SOURCES + ["rtp_host_base.hpp", "rtp_scene.hpp", "rtp_mesh.hpp", "rtp_bvh_host.hpp"]:
        with open(os.path.join(build.CSRC, unit)) as f:
            includes = [line for line in f if line.lstrip().startswith("#include")]
        assert not any(h in line for line in includes
                       for h in ("hip/", "rtp_context.hpp", "rtp_host_util.hpp", "rtp_mesh_gpu.hpp")), unit
    _run(build.build_scene_build_check())


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a HIP device is present: sanitized programs do not run there")
def test_scene_build_sanitized_without_device():
    from raytracingtherestofyourlife_amd import build

    r = _run({os.path.basename(e): e for e in build.build_asan()}["scene_build_check"])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
