"""The adaptive entry points (include/rtp_adaptive.h) under the host
AddressSanitizer + UBSan: tests/cpp/asan_adaptive.cpp, a stand-alone program
linked by build.build_asan() against the host-sanitized library sources (the
new sources are picked up from build.SOURCES).  The host helper and the
refusals that need no context; the program creates no context and is not run
where a HIP device is present."""
from __future__ import annotations

import os
import subprocess

import pytest

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def asan_adaptive():
    from raytracingtherestofyourlife_amd import build

    assert "rtp_adaptive.hip" in build.SOURCES and "rtp_adaptive_host.cpp" in build.SOURCES
    return {os.path.basename(e): e for e in build.build_asan()}["asan_adaptive"]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a HIP device is present: sanitized programs do not run there")
def test_adaptive_host_helpers_sanitized_without_device(asan_adaptive):
    r = subprocess.run([asan_adaptive], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "OK"
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
