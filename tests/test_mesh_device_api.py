"""rtp_set_scene_mesh_device through the layers that need no GPU: the binding's
signature table, the public header, the library's exports and the Device
method with its argument checks' place (before any call into the library)."""
from __future__ import annotations

import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_table():
    from raytracingtherestofyourlife_amd import _lib

    assert _lib.SIGNATURES["include/rtp_mesh.h"]["rtp_set_scene_mesh_device"] == (
        ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(_lib.RtpSceneDesc), ctypes.c_void_p])
    assert "rtp_set_scene_mesh_device" not in _lib.SIGNATURES["include/rtp.h"]
    assert "rtp_set_scene_mesh_device" not in _lib.EXPORTED_SYMBOLS


def test_prototype_in_the_public_header():
    with open(os.path.join(ROOT, "include", "rtp_mesh.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("rtp_status rtp_set_scene_mesh_device(rtp_context* ctx, const rtp_scene_desc* scene, void* hip_stream);"
            in text)
    with open(os.path.join(ROOT, "include", "rtp.h")) as f:
        assert "rtp_set_scene_mesh_device" not in f.read()


def test_symbols_exported():
    from raytracingtherestofyourlife_amd import _lib, build

    L = ctypes.CDLL(build.build())
    for name in ("rtp_set_scene_mesh_device", "rtp_debug_mesh_readback", "rtp_set_scene_mesh", "rtp_mesh_build_host"):
        assert hasattr(L, name), name
    assert set(_lib.SIGNATURES["include/rtp_mesh.h"]) == {"rtp_set_scene_mesh", "rtp_mesh_guarantee", "rtp_mesh_counts",
                                                          "rtp_set_scene_mesh_device"}


def test_device_method():
    from raytracingtherestofyourlife_amd import Device

    host = list(inspect.signature(Device.set_scene_mesh).parameters)
    dev = list(inspect.signature(Device.set_scene_mesh_device).parameters)
    assert dev == host + ["stream"]
    assert inspect.signature(Device.set_scene_mesh_device).parameters["stream"].default is None
