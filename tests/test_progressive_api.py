"""The resumable render's interface without a device: the C ABI additions
(rtp_render_resume*, rtp_render_state), the noise estimate and the refine
selection as pure functions, the checkpoint file and the pass-size split (the
same in Python and in rtp_path -passes N -dry-run)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ ABI --
def test_library_exports_resume_symbols():
    import raytracingtherestofyourlife_amd as rtp
    from raytracingtherestofyourlife_amd import _lib

    L = ctypes.CDLL(rtp.LIB_PATH)
    for name in ("rtp_render_resume_device", "rtp_render_resume"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert not _lib.bind(L)
    assert L.rtp_abi_version() == 3


def test_render_state_layout_matches_the_header(tmp_path):
    """rtp_render_state and every other struct of include/rtp.h that _lib.py
    mirrors: size, and each field's name and offset in declaration order."""
    from raytracingtherestofyourlife_amd import _lib
    from raytracingtherestofyourlife_amd._lib import RtpRenderState

    exe = str(tmp_path / "state_layout_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "state_layout_check.cpp"), "-o", exe], check=True,
                   capture_output=True)
    mirrors = dict(rtp_camera=_lib.RtpCamera, rtp_view=_lib.RtpView, rtp_scene_desc=_lib.RtpSceneDesc,
                   rtp_stats=_lib.RtpStats, rtp_pixel_aux=_lib.RtpPixelAux, rtp_render_state=RtpRenderState,
                   rtp_direct_desc=_lib.RtpDirectDesc, rtp_denoise_params=_lib.RtpDenoiseParams,
                   rtp_ff_info=_lib.RtpFfInfo)
    seen = []
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        if not line:
            continue
        name, size, *fields = line.split()
        mirror = mirrors[name]
        assert ctypes.sizeof(mirror) == int(size), name
        assert [f"{f}={getattr(mirror, f).offset}" for f, _ in mirror._fields_] == fields, name
        seen.append(name)
    assert seen == list(mirrors)
    assert [f for f, _ in RtpRenderState._fields_] == ["rgba", "seed", "live_bounces", "m2"]


# ---------------------------------------------------------------- noise --
LUMA = np.array([0.2126, 0.7152, 0.0722])


def _state_of(samples):
    """Sums, m2 and count of one pixel from its samples' rgb (float32
    accumulation in sample order, m2 with the contract's operation order)."""
    f = np.float32
    sums, m2 = np.zeros(4, dtype=np.float32), f(0)
    for c in np.asarray(samples, dtype=np.float32):
        sums[:3] = sums[:3] + c
        y = f(f(f(f(0.2126) * c[0]) + f(f(0.7152) * c[1])) + f(f(0.0722) * c[2]))
        m2 = f(m2 + f(y * y))
    return sums, m2, len(samples)


def _stack(pixels):
    return (np.stack([p[0] for p in pixels]), np.array([p[1] for p in pixels], dtype=np.float32),
            np.array([p[2] for p in pixels], dtype=np.int32))


def test_noise_constant_two_value_and_nan():
    from raytracingtherestofyourlife_amd.progressive import noise_from_state, select_active, state_finite

    a, b = (0.5, 0.25, 1.0), (1.5, 0.25, 0.0)
    pixels = [
        _state_of([(0.3, 0.6, 0.9)] * 8),          # constant luminance
        _state_of([(0.0, 0.0, 0.0)] * 4),          # black
        _state_of([a, b]),                         # two values
        _state_of([a, b] * 8),                     # the same two values, 16 samples
        _state_of([(np.nan, 0.1, 0.1), a, b]),     # a NaN sample poisons sums and m2
        _state_of([a]),                            # one sample: no estimate yet
    ]
    sums, m2, count = _stack(pixels)
    noise = noise_from_state(sums, m2, count)
    assert noise.shape == (6,) and noise.dtype == np.float64
    assert noise[0] == 0.0 and noise[1] == 0.0
    ya, yb = float(LUMA @ a), float(LUMA @ b)
    # n = 2: mean (ya+yb)/2, s2 = (ya-yb)^2 / 2, sem = |ya-yb| / 2  ->  |ya-yb| / (ya+yb)
    assert noise[2] == pytest.approx(abs(ya - yb) / (ya + yb), rel=1e-5)
    # n = 16, half a half b: s2 = (16/15) (ya-yb)^2 / 4, sem = sqrt(s2 / 16)
    assert noise[3] == pytest.approx(np.sqrt((16 / 15) * (ya - yb) ** 2 / 4 / 16) / ((ya + yb) / 2), rel=1e-5)
    assert np.isnan(m2[4]) and np.isinf(noise[4]) and np.isinf(noise[5])
    finite = state_finite(sums, m2)
    assert finite.tolist() == [True, True, True, True, False, True]
    # the NaN pixel is never active, whatever the threshold
    for thr in (0.0, 1e30):
        assert 4 not in select_active(noise, count, 4, thr, 10 ** 6, finite=finite).tolist()
    assert 5 in select_active(noise, count, 4, 0.5, 10 ** 6, finite=finite).tolist()


def test_noise_rejects_mismatched_shapes():
    from raytracingtherestofyourlife_amd import ErrorBadValue
    from raytracingtherestofyourlife_amd.progressive import noise_from_state

    with pytest.raises(ErrorBadValue):
        noise_from_state(np.zeros((4, 4), np.float32), np.zeros(3, np.float32), np.zeros(4, np.int32))


def test_refine_selection_rule():
    from raytracingtherestofyourlife_amd.progressive import select_active

    noise = np.array([0.5, 0.05, 0.2, np.inf, 0.2, np.nan, 0.1])
    count = np.array([4, 4, 12, 4, 13, 4, 4])
    got = select_active(noise, count, spp=4, threshold=0.1, max_spp=16)
    # 0: noisy; 1: clean; 2: 12 + 4 <= 16; 3: inf noise without a mask counts as noisy;
    # 4: 13 + 4 > 16; 5: NaN compares false; 6: not above the threshold
    assert got.dtype == np.int64 and got.tolist() == [0, 2, 3]
    finite = np.array([True, True, True, False, True, True, True])
    assert select_active(noise, count, 4, 0.1, 16, finite=finite).tolist() == [0, 2]
    assert select_active(noise, count, 4, 0.1, 7).size == 0


# ----------------------------------------------------------- checkpoint --
def _fake_state(n, rng):
    return dict(sums=rng.random((n, 4), dtype=np.float32), seed=rng.integers(0, 2 ** 32, n, dtype=np.uint32),
                live=rng.integers(0, 1000, n, dtype=np.uint32), m2=rng.random(n, dtype=np.float32),
                count=rng.integers(0, 50, n).astype(np.int32))


def test_checkpoint_round_trip_and_wrong_shape(tmp_path):
    import raytracingtherestofyourlife_amd as rtp
    from raytracingtherestofyourlife_amd.progressive import checkpoint_arrays, read_checkpoint

    nx, ny = 7, 5
    state = _fake_state(nx * ny, np.random.default_rng(3))
    state["sums"][3, 1] = np.nan
    cam = rtp.default_camera()
    cam.SetPosition([0.9, 0.7, -1.1])
    cam.SetFieldOfView(52.0)
    path = str(tmp_path / "ck.npz")
    np.savez(path, **checkpoint_arrays(state, cam, nx, ny, 9, 0xFFFFFFF0))
    ck = read_checkpoint(path)
    for k, v in state.items():
        assert ck[k].dtype == v.dtype and ck[k].tobytes() == v.tobytes(), k
    assert (ck["nx"], ck["ny"], ck["depth"], ck["seed_base"]) == (nx, ny, 9, 0xFFFFFFF0)
    assert np.array_equal(ck["cam_position"], cam.position) and np.array_equal(ck["cam_look_at"], cam.look_at)
    assert np.array_equal(ck["cam_view_up"], cam.view_up) and ck["cam_fov"] == 52.0
    # a state of another canvas size, a wrong dtype and a missing array are rejected
    bad = checkpoint_arrays(state, cam, nx, ny, 9, 0)
    for name, change in (("shape", dict(m2=bad["m2"][:-1])), ("sums", dict(sums=bad["sums"][:, :3])),
                         ("dtype", dict(seed=bad["seed"].astype(np.int64))), ("size", dict(nx=np.int32(nx + 1)))):
        p = str(tmp_path / f"bad_{name}.npz")
        np.savez(p, **{**bad, **change})
        with pytest.raises(rtp.ErrorBadValue):
            read_checkpoint(p)
    p = str(tmp_path / "bad_missing.npz")
    np.savez(p, **{k: v for k, v in bad.items() if k != "live"})
    with pytest.raises(rtp.ErrorBadValue):
        read_checkpoint(p)


# ------------------------------------------------------------ pass split --
@pytest.fixture(scope="module")
def rtp_path():
    from raytracingtherestofyourlife_amd import build

    return {os.path.basename(e): e for e in build.build_cpp()}["rtp_path"]


@pytest.mark.parametrize("total,passes,want", [(10, 3, [4, 3, 3]), (9, 4, [3, 2, 2, 2]), (7, 7, [1] * 7),
                                               (2, 5, [1, 1, 0, 0, 0]), (12, 1, [12]), (0, 2, [0, 0])])
def test_pass_split_python_and_driver(rtp_path, total, passes, want):
    from raytracingtherestofyourlife_amd import split_passes

    assert split_passes(total, passes) == want
    r = subprocess.run([rtp_path, "-samplecount", str(total), "-passes", str(passes), "-dry-run"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == want


def test_pass_split_rejects_bad_counts(rtp_path):
    from raytracingtherestofyourlife_amd import ErrorBadValue, split_passes

    with pytest.raises(ErrorBadValue):
        split_passes(10, 0)
    for args in (["-passes", "0"], ["-passes", "-3"], ["-passes", "2", "-hemisphere"], ["-passes", "2", "-direct"],
                 ["-passes", "0", "-dry-run"]):
        r = subprocess.run([rtp_path, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "-passes" in r.stderr
