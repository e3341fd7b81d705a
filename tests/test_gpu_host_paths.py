"""The host runtime behind the C ABI (rtp_host.cpp, rtp_direct_host.cpp): the
synchronous host-buffer entries against their _device siblings, every argument
check's status and rtp_last_error text, and a context that stays usable after
bad calls and after a rejected rtp_set_scene.  The Cornell box at 16 x 8,
2 spp, depth 3.

Pairs other tests already hold, not repeated here:
 - rtp_render_guides == rtp_render_guides_device bit for bit:
   test_gpu_guides.py::test_gpu_guides_repeatable_and_device_variant;
 - rtp_render_views == rtp_render_views_device (rgb bits, samples,
   live_bounces): test_gpu_views.py::test_views_aux_and_stats;
 - rtp_render_resume over the whole canvas: test_gpu_resume.py::test_host_entry_point.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from _util import assert_render_equal, same_bits_or_both_nan

pytestmark = pytest.mark.gpu

NX, NY, SPP, DEPTH = 16, 8, 2, 3
N = NX * NY
IDS = np.array([15, 16, 47, 48, 2], dtype=np.int64)  # crosses a row boundary twice, then steps back

INVALID, NO_SCENE = -1, -2


@pytest.fixture(scope="module")
def rtp():
    import raytracingtherestofyourlife_amd as m

    return m


@pytest.fixture(scope="module")
def frame(rtp, device):
    """The tiny frame every test compares against, rendered once:
    rtp_render_device with both aux arrays."""
    device.set_cornell_box(0)
    return _render_device(device, rtp.default_camera())


def _nan_pixels(rgba) -> int:
    return int(np.isnan(rgba[:, :3]).any(axis=1).sum())


def _render_device(device, cam, ids=None):
    import torch

    n = N if ids is None else ids.size
    out = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
    live = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ids = torch.from_numpy(ids).cuda() if ids is not None else None
    device.render_device(cam, NX, NY, SPP, DEPTH, out.data_ptr(), pixel_count=n,
                         pixel_ids_ptr=d_ids.data_ptr() if d_ids is not None else 0,
                         stream=torch.cuda.current_stream().cuda_stream, seed_ptr=seeds.data_ptr(),
                         live_ptr=live.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), seeds.cpu().numpy().view(np.uint32), live.cpu().numpy().view(np.uint32)


def _assert_frame(device, rtp, frame, what):
    """A good rtp_render on the context still gives the first frame's bits."""
    rgba, st = device.render(rtp.default_camera(), NX, NY, SPP, DEPTH)
    assert_render_equal((rgba, None, None), frame, what)
    assert st.samples == N * SPP


# ------------------------------------------------- host == device entries --
def test_render_equals_render_device(rtp, device, frame):
    device.set_cornell_box(0)
    rgba, st = device.render(rtp.default_camera(), NX, NY, SPP, DEPTH)
    assert_render_equal((rgba, None, None), frame, "rtp_render vs rtp_render_device")
    assert (st.samples, st.live_bounces, st.nan_pixels) == (N * SPP, int(frame[2].astype(np.uint64).sum()),
                                                            _nan_pixels(rgba))
    assert st.kernel_ms > 0


def test_render_pixels_equals_render_device(rtp, device, frame):
    device.set_cornell_box(0)
    rgba, seeds, live, st = device.render_pixels(rtp.default_camera(), NX, NY, SPP, DEPTH, IDS)
    want = _render_device(device, rtp.default_camera(), IDS)
    assert_render_equal((rgba, seeds, live), want, "rtp_render_pixels vs rtp_render_device(list)")
    assert_render_equal((rgba, seeds, live), tuple(a[IDS] for a in frame), "rtp_render_pixels vs the frame")
    assert (st.samples, st.live_bounces, st.nan_pixels) == (IDS.size * SPP, int(live.astype(np.uint64).sum()),
                                                            _nan_pixels(rgba))


def test_render_resume_equals_resume_device(rtp, device, frame):
    """One pass over a fresh state of the pixel list, all four arrays."""
    import torch

    device.set_cornell_box(0)
    cam = rtp.default_camera()
    n = IDS.size
    rgba, seed = np.zeros((n, 4), np.float32), IDS.astype(np.uint32)
    live, m2 = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    st = device.render_resume(cam, NX, NY, SPP, DEPTH, rgba, seed, live, m2, pixels=IDS)
    d = dict(rgba=torch.zeros((n, 4), dtype=torch.float32, device="cuda"),
             seed=torch.from_numpy(IDS.astype(np.uint32).view(np.int32)).cuda(),
             live=torch.zeros(n, dtype=torch.int32, device="cuda"),
             m2=torch.zeros(n, dtype=torch.float32, device="cuda"), ids=torch.from_numpy(IDS).cuda())
    st_d = device.render_resume_device(cam, NX, NY, SPP, DEPTH, d["rgba"].data_ptr(), d["seed"].data_ptr(),
                                       live_ptr=d["live"].data_ptr(), m2_ptr=d["m2"].data_ptr(), pixel_count=n,
                                       pixel_ids_ptr=d["ids"].data_ptr(), timed=True)
    torch.cuda.synchronize()
    want = (d["rgba"].cpu().numpy(), d["seed"].cpu().numpy().view(np.uint32), d["live"].cpu().numpy().view(np.uint32))
    assert_render_equal((rgba, seed, live), want, "rtp_render_resume vs rtp_render_resume_device")
    assert same_bits_or_both_nan(m2, d["m2"].cpu().numpy()).all()
    assert_render_equal((rgba, seed, live), tuple(a[IDS] for a in frame), "rtp_render_resume vs the frame")
    for s in (st, st_d):  # (the resume entries report no live bounces or NaN pixels)
        assert (s.samples, s.live_bounces, s.nan_pixels) == (n * SPP, 0, 0)


def test_render_views_stats(rtp, device, frame):
    """What test_views_aux_and_stats leaves out: nan_pixels, and the view that
    is the frame's camera against the frame."""
    device.set_cornell_box(0)
    cams = [rtp.default_camera(), rtp.hemisphere_cameras(2, 3)[4]]
    rgba, st = device.render_views(cams, NX, NY, SPP, DEPTH)
    assert_render_equal((rgba[0], None, None), frame, "rtp_render_views view 0 vs rtp_render_device")
    assert (st.samples, st.nan_pixels) == (2 * N * SPP, _nan_pixels(rgba.reshape(-1, 4)))


def test_render_guides_stats(rtp, device):
    device.set_cornell_box(0)
    *_, st = device.render_guides(rtp.default_camera(), NX, NY)
    assert (st.samples, st.live_bounces, st.nan_pixels) == (N, 0, 0) and st.kernel_ms > 0


def _direct_desc(rtp, cam, qs, cmap):
    from raytracingtherestofyourlife_amd import _lib

    d = _lib.RtpDirectDesc()
    d.clip_near, d.clip_far = float(cam.clipping[0]), float(cam.clipping[1])
    d.background[:] = [0.0, 0.0, 0.0, 1.0]
    d.composite_background = 1
    d.quad_scalar = qs.ctypes.data_as(_lib.f32p) if qs is not None else None
    d.color_map = cmap.ctypes.data_as(_lib.f32p) if cmap is not None else None
    d.color_map_size = 0 if cmap is None else cmap.shape[0]
    return d


def _direct_inputs(rtp):
    cb = rtp.CornellBox(variant=0)
    cb.buildDataSet()
    qs = rtp.direct.quad_scalars(cb.ds.GetField("point_var").values, cb.ds.GetCellSet().quad_cells)
    cmap = np.ascontiguousarray(rtp.direct.main_pallet_color_table().Sample(64), dtype=np.float32)
    return qs, cmap


def test_render_direct_equals_direct_device(rtp, device):
    import torch

    from raytracingtherestofyourlife_amd import _lib

    device.set_cornell_box(0)
    cam = rtp.default_camera()
    qs, cmap = _direct_inputs(rtp)
    host = rtp.direct.render_direct(device, cam, NX, NY, qs, cmap, aovs=7, depth=True)
    outs = {k: torch.full((N, w), 7.0, dtype=torch.float32, device="cuda")
            for k, w in (("color", 4), ("normals", 4), ("albedo", 4), ("depth", 1))}
    d, c, st = _direct_desc(rtp, cam, qs, cmap), cam.to_c(), _lib.RtpStats()
    _lib.check(device._L.rtp_render_direct_device(device.handle, ctypes.byref(c), NX, NY, ctypes.byref(d),
                                                  *[ctypes.c_void_p(outs[k].data_ptr()) for k in outs], None,
                                                  ctypes.byref(st)))
    torch.cuda.synchronize()
    for k in outs:
        assert same_bits_or_both_nan(host[k].reshape(N, -1), outs[k].cpu().numpy()).all(), k
    for s in (host["stats"], st):
        assert (s.samples, s.live_bounces, s.nan_pixels) == (N, 0, 0)


# ---------------------------------------------------------- argument errors --
def _camera(rtp, fov=None):
    cam = rtp.default_camera().to_c()
    if fov is not None:
        cam.fov_y_deg = fov
    return cam


def _check(L, rc, status, text, what):
    got = L.rtp_last_error().decode()
    assert (rc, got) == (status, text), f"{what}: status {rc}, '{got}'"


# what every entry's check_render_args refuses: (nx, ny, spp, depth, fov), status, text
RENDER_ARGS = [
    ((0, NY, SPP, DEPTH, None), INVALID, "Camera width/height must be greater than zero."),
    ((NX, -1, SPP, DEPTH, None), INVALID, "Camera width/height must be greater than zero."),
    ((65536, 65536, SPP, DEPTH, None), INVALID, "render: canvas too large"),
    ((NX, NY, SPP, DEPTH, 0.0), INVALID, "Camera feild of view must be greater than zero."),
    ((NX, NY, SPP, DEPTH, float("nan")), INVALID, "Camera feild of view must be greater than zero."),
    ((NX, NY, SPP, DEPTH, 180.5), INVALID, "Camera feild of view must be less than 180."),
    ((NX, NY, -1, DEPTH, None), INVALID, "render: samplecount must be >= 0"),
    ((NX, NY, SPP, 0, None), INVALID, "render: depthcount must be >= 1"),
    ((NX, NY, SPP, 16384, None), INVALID, "render: depthcount must be <= 16383"),
    ((NX, NY, 8388608, DEPTH, None), INVALID, "render: samplecount must be <= 8388607"),
]


def test_render_args_errors(rtp, device, frame):
    """check_render_args through rtp_render, and its NULL / no-scene answers
    through every entry that starts with it."""
    from raytracingtherestofyourlife_amd import _lib

    L = device._L
    device.set_cornell_box(0)
    out = np.full((N, 4), 7.0, np.float32)
    po = out.ctypes.data_as(_lib.f32p)
    for (nx, ny, spp, depth, fov), status, text in RENDER_ARGS:
        cam = _camera(rtp, fov)
        _check(L, L.rtp_render(device.handle, ctypes.byref(cam), nx, ny, spp, depth, 0, po, None), status, text,
               (nx, ny, spp, depth, fov))
    cam = _camera(rtp)
    _check(L, L.rtp_render(device.handle, ctypes.byref(cam), NX, NY, SPP, DEPTH, 0, None, None), INVALID,
           "rtp_render: rgba_out is NULL", "rgba_out")
    state = _lib.RtpRenderState(po, ctypes.cast(po, _lib.u32p), None, None)
    fresh = rtp.Device(device.device)
    try:
        for h, status, text in ((None, INVALID, "render: NULL argument"),
                                (fresh.handle, NO_SCENE, "render: rtp_set_scene was not called")):
            p = ctypes.byref(cam)
            calls = {
                "rtp_render": lambda: L.rtp_render(h, p, NX, NY, SPP, DEPTH, 0, po, None),
                "rtp_render_pixels": lambda: L.rtp_render_pixels(h, p, NX, NY, SPP, DEPTH, 0, None, 0, po, None, None),
                "rtp_render_device": lambda: L.rtp_render_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None, None, None,
                                                                 None, None),
                "rtp_render_planned_device": lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None,
                                                                                 None, 1, None, None, None, None),
                "rtp_render_tiles_device": lambda: L.rtp_render_tiles_device(h, p, NX, NY, SPP, DEPTH, 0, 0, 1, None,
                                                                             None, None),
                "rtp_render_resume": lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, None, N, ctypes.byref(state),
                                                                 None),
                "rtp_render_resume_device": lambda: L.rtp_render_resume_device(h, p, NX, NY, SPP, DEPTH, 0, N, None,
                                                                               ctypes.byref(state), None, None),
                "rtp_render_guides": lambda: L.rtp_render_guides(h, p, NX, NY, po, None, None, None),
                "rtp_render_guides_device": lambda: L.rtp_render_guides_device(h, p, NX, NY, None, None, None, None,
                                                                               None),
            }
            for name, call in calls.items():
                _check(L, call(), status, text, name)
        _check(L, L.rtp_render(device.handle, None, NX, NY, SPP, DEPTH, 0, po, None), INVALID, "render: NULL argument",
               "camera")
    finally:
        fresh.close()
    assert (out == 7.0).all()
    _assert_frame(device, rtp, frame, "after the check_render_args errors")


def test_entry_errors(rtp, device, frame, monkeypatch):
    """The checks each entry adds to check_render_args."""
    import torch

    from raytracingtherestofyourlife_amd import _lib

    L, h = device._L, device.handle
    device.set_cornell_box(0)
    cam = _camera(rtp)
    p = ctypes.byref(cam)
    out = np.full((N, 4), 7.0, np.float32)
    po = out.ctypes.data_as(_lib.f32p)
    d_out = torch.full((N, 4), 7.0, dtype=torch.float32, device="cuda")
    dp = ctypes.c_void_p(d_out.data_ptr())
    ids = np.array([3, N], dtype=np.int64)
    pi = ids.ctypes.data_as(_lib.i64p)
    state = _lib.RtpRenderState(po, ctypes.cast(po, _lib.u32p), None, None)
    ps = ctypes.byref(state)
    no_seed = _lib.RtpRenderState(po, None, None, None)
    plan = torch.tensor([0, 129, N], dtype=torch.int32, device="cuda")  # a wave of more than 128 entries
    dplan = ctypes.c_void_p(plan.data_ptr())
    big = 1 << 27  # (x 15 rows: a canvas within 2^31-1 pixels whose tile rows are not)
    table = [
        (lambda: L.rtp_render_pixels(h, p, NX, NY, SPP, DEPTH, 0, pi, -1, po, None, None),
         "rtp_render_pixels: bad pixel list / output"),
        (lambda: L.rtp_render_pixels(h, p, NX, NY, SPP, DEPTH, 0, None, 2, po, None, None),
         "rtp_render_pixels: bad pixel list / output"),
        (lambda: L.rtp_render_pixels(h, p, NX, NY, SPP, DEPTH, 0, pi, 2, None, None, None),
         "rtp_render_pixels: bad pixel list / output"),
        (lambda: L.rtp_render_pixels(h, p, NX, NY, SPP, DEPTH, 0, pi, 2, po, None, None),
         "rtp_render_pixels: pixel id out of range"),
        (lambda: L.rtp_render_device(h, p, NX, NY, SPP, DEPTH, 0, 0, -1, None, dp, None, None, None),
         "rtp_render_device: bad output"),
        (lambda: L.rtp_render_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None, None, None, None, None),
         "rtp_render_device: bad output"),
        (lambda: L.rtp_render_device(h, p, NX, NY, SPP, DEPTH, 0, -1, N, None, dp, None, None, None),
         "rtp_render_device: pixel range outside the canvas"),
        (lambda: L.rtp_render_device(h, p, NX, NY, SPP, DEPTH, 0, 1, N, None, dp, None, None, None),
         "rtp_render_device: pixel range outside the canvas"),
        (lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 0, 0, None, dplan, 2, dp, None, None, None),
         "rtp_render_planned_device: bad plan / output"),
        (lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None, None, 2, dp, None, None, None),
         "rtp_render_planned_device: bad plan / output"),
        (lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None, dplan, 0, dp, None, None, None),
         "rtp_render_planned_device: bad plan / output"),
        (lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None, dplan, 2, None, None, None, None),
         "rtp_render_planned_device: bad plan / output"),
        (lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 1, N, None, dplan, 2, dp, None, None, None),
         "rtp_render_planned_device: pixel range outside the canvas"),
        (lambda: L.rtp_render_planned_device(h, p, NX, NY, SPP, DEPTH, 0, 0, N, None, dplan, 2, dp, None, None, None),
         "rtp_render_planned_device: wave_begin must rise from 0 to pixel_count in steps of at most 128"),
        (lambda: L.rtp_render_tiles_device(h, p, NX, NY, SPP, DEPTH, 0, 0, 0, dp, None, None),
         "rtp_render_tiles_device: rank outside [0, world)"),
        (lambda: L.rtp_render_tiles_device(h, p, NX, NY, SPP, DEPTH, 0, 2, 2, dp, None, None),
         "rtp_render_tiles_device: rank outside [0, world)"),
        (lambda: L.rtp_render_tiles_device(h, p, big, 15, SPP, DEPTH, 0, 0, 1, dp, None, None),
         "rtp_render_tiles_device: canvas too large"),
        (lambda: L.rtp_render_tiles_device(h, p, NX, NY, SPP, DEPTH, 0, 0, 1, None, None, None),
         "rtp_render_tiles_device: bad output"),
        (lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, None, N, None, None),
         "rtp_render_resume: state, state->rgba and state->seed are required"),
        (lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, None, N, ctypes.byref(no_seed), None),
         "rtp_render_resume: state, state->rgba and state->seed are required"),
        (lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, None, N - 1, ps, None),
         "rtp_render_resume: without a pixel list pixel_count must be nx * ny"),
        (lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, pi, -1, ps, None),
         "rtp_render_resume: without a pixel list pixel_count must be nx * ny"),
        (lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, pi, 2, ps, None),
         "rtp_render_resume: pixel id out of range"),
        (lambda: L.rtp_render_resume_device(h, p, NX, NY, SPP, DEPTH, 0, N, None, None, None, None),
         "rtp_render_resume_device: state, state->rgba and state->seed are required"),
        (lambda: L.rtp_render_resume_device(h, p, NX, NY, SPP, DEPTH, 0, -1, None, ps, None, None),
         "rtp_render_resume_device: pixel_count < 0"),
        (lambda: L.rtp_render_resume_device(h, p, NX, NY, SPP, DEPTH, 1, N, None, ps, None, None),
         "rtp_render_resume_device: pixel range outside the canvas"),
        (lambda: L.rtp_render_guides(h, p, NX, NY, None, None, None, None), "render_guides: every output is NULL"),
        (lambda: L.rtp_render_guides_device(h, p, NX, NY, None, None, None, None, None),
         "render_guides: every output is NULL"),
    ]
    for k, (call, text) in enumerate(table):
        _check(L, call(), INVALID, text, f"case {k}")
    # (refused by the environment before the pixel set is looked at)
    resume = {"rtp_render_resume": lambda: L.rtp_render_resume(h, p, NX, NY, SPP, DEPTH, None, N - 1, ps, None),
              "rtp_render_resume_device": lambda: L.rtp_render_resume_device(h, p, NX, NY, SPP, DEPTH, 0, -1, None, ps,
                                                                             None, None)}
    for var in ("RTP_KERNEL", "RTP_DEBUG_STATS"):
        monkeypatch.setenv(var, "1")
        for entry, call in resume.items():
            _check(L, call(), INVALID, f"{entry}: not available with {var}=1", (var, entry))
        monkeypatch.delenv(var)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and bool((d_out == 7.0).all())
    _assert_frame(device, rtp, frame, "after the per-entry errors")


def test_views_errors(rtp, device, frame):
    from raytracingtherestofyourlife_amd import _lib

    L, h = device._L, device.handle
    device.set_cornell_box(0)
    views = (_lib.RtpView * 2)()
    for v in views:
        v.camera = _camera(rtp)
    out = np.full((2 * N, 4), 7.0, np.float32)
    po = out.ctypes.data_as(_lib.f32p)
    dv = ctypes.c_void_p(out.ctypes.data)  # (stands in for a device buffer: every call is refused before it is used)
    for args, text in (((None, 2, NX, NY, SPP, DEPTH), "render_views: NULL argument"),
                       ((views, 0, NX, NY, SPP, DEPTH), "render_views: n_views must be >= 1"),
                       ((views, 2, 32768, 32768, SPP, DEPTH),
                        "render_views: n_views * nx * ny exceeds 2^31-1 entries; render in batches")):
        _check(L, L.rtp_render_views(h, *args, po, None), INVALID, text, text)
        _check(L, L.rtp_render_views_device(h, *args, dv, None, None, None), INVALID, text, text + " (device)")
    views[1].camera.fov_y_deg = 181.0  # the second view's camera is checked like the first
    _check(L, L.rtp_render_views(h, views, 2, NX, NY, SPP, DEPTH, po, None), INVALID,
           "Camera feild of view must be less than 180.", "view 1 fov")
    views[1].camera = _camera(rtp)
    _check(L, L.rtp_render_views(h, views, 2, NX, NY, SPP, DEPTH, None, None), INVALID,
           "rtp_render_views: rgba_out is NULL", "rgba_out")
    _check(L, L.rtp_render_views_device(h, views, 2, NX, NY, SPP, DEPTH, None, None, None, None), INVALID,
           "rtp_render_views_device: bad output", "d_rgba_out")
    assert (out == 7.0).all()
    _assert_frame(device, rtp, frame, "after the render_views errors")


def test_direct_errors(rtp, device, frame):
    from raytracingtherestofyourlife_amd import _lib

    L, h = device._L, device.handle
    device.set_cornell_box(0)
    qs, cmap = _direct_inputs(rtp)
    cam = rtp.default_camera()
    out = np.full((N, 4), 7.0, np.float32)
    po = out.ctypes.data_as(_lib.f32p)

    def both(hh, c, nx, ny, d, o, status, text):
        pc = ctypes.byref(c) if c is not None else None
        pd = ctypes.byref(d) if d is not None else None
        _check(L, L.rtp_render_direct(hh, pc, nx, ny, pd, None, o, None, None, None), status, text, text)
        dev_o = ctypes.c_void_p(out.ctypes.data) if o is not None else None  # (refused before it is used)
        _check(L, L.rtp_render_direct_device(hh, pc, nx, ny, pd, None, dev_o, None, None, None, None), status, text,
               text + " (device)")

    good = _direct_desc(rtp, cam, qs, cmap)
    both(None, _camera(rtp), NX, NY, good, po, INVALID, "render_direct: NULL argument")
    both(h, None, NX, NY, good, po, INVALID, "render_direct: NULL argument")
    both(h, _camera(rtp), NX, NY, None, po, INVALID, "render_direct: NULL argument")
    fresh = rtp.Device(device.device)
    try:
        both(fresh.handle, _camera(rtp), NX, NY, good, po, NO_SCENE, "render_direct: rtp_set_scene was not called")
    finally:
        fresh.close()
    both(h, _camera(rtp), NX, 0, good, po, INVALID, "Camera width/height must be greater than zero.")
    both(h, _camera(rtp), 65536, 65536, good, po, INVALID, "render_direct: canvas too large")
    both(h, _camera(rtp, -1.0), NX, NY, good, po, INVALID, "Camera feild of view must be greater than zero.")
    both(h, _camera(rtp, 200.0), NX, NY, good, po, INVALID, "Camera feild of view must be less than 180.")
    both(h, _camera(rtp), NX, NY, good, None, INVALID, "render_direct: no output buffer")
    both(h, _camera(rtp), NX, NY, _direct_desc(rtp, cam, None, cmap), po, INVALID, "render_direct: quad_scalar is NULL")
    assert (out == 7.0).all()
    _assert_frame(device, rtp, frame, "after the render_direct errors")


# ------------------------------------------------ a rejected rtp_set_scene --
def test_rejected_set_scene_keeps_the_old_scene(rtp, device, frame):
    """A description that fails validation (a quad point id out of range) is
    refused before anything of the old scene is freed: the old scene renders
    the same bits.  (A replacement whose upload fails leaves the context
    without a scene, RTP_ERR_NO_SCENE; that path is not provoked here.)"""
    from raytracingtherestofyourlife_amd import _lib

    L = device._L
    device.set_cornell_box(0)
    d = _lib.RtpSceneDesc()
    _lib.check(L.rtp_cornell_box(0, ctypes.byref(d)))
    quad_points = np.ctypeslib.as_array(d.quad_points, shape=(4 * d.n_quads,)).copy()
    quad_points[5] = d.n_points
    d.quad_points = quad_points.ctypes.data_as(_lib.i32p)
    _check(L, L.rtp_set_scene(device.handle, ctypes.byref(d)), INVALID, "rtp_set_scene: quad point id out of range",
           "set_scene")
    _assert_frame(device, rtp, frame, "after the rejected rtp_set_scene")
