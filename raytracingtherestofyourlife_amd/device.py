"""Device: the ctypes wrapper of one rtp_context (include/rtp.h).

Every method is one entry point of the C ABI: its argument checks, its output
buffers and its argument order.  The marshalling they share is _lib's
(signatures, pointer conversions) and Device._call (status and stats).
"""
from __future__ import annotations

import ctypes
from typing import TYPE_CHECKING

import numpy as np

from . import _lib
from ._lib import ErrorBadValue, RtpFfInfo, RtpSceneDesc, RtpStats, RtpView, check, pixel_aux, ptr, render_state
from .mesh import cell_rows

if TYPE_CHECKING:
    from .mapper import Camera


def scene_desc(coords, quad_points, quad_mat, quad_tex, sphere_points, sphere_radius, sphere_mat, sphere_tex,
               mat_type, tex_type, tex, light_quad_points=(8, 9, 10, 11), light_sphere_point=48, ior=1.5):
    """The rtp_scene_desc of a scene in the reference's arrays (no device
    needed): (desc, arrays).  The desc points into the arrays, converted to
    the ABI's types; keep them for as long as the desc is used."""
    i32, f32 = np.int32, np.float32
    flat = lambda a, dt: np.ascontiguousarray(a, dtype=dt).reshape(-1)
    arrs = dict(
        points=flat(coords, f32),
        quad_points=flat(quad_points, i32),
        quad_mat=np.ascontiguousarray(quad_mat, dtype=i32),
        quad_tex=np.ascontiguousarray(quad_tex, dtype=i32),
        sphere_point=np.ascontiguousarray(sphere_points, dtype=i32),
        sphere_radius=np.ascontiguousarray(sphere_radius, dtype=f32),
        sphere_mat=np.ascontiguousarray(sphere_mat, dtype=i32),
        sphere_tex=np.ascontiguousarray(sphere_tex, dtype=i32),
        mat_type=np.ascontiguousarray(mat_type, dtype=i32),
        tex_type=np.ascontiguousarray(tex_type, dtype=i32),
        tex_rgb=flat(tex, f32),
    )
    d = RtpSceneDesc()
    for name, a in arrs.items():
        setattr(d, name, ptr(a))
    d.n_points = arrs["points"].size // 3
    d.n_quads = arrs["quad_mat"].size
    d.n_spheres = arrs["sphere_point"].size
    d.n_mat = arrs["mat_type"].size
    d.n_tex_type = arrs["tex_type"].size
    d.n_tex = arrs["tex_rgb"].size // 3
    d.light_quad_points[:] = [int(v) for v in light_quad_points]
    d.light_sphere_point = int(light_sphere_point)
    d.ior = float(ior)
    return d, arrs


def mesh_scene_desc(coords, quad_points, *rest, **kw):
    """scene_desc for a mesh scene (rtp_set_scene_mesh): quad_points may also
    be [N, 3], triangle cells -- a row (a, b, c) becomes (a, b, c, c)
    (include/rtp_mesh.h)."""
    return scene_desc(coords, cell_rows(quad_points), *rest, **kw)


class Device:
    """One rtp_context (one HIP device)."""

    def __init__(self, device: int = 0, lib: ctypes.CDLL | None = None):
        """``lib``: a librtp loaded and bound by the caller (the A/B tools run
        several builds side by side); None: the in-tree library."""
        self._L = _lib.load() if lib is None else lib
        h = _lib.vp()
        check(self._L.rtp_create(int(device), h))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            self._L.rtp_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, entry: str, *args, stats: bool = True) -> RtpStats:
        """entry(ctx, *args, rtp_stats*): raise unless RTP_OK, return the stats.
        The *_device entries end in (..., hip_stream, stats) and fill the
        stats only when asked, which synchronises: they pass stats=timed."""
        st = RtpStats()
        check(getattr(self._L, entry)(self.handle, *args, st if stats else None))
        return st

    def set_scene(self, coords, quad_points, quad_mat, quad_tex, sphere_points, sphere_radius, sphere_mat,
                  sphere_tex, mat_type, tex_type, tex, light_quad_points=(8, 9, 10, 11), light_sphere_point=48,
                  ior=1.5):
        d, _arrays = scene_desc(coords, quad_points, quad_mat, quad_tex, sphere_points, sphere_radius, sphere_mat,
                                sphere_tex, mat_type, tex_type, tex, light_quad_points, light_sphere_point, ior)
        check(self._L.rtp_set_scene(self.handle, d))

    def set_scene_mesh(self, coords, quad_points, quad_mat, quad_tex, sphere_points, sphere_radius, sphere_mat,
                       sphere_tex, mat_type, tex_type, tex, light_quad_points=(8, 9, 10, 11), light_sphere_point=48,
                       ior=1.5):
        """rtp_set_scene_mesh: set_scene's arguments, any number of quads up to
        2^22 behind a BVH in device memory, at most 8 spheres.  quad_points is
        [N, 4], or [N, 3] for triangle cells: a row (a, b, c) is the cell
        (a, b, c, c), which always gets a tight box (rtp.triangulate splits
        the bent quads of a curved surface; mesh_counts() tells how many
        cells every ray has to test)."""
        d, _arrays = mesh_scene_desc(coords, quad_points, quad_mat, quad_tex, sphere_points, sphere_radius,
                                     sphere_mat, sphere_tex, mat_type, tex_type, tex, light_quad_points,
                                     light_sphere_point, ior)
        check(self._L.rtp_set_scene_mesh(self.handle, d))

    def set_scene_mesh_device(self, coords, quad_points, quad_mat, quad_tex, sphere_points, sphere_radius, sphere_mat,
                              sphere_tex, mat_type, tex_type, tex, light_quad_points=(8, 9, 10, 11),
                              light_sphere_point=48, ior=1.5, stream=None):
        """rtp_set_scene_mesh_device: the mesh scene of set_scene_mesh from
        tensors that live on this device's GPU -- coords float32 [P, 3],
        quad_points int32 [Q, 4], quad_mat and quad_tex int32 [Q], contiguous
        -- with the BVH built there.  The other arguments are host arrays as
        for set_scene_mesh.  ``stream``: a torch stream or a raw hipStream_t
        (None: torch's current stream on this device); the build is queued
        behind the work that produced the tensors there, and the call returns
        when the scene is in place.  The tensors are not kept.  quad_points
        may be int32 [Q, 3]: triangle cells, expanded to (a, b, c, c) with
        torch on the device, on the build's stream (no host copy)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if isinstance(quad_points, torch.Tensor) and quad_points.dim() == 2 and quad_points.shape[1] == 3 \
                and quad_points.is_cuda and quad_points.dtype == torch.int32:
            on = stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=self.device)
            with torch.cuda.stream(on):
                quad_points = cell_rows(quad_points).contiguous()
        want = (("coords", coords, torch.float32, (None, 3)), ("quad_points", quad_points, torch.int32, (None, 4)),
                ("quad_mat", quad_mat, torch.int32, (None,)), ("quad_tex", quad_tex, torch.int32, (None,)))
        for name, t, dtype, shape in want:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"set_scene_mesh_device: {name} must be a CUDA tensor on device {self.device}")
            if t.dtype != dtype or t.dim() != len(shape) or any(s is not None and t.shape[i] != s
                                                                 for i, s in enumerate(shape)):
                raise ValueError(f"set_scene_mesh_device: {name} must be {dtype} of shape "
                                 f"[{', '.join('N' if s is None else str(s) for s in shape)}]")
            if not t.is_contiguous():
                raise ValueError(f"set_scene_mesh_device: {name} must be contiguous")
        if not (quad_points.shape[0] == quad_mat.shape[0] == quad_tex.shape[0]):
            raise ValueError("set_scene_mesh_device: quad_points, quad_mat and quad_tex differ in length")
        none = np.zeros(0, dtype=np.int32)
        d, _arrays = scene_desc(np.zeros(0, dtype=np.float32), none, none, none, sphere_points, sphere_radius,
                                sphere_mat, sphere_tex, mat_type, tex_type, tex, light_quad_points,
                                light_sphere_point, ior)
        d.points = ctypes.cast(coords.data_ptr(), _lib.f32p)
        d.n_points = coords.shape[0]
        d.quad_points = ctypes.cast(quad_points.data_ptr(), _lib.i32p)
        d.quad_mat = ctypes.cast(quad_mat.data_ptr(), _lib.i32p)
        d.quad_tex = ctypes.cast(quad_tex.data_ptr(), _lib.i32p)
        d.n_quads = quad_points.shape[0]
        handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        check(self._L.rtp_set_scene_mesh_device(self.handle, d, handle))

    def mesh_guarantee(self) -> tuple[float, float]:
        """(cos_min, reach) of the current mesh scene (rtp_mesh_guarantee): the
        walk equals the scan of every quad for rays from within ``reach`` of
        the hit quad that meet its plane with |cos| >= ``cos_min``."""
        cm, rc = ctypes.c_float(), ctypes.c_float()
        check(self._L.rtp_mesh_guarantee(self.handle, cm, rc))
        return float(cm.value), float(rc.value)

    def mesh_counts(self) -> tuple[int, int, int]:
        """(cells, triangle cells, cells with an unbounded box) of the current
        mesh scene (rtp_mesh_counts).  Every ray tests the unbounded ones: a
        large third number is why a mesh renders slowly, and rtp.triangulate
        with rtp.unbounded_cells is the remedy."""
        n, tri, unb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(self._L.rtp_mesh_counts(self.handle, n, tri, unb))
        return int(n.value), int(tri.value), int(unb.value)

    def set_cornell_box(self, variant: int = 0):
        d = RtpSceneDesc()
        check(self._L.rtp_cornell_box(variant, d))
        check(self._L.rtp_set_scene(self.handle, d))

    def render(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, seed_base: int = 0):
        """Full canvas into host memory: (rgba_sum[nx*ny,4], stats)."""
        out = np.zeros((nx * ny, 4), dtype=np.float32)
        st = self._call("rtp_render", camera.to_c(), nx, ny, spp, depth, seed_base, ptr(out))
        return out, st

    def render_pixels(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, pixels, seed_base: int = 0):
        """Arbitrary pixel subset: (rgba_sum[n,4], final_seed[n], live[n], stats)."""
        ids = np.ascontiguousarray(pixels, dtype=np.int64)
        n = ids.size
        out = np.zeros((n, 4), dtype=np.float32)
        seeds = np.zeros(n, dtype=np.uint32)
        live = np.zeros(n, dtype=np.uint32)
        st = self._call("rtp_render_pixels", camera.to_c(), nx, ny, spp, depth, seed_base, ptr(ids), n,
                        ptr(out), pixel_aux(seeds, live))
        return out, seeds, live, st

    def render_device(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, out_ptr: int,
                      pixel_begin: int = 0, pixel_count: int | None = None, pixel_ids_ptr: int = 0,
                      seed_base: int = 0, stream: int = 0, seed_ptr: int = 0, live_ptr: int = 0,
                      timed: bool = False):
        """Device-resident render (out_ptr: device float4[pixel_count])."""
        if pixel_count is None:
            pixel_count = nx * ny - pixel_begin
        return self._call("rtp_render_device", camera.to_c(), nx, ny, spp, depth, seed_base, pixel_begin,
                          pixel_count, pixel_ids_ptr, out_ptr, pixel_aux(seed_ptr, live_ptr), stream, stats=timed)

    def render_planned_device(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, out_ptr: int,
                              pixel_count: int, wave_begin_ptr: int, n_waves: int, pixel_ids_ptr: int = 0,
                              pixel_begin: int = 0, seed_base: int = 0, stream: int = 0, seed_ptr: int = 0,
                              live_ptr: int = 0, timed: bool = False):
        """rtp_render_planned_device: wave w owns entries [wave_begin[w], wave_begin[w+1])."""
        return self._call("rtp_render_planned_device", camera.to_c(), nx, ny, spp, depth, seed_base,
                          pixel_begin, pixel_count, pixel_ids_ptr, wave_begin_ptr, n_waves, out_ptr,
                          pixel_aux(seed_ptr, live_ptr), stream, stats=timed)

    def render_tiles_device(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, out_ptr: int,
                            rank: int, world: int, seed_base: int = 0, stream: int = 0, timed: bool = False):
        """Device-resident render of rank's tiles of the round-robin 16x16
        tile deal (out_ptr: device float4[256 * tiles owned], each tile whole;
        on a canvas that is not whole tiles, shard.tile_entries gives the
        entries inside the canvas and their pixels)."""
        return self._call("rtp_render_tiles_device", camera.to_c(), nx, ny, spp, depth, seed_base, rank,
                          world, out_ptr, stream, stats=timed)

    @staticmethod
    def _views(cameras, seed_bases):
        """The rtp_view array of a camera list (checked before the library is touched)."""
        cameras = list(cameras)
        if not cameras:
            raise ErrorBadValue("render_views: at least one camera is required")
        if seed_bases is None:
            seed_bases = [0] * len(cameras)
        seed_bases = [int(b) for b in seed_bases]
        if len(seed_bases) != len(cameras):
            raise ErrorBadValue(f"render_views: {len(seed_bases)} seed bases for {len(cameras)} cameras")
        views = (RtpView * len(cameras))()
        for v, (cam, base) in enumerate(zip(cameras, seed_bases)):
            views[v].camera = cam.to_c()
            views[v].seed_base = base & 0xFFFFFFFF
        return views

    def render_views(self, cameras, nx: int, ny: int, spp: int, depth: int, seed_bases=None):
        """Several cameras in one launch into host memory (rtp_render_views):
        (rgba_sum[V, nx*ny, 4], stats with the totals over all views).  View v
        equals render(cameras[v], ..., seed_base=seed_bases[v]) bit for bit."""
        views = self._views(cameras, seed_bases)
        out = np.zeros((len(views), nx * ny, 4), dtype=np.float32)
        st = self._call("rtp_render_views", views, len(views), nx, ny, spp, depth, ptr(out))
        return out, st

    def render_views_device(self, cameras, nx: int, ny: int, spp: int, depth: int, out_ptr: int, seed_bases=None,
                            stream: int = 0, seed_ptr: int = 0, live_ptr: int = 0, timed: bool = False):
        """Device-resident rtp_render_views_device (out_ptr: device
        float4[V * nx*ny], view-major; seed_ptr / live_ptr: device u32 arrays
        of the same length).  Asynchronous unless timed."""
        views = self._views(cameras, seed_bases)
        return self._call("rtp_render_views_device", views, len(views), nx, ny, spp, depth, out_ptr,
                          pixel_aux(seed_ptr, live_ptr), stream, stats=timed)

    def render_resume_device(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, rgba_ptr: int,
                             seed_ptr: int, live_ptr: int = 0, m2_ptr: int = 0, pixel_begin: int = 0,
                             pixel_count: int | None = None, pixel_ids_ptr: int = 0, stream: int = 0,
                             timed: bool = False):
        """rtp_render_resume_device: spp more samples of every entry of a
        device-resident render state (rgba_ptr: float4[pixel_count] running
        sums, seed_ptr: u32 RNG states; live_ptr, m2_ptr optional), updated in
        place.  Asynchronous unless timed."""
        if pixel_count is None:
            pixel_count = nx * ny - pixel_begin
        return self._call("rtp_render_resume_device", camera.to_c(), nx, ny, spp, depth, pixel_begin,
                          pixel_count, pixel_ids_ptr, render_state(rgba_ptr, seed_ptr, live_ptr, m2_ptr), stream,
                          stats=timed)

    def render_resume(self, camera: Camera, nx: int, ny: int, spp: int, depth: int, rgba: np.ndarray,
                      seed: np.ndarray, live: np.ndarray | None = None, m2: np.ndarray | None = None, pixels=None):
        """rtp_render_resume on host arrays, in place: rgba float32 [n, 4],
        seed uint32 [n], live uint32 [n] and m2 float32 [n] (optional), over
        the pixel list ``pixels`` (None: the whole canvas).  Returns stats."""
        n = rgba.shape[0]
        want = [(rgba, np.float32, (n, 4)), (seed, np.uint32, (n,))]
        want += [(a, dt, (n,)) for a, dt in ((live, np.uint32), (m2, np.float32)) if a is not None]
        for a, dt, shape in want:
            if not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == dt and a.shape == shape):
                raise ErrorBadValue(f"render_resume: expects C-contiguous {np.dtype(dt).name} arrays of shape {shape}")
        ids = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.int64)
        if ids is not None and ids.size != n:
            raise ErrorBadValue(f"render_resume: {ids.size} pixels for a state of {n} entries")
        return self._call("rtp_render_resume", camera.to_c(), nx, ny, spp, depth, ptr(ids), n,
                          render_state(rgba, seed, live, m2))

    # ------------------------------------------------ denoised previews --
    def render_guides_device(self, camera: Camera, nx: int, ny: int, g0_ptr: int = 0, g1_ptr: int = 0,
                             prim_ptr: int = 0, stream: int = 0, timed: bool = False):
        """rtp_render_guides_device: the path camera's first hit per pixel
        centre into device buffers (each optional): g0_ptr float4[nx*ny]
        (normal facing the ray, t), g1_ptr float4[nx*ny] (texture colour, hit
        flag), prim_ptr int32[nx*ny] (kind << 24 | index, -1 on a miss).
        Asynchronous unless timed."""
        cam = camera.to_c() if camera is not None else None
        return self._call("rtp_render_guides_device", cam, nx, ny, g0_ptr, g1_ptr, prim_ptr, stream,
                          stats=timed)

    def render_guides(self, camera: Camera, nx: int, ny: int):
        """rtp_render_guides into host memory: (g0 float32 [nx*ny, 4],
        g1 float32 [nx*ny, 4], prim int32 [nx*ny], stats)."""
        n = max(int(nx) * int(ny), 0)
        g0 = np.zeros((n, 4), dtype=np.float32)
        g1 = np.zeros((n, 4), dtype=np.float32)
        prim = np.zeros(n, dtype=np.int32)
        st = self._call("rtp_render_guides", camera.to_c(), nx, ny, ptr(g0), ptr(g1), ptr(prim))
        return g0, g1, prim, st

    def resolve_device(self, sums_ptr: int, n: int, cv_ptr: int, m2_ptr: int = 0, count_ptr: int = 0, spp: int = 0,
                       stream: int = 0, timed: bool = False):
        """rtp_resolve_device: a device-resident render state (sums_ptr
        float4[n]; m2_ptr float[n] and count_ptr int32[n] optional, without
        counts every entry has ``spp`` samples) to cv_ptr float4[n]: mean rgb
        and the variance of the mean luminance (-1: an invalid entry).
        Asynchronous unless timed."""
        return self._call("rtp_resolve_device", sums_ptr, m2_ptr, count_ptr, int(spp), int(n), cv_ptr, stream,
                          stats=timed)

    def denoise_device(self, cv_ptr: int, nx: int, ny: int, out_ptr: int, scratch_ptr: int, g0_ptr: int = 0,
                       g1_ptr: int = 0, levels: int = 5, sigma_l: float = 4.0, sigma_z: float = 1.0,
                       sigma_a: float = 0.1, normal_log2: int = 5, stream: int = 0, timed: bool = False):
        """rtp_denoise_device: ``levels`` levels of the a-trous filter over
        cv_ptr (float4[nx*ny] from resolve_device) guided by g0_ptr / g1_ptr
        (both or neither) into out_ptr; scratch_ptr is a second float4[nx*ny].
        Parameters: include/rtp.h rtp_denoise_params (the defaults are
        ProgressiveRender.denoised's).  Asynchronous unless timed."""
        prm = _lib.RtpDenoiseParams(int(levels), float(sigma_l), float(sigma_z), float(sigma_a), int(normal_log2))
        return self._call("rtp_denoise_device", cv_ptr, g0_ptr, g1_ptr, nx, ny, prm, out_ptr, scratch_ptr,
                          stream, stats=timed)

    FF_POLICIES = {"auto": _lib.RTP_FF_TABLES_AUTO, "off": _lib.RTP_FF_TABLES_OFF, "on": _lib.RTP_FF_TABLES_ON}

    def sphere_walk(self) -> str:
        """How renders search the current scene's spheres (include/rtp.h
        rtp_sphere_walk): 'scan', 'global' (threaded BVH in global memory) or
        'lds' (the LDS-resident walk)."""
        return ("scan", "global", "lds")[self._L.rtp_sphere_walk(self.handle)]

    def sphere_walk_oct_mask(self) -> int:
        """The global sphere walk's octant mask (rtp_sphere_walk_oct_mask): 7
        = every direction octant walks its own near-to-far copy; -1 without a
        sphere BVH."""
        return int(self._L.rtp_sphere_walk_oct_mask(self.handle))

    def set_ff_tables(self, policy: str) -> dict:
        """RNG jump-table policy of this context (include/rtp.h rtp_set_ff_tables):
        'auto' (default), 'off', or 'on' (build now: a long-lived renderer).
        Returns ff_info()."""
        check(self._L.rtp_set_ff_tables(self.handle, self.FF_POLICIES[policy]))
        return self.ff_info()

    def ff_info(self) -> dict:
        """The device's jump tables: policy, what is built, bytes, setup cost."""
        i = RtpFfInfo()
        check(self._L.rtp_get_ff_tables(self.handle, i))
        d = {k: getattr(i, k) for k, _ in RtpFfInfo._fields_}
        d["policy"] = {v: k for k, v in self.FF_POLICIES.items()}.get(d["policy"], d["policy"])
        return d

    DEBUG_COUNTERS = _lib.DEBUG_COUNTERS

    def debug_counters(self) -> dict:
        """Pool-kernel counters of the last launch made with RTP_DEBUG_STATS=1."""
        out = np.zeros(_lib.N_DBG_COUNTERS + 1, dtype=np.uint64)
        waves = self._L.rtp_debug_counters(self.handle, ptr(out), out.size)
        d = {k: int(v) for k, v in zip(self.DEBUG_COUNTERS, out)}
        d["waves"] = int(waves)
        return d

    def debug_wave_records(self) -> np.ndarray:
        """Raw per-wave counter records [waves, kDbgCounters] of the last stats launch."""
        waves = self.debug_counters()["waves"]
        buf = np.zeros((max(waves, 1), _lib.N_DBG_COUNTERS), dtype=np.uint64)
        self._L.rtp_debug_counters(self.handle, ptr(buf), -1)
        return buf[:waves]

    def verify_fast_math(self, kind: int, lo: float, hi: float) -> tuple[int, int]:
        """Exhaustive device check over every float in [lo, hi] (same sign)."""
        lb = int(np.float32(lo).view(np.uint32))
        hb = int(np.float32(hi).view(np.uint32))
        lb, hb = min(lb, hb), max(lb, hb)
        bad = ctypes.c_uint64(0)
        first = ctypes.c_uint32(0)
        check(self._L.rtp_verify_fast_math(self.handle, kind, lb, hb, bad, first))
        return int(bad.value), int(first.value)

    def eval_primitive(self, kind: int, values: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(values)
        assert a.dtype.itemsize == 4
        out = np.zeros_like(a)
        check(self._L.rtp_eval_primitive(self.handle, kind, a.ctypes.data, out.ctypes.data, a.size))
        return out

    def debug_closest_hit(self, rays: np.ndarray) -> np.ndarray:
        """(n, 6) float32 rays (o, d) -> (n, 7) uint32: prefiltered (t bits,
        kind, index), exact scan (t bits, kind, index), fell-back flag."""
        a = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((a.shape[0], 7), dtype=np.uint32)
        check(self._L.rtp_debug_closest_hit(self.handle, ptr(a), a.shape[0], ptr(out)))
        return out

    def debug_raygen(self, camera: Camera, nx: int, ny: int, pixels, seeds):
        """The path kernel's camera ray for rows of (pixel index, RNG state):
        (the 12 camera constants the host derived for the launch as float32
        -- eye, nlook, delta_x, delta_y --, and (n, 5) uint32: the direction
        (float bits), the RNG state after the two draws, the pixel index)."""
        ids = np.ascontiguousarray(pixels, dtype=np.int64).reshape(-1)
        s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        if s.shape[0] != ids.shape[0]:
            raise ValueError("debug_raygen: one seed per pixel")
        out = np.zeros(12 + 5 * ids.shape[0], dtype=np.uint32)
        check(self._L.rtp_debug_raygen(self.handle, camera.to_c(), nx, ny, ptr(ids), ptr(s), ids.shape[0], ptr(out)))
        return out[:12].view(np.float32).copy(), out[12:].reshape(-1, 5).copy()

    def debug_bounce(self, rays: np.ndarray, seeds: np.ndarray) -> np.ndarray:
        """(n, 6) float32 rays (o, d) and (n,) uint32 RNG states -> (n, 15)
        uint32, one depth of the path kernel's bounce: result (0 goes on, 1
        missed, 2 light), emitted, attenuation[0], next origin, next
        direction (float bits), the RNG state after the depth, non-finite flag."""
        a = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        if s.shape[0] != a.shape[0]:
            raise ValueError("debug_bounce: one seed per ray")
        out = np.zeros((a.shape[0], 15), dtype=np.uint32)
        check(self._L.rtp_debug_bounce(self.handle, ptr(a), ptr(s), a.shape[0], ptr(out)))
        return out
