"""Host-side mirror of the reference's MapperPathTracer API over librtp.so.

Names, argument meaning and error behaviour follow the reference so that
code written against ``vtkm::rendering::MapperPathTracer`` (and the parts of
main.cc that drive it) reads the same:

    cb = CornellBox(); cb.buildDataSet()
    canvas = CanvasRayTracer(nx, ny)
    cam = Camera(); cam.SetPosition(...); cam.SetLookAt(...); ...
    mapper = MapperPathTracer(spp, depth, cb.matIdx, cb.texIdx, cb.matType, cb.texType, cb.tex)
    mapper.SetCanvas(canvas)
    mapper.RenderCells(cb.ds.GetCellSet(), cb.coord, field, ct, cam, sr)
    normalize(canvas.GetColorBuffer(), spp)            # NormalizeFunctor
    save_pnm("output.pnm", canvas.GetColorBuffer(), nx, ny)

Reference: MapperPathTracer.h:44-159, MapperPathTracer.cxx:94-406,
main.cc:253-384, CornellBox.cpp:141-418.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._lib import ErrorBadValue, RtpCamera, RtpSceneDesc, check, ptr
from .device import Device  # (Device, ErrorBadValue and check are also imported from here by callers)


# ------------------------------------------------------------- camera --
class Camera:
    """The vtkm::rendering::Camera fields MapperPathTracer reads
    (pathtracing/Camera.cxx:624-637)."""

    def __init__(self):
        self.position = np.array([0.0, 0.0, 1.0], dtype=np.float32)
        self.look_at = np.zeros(3, dtype=np.float32)
        self.view_up = np.array([0.0, 1.0, 0.0], dtype=np.float32)
        self.fov = np.float32(60.0)
        self.zoom = np.float32(1.0)
        self.clipping = (0.01, 1000.0)

    def SetPosition(self, p):
        self.position = np.asarray(p, dtype=np.float32).reshape(3).copy()

    def SetLookAt(self, p):
        self.look_at = np.asarray(p, dtype=np.float32).reshape(3).copy()

    def SetViewUp(self, p):
        self.view_up = np.asarray(p, dtype=np.float32).reshape(3).copy()

    def SetFieldOfView(self, deg):
        self.fov = np.float32(deg)

    def SetZoom(self, z):  # RayGen is built with _zoom = 0: zoom never reaches the path
        self.zoom = np.float32(z)

    def SetClippingRange(self, near, far):  # unused by the path tracer
        self.clipping = (near, far)

    def GetPosition(self):
        return self.position.copy()

    def GetLookAt(self):
        return self.look_at.copy()

    def GetViewUp(self):
        return self.view_up.copy()

    def GetFieldOfView(self):
        return float(self.fov)

    def to_c(self) -> RtpCamera:
        c = RtpCamera()
        c.position[:] = [float(v) for v in self.position]
        c.look_at[:] = [float(v) for v in self.look_at]
        c.view_up[:] = [float(v) for v in self.view_up]
        c.fov_y_deg = float(self.fov)
        return c


def default_camera() -> Camera:
    """The camera of main.cc:616-622."""
    cam = Camera()
    cam.SetClippingRange(0.1, 5.0)
    cam.SetPosition([278 / 555.0, 278 / 555.0, -800 / 555.0])
    cam.SetFieldOfView(40.0)
    cam.SetViewUp([0, 1, 0])
    cam.SetLookAt([278 / 555.0, 278 / 555.0, 278 / 555.0])
    return cam


# ------------------------------------------------------------- canvas --
class Canvas:
    def __init__(self, nx: int, ny: int):
        self.width, self.height = int(nx), int(ny)

    def GetWidth(self):
        return self.width

    def GetHeight(self):
        return self.height


class CanvasRayTracer(Canvas):
    """Colour buffer = Vec4f per pixel, index j*nx + i (row 0 = camera bottom)."""

    def __init__(self, nx: int, ny: int):
        super().__init__(nx, ny)
        self.color = np.zeros((self.width * self.height, 4), dtype=np.float32)
        self.depth = np.full(self.width * self.height, np.float32(1.001), dtype=np.float32)

    def GetColorBuffer(self) -> np.ndarray:
        return self.color

    def GetDepthBuffer(self) -> np.ndarray:
        """Canvas depth (written by the -direct mappers; 1.001 = cleared)."""
        return self.depth


# -------------------------------------------------------------- scene --
@dataclass
class CellSet:
    """The parts of the explicit cell set the path tracer consumes: quad
    cells (QuadExtractor rows p0..p3) and vertex cells (sphere centres)."""

    quad_points: np.ndarray  # int32 [Q,4]
    sphere_points: np.ndarray  # int32 [S]
    quad_cells: np.ndarray | None = None  # int32 [Q]: QuadIds[0], the cell id of each quad
    sphere_radius: np.ndarray | None = None  # float32 [S]: SphereRadii (None: 90/555 each, extract())


@dataclass
class Field:
    """vtkm::cont::Field (point association): a name and one value per entry."""

    name: str
    values: np.ndarray  # float32

    def GetName(self) -> str:
        return self.name

    def GetRange(self) -> tuple[float, float]:
        return float(self.values.min()), float(self.values.max())


@dataclass
class DataSet:
    cellset: CellSet
    coords: np.ndarray  # float32 [P,3]
    fields: dict = field(default_factory=dict)

    def GetCellSet(self) -> CellSet:
        return self.cellset

    def GetField(self, name: str) -> Field:
        if name not in self.fields:
            raise ErrorBadValue(f"No field with requested name: {name}")
        return self.fields[name]

    def AddField(self, f: Field) -> None:
        self.fields[f.name] = f


@dataclass
class CornellBox:
    """CornellBox (CornellBox.h:9-55); buildDataSet delegates to librtp's
    rtp_cornell_box (the same float/double arithmetic as CornellBox.cpp)."""

    variant: int = 0
    tex: np.ndarray | None = None
    matIdx: list = field(default_factory=list)
    texIdx: list = field(default_factory=list)
    matType: np.ndarray | None = None
    texType: np.ndarray | None = None
    coord: np.ndarray | None = None
    SphereRadii: np.ndarray | None = None
    ds: DataSet | None = None
    light_quad_points: tuple = (8, 9, 10, 11)
    light_sphere_point: int = 48
    ior: float = 1.5

    def buildDataSet(self) -> DataSet:
        L = _lib.load()
        d = RtpSceneDesc()
        check(L.rtp_cornell_box(self.variant, d))
        npz = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy()
        self.coord = npz(d.points, 3 * d.n_points, np.float32).reshape(-1, 3)
        quads = npz(d.quad_points, 4 * d.n_quads, np.int32).reshape(-1, 4)
        spheres = npz(d.sphere_point, d.n_spheres, np.int32)
        self.SphereRadii = npz(d.sphere_radius, d.n_spheres, np.float32)
        self.matIdx = [npz(d.quad_mat, d.n_quads, np.int32), npz(d.sphere_mat, d.n_spheres, np.int32)]
        self.texIdx = [npz(d.quad_tex, d.n_quads, np.int32), npz(d.sphere_tex, d.n_spheres, np.int32)]
        self.matType = npz(d.mat_type, d.n_mat, np.int32)
        self.texType = npz(d.tex_type, d.n_tex_type, np.int32)
        self.tex = npz(d.tex_rgb, 3 * d.n_tex, np.float32).reshape(-1, 3)
        self.light_quad_points = tuple(int(v) for v in d.light_quad_points)
        self.light_sphere_point = int(d.light_sphere_point)
        self.ior = float(d.ior)
        fp, nf, qc, nq = _lib.f32p(), ctypes.c_int32(), _lib.i32p(), ctypes.c_int32()
        check(L.rtp_cornell_point_field(self.variant, fp, nf, qc, nq))
        cells = npz(qc, nq.value, np.int32)
        self.ds = DataSet(CellSet(quads, spheres, cells), self.coord)
        self.ds.AddField(Field("point_var", npz(fp, nf.value, np.float32)))  # CornellBox.cpp:411-416
        return self.ds


# ------------------------------------------------------------- mapper --
def _set_scene(dev: Device, cellset: CellSet, coords, matIdx, texIdx, matType, texType, tex, light_quad_points,
               light_sphere_point, ior):
    """The reference's scene pieces (index 0 of matIdx / texIdx: quads, 1:
    spheres) in Device.set_scene's order."""
    radii = cellset.sphere_radius
    if radii is None:
        radii = np.full(len(cellset.sphere_points), np.float32(90 / 555.0), dtype=np.float32)  # extract(), :182
    # more than 256 distinct quads (rtp_set_scene's inline limit): a mesh scene, the quads behind a BVH
    setter = dev.set_scene_mesh if _distinct_quads(coords, cellset.quad_points, matIdx[0], texIdx[0]) > 256 \
        else dev.set_scene
    setter(coords, cellset.quad_points, matIdx[0], texIdx[0], cellset.sphere_points, radii, matIdx[1],
           texIdx[1], matType, texType, tex, light_quad_points, light_sphere_point, ior)


def _distinct_quads(coords, quad_points, quad_mat, quad_tex) -> int:
    """Quads that differ from every earlier one in a vertex (bit for bit, in
    order), the material or the texture: what rtp_set_scene keeps."""
    qp = np.asarray(quad_points, dtype=np.int64).reshape(-1, 4)
    if len(qp) <= 256:
        return len(qp)
    pts = np.ascontiguousarray(coords, dtype=np.float32).reshape(-1, 3).view(np.uint32)
    if qp.min() < 0 or qp.max() >= len(pts):
        return len(qp)  # (the library reports the bad id)
    key = np.concatenate([pts[qp].reshape(len(qp), 12).astype(np.int64),
                          np.asarray(quad_mat, dtype=np.int64).reshape(-1, 1),
                          np.asarray(quad_tex, dtype=np.int64).reshape(-1, 1)], axis=1)
    return len(np.unique(key, axis=0))


def _cells_with_radii(cb: CornellBox) -> CellSet:
    """The box's cell set carrying its SphereRadii (main.cc hands both to the mapper)."""
    return replace(cb.ds.GetCellSet(), sphere_radius=cb.SphereRadii)


def _set_cornell_scene(dev: Device, cb: CornellBox) -> None:
    _set_scene(dev, _cells_with_radii(cb), cb.coord, cb.matIdx, cb.texIdx, cb.matType, cb.texType, cb.tex,
               cb.light_quad_points, cb.light_sphere_point, cb.ior)


class MapperPathTracer:
    """vtkm::rendering::MapperPathTracer (MapperPathTracer.h:44-159)."""

    def __init__(self, sc: int, dc: int, matIdx, texIdx, matType, texType, tex, device: int | Device = 0):
        self.samplecount = int(sc)
        self.depthcount = int(dc)
        self.MatIdx, self.TexIdx = matIdx, texIdx
        self.MatType, self.TexType, self.Tex = matType, texType, tex
        self._dev = device if isinstance(device, Device) else Device(device)
        self._canvas = None
        self.CompositeBackground = True
        self.last_stats = None

    def SetCanvas(self, canvas):  # MapperPathTracer.cxx:155-172
        if canvas is not None and not isinstance(canvas, CanvasRayTracer):
            raise ErrorBadValue("Ray Tracer: bad canvas type. Must be CanvasRayTracer")
        self._canvas = canvas

    def GetCanvas(self):
        return self._canvas

    def SetCompositeBackground(self, on: bool):
        self.CompositeBackground = bool(on)

    def StartScene(self):
        pass

    def EndScene(self):
        pass

    def NewCopy(self) -> "MapperPathTracer":  # shallow copy sharing Internals (:403-406)
        m = MapperPathTracer.__new__(MapperPathTracer)
        m.__dict__.update(self.__dict__)
        return m

    def RenderCells(self, cellset: CellSet, coords, scalarField=None, colorTable=None, camera: Camera = None,
                    scalarRange=None, light_quad_points=(8, 9, 10, 11), light_sphere_point=48, ior=1.5):
        """MapperPathTracer.cxx:356-383: the canvas colour buffer receives the
        un-normalised per-pixel sum over samplecount samples."""
        if self._canvas is None:
            raise ErrorBadValue("MapperPathTracer: SetCanvas was not called")
        if camera is None:
            raise ErrorBadValue("MapperPathTracer: no camera")
        _set_scene(self._dev, cellset, coords, self.MatIdx, self.TexIdx, self.MatType, self.TexType, self.Tex,
                   light_quad_points, light_sphere_point, ior)
        nx, ny = self._canvas.GetWidth(), self._canvas.GetHeight()
        out, st = self._dev.render(camera, nx, ny, self.samplecount, self.depthcount)
        self._canvas.color[...] = out
        self.last_stats = st


# -------------------------------------------------------- application --
def normalize(colors: np.ndarray, samplecount: int) -> np.ndarray:
    """NormalizeFunctor (main.cc:253-287), in place; returns colors."""
    a = colors
    if not (a.flags.c_contiguous and a.dtype == np.float32):
        raise ValueError("normalize: expects a C-contiguous float32 [N,4] buffer")
    check(_lib.load().rtp_normalize(ptr(a), a.shape[0], int(samplecount)))
    return a


def save_pnm(path: str, colors: np.ndarray, nx: int, ny: int) -> None:
    """save() (main.cc:325-384): P3, buffer order, int(255.99*c)."""
    a = np.ascontiguousarray(colors, dtype=np.float32)
    check(_lib.load().rtp_write_pnm(path.encode(), ptr(a), nx, ny))


def runPath(nx: int, ny: int, samplecount: int, depthcount: int, canvas: CanvasRayTracer, cam: Camera,
            cb: CornellBox, device: int | Device = 0) -> MapperPathTracer:
    """main.cc:289-323."""
    mapper = MapperPathTracer(samplecount, depthcount, cb.matIdx, cb.texIdx, cb.matType, cb.texType, cb.tex,
                              device=device)
    mapper.SetCanvas(canvas)
    mapper.RenderCells(_cells_with_radii(cb), cb.coord, None, None, cam, None, cb.light_quad_points,
                       cb.light_sphere_point, cb.ior)
    normalize(canvas.GetColorBuffer(), samplecount)
    return mapper


def runPathViews(nx: int, ny: int, samplecount: int, depthcount: int, cameras, cb: CornellBox,
                 device: int | Device = 0) -> np.ndarray:
    """runPath (main.cc:289-323) for every camera of a list in one launch:
    the normalised colour buffers [V, nx*ny, 4], view v equal to runPath's
    canvas for cameras[v]."""
    cameras = list(cameras)
    if not cameras:
        raise ErrorBadValue("runPathViews: at least one camera is required")
    dev = device if isinstance(device, Device) else Device(device)
    _set_cornell_scene(dev, cb)
    out, _ = dev.render_views(cameras, nx, ny, samplecount, depthcount)
    normalize(out.reshape(-1, 4), samplecount)
    return out


def runPathProgressive(nx: int, ny: int, samplecount: int, depthcount: int, canvas: CanvasRayTracer, cam: Camera,
                       cb: CornellBox, passes: int, device: int | Device = 0, on_pass=None):
    """runPath rendered in ``passes`` resumable passes (progressive.split_passes):
    the canvas receives the same normalised colours as runPath's.  on_pass(i,
    render), when given, is called after each pass (a preview hook).  Returns
    the ProgressiveRender."""
    from .progressive import ProgressiveRender, split_passes

    sizes = split_passes(samplecount, passes)
    dev = device if isinstance(device, Device) else Device(device)
    _set_cornell_scene(dev, cb)
    render = ProgressiveRender(dev, cam, nx, ny, depthcount)
    for i, spp in enumerate(sizes):
        render.step(spp)
        if on_pass is not None:
            on_pass(i, render)
    canvas.color[...] = render.sums.cpu().numpy()
    normalize(canvas.GetColorBuffer(), samplecount)
    return render


def hemisphere_cameras(phi_count: int = 15, theta_count: int = 15) -> list:
    """The cameras of generateHemisphere (main.cc:504-561) with the parameters
    main() passes (:583-595), in its loop order: phi in [0, 1) by 1/phiCount,
    theta in [0, 2pi) by (float)(2pi)/thetaCount, radius -1078/555 around
    (278,278,278)/555.  The reference's float variables and its mix of float
    and double operations, restated in float32 (cosf/sinf are libm's, as in
    the C++ driver); each camera also carries its .phi and .theta (the view's
    file-name suffix is "-%.4f-%.4f" of them)."""
    if phi_count < 1 or theta_count < 1:
        raise ErrorBadValue("hemisphere_cameras: phi_count and theta_count must be >= 1")
    import ctypes.util

    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f32 = np.float32
    fn = {}
    for name in ("cosf", "sinf"):
        f = getattr(libm, name)
        f.argtypes, f.restype = [ctypes.c_float], ctypes.c_float
        fn[name] = lambda x, f=f: f32(f(float(x)))
    theta_end = f32(2 * 3.14159265358979323846)
    r_theta = f32(theta_end / f32(theta_count))
    r_phi = f32(f32(1.0) / f32(phi_count))
    r = f32(-1078 / 555.0)
    c = 278 / 555.0
    phi_bound = 1.0 - 0.5 * float(r_phi)  # compared in double
    cams = []
    phi = f32(0.0)
    while float(phi) < phi_bound:
        theta = f32(0.0)
        while theta < theta_end:
            px = f32(f32(r * fn["cosf"](theta)) * fn["sinf"](phi))
            py = f32(f32(r * fn["sinf"](theta)) * fn["sinf"](phi))
            pz = f32(r * fn["cosf"](phi))
            cam = default_camera()
            cam.SetClippingRange(1.0, 5.0)  # generateHemisphere's own near plane (main.cc:519)
            cam.SetPosition([f32(float(px) + c), f32(float(py) + c), f32(float(pz) + c)])
            cam.phi, cam.theta = float(phi), float(theta)
            cams.append(cam)
            theta = f32(theta + r_theta)
        phi = f32(phi + r_phi)
    return cams
