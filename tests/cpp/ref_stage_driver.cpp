// ref_stage_driver.cpp: runs the reference's own code -- its worklet headers,
// its ray generator, its seed initialiser and the kernel of its backward
// product -- one stage, one whole depth or one whole small frame at a time, on
// cases read from a flat binary file.
//
// TEST INFRASTRUCTURE ONLY.  The headers below are the reference's, found by
// oracle/ref_build.py in the reference tree (nothing of them is in this
// repository); the VTK-m names they include resolve in tests/cpp/vtkm_min/.
// Two reference classes live in .cxx files that cannot be compiled whole
// (Camera::RayGen in pathtracing/Camera.cxx, details::WangInit in
// MapperPathTracer.cxx): ref_build.py cuts their text, unchanged, into
// oracle/_ref/gen/*.inc at build time, and this file includes those.
// What this file adds is glue: which array goes to which argument, the
// per-depth resets RenderCellsImpl performs between the worklets, what
// CreateRays resets per sample, and the order of the backward product's
// passes.  Every such line cites the reference line it restates.  The built
// program is oracle/_ref/ref_stages; tools/make_ref_stage_golden.py records
// its outputs in tests/golden/ref_stages.npz and ref_frames.npz, and
// tests/test_ref_stages.py replays them.
//
//   ref_stages CASES RESULTS
//
// CASES   : u32 magic, i32 mode, i32 n, i32 kin, the scene section, n*kin words
// RESULTS : i32 mode, i32 n, i32 kout, n*kout words
// The word layouts of every mode are those of tests/_ref_cases.py (STAGES,
// FRAME_STAGES).  `backward` rows start with their own D and S (kin = 2 + 8*S*D);
// `frame` takes one row and answers 5 words per pixel and one 37-word state
// per (sample, depth, ray): kout is what that comes to.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pathtracing/EmitWorklet.h"
#include "pathtracing/PathAlgorithms.h"
#include "pathtracing/PdfWorklet.h"
#include "pathtracing/ScatterWorklet.h"
#include "pathtracing/SurfaceWorklets.h"

// The reference's text, in the scopes it has there (Camera.h declares `class RayGen;` inside Camera;
// MapperPathTracer.cxx:58-77 opens vtkm::rendering::details).
namespace vtkm {
namespace rendering {
namespace pathtracing {
class Camera {
public:
  class RayGen;
};
#include "gen/camera_raygen.inc"
} // namespace pathtracing
namespace details {
#include "gen/wang_init.inc"
} // namespace details
} // namespace rendering
} // namespace vtkm

namespace {

using Dev = vtkm::cont::DeviceAdapterTagSerial;
using HitRecord = vtkm::Vec<vtkm::Float32, 9>;     // QuadIntersector::HitRecord's value (Record.h HR)
using HitId = vtkm::Vec<vtkm::Int32, 2>;           // matIdArray, texIdArray (MapperPathTracer.cxx:241, 263)
using ScatterRecord = vtkm::Vec<vtkm::Float32, 9>; // Record.h SR
template <typename T>
using Portal = vtkm::cont::ArrayPortal<T>;
using vtkm::Id;

enum Mode {
  RNG = 0, WHICH, ONB, QUADHIT, SPHEREHIT, MATERIAL, DIELECTRIC, GENERATOR, LIGHTPDF, SCATTER, COLLECT, BOUNCE,
  CAMERA, RAYGEN, SEED_INIT, BACKWARD, FRAME
};
const int KIN[] = {1, 1, 6, 20, 12, 20, 12, 9, 10, 26, 1, 7, 12, 14, 1, -1, 14}; // -1: set by the rows themselves
const int REC = 37; // one bounce checkpoint
const int CHECKPOINTS = 13;
const int KOUT[] = {3, 2, 12, 12, 8, 14, 9, 4, 2, 10, 7, REC * CHECKPOINTS, 9, 5, 1, 4, -1}; // -1: set by the run
using Vec4 = vtkm::Vec<vtkm::Float32, 4>;
using RayGen = vtkm::rendering::pathtracing::Camera::RayGen;

union Word {
  uint32_t u;
  int32_t i;
  float f;
};

struct Reader {
  const Word* p;
  const Word* end;
  Word next() {
    if (p >= end) {
      fprintf(stderr, "ref_stages: case file is truncated\n");
      exit(2);
    }
    return *p++;
  }
  int32_t i() { return next().i; }
  float f() { return next().f; }
  vec3 v() {
    float a = f(), b = f(), c = f();
    return vec3(a, b, c);
  }
};

struct Scene {
  std::vector<vec3> points;
  std::vector<vtkm::Vec<Id, 5>> quad_ids;
  std::vector<Id> quad_mat, quad_tex, sphere_point, sphere_mat, sphere_tex;
  std::vector<float> sphere_radius;
  std::vector<int> mat_type, tex_type;
  std::vector<vec3> tex;
  vtkm::Vec<Id, 5> light_box_pointids[1];
  Id light_box_indices[1] = {0};      // MapperPathTracer.cxx:143-144
  Id light_sphere_pointids[1];
  Id light_sphere_indices[1] = {0};   // MapperPathTracer.cxx:147-148
  float ior;
  std::vector<Id> quad_leaf, sphere_leaf; // one leaf holding every primitive in scene order

  void read(Reader& r) {
    int n = r.i();
    for (int k = 0; k < n; k++) points.push_back(r.v());
    n = r.i();
    for (int k = 0; k < n; k++) {
      Id a = r.i(), b = r.i(), c = r.i(), d = r.i(), e = r.i();
      quad_ids.push_back(vtkm::Vec<Id, 5>(a, b, c, d, e));
    }
    for (int k = 0; k < n; k++) quad_mat.push_back(r.i());
    for (int k = 0; k < n; k++) quad_tex.push_back(r.i());
    n = r.i();
    for (int k = 0; k < n; k++) sphere_point.push_back(r.i());
    for (int k = 0; k < n; k++) sphere_radius.push_back(r.f());
    for (int k = 0; k < n; k++) sphere_mat.push_back(r.i());
    for (int k = 0; k < n; k++) sphere_tex.push_back(r.i());
    n = r.i();
    for (int k = 0; k < n; k++) mat_type.push_back(r.i());
    n = r.i();
    for (int k = 0; k < n; k++) tex_type.push_back(r.i());
    n = r.i();
    for (int k = 0; k < n; k++) tex.push_back(r.v());
    Id l[5];
    for (int k = 0; k < 5; k++) l[k] = r.i();
    light_box_pointids[0] = vtkm::Vec<Id, 5>(l[0], l[1], l[2], l[3], l[4]); // MapperPathTracer.cxx:141
    light_sphere_pointids[0] = r.i();                                       // MapperPathTracer.cxx:145
    ior = r.f();
    // LinearBVH's leaf layout [count, index...] (BVHTraverser.h:209, Surface.h:224-227); the order
    // inside is this build's assumption: every primitive in one leaf, in scene order.
    quad_leaf.push_back((Id)quad_ids.size());
    for (size_t k = 0; k < quad_ids.size(); k++) quad_leaf.push_back((Id)k);
    sphere_leaf.push_back((Id)sphere_point.size());
    for (size_t k = 0; k < sphere_point.size(); k++) sphere_leaf.push_back((Id)k);
  }
  template <typename T>
  static Portal<const T> in(const std::vector<T>& v) {
    Portal<const T> p;
    p.p = v.data();
    p.n = (Id)v.size();
    return p;
  }
  template <typename T>
  static Portal<const T> in(const T* v, Id n) {
    Portal<const T> p;
    p.p = v;
    p.n = n;
    return p;
  }
  QuadLeafIntersector<Dev> quad_surf() const {
    return QuadLeafIntersector<Dev>(vtkm::cont::ArrayHandle<vtkm::Vec<Id, 5>>(quad_ids.data(), (Id)quad_ids.size()),
                                    vtkm::cont::ArrayHandle<Id>(quad_mat.data(), (Id)quad_mat.size()),
                                    vtkm::cont::ArrayHandle<Id>(quad_tex.data(), (Id)quad_tex.size()));
  }
  SphereLeafIntersector<Dev> sphere_surf() const {
    return SphereLeafIntersector<Dev>(vtkm::cont::ArrayHandle<Id>(sphere_point.data(), (Id)sphere_point.size()),
                                      vtkm::cont::ArrayHandle<float>(sphere_radius.data(), (Id)sphere_radius.size()),
                                      vtkm::cont::ArrayHandle<Id>(sphere_mat.data(), (Id)sphere_mat.size()),
                                      vtkm::cont::ArrayHandle<Id>(sphere_tex.data(), (Id)sphere_tex.size()));
  }
};

struct Writer {
  std::vector<Word> w;
  void u(uint32_t x) {
    Word t;
    t.u = x;
    w.push_back(t);
  }
  void i(int32_t x) {
    Word t;
    t.i = x;
    w.push_back(t);
  }
  void f(float x) {
    Word t;
    t.f = x;
    w.push_back(t);
  }
  void v(const vec3& x) { f(x[0]), f(x[1]), f(x[2]); }
};

HitRecord zero_hrec() { return HitRecord(0.f); }

// One ray's state between the worklets of one depth: the arrays of
// RenderCellsImpl that a worklet reads or writes, for one index.
struct Ray {
  vec3 org, dir;
  vtkm::UInt8 status;
  HitRecord hrec;
  HitId hid;
  ScatterRecord srec;
  int which;
  vec3 gen;
  float sum, tmin;
  vec3 E, A;
  unsigned int seed;
};

void put_ray(Writer& o, const Ray& r) {
  o.u(r.status);
  for (int k = 2; k < 9; k++) o.f(r.hrec[k]); // T, N, P (U, V are never read downstream)
  o.i(r.hid[0]), o.i(r.hid[1]);
  for (int k = 0; k < 9; k++) o.f(r.srec[k]);
  o.i(r.which);
  o.v(r.gen);
  o.f(r.sum);
  o.v(r.E), o.v(r.A), o.v(r.org), o.v(r.dir);
  o.u(r.seed);
}

// One depth of RenderCellsImpl (MapperPathTracer.cxx:286-301) for ray idx of a canvas of cs rays: every
// worklet writes plane `depth` of emitted and attenuation at canvasSize * depth + idx.  Where `rec` is given
// the ray's state goes there after every worklet, r.E and r.A being that plane's entries.
void bounce_at(const Scene& sc, Ray& r, Id cs, Id depth, Id idx, Portal<vec3> emitted, Portal<vec3> attenuation,
               Writer* rec) {
  auto pts = Scene::in(sc.points);
  auto put = [&](Writer&, const Ray&) {
    r.E = emitted.p[cs * depth + idx], r.A = attenuation.p[cs * depth + idx];
    if (rec) put_ray(*rec, r);
  };
  Writer unused;
  Writer& o = unused; // the puts below keep the text of one depth as it was; they write to rec
  r.sum = 0;                 // MapperPathTracer.cxx:287
  r.hrec[2] = FLT_MAX;       // :419 (rays.Distance is the T component of hrecs, :262)
  r.tmin = (float)0.001;     // :420
  auto qsurf = sc.quad_surf();
  auto ssurf = sc.sphere_surf();
  {                          // quadIntersector.IntersectRays (:426): BVHTraverser.h:128-227 over one leaf
    float tmax = r.hrec[2];  // BVHTraverser.h:249: rays.Distance is the tmax argument
    float closest = tmax;    // BVHTraverser.h:141
    qsurf.IntersectLeaf(0, r.org, r.dir, r.hrec, r.hid, r.tmin, closest, r.status, pts, Scene::in(sc.quad_leaf));
    if ((r.status & 8) && (r.status & 4)) tmax = closest; // BVHTraverser.h:225-226
    r.hrec[2] = tmax;        // the FieldInOut tmax is stored after hrecs into the same array
  }
  put(o, r);
  {                          // sphereIntersector.IntersectRays (:429)
    float tmax = r.hrec[2];
    float closest = tmax;
    ssurf.IntersectLeaf(0, r.org, r.dir, r.hrec, r.hid, r.tmin, closest, r.status, pts, Scene::in(sc.sphere_leaf));
    if ((r.status & 8) && (r.status & 4)) tmax = closest;
    r.hrec[2] = tmax;
  }
  put(o, r);
  CollectIntersecttWorklet(cs, (int)depth)(idx, r.status, emitted, attenuation); // :431-432
  put(o, r);
  auto tex = Scene::in(sc.tex);
  auto mt = Scene::in(sc.mat_type);
  auto tt = Scene::in(sc.tex_type);
  LambertianWorklet(cs, depth)(idx, r.org, r.dir, r.hrec, r.hid, r.srec, r.status, tex, mt, tt, emitted); // :470
  put(o, r);
  DiffuseLightWorklet(cs, depth)(idx, r.org, r.dir, r.hrec, r.hid, r.srec, r.status, tex, mt, tt, emitted); // :473
  put(o, r);
  DielectricWorklet(cs, depth, sc.ior, (vtkm::UInt32)cs)( // :467 (the literal 1.5), :476
      idx, r.seed, r.org, r.dir, r.hrec, r.hid, r.srec, r.status, tex, mt, tt, emitted);
  put(o, r);
  WorketletGenerateDir(3)(r.seed, r.which); // WhichGenerateDir.cxx:10-11
  put(o, r);
  CosineWorketletGenerateDir(1)(r.which, r.hrec, r.gen, r.seed); // CosineGenerateDir.h:18, 29
  put(o, r);
  QuadWorkletGenerateDir(2)(r.which, r.hrec, r.gen, r.seed, Scene::in(sc.light_box_pointids, 1), // QuadGenerateDir.h:22, 33
                            Scene::in(sc.light_box_indices, 1), pts);
  put(o, r);
  SphereWorkletGenerateDir(3)(idx, r.which, r.hrec, r.gen, r.seed, Scene::in(sc.light_sphere_pointids, 1), // SphereGenerateDir.h:24, 35
                              Scene::in(sc.light_sphere_indices, 1), pts, Scene::in(sc.sphere_radius));
  put(o, r);
  QuadPDFWorklet(2)(idx, r.org, r.dir, r.hrec, r.status, r.sum, r.gen, r.seed, qsurf, // QuadPdf.h:23, 35-37; lightables = 2 (:218)
                    Scene::in(sc.light_box_pointids, 1), Scene::in(sc.light_box_indices, 1), pts);
  put(o, r);
  SpherePDFWorklet(2)(idx, r.org, r.dir, r.hrec, r.status, r.sum, r.gen, r.seed, ssurf, // SpherePdf.h:26, 39-51
                      Scene::in(sc.light_sphere_pointids, 1), Scene::in(sc.light_sphere_indices, 1), pts,
                      Scene::in(sc.sphere_radius));
  put(o, r);
  {
    // :536-537: rays.Origin and rays.Dir are both the input and the output arguments; each
    // argument is loaded before the call and stored after it in argument order, so the
    // out_ arguments (8, 9) are what the arrays hold afterwards.
    vec3 out_o = r.org, out_d = r.dir;
    PDFCosineWorklet((int)cs, (int)depth, (vtkm::UInt32)cs, 2)(idx, r.org, r.dir, r.hrec, r.srec, r.status, r.sum,
                                                               r.gen, out_o, out_d, attenuation);
    r.org = out_o, r.dir = out_d;
  }
  put(o, r);
}

// ... for one ray with depth = 0 and a canvas of one ray, so that canvasSize * depth + idx = 0 in every worklet.
void bounce(const Scene& sc, Ray& r, Writer& o) {
  Portal<vec3> emitted, attenuation;
  emitted.p = &r.E, emitted.n = 1;
  attenuation.p = &r.A, attenuation.n = 1;
  bounce_at(sc, r, 1, 0, 0, emitted, attenuation, &o);
}

// What Camera::SetParameters and CreateRaysImpl hand RayGen's constructor, from a view's position, look-at,
// up, field of view and canvas.
struct CamIn {
  vec3 position, look_at, up;
  float fov;
  vtkm::Int32 nx, ny;
  void read(Reader& r) {
    position = r.v(), look_at = r.v(), up = r.v();
    fov = r.f();
    nx = r.i(), ny = r.i();
  }
  RayGen raygen() const {
    // Camera.cxx:773-781 SetUp: an up that differs from the one held (the constructor's (0, 1, 0), :595-597) is
    // stored and normalised; an equal one leaves it alone.
    vec3 Up(0.f, 1.f, 0.f);
    if (Up[0] != up[0] || Up[1] != up[1] || Up[2] != up[2]) {
      Up = up;
      vtkm::Normalize(Up);
    }
    // :790-797 SetLookAt and :806-813 SetPosition store their arguments; :716-764 SetFieldOfView keeps the
    // degrees as FovY (GetFieldOfView, :767-770) whatever FovX it derives from the aspect ratio.
    vec3 Look = look_at - position; // :913
    vtkm::Normalize(Look);          // :914
    // :936-941: fovX = fovY = GetFieldOfView(), zoom 0, the subset is the whole width from (0, 0)
    return RayGen(nx, ny, fov, fov, Look, Up, 0, nx, 0, 0);
  }
};

// The backward product of one sample, MapperPathTracer.cxx:326-348, through the reference's own kernel functor
// (PathAlgorithms.h:128-171); SliceTransform schedules it over output.GetNumberOfValues() indices (:244, 254).
// emitted4 and attenuation4 are D planes of cs entries, sumtotl cs entries.
void backward(Id cs, int depthcount, const std::vector<Vec4>& emitted4, const std::vector<Vec4>& attenuation4,
              std::vector<Vec4>& sumtotl) {
  namespace pd = vtkm::rendering::pathtracing::details;
  using In = Portal<const Vec4>;
  using Out = Portal<Vec4>;
  using Zero = vtkm::cont::ArrayHandleConstant<Vec4>;
  In E = Scene::in(emitted4), A = Scene::in(attenuation4), Sin = Scene::in(sumtotl);
  Out S;
  S.p = sumtotl.data(), S.n = cs;
  Zero zero(Vec4(0.0f), cs); // :326
  {
    pd::BinarySliceTransformIdxKernel<In, Zero, Out, vtkm::Sum> k( // :328-331
        std::make_tuple((depthcount - 1) * cs, (depthcount - 1) * cs + cs), E, std::make_tuple(0, cs), zero,
        std::make_tuple(0, cs), S, vtkm::Sum());
    for (Id i = 0; i < cs; i++) k(i);
  }
  for (int depth = depthcount - 2; depth >= 0; depth--) { // :333
    pd::BinarySliceTransformIdxKernel<In, In, Out, vtkm::Multiply> m( // :334-338
        std::make_tuple(depth * cs, depth * cs + cs), A, std::make_tuple(0, cs), Sin, std::make_tuple(0, cs), S,
        vtkm::Multiply());
    for (Id i = 0; i < cs; i++) m(i);
    pd::BinarySliceTransformIdxKernel<In, In, Out, vtkm::Sum> a( // :340-344
        std::make_tuple(depth * cs, depth * cs + cs), E, std::make_tuple(0, cs), Sin, std::make_tuple(0, cs), S,
        vtkm::Sum());
    for (Id i = 0; i < cs; i++) a(i);
  }
}

// cols = Transform(cols, sumtotl, Sum) (:350)
void canvas_sum(std::vector<Vec4>& cols, const std::vector<Vec4>& sumtotl) {
  for (size_t i = 0; i < cols.size(); i++) cols[i] = vtkm::Sum()(cols[i], sumtotl[i]);
}

// RenderCellsImpl:265-354 for a whole canvas.  The arrays the reference allocates and does not fill before it
// reads them (hrecs, srecs, hids, whichPDF, generated_dir, the depth planes, both alpha buffers) start as zero
// here: that is this build's assumption, as in the one-depth mode.  o gets 5 words per pixel (the canvas rgb, the
// final seed, the count of depths entered with the scatter bit set), st the state of every ray after every depth
// of every sample.
void frame(const Scene& sc, const CamIn& cam, int samplecount, int depthcount, Writer& o, Writer& st) {
  const Id cs = (Id)cam.nx * cam.ny; // :213
  std::vector<Ray> rays((size_t)cs);
  memset((void*)rays.data(), 0, sizeof(Ray) * rays.size());
  std::vector<vec3> emitted((size_t)(cs * depthcount), vec3(0.f)), attenuation((size_t)(cs * depthcount), vec3(0.f));
  std::vector<float> alphaAE((size_t)(cs * depthcount), 0.f); // :138
  std::vector<Vec4> sumtotl((size_t)cs, Vec4(0.f));          // :133-135, 139: sumtotlx/y/z and alphaChannel
  std::vector<Vec4> cols((size_t)cs, Vec4(0.0)); // :223
  std::vector<uint32_t> live((size_t)cs, 0);
  std::vector<vtkm::UInt32> seeds;
  vtkm::cont::Algorithm::CopyIf(vtkm::cont::ArrayHandleCounting<vtkm::UInt32>(0, 1, cs), // :265-267
                                vtkm::cont::ArrayHandleConstant<vtkm::UInt32>(1, cs), seeds,
                                vtkm::rendering::details::WangInit());
  if ((Id)seeds.size() != cs) {
    fprintf(stderr, "ref_stages: CopyIf kept %zu of %lld seeds\n", seeds.size(), (long long)cs);
    exit(3);
  }
  for (Id i = 0; i < cs; i++) rays[i].seed = seeds[i]; // rayCam.seeds (:248) is what RayGen and the worklets draw from
  Portal<vec3> E, A;
  E.p = emitted.data(), E.n = cs * depthcount;
  A.p = attenuation.data(), A.n = cs * depthcount;
  const RayGen raygen = cam.raygen();
  for (int s = 0; s < samplecount; s++) { // :278
    for (Id i = 0; i < cs; i++) {         // :282 rayCam.CreateRays
      Ray& r = rays[i];
      r.tmin = 0;    // Camera.cxx:900-901 MinDistance
      r.hrec[2] = 0; // Camera.cxx:902 Distance (the T component of hrecs, MapperPathTracer.cxx:262)
      vtkm::Id pixelIndex = 0;
      raygen(i, r.dir[0], r.dir[1], r.dir[2], r.seed, pixelIndex); // Camera.cxx:944
      r.org = cam.position;                                         // Camera.cxx:946-953
      r.status = 1u << 3;                                           // :283
    }
    for (int depth = 0; depth < depthcount; depth++) { // :286
      for (Id i = 0; i < cs; i++) {
        if (rays[i].status & 8) live[i]++;
        bounce_at(sc, rays[i], cs, depth, i, E, A, nullptr);
        rays[i].E = emitted[cs * depth + i], rays[i].A = attenuation[cs * depth + i];
        put_ray(st, rays[i]);
      }
    }
    // :315-324: the rgb of the planes with the alpha buffers as fourth component
    std::vector<Vec4> emitted4((size_t)(cs * depthcount)), attenuation4((size_t)(cs * depthcount));
    for (Id k = 0; k < cs * depthcount; k++) {
      emitted4[k] = Vec4(emitted[k][0], emitted[k][1], emitted[k][2], alphaAE[k]);
      attenuation4[k] = Vec4(attenuation[k][0], attenuation[k][1], attenuation[k][2], alphaAE[k]);
    }
    backward(cs, depthcount, emitted4, attenuation4, sumtotl);
    canvas_sum(cols, sumtotl); // :350
  }
  for (Id i = 0; i < cs; i++) {
    o.f(cols[i][0]), o.f(cols[i][1]), o.f(cols[i][2]);
    o.u(rays[i].seed), o.u(live[i]);
  }
}

void run(int mode, int n, int kin, const Scene& sc, Reader& in, Writer& o) {
  auto pts = Scene::in(sc.points);
  auto tex = Scene::in(sc.tex);
  auto mtp = Scene::in(sc.mat_type);
  auto ttp = Scene::in(sc.tex_type);
  for (int c = 0; c < n; c++) {
    switch (mode) {
      case RNG: {
        vtkm::UInt32 s = in.next().u, s2 = s;
        o.u(xorshiftWang::getWang32(s));
        float f = xorshiftWang::getRandF(s2);
        o.f(f), o.u(s2);
        break;
      }
      case WHICH: {
        unsigned int s = in.next().u;
        int which = 0;
        WorketletGenerateDir(3)(s, which);
        o.i(which), o.u(s);
        break;
      }
      case ONB: {
        vec3 nn = in.v(), a = in.v();
        onb uvw;
        uvw.build_from_w(nn);
        o.v(uvw.u()), o.v(uvw.v()), o.v(uvw.w()), o.v(uvw.local(a));
        break;
      }
      case QUADHIT: {
        vec3 org = in.v(), d = in.v(), v00 = in.v(), v10 = in.v(), v11 = in.v(), v01 = in.v();
        float tmin = in.f(), tmax = in.f();
        auto surf = sc.quad_surf();
        float u = 0, v = 0, t = 0;
        bool h = surf.hit(org, d, v00, v10, v11, v01, u, v, t);
        o.i(h), o.f(h ? u : 0), o.f(h ? v : 0), o.f(h ? t : 0); // recorded only where hit() reports a hit
        HitRecord rec = zero_hrec();
        HitId hid(0, 0);
        bool hi = surf.intersect(org, d, rec, hid, tmin, tmax, v00, v10, v11, v01, 0);
        o.i(hi);
        for (int k = 2; k < 9; k++) o.f(hi ? rec[k] : 0);
        break;
      }
      case SPHEREHIT: {
        vec3 org = in.v(), d = in.v(), ctr = in.v();
        float radius = in.f(), tmin = in.f(), tmax = in.f();
        HitRecord rec = zero_hrec();
        HitId hid(0, 0);
        bool h = sc.sphere_surf().hit(org, d, rec, hid, tmin, tmax, ctr, radius, 0, 0);
        o.i(h);
        for (int k = 2; k < 9; k++) o.f(h ? rec[k] : 0);
        break;
      }
      case MATERIAL: {
        int kind = in.i();
        vtkm::UInt8 fin = (vtkm::UInt8)in.i();
        vec3 org = in.v(), d = in.v();
        HitRecord hrec;
        for (int k = 0; k < 9; k++) hrec[k] = in.f();
        int hm = in.i(), ht = in.i();
        HitId hid(hm, ht);
        unsigned int seed = in.next().u;
        ScatterRecord srec(0.f);
        vec3 E(0.f);
        Portal<vec3> emitted;
        emitted.p = &E, emitted.n = 1;
        if (kind == 0) LambertianWorklet(1, 0)(0, org, d, hrec, hid, srec, fin, tex, mtp, ttp, emitted);
        if (kind == 1) DiffuseLightWorklet(1, 0)(0, org, d, hrec, hid, srec, fin, tex, mtp, ttp, emitted);
        if (kind == 2) DielectricWorklet(1, 0, sc.ior, 1)(0, seed, org, d, hrec, hid, srec, fin, tex, mtp, ttp, emitted);
        o.u(fin);
        for (int k = 0; k < 9; k++) o.f(srec[k]);
        o.v(E), o.u(seed);
        break;
      }
      case DIELECTRIC: {
        vec3 d = in.v(), nn = in.v(), p = in.v();
        uint64_t lo = in.next().u, hi = in.next().u, bits = lo | (hi << 32);
        double rnd;
        memcpy(&rnd, &bits, 8);
        float ref_idx = in.f();
        HitRecord hrec = zero_hrec();
        for (int k = 0; k < 3; k++) hrec[3 + k] = nn[k], hrec[6 + k] = p[k];
        ScatterRecord srec(0.f);
        DielectricWorklet(1, 0, ref_idx, 1).scatter(vec3(0.f), d, hrec, srec, vec3(0.f), rnd);
        for (int k = 0; k < 9; k++) o.f(srec[k]);
        break;
      }
      case GENERATOR: {
        int kind = in.i(), which = in.i();
        HitRecord hrec = zero_hrec();
        for (int k = 3; k < 9; k++) hrec[k] = in.f();
        unsigned int seed = in.next().u;
        vec3 gen(0.f);
        if (kind == 0) CosineWorketletGenerateDir(1)(which, hrec, gen, seed);
        if (kind == 1)
          QuadWorkletGenerateDir(2)(which, hrec, gen, seed, Scene::in(sc.light_box_pointids, 1),
                                    Scene::in(sc.light_box_indices, 1), pts);
        if (kind == 2)
          SphereWorkletGenerateDir(3)(0, which, hrec, gen, seed, Scene::in(sc.light_sphere_pointids, 1),
                                      Scene::in(sc.light_sphere_indices, 1), pts, Scene::in(sc.sphere_radius));
        o.v(gen), o.u(seed);
        break;
      }
      case LIGHTPDF: {
        int kind = in.i();
        vtkm::UInt8 fin = (vtkm::UInt8)in.i();
        HitRecord hrec = zero_hrec();
        for (int k = 6; k < 9; k++) hrec[k] = in.f();
        vec3 gen = in.v();
        float sum = in.f();
        unsigned int seed = in.next().u;
        vec3 org(0.f), d(0.f);
        if (kind == 0)
          QuadPDFWorklet(2)(0, org, d, hrec, fin, sum, gen, seed, sc.quad_surf(), Scene::in(sc.light_box_pointids, 1),
                            Scene::in(sc.light_box_indices, 1), pts);
        if (kind == 1)
          SpherePDFWorklet(2)(0, org, d, hrec, fin, sum, gen, seed, sc.sphere_surf(),
                              Scene::in(sc.light_sphere_pointids, 1), Scene::in(sc.light_sphere_indices, 1), pts,
                              Scene::in(sc.sphere_radius));
        o.f(sum), o.u(seed);
        break;
      }
      case SCATTER: {
        vtkm::UInt8 fin = (vtkm::UInt8)in.i();
        vec3 org = in.v(), d = in.v();
        HitRecord hrec = zero_hrec();
        for (int k = 3; k < 9; k++) hrec[k] = in.f();
        ScatterRecord srec;
        for (int k = 0; k < 9; k++) srec[k] = in.f();
        float sum = in.f();
        vec3 gen = in.v();
        vec3 A(0.f), out_o = org, out_d = d; // the aliased arguments of MapperPathTracer.cxx:537, as in bounce()
        Portal<vec3> attenuation;
        attenuation.p = &A, attenuation.n = 1;
        PDFCosineWorklet(1, 0, 1, 2)(0, org, d, hrec, srec, fin, sum, gen, out_o, out_d, attenuation);
        o.u(fin), o.v(out_o), o.v(out_d), o.v(A);
        break;
      }
      case COLLECT: {
        vtkm::UInt8 st = (vtkm::UInt8)in.i();
        vec3 E(7.f), A(7.f); // 7: left alone by the worklet
        Portal<vec3> emitted, attenuation;
        emitted.p = &E, emitted.n = 1;
        attenuation.p = &A, attenuation.n = 1;
        CollectIntersecttWorklet(1, 0)(0, st, emitted, attenuation);
        o.u(st), o.v(E), o.v(A);
        break;
      }
      case CAMERA: {
        CamIn cam;
        cam.read(in);
        RayGen g = cam.raygen();
        o.v(g.nlook), o.v(g.delta_x), o.v(g.delta_y);
        break;
      }
      case RAYGEN: {
        CamIn cam;
        cam.read(in);
        vtkm::Id idx = in.i();
        unsigned int seed = in.next().u;
        float dx = 0, dy = 0, dz = 0; // FieldOut: what they hold before is not used
        vtkm::Id pixelIndex = -1;
        cam.raygen()(idx, dx, dy, dz, seed, pixelIndex);
        o.f(dx), o.f(dy), o.f(dz), o.u(seed), o.i((int32_t)pixelIndex);
        break;
      }
      case SEED_INIT: {
        o.u(vtkm::rendering::details::WangInit()(in.next().u));
        break;
      }
      case BACKWARD: {
        // all n rows are the pixels of one canvas; they share D and S
        const Word* row0 = in.p;
        const int D = row0[0].i, S = row0[1].i;
        if (D < 1 || S < 1 || kin != 2 + 8 * S * D) fprintf(stderr, "ref_stages: bad backward rows\n"), exit(2);
        const Id cs = n;
        std::vector<Vec4> cols((size_t)cs, Vec4(0.0)), sumtotl((size_t)cs, Vec4(0.f)); // :223
        std::vector<Vec4> emitted4((size_t)(cs * D)), attenuation4((size_t)(cs * D));
        for (int s = 0; s < S; s++) { // :278
          for (Id i = 0; i < cs; i++) {
            const Word* w = row0 + i * kin;
            if (w[0].i != D || w[1].i != S) fprintf(stderr, "ref_stages: backward rows differ in D or S\n"), exit(2);
            w += 2 + 8 * D * s;
            for (int d = 0; d < D; d++, w += 8) {
              emitted4[d * cs + i] = Vec4(w[0].f, w[1].f, w[2].f, w[3].f);
              attenuation4[d * cs + i] = Vec4(w[4].f, w[5].f, w[6].f, w[7].f);
            }
          }
          backward(cs, D, emitted4, attenuation4, sumtotl);
          canvas_sum(cols, sumtotl);
        }
        for (Id i = 0; i < cs; i++) o.f(cols[i][0]), o.f(cols[i][1]), o.f(cols[i][2]), o.f(cols[i][3]);
        in.p += (size_t)n * kin;
        return;
      }
      case FRAME: {
        CamIn cam;
        cam.read(in);
        int spp = in.i(), depth = in.i();
        if (n != 1 || spp < 1 || depth < 1 || cam.nx < 1 || cam.ny < 1) fprintf(stderr, "ref_stages: bad frame\n"), exit(2);
        Writer st;
        frame(sc, cam, spp, depth, o, st);
        o.w.insert(o.w.end(), st.w.begin(), st.w.end());
        break;
      }
      case BOUNCE: {
        Ray r;
        memset(&r, 0, sizeof(r)); // the buffers a first depth finds: zero
        r.org = in.v(), r.dir = in.v();
        r.seed = in.next().u;
        r.status = 1u << 3; // MapperPathTracer.cxx:283
        bounce(sc, r, o);
        break;
      }
    }
  }
}

} // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<Word> buf((size_t)sz / 4);
  if (fread(buf.data(), 4, buf.size(), f) != buf.size()) return perror("read"), 2;
  fclose(f);
  Reader in{buf.data(), buf.data() + buf.size()};
  if (in.next().u != 0x47545352u) return fprintf(stderr, "ref_stages: bad magic\n"), 2;
  int mode = in.i(), n = in.i(), kin = in.i();
  if (mode < 0 || mode > FRAME || n < 0 || (KIN[mode] >= 0 && kin != KIN[mode]) || kin < 1)
    return fprintf(stderr, "ref_stages: bad header\n"), 2;
  Scene sc;
  sc.read(in);
  if ((long)(in.end - in.p) != (long)n * kin) return fprintf(stderr, "ref_stages: bad case count\n"), 2;
  Writer o;
  o.i(mode), o.i(n), o.i(KOUT[mode]);
  run(mode, n, kin, sc, in, o);
  if (KOUT[mode] < 0) o.w[2].i = (int32_t)((o.w.size() - 3) / (size_t)(n ? n : 1));
  if (o.w.size() != 3 + (size_t)n * o.w[2].i) return fprintf(stderr, "ref_stages: internal size error\n"), 3;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return perror(argv[2]), 2;
  if (fwrite(o.w.data(), 4, o.w.size(), g) != o.w.size()) return perror("write"), 2;
  fclose(g);
  return 0;
}
