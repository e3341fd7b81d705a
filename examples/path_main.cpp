// path_main.cpp -- the path-traced modes of the reference's main.cc (parse,
// runPath, save, generateHemisphere; main.cc:54-119, 289-384, 385-427,
// 504-664) written against rtp/rendering.hpp, i.e. the reference driver on
// the MI355X path.
//
//   rtp_path [-x 128] [-y 128] [-samplecount 10] [-raydepth 5]
//            [-hemisphere [-phicount 15] [-thetacount 15]]
//            [-o output] [-raw prefix] [-variant 0] [-device 0]
//            [-rank 0 -world 1] [-dry-run] [-viewbatch N]
//            [-passes N [-preview]] [-denoise [-levels N]]
//            [-adaptive T -maxspp M [-passspp P]]
//
// Writes <o>.pnm like main.cc, or <o>-<phi>-<theta>.pnm per hemisphere view
// (generate(), "%.4f" formatting).  -raw additionally dumps the normalised
// float RGBA buffer (nx*ny*4 float32, buffer order) to <raw> (single view) or
// <raw>-<phi>-<theta>.f32 (hemisphere) for bit-exact comparisons.  -rank/-world shard the hemisphere views (view v
// goes to rank v mod world; no communication).  -dry-run prints the views
// (phi, theta, camera position as float bit patterns) and renders nothing.
// -viewbatch N: the path-traced hemisphere renders its views N at a time, each
// batch one launch (rtp::runPathViews); default: all of the rank's views,
// capped so that a batch has at most 2^31-1 pixels and under 1 GiB of output;
// 0: one launch per view (runPath).  The files are the same bytes either way.
// -passes N: the single view's -samplecount rendered in N resumable passes
// (rtp::runPathProgressive), the pass sizes as equal as possible with the
// earlier passes taking the remainder; <o>.pnm and the -raw dump are the same
// bytes as without -passes.  -preview writes <o>-pass<i>.pnm (i from 1) after
// each pass: the image of the samples so far.  With -dry-run the pass sizes
// are printed, one line, and nothing is rendered.  -passes with -hemisphere or
// -direct, or N < 1, is an error (exit code 2).
// -denoise: also writes <o>-denoised.pnm, the denoised preview of the finished
// render (rtp::ProgressiveRender::Denoised: first-hit guides and an a-trous
// filter of -levels N levels, default 5), and with -preview
// <o>-pass<i>-denoised.pnm after each pass; the render goes through the
// resumable passes (one pass without -passes) and every other file keeps its
// bytes.  -denoise with -hemisphere or -direct, or -levels outside 1..8, is an
// error (exit code 2).
// -adaptive T -maxspp M [-passspp P]: adaptive sampling of the single view
// (rtp::ProgressiveRender::Refine, include/rtp_adaptive.h).  -samplecount K is
// the uniform first pass; then adaptive passes of P samples (default K) over
// the pixels whose noise estimate exceeds T and whose count stays within M,
// until a pass selects none.  <o>.pnm (and the -raw dump) is normalised with
// each pixel's own count (rtp_normalize_counts); <o>-spp.pnm is the
// sample-count map, grey = (float)count / (float)M on all three channels
// written by rtp_write_pnm (int(255.99 * grey), no square root).  Without
// -adaptive every file keeps its bytes.  -adaptive with -hemisphere, -direct,
// -passes or -denoise, T < 0, M < 1, P < 1 or K < 1, and -maxspp or -passspp
// without -adaptive, is an error (exit code 2).
// -direct: the quad mappers' one-bounce AOVs (main.cc:623-651, generate()
// :399-420): direct.pnm, depth.pnm, normals.pnm, albedo.pnm (or
// direct-<phi>-<theta>.pnm ... per hemisphere view), all four from one launch.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include <cmath>
#include <cstdint>
#include <vector>

#include "rtp/rendering.hpp"

namespace {

struct View {
  float phi, theta;
  rtp::Vec3f pos;
};

// generateHemisphere (main.cc:504-561) with the parameters main() passes
// (:583-595): phi in [0, 1) by 1/phiCount, theta in [0, 2pi) by
// (float)(2pi)/thetaCount, radius -1078/555 around (278,278,278)/555.  Float
// variables as declared there; the phi bound is compared in double
// (phiEnd - 0.5*rPhi); cos/sin of float arguments are the float overloads.
std::vector<View> hemisphere_views(int phiCount, int thetaCount) {
  std::vector<View> v;
  const float phiBegin = 0.0, phiEnd = 1.0;
  const float thetaEnd = 2 * 3.14159265358979323846;  // 2*vtkm::Pi()
  const float rTheta = thetaEnd / (static_cast<float>(thetaCount));
  const float thetaBegin = 0;
  const float rPhi = (phiEnd - phiBegin) / float(phiCount);
  const float r = -1078 / 555.0;
  for (float phi = phiBegin; phi < (phiEnd - 0.5 * rPhi); phi += rPhi)
    for (float theta = thetaBegin; theta < thetaEnd; theta += rTheta) {
      const float px = r * std::cos(theta) * std::sin(phi);
      const float py = r * std::sin(theta) * std::sin(phi);
      const float pz = r * std::cos(phi);
      v.push_back({phi, theta, {(float)(px + 278 / 555.0), (float)(py + 278 / 555.0), (float)(pz + 278 / 555.0)}});
    }
  return v;
}

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

}  // namespace

int main(int argc, char** argv) {
  int x = 128, y = 128, s = 10, depth = 5, variant = 0, device = 0;  // main.cc:56-62 defaults
  int phiCount = 15, thetaCount = 15, rank = 0, world = 1, viewBatch = -1;
  bool hemi = false, dry = false, direct = false, preview = false, havePasses = false;
  int passes = 1, levels = 5;
  bool denoise = false, adaptive = false;
  float threshold = 0.f;
  int maxSpp = 0, passSpp = 0;
  bool haveMaxSpp = false, havePassSpp = false;
  std::string out = "output", raw;
  for (int i = 1; i < argc; i++) {
    auto next = [&](const char* flag) -> const char* {
      if (!std::strcmp(argv[i], flag) && i + 1 < argc) return argv[++i];
      return nullptr;
    };
    const char* v;
    if ((v = next("-x"))) x = std::atoi(v);
    else if ((v = next("-y"))) y = std::atoi(v);
    else if ((v = next("-samplecount"))) s = std::atoi(v);
    else if ((v = next("-raydepth"))) depth = std::atoi(v);
    else if ((v = next("-o"))) out = v;
    else if ((v = next("-raw"))) raw = v;
    else if ((v = next("-variant"))) variant = std::atoi(v);
    else if ((v = next("-device"))) device = std::atoi(v);
    else if ((v = next("-phicount"))) phiCount = std::atoi(v);
    else if ((v = next("-thetacount"))) thetaCount = std::atoi(v);
    else if ((v = next("-rank"))) rank = std::atoi(v);
    else if ((v = next("-world"))) world = std::atoi(v);
    else if ((v = next("-viewbatch"))) viewBatch = std::atoi(v);
    else if ((v = next("-passes"))) passes = std::atoi(v), havePasses = true;
    else if ((v = next("-levels"))) levels = std::atoi(v);
    else if ((v = next("-adaptive"))) threshold = (float)std::atof(v), adaptive = true;
    else if ((v = next("-maxspp"))) maxSpp = std::atoi(v), haveMaxSpp = true;
    else if ((v = next("-passspp"))) passSpp = std::atoi(v), havePassSpp = true;
    else if (!std::strcmp(argv[i], "-denoise")) denoise = true;
    else if (!std::strcmp(argv[i], "-preview")) preview = true;
    else if (!std::strcmp(argv[i], "-hemisphere")) hemi = true;
    else if (!std::strcmp(argv[i], "-dry-run")) dry = true;
    else if (!std::strcmp(argv[i], "-direct")) direct = true;
  }
  if (world < 1 || rank < 0 || rank >= world || phiCount < 1 || thetaCount < 1) {
    std::cerr << "rtp_path: bad -rank/-world/-phicount/-thetacount" << std::endl;
    return 2;
  }
  if (havePasses && (passes < 1 || hemi || direct)) {
    std::cerr << "rtp_path: -passes needs N >= 1 and renders the single view (no -hemisphere, no -direct)"
              << std::endl;
    return 2;
  }
  if (denoise && (hemi || direct || levels < 1 || levels > 8)) {
    std::cerr << "rtp_path: -denoise renders the single view (no -hemisphere, no -direct) with -levels 1..8"
              << std::endl;
    return 2;
  }
  if (!adaptive && (haveMaxSpp || havePassSpp)) {
    std::cerr << "rtp_path: -maxspp and -passspp belong to -adaptive T" << std::endl;
    return 2;
  }
  if (adaptive && !havePassSpp) passSpp = s;
  if (adaptive && (hemi || direct || havePasses || denoise || !(threshold >= 0.f) || maxSpp < 1 || passSpp < 1 || s < 1)) {
    std::cerr << "rtp_path: -adaptive T -maxspp M [-passspp P] renders the single view (no -hemisphere, -direct, "
                 "-passes or -denoise) with T >= 0, M >= 1, P >= 1 and -samplecount >= 1"
              << std::endl;
    return 2;
  }
  if (havePasses && dry) {
    if (s < 0) return 2;
    const std::vector<int> sizes = rtp::SplitPasses(s, passes);
    for (size_t i = 0; i < sizes.size(); i++) std::printf(i ? " %d" : "%d", sizes[i]);
    std::printf("\n");
    return 0;
  }
  std::vector<View> views;
  if (hemi) {
    const std::vector<View> all = hemisphere_views(phiCount, thetaCount);
    for (size_t k = rank; k < all.size(); k += world) views.push_back(all[k]);
  }
  if (dry) {
    for (const View& w : views)
      std::printf("%.4f-%.4f %08x %08x %08x\n", w.phi, w.theta, bits(w.pos[0]), bits(w.pos[1]), bits(w.pos[2]));
    return 0;
  }
  try {
    const auto t0 = std::chrono::steady_clock::now();
    rtp::CornellBox cb;
    cb.variant = variant;
    cb.buildDataSet();
    rtp::rendering::CanvasRayTracer canvas(x, y);
    rtp::rendering::Camera cam = rtp::DefaultCamera();
    auto dev = std::make_shared<rtp::Device>(device);
    auto save = [&](const std::string& suffix) {  // the canvas as <o><suffix>.pnm (and the -raw dump)
      rtp::SavePNM(out + suffix + ".pnm", canvas);
      if (!raw.empty()) {
        const std::string fn = suffix.empty() ? raw : raw + suffix + ".f32";
        FILE* f = std::fopen(fn.c_str(), "wb");
        if (!f) throw rtp::ErrorBadValue("cannot open " + fn);
        const auto& c = canvas.GetColorBuffer();
        std::fwrite(c.data(), sizeof(rtp::Vec4f), c.size(), f);
        std::fclose(f);
      }
    };
    auto render = [&](const std::string& suffix) {  // generate() / the default branch of main()
      if (direct) {  // runRay + depth, runNorms, runAlbedo (main.cc:399-420, 625-650)
        const rtp::rendering::DirectBuffers b = rtp::RunDirect(x, y, cam, cb, dev);
        rtp::SavePNM("direct" + suffix + ".pnm", b.color, x, y);
        rtp::SaveDepthPNM("depth" + suffix + ".pnm", b.depth, x, y);
        rtp::SavePNM("normals" + suffix + ".pnm", b.normals, x, y);
        rtp::SavePNM("albedo" + suffix + ".pnm", b.albedo, x, y);
        return;
      }
      if (adaptive) {
        rtp::rendering::MapperPathTracer mapper(s, depth, cb.matIdx, cb.texIdx, cb.matType, cb.texType, cb.tex, dev);
        mapper.SetLights(cb.lightQuad, cb.lightSphere, cb.ior);
        rtp::ProgressiveRender r(mapper.UploadScene(cb.ds.GetCellSet(), cb.coord), cam, x, y, depth);
        r.Step(s);
        while (r.Refine(passSpp, threshold, maxSpp) > 0) {
        }
        r.Canvas(canvas);
        std::vector<rtp::Vec4f> map(r.Counts().size());
        for (size_t i = 0; i < map.size(); i++) {
          const float g = (float)r.Counts()[i] / (float)maxSpp;
          map[i] = rtp::Vec4f{g, g, g, 0.f};
        }
        rtp::SavePNM(out + suffix + "-spp.pnm", map, x, y);
      } else if (havePasses || denoise) {
        rtp_denoise_params prm = rtp::ProgressiveRender::DefaultDenoiseParams();
        prm.levels = levels;
        rtp::runPathProgressiveRender(x, y, s, depth, canvas, cam, cb, passes, dev,
                                      [&](int i, rtp::ProgressiveRender& r) {
          const std::string pass = out + "-pass" + std::to_string(i + 1);
          if (preview) rtp::SavePNM(pass + ".pnm", canvas);
          if (preview && denoise) rtp::SavePNM(pass + "-denoised.pnm", r.Denoised(prm), x, y);
          if (denoise && i + 1 == passes) rtp::SavePNM(out + suffix + "-denoised.pnm", r.Denoised(prm), x, y);
        });
      } else {
        rtp::runPath(x, y, s, depth, canvas, cam, cb, dev);
      }
      save(suffix);
    };
    auto suffix_of = [](const View& w) {
      char suffix[64];
      std::snprintf(suffix, sizeof(suffix), "-%.4f-%.4f", w.phi, w.theta);
      return std::string(suffix);
    };
    if (hemi) {
      // generateHemisphere's own camera: near plane 1, not main()'s 0.1
      // (main.cc:519 `SetClippingRange(01.f, 5.f)`; it moves the depth AOV)
      cam.SetClippingRange(1.0f, 5.f);
      // a batch of views per launch: at most 2^31-1 pixels and under 1 GiB of float4 output
      const int64_t npv = (int64_t)x * y;
      const int64_t cap = npv > 0 ? std::max<int64_t>(1, std::min<int64_t>(INT32_MAX / npv, ((1ll << 30) - 1) / (16 * npv))) : 1;
      const int64_t batch = viewBatch < 0 ? cap : std::min<int64_t>(viewBatch, cap);
      if (direct || batch == 0) {
        for (const View& w : views) {
          cam.SetPosition(w.pos);
          render(suffix_of(w));
        }
      } else {
        for (size_t b = 0; b < views.size(); b += (size_t)batch) {
          const size_t e = std::min(views.size(), b + (size_t)batch);
          std::vector<rtp::rendering::Camera> cams;
          for (size_t k = b; k < e; k++) {
            cam.SetPosition(views[k].pos);
            cams.push_back(cam);
          }
          const std::vector<rtp::Vec4f> cols = rtp::runPathViews(x, y, s, depth, cams, cb, dev);
          for (size_t k = b; k < e; k++) {
            std::copy(cols.begin() + (k - b) * npv, cols.begin() + (k - b + 1) * npv, canvas.GetColorBuffer().begin());
            save(suffix_of(views[k]));
          }
        }
      }
    } else {
      render("");
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << " Elapsed time         = " << el << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "rtp_path: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
