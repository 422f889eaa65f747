// Main.cpp — the RayTracer application on the GPU path.
// Same flow as reference source/Main.cpp:153-235 (parse, build the Cornell-box
// scene, construct the Renderer with or without a photon map, fill the background,
// render, save the PPM, print the total time); the scene script itself lives in
// ScenePresets.cpp so that tests and bench.py build the identical scene.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <string>

#include "CommandLine.h"
#include "Image.cpp"
#include "Renderer.cpp"
#include "ScenePresets.h"

int main(int argc, char** argv) {
  CommandLine args;
  try {
    args.parse(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    args.printUsage(argv[0]);
    return 1;
  }
  const auto begin = std::chrono::steady_clock::now();
  GpuSettings::get().device = static_cast<int>(args.gpu());
  GpuSettings::get().seed = static_cast<unsigned>(args.seed());
  GpuSettings::get().accel = args.accel() ? RT_ACCEL_BRUTE : RT_ACCEL_BVH;
  GpuSettings::get().progress = static_cast<unsigned>(args.progress());
  GpuSettings::get().tune = args.tune();
  GpuSettings::get().denoise = args.denoise() != 0;
  GpuSettings::get().aov = args.aov() != 0;
  GpuSettings::get().adaptive = args.adaptive();
  GpuSettings::get().pass = static_cast<unsigned>(args.pass());
  GpuSettings::get().ao = static_cast<unsigned>(args.ao());
  GpuSettings::get().aoDistance = args.aoDist();
  GpuSettings::get().aperture = args.aperture();
  GpuSettings::get().focus = args.focus();
  // -gpus N: devices gpu..gpu+N-1; -devices a,b,c: an explicit list (may repeat a device:
  // rehearsal of the N-rank flow on one GPU)
  if (!args.devices().empty()) {
    size_t pos = 0;
    const std::string& d = args.devices();
    while (pos <= d.size()) {
      const size_t c = d.find(',', pos);
      GpuSettings::get().devices.push_back(std::atoi(d.substr(pos, c == std::string::npos ? c : c - pos).c_str()));
      if (c == std::string::npos) break;
      pos = c + 1;
    }
  } else if (args.gpus() > 1) {
    for (size_t i = 0; i < args.gpus(); ++i) GpuSettings::get().devices.push_back(static_cast<int>(args.gpu() + i));
  }

  if ((args.denoise() || args.aov()) && GpuSettings::get().devices.size() > 1) {
    std::cerr << "error: -denoise / -aov run on one GPU only (not with -gpus > 1)" << std::endl;
    return 1;
  }
  if (args.ao() && GpuSettings::get().devices.size() > 1) {
    std::cerr << "error: -ao runs on one GPU only (not with -gpus > 1)" << std::endl;
    return 1;
  }
  // (before the frame is rendered: rt_render_ao would refuse these after it)
  if (args.ao() > RT_AO_MAX_RAYS) {  // (a negative value wraps far above)
    std::cerr << "error: -ao must be in 0.." << RT_AO_MAX_RAYS << " (0 = off)" << std::endl;
    return 1;
  }
  if (!(args.aoDist() >= 0.) || !(args.aoDist() < 3.0e38)) {
    std::cerr << "error: -aodist must be a finite distance >= 0 (0 = unbounded)" << std::endl;
    return 1;
  }
  if (!(args.aperture() >= 0.) || !(args.aperture() < 3.0e38)) {
    std::cerr << "error: -aperture must be a finite lens radius >= 0 (0 = pinhole)" << std::endl;
    return 1;
  }
  if (args.aperture() > 0.) {
    if (!(args.focus() > 0.) || !(args.focus() < 3.0e38)) {
      std::cerr << "error: -aperture needs -focus, a finite distance > 0" << std::endl;
      return 1;
    }
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0.) {
      std::cerr << "error: -aperture runs on one GPU, without -p and without -adaptive" << std::endl;
      return 1;
    }
  }
  if (!args.shutter().empty()) {
    // -shutter dx,dy,dz: three finite numbers and nothing else
    double m[3];
    char rest;
    if (std::sscanf(args.shutter().c_str(), "%lf,%lf,%lf%c", &m[0], &m[1], &m[2], &rest) != 3 || !(std::fabs(m[0]) < 3.0e38) ||
        !(std::fabs(m[1]) < 3.0e38) || !(std::fabs(m[2]) < 3.0e38)) {
      std::cerr << "error: -shutter must be dx,dy,dz, three finite numbers (the camera's move while the shutter is open)" << std::endl;
      return 1;
    }
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0.) {
      std::cerr << "error: -shutter runs on one GPU, without -p and without -adaptive" << std::endl;
      return 1;
    }
    GpuSettings::get().shutter = true;
    for (int k = 0; k < 3; ++k) GpuSettings::get().shutterMove[k] = static_cast<float>(m[k]);
  }
  if (!args.lights().empty()) {
    // -lights each | M0,M1,...: one group per light, or groups by masks (decimal, 0x.. or 0..), and nothing else
    if (args.lights() == "each") {
      GpuSettings::get().lightsEach = true;
    } else {
      const char* s = args.lights().c_str();
      for (;;) {
        char* end = nullptr;
        const unsigned long long m = std::strtoull(s, &end, 0);
        if (end == s || *s == '-' || *s == '+' || m > 0xffffffffull || (*end != ',' && *end != '\0')) {
          std::cerr << "error: -lights must be `each` or M0,M1,...: masks of lights (bit l: light l is lit)" << std::endl;
          return 1;
        }
        GpuSettings::get().lightMasks.push_back(static_cast<unsigned>(m));
        if (*end == '\0') break;
        s = end + 1;
      }
      if (GpuSettings::get().lightMasks.size() > RT_LIGHT_GROUPS_MAX) {
        std::cerr << "error: -lights takes at most " << RT_LIGHT_GROUPS_MAX << " groups per frame" << std::endl;
        return 1;
      }
    }
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0. || !args.shutter().empty() ||
        args.aperture() > 0.) {
      std::cerr << "error: -lights runs on one GPU, without -p, -adaptive, -shutter and -aperture" << std::endl;
      return 1;
    }
  }
  if (args.lightPick() != 0) {
    // -lightpick M: M = 1..RT_PICK_SLOTS_MAX sampled lights per path vertex, and nothing else
    if (args.lightPick() < 1 || args.lightPick() > RT_PICK_SLOTS_MAX) {
      std::cerr << "error: -lightpick must be 1.." << RT_PICK_SLOTS_MAX << " light samples per path vertex" << std::endl;
      return 1;
    }
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0. || !args.shutter().empty() ||
        args.aperture() > 0. || !args.lights().empty()) {
      std::cerr << "error: -lightpick runs on one GPU, without -p, -adaptive, -shutter, -aperture and -lights" << std::endl;
      return 1;
    }
    GpuSettings::get().lightPick = static_cast<unsigned>(args.lightPick());
  }
  if (args.vcolors() != 0) {
    // -vcolors 1: the frame with the per-vertex colours of the scene's COFF meshes, and nothing else
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0. || !args.shutter().empty() ||
        args.aperture() > 0. || !args.lights().empty() || args.lightPick() != 0) {
      std::cerr << "error: -vcolors runs on one GPU, without -p, -adaptive, -shutter, -aperture, -lights and -lightpick" << std::endl;
      return 1;
    }
    GpuSettings::get().vcolors = true;
  }
  if (args.matmaps() != 0) {
    // -matmaps 1: the textured frame with f0 and (kd, alpha) from the images beside the scene's STOFF meshes too; it
    // needs -textures 1 and composes with what that composes with
    if (args.textures() == 0) {
      std::cerr << "error: -matmaps needs -textures 1" << std::endl;
      return 1;
    }
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0. || !args.shutter().empty() ||
        args.aperture() > 0. || !args.lights().empty() || args.lightPick() != 0 || args.vcolors() != 0) {
      std::cerr << "error: -matmaps runs on one GPU, without -p, -adaptive, -shutter, -aperture, -lights, -lightpick and -vcolors" << std::endl;
      return 1;
    }
    GpuSettings::get().matmaps = true;
  }
  if (args.normalmaps() != 0) {
    // -normalmaps 1: the textured frame, with or without -matmaps 1, with the shading normals turned by the normal maps
    // beside the scene's STOFF meshes; it needs -textures 1 and composes with what that composes with
    if (args.textures() == 0) {
      std::cerr << "error: -normalmaps needs -textures 1" << std::endl;
      return 1;
    }
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0. || !args.shutter().empty() ||
        args.aperture() > 0. || !args.lights().empty() || args.lightPick() != 0 || args.vcolors() != 0) {
      std::cerr << "error: -normalmaps runs on one GPU, without -p, -adaptive, -shutter, -aperture, -lights, -lightpick and -vcolors" << std::endl;
      return 1;
    }
    GpuSettings::get().normalmaps = true;
  }
  if (args.textures() != 0) {
    // -textures 1: the frame with the images beside the scene's STOFF meshes as albedo, and nothing else
    if (GpuSettings::get().devices.size() > 1 || args.numPhotons() > 0 || args.adaptive() >= 0. || !args.shutter().empty() ||
        args.aperture() > 0. || !args.lights().empty() || args.lightPick() != 0 || args.vcolors() != 0) {
      std::cerr << "error: -textures runs on one GPU, without -p, -adaptive, -shutter, -aperture, -lights, -lightpick and -vcolors" << std::endl;
      return 1;
    }
    GpuSettings::get().textures = true;
  }
  if (args.adaptive() >= 0.) {
    if (GpuSettings::get().devices.size() > 1) {
      std::cerr << "error: -adaptive runs on one GPU only (not with -gpus > 1)" << std::endl;
      return 1;
    }
    if (args.pass() == 0 || args.numRays() % args.pass() != 0) {
      std::cerr << "error: -N (" << args.numRays() << ") must be a multiple of -pass (" << args.pass() << ")" << std::endl;
      return 1;
    }
  }
  try {
    Image image(args.width(), args.height());
    Scene scene = rtpreset::buildCornellScene(args.scene(), args.meshDir(), args.width(), args.height());

    RayTracer rayTracer;
    Renderer renderer;
    if (args.numPhotons() > 0) {
      renderer = Renderer(scene, args.numRays(), args.mode(), rayTracer, args.numPhotons(), args.k());
      renderer.savePhotonMap();
    } else {
      renderer = Renderer(scene, args.numRays(), args.mode(), rayTracer);
    }
    image.fillBackground();
    renderer.render(image);
    image.savePPM(args.outputFilename());
    // -denoise / -aov / -ao: <stem>_denoised.ppm, <stem>_albedo.ppm, <stem>_normal.ppm, <stem>_ao.ppm next to the output
    const std::string& of = args.outputFilename();
    const std::string stem = of.size() > 4 && of.compare(of.size() - 4, 4, ".ppm") == 0 ? of.substr(0, of.size() - 4) : of;
    if (args.denoise()) renderer.denoised().savePPM(stem + "_denoised.ppm");
    if (args.aov()) renderer.albedo().savePPM(stem + "_albedo.ppm"), renderer.normal().savePPM(stem + "_normal.ppm");
    if (args.adaptive() >= 0.) renderer.sppMap().savePPM(stem + "_spp.ppm");
    if (args.ao()) renderer.ao().savePPM(stem + "_ao.ppm");
    for (size_t g = 0; g < renderer.lightGroups().size(); ++g) renderer.lightGroups()[g].savePPM(stem + "_g" + std::to_string(g) + ".ppm");

    const rt_stats& st = renderer.lastStats();
    const double rays = static_cast<double>(st.rays_closest + st.rays_shadow);
    std::cout << "GPU: " << rays / 1e6 << " Mrays in " << st.kernel_ms << " ms ("
              << (st.kernel_ms > 0 ? rays / st.kernel_ms / 1e3 : 0.0) << " Mrays/s)" << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 1;
  }
  const auto end = std::chrono::steady_clock::now();
  std::cout << "Total time is " << std::chrono::duration_cast<std::chrono::seconds>(end - begin).count() << "[s]"
            << std::endl;
  return 0;
}
