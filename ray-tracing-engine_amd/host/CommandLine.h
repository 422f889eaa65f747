// CommandLine.h — argument parser of the RayTracer application.
// Flag set, defaults and error behaviour of reference source/CommandLine.h:8-102
// (-w/-width -h/-height -o/-output -N/-n/-numRays -m/-mode -p/-numPhotons -k -help;
// 380x270, N=16, mode 0, no photons, k=5, output.ppm; a trailing flag without a
// value is "Missing argument" unless it is -help; unknown flags throw; a mode other
// than 0/1 silently becomes 0), plus build-defined extensions the reference has
// no equivalent for: -scene, -meshdir, -seed, -gpu, -gpus, -devices, -accel,
// -progress, -tune, -denoise, -aov, -adaptive, -pass, -ao, -aodist, -aperture, -focus, -shutter, -lights, -lightpick, -vcolors, -textures,
// -matmaps, -normalmaps.
#pragma once

#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>

using namespace std;  // the reference header leaks this; user code relies on it

class CommandLine {
 public:
  CommandLine()
      : m_width(380), m_height(270), m_numRays(16), m_mode(0), m_numPhotons(0), m_k(5), m_seed(1), m_gpu(0),
        m_accel(0), m_progress(0), m_gpus(1), m_denoise(0), m_aov(0), m_pass(16), m_ao(0), m_vcolors(0), m_textures(0), m_matmaps(0), m_normalmaps(0), m_lightPick(0), m_tune(0.), m_adaptive(-1.), m_aoDist(0.), m_aperture(0.), m_focus(0.), m_outputFilename("output.ppm"), m_scene("cubes"), m_meshDir("../meshes") {}
  virtual ~CommandLine() {}

  size_t width() const { return m_width; }
  size_t height() const { return m_height; }
  size_t numRays() const { return m_numRays; }
  size_t mode() const { return m_mode; }
  size_t numPhotons() const { return m_numPhotons; }
  size_t k() const { return m_k; }
  const std::string& outputFilename() const { return m_outputFilename; }
  // extensions
  size_t seed() const { return m_seed; }
  size_t gpu() const { return m_gpu; }
  size_t accel() const { return m_accel; }
  size_t progress() const { return m_progress; }
  double tune() const { return m_tune; }
  size_t denoise() const { return m_denoise; }
  size_t aov() const { return m_aov; }
  double adaptive() const { return m_adaptive; }
  size_t pass() const { return m_pass; }
  size_t ao() const { return m_ao; }
  double aoDist() const { return m_aoDist; }
  double aperture() const { return m_aperture; }
  double focus() const { return m_focus; }
  const std::string& shutter() const { return m_shutter; }
  const std::string& lights() const { return m_lights; }
  int lightPick() const { return m_lightPick; }
  size_t vcolors() const { return m_vcolors; }
  size_t textures() const { return m_textures; }
  size_t matmaps() const { return m_matmaps; }
  size_t normalmaps() const { return m_normalmaps; }
  size_t gpus() const { return m_gpus; }
  const std::string& devices() const { return m_devices; }
  const std::string& scene() const { return m_scene; }
  const std::string& meshDir() const { return m_meshDir; }

  void printUsage(const char* command) {
    std::cerr << "USAGE: " << command
              << " [-w/-width <image width>][-h/-height <image height>][-o/-output <outputfilename>]"
                 "[-N/-n/-numRays <number of rays per pixel>][-m/-mode <mode (0 for Ray tracing, 1 for Path "
                 "tracing)>][-p/-numPhotons <number of photons for a photon map. If defined, photon map-based "
                 "rendering is used.>][-k <number of neighbours in photon mapping. Use only with -p/-numPhotons>]"
                 "[-scene <cubes|lowres|hires|stress|file:NAME.off>][-meshdir <dir with .off files>]"
                 "[-seed <per-pixel RNG stream key>][-gpu <HIP device>][-gpus <N: tile-shard the frame over devices gpu..gpu+N-1>]"
                 "[-devices <a,b,c: explicit device list for -gpus>][-accel <0 BVH | 1 brute force>]"
                 "[-progress <samples per update.ppm; 1 = after every pass like the reference, 0 = once>]"
                 "[-tune <seconds: tune the BVH on probe frames of this camera before rendering (rt_bvh_tune); 0 = off>]"
                 "[-denoise <1: also write <output stem>_denoised.ppm (a-trous filter guided by the first-hit AOVs)>]"
                 "[-aov <1: also write <output stem>_albedo.ppm and <output stem>_normal.ppm>]"
                 "[-adaptive <threshold: adaptive sampling, passes of -pass samples up to -N per pixel; also writes "
                 "<output stem>_spp.ppm>][-pass <samples per adaptive pass (default 16; -N must be a multiple)>]"
                 "[-ao <N: also write <output stem>_ao.ppm, the ambient occlusion of N rays per primary hit (1..256)>]"
                 "[-aodist <D: occluders count up to distance D in scene units (default 0 = unbounded)>]"
                 "[-aperture <A: render through a thin lens of radius A in scene units (depth of field; default 0 = pinhole)>]"
                 "[-focus <D: distance of the plane of focus along the optical axis; required with -aperture>]"
                 "[-shutter <dx,dy,dz: the camera translates by this vector while the shutter is open (camera motion blur)>]"
                 "[-lights <each | M0,M1,...: also write <output stem>_g<k>.ppm, the frame with only one light lit (each) or "
                 "only the lights of mask Mk lit (bit l: light l), from one launch; at most 4 groups>]"
                 "[-lightpick <M: sample M = 1..3 of the scene's lights per path vertex by their power instead of all of them (scenes of many lights)>]"
                 "[-vcolors <1: shade with the per-vertex colours of COFF meshes (meshes without colours keep their material's albedo)>]"
                 "[-textures <1: shade every mesh that has texture coordinates (STOFF) and a <mesh stem>.ppm beside its .off with that image as albedo, bilinear and repeating>]"
                 "[-matmaps <1: with -textures 1, also take f0 from <mesh stem>_f0.ppm (rgb) and kd and alpha from <mesh stem>_kda.ppm (r, g) where they lie beside the .off>]"
                 "[-normalmaps <1: with -textures 1, also turn the shading normal by the tangent-space normal map <mesh stem>_n.ppm (rgb = (n + 1) / 2) where it lies beside the .off>]"
              << std::endl;
  }

  void parse(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
      const std::string flag = argv[i];
      if (i == argc - 1) {
        if (flag == "-help") {
          printUsage(argv[0]);
          std::exit(0);
        }
        throw std::runtime_error("Missing argument");
      }
      const char* value = argv[++i];
      if (flag == "-w" || flag == "-width") m_width = std::atoi(value);
      else if (flag == "-h" || flag == "-height") m_height = std::atoi(value);
      else if (flag == "-o" || flag == "-output") m_outputFilename = value;
      else if (flag == "-N" || flag == "-n" || flag == "-numRays") m_numRays = std::atoi(value);
      else if (flag == "-m" || flag == "-mode") m_mode = std::atoi(value);
      else if (flag == "-p" || flag == "-numPhotons") m_numPhotons = std::atoi(value);
      else if (flag == "-k") m_k = std::atoi(value);
      else if (flag == "-scene") m_scene = value;
      else if (flag == "-meshdir") m_meshDir = value;
      else if (flag == "-seed") m_seed = std::atoi(value);
      else if (flag == "-gpu") m_gpu = std::atoi(value);
      else if (flag == "-gpus") m_gpus = std::atoi(value);
      else if (flag == "-devices") m_devices = value;
      else if (flag == "-accel") m_accel = std::atoi(value);
      else if (flag == "-progress") m_progress = std::atoi(value);
      else if (flag == "-tune") m_tune = std::atof(value);
      else if (flag == "-denoise") m_denoise = std::atoi(value);
      else if (flag == "-aov") m_aov = std::atoi(value);
      else if (flag == "-adaptive") m_adaptive = std::atof(value);
      else if (flag == "-pass") m_pass = std::atoi(value);
      else if (flag == "-ao") m_ao = std::atoi(value);
      else if (flag == "-aodist") m_aoDist = std::atof(value);
      else if (flag == "-aperture") m_aperture = std::atof(value);
      else if (flag == "-focus") m_focus = std::atof(value);
      else if (flag == "-shutter") m_shutter = value;
      else if (flag == "-lights") m_lights = value;
      else if (flag == "-lightpick") m_lightPick = std::atoi(value);
      else if (flag == "-vcolors") m_vcolors = std::atoi(value);
      else if (flag == "-textures") m_textures = std::atoi(value);
      else if (flag == "-matmaps") m_matmaps = std::atoi(value);
      else if (flag == "-normalmaps") m_normalmaps = std::atoi(value);
      else throw std::runtime_error("Unknown argument <" + flag + ">");
    }
    if (m_mode != 0 && m_mode != 1) m_mode = 0;
    cout << "#########################" << endl;
    cout << "Mode: " << (m_mode == 1 ? "Path tracing" : "Ray tracing") << endl;
    cout << "Photon map ";
    if (m_numPhotons == 0) cout << "OFF" << endl;
    else cout << "ON with " << m_numPhotons << " photons. Number of searched neighbours equals " << m_k << endl;
    cout << "width: " << m_width << ", height: " << m_height << endl;
    cout << "Output image filename: " << m_outputFilename << endl;
    cout << "#########################" << endl << endl;
  }

 private:
  size_t m_width, m_height, m_numRays, m_mode, m_numPhotons, m_k, m_seed, m_gpu, m_accel, m_progress, m_gpus, m_denoise, m_aov, m_pass, m_ao, m_vcolors, m_textures, m_matmaps, m_normalmaps;
  int m_lightPick;
  double m_tune, m_adaptive, m_aoDist, m_aperture, m_focus;
  std::string m_outputFilename, m_scene, m_meshDir, m_devices, m_shutter, m_lights;
};
