// GpuSession.h — RAII owner of an rt_ctx for the host classes.  Every host class
// that has to EVALUATE something (Renderer, RayTracer, PhotonMap, kdtree) goes
// through one of these; construction throws std::runtime_error with the C ABI's
// message when the HIP library cannot reach a gfx950 device — there is no host
// implementation to fall back to.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "SceneFlatten.h"
#include "rt_amd.h"

class GpuSession {
 public:
  GpuSession() : m_ctx(nullptr) {}
  explicit GpuSession(const Scene& scene, int device = 0) : m_flat(scene), m_ctx(nullptr) { open(device); }
  ~GpuSession() { close(); }
  GpuSession(const GpuSession&) = delete;
  GpuSession& operator=(const GpuSession&) = delete;

  void reset(const Scene& scene, int device = 0) {
    close();
    m_flat.assign(scene);
    open(device);
  }
  void close() {
    if (m_ctx) rt_destroy(m_ctx);
    m_ctx = nullptr;
  }
  rt_ctx* ctx() const { return m_ctx; }
  const FlatScene& flat() const { return m_flat; }
  bool valid() const { return m_ctx != nullptr; }

  static void check(int rc, const char* what) {
    if (rc != RT_OK) throw std::runtime_error(std::string(what) + ": " + rt_last_error());
  }

 private:
  void open(int device) {
    rt_options opt = {};
    opt.device = device;
    check(rt_create(&m_flat.desc, &opt, &m_ctx), "rt_create");
  }
  FlatScene m_flat;
  rt_ctx* m_ctx;
};

// N devices behind one Renderer::render (rt_group: replicated scene, tile-sharded frame,
// owned tiles to devices[0] over xGMI)
class GpuGroupSession {
 public:
  GpuGroupSession(const Scene& scene, const std::vector<int>& devices) : m_flat(scene), m_group(nullptr) {
    std::vector<int32_t> d(devices.begin(), devices.end());
    GpuSession::check(rt_group_create(&m_flat.desc, d.data(), static_cast<uint32_t>(d.size()), nullptr, &m_group),
                      "rt_group_create");
  }
  ~GpuGroupSession() {
    if (m_group) rt_group_destroy(m_group);
  }
  GpuGroupSession(const GpuGroupSession&) = delete;
  GpuGroupSession& operator=(const GpuGroupSession&) = delete;
  rt_group* group() const { return m_group; }
  rt_ctx* ctx0() const { return rt_group_ctx(m_group, 0); }

 private:
  FlatScene m_flat;
  rt_group* m_group;
};

// process-wide settings the reference has no place for (set by Main.cpp's extra
// flags; defaults reproduce `./RayTracer` without them)
struct GpuSettings {
  int device = 0;
  unsigned seed = 1;
  unsigned accel = RT_ACCEL_BVH;
  unsigned progress = 0;  // samples per launch / per update.ppm (0 = whole frame at once)
  double tune = 0.;       // seconds of measured-cost BVH tuning before the frame (rt_bvh_tune; 0 = none)
  bool denoise = false;   // also the a-trous-filtered frame (Renderer::denoised(); single device only)
  bool aov = false;       // also the first-hit AOV means (Renderer::albedo() / normal(); single device only)
  double adaptive = -1.;  // >= 0: adaptive sampling with this threshold (rt_render_adaptive; single device only)
  unsigned pass = 16;     // samples per adaptive pass (the frame's spp is the per-pixel maximum, a multiple of it)
  unsigned ao = 0;        // > 0: also the ambient occlusion of this many rays per primary hit (Renderer::ao(); single device only)
  double aoDistance = 0.; // ... with occluders up to this distance in scene units (0 = unbounded)
  double aperture = 0.;   // > 0: the frame through a thin lens of this radius (rt_render_lens; single device, no photons, not adaptive)
  double focus = 0.;      // ... focused at this distance along the optical axis
  bool shutter = false;   // the frame under an open shutter (rt_render_shutter; single device, no photons, not adaptive) ...
  float shutterMove[3] = {0.f, 0.f, 0.f};  // ... while the camera translates by this vector; -aperture / -focus put the lens on it
  bool lightsEach = false;            // also one frame per light (rt_render_lights: Renderer::lightGroups(); single device, plain frames only) ...
  std::vector<unsigned> lightMasks;   // ... or one per mask of lights (bit l: light l is lit); at most RT_LIGHT_GROUPS_MAX groups
  bool vcolors = false;               // shade with the meshes' per-vertex colours where any mesh has them (rt_render_colors; single device, plain frames only)
  bool textures = false;              // shade the meshes that have texture coordinates and a <stem>.ppm beside their .off with that image (rt_render_textured; single device, plain frames only)
  bool matmaps = false;               // with textures: also f0 from <stem>_f0.ppm and (kd, alpha) from <stem>_kda.ppm where they lie beside the .off (rt_render_material)
  bool normalmaps = false;            // with textures: also the shading normal turned by <stem>_n.ppm where it lies beside the .off (rt_render_normal_mapped; with or without matmaps)
  unsigned lightPick = 0;             // > 0: the frame with this many sampled lights per path vertex (rt_render_pick; single device, plain frames only)
  std::vector<int> devices;  // more than one entry: Renderer::render tile-shards the frame over them (rt_group)
  static GpuSettings& get() {
    static GpuSettings s;
    return s;
  }
};
