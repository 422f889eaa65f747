// Renderer.cpp — see Renderer.h.  Header-style (include-guarded) because the
// reference application #includes "Renderer.cpp" from Main.cpp (source/Main.cpp:21).
#pragma once
#include "Renderer.h"

#include <algorithm>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Texture.h"

// does any mesh carry per-vertex colours (a COFF file)?
inline bool sceneHasVertexColors(const Scene& scene) {
  for (const Mesh& m : scene.meshes())
    if (!m.vertexColors().empty() && m.vertexColors().size() == m.vertexPositions().size()) return true;
  return false;
}

// The image -textures gives a mesh: <stem>.ppm beside the .off it was loaded from, if the mesh has texture coordinates
// and that file can be opened ("" otherwise).
// suffix: "" for the albedo image; "_f0" and "_kda" name the images -matmaps binds (<stem>_f0.ppm, <stem>_kda.ppm), "_n"
// the one -normalmaps binds (<stem>_n.ppm).
inline std::string meshTextureFile(const Mesh& m, const std::string& suffix = "") {
  if (m.vertexUVs().empty() || m.vertexUVs().size() != 2 * m.vertexPositions().size()) return "";
  const std::string& off = m.sourceFile();
  const size_t dot = off.rfind('.'), slash = off.find_last_of("/\\");
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return "";
  const std::string ppm = off.substr(0, dot) + suffix + ".ppm";
  return std::ifstream(ppm.c_str()) ? ppm : "";
}

inline bool sceneHasTextures(const Scene& scene) {
  for (const Mesh& m : scene.meshes())
    if (!meshTextureFile(m).empty()) return true;
  return false;
}

inline void Renderer::render(Image& image) {
  const uint32_t w = static_cast<uint32_t>(image.width()), h = static_cast<uint32_t>(image.height());
  // one device, or (GpuSettings::devices, `-gpus N`) the frame tile-sharded over N of them
  const std::vector<int>& devs = GpuSettings::get().devices;
  const bool multi = devs.size() > 1;
  std::unique_ptr<GpuSession> single;
  std::unique_ptr<GpuGroupSession> many;
  if (multi) many.reset(new GpuGroupSession(m_scene, devs));
  else single.reset(new GpuSession(m_scene, devs.size() == 1 ? devs[0] : GpuSettings::get().device));
  rt_ctx* ctx0 = multi ? many->ctx0() : single->ctx();

  rt_params p = {};
  p.width = w, p.height = h;
  p.spp = static_cast<uint32_t>(m_numRays);
  p.mode = m_mode == PATHTRACE ? RT_MODE_PATH : RT_MODE_RAY;
  p.max_depth = 3;  // calculateColorPath(ray, found, 0, 3) — Renderer.cpp:245,248
  p.seed = GpuSettings::get().seed;
  p.rng_mode = RT_RNG_PIXEL;
  p.accel = GpuSettings::get().accel;
  p.tile = 8;

  // Renderer.cpp:209-213: the photon map and its kd-tree are built inside render();
  // the map is a local there (the member stays empty, so a savePhotonMap() issued
  // BEFORE render() writes an empty cloud, as in the reference).  We keep the member
  // filled afterwards (in tree order) so that a later savePhotonMap() is useful.
  if (m_numPhotons > 0) {
    // the whole map on the device(s): emission, compaction and the kd order (the
    // reference's std::nth_element order, restated tie-exactly: csrc/kd_build.hip); every
    // device of a group builds the same map from the same streams.  The host copy only
    // feeds a later savePhotonMap().
    std::cout << "Constructing a photon map with " << m_numPhotons << " photons" << std::endl;
    if (!m_scene.lightsources().empty())
      std::cout << "Emitting " << static_cast<int>(m_numPhotons * (1.f / m_scene.lightsources().size()))
                << " photons per light source" << std::endl;
    std::cout << "Constructing a kd-tree for the photon map." << std::endl;
    uint32_t stored = 0;
    const uint32_t ranks = multi ? rt_group_size(many->group()) : 1u;
    for (uint32_t r = 0; r < ranks; ++r) {
      rt_ctx* cr = multi ? rt_group_ctx(many->group(), r) : ctx0;
      GpuSession::check(rt_build_photon_map(cr, static_cast<uint32_t>(m_numPhotons), GpuSettings::get().seed, &stored, nullptr),
                        "rt_build_photon_map");
    }
    std::cout << stored << " photons stored" << std::endl;
    if (stored) {
      std::vector<float> pos(3 * static_cast<size_t>(stored)), dir(pos.size()), wt(stored);
      uint32_t n = 0;
      GpuSession::check(rt_get_photons(ctx0, pos.data(), dir.data(), wt.data(), stored, &n), "rt_get_photons");
      PhotonMap map;
      for (uint32_t i = 0; i < n; ++i)
        map.list().push_back(Particle(Vec3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]),
                                      Vec3f(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]), wt[i]));
      m_photonMap = map;
      p.use_photons = 1, p.k = static_cast<uint32_t>(m_k), p.photons_requested = static_cast<uint32_t>(m_numPhotons);
    }
  }

  // -tune S (extension): the tree tuned on probe frames of THIS camera and integrator (rt_bvh_tune: same picture,
  // fewer node visits; pays off on small scenes rendered with many samples)
  if (GpuSettings::get().tune > 0. && !multi && !p.use_photons && p.accel == RT_ACCEL_BVH && p.spp > 0) {
    rt_params probe = p;
    const uint32_t longer = w > h ? w : h, scale = longer > 128u ? (longer + 127u) / 128u : 1u;
    probe.width = (w + scale - 1u) / scale, probe.height = (h + scale - 1u) / scale;
    probe.spp = 1;
    rt_tune_report rep = {};
    GpuSession::check(rt_bvh_tune(ctx0, &probe, GpuSettings::get().tune, 0u, &rep), "rt_bvh_tune");
    std::cout << "BVH tuned on " << probe.width << "x" << probe.height << " probe frames: " << rep.probes << " probes, " << rep.accepted
              << " changes kept, measured cost " << rep.cost_before << " -> " << rep.cost_after << " in " << rep.seconds << " s" << std::endl;
  }

  Image result(w, h);
  bool colouredFrame = false;  // the frame went through rt_render_colors: its AOVs' albedo is the interpolated colour
  bool texturedFrame = false;  // the frame went through rt_render_textured: its AOVs' albedo is the texture sample
  if (p.spp > 0 && multi) {
    // N devices: the whole frame in one sharded launch per device (rt_group_render);
    // update.ppm is written once, after the last pass
    p.tile = 32;
    rt_stats st = {};
    GpuSession::check(rt_group_render(many->group(), &p, image.data(), result.data(), nullptr, &st), "rt_group_render");
    m_stats = st;
    result.savePPM("update.ppm");
    std::cout << "Raytracing on " << devs.size() << " GPUs" << (rt_group_uses_rccl(many->group()) ? " (RCCL)" : " (peer copies)")
              << "... [" << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0 && GpuSettings::get().adaptive >= 0.) {
    // -adaptive T (extension): passes of -pass samples with seeds seed, seed + 1, ... over the 8x8-pixel granules whose
    // estimate has not converged (rt_render_adaptive); -N is the per-pixel maximum.  update.ppm is written once.  The
    // -aov / -denoise block below sees pass 0's parameters.
    const uint32_t maxSpp = p.spp;
    rt_adaptive_params a = {};
    p.spp = GpuSettings::get().pass;
    a.max_passes = maxSpp / p.spp;
    a.threshold = static_cast<float>(GpuSettings::get().adaptive);
    std::vector<uint32_t> spp(static_cast<size_t>(w) * h);
    rt_adaptive_report rep = {};
    rt_stats st = {};
    GpuSession::check(rt_render_adaptive(ctx0, &p, &a, image.data(), result.data(), nullptr, spp.data(), &rep, &st),
                      "rt_render_adaptive");
    m_stats = st;
    m_spp = Image(w, h);
    for (size_t i = 0; i < spp.size(); ++i)
      for (int k = 0; k < 3; ++k) m_spp.data()[3 * i + k] = static_cast<float>(spp[i]) / static_cast<float>(maxSpp);
    result.savePPM("update.ppm");
    std::cout << "Adaptive sampling: " << rep.passes << " passes of " << p.spp << " samples, "
              << static_cast<double>(rep.pixel_samples) / (static_cast<double>(w) * h) << " samples per pixel on average (at most "
              << maxSpp << ")" << std::endl;
    std::cout << "Raytracing... [" << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0 && GpuSettings::get().shutter) {
    // -shutter dx,dy,dz (extension): the frame under a shutter that stays open while the camera translates by that
    // vector (rt_render_shutter), in one launch; -aperture A -focus D put the thin lens on the moving camera.
    // update.ppm is written once.  Without -shutter this branch is not taken.
    if (p.use_photons) throw std::runtime_error("-shutter does not shade from the photon map (not with -p)");
    rt_shutter sh = {};
    sh.camera_close = single->flat().desc.camera;
    for (int k = 0; k < 3; ++k) {
      sh.camera_close.position[k] += GpuSettings::get().shutterMove[k];
      sh.camera_close.lower_left[k] += GpuSettings::get().shutterMove[k];
    }
    sh.open = 0.f, sh.close = 1.f;
    sh.aperture = static_cast<float>(GpuSettings::get().aperture);
    sh.focus_distance = static_cast<float>(GpuSettings::get().focus);
    rt_stats st = {};
    GpuSession::check(rt_render_shutter(ctx0, &p, &sh, image.data(), result.data(), nullptr, &st), "rt_render_shutter");
    m_stats = st;
    result.savePPM("update.ppm");
    std::cout << "Raytracing under an open shutter, the camera moving by (" << GpuSettings::get().shutterMove[0] << ", "
              << GpuSettings::get().shutterMove[1] << ", " << GpuSettings::get().shutterMove[2] << ")";
    if (sh.aperture > 0.f) std::cout << ", through a lens of radius " << sh.aperture << " focused at " << sh.focus_distance;
    std::cout << "... [" << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0 && GpuSettings::get().aperture > 0.) {
    // -aperture A -focus D (extension): the frame through a thin lens (rt_render_lens), in one launch; update.ppm is
    // written once.  Without -aperture this branch is not taken and the path below is unchanged.
    if (p.use_photons) throw std::runtime_error("-aperture does not shade from the photon map (not with -p)");
    rt_lens lens = {};
    lens.model = RT_LENS_THIN;
    lens.aperture = static_cast<float>(GpuSettings::get().aperture);
    lens.focus_distance = static_cast<float>(GpuSettings::get().focus);
    rt_stats st = {};
    GpuSession::check(rt_render_lens(ctx0, &p, &lens, image.data(), result.data(), nullptr, &st), "rt_render_lens");
    m_stats = st;
    result.savePPM("update.ppm");
    std::cout << "Raytracing through a lens of radius " << lens.aperture << " focused at " << lens.focus_distance << "... ["
              << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0 && GpuSettings::get().lightPick > 0) {
    // -lightpick M (extension): the frame with M sampled lights per path vertex, picked by the lights' power
    // (rt_render_pick), in one launch; update.ppm is written once.  Without -lightpick this branch is not taken.
    if (multi || p.use_photons) throw std::runtime_error("-lightpick runs on one GPU, without -p");
    rt_light_pick pick = {};
    pick.slots = GpuSettings::get().lightPick;
    rt_stats st = {};
    GpuSession::check(rt_render_pick(ctx0, &p, &pick, image.data(), result.data(), nullptr, &st), "rt_render_pick");
    m_stats = st;
    result.savePPM("update.ppm");
    std::cout << "Raytracing with " << pick.slots << " of " << m_scene.lightsources().size() << " lights sampled per path vertex... ["
              << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0 && GpuSettings::get().vcolors && sceneHasVertexColors(m_scene)) {
    // -vcolors 1 (extension): the frame with per-vertex albedo (rt_render_colors), in one launch: the colours of the
    // meshes that have them (COFF files), their material's albedo on the vertices of the others, which those meshes then
    // shade with as they always did.  update.ppm is written once.  Without -vcolors, or where no mesh has colours, this
    // branch is not taken.
    if (multi || p.use_photons) throw std::runtime_error("-vcolors runs on one GPU, without -p");
    std::vector<float> rgb;
    size_t colored = 0;
    for (const Mesh& m : m_scene.meshes()) {
      const bool has = m.vertexColors().size() == m.vertexPositions().size() && !m.vertexColors().empty();
      colored += has ? 1 : 0;
      for (size_t i = 0; i < m.vertexPositions().size(); ++i) {
        const Vec3f c = has ? m.vertexColors()[i] : m.material().albedo();
        rgb.insert(rgb.end(), {c[0], c[1], c[2]});
      }
    }
    GpuSession::check(rt_set_vertex_colors(ctx0, rgb.data(), static_cast<uint32_t>(rgb.size() / 3)), "rt_set_vertex_colors");
    rt_stats st = {};
    GpuSession::check(rt_render_colors(ctx0, &p, image.data(), result.data(), nullptr, &st), "rt_render_colors");
    colouredFrame = true;
    m_stats = st;
    result.savePPM("update.ppm");
    std::cout << "Raytracing with the vertex colours of " << colored << " of " << m_scene.meshes().size() << " meshes... ["
              << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0 && GpuSettings::get().textures && sceneHasTextures(m_scene)) {
    // -textures 1 (extension): the frame with image-textured albedo (rt_render_textured), in one launch: every mesh with
    // texture coordinates (an STOFF file) and a <stem>.ppm beside its .off samples that image, bilinear and repeating on
    // both axes; the other meshes stay untextured and shade as they always did.  update.ppm is written once.  Without
    // -textures, or where no mesh has a texture, this branch is not taken.
    if (multi || p.use_photons) throw std::runtime_error("-textures runs on one GPU, without -p");
    std::vector<TextureImage> images;
    std::vector<rt_texture> textures;
    std::vector<uint32_t> meshTexture, meshF0, meshKdAlpha, meshNormal;
    std::vector<float> uv;
    // -matmaps 1 (extension): <stem>_f0.ppm and <stem>_kda.ppm beside the .off join the set, bilinear and repeating as
    // the albedo image, and the frame goes through rt_render_material; a mesh without one keeps that field of its material
    const bool matmaps = GpuSettings::get().matmaps;
    uint32_t nMaps = 0;
    // -normalmaps 1 (extension): <stem>_n.ppm beside the .off joins the set likewise, and the frame goes through
    // rt_render_normal_mapped, with the material maps where -matmaps 1 is given too; a mesh without one keeps its normals
    const bool normalmaps = GpuSettings::get().normalmaps;
    uint32_t nNormals = 0;
    for (const Mesh& m : m_scene.meshes()) {
      const std::string file = meshTextureFile(m);
      meshTexture.push_back(file.empty() ? RT_TEX_NONE : static_cast<uint32_t>(images.size()));
      if (!file.empty()) images.push_back(TextureImage::loadPPM(file));
      const std::string f0 = matmaps ? meshTextureFile(m, "_f0") : "", kda = matmaps ? meshTextureFile(m, "_kda") : "";
      meshF0.push_back(f0.empty() ? RT_TEX_NONE : static_cast<uint32_t>(images.size()));
      if (!f0.empty()) images.push_back(TextureImage::loadPPM(f0)), ++nMaps;
      meshKdAlpha.push_back(kda.empty() ? RT_TEX_NONE : static_cast<uint32_t>(images.size()));
      if (!kda.empty()) images.push_back(TextureImage::loadPPM(kda)), ++nMaps;
      const std::string nrm = normalmaps ? meshTextureFile(m, "_n") : "";
      meshNormal.push_back(nrm.empty() ? RT_TEX_NONE : static_cast<uint32_t>(images.size()));
      if (!nrm.empty()) images.push_back(TextureImage::loadPPM(nrm)), ++nNormals;
      // (the coordinates of a mesh without a texture are never read)
      if (m.vertexUVs().size() == 2 * m.vertexPositions().size()) uv.insert(uv.end(), m.vertexUVs().begin(), m.vertexUVs().end());
      else uv.insert(uv.end(), 2 * m.vertexPositions().size(), 0.f);
    }
    for (const TextureImage& t : images) {
      rt_texture x = {};
      x.width = t.width, x.height = t.height, x.wrap_s = x.wrap_t = RT_TEX_REPEAT, x.filter = RT_TEX_BILINEAR, x.texels = t.texels.data();
      textures.push_back(x);
    }
    rt_texture_set set = {};
    set.n_textures = static_cast<uint32_t>(textures.size()), set.n_meshes = static_cast<uint32_t>(meshTexture.size());
    set.n_vertices = static_cast<uint32_t>(uv.size() / 2);
    set.textures = textures.data(), set.mesh_texture = meshTexture.data(), set.vertex_uv = uv.data();
    GpuSession::check(rt_set_textures(ctx0, &set), "rt_set_textures");
    rt_stats st = {};
    if (matmaps) {
      rt_material_maps maps = {};
      maps.n_meshes = set.n_meshes, maps.mesh_f0 = meshF0.data(), maps.mesh_kd_alpha = meshKdAlpha.data();
      GpuSession::check(rt_set_material_maps(ctx0, &maps), "rt_set_material_maps");
    }
    if (normalmaps) {
      rt_normal_maps maps = {};
      maps.n_meshes = set.n_meshes, maps.mesh_normal = meshNormal.data();
      GpuSession::check(rt_set_normal_maps(ctx0, &maps), "rt_set_normal_maps");
      GpuSession::check(rt_render_normal_mapped(ctx0, &p, image.data(), result.data(), nullptr, &st), "rt_render_normal_mapped");
    } else if (matmaps) {
      GpuSession::check(rt_render_material(ctx0, &p, image.data(), result.data(), nullptr, &st), "rt_render_material");
    } else
    GpuSession::check(rt_render_textured(ctx0, &p, image.data(), result.data(), nullptr, &st), "rt_render_textured");
    texturedFrame = true;
    m_stats = st;
    result.savePPM("update.ppm");
    if (matmaps) std::cout << "Material maps: " << nMaps << " images" << std::endl;
    if (normalmaps) std::cout << "Normal maps: " << nNormals << " images" << std::endl;
    std::cout << "Raytracing with the textures of " << images.size() - nMaps - nNormals << " of " << m_scene.meshes().size() << " meshes... ["
              << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  } else if (p.spp > 0) {
    // The reference re-saves update.ppm after EVERY pass (Renderer.cpp:261-269).  Here a
    // "pass" is a sample range of one launch; GpuSettings::progress = P > 0 renders P
    // samples per launch and saves the running estimate after each (resolved with the
    // number of samples so far, as the reference does), 0 renders the frame in one launch.
    // Sample ranges never change the result (the per-pixel sum order is fixed).
    const uint32_t chunk = GpuSettings::get().progress ? GpuSettings::get().progress : p.spp;
    std::vector<float> accum(static_cast<size_t>(w) * h * 4, 0.f);
    rt_stats total = {};
    for (uint32_t done = 0; done < p.spp; done += chunk) {
      p.spp_begin = done;
      p.spp_count = done + chunk > p.spp ? p.spp - done : chunk;
      rt_stats st = {};
      GpuSession::check(rt_render_passes(ctx0, &p, image.data(), accum.data(), result.data(), &st), "rt_render");
      total.samples += st.samples, total.rays_closest += st.rays_closest, total.rays_shadow += st.rays_shadow;
      total.knn_queries += st.knn_queries, total.kernel_ms += st.kernel_ms;
      result.savePPM("update.ppm");
    }
    m_stats = total;
    std::cout << "Raytracing... [" << std::string(50, '#') << "] 100%" << std::endl;
    image = result;
  }

  // -aov / -denoise (extensions): the first-hit AOVs of this frame's primary rays (rt_render_aov; of a coloured frame
  // rt_render_aov_colors, of a textured one rt_render_aov_textured: the albedo channel is the colour the frame shaded with) and the a-trous filter of the frame
  // guided by them (rt_denoise).  The frame itself stays as it is.
  const bool wantAov = GpuSettings::get().aov, wantDenoise = GpuSettings::get().denoise;
  if ((wantAov || wantDenoise) && multi) throw std::runtime_error("-aov / -denoise run on one GPU only (not with -gpus > 1)");
  if ((wantAov || wantDenoise) && p.spp > 0) {
    p.spp_begin = 0, p.spp_count = 0;
    const size_t npx = static_cast<size_t>(w) * h;
    std::vector<float> alb(3 * npx), nrm(3 * npx), pos(3 * npx);
    std::vector<uint32_t> hits(npx);
    rt_aov aov = {};
    aov.albedo = alb.data(), aov.normal = nrm.data(), aov.position = pos.data(), aov.hits = hits.data();
    if (colouredFrame) GpuSession::check(rt_render_aov_colors(ctx0, &p, &aov), "rt_render_aov_colors");
    else if (texturedFrame) GpuSession::check(rt_render_aov_textured(ctx0, &p, &aov), "rt_render_aov_textured");
    else GpuSession::check(rt_render_aov(ctx0, &p, &aov), "rt_render_aov");
    if (wantAov) {  // the means (sum / hits; 0 where no sample hit)
      m_albedo = Image(w, h), m_normal = Image(w, h);
      for (size_t i = 0; i < npx; ++i)
        for (int k = 0; k < 3; ++k) {
          const float n = static_cast<float>(hits[i]);
          m_albedo.data()[3 * i + k] = hits[i] ? alb[3 * i + k] / n : 0.f;
          m_normal.data()[3 * i + k] = hits[i] ? 0.5f * (nrm[3 * i + k] / n) + 0.5f : 0.f;
        }
    }
    if (wantDenoise) {
      rt_denoise_params dp = {};
      dp.width = w, dp.height = h;
      m_denoised = Image(w, h);
      GpuSession::check(rt_denoise(ctx0, &dp, image.data(), &aov, m_denoised.data()), "rt_denoise");
    }
  }

  // -ao N [-aodist D] (extension): N occlusion rays at every primary hit of this frame (rt_render_ao, the default bias),
  // as the grey mean unoccluded / (hits N), 1 where no sample hit.  The frame itself stays as it is.
  const uint32_t aoRays = GpuSettings::get().ao;
  if (aoRays && multi) throw std::runtime_error("-ao runs on one GPU only (not with -gpus > 1)");
  if (aoRays && p.spp > 0) {
    p.spp_begin = 0, p.spp_count = 0;
    const size_t npx = static_cast<size_t>(w) * h;
    std::vector<uint32_t> un(npx), hits(npx);
    rt_ao_params ap = {};
    ap.n_rays = aoRays, ap.max_distance = static_cast<float>(GpuSettings::get().aoDistance);
    rt_ao out = {};
    out.unoccluded = un.data(), out.hits = hits.data();
    GpuSession::check(rt_render_ao(ctx0, &p, &ap, &out), "rt_render_ao");
    m_ao = Image(w, h);
    for (size_t i = 0; i < npx; ++i) {
      const float den = static_cast<float>(hits[i]) * static_cast<float>(aoRays);
      const float v = hits[i] ? static_cast<float>(un[i]) / den : 1.f;
      for (int k = 0; k < 3; ++k) m_ao.data()[3 * i + k] = v;
    }
  }

  // -lights each | M0,M1,... (extension): this frame split by light group (rt_render_lights) — the frame with only one
  // light lit, or only the lights of a mask, every group from the rays of ONE launch, resolved over the frame's
  // background.  The frame itself stays as it is.
  const bool each = GpuSettings::get().lightsEach;
  std::vector<unsigned> masks = GpuSettings::get().lightMasks;
  if ((each || !masks.empty()) && (multi || p.use_photons || GpuSettings::get().adaptive >= 0. || GpuSettings::get().shutter ||
                                   GpuSettings::get().aperture > 0.))
    throw std::runtime_error("-lights runs on one GPU, without -p, -adaptive, -shutter and -aperture");
  if (each) {
    const size_t nl = m_scene.lightsources().size();
    if (nl == 0 || nl > RT_LIGHT_GROUPS_MAX)
      throw std::runtime_error("-lights each: the scene has " + std::to_string(nl) + " lights and a frame takes 1.." +
                               std::to_string(RT_LIGHT_GROUPS_MAX) + " groups (use -lights M0,M1,...)");
    for (size_t l = 0; l < nl; ++l) masks.push_back(1u << l);
  }
  m_groups.clear();
  if (!masks.empty() && p.spp > 0) {
    p.spp_begin = 0, p.spp_count = 0;
    rt_light_groups lg = {};
    lg.n_groups = static_cast<uint32_t>(masks.size());
    for (size_t g = 0; g < masks.size(); ++g) lg.masks[g] = masks[g];
    const size_t npx = static_cast<size_t>(w) * h;
    std::vector<float> out(3 * npx * masks.size());
    rt_stats st = {};
    // (the background the frame was resolved over: `image` holds the frame by now)
    Image bg(w, h);
    bg.fillBackground();
    GpuSession::check(rt_render_lights(ctx0, &p, &lg, bg.data(), out.data(), nullptr, &st), "rt_render_lights");
    for (size_t g = 0; g < masks.size(); ++g) {
      m_groups.emplace_back(w, h);
      std::copy(out.begin() + 3 * npx * g, out.begin() + 3 * npx * (g + 1), m_groups.back().data());
    }
    std::cout << "Light groups: " << masks.size() << " frames from one launch, " << static_cast<double>(st.rays_closest + st.rays_shadow) / 1e6
              << " Mrays in " << st.kernel_ms << " ms" << std::endl;
  }
}
