// mat_host_check.cpp — the host side of rt_set_material_maps / rt_render_material as a stand-alone program, for sanitizer
// runs on the CPU (no GPU, no Python).  It covers what runs without a device: material_maps.h's scan of tables that are
// exactly as long as n_meshes says, on the heap (a scan that reads one entry too many is the sanitizer's to report), and
// the tables it builds; every rejection of rt_set_material_maps and of the frame calls that the arguments alone decide
// (the context is NULL or never looked at); and TextureImage::loadPPM on the two map fixtures.
//
// rt_api.cpp and bvh_build.cpp are compiled with the sanitizers; the kernels' objects come from the product's build
// (make -C ray-tracing-engine_amd) through an archive, from the repository root:
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/mat_host_check.cpp ray-tracing-engine_amd/csrc/rt_api.cpp ray-tracing-engine_amd/csrc/bvh_build.cpp; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -ffp-contract=off -pthread -Iinclude -Iray-tracing-engine_amd/csrc \
//         -Iray-tracing-engine_amd/host -c $f -o $(basename $f).o; done
//   ar rcs kernels.a ray-tracing-engine_amd/build/*.hip.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread mat_host_check.cpp.o rt_api.cpp.o bvh_build.cpp.o \
//       -Wl,--whole-archive kernels.a -Wl,--no-whole-archive -o mat_host_check
//   ./mat_host_check tests/golden/meshes/cube_st_f0.ppm tests/golden/meshes/cube_st_kda.ppm
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "Texture.h"
#include "material_maps.h"
#include "rt_amd.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, rt_last_error()); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

bool says(const char* word) { return strstr(rt_last_error(), word) != nullptr; }

rt_ctx* const FAKE = reinterpret_cast<rt_ctx*>(1);  // (never looked at by the calls below)
constexpr uint32_t NM = 1009, NT = 7;               // (no multiples of anything)

// Valid maps on the heap, both tables exactly as long as n_meshes says: indices below NT with RT_TEX_NONE between them.
struct Maps {
  std::unique_ptr<uint32_t[]> f0{new uint32_t[NM]}, kda{new uint32_t[NM]};
  rt_material_maps maps = {};
  Maps() {
    for (uint32_t m = 0; m < NM; ++m) f0[m] = m % 5 == 4 ? RT_TEX_NONE : m % NT, kda[m] = m % 3 == 2 ? RT_TEX_NONE : (m + 3) % NT;
    maps.n_meshes = NM, maps.mesh_f0 = f0.get(), maps.mesh_kd_alpha = kda.get();
  }
};

void table_checks() {
  rtmat::Tables t;
  std::string why;
  {
    Maps m;
    EXPECT(rtmat::first_reserved(m.maps) == -1);
    EXPECT(rtmat::build_tables(m.maps, NT, &t, &why) && t.f0.size() == NM && t.kdAlpha.size() == NM);
    EXPECT(memcmp(t.f0.data(), m.f0.get(), NM * sizeof(uint32_t)) == 0 && memcmp(t.kdAlpha.data(), m.kda.get(), NM * sizeof(uint32_t)) == 0);
    // the last entry of each table is read, and is the largest index that passes
    m.f0[NM - 1] = NT - 1, m.kda[NM - 1] = NT - 1;
    EXPECT(rtmat::build_tables(m.maps, NT, &t, &why) && t.f0[NM - 1] == NT - 1 && t.kdAlpha[NM - 1] == NT - 1);
    // a null table is RT_TEX_NONE on every mesh, and the other one is still scanned
    m.maps.mesh_f0 = nullptr;
    EXPECT(rtmat::build_tables(m.maps, NT, &t, &why) && t.f0.size() == NM && t.f0[0] == RT_TEX_NONE && t.f0[NM - 1] == RT_TEX_NONE);
    EXPECT(t.kdAlpha[0] == m.kda[0]);
    m.maps.mesh_kd_alpha = nullptr;
    EXPECT(rtmat::build_tables(m.maps, NT, &t, &why) && t.kdAlpha[NM / 2] == RT_TEX_NONE);
    m.maps.n_meshes = 0;
    EXPECT(rtmat::build_tables(m.maps, NT, &t, &why) && t.f0.empty() && t.kdAlpha.empty());
  }
  for (uint32_t bad : {NT, NT + 1u, 0xfffffffeu}) {
    for (uint32_t at : {0u, 500u, NM - 1u}) {
      char want[96];
      Maps a;
      a.f0[at] = bad, a.kda[0] = bad;  // (mesh_f0 is scanned first)
      if (at + 1 < NM) a.f0[NM - 1] = bad;  // (a later bad entry is not the one named)
      snprintf(want, sizeof want, "mesh_f0[%u] is %u: neither one of %u textures", at, bad, NT);
      EXPECT(!rtmat::build_tables(a.maps, NT, &t, &why) && why.find(want) != std::string::npos);
      Maps b;
      b.kda[at] = bad;
      snprintf(want, sizeof want, "mesh_kd_alpha[%u] is %u: neither one of %u textures", at, bad, NT);
      EXPECT(!rtmat::build_tables(b.maps, NT, &t, &why) && why.find(want) != std::string::npos);
    }
  }
  // a smaller resident set refuses what a larger one takes
  {
    Maps m;
    EXPECT(!rtmat::build_tables(m.maps, NT - 1, &t, &why) && why.find("mesh_f0[6] is 6") != std::string::npos);
  }
  for (int k = 0; k < 5; ++k) {
    Maps m;
    m.maps.reserved[k] = 1u + (uint32_t)k, m.maps.reserved[4] = 9;
    EXPECT(rtmat::first_reserved(m.maps) == k);
  }
}

void set_checks() {
  EXPECT(rt_set_material_maps(nullptr, nullptr) == RT_ERR_INVALID && says("null"));
  {
    // clean maps end at the null context — with an entry beyond any set, which only a context's set can tell
    Maps m;
    EXPECT(rt_set_material_maps(nullptr, &m.maps) == RT_ERR_INVALID && says("ctx"));
    m.f0[3] = 0xfffffffeu;
    EXPECT(rt_set_material_maps(nullptr, &m.maps) == RT_ERR_INVALID && says("ctx"));
    m.maps.mesh_f0 = m.maps.mesh_kd_alpha = nullptr;
    EXPECT(rt_set_material_maps(nullptr, &m.maps) == RT_ERR_INVALID && says("ctx"));
  }
  for (int k = 0; k < 5; ++k) {
    // a reserved word comes before the context, null or not
    Maps m;
    m.maps.reserved[k] = 3;
    char want[32];
    snprintf(want, sizeof want, "reserved[%d] is 3", k);
    EXPECT(rt_set_material_maps(FAKE, &m.maps) == RT_ERR_INVALID && says(want));
    EXPECT(rt_set_material_maps(nullptr, &m.maps) == RT_ERR_INVALID && says(want));
  }
}

void frame_checks() {
  rt_params p = {};
  p.width = 5, p.height = 3, p.spp = 4, p.mode = RT_MODE_PATH, p.max_depth = 3, p.rng_mode = RT_RNG_PIXEL, p.tile = 8;
  float bg[45] = {}, out[45], acc[60];
  EXPECT(rt_render_material(nullptr, &p, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_material(FAKE, nullptr, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_material(FAKE, &p, bg, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("neither"));
  EXPECT(rt_render_material(FAKE, &p, nullptr, out, acc, nullptr) == RT_ERR_INVALID && says("background"));
  EXPECT(rt_render_material_device(FAKE, &p, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("d_accum"));
  rt_params q = p;
  q.spp = 0;
  EXPECT(rt_render_material(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_INVALID);
  q = p, q.world = 2;
  EXPECT(rt_render_material(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED && says("world"));
  q = p, q.use_photons = 1, q.k = 4, q.photons_requested = 10;
  EXPECT(rt_render_material_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("photon"));
  q = p, q.reserved[2] = 1;
  EXPECT(rt_render_material_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("wavefront"));
  q = p, q.rng_mode = RT_RNG_LEGACY;
  EXPECT(rt_render_material(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED);
}

void fixture_checks(const char* f0File, const char* kdaFile) {
  const TextureImage f0 = TextureImage::loadPPM(f0File), kda = TextureImage::loadPPM(kdaFile);
  EXPECT(f0.width == 2 && f0.height == 2 && f0.texels.size() == 12 && f0.texels[3] == 1.f && f0.texels[5] == 80.f / 255.f);
  EXPECT(kda.width == 3 && kda.height == 2 && kda.texels.size() == 18 && kda.texels[0] == 230.f / 255.f && kda.texels[16] == 90.f / 255.f);
  for (size_t i = 1; i < kda.texels.size(); i += 3) EXPECT(kda.texels[i] > 0.f);  // (no alpha of 0)
}

}  // namespace

int main(int argc, char** argv) {
  table_checks();
  set_checks();
  frame_checks();
  if (argc > 2) fixture_checks(argv[1], argv[2]);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("mat_host_check: all checks passed\n");
  return 0;
}
