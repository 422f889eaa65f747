// nmap_host_check.cpp — the host side of rt_set_normal_maps / rt_render_normal_mapped as a stand-alone program, for
// sanitizer runs on the CPU (no GPU, no Python).  It covers what runs without a device: normal_maps.h's scan of a table
// that is exactly as long as n_meshes says, on the heap (a scan that reads one entry too many is the sanitizer's to
// report), and the table it builds; every rejection of rt_set_normal_maps and of the frame calls that the arguments alone
// decide (the context is NULL or never looked at); and TextureImage::loadPPM on the normal-map fixture.
//
// rt_api.cpp and bvh_build.cpp are compiled with the sanitizers; the kernels' objects come from the product's build
// (make -C ray-tracing-engine_amd) through an archive, from the repository root:
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/nmap_host_check.cpp ray-tracing-engine_amd/csrc/rt_api.cpp ray-tracing-engine_amd/csrc/bvh_build.cpp; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -ffp-contract=off -pthread -Iinclude -Iray-tracing-engine_amd/csrc \
//         -Iray-tracing-engine_amd/host -c $f -o $(basename $f).o; done
//   ar rcs kernels.a ray-tracing-engine_amd/build/*.hip.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread nmap_host_check.cpp.o rt_api.cpp.o bvh_build.cpp.o \
//       -Wl,--whole-archive kernels.a -Wl,--no-whole-archive -o nmap_host_check
//   ./nmap_host_check tests/golden/meshes/cube_st_n.ppm
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "Texture.h"
#include "normal_maps.h"
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
constexpr int NR = rtnrm::kReservedWords;

// Valid maps on the heap, the table exactly as long as n_meshes says: indices below NT with RT_TEX_NONE between them.
struct Maps {
  std::unique_ptr<uint32_t[]> normal{new uint32_t[NM]};
  rt_normal_maps maps = {};
  Maps() {
    for (uint32_t m = 0; m < NM; ++m) normal[m] = m % 5 == 4 ? RT_TEX_NONE : m % NT;
    maps.n_meshes = NM, maps.mesh_normal = normal.get();
  }
};

void table_checks() {
  static_assert(NR == 6, "rt_normal_maps has six reserved words");
  std::vector<uint32_t> t;
  std::string why;
  {
    Maps m;
    EXPECT(rtnrm::first_reserved(m.maps) == -1);
    EXPECT(rtnrm::build_table(m.maps, NT, &t, &why) && t.size() == NM);
    EXPECT(memcmp(t.data(), m.normal.get(), NM * sizeof(uint32_t)) == 0);
    // the last entry is read, and is the largest index that passes
    m.normal[NM - 1] = NT - 1;
    EXPECT(rtnrm::build_table(m.maps, NT, &t, &why) && t[NM - 1] == NT - 1);
    // a null table is RT_TEX_NONE on every mesh
    m.maps.mesh_normal = nullptr;
    EXPECT(rtnrm::build_table(m.maps, NT, &t, &why) && t.size() == NM && t[0] == RT_TEX_NONE && t[NM - 1] == RT_TEX_NONE);
    m.maps.n_meshes = 0;
    EXPECT(rtnrm::build_table(m.maps, NT, &t, &why) && t.empty());
  }
  for (uint32_t bad : {NT, NT + 1u, 0xfffffffeu}) {
    for (uint32_t at : {0u, 500u, NM - 1u}) {
      char want[96];
      Maps a;
      a.normal[at] = bad;
      if (at + 1 < NM) a.normal[NM - 1] = bad;  // (a later bad entry is not the one named)
      snprintf(want, sizeof want, "normal maps: mesh_normal[%u] is %u: neither one of %u textures", at, bad, NT);
      EXPECT(!rtnrm::build_table(a.maps, NT, &t, &why) && why.find(want) != std::string::npos);
    }
  }
  // a smaller resident set refuses what a larger one takes
  {
    Maps m;
    EXPECT(!rtnrm::build_table(m.maps, NT - 1, &t, &why) && why.find("mesh_normal[6] is 6") != std::string::npos);
  }
  for (int k = 0; k < NR; ++k) {
    Maps m;
    m.maps.reserved[k] = 1u + (uint32_t)k, m.maps.reserved[NR - 1] = 9;
    EXPECT(rtnrm::first_reserved(m.maps) == k);
  }
}

void set_checks() {
  EXPECT(rt_set_normal_maps(nullptr, nullptr) == RT_ERR_INVALID && says("null"));
  {
    // clean maps end at the null context — with an entry beyond any set, which only a context's set can tell
    Maps m;
    EXPECT(rt_set_normal_maps(nullptr, &m.maps) == RT_ERR_INVALID && says("ctx"));
    m.normal[3] = 0xfffffffeu;
    EXPECT(rt_set_normal_maps(nullptr, &m.maps) == RT_ERR_INVALID && says("ctx"));
    m.maps.mesh_normal = nullptr;
    EXPECT(rt_set_normal_maps(nullptr, &m.maps) == RT_ERR_INVALID && says("ctx"));
  }
  for (int k = 0; k < NR; ++k) {
    // a reserved word comes before the context, null or not
    Maps m;
    m.maps.reserved[k] = 3;
    char want[48];
    snprintf(want, sizeof want, "normal maps: reserved[%d] is 3", k);
    EXPECT(rt_set_normal_maps(FAKE, &m.maps) == RT_ERR_INVALID && says(want));
    EXPECT(rt_set_normal_maps(nullptr, &m.maps) == RT_ERR_INVALID && says(want));
  }
}

void frame_checks() {
  rt_params p = {};
  p.width = 5, p.height = 3, p.spp = 4, p.mode = RT_MODE_PATH, p.max_depth = 3, p.rng_mode = RT_RNG_PIXEL, p.tile = 8;
  float bg[45] = {}, out[45], acc[60];
  EXPECT(rt_render_normal_mapped(nullptr, &p, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_normal_mapped(FAKE, nullptr, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_normal_mapped(FAKE, &p, bg, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("neither"));
  EXPECT(rt_render_normal_mapped(FAKE, &p, nullptr, out, acc, nullptr) == RT_ERR_INVALID && says("background"));
  EXPECT(rt_render_normal_mapped_device(FAKE, &p, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("d_accum"));
  rt_params q = p;
  q.spp = 0;
  EXPECT(rt_render_normal_mapped(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_INVALID);
  q = p, q.world = 2;
  EXPECT(rt_render_normal_mapped(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED && says("world") && says("normal-mapped"));
  q = p, q.use_photons = 1, q.k = 4, q.photons_requested = 10;
  EXPECT(rt_render_normal_mapped_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("photon"));
  q = p, q.reserved[2] = 1;
  EXPECT(rt_render_normal_mapped_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("wavefront"));
  q = p, q.rng_mode = RT_RNG_LEGACY;
  EXPECT(rt_render_normal_mapped(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED);
}

void fixture_checks(const char* file) {
  const TextureImage n = TextureImage::loadPPM(file);
  EXPECT(n.width == 3 && n.height == 3 && n.texels.size() == 27 && n.texels[0] == 128.f / 255.f && n.texels[26] == 180.f / 255.f);
  for (size_t i = 2; i < n.texels.size(); i += 3) EXPECT(n.texels[i] > 0.5f);  // (every z is positive)
}

}  // namespace

int main(int argc, char** argv) {
  table_checks();
  set_checks();
  frame_checks();
  if (argc > 1) fixture_checks(argv[1]);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("nmap_host_check: all checks passed\n");
  return 0;
}
