// vcol_host_check.cpp — the host side of rt_set_vertex_colors / rt_render_colors and the COFF loader as a stand-alone
// program, for sanitizer runs on the CPU (no GPU, no Python).  It covers what runs without a device: rt_set_vertex_colors'
// scan of an array of exactly n_vertices x 3 floats on the heap (a scan that reads one element too many is the
// sanitizer's to report), every rejection of the frame calls that the arguments alone decide (the context is NULL or
// never looked at), and Mesh::loadOFF on COFF files: integer and float colours, three and four values, comments, and the
// malformed lines it refuses.
//
// rt_api.cpp and bvh_build.cpp are compiled with the sanitizers; the kernels' objects come from the product's build
// (make -C ray-tracing-engine_amd) through an archive, from the repository root:
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/vcol_host_check.cpp ray-tracing-engine_amd/csrc/rt_api.cpp ray-tracing-engine_amd/csrc/bvh_build.cpp; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -ffp-contract=off -pthread -Iinclude -Iray-tracing-engine_amd/csrc \
//         -Iray-tracing-engine_amd/host -c $f -o $(basename $f).o; done
//   ar rcs kernels.a ray-tracing-engine_amd/build/*.hip.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread vcol_host_check.cpp.o rt_api.cpp.o bvh_build.cpp.o \
//       -Wl,--whole-archive kernels.a -Wl,--no-whole-archive -o vcol_host_check
//   ./vcol_host_check tests/golden/meshes/cube_colors.off
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <string>

#include "Mesh.h"
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

constexpr uint32_t NV = 5003;  // (no multiple of anything)
rt_ctx* const FAKE = reinterpret_cast<rt_ctx*>(1);  // (never looked at by the calls below)

void colour_array_checks() {
  std::unique_ptr<float[]> rgb{new float[3 * NV]};
  for (uint32_t i = 0; i < 3 * NV; ++i) rgb[i] = (float)(i % 7) * 0.25f - 0.25f;  // (no range is imposed)
  // a clean array ends at the null context, after the whole scan
  EXPECT(rt_set_vertex_colors(nullptr, rgb.get(), NV) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_set_vertex_colors(nullptr, nullptr, NV) == RT_ERR_INVALID && says("null"));
  const float bad[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                       -std::numeric_limits<float>::infinity()};
  const uint32_t at[] = {0u, 1u, 3u * NV / 2u, 3u * NV - 1u};
  for (float b : bad)
    for (uint32_t j : at) {
      const float keep = rgb[j], keepLast = rgb[3 * NV - 1];
      rgb[j] = b;
      rgb[3 * NV - 1] = bad[0];  // (a later bad value is not the one named)
      char want[64];
      snprintf(want, sizeof want, "rgb[%u] (vertex %u,", j, j / 3u);
      EXPECT(rt_set_vertex_colors(FAKE, rgb.get(), NV) == RT_ERR_INVALID && says(want));
      rgb[j] = keep, rgb[3 * NV - 1] = keepLast;
    }
}

void frame_checks() {
  rt_params p = {};
  p.width = 5, p.height = 3, p.spp = 4, p.mode = RT_MODE_PATH, p.max_depth = 3, p.rng_mode = RT_RNG_PIXEL, p.tile = 8;
  float bg[45] = {}, out[45], acc[60];
  EXPECT(rt_render_colors(nullptr, &p, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_colors(FAKE, nullptr, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_colors(FAKE, &p, bg, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("neither"));
  EXPECT(rt_render_colors(FAKE, &p, nullptr, out, acc, nullptr) == RT_ERR_INVALID && says("background"));
  EXPECT(rt_render_colors_device(FAKE, &p, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("d_accum"));
  rt_params q = p;
  q.spp = 0;
  EXPECT(rt_render_colors(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_INVALID);
  q = p, q.world = 2;
  EXPECT(rt_render_colors(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED && says("world"));
  q = p, q.use_photons = 1, q.k = 4, q.photons_requested = 10;
  EXPECT(rt_render_colors_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("photon"));
  q = p, q.reserved[2] = 1;
  EXPECT(rt_render_colors_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("wavefront"));
  q = p, q.rng_mode = RT_RNG_LEGACY;
  EXPECT(rt_render_colors(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED);
  rt_aov a = {};
  EXPECT(rt_render_aov_colors(nullptr, &p, &a) == RT_ERR_INVALID);
  EXPECT(rt_render_aov_colors_device(nullptr, &p, &a, nullptr) == RT_ERR_INVALID);
}

bool loads(const std::string& text, Mesh* m) {
  const char* path = "vcol_host_check_tmp.off";
  {
    std::ofstream f(path);
    f << text;
  }
  bool ok = true;
  try {
    m->loadOFF(path);
  } catch (const std::exception&) {
    ok = false;
  }
  remove(path);
  return ok;
}

void loader_checks(const char* fixture) {
  Mesh m;
  const std::string faces = "3 0 1 2\n";
  EXPECT(loads("COFF\n3 1 0\n0 0 0 255 0 51\n1 0 0 0 255 0 7\n0 1 0 0 0 0\n" + faces, &m));
  EXPECT(m.vertexColors().size() == 3 && m.indexedTriangles().size() == 1 && m.vertexNormals().size() == 3);
  EXPECT(m.vertexColors()[0][0] == 1.f && m.vertexColors()[0][2] == 51.f / 255.f && m.vertexColors()[1][1] == 1.f);
  EXPECT(m.vertexPositions()[1][0] == 1.f && m.vertexPositions()[2][1] == 1.f);
  // floats 0..1 (one value with a point makes the file's colours floats), a comment behind a vertex
  EXPECT(loads("COFF\n# c\n3 1 0\n0 0 0 1 0 0.5 # red\n1 0 0 0 1 0 1\n0 1 0 0 0 1\n" + faces, &m));
  EXPECT(m.vertexColors().size() == 3 && m.vertexColors()[0][0] == 1.f && m.vertexColors()[0][2] == 0.5f && m.vertexColors()[2][2] == 1.f);
  // a plain OFF file has none, and a mesh loaded twice forgets the colours of the first file
  EXPECT(loads("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n" + faces, &m));
  EXPECT(m.vertexColors().empty() && m.vertexPositions().size() == 3 && m.indexedTriangles().size() == 1);
  // two or five colour values, and a value that is no number
  EXPECT(!loads("COFF\n3 1 0\n0 0 0 1 2\n1 0 0 0 1 0\n0 1 0 0 0 1\n" + faces, &m));
  EXPECT(!loads("COFF\n3 1 0\n0 0 0 1 2 3 4 5\n1 0 0 0 1 0\n0 1 0 0 0 1\n" + faces, &m));
  EXPECT(!loads("COFF\n3 1 0\n0 0 0 1 x 3\n1 0 0 0 1 0\n0 1 0 0 0 1\n" + faces, &m));
  // what strtod would read but a colour is not: nan, inf, a hexadecimal float; a negative value; an integer above 255
  for (const char* bad : {"nan", "inf", "-inf", "0x1p-1", "-1", "-0.5", "256"})
    EXPECT(!loads(std::string("COFF\n3 1 0\n0 0 0 1 ") + bad + " 3\n1 0 0 0 1 0\n0 1 0 0 0 1\n" + faces, &m));
  // ... while a float above 1 is kept, and 256 is a float's value where the file's colours are floats
  EXPECT(loads("COFF\n3 1 0\n0 0 0 1.5 256 0\n1 0 0 0 1 0\n0 1 0 0 0 1\n" + faces, &m) && m.vertexColors()[0][0] == 1.5f && m.vertexColors()[0][1] == 256.f);
  if (fixture) {
    Mesh cube;
    cube.loadOFF(fixture);
    EXPECT(cube.vertexPositions().size() == 8 && cube.indexedTriangles().size() == 12 && cube.vertexColors().size() == 8);
    EXPECT(cube.vertexColors()[0][0] == 1.f && cube.vertexColors()[0][1] == 40.f / 255.f && cube.vertexColors()[7][2] == 0.f);
  }
}

}  // namespace

int main(int argc, char** argv) {
  colour_array_checks();
  frame_checks();
  loader_checks(argc > 1 ? argv[1] : nullptr);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("vcol_host_check: all checks passed\n");
  return 0;
}
