// tex_host_check.cpp — the host side of rt_set_textures / rt_render_textured, the STOFF loader and the PPM reader as a
// stand-alone program, for sanitizer runs on the CPU (no GPU, no Python).  It covers what runs without a device:
// rt_set_textures' scan of a set whose arrays are exactly as long as its counts say, on the heap (a scan that reads one
// element too many is the sanitizer's to report), every rejection of the set and of the frame calls that the arguments
// alone decide (the context is NULL or never looked at), Mesh::loadOFF on STOFF and STCOFF files, and
// TextureImage::loadPPM on plain and binary files, with the malformed ones both refuse.
//
// rt_api.cpp and bvh_build.cpp are compiled with the sanitizers; the kernels' objects come from the product's build
// (make -C ray-tracing-engine_amd) through an archive, from the repository root:
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/tex_host_check.cpp ray-tracing-engine_amd/csrc/rt_api.cpp ray-tracing-engine_amd/csrc/bvh_build.cpp; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -ffp-contract=off -pthread -Iinclude -Iray-tracing-engine_amd/csrc \
//         -Iray-tracing-engine_amd/host -c $f -o $(basename $f).o; done
//   ar rcs kernels.a ray-tracing-engine_amd/build/*.hip.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread tex_host_check.cpp.o rt_api.cpp.o bvh_build.cpp.o \
//       -Wl,--whole-archive kernels.a -Wl,--no-whole-archive -o tex_host_check
//   ./tex_host_check tests/golden/meshes/cube_st.off tests/golden/meshes/cube_st.ppm
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "Mesh.h"
#include "Texture.h"
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
constexpr uint32_t NV = 5003, NM = 7;               // (no multiples of anything)

// A valid set on the heap, every array exactly as long as the counts say: a 5x3 and a 64x32 texture.
struct Set {
  std::unique_ptr<float[]> t0{new float[3 * 5 * 3]}, t1{new float[3 * 64 * 32]}, uv{new float[2 * NV]};
  std::unique_ptr<uint32_t[]> mesh{new uint32_t[NM]};
  std::unique_ptr<rt_texture[]> tex{new rt_texture[2]};
  rt_texture_set set = {};
  Set() {
    for (int i = 0; i < 45; ++i) t0[i] = (float)(i % 7) * 0.25f - 0.25f;  // (no range is imposed on texels)
    for (int i = 0; i < 3 * 64 * 32; ++i) t1[i] = (float)(i % 11) * 0.125f;
    for (uint32_t i = 0; i < 2 * NV; ++i) uv[i] = (float)(i % 4097) * 0.5f - 1024.f;  // (-1024 .. 1024: the limits pass)
    for (uint32_t m = 0; m < NM; ++m) mesh[m] = m % 3 == 2 ? RT_TEX_NONE : m % 3;
    memset(tex.get(), 0, 2 * sizeof(rt_texture));
    tex[0].width = 5, tex[0].height = 3, tex[0].wrap_s = RT_TEX_CLAMP, tex[0].filter = RT_TEX_NEAREST, tex[0].texels = t0.get();
    tex[1].width = 64, tex[1].height = 32, tex[1].wrap_t = RT_TEX_CLAMP, tex[1].filter = RT_TEX_BILINEAR, tex[1].texels = t1.get();
    set.n_textures = 2, set.n_meshes = NM, set.n_vertices = NV;
    set.textures = tex.get(), set.mesh_texture = mesh.get(), set.vertex_uv = uv.get();
  }
};

bool refused(const rt_texture_set& s, const char* word) { return rt_set_textures(FAKE, &s) == RT_ERR_INVALID && says(word); }

void set_checks() {
  EXPECT(rt_set_textures(nullptr, nullptr) == RT_ERR_INVALID && says("null"));
  {
    // a clean set ends at the null context, after the whole scan
    Set s;
    EXPECT(rt_set_textures(nullptr, &s.set) == RT_ERR_INVALID && says("ctx"));
  }
  { Set s; s.set.textures = nullptr; EXPECT(refused(s.set, "null")); }
  { Set s; s.set.mesh_texture = nullptr; EXPECT(refused(s.set, "null")); }
  { Set s; s.set.vertex_uv = nullptr; EXPECT(refused(s.set, "null")); }
  { Set s; s.set.n_textures = 0; EXPECT(refused(s.set, "n_textures is 0")); }
  { Set s; s.set.reserved[3] = 1; EXPECT(refused(s.set, "reserved[3]")); }
  { Set s; s.tex[1].width = 0; EXPECT(refused(s.set, "texture 1: width 0")); }
  { Set s; s.tex[1].width = 16385; EXPECT(refused(s.set, "texture 1: width 16385")); }
  { Set s; s.tex[0].height = 0; EXPECT(refused(s.set, "texture 0: height 0")); }
  { Set s; s.tex[0].height = 0xffffffffu; EXPECT(refused(s.set, "texture 0: height")); }
  { Set s; s.tex[1].wrap_s = 2; EXPECT(refused(s.set, "texture 1: wrap_s 2")); }
  { Set s; s.tex[1].wrap_t = 2; EXPECT(refused(s.set, "texture 1: wrap_t 2")); }
  { Set s; s.tex[0].filter = 2; EXPECT(refused(s.set, "texture 0: filter 2")); }
  { Set s; s.tex[0].reserved[2] = 5; s.tex[1].width = 0; EXPECT(refused(s.set, "texture 0: reserved[2]")); }
  { Set s; s.tex[1].texels = nullptr; EXPECT(refused(s.set, "texture 1: texels is null")); }
  {
    // more than 2^28 texels: told from the headers, before a texel is read (the arrays are far shorter)
    Set s;
    s.tex[0].width = s.tex[0].height = s.tex[1].width = s.tex[1].height = 16384;
    EXPECT(refused(s.set, "536870912 texels"));
  }
  const float bad[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                       -std::numeric_limits<float>::infinity()};
  for (float b : bad) {
    for (int j : {0, 22, 44}) {
      Set s;
      s.t0[j] = b, s.t1[3 * 64 * 32 - 1] = bad[0];  // (a later bad value is not the one named)
      char want[64];
      snprintf(want, sizeof want, "texture 0: texels[%d] (row %d, column %d,", j, j / 3 / 5, j / 3 % 5);
      EXPECT(refused(s.set, want));
    }
    Set s;
    s.t1[3 * 64 * 32 - 1] = b;
    EXPECT(refused(s.set, "texture 1: texels[6143] (row 31, column 63, component 2)"));
    for (uint32_t j : {0u, 1u, NV, 2u * NV - 1u}) {
      Set u;
      u.uv[j] = b, u.uv[2 * NV - 1] = bad[0];
      char want[64];
      snprintf(want, sizeof want, "vertex_uv[%u] (vertex %u, component %u)", j, j / 2u, j % 2u);
      EXPECT(refused(u.set, want));
    }
  }
  { Set s; s.uv[2 * NV - 1] = 1024.5f; EXPECT(refused(s.set, "beyond 1024")); }
  { Set s; s.uv[0] = -1025.f; EXPECT(refused(s.set, "vertex_uv[0]")); }
  { Set s; s.mesh[NM - 1] = 2; EXPECT(refused(s.set, "mesh_texture[6] is 2")); }
  { Set s; s.mesh[0] = 0xfffffffeu; s.mesh[NM - 1] = 2; EXPECT(refused(s.set, "mesh_texture[0] is 4294967294")); }
}

void frame_checks() {
  rt_params p = {};
  p.width = 5, p.height = 3, p.spp = 4, p.mode = RT_MODE_PATH, p.max_depth = 3, p.rng_mode = RT_RNG_PIXEL, p.tile = 8;
  float bg[45] = {}, out[45], acc[60];
  EXPECT(rt_render_textured(nullptr, &p, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_textured(FAKE, nullptr, bg, out, acc, nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(rt_render_textured(FAKE, &p, bg, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("neither"));
  EXPECT(rt_render_textured(FAKE, &p, nullptr, out, acc, nullptr) == RT_ERR_INVALID && says("background"));
  EXPECT(rt_render_textured_device(FAKE, &p, nullptr, nullptr, nullptr) == RT_ERR_INVALID && says("d_accum"));
  rt_params q = p;
  q.spp = 0;
  EXPECT(rt_render_textured(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_INVALID);
  q = p, q.world = 2;
  EXPECT(rt_render_textured(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED && says("world"));
  q = p, q.use_photons = 1, q.k = 4, q.photons_requested = 10;
  EXPECT(rt_render_textured_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("photon"));
  q = p, q.reserved[2] = 1;
  EXPECT(rt_render_textured_device(FAKE, &q, acc, nullptr, nullptr) == RT_ERR_UNSUPPORTED && says("wavefront"));
  q = p, q.rng_mode = RT_RNG_LEGACY;
  EXPECT(rt_render_textured(FAKE, &q, bg, out, acc, nullptr) == RT_ERR_UNSUPPORTED);
  rt_aov a = {};
  EXPECT(rt_render_aov_textured(nullptr, &p, &a) == RT_ERR_INVALID);
  EXPECT(rt_render_aov_textured_device(nullptr, &p, &a, nullptr) == RT_ERR_INVALID);
}

void write_file(const char* path, const std::string& bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(bytes.data(), (std::streamsize)bytes.size());
}

bool loads(const std::string& text, Mesh* m) {
  const char* path = "tex_host_check_tmp.off";
  write_file(path, text);
  bool ok = true;
  try {
    m->loadOFF(path);
  } catch (const std::exception& e) {
    ok = false;
    if (!strstr(e.what(), path)) ++failures, fprintf(stderr, "the loader's message does not name the file: %s\n", e.what());
  }
  remove(path);
  return ok;
}

bool reads(const std::string& bytes, TextureImage* t) {
  const char* path = "tex_host_check_tmp.ppm";
  write_file(path, bytes);
  bool ok = true;
  try {
    *t = TextureImage::loadPPM(path);
  } catch (const std::exception& e) {
    ok = false;
    if (!strstr(e.what(), path)) ++failures, fprintf(stderr, "the reader's message does not name the file: %s\n", e.what());
  }
  remove(path);
  return ok;
}

void loader_checks(const char* fixture) {
  Mesh m;
  const std::string faces = "3 0 1 2\n";
  EXPECT(loads("STOFF\n3 1 0\n0 0 0 0.25 -1.5\n1 0 0 1 0 # s t\n0 1 0 2e0 1024\n" + faces, &m));
  EXPECT(m.vertexUVs().size() == 6 && m.vertexColors().empty() && m.indexedTriangles().size() == 1 && m.vertexNormals().size() == 3);
  EXPECT(m.vertexUVs()[0] == 0.25f && m.vertexUVs()[1] == -1.5f && m.vertexUVs()[4] == 2.f && m.vertexUVs()[5] == 1024.f);
  EXPECT(m.vertexPositions()[1][0] == 1.f && m.sourceFile() == "tex_host_check_tmp.off");
  // colours (three or four values) in front of the coordinates
  EXPECT(loads("STCOFF\n3 1 0\n0 0 0 255 0 51 0.5 0.75\n1 0 0 0 255 0 7 1 0\n0 1 0 0 0 0 0 1\n" + faces, &m));
  EXPECT(m.vertexUVs().size() == 6 && m.vertexColors().size() == 3 && m.vertexColors()[0][2] == 51.f / 255.f);
  EXPECT(m.vertexUVs()[0] == 0.5f && m.vertexUVs()[1] == 0.75f && m.vertexUVs()[2] == 1.f && m.vertexUVs()[5] == 1.f);
  // a plain OFF or COFF file has none, and a mesh loaded twice forgets the coordinates of the first file
  EXPECT(loads("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n" + faces, &m) && m.vertexUVs().empty() && m.vertexColors().empty());
  EXPECT(loads("COFF\n3 1 0\n0 0 0 1 0 0.5\n1 0 0 0 1 0 1\n0 1 0 0 0 1\n" + faces, &m) && m.vertexUVs().empty() && m.vertexColors().size() == 3);
  // one or three coordinates, a colour count that does not fit, and values that are no finite decimal numbers
  EXPECT(!loads("STOFF\n3 1 0\n0 0 0 0.5\n1 0 0 1 0\n0 1 0 0 1\n" + faces, &m));
  EXPECT(!loads("STOFF\n3 1 0\n0 0 0 0.5 0.5 0.5\n1 0 0 1 0\n0 1 0 0 1\n" + faces, &m));
  EXPECT(!loads("STCOFF\n3 1 0\n0 0 0 1 2 0.5 0.5\n1 0 0 0 1 0 1 0\n0 1 0 0 0 1 0 1\n" + faces, &m));
  for (const char* bad : {"nan", "inf", "-inf", "0x1p-1", "x", "1e999"})
    EXPECT(!loads(std::string("STOFF\n3 1 0\n0 0 0 0.5 ") + bad + "\n1 0 0 1 0\n0 1 0 0 1\n" + faces, &m));
  if (fixture) {
    Mesh cube;
    cube.loadOFF(fixture);
    EXPECT(cube.vertexPositions().size() == 8 && cube.indexedTriangles().size() == 12 && cube.vertexUVs().size() == 16);
    EXPECT(cube.vertexUVs()[6] == 1.f && cube.vertexUVs()[7] == 1.f && cube.vertexUVs()[8] == -0.5f && cube.vertexUVs()[15] == 1.625f);
  }
}

void ppm_checks(const char* fixture) {
  TextureImage t;
  EXPECT(reads("P3\n# c\n2 3 # w h\n255\n255 0 51  0 0 0\n1 2 3  4 5 6\n7 8 9  10 11 255\n", &t));
  EXPECT(t.width == 2 && t.height == 3 && t.texels.size() == 18 && t.texels[0] == 1.f && t.texels[2] == 51.f / 255.f &&
         t.texels[6] == 1.f / 255.f && t.texels[17] == 1.f);
  // binary: one white-space byte, then the raster — whose bytes may be white space, '#' or 255 themselves
  std::string p6 = "P6 3 2\n255\n";
  const unsigned char raster[18] = {255, 0, 51, '#', ' ', '\n', 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 255};
  p6.append(reinterpret_cast<const char*>(raster), 18);
  EXPECT(reads(p6, &t));
  EXPECT(t.width == 3 && t.height == 2 && t.texels.size() == 18 && t.texels[0] == 1.f && t.texels[3] == 35.f / 255.f &&
         t.texels[4] == 32.f / 255.f && t.texels[5] == 10.f / 255.f && t.texels[17] == 1.f);
  EXPECT(!reads(p6.substr(0, p6.size() - 1), &t));                      // one byte short
  EXPECT(!reads("P3\n2 1\n255\n1 2 3 4 5\n", &t));                      // one value short
  EXPECT(!reads("P3\n2 1\n255\n1 2 3 4 5 256\n", &t));                  // a value above 255
  EXPECT(!reads("P3\n2 1\n255\n1 2 3 4 x 6\n", &t));                    // no number
  EXPECT(!reads("P3\n2 1\n255\n1 2 3 4 -5 6\n", &t));
  EXPECT(!reads("P3\n2 1\n65535\n1 2 3 4 5 6\n", &t));                  // another maxval
  EXPECT(!reads("P3\n0 1\n255\n", &t) && !reads("P3\n1 16385\n255\n", &t) && !reads("P3\n99999999 1\n255\n", &t));
  EXPECT(!reads("P5\n1 1\n255\n1\n", &t) && !reads("P", &t) && !reads("", &t) && !reads("P6 1 1 255", &t));
  try {
    TextureImage::loadPPM("tex_host_check_no_such_file.ppm");
    EXPECT(!"a missing file is refused");
  } catch (const std::exception&) {
  }
  if (fixture) {
    const TextureImage f = TextureImage::loadPPM(fixture);
    EXPECT(f.width == 4 && f.height == 3 && f.texels[0] == 1.f && f.texels[1] == 0.f && f.texels[12] == 40.f / 255.f &&
           f.texels[35] == 1.f);
    // the image as a set of its own passes rt_set_textures' argument checks
    rt_texture x = {};
    x.width = f.width, x.height = f.height, x.filter = RT_TEX_BILINEAR, x.texels = f.texels.data();
    const uint32_t mesh[1] = {0};
    const float uv[2] = {0.5f, 0.5f};
    rt_texture_set s = {};
    s.n_textures = 1, s.n_meshes = 1, s.n_vertices = 1, s.textures = &x, s.mesh_texture = mesh, s.vertex_uv = uv;
    EXPECT(rt_set_textures(nullptr, &s) == RT_ERR_INVALID && says("ctx"));
  }
}

}  // namespace

int main(int argc, char** argv) {
  set_checks();
  frame_checks();
  loader_checks(argc > 1 ? argv[1] : nullptr);
  ppm_checks(argc > 2 ? argv[2] : nullptr);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("tex_host_check: all checks passed\n");
  return 0;
}
