// skin_host_check.cpp — the host side of rt_set_skin and rt_update_skin as a stand-alone program, for sanitizer runs on the
// CPU (no GPU, no Python).  It covers what runs without a device: every rejection that the arguments alone decide — each
// is answered before the context is looked at, so the context is NULL throughout and a clean call ends at "ctx is null" —
// and rt_set_skin's scan of the index and weight arrays, over arrays of exactly n_vertices x 4 elements on the heap, so
// that a scan that reads one element too many is the sanitizer's to report.
//
// rt_api.cpp and bvh_build.cpp are compiled with the sanitizers; the kernels' objects come from the product's build
// (make -C ray-tracing-engine_amd) through an archive, from the repository root:
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/skin_host_check.cpp ray-tracing-engine_amd/csrc/rt_api.cpp ray-tracing-engine_amd/csrc/bvh_build.cpp; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -ffp-contract=off -pthread -Iinclude -Iray-tracing-engine_amd/csrc \
//         -c $f -o $(basename $f).o; done
//   ar rcs kernels.a ray-tracing-engine_amd/build/*.hip.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread skin_host_check.cpp.o rt_api.cpp.o bvh_build.cpp.o \
//       -Wl,--whole-archive kernels.a -Wl,--no-whole-archive -o skin_host_check
//   ./skin_host_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

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

constexpr uint32_t NV = 5003, NB = 97;  // (no multiple of anything)

struct Skin {
  std::unique_ptr<uint16_t[]> bone{new uint16_t[4 * NV]};
  std::unique_ptr<float[]> weight{new float[4 * NV]};
  rt_skin s = {};
  explicit Skin(uint32_t nBones = NB) {
    uint32_t x = 12345u;
    for (uint32_t i = 0; i < 4 * NV; ++i) {
      x = x * 1664525u + 1013904223u;
      bone[i] = (uint16_t)((x >> 8) % nBones);
      weight[i] = (x >> 28) == 0 ? (i & 1 ? -0.f : 0.f) : 0.1f + 0.8f * (float)(x >> 8 & 0xffff) / 65536.f;
    }
    s.n_vertices = NV, s.n_bones = nBones, s.bone = bone.get(), s.weight = weight.get();
  }
};

// a clean call gets as far as the context, which is NULL here
bool reaches_ctx(const rt_skin& s) { return rt_set_skin(nullptr, &s) == RT_ERR_INVALID && says("ctx/skin is null"); }

void check_set_skin() {
  EXPECT(rt_set_skin(nullptr, nullptr) == RT_ERR_INVALID && says("null"));
  {
    Skin k;
    EXPECT(reaches_ctx(k.s));
    rt_skin x = k.s;
    x.bone = nullptr;
    EXPECT(rt_set_skin(nullptr, &x) == RT_ERR_INVALID && says("bone/weight is null"));
    x = k.s, x.weight = nullptr;
    EXPECT(rt_set_skin(nullptr, &x) == RT_ERR_INVALID && says("bone/weight is null"));
    for (int r = 0; r < 6; ++r) {
      x = k.s, x.reserved[r] = 1u << r;
      EXPECT(rt_set_skin(nullptr, &x) == RT_ERR_INVALID && says("reserved"));
    }
    for (uint32_t n : {0u, 65537u, 0xffffffffu}) {
      x = k.s, x.n_bones = n;
      EXPECT(rt_set_skin(nullptr, &x) == RT_ERR_INVALID && says("n_bones"));
    }
    // the arrays are not read beyond n_vertices, nor at all when there are none
    x = k.s, x.n_vertices = 0;
    EXPECT(reaches_ctx(x));
  }
  // the scan: a non-finite weight names its vertex, first and last vertex and every slot
  const float bad[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
  for (float b : bad)
    for (uint32_t v : {0u, 2501u, NV - 1})
      for (uint32_t slot = 0; slot < 4; ++slot) {
        Skin k;
        k.weight[4 * v + slot] = b;
        EXPECT(rt_set_skin(nullptr, &k.s) == RT_ERR_INVALID && says("non-finite") && says(("vertex " + std::to_string(v) + ":").c_str()));
        rt_skin x = k.s;
        x.n_vertices = v;  // (the vertices before it are clean)
        EXPECT(reaches_ctx(x));
      }
  // ... an index names its vertex and slot, under a weight of zero too
  for (float w : {0.f, -0.f, 0.5f})
    for (uint32_t v : {0u, 2501u, NV - 1})
      for (uint32_t slot = 0; slot < 4; ++slot) {
        Skin k;
        k.bone[4 * v + slot] = NB, k.weight[4 * v + slot] = w;
        EXPECT(rt_set_skin(nullptr, &k.s) == RT_ERR_INVALID && says(("vertex " + std::to_string(v) + " slot " + std::to_string(slot)).c_str()));
        k.s.n_bones = NB + 1;
        EXPECT(reaches_ctx(k.s));
      }
  // the first offender in vertex order is the one named; within a vertex the weights come first
  {
    Skin k;
    k.bone[4 * 40 + 1] = NB, k.weight[4 * 41 + 0] = bad[0], k.bone[4 * 4000 + 3] = 60000;
    EXPECT(rt_set_skin(nullptr, &k.s) == RT_ERR_INVALID && says("vertex 40 slot 1"));
    k.weight[4 * 40 + 3] = bad[1];
    EXPECT(rt_set_skin(nullptr, &k.s) == RT_ERR_INVALID && says("vertex 40:") && says("non-finite"));
  }
  // the whole range of a uint16 under 65,536 bones
  {
    Skin k(65536);
    k.bone[4 * (NV - 1) + 3] = 65535, k.bone[0] = 65535;
    EXPECT(reaches_ctx(k.s));
    k.s.n_bones = 65535;
    EXPECT(rt_set_skin(nullptr, &k.s) == RT_ERR_INVALID && says("vertex 0 slot 0"));
  }
}

struct Bones {
  uint32_t n;
  std::unique_ptr<rt_mesh_transform[]> t;
  rt_skin_update u = {};
  explicit Bones(uint32_t n_ = NB) : n(n_), t(new rt_mesh_transform[n_]) {
    for (uint32_t j = 0; j < n; ++j) {
      rt_mesh_transform r = {};
      for (int i = 0; i < 3; ++i) r.m[i][i] = r.n[i][i] = 1.f + 0.01f * (float)j, r.m[i][3] = 0.001f * (float)j;
      t[j] = r;
    }
    u.bones = t.get(), u.n_bones = n;
  }
};

int update(const rt_skin_update* u, bool withReport = true) {
  rt_update_report rep;
  memset(&rep, 0x5a, sizeof rep);
  const int rc = rt_update_skin(nullptr, u, nullptr, withReport ? &rep : nullptr);
  const rt_update_report zero = {};
  if (withReport) EXPECT(memcmp(&rep, &zero, sizeof rep) == 0);  // a rejected call reports nothing
  return rc;
}

void check_update_skin() {
  EXPECT(update(nullptr) == RT_ERR_INVALID && says("null"));
  EXPECT(update(nullptr, false) == RT_ERR_INVALID);
  Bones clean;
  EXPECT(update(&clean.u) == RT_ERR_INVALID && says("ctx/update is null"));
  EXPECT(update(&clean.u, false) == RT_ERR_INVALID && says("ctx/update is null"));
  rt_skin_update x = clean.u;
  x.bones = nullptr;
  EXPECT(update(&x) == RT_ERR_INVALID && says("bones is null"));
  for (int r = 0; r < 6; ++r) {
    x = clean.u, x.reserved[r] = 7;
    EXPECT(update(&x) == RT_ERR_INVALID && says("reserved"));
  }
  x = clean.u, x.n_lights = 3;
  EXPECT(update(&x) == RT_ERR_INVALID && says("lights is null"));
  x = clean.u, x.n_bones = 0;  // (no bone is read; the count is the context's to judge)
  EXPECT(update(&x) == RT_ERR_INVALID && says("ctx/update is null"));
  for (uint32_t j : {0u, 50u, NB - 1}) {
    for (uint32_t flags : {1u, 2u, 0x80000000u}) {
      Bones b;
      b.t[j].flags = flags;
      EXPECT(update(&b.u) == RT_ERR_INVALID && says("flags") && says(("bone " + std::to_string(j) + ":").c_str()));
      b.u.n_bones = j;
      EXPECT(update(&b.u) == RT_ERR_INVALID && says("ctx/update is null"));
    }
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()})
      for (int e = 0; e < 21; ++e) {
        Bones b;
        (e < 12 ? b.t[j].m[e / 4][e % 4] : b.t[j].n[(e - 12) / 3][(e - 12) % 3]) = bad;
        EXPECT(update(&b.u) == RT_ERR_INVALID && says("non-finite") && says(("bone " + std::to_string(j) + ":").c_str()));
      }
  }
  // bones in order, and the flags of a bone before its entries
  Bones b;
  b.t[7].flags = 1, b.t[7].m[0][0] = std::numeric_limits<float>::quiet_NaN(), b.t[9].n[2][2] = std::numeric_limits<float>::infinity();
  EXPECT(update(&b.u) == RT_ERR_INVALID && says("bone 7:") && says("flags"));
  b.t[5].n[1][1] = -std::numeric_limits<float>::infinity();
  EXPECT(update(&b.u) == RT_ERR_INVALID && says("bone 5:") && says("non-finite"));
}

}  // namespace

int main() {
  check_set_skin();
  check_update_skin();
  if (failures) {
    fprintf(stderr, "FAILED: %d checks\n", failures);
    return 1;
  }
  printf("skin_host_check: argument rejections and the skin scan ok\n");
  return 0;
}
