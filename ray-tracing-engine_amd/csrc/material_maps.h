// material_maps.h — the host side of rt_set_material_maps that needs no device: what an rt_material_maps
// says of itself, and the two per-mesh tables the context keeps.  Plain C++ over the caller's arrays, shared by rt_api.cpp
// and tools/mat_host_check.cpp (which runs it under the sanitizers).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "rt_amd.h"

namespace rtmat {

// the first non-zero reserved word of the maps, or -1
inline int first_reserved(const rt_material_maps& m) {
  for (int k = 0; k < 5; ++k)
    if (m.reserved[k]) return k;
  return -1;
}

// the tables rt_render_material's kernels read: one texture index or RT_TEX_NONE per mesh for f0 and for (kd, alpha)
struct Tables {
  std::vector<uint32_t> f0, kdAlpha;
};

// Builds the tables of m for a resident set of nTextures textures: a null table of m is RT_TEX_NONE on every mesh.
// false, with *why naming the table and the mesh of the first entry that is neither an index below nTextures nor
// RT_TEX_NONE: mesh_f0 is scanned before mesh_kd_alpha, each in mesh order, and exactly n_meshes entries of each are read.
inline bool build_tables(const rt_material_maps& m, uint32_t nTextures, Tables* out, std::string* why) {
  const uint32_t* const src[2] = {m.mesh_f0, m.mesh_kd_alpha};
  const char* const name[2] = {"mesh_f0", "mesh_kd_alpha"};
  std::vector<uint32_t>* const dst[2] = {&out->f0, &out->kdAlpha};
  for (int t = 0; t < 2; ++t) {
    dst[t]->assign(m.n_meshes, RT_TEX_NONE);
    if (!src[t]) continue;
    for (uint32_t i = 0; i < m.n_meshes; ++i) {
      const uint32_t x = src[t][i];
      if (x != RT_TEX_NONE && x >= nTextures) {
        char buf[160];
        snprintf(buf, sizeof buf, "material maps: %s[%u] is %u: neither one of %u textures nor RT_TEX_NONE", name[t], i, x, nTextures);
        *why = buf;
        return false;
      }
      (*dst[t])[i] = x;
    }
  }
  return true;
}

}  // namespace rtmat
