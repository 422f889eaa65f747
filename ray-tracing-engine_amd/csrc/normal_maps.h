// normal_maps.h — the host side of rt_set_normal_maps that needs no device: what an rt_normal_maps says
// of itself, and the per-mesh table the context keeps.  Plain C++ over the caller's array, shared by rt_api.cpp and
// tools/nmap_host_check.cpp (which runs it under the sanitizers).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "rt_amd.h"

namespace rtnrm {

constexpr int kReservedWords = (int)(sizeof(rt_normal_maps::reserved) / sizeof(uint32_t));

// the first non-zero reserved word of the maps, or -1
inline int first_reserved(const rt_normal_maps& m) {
  for (int k = 0; k < kReservedWords; ++k)
    if (m.reserved[k]) return k;
  return -1;
}

// Builds the table rt_render_normal_mapped's kernels read — one texture index or RT_TEX_NONE per mesh — of m for a
// resident set of nTextures textures: a null mesh_normal is RT_TEX_NONE on every mesh.  false, with *why naming the mesh
// of the first entry that is neither an index below nTextures nor RT_TEX_NONE; exactly n_meshes entries are read.
inline bool build_table(const rt_normal_maps& m, uint32_t nTextures, std::vector<uint32_t>* out, std::string* why) {
  out->assign(m.n_meshes, RT_TEX_NONE);
  if (!m.mesh_normal) return true;
  for (uint32_t i = 0; i < m.n_meshes; ++i) {
    const uint32_t x = m.mesh_normal[i];
    if (x != RT_TEX_NONE && x >= nTextures) {
      char buf[160];
      snprintf(buf, sizeof buf, "normal maps: mesh_normal[%u] is %u: neither one of %u textures nor RT_TEX_NONE", i, x, nTextures);
      *why = buf;
      return false;
    }
    (*out)[i] = x;
  }
  return true;
}

}  // namespace rtnrm
