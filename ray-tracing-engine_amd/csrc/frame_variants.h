// frame_variants.h — the frame integrator with another generator, another split of its samples or another light list:
// rt_render_lens, rt_render_shutter, rt_render_views_shutter, rt_render_lights (DESIGN.md §6m–§6p), rt_render_pick (§6r)
// and, with another albedo at every vertex, rt_render_colors (§6t), rt_render_textured (§6u), both under the multi-view
// shutter's generator, rt_render_views_shutter_albedo (§6v), and, with a whole material at every vertex, rt_render_material
// (§6w), and with a tangent-space normal map turning every vertex's shading normal, rt_render_normal_mapped (§6y).
//
// Every variant is render_tile itself under one more LT_* bit, on the one-wave-per-workgroup family that k_render serves:
// brute, sequential and pooled, each counted (STATS, one wave per SIMD) and timed (four waves per SIMD, k_render's target);
// none with LT_FASTDET (they divide: the operand bounds of the short forms were proved for the context's camera only),
// none persistent.  The lane layout, the sample hand-over and the vertex pool are the frame's, so reserved[0] and
// reserved[1] mean what they mean there.  What a variant's kernels read beyond the frame's arguments travels as ONE
// record, a kernel argument of its own (k_render_rec): RenderArgs and the frame's entry points stay as they are, and a
// test on the record is a scalar one.
//   lens          LT_LENS                LensRec: lens_ray in place of camera_ray where aperture > 0 (a wave-uniform test;
//                                        aperture == 0 is rt_render's frame bit for bit)
//   shutter       LT_SHUTTER             ShutterRec: every sample draws a time, forms its camera in registers and casts
//                                        that camera's primary ray by shutter_ray, through the lens where aperture > 0
//   light groups  LT_LIGHTS              LightGroupsRec: everything up to the light loop of a vertex runs ONCE for all
//                                        groups, which differ only in the terms added (vertex_pool's and shade_direct_seq's
//                                        GROUPS switch); the sample hand-over grows to LG_EX_ROWS rows (group_samples_add)
//   views+shutter LT_VIEWS | LT_SHUTTER  no record: the tile's view picks its ViewRec and, from the table parallel to
//                                        views (RenderArgs::viewShutters), its shutter record, by scalar loads; these are
//                                        plain k_render instances
//   light picks   LT_PICK                PickRec: every sample draws m <= POOL_L indices into the record's table of scaled
//                                        lights and all of its vertices shade with those (vertex_pool's and
//                                        shade_direct_seq's PICK switch): pooled whatever the scene's light count
// Those are the GENERATOR parts: what forms a sample's primary ray, splits its samples or lists its lights.  The SURFACE
// parts are rt_kernels.hip's surface policies, what a path vertex shades with:
//   vertex colours SurfVCol (LT_VCOL)    VColRec: every shaded vertex forms its kdDiffuse from the colours of the hit
//                                        triangle's vertices (vertex_kd) and shades with it (vertex_pool's and
//                                        shade_direct_seq's VC switch), parked in three rows of LDS over every walk
//   textures      SurfTex (LT_TEX)       TexRec: every shaded vertex of a mesh with a texture forms its kdDiffuse from
//                                        the texture's sample at the hit's uv (tex_kd), in the same three rows
//   material maps SurfMat (LT_MAT)       MatRec: every shaded vertex forms its whole material from up to three samples
//                                        at the hit's uv (tex_mat: albedo, f0, (kd, alpha)), parked in eight rows, and
//                                        shades with bsdf_base(const rt_material&) of it
//   normal maps   SurfNrm (LT_NMAP)      NrmRec: the material-map frame's vertex (tex_mat, the same eight rows; without
//                                        resident material maps the two tables are kTexNone everywhere) whose shading
//                                        normal is replaced at the set-up, before anything reads it, by the one the
//                                        mesh's normal map turns in the triangle's tangent frame (nmap_bend): the
//                                        light terms, the BSDF and the bounce use that, so the paths are its own
// A variant is one generator part with one surface part (Variant<G, SF>): its LT_* bits are the OR of theirs, its record
// the one part's that has one, its LDS the generator's stack rows and the surface's parked rows.  The two meet nowhere in
// render_tile: the sample's primary ray is complete before the first vertex reads the surface's record.  variant_exists
// says which pairs are compiled: every generator alone, every surface under the plain generator, and the colours and the
// textures under views+shutter (rt_render_views_shutter_albedo); the launcher refuses every other pair.
// A new generator supplies a Gen* row below (its LT_* bits, its record, the stack rows its sample hand-over needs, its
// argument check), a FrameVariant::Gen and a case in launch_render_variant.  A new surface supplies a policy in
// rt_kernels.hip, a FrameVariant::Surface and a case in launch_surface; a new pair, a term in variant_exists.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

static_assert(LG_EX_ROWS * BLOCK <= VP_WORDS, "the pooled instances hand the groups' samples over in the pool's words");

// the fewest stack rows of a launch whose waves park a value behind them (the ROWS and ROWS_POOLED of their generators)
constexpr uint32_t kParkMinRows = 4;

// k_render (no photons) with the variant's record R beside its arguments
template <bool BRUTE, bool POOLED, bool STATS, int MINW, int LTV, class REC>
__global__ __launch_bounds__(BLOCK, MINW) void k_render_rec(DevScene S, RenderArgs A, REC R, float4* __restrict__ accum,
                                                            unsigned long long* __restrict__ counters) {
  static_assert(!POOLED || !BRUTE, "the vertex pool serves BVH direct lighting");
  // dynamic LDS as k_render's: [levels][64] traversal stack, then (POOLED) the ray pool; without a pool the sample
  // hand-over area lies in the first stack rows
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<false>(lds, A.stackLevels, 0);
  uint32_t* pool = lds + A.stackLevels * BLOCK;
  float* ex = reinterpret_cast<float*>(POOLED ? pool : lds);
  // then (a surface with rows) the rows where a vertex's value is parked: behind everything launch_variant2 allocates
  // before them — max(stackLevels, kParkMinRows) stack rows and, with one, the pool
  float* park = nullptr;
  if constexpr (surface_t<LTV>::Parked::ROWS != 0)
    park = reinterpret_cast<float*>(lds + (A.stackLevels < kParkMinRows ? kParkMinRows : A.stackLevels) * BLOCK + (POOLED ? VP_WORDS : 0));
  LaneStats st;
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t) render_tile<BRUTE, false, POOLED, STATS, LTV>(S, A, accum, L, pool, ex, t, st, &R, park);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_variant2 folds the stripes)
}

// The generators' rows.  ROWS, ROWS_POOLED: the fewest stack rows a launch without / with a vertex pool allocates (the
// hand-over area lies in the stack rows without a pool, in the pool's words with one: launch_render2's four in both
// cases, LG_EX_ROWS and none for the light groups).  refused: the arguments the launcher answers hipErrorInvalidValue to.
struct GenPlain {
  static constexpr int LT = 0;
  using Rec = NoRec;
  static constexpr uint32_t ROWS = 4, ROWS_POOLED = 4;
  static bool refused(const DevScene&, const RenderArgs& A, const Rec&) { return A.tileView != nullptr; }
};
struct GenLens {
  static constexpr int LT = LT_LENS;
  using Rec = LensRec;
  static constexpr uint32_t ROWS = 4, ROWS_POOLED = 4;
  static bool refused(const DevScene&, const RenderArgs& A, const Rec&) { return A.tileView != nullptr; }  // (no multi-view lens frames)
};
struct GenShutter {
  static constexpr int LT = LT_SHUTTER;
  using Rec = ShutterRec;
  static constexpr uint32_t ROWS = 4, ROWS_POOLED = 4;
  static bool refused(const DevScene&, const RenderArgs& A, const Rec&) { return A.tileView != nullptr; }  // (those are GenViewsShutter's)
};
struct GenLights {
  static constexpr int LT = LT_LIGHTS;
  using Rec = LightGroupsRec;
  static constexpr uint32_t ROWS = LG_EX_ROWS, ROWS_POOLED = 0;
  static bool refused(const DevScene& S, const RenderArgs& A, const Rec& G) {
    return A.tileView || G.n < 1u || G.n > (uint32_t)RT_LIGHT_GROUPS_MAX || S.n_lights > 32u;
  }
};
struct GenPick {
  static constexpr int LT = LT_PICK;
  using Rec = PickRec;
  static constexpr uint32_t ROWS = 4, ROWS_POOLED = 4;
  static bool refused(const DevScene&, const RenderArgs& A, const Rec& R) {
    return A.tileView || R.m < 1u || R.m > (uint32_t)RT_PICK_SLOTS_MAX || R.n == 0u || !R.thresholds || !R.lights;
  }
};
struct GenViewsShutter {
  static constexpr int LT = LT_VIEWS | LT_SHUTTER;
  using Rec = NoRec;
  static constexpr uint32_t ROWS = 4, ROWS_POOLED = 4;
  // (the three tables of a multi-view shutter frame)
  static bool refused(const DevScene&, const RenderArgs& A, const Rec&) { return !A.tileView || !A.views || !A.viewShutters; }
};

// the pairs that are compiled, by the parts' LT_* bits ((0, 0), the plain frame itself, is launch_render's)
constexpr bool variant_exists(int gen, int surface) {
  // (every surface, SurfNrm among them, under the plain generator; the two albedo surfaces under views+shutter too)
  return surface == 0 || gen == 0 || (gen == (LT_VIEWS | LT_SHUTTER) && (surface == LT_VCOL || surface == LT_TEX));
}

// generator G with surface SF
template <class G, class SF>
struct Variant {
  static constexpr bool SURFACE = SF::LT != 0;
  static_assert(!SURFACE || std::is_same_v<typename G::Rec, NoRec>, "k_render_rec takes one record: the generator's or the surface's");
  static constexpr int LTV = G::LT | SF::LT;
  using Rec = std::conditional_t<SURFACE, typename SF::Rec, typename G::Rec>;
  static constexpr uint32_t ROWS = G::ROWS, ROWS_POOLED = G::ROWS_POOLED;
  static constexpr uint32_t PARK_WORDS = SF::Parked::ROWS * 64;  // (the vertex's value behind the stack rows and pool: k_render_rec's `park`)
  static bool refused(const DevScene& S, const RenderArgs& A, const Rec& R) {
    if constexpr (SURFACE) return G::refused(S, A, NoRec()) || SF::refused(R);
    else return G::refused(S, A, R);
  }
};

template <class V, bool BRUTE, bool POOLED, bool STATS, int MINW>
static void launch_variant_instance(size_t ldsBytes, hipStream_t stream, const DevScene& S, const RenderArgs& A,
                                    const typename V::Rec& R, float4* accum, unsigned long long* counters) {
  if constexpr (std::is_same_v<typename V::Rec, NoRec>)
    hipLaunchKernelGGL((k_render<BRUTE, false, POOLED, STATS, MINW, V::LTV>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A, accum, counters);
  else
    hipLaunchKernelGGL((k_render_rec<BRUTE, POOLED, STATS, MINW, V::LTV, typename V::Rec>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A, R, accum, counters);
}

template <class V, bool BRUTE, bool POOLED>
static hipError_t launch_variant2(bool stats, const DevScene& S, const RenderArgs& A, const typename V::Rec& R, float4* accum,
                                  unsigned long long* counters, hipStream_t stream) {
  if (A.n_tiles == 0) return hipSuccess;
  constexpr uint32_t minRows = POOLED ? V::ROWS_POOLED : V::ROWS;
  constexpr uint32_t parkWords = V::PARK_WORDS;
  static_assert(parkWords == 0 || minRows == kParkMinRows, "k_render_rec places the parked rows behind kParkMinRows stack rows at least");
  const size_t ldsBytes = 4u * ((A.stackLevels < minRows ? minRows : A.stackLevels) * BLOCK + (POOLED ? VP_WORDS : 0) + parkWords);
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;
  if (stats) {
    launch_variant_instance<V, BRUTE, POOLED, true, 1>(ldsBytes, stream, S, A1, R, accum, counters);
  } else {
    launch_variant_instance<V, BRUTE, POOLED, false, 4>(ldsBytes, stream, S, A1, R, accum, counters);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
  return hipGetLastError();
}

template <class V>
static hipError_t launch_variant(bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, const typename V::Rec& R,
                                 float4* accum, unsigned long long* counters, hipStream_t stream) {
  if (V::refused(S, A, R)) return hipErrorInvalidValue;
  if (brute_force) return launch_variant2<V, true, false>(stats, S, A, R, accum, counters, stream);
  // the vertex pool handles up to POOL_L lights, as in launch_render; a picked frame's vertex has m <= POOL_L of them
  // whatever the scene's count
  constexpr bool anyCount = (V::LTV & LT_PICK) != 0;
  if ((A.flags & 1u) && (anyCount || S.n_lights <= (uint32_t)POOL_L)) return launch_variant2<V, false, true>(stats, S, A, R, accum, counters, stream);
  return launch_variant2<V, false, false>(stats, S, A, R, accum, counters, stream);
}

// F's launch under generator G: by F's surface, the pairs that exist
template <class G, class SF>
static hipError_t launch_pair(const FrameVariant& F, bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, float4* accum,
                              unsigned long long* counters, hipStream_t stream) {
  if constexpr (!variant_exists(G::LT, SF::LT) || (G::LT | SF::LT) == 0) return hipErrorInvalidValue;  // (nothing of the pair is instantiated)
  else {
    using V = Variant<G, SF>;
    if constexpr (std::is_same_v<typename V::Rec, NoRec>) return launch_variant<V>(brute_force, stats, S, A, NoRec(), accum, counters, stream);
    else return launch_variant<V>(brute_force, stats, S, A, *static_cast<const typename V::Rec*>(F.rec), accum, counters, stream);
  }
}
template <class G>
static hipError_t launch_surface(const FrameVariant& F, bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, float4* accum,
                                 unsigned long long* counters, hipStream_t stream) {
  switch (F.surface) {
    case FrameVariant::NONE: return launch_pair<G, SurfNone>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::VCOL: return launch_pair<G, SurfVCol>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::TEX: return launch_pair<G, SurfTex>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::MAT: return launch_pair<G, SurfMat>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::NMAP: return launch_pair<G, SurfNrm>(F, brute_force, stats, S, A, accum, counters, stream);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_render_variant(const FrameVariant& F, bool brute_force, bool stats, const DevScene& S, const RenderArgs& A,
                                 float4* accum, unsigned long long* counters, hipStream_t stream) {
  switch (F.gen) {
    case FrameVariant::PLAIN: return launch_surface<GenPlain>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::LENS: return launch_surface<GenLens>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::SHUTTER: return launch_surface<GenShutter>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::LIGHTS: return launch_surface<GenLights>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::PICK: return launch_surface<GenPick>(F, brute_force, stats, S, A, accum, counters, stream);
    case FrameVariant::VIEWS_SHUTTER: return launch_surface<GenViewsShutter>(F, brute_force, stats, S, A, accum, counters, stream);
  }
  return hipErrorInvalidValue;
}
