// lights_kernels.h — the frame split by light group: rt_render_lights.
//
// The frame integrator itself, render_tile, with one colour per light group at every vertex (LT_LIGHTS).  Everything up
// to the light loop of a vertex — the stream, the jitter, the camera ray, every cast, the light draws and the hemisphere
// draws — runs ONCE for all groups: the frame "with only these lights lit" shares every ray and every random draw with
// the full frame and differs only in which terms are added (vertex_pool's and shade_direct_seq's GROUPS switch:
// group_cols_add).  The lane layout and the vertex pool are the frame's, so reserved[0] and reserved[1] mean what they
// mean there; the sample hand-over grows to LG_EX_ROWS rows (group_samples_add).  The group record travels as a kernel
// argument of its own, so the mask tests are scalar.  The instances mirror k_render_lens': brute, sequential and pooled,
// each counted (STATS, one wave per SIMD) and timed (four waves per SIMD); none with LT_FASTDET, none persistent.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

static_assert(LG_EX_ROWS * BLOCK <= VP_WORDS, "the pooled instances hand the groups' samples over in the pool's words");

template <bool BRUTE, bool POOLED, bool STATS, int MINW>
__global__ __launch_bounds__(BLOCK, MINW) void k_render_lights(DevScene S, RenderArgs A, LightGroupsRec G, float4* __restrict__ accum,
                                                               unsigned long long* __restrict__ counters) {
  static_assert(!POOLED || !BRUTE, "the vertex pool serves BVH direct lighting");
  // dynamic LDS as k_render's: [levels][64] traversal stack (at least LG_EX_ROWS rows without a pool: the hand-over area
  // lies in the stack rows there), then (POOLED) the ray pool
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<false>(lds, A.stackLevels, 0);
  uint32_t* pool = lds + A.stackLevels * BLOCK;
  float* ex = reinterpret_cast<float*>(POOLED ? pool : lds);
  LaneStats st;
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t)
    render_tile<BRUTE, false, POOLED, STATS, LT_LIGHTS>(S, A, accum, L, pool, ex, t, st, nullptr, nullptr, &G);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_render_lights folds the stripes)
}

template <bool BRUTE, bool POOLED>
static hipError_t launch_render_lights2(bool stats, const DevScene& S, const RenderArgs& A, const LightGroupsRec& G, float4* accum,
                                        unsigned long long* counters, hipStream_t stream) {
  if (A.n_tiles == 0) return hipSuccess;
  // (the instances without a pool hand the samples over in their stack rows: LG_EX_ROWS of them at least, where the
  // single frame needs four)
  const uint32_t rows = POOLED || A.stackLevels >= (uint32_t)LG_EX_ROWS ? A.stackLevels : (uint32_t)LG_EX_ROWS;
  const size_t ldsBytes = 4u * (rows * BLOCK + (POOLED ? VP_WORDS : 0));
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;
  if (stats) {
    hipLaunchKernelGGL((k_render_lights<BRUTE, POOLED, true, 1>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, G, accum, counters);
  } else {
    hipLaunchKernelGGL((k_render_lights<BRUTE, POOLED, false, 4>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, G, accum, counters);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
  return hipGetLastError();
}

hipError_t launch_render_lights(bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, const LightGroupsRec& G,
                                float4* accum, unsigned long long* counters, hipStream_t stream) {
  if (A.tileView || G.n < 1u || G.n > (uint32_t)RT_LIGHT_GROUPS_MAX || S.n_lights > 32u) return hipErrorInvalidValue;
  if (brute_force) return launch_render_lights2<true, false>(stats, S, A, G, accum, counters, stream);
  // the vertex pool handles up to POOL_L lights, as in launch_render
  if ((A.flags & 1u) && S.n_lights <= (uint32_t)POOL_L) return launch_render_lights2<false, true>(stats, S, A, G, accum, counters, stream);
  return launch_render_lights2<false, false>(stats, S, A, G, accum, counters, stream);
}
