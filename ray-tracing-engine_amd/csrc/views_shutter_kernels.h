// views_shutter_kernels.h — many views of one scene, each under its own open shutter, in one launch:
// rt_render_views_shutter.
//
// render_tile with LT_VIEWS | LT_SHUTTER: the wave tile's view index picks the view's camera, stream key and accumulator
// slice from RenderArgs::views as in a multi-view frame, and the view's shutter record from RenderArgs::viewShutters, a
// table parallel to views (ViewRec stays 64 bytes).  Both records are read by scalar loads and stay in SGPRs, so
// `aperture > 0` is a wave-uniform branch per tile and views with and without a lens share a launch.  shutter_ray then
// runs on the view's camera and seed exactly as k_render_shutter runs it on the context's.  No record travels as a kernel
// argument.  The instances mirror k_render_shutter's: brute, sequential and pooled, each counted (STATS, one wave per
// SIMD) and timed (four waves per SIMD); none with LT_FASTDET, none persistent.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

template <bool BRUTE, bool POOLED, bool STATS, int MINW>
__global__ __launch_bounds__(BLOCK, MINW) void k_render_views_shutter(DevScene S, RenderArgs A, float4* __restrict__ accum,
                                                                      unsigned long long* __restrict__ counters) {
  static_assert(!POOLED || !BRUTE, "the vertex pool serves BVH direct lighting");
  // dynamic LDS as k_render's: [levels][64] traversal stack, then (POOLED) the ray pool
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<false>(lds, A.stackLevels, 0);
  uint32_t* pool = lds + A.stackLevels * BLOCK;
  float* ex = reinterpret_cast<float*>(POOLED ? pool : lds);
  LaneStats st;
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t) render_tile<BRUTE, false, POOLED, STATS, LT_VIEWS | LT_SHUTTER>(S, A, accum, L, pool, ex, t, st);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_render_views_shutter folds the stripes)
}

template <bool BRUTE, bool POOLED>
static hipError_t launch_render_views_shutter2(bool stats, const DevScene& S, const RenderArgs& A, float4* accum,
                                               unsigned long long* counters, hipStream_t stream) {
  if (A.n_tiles == 0) return hipSuccess;
  // (launch_render2's sizes: at least four rows for the sample hand-over of the instances without a pool)
  const size_t ldsBytes = 4u * ((A.stackLevels < 4u ? 4u : A.stackLevels) * BLOCK + (POOLED ? VP_WORDS : 0));
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;
  if (stats) {
    hipLaunchKernelGGL((k_render_views_shutter<BRUTE, POOLED, true, 1>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, accum, counters);
  } else {
    hipLaunchKernelGGL((k_render_views_shutter<BRUTE, POOLED, false, 4>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, accum, counters);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
  return hipGetLastError();
}

hipError_t launch_render_views_shutter(bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, float4* accum,
                                       unsigned long long* counters, hipStream_t stream) {
  if (!A.tileView || !A.views || !A.viewShutters) return hipErrorInvalidValue;  // (the three tables of a multi-view shutter frame)
  if (brute_force) return launch_render_views_shutter2<true, false>(stats, S, A, accum, counters, stream);
  // the vertex pool handles up to POOL_L lights, as in launch_render
  if ((A.flags & 1u) && S.n_lights <= (uint32_t)POOL_L) return launch_render_views_shutter2<false, true>(stats, S, A, accum, counters, stream);
  return launch_render_views_shutter2<false, false>(stats, S, A, accum, counters, stream);
}
