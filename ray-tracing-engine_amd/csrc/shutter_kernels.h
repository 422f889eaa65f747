// shutter_kernels.h — the frame under an open shutter while the camera moves: rt_render_shutter.
//
// The frame integrator itself, render_tile, with shutter_ray in place of camera_ray (LT_SHUTTER): every sample draws a
// time, forms its camera in registers and casts that camera's primary ray — through rt_render_lens' lens where the record
// has an aperture.  The lane layout, the sample hand-over and the vertex pool are the frame's, so reserved[0] and
// reserved[1] mean what they mean there.  The record travels as a kernel argument of its own: RenderArgs, LensRec and the
// entry points of the frame and of the lens stay as they are.  The instances mirror k_render_lens': brute, sequential
// and pooled, each counted (STATS, one wave per SIMD) and timed (four waves per SIMD); none with LT_FASTDET — the
// operand bounds of the short forms were proved for the context's camera only — and none persistent.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

template <bool BRUTE, bool POOLED, bool STATS, int MINW>
__global__ __launch_bounds__(BLOCK, MINW) void k_render_shutter(DevScene S, RenderArgs A, ShutterRec R, float4* __restrict__ accum,
                                                                unsigned long long* __restrict__ counters) {
  static_assert(!POOLED || !BRUTE, "the vertex pool serves BVH direct lighting");
  // dynamic LDS as k_render's: [levels][64] traversal stack, then (POOLED) the ray pool
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<false>(lds, A.stackLevels, 0);
  uint32_t* pool = lds + A.stackLevels * BLOCK;
  float* ex = reinterpret_cast<float*>(POOLED ? pool : lds);
  LaneStats st;
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t) render_tile<BRUTE, false, POOLED, STATS, LT_SHUTTER>(S, A, accum, L, pool, ex, t, st, nullptr, &R);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_render_shutter folds the stripes)
}

template <bool BRUTE, bool POOLED>
static hipError_t launch_render_shutter2(bool stats, const DevScene& S, const RenderArgs& A, const ShutterRec& R, float4* accum,
                                         unsigned long long* counters, hipStream_t stream) {
  if (A.n_tiles == 0) return hipSuccess;
  // (launch_render2's sizes: at least four rows for the sample hand-over of the instances without a pool)
  const size_t ldsBytes = 4u * ((A.stackLevels < 4u ? 4u : A.stackLevels) * BLOCK + (POOLED ? VP_WORDS : 0));
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;
  if (stats) {
    hipLaunchKernelGGL((k_render_shutter<BRUTE, POOLED, true, 1>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, R, accum, counters);
  } else {
    hipLaunchKernelGGL((k_render_shutter<BRUTE, POOLED, false, 4>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, R, accum, counters);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
  return hipGetLastError();
}

hipError_t launch_render_shutter(bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, const ShutterRec& R,
                                 float4* accum, unsigned long long* counters, hipStream_t stream) {
  if (A.tileView) return hipErrorInvalidValue;  // (multi-view shutter frames: launch_render_views_shutter)
  if (brute_force) return launch_render_shutter2<true, false>(stats, S, A, R, accum, counters, stream);
  // the vertex pool handles up to POOL_L lights, as in launch_render
  if ((A.flags & 1u) && S.n_lights <= (uint32_t)POOL_L) return launch_render_shutter2<false, true>(stats, S, A, R, accum, counters, stream);
  return launch_render_shutter2<false, false>(stats, S, A, R, accum, counters, stream);
}
