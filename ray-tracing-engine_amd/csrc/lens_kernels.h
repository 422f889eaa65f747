// lens_kernels.h — the frame through a thin lens: rt_render_lens.
//
// The frame integrator itself, render_tile, with lens_ray in place of camera_ray (LT_LENS): the lane layout, the sample
// hand-over and the vertex pool are the frame's, so reserved[0] and reserved[1] mean what they mean there.  The host-
// derived constants travel as a kernel argument of their own: RenderArgs and the frame's entry points stay as they are.
// Only the one-wave-per-workgroup family that k_render serves is instantiated — brute, sequential and pooled, each
// counted (STATS, one wave per SIMD) and timed (four waves per SIMD, k_render's target) — and none with LT_FASTDET: they
// divide.  There are no persistent instances.  aperture == 0 runs the same instances: the lens branch is a wave-uniform
// test on the record, and the frame is rt_render's bit for bit.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

template <bool BRUTE, bool POOLED, bool STATS, int MINW>
__global__ __launch_bounds__(BLOCK, MINW) void k_render_lens(DevScene S, RenderArgs A, LensRec R, float4* __restrict__ accum,
                                                             unsigned long long* __restrict__ counters) {
  static_assert(!POOLED || !BRUTE, "the vertex pool serves BVH direct lighting");
  // dynamic LDS as k_render's: [levels][64] traversal stack, then (POOLED) the ray pool
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<false>(lds, A.stackLevels, 0);
  uint32_t* pool = lds + A.stackLevels * BLOCK;
  float* ex = reinterpret_cast<float*>(POOLED ? pool : lds);
  LaneStats st;
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t) render_tile<BRUTE, false, POOLED, STATS, LT_LENS>(S, A, accum, L, pool, ex, t, st, &R);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_render_lens folds the stripes)
}

template <bool BRUTE, bool POOLED>
static hipError_t launch_render_lens2(bool stats, const DevScene& S, const RenderArgs& A, const LensRec& R, float4* accum,
                                      unsigned long long* counters, hipStream_t stream) {
  if (A.n_tiles == 0) return hipSuccess;
  // (launch_render2's sizes: at least four rows for the sample hand-over of the instances without a pool)
  const size_t ldsBytes = 4u * ((A.stackLevels < 4u ? 4u : A.stackLevels) * BLOCK + (POOLED ? VP_WORDS : 0));
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;
  if (stats) {
    hipLaunchKernelGGL((k_render_lens<BRUTE, POOLED, true, 1>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, R, accum, counters);
  } else {
    hipLaunchKernelGGL((k_render_lens<BRUTE, POOLED, false, 4>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, R, accum, counters);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
  return hipGetLastError();
}

hipError_t launch_render_lens(bool brute_force, bool stats, const DevScene& S, const RenderArgs& A, const LensRec& R,
                              float4* accum, unsigned long long* counters, hipStream_t stream) {
  if (A.tileView) return hipErrorInvalidValue;  // (no multi-view lens frames)
  if (brute_force) return launch_render_lens2<true, false>(stats, S, A, R, accum, counters, stream);
  // the vertex pool handles up to POOL_L lights, as in launch_render
  if ((A.flags & 1u) && S.n_lights <= (uint32_t)POOL_L) return launch_render_lens2<false, true>(stats, S, A, R, accum, counters, stream);
  return launch_render_lens2<false, false>(stats, S, A, R, accum, counters, stream);
}
