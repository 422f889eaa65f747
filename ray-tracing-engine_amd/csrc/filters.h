// filters.h — what the three image-space filters share with the C ABI and with one another: the argument blocks and
// launchers of rt_denoise (denoise.hip), rt_temporal_accumulate (temporal.hip) and rt_svgf (svgf.hip), the layout of their
// scratch, and the sigmas every one of them derives from the scene's extent.  filters_device.h holds the device code.
#pragma once

#include <cstddef>

#include "rt_kernels.h"

namespace rtk {

// What the filters leave in device memory for their kernels to read: the box of the vertices the triangles reference
// as order-preserving words (min x, y, z, then max), and the two sigmas derived from it or given by the caller.
struct FilterBlock {
  uint32_t ext[6];
  float isx;  // 1 / sigma_position^2, the spatial guide (rt_denoise, rt_svgf)
  double s2;  // sigma^2 of the tap acceptance (rt_temporal_accumulate's sigma_position, rt_svgf's sigma_reproject)
};
static_assert(offsetof(FilterBlock, s2) % 8 == 0, "s2 is read and written as one 8-byte word");

// The scratch of rt_denoise and rt_svgf for w x h pixels, in float4: the guides (normal + validity flag, position), the
// albedo factor, two working (r, g, b[, var]) planes, then the block.
inline size_t filter_scratch(uint32_t w, uint32_t h) {
  return 5 * (size_t)w * h + (sizeof(FilterBlock) + sizeof(float4) - 1) / sizeof(float4);
}
struct FilterScratch {
  float4 *g0, *g1, *fac, *ca, *cb;
  FilterBlock* block;
};
inline FilterScratch carve_filter_scratch(float4* s, size_t n) {
  return {s, s + n, s + 2 * n, s + 3 * n, s + 4 * n, reinterpret_cast<FilterBlock*>(s + 5 * n)};
}

// order-preserving float <-> uint32 (atomicMin / atomicMax on the bits)
__device__ __forceinline__ uint32_t f2o(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float o2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
// the box of the vertices the triangles reference into ext[0..5] (denoise.hip k_ref_extent)
hipError_t launch_ref_extent(const DevScene& S, uint32_t* ext, hipStream_t stream);
// block->isx from sigmaPos and block->s2 from sigmaRep (denoise.hip k_filter_sigmas).  A sigma of 0: scale times the
// diagonal of that box, which is reduced first; a filter that reads only one of the two passes its sigma twice.
hipError_t launch_filter_sigmas(const DevScene& S, FilterBlock* block, float sigmaPos, float sigmaRep, float scale, hipStream_t stream);

// the edge-avoiding a-trous filter (denoise.hip, rt_denoise): inputs and output [h][w][3] / [h][w], device memory;
// scratch = filter_scratch(width, height) float4
struct DenoiseArgs {
  uint32_t width, height, iterations;
  float sigma_color, sigma_normal, sigma_position;  // sigma_position 0: 2 % of the referenced vertices' box diagonal
  const float *rgb, *albedo, *normal, *position;
  const uint32_t* hits;
  float* out;
  float4* scratch;
};
hipError_t launch_denoise(const DevScene& S, const DenoiseArgs& D, hipStream_t stream);
// the same filter over nFrames frames of width x height stacked in every buffer (rt_denoise_batch): one pack launch and
// one launch per iteration over all frames, no tap across a frame boundary, the sigma reduction once; scratch =
// nFrames * filter_scratch(width, height) float4, nFrames * width * height < 2^31
hipError_t launch_denoise_batch(const DevScene& S, const DenoiseArgs& D, uint32_t nFrames, hipStream_t stream);

// temporal accumulation (temporal.hip, rt_temporal_accumulate): the history reprojected along the motion vectors and
// blended with the current frame; all buffers device memory.  filters_device.h reproject_blend reads the fields from
// width to hMesh by name, here and in SvgfArgs.
struct TemporalArgs {
  uint32_t width, height, maxHistory;
  float alphaMin, sigmaPosition;  // sigmaPosition 0: sigmaScale times the diagonal of the referenced vertices' box
  float sigmaScale;
  const float *curRgb, *motion, *prevPosition;  // the current frame: [h][w][3], rt_motion.motion, rt_motion.prev_position
  const uint32_t* mesh;                         // rt_motion.mesh
  const float *hRgb, *hPosition, *hLength;      // the history
  const uint32_t* hMesh;
  float *outRgb, *outLength;
  FilterBlock* block;  // one block of its own: the accumulation may run beside a filter on another stream
};
hipError_t launch_temporal(const DevScene& S, const TemporalArgs& T, hipStream_t stream);

// variance-guided spatiotemporal filtering (svgf.hip, rt_svgf): every buffer is device memory; scratch =
// filter_scratch(width, height) float4
struct SvgfArgs {
  uint32_t width, height, iterations, maxHistory;
  float alphaMin, alphaMinMoments, sigmaLuminance, sigmaNormal;
  float sigmaPosition, sigmaReproject, sigmaScale;   // a sigma of 0: sigmaScale of the referenced vertices' box diagonal
  const float *curRgb, *albedo, *normal, *position;  // the frame and rt_render_aov's sums
  const uint32_t* hits;
  const float *motion, *prevPosition;                // rt_render_motion's channels
  const uint32_t* mesh;
  const float *hColor, *hMoments, *hPosition, *hLength;  // the history
  const uint32_t* hMesh;
  float *outRgb, *outColor, *outMoments, *outLength, *outAccum, *outVariance;  // the last two may be null
  float4* scratch;
};
hipError_t launch_svgf(const DevScene& S, const SvgfArgs& A, hipStream_t stream);

}  // namespace rtk
