// svgf.h — argument block and launcher of the variance-guided spatiotemporal filter (svgf.hip, rt_svgf).
#pragma once

#include "rt_kernels.h"

namespace rtk {

// every buffer is device memory; scratch = 5 * w * h + 4 float4 (svgf_scratch): the guides (normal + validity flag,
// position), the albedo factor, two working (r, g, b, var) buffers, then the extent words and the two sigmas
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
inline size_t svgf_scratch(uint32_t w, uint32_t h) { return 5 * (size_t)w * h + 4; }
hipError_t launch_svgf(const DevScene& S, const SvgfArgs& A, hipStream_t stream);

}  // namespace rtk
