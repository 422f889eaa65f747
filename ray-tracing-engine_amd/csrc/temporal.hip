// temporal.hip — temporal accumulation of animated frames: rt_temporal_accumulate.  DESIGN.md "Motion vectors and
// temporal accumulation" defines the rule; rt_amd.h states it operation by operation.
//
//   k_tp_blend   one lane per pixel: the current frame's colour, motion vector, previous-frame surface point and mesh
//                (coalesced), the four bilinear taps of the history around the reprojected position (gathered), each
//                accepted only on the same mesh and within sigma_position of the surface point; float64 throughout
//                (filters_device.h reproject_blend over three channels).  sigma_position^2 comes from the block that
//                launch_filter_sigmas fills: the caller's sigma, or (default) a fraction of the diagonal of the box of
//                the vertices the triangles reference
#include <hip/hip_runtime.h>

#include <math.h>

#include "filters_device.h"

namespace rtk {
namespace {

__global__ __launch_bounds__(256) void k_tp_blend(TemporalArgs T) {
  const uint32_t px = blockIdx.x * 64u + (threadIdx.x & 63u), py = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (px >= T.width || py >= T.height) return;
  const size_t p = (size_t)py * T.width + px;
  const double c[3] = {(double)T.curRgb[3 * p], (double)T.curRgb[3 * p + 1], (double)T.curRgb[3 * p + 2]};
  const float alphaMin[3] = {T.alphaMin, T.alphaMin, T.alphaMin};
  double out[3];
  const double len = reproject_blend<3>(T, px, py, &T.block->s2, c, alphaMin, [&](int k, size_t q) { return T.hRgb[3 * q + k]; }, out);
  T.outRgb[3 * p] = (float)out[0], T.outRgb[3 * p + 1] = (float)out[1], T.outRgb[3 * p + 2] = (float)out[2];
  T.outLength[p] = (float)len;
}

}  // namespace

hipError_t launch_temporal(const DevScene& S, const TemporalArgs& T, hipStream_t stream) {
  if (T.width == 0 || T.height == 0) return hipSuccess;
  const hipError_t e = launch_filter_sigmas(S, T.block, T.sigmaPosition, T.sigmaPosition, T.sigmaScale, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tp_blend, dim3((T.width + 63u) / 64u, (T.height + 3u) / 4u), dim3(256), 0, stream, T);
  return hipGetLastError();
}

}  // namespace rtk
