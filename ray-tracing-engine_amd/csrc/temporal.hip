// temporal.hip — temporal accumulation of animated frames: rt_temporal_accumulate.  DESIGN.md "Motion vectors and
// temporal accumulation" defines the rule; rt_amd.h states it operation by operation.
//
//   k_tp_sigma   sigma_position^2 as a double into device memory: the caller's sigma, or (default) a fraction of the
//                diagonal of the box of the vertices the triangles reference (launch_ref_extent, the denoiser's reduction)
//   k_tp_blend   one lane per pixel: the current frame's colour, motion vector, previous-frame surface point and mesh
//                (coalesced), the four bilinear taps of the history around the reprojected position (gathered), each
//                accepted only on the same mesh and within sigma_position of the surface point; float64 throughout
#include <hip/hip_runtime.h>

#include <math.h>

#include "rt_kernels.h"

namespace rtk {
namespace {

__global__ void k_tp_sigma(const uint32_t* __restrict__ ext, float sigma, float scale, double* __restrict__ s2) {
  if (sigma <= 0.f) {
    const float dx = o2f(ext[3]) - o2f(ext[0]), dy = o2f(ext[4]) - o2f(ext[1]), dz = o2f(ext[5]) - o2f(ext[2]);
    sigma = scale * sqrtf((dx * dx + dy * dy) + dz * dz);
    if (!(sigma > 0.f) || !(sigma < INFINITY)) sigma = 1.f;  // (a flat or empty scene: any scale does)
  }
  *s2 = (double)sigma * (double)sigma;
}

__global__ __launch_bounds__(256) void k_tp_blend(TemporalArgs T, const double* __restrict__ s2p) {
  const uint32_t px = blockIdx.x * 64u + (threadIdx.x & 63u), py = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (px >= T.width || py >= T.height) return;
  const size_t p = (size_t)py * T.width + px;
  const double c[3] = {(double)T.curRgb[3 * p], (double)T.curRgb[3 * p + 1], (double)T.curRgb[3 * p + 2]};
  const uint32_t mesh = T.mesh[p];
  const float mx = T.motion[2 * p], my = T.motion[2 * p + 1];
  double out[3] = {c[0], c[1], c[2]}, len = 1.0;  // no history: the current frame, length 1
  const double rx = (double)px + (double)mx, ry = (double)py + (double)my;
  // (a non-finite motion component makes rx or ry non-finite: spelled out all the same, the rule's order)
  if (mesh != 0xffffffffu && isfinite(mx) && isfinite(my) && !(rx < -1.0) && !(rx >= (double)T.width) && !(ry < -1.0) &&
      !(ry >= (double)T.height)) {
    const double s2 = *s2p;
    const double fx = floor(rx), fy = floor(ry);
    const double ax = rx - fx, ay = ry - fy;
    const int x0 = (int)fx, y0 = (int)fy;
    const double wx[2] = {1.0 - ax, ax}, wy[2] = {1.0 - ay, ay};
    const double X[3] = {(double)T.prevPosition[3 * p], (double)T.prevPosition[3 * p + 1], (double)T.prevPosition[3 * p + 2]};
    double W = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sl = 0.0;
    for (int j = 0; j < 2; j++)
      for (int i = 0; i < 2; i++) {
        const double w = wx[i] * wy[j];
        const int x = x0 + i, y = y0 + j;
        if (!(w > 0.0) || x < 0 || x >= (int)T.width || y < 0 || y >= (int)T.height) continue;
        const size_t q = (size_t)y * T.width + (size_t)x;
        const float hl = T.hLength[q];
        if (!(hl > 0.f) || T.hMesh[q] != mesh) continue;
        const double dx = (double)T.hPosition[3 * q] - X[0], dy = (double)T.hPosition[3 * q + 1] - X[1],
                     dz = (double)T.hPosition[3 * q + 2] - X[2];
        if (!((dx * dx + dy * dy) + dz * dz <= s2)) continue;
        W += w;
        sr += w * (double)T.hRgb[3 * q], sg += w * (double)T.hRgb[3 * q + 1], sb += w * (double)T.hRgb[3 * q + 2];
        sl += w * (double)hl;
      }
    if (W > 0.0) {
      const double h[3] = {sr / W, sg / W, sb / W};
      const double L = sl / W;
      const double Ln = fmin(L + 1.0, (double)T.maxHistory);
      const double alpha = fmax(1.0 / Ln, (double)T.alphaMin);
      for (int k = 0; k < 3; k++) out[k] = h[k] + alpha * (c[k] - h[k]);
      len = Ln;
    }
  }
  T.outRgb[3 * p] = (float)out[0], T.outRgb[3 * p + 1] = (float)out[1], T.outRgb[3 * p + 2] = (float)out[2];
  T.outLength[p] = (float)len;
}

}  // namespace

hipError_t launch_temporal(const DevScene& S, const TemporalArgs& T, hipStream_t stream) {
  if (T.width == 0 || T.height == 0) return hipSuccess;
  double* s2 = reinterpret_cast<double*>(T.scratch + 8);
  if (T.sigmaPosition <= 0.f) {
    const hipError_t e = launch_ref_extent(S, T.scratch, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_tp_sigma, dim3(1), dim3(1), 0, stream, T.scratch, T.sigmaPosition, T.sigmaScale, s2);
  hipLaunchKernelGGL(k_tp_blend, dim3((T.width + 63u) / 64u, (T.height + 3u) / 4u), dim3(256), 0, stream, T, s2);
  return hipGetLastError();
}

}  // namespace rtk
