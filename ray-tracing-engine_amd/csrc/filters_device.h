// filters_device.h — the device code the filters share (denoise.hip, temporal.hip, svgf.hip): the guide distances and tap
// weights of the a-trous iterations, the albedo demodulation, and the reprojection of a history along the motion vectors.
// Every expression keeps the order rt_amd.h states; the library is built without contraction, so inlining changes no bit.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include "filters.h"

namespace rtk {

__device__ __forceinline__ float sq3(float4 a, float4 b) {
  const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
  return (x * x + y * y) + z * z;
}

__device__ __forceinline__ float lum(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// the 5-tap B3 spline of the a-trous iterations, i in 0..4
__device__ __forceinline__ float atrous5(int i) {
  const float kh[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
  return kh[i];
}

// Pixel i of a frame and rt_render_aov's sums as the spatial stages read it: the guides (normal + validity flag,
// position), the albedo factor max(albedo / hits, 1e-3) and the demodulated colour rgb / factor.  A pixel without a hit
// passes through (factor 1, colour rgb) and weighs 0 as a tap (flag 0).
struct Demodulated {
  float4 g0, g1, fac;
  float r, g, b;
};
__device__ __forceinline__ Demodulated demodulate(size_t i, const float* __restrict__ rgb, const float* __restrict__ alb,
                                                  const float* __restrict__ nrm, const float* __restrict__ pos, uint32_t hits) {
  const size_t i3 = 3 * i;
  const float r = rgb[i3], g = rgb[i3 + 1], b = rgb[i3 + 2];
  if (hits == 0) return {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(1.f, 1.f, 1.f, 0.f), r, g, b};
  const float fh = (float)hits;
  const float ax = fmaxf(alb[i3] / fh, 1e-3f), ay = fmaxf(alb[i3 + 1] / fh, 1e-3f), az = fmaxf(alb[i3 + 2] / fh, 1e-3f);
  return {make_float4(nrm[i3] / fh, nrm[i3 + 1] / fh, nrm[i3 + 2] / fh, 1.f),
          make_float4(pos[i3] / fh, pos[i3 + 1] / fh, pos[i3 + 2] / fh, 0.f), make_float4(ax, ay, az, 0.f), r / ax, g / ay, b / az};
}

// Steps 1-4 of rt_temporal_accumulate (rt_amd.h) for pixel (px, py) over N channels, float64 throughout: the four
// bilinear taps of the history around the reprojected position, each accepted only on the same mesh and within
// sqrt(*s2p) of the surface point, then out[k] = h + max(1 / Ln, alphaMin[k]) (c[k] - h) with h the weighted mean of
// hist(k, q) over the accepted taps q.  No history: out = c.  Returns the new history length.
// A: TemporalArgs or SvgfArgs (width, height, maxHistory, motion, prevPosition, mesh, hPosition, hLength, hMesh).
template <int N, class Args, class Hist>
__device__ __forceinline__ double reproject_blend(const Args& A, uint32_t px, uint32_t py, const double* __restrict__ s2p,
                                                  const double (&c)[N], const float (&alphaMin)[N], Hist hist, double (&out)[N]) {
  const size_t p = (size_t)py * A.width + px;
  const uint32_t mesh = A.mesh[p];
  const float mx = A.motion[2 * p], my = A.motion[2 * p + 1];
  for (int k = 0; k < N; k++) out[k] = c[k];  // no history: the current frame, length 1
  const double rx = (double)px + (double)mx, ry = (double)py + (double)my;
  // (a non-finite motion component makes rx or ry non-finite: spelled out all the same, the rule's order)
  if (!(mesh != 0xffffffffu && isfinite(mx) && isfinite(my) && !(rx < -1.0) && !(rx >= (double)A.width) && !(ry < -1.0) &&
        !(ry >= (double)A.height)))
    return 1.0;
  const double s2 = *s2p;
  const double fx = floor(rx), fy = floor(ry);
  const double ax = rx - fx, ay = ry - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const double wx[2] = {1.0 - ax, ax}, wy[2] = {1.0 - ay, ay};
  const double X[3] = {(double)A.prevPosition[3 * p], (double)A.prevPosition[3 * p + 1], (double)A.prevPosition[3 * p + 2]};
  double W = 0.0, s[N] = {}, sl = 0.0;
  for (int j = 0; j < 2; j++)
    for (int i = 0; i < 2; i++) {
      const double w = wx[i] * wy[j];
      const int x = x0 + i, y = y0 + j;
      if (!(w > 0.0) || x < 0 || x >= (int)A.width || y < 0 || y >= (int)A.height) continue;
      const size_t q = (size_t)y * A.width + (size_t)x;
      const float hl = A.hLength[q];
      if (!(hl > 0.f) || A.hMesh[q] != mesh) continue;
      const double dx = (double)A.hPosition[3 * q] - X[0], dy = (double)A.hPosition[3 * q + 1] - X[1],
                   dz = (double)A.hPosition[3 * q + 2] - X[2];
      if (!((dx * dx + dy * dy) + dz * dz <= s2)) continue;
      W += w;
      for (int k = 0; k < N; k++) s[k] += w * (double)hist(k, q);
      sl += w * (double)hl;
    }
  if (!(W > 0.0)) return 1.0;
  const double L = sl / W;
  const double Ln = fmin(L + 1.0, (double)A.maxHistory);
  const double inv = 1.0 / Ln;
  for (int k = 0; k < N; k++) {
    const double h = s[k] / W;
    out[k] = h + fmax(inv, (double)alphaMin[k]) * (c[k] - h);
  }
  return Ln;
}

}  // namespace rtk
