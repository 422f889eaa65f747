// svgf.hip — variance-guided spatiotemporal filtering (Schied et al., HPG 2017): rt_svgf.  DESIGN.md "Variance-guided
// spatiotemporal filtering" defines the rule; rt_amd.h states it operation by operation.
//
//   k_svgf_temporal  stage A, one lane per pixel, 64x4 pixels per workgroup as k_tp_blend: the demodulation and the
//                    reprojection of filters_device.h, the latter over five channels (colour, both moments) and the
//                    length in float64; writes the next history's moments and length, the packed guides and factor, and
//                    the working (r, g, b, var) with the variance the temporal moments give.  The two position sigmas
//                    come from the block launch_filter_sigmas fills
//   k_svgf_variance  stage B for pixels with a history shorter than 4 frames: the 7x7 window over a 22x22 apron of
//                    guides and moments staged in LDS; a workgroup in which no lane needs the window leaves after one
//                    block-wide vote, before the staging
//   k_svgf_atrous    stage C, one iteration (step 2^i): the 3x3 Gaussian of the variance, then 5x5 taps of three float4
//                    each — at step 1 from a 20x20 tile staged in LDS (measured on the step-1 dispatches alone: 51 against 123 us at 1024^2), at the
//                    larger steps straight from global memory through L1 / L2
#include <hip/hip_runtime.h>

#include <math.h>

#include "filters_device.h"

namespace rtk {
namespace {

__global__ __launch_bounds__(256) void k_svgf_temporal(SvgfArgs A, float4* __restrict__ g0, float4* __restrict__ g1,
                                                       float4* __restrict__ fac, float4* __restrict__ col,
                                                       const double* __restrict__ s2p) {
  const uint32_t px = blockIdx.x * 64u + (threadIdx.x & 63u), py = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (px >= A.width || py >= A.height) return;
  const size_t p = (size_t)py * A.width + px, p3 = 3 * p;
  const uint32_t nh = A.hits[p];
  const Demodulated d = demodulate(p, A.curRgb, A.albedo, A.normal, A.position, nh);
  g0[p] = d.g0, g1[p] = d.g1, fac[p] = d.fac;
  double c[5] = {(double)d.r, (double)d.g, (double)d.b, 0.0, 0.0};  // colour, then the two luminance moments
  c[3] = (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2];
  c[4] = c[3] * c[3];
  const float alphaMin[5] = {A.alphaMin, A.alphaMin, A.alphaMin, A.alphaMinMoments, A.alphaMinMoments};
  double out[5];
  const double len = reproject_blend<5>(
      A, px, py, s2p, c, alphaMin, [&](int k, size_t q) { return k < 3 ? A.hColor[3 * q + k] : A.hMoments[2 * q + (k - 3)]; }, out);
  const float m1 = (float)out[3], m2 = (float)out[4];
  A.outMoments[2 * p] = m1, A.outMoments[2 * p + 1] = m2;
  A.outLength[p] = (float)len;
  const float cr = (float)out[0], cg = (float)out[1], cb = (float)out[2];
  if (A.outAccum) A.outAccum[p3] = cr, A.outAccum[p3 + 1] = cg, A.outAccum[p3 + 2] = cb;
  // the variance of a long history; k_svgf_variance replaces it where the history is shorter than 4 frames
  col[p] = make_float4(cr, cg, cb, nh ? fmaxf(0.f, m2 - m1 * m1) : 0.f);
}

// 16x16 pixels per workgroup (four waves of 16x4) and their 3-pixel apron
constexpr int kVarTile = 22;

__global__ __launch_bounds__(256) void k_svgf_variance(uint32_t W, uint32_t H, float isn, const float* __restrict__ isxp,
                                                       const float4* __restrict__ g0, const float4* __restrict__ g1,
                                                       const float* __restrict__ moments, const float* __restrict__ length,
                                                       float4* __restrict__ col) {
  __shared__ float4 sN[kVarTile * kVarTile], sX[kVarTile * kVarTile];
  __shared__ float2 sM[kVarTile * kVarTile];
  const int tx = (int)(threadIdx.x & 15u), ty = (int)(threadIdx.x >> 4);
  const int x = (int)(blockIdx.x * 16u) + tx, y = (int)(blockIdx.y * 16u) + ty;
  const bool inside = x < (int)W && y < (int)H;
  const size_t p = inside ? (size_t)y * W + x : 0;
  const float Ln = inside ? length[p] : 4.f;
  const bool need = inside && Ln < 4.f && g0[p].w != 0.f;
  // one vote for the whole workgroup, reached by every lane: after a few frames almost no tile needs the window
  if (!__syncthreads_or(need)) return;
  for (int t = (int)threadIdx.x; t < kVarTile * kVarTile; t += 256) {
    const int qx = (int)(blockIdx.x * 16u) - 3 + t % kVarTile, qy = (int)(blockIdx.y * 16u) - 3 + t / kVarTile;
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f), xq = n;  // (outside the image: not a tap)
    float2 m = make_float2(0.f, 0.f);
    if (qx >= 0 && qx < (int)W && qy >= 0 && qy < (int)H) {
      const size_t q = (size_t)qy * W + qx;
      n = g0[q], xq = g1[q], m = make_float2(moments[2 * q], moments[2 * q + 1]);
    }
    sN[t] = n, sX[t] = xq, sM[t] = m;
  }
  __syncthreads();
  if (!need) return;
  const float isx = *isxp;
  const float4 np = sN[(ty + 3) * kVarTile + tx + 3], xp = sX[(ty + 3) * kVarTile + tx + 3];
  float sw = 0.f, s1 = 0.f, s2 = 0.f;
  for (int j = 0; j < 7; j++)
    for (int i = 0; i < 7; i++) {
      const int t = (ty + j) * kVarTile + tx + i;
      const float4 nq = sN[t];
      if (nq.w == 0.f) continue;
      const float2 m = sM[t];
      const float w = expf(-(sq3(np, nq) * isn + sq3(xp, sX[t]) * isx));
      sw += w, s1 += w * m.x, s2 += w * m.y;
    }
  const float M1 = s1 / sw, M2 = s2 / sw;  // (sw >= 1: the centre tap)
  reinterpret_cast<float*>(col + p)[3] = fmaxf(0.f, M2 - M1 * M1) * (4.f / Ln);
}

// 16x16 pixels per workgroup (four waves of 16x4).  outColor: iteration 0 only; outRgb: the last iteration only, which
// multiplies the factor back (and writes outVar when given) instead of cout.  TILE (step 1 only): the taps and the 3x3
// Gaussian come from a 20x20 tile of the three float4 arrays staged in LDS; otherwise straight from global memory.
constexpr int kTile = 20;

template <bool TILE>
__global__ __launch_bounds__(256) void k_svgf_atrous(uint32_t W, uint32_t H, int step, float isn, float sl,
                                                     const float* __restrict__ isxp, const float4* __restrict__ g0,
                                                     const float4* __restrict__ g1, const float4* __restrict__ fac,
                                                     const float4* __restrict__ cin, float4* __restrict__ cout,
                                                     float* __restrict__ outColor, float* __restrict__ outRgb,
                                                     float* __restrict__ outVar) {
  __shared__ float4 sN[TILE ? kTile * kTile : 1], sX[TILE ? kTile * kTile : 1], sC[TILE ? kTile * kTile : 1];
  const int x0 = (int)(blockIdx.x * 16u) - 2, y0 = (int)(blockIdx.y * 16u) - 2;
  if (TILE) {
    for (int t = (int)threadIdx.x; t < kTile * kTile; t += 256) {
      const int qx = x0 + t % kTile, qy = y0 + t / kTile;
      float4 n = make_float4(0.f, 0.f, 0.f, 0.f), xq = n, c = n;
      if (qx >= 0 && qx < (int)W && qy >= 0 && qy < (int)H) {
        const size_t q = (size_t)qy * W + qx;
        n = g0[q], xq = g1[q], c = cin[q];
      }
      sN[t] = n, sX[t] = xq, sC[t] = c;
    }
    __syncthreads();
  }
  const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
  if (x >= (int)W || y >= (int)H) return;
  auto N = [&](int xx, int yy) { return TILE ? sN[(yy - y0) * kTile + (xx - x0)] : g0[(size_t)yy * W + xx]; };
  auto X = [&](int xx, int yy) { return TILE ? sX[(yy - y0) * kTile + (xx - x0)] : g1[(size_t)yy * W + xx]; };
  auto C = [&](int xx, int yy) { return TILE ? sC[(yy - y0) * kTile + (xx - x0)] : cin[(size_t)yy * W + xx]; };
  const size_t p = (size_t)y * W + x;
  const float4 np = N(x, y), cp = C(x, y);
  float4 res = cp;
  if (np.w != 0.f) {
    const float4 xp = X(x, y);
    const float isx = *isxp;
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    float gs = 0.f, gk = 0.f;  // the 3x3 Gaussian of the variance over the valid neighbours
    for (int j = 0; j < 3; j++) {
      const int yy = y + j - 1;
      if (yy < 0 || yy >= (int)H) continue;
      for (int i = 0; i < 3; i++) {
        const int xx = x + i - 1;
        if (xx < 0 || xx >= (int)W) continue;
        if (N(xx, yy).w == 0.f) continue;
        const float k = k3[i] * k3[j];
        gs += k * C(xx, yy).w, gk += k;
      }
    }
    const float den = sl * sqrtf(gs / gk) + 1e-4f;
    const float lp = lum(cp);
    float sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f, sw = 0.f;
    for (int j = 0; j < 5; j++) {
      const int yy = y + (j - 2) * step;
      if (yy < 0 || yy >= (int)H) continue;
      for (int i = 0; i < 5; i++) {
        const int xx = x + (i - 2) * step;
        if (xx < 0 || xx >= (int)W) continue;
        const float4 nq = N(xx, yy);
        if (nq.w == 0.f) continue;
        const float4 cq = C(xx, yy), xq = X(xx, yy);
        const float w = atrous5(i) * atrous5(j) * expf(-((sq3(np, nq) * isn + sq3(xp, xq) * isx) + fabsf(lp - lum(cq)) / den));
        sr += w * cq.x, sg += w * cq.y, sb += w * cq.z, sv += (w * w) * cq.w, sw += w;
      }
    }
    res = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));  // (sw >= (3/8)^2: the centre tap)
  }
  if (outColor) outColor[3 * p] = res.x, outColor[3 * p + 1] = res.y, outColor[3 * p + 2] = res.z;
  if (!outRgb) {
    cout[p] = res;
    return;
  }
  const float4 f = fac[p];  // (1, 1, 1 for pixels without a hit)
  outRgb[3 * p] = res.x * f.x, outRgb[3 * p + 1] = res.y * f.y, outRgb[3 * p + 2] = res.z * f.z;
  if (outVar) outVar[p] = res.w;
}

}  // namespace

hipError_t launch_svgf(const DevScene& S, const SvgfArgs& A, hipStream_t stream) {
  const size_t n = (size_t)A.width * A.height;
  if (n == 0) return hipSuccess;
  FilterScratch s = carve_filter_scratch(A.scratch, n);
  const float* isx = &s.block->isx;
  const hipError_t e = launch_filter_sigmas(S, s.block, A.sigmaPosition, A.sigmaReproject, A.sigmaScale, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_svgf_temporal, dim3((A.width + 63u) / 64u, (A.height + 3u) / 4u), dim3(256), 0, stream, A, s.g0, s.g1, s.fac,
                     s.ca, &s.block->s2);
  const dim3 grid((A.width + 15u) / 16u, (A.height + 15u) / 16u);
  const float isn = 1.f / (A.sigmaNormal * A.sigmaNormal);
  hipLaunchKernelGGL(k_svgf_variance, grid, dim3(256), 0, stream, A.width, A.height, isn, isx, s.g0, s.g1, A.outMoments, A.outLength, s.ca);
  for (uint32_t it = 0; it < A.iterations; it++) {
    const bool last = it + 1 == A.iterations;
    hipLaunchKernelGGL(it == 0 ? k_svgf_atrous<true> : k_svgf_atrous<false>, grid, dim3(256), 0, stream, A.width, A.height,
                       1 << it, isn, A.sigmaLuminance, isx, s.g0, s.g1, s.fac, s.ca, s.cb, it == 0 ? A.outColor : nullptr,
                       last ? A.outRgb : nullptr, last ? A.outVariance : nullptr);
    float4* t = s.ca;
    s.ca = s.cb, s.cb = t;
  }
  return hipGetLastError();
}

}  // namespace rtk
