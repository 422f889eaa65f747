// denoise.hip — the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) guided by the first-hit AOVs of
// rt_render_aov, with albedo demodulation: rt_denoise.  DESIGN.md "AOVs and the a-trous denoiser" defines it; every
// kernel here is one lane per pixel.  The first two serve all three filters (filters.h).
//
//   k_ref_extent     bounding box of the vertices the triangles reference (only when a caller leaves a sigma 0)
//   k_filter_sigmas  1 / sigma_position^2 (float) and the tap acceptance's sigma^2 (double) into the filter's block: the
//                    caller's sigmas, or a fraction of that box's diagonal (the denoiser: 2 %)
//   k_dn_pack        per pixel the guides, the albedo factor and the demodulated colour (filters_device.h demodulate)
//   k_dn_iter        one iteration (step 2^i): 5x5 taps straight from global memory through L1 / L2; the last one
//                    multiplies the factor back and writes the [h][w][3] output
//   k_dn_iter_batch  the same iteration over a stack of frames (rt_denoise_batch): one launch, the frame a grid dimension
#include <hip/hip_runtime.h>

#include <math.h>

#include "filters_device.h"

namespace rtk {
namespace {

// ext[0..2] = min x, y, z (initialised to 0xffffffff), ext[3..5] = max (initialised to 0)
__global__ __launch_bounds__(256) void k_ref_extent(const float* __restrict__ vpos, const uint4* __restrict__ triShade,
                                                   uint32_t nTris, uint32_t* __restrict__ ext) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nTris; t += gridDim.x * blockDim.x) {
    const uint4 tv = triShade[t];
    const uint32_t v[3] = {tv.x, tv.y, tv.z};
    for (int k = 0; k < 3; k++)
      for (int a = 0; a < 3; a++) {
        const float c = vpos[3 * (size_t)v[k] + a];
        lo[a] = fminf(lo[a], c), hi[a] = fmaxf(hi[a], c);
      }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int a = 0; a < 3; a++) lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64)), hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
  if ((threadIdx.x & 63u) == 0)
    for (int a = 0; a < 3; a++) atomicMin(&ext[a], f2o(lo[a])), atomicMax(&ext[3 + a], f2o(hi[a]));
}

__global__ void k_filter_sigmas(FilterBlock* __restrict__ blk, float sigmaPos, float sigmaRep, float scale) {
  if (sigmaPos <= 0.f || sigmaRep <= 0.f) {
    const uint32_t* ext = blk->ext;
    const float dx = o2f(ext[3]) - o2f(ext[0]), dy = o2f(ext[4]) - o2f(ext[1]), dz = o2f(ext[5]) - o2f(ext[2]);
    float sigma = scale * sqrtf((dx * dx + dy * dy) + dz * dz);
    if (!(sigma > 0.f) || !(sigma < INFINITY)) sigma = 1.f;  // (a flat or empty scene: any scale does)
    if (sigmaPos <= 0.f) sigmaPos = sigma;
    if (sigmaRep <= 0.f) sigmaRep = sigma;
  }
  blk->isx = 1.f / (sigmaPos * sigmaPos);
  blk->s2 = (double)sigmaRep * (double)sigmaRep;
}

__global__ __launch_bounds__(256) void k_dn_pack(uint32_t n, const float* __restrict__ rgb, const float* __restrict__ alb,
                                                 const float* __restrict__ nrm, const float* __restrict__ pos,
                                                 const uint32_t* __restrict__ hits, float4* __restrict__ g0,
                                                 float4* __restrict__ g1, float4* __restrict__ fac, float4* __restrict__ col) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Demodulated d = demodulate(i, rgb, alb, nrm, pos, hits[i]);
  g0[i] = d.g0, g1[i] = d.g1, fac[i] = d.fac, col[i] = make_float4(d.r, d.g, d.b, 0.f);
}

// Pixel (x, y) of one iteration over ONE frame of W x H pixels: every plane pointer is the frame's own (its first
// pixel), so no tap leaves the frame.  k_dn_iter hands in the image, k_dn_iter_batch a frame's slice of a stack.
__device__ __forceinline__ void dn_iter_pixel(int x, int y, uint32_t W, uint32_t H, int step, float isc, float isn,
                                              const float* __restrict__ isxp, const float4* __restrict__ g0,
                                              const float4* __restrict__ g1, const float4* __restrict__ fac,
                                              const float4* __restrict__ cin, float4* __restrict__ cout, float* __restrict__ out) {
  const size_t p = (size_t)y * W + x;
  const float4 np = g0[p], cp = cin[p];
  float4 res = cp;
  if (np.w != 0.f) {
    const float4 xp = g1[p];
    const float isx = *isxp;
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
    for (int j = 0; j < 5; j++) {
      const int yy = y + (j - 2) * step;
      if (yy < 0 || yy >= (int)H) continue;
      for (int i = 0; i < 5; i++) {
        const int xx = x + (i - 2) * step;
        if (xx < 0 || xx >= (int)W) continue;
        const size_t q = (size_t)yy * W + xx;
        const float4 nq = g0[q];
        if (nq.w == 0.f) continue;
        const float4 cq = cin[q], xq = g1[q];
        const float w = atrous5(i) * atrous5(j) * expf(-(sq3(cp, cq) * isc + sq3(np, nq) * isn + sq3(xp, xq) * isx));
        sr += w * cq.x, sg += w * cq.y, sb += w * cq.z, sw += w;
      }
    }
    res = make_float4(sr / sw, sg / sw, sb / sw, 0.f);  // (sw >= (3/8)^2: the centre tap)
  }
  if (!out) {
    cout[p] = res;
    return;
  }
  const float4 f = fac[p];  // (1, 1, 1 for pixels without a hit: res is their rgb)
  out[3 * p] = np.w != 0.f ? res.x * f.x : res.x;
  out[3 * p + 1] = np.w != 0.f ? res.y * f.y : res.y;
  out[3 * p + 2] = np.w != 0.f ? res.z * f.z : res.z;
}

// 16x16 pixels per workgroup (four waves of 16x4)
__global__ __launch_bounds__(256) void k_dn_iter(uint32_t W, uint32_t H, int step, float isc, float isn,
                                                 const float* __restrict__ isxp, const float4* __restrict__ g0,
                                                 const float4* __restrict__ g1, const float4* __restrict__ fac,
                                                 const float4* __restrict__ cin, float4* __restrict__ cout,
                                                 float* __restrict__ out) {
  const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
  if (x >= (int)W || y >= (int)H) return;
  dn_iter_pixel(x, y, W, H, step, isc, isn, isxp, g0, g1, fac, cin, cout, out);
}

// The same over a stack of nFrames frames (rt_denoise_batch): the frame is the grid's z dimension (a stride loop past
// 65,535 frames) and a slice base added to every plane, in 64 bits; x, y and the taps stay inside the frame.
__global__ __launch_bounds__(256) void k_dn_iter_batch(uint32_t W, uint32_t H, uint32_t nFrames, int step, float isc, float isn,
                                                       const float* __restrict__ isxp, const float4* __restrict__ g0,
                                                       const float4* __restrict__ g1, const float4* __restrict__ fac,
                                                       const float4* __restrict__ cin, float4* __restrict__ cout,
                                                       float* __restrict__ out) {
  const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
  if (x >= (int)W || y >= (int)H) return;
  for (uint32_t f = blockIdx.z; f < nFrames; f += gridDim.z) {
    const size_t b = view_slice(f, W, H, 1);
    dn_iter_pixel(x, y, W, H, step, isc, isn, isxp, g0 + b, g1 + b, fac + b, cin + b, cout + b, out ? out + 3 * b : nullptr);
  }
}

}  // namespace

hipError_t launch_ref_extent(const DevScene& S, uint32_t* ext, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(ext, 0xff, 3 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(ext + 3, 0, 3 * sizeof(uint32_t), stream)) != hipSuccess) return e;
  const uint32_t blocks = S.n_tris ? (S.n_tris + 255u) / 256u < 1024u ? (S.n_tris + 255u) / 256u : 1024u : 1u;
  hipLaunchKernelGGL(k_ref_extent, dim3(blocks), dim3(256), 0, stream, S.vpos, S.triShade, S.n_tris, ext);
  return hipGetLastError();
}

hipError_t launch_filter_sigmas(const DevScene& S, FilterBlock* block, float sigmaPos, float sigmaRep, float scale, hipStream_t stream) {
  if (sigmaPos <= 0.f || sigmaRep <= 0.f) {
    const hipError_t e = launch_ref_extent(S, block->ext, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_filter_sigmas, dim3(1), dim3(1), 0, stream, block, sigmaPos, sigmaRep, scale);
  return hipGetLastError();
}

// nFrames frames of D.width x D.height stacked in every buffer; batch: the frame-indexed iteration kernel
static hipError_t denoise_frames(const DevScene& S, const DenoiseArgs& D, uint32_t nFrames, bool batch, hipStream_t stream) {
  const size_t n = (size_t)D.width * D.height * nFrames;
  if (n == 0) return hipSuccess;
  FilterScratch s = carve_filter_scratch(D.scratch, n);
  const hipError_t e = launch_filter_sigmas(S, s.block, D.sigma_position, D.sigma_position, 0.02f, stream);
  if (e != hipSuccess) return e;
  // (the guides, the factor and the demodulated colour are per pixel: a stack packs as one image does)
  hipLaunchKernelGGL(k_dn_pack, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, (uint32_t)n, D.rgb, D.albedo, D.normal,
                     D.position, D.hits, s.g0, s.g1, s.fac, s.ca);
  const dim3 grid((D.width + 15u) / 16u, (D.height + 15u) / 16u, batch ? (nFrames < 65535u ? nFrames : 65535u) : 1u);
  const float isn = 1.f / (D.sigma_normal * D.sigma_normal);
  for (uint32_t it = 0; it < D.iterations; it++) {
    const float sc = D.sigma_color * ldexpf(1.f, -(int)it);  // the colour sigma halves every iteration
    const bool last = it + 1 == D.iterations;
    if (batch)
      hipLaunchKernelGGL(k_dn_iter_batch, grid, dim3(256), 0, stream, D.width, D.height, nFrames, 1 << it, 1.f / (sc * sc), isn,
                         &s.block->isx, s.g0, s.g1, s.fac, s.ca, s.cb, last ? D.out : nullptr);
    else
      hipLaunchKernelGGL(k_dn_iter, grid, dim3(256), 0, stream, D.width, D.height, 1 << it, 1.f / (sc * sc), isn, &s.block->isx, s.g0,
                         s.g1, s.fac, s.ca, s.cb, last ? D.out : nullptr);
    float4* t = s.ca;
    s.ca = s.cb, s.cb = t;
  }
  return hipGetLastError();
}

hipError_t launch_denoise(const DevScene& S, const DenoiseArgs& D, hipStream_t stream) { return denoise_frames(S, D, 1, false, stream); }

hipError_t launch_denoise_batch(const DevScene& S, const DenoiseArgs& D, uint32_t nFrames, hipStream_t stream) {
  return denoise_frames(S, D, nFrames, true, stream);
}

}  // namespace rtk
