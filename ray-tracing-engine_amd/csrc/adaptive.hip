// adaptive.hip — adaptive sampling: rt_render_adaptive.  DESIGN.md "Adaptive sampling" defines it.  The passes themselves
// are the render kernels over a shorter wave-tile list; what is here runs between them.
//
//   k_adapt_compact   one workgroup: the active granules (retired == 0), row-major, into list; their in-image pixels
//                     and their wave tiles at every sshift into counts (the host reads them back and picks the sshift)
//   k_adapt_expand    one workgroup: the wave tiles of the listed granules for one footprint, row-major inside each
//                     granule and skipping tiles wholly outside the image (the order rt_api.cpp ensure_tiles uses)
//   k_adapt_update    one wave per granule the last pass rendered, lane = pixel: the moments, the rule, and the
//                     granule's verdict by ballot over its in-image lanes
//   k_resolve_adaptive k_resolve (rt_kernels.hip) with the per-pixel spp = passes * P: same expression, same order
#include <hip/hip_runtime.h>

#include "rt_kernels.h"

namespace rtk {
namespace {

// wave footprints by sshift (rt_api.cpp wave_tile_shape)
__device__ constexpr uint32_t kTileW[7] = {8, 8, 4, 4, 2, 2, 1}, kTileH[7] = {8, 4, 4, 2, 2, 1, 1};

// Exclusive prefix sum of v over the workgroup (a multiple of 64 threads, at most 1024) and its total.  Every thread
// calls it; wsum is reused by the next call.
__device__ uint32_t block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t inc = v;
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63u) wsum[wid] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (uint32_t w = 0; w < nw; w++) {
    const uint32_t s = wsum[w];
    off += w < wid ? s : 0u;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return off + inc - v;
}

__global__ __launch_bounds__(1024) void k_adapt_compact(AdaptArgs A) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t cnt[ADAPT_CNT_WORDS];
  if (threadIdx.x < ADAPT_CNT_WORDS) cnt[threadIdx.x] = 0;
  const uint32_t nG = A.gx * A.gy;
  uint32_t base = 0, px = 0, t[7] = {0, 0, 0, 0, 0, 0, 0};
  for (uint32_t s0 = 0; s0 < nG; s0 += blockDim.x) {
    const uint32_t g = s0 + threadIdx.x;
    const bool act = g < nG && A.retired[g] == 0u;
    if (act) {
      const uint32_t x8 = g % A.gx, y8 = g / A.gx;
      const uint32_t cw = min(8u, A.width - x8 * 8u), ch = min(8u, A.height - y8 * 8u);
      px += cw * ch;
#pragma unroll
      for (int s = 0; s < 7; s++) t[s] += ((cw + kTileW[s] - 1u) / kTileW[s]) * ((ch + kTileH[s] - 1u) / kTileH[s]);
    }
    uint32_t tot;
    const uint32_t off = block_scan(act ? 1u : 0u, wsum, tot);
    if (act) A.list[base + off] = g;
    base += tot;
  }
  __syncthreads();
  // (integer sums: the same whatever the order of the adds)
  if (px) atomicAdd(&cnt[ADAPT_CNT_PIXELS], px);
#pragma unroll
  for (int s = 0; s < 7; s++)
    if (t[s]) atomicAdd(&cnt[ADAPT_CNT_TILES + s], t[s]);
  __syncthreads();
  if (threadIdx.x < ADAPT_CNT_WORDS) A.counts[threadIdx.x] = threadIdx.x == ADAPT_CNT_GRANULES ? base : cnt[threadIdx.x];
}

__global__ __launch_bounds__(1024) void k_adapt_expand(AdaptArgs A, uint32_t nAct, uint32_t tw, uint32_t th) {
  __shared__ uint32_t wsum[16];
  uint32_t base = 0;
  for (uint32_t s0 = 0; s0 < nAct; s0 += blockDim.x) {
    const uint32_t i = s0 + threadIdx.x;
    uint32_t x0 = 0, y0 = 0, ntx = 0, nty = 0;
    if (i < nAct) {
      const uint32_t g = A.list[i];
      x0 = (g % A.gx) * 8u, y0 = (g / A.gx) * 8u;
      ntx = (min(8u, A.width - x0) + tw - 1u) / tw;
      nty = (min(8u, A.height - y0) + th - 1u) / th;
    }
    uint32_t tot;
    uint32_t* dst = A.tiles + base + block_scan(ntx * nty, wsum, tot);
    for (uint32_t ty = 0; ty < nty; ty++)
      for (uint32_t tx = 0; tx < ntx; tx++) dst[ty * ntx + tx] = (x0 + tx * tw) | ((y0 + ty * th) << 16);
    base += tot;
  }
}

__global__ __launch_bounds__(64) void k_adapt_update(AdaptArgs A) {
  const uint32_t g = A.list[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const uint32_t px = (g % A.gx) * 8u + (lane & 7u), py = (g / A.gx) * 8u + (lane >> 3);
  const bool in = px < A.width && py < A.height;
  const uint32_t K = A.passes[g] + 1u;
  bool conv = false;
  if (in) {
    const size_t pix = (size_t)py * A.width + px;
    const float4 a = A.accum[pix], q = A.prev[pix];
    A.prev[pix] = a;
    const float dx = a.x - q.x, dy = a.y - q.y, dz = a.z - q.z, dw = a.w - q.w;
    const double P = (double)A.P, miss = P - (double)dw;
    const float* bg = A.bg + 3 * pix;
    const double y = (0.2126 * ((double)dx + (double)bg[0] * miss) + 0.7152 * ((double)dy + (double)bg[1] * miss) +
                      0.0722 * ((double)dz + (double)bg[2] * miss)) / P;
    double2 m = A.mom[pix];
    m.x += y;
    m.y += y * y;
    A.mom[pix] = m;
    if (A.threshold > 0.f && K >= A.minPasses && K >= 2u) {
      const double k = (double)K, mean = m.x / k;
      double v = (m.y - m.x * mean) / (k - 1.0);
      if (v < 0.0) v = 0.0;
      const double lim = (double)A.threshold * (mean + (double)A.floor);
      conv = v / k <= lim * lim;
    }
  }
  const unsigned long long open = __ballot(in && !conv);
  if (lane == 0) A.passes[g] = K, A.retired[g] = open == 0ull ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_resolve_adaptive(AdaptArgs A, float* __restrict__ out, uint32_t* __restrict__ sppOut) {
  const uint32_t n = A.width * A.height;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t px = i % A.width, py = i / A.width;
  const uint32_t N = A.passes[(py >> 3) * A.gx + (px >> 3)] * A.P;
  if (sppOut) sppOut[i] = N;
  const float spp = (float)N;
  const float4 a = A.accum[i];
  const float miss = (float)((int)spp - (int)a.w);
  out[3 * i + 0] = a.x / spp + A.bg[3 * i + 0] * miss / spp;
  out[3 * i + 1] = a.y / spp + A.bg[3 * i + 1] * miss / spp;
  out[3 * i + 2] = a.z / spp + A.bg[3 * i + 2] * miss / spp;
}

}  // namespace

hipError_t launch_adapt_compact(const AdaptArgs& A, hipStream_t stream) {
  hipLaunchKernelGGL(k_adapt_compact, dim3(1), dim3(1024), 0, stream, A);
  return hipGetLastError();
}

hipError_t launch_adapt_expand(const AdaptArgs& A, uint32_t nAct, uint32_t tw, uint32_t th, hipStream_t stream) {
  if (nAct == 0) return hipSuccess;
  hipLaunchKernelGGL(k_adapt_expand, dim3(1), dim3(1024), 0, stream, A, nAct, tw, th);
  return hipGetLastError();
}

hipError_t launch_adapt_update(const AdaptArgs& A, uint32_t nAct, hipStream_t stream) {
  if (nAct == 0) return hipSuccess;
  hipLaunchKernelGGL(k_adapt_update, dim3(nAct), dim3(64), 0, stream, A);
  return hipGetLastError();
}

hipError_t launch_resolve_adaptive(const AdaptArgs& A, float* out, uint32_t* spp, hipStream_t stream) {
  const uint32_t n = A.width * A.height;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_resolve_adaptive, dim3((n + 255) / 256), dim3(256), 0, stream, A, out, spp);
  return hipGetLastError();
}

}  // namespace rtk
