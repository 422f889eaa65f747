// aov_kernels.h — first-hit AOVs (arbitrary output variables) of a frame's primary rays: rt_render_aov.
//
// The primary rays of wf_generate (RNG stream of (pixel, sample), jitter_sample, camera_ray), cast through the same
// closest-hit walk (or the exhaustive loop), and at the hit vertex_setup_ray: the shading normal, the hit point and the
// mesh exactly as the frame shades them (Renderer.cpp:42-43).  One lane owns one pixel and loops over the sample range,
// so every sum is formed in float32 in sample order; a wave owns an 8x8-pixel tile, so its rays share nodes.  A miss adds
// nothing.  Channels whose pointer is null are not written.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

template <bool BRUTE>
__global__ __launch_bounds__(64) void k_aov(DevScene S, AovArgs A) {
  __shared__ uint32_t lds[(rtbvh::kMaxDepth + 1) * 64];
  const uint32_t tilesX = (A.width + 7u) / 8u;
  const uint32_t px = (blockIdx.x % tilesX) * 8u + (threadIdx.x & 7u), py = (blockIdx.x / tilesX) * 8u + (threadIdx.x >> 3);
  const bool in = px < A.width && py < A.height;
  const uint32_t pix = py * A.width + px;
  f3 alb = mk(0.f, 0.f, 0.f), nsum = mk(0.f, 0.f, 0.f), psum = mk(0.f, 0.f, 0.f);
  float dsum = 0.f;
  uint32_t nhit = 0, mesh0 = 0xffffffffu, tri0 = 0xffffffffu;
  for (uint32_t smp = A.s0; smp < A.s1; smp++) {  // (wave-uniform: the walk below needs every lane of the wave)
    Rng g{rt_stream_seed(A.seed, RT_STREAM_PIXEL, pix, smp)};
    float sx, sy;
    jitter_sample(g, (int)smp, (int)A.spp, sx, sy);
    f3 o, d;
    camera_ray(S.cam, ((float)px + sx) / (float)A.width, 1.f - ((float)py + sy) / (float)A.height, o, d);
    HitRec h;
    LaneStats st;
    const bool hit = cast<BRUTE, false, false, LT_NONE>(S, in, o, d, lds + threadIdx.x, h, st);
    if (in && hit) {
      f3 nrm, pt;
      uint32_t mesh;
      vertex_setup_ray(S, h.id, o, d, nrm, pt, mesh);
      const rt_material& m = S.mats[mesh];
      alb = alb + mk(m.albedo[0], m.albedo[1], m.albedo[2]);
      nsum = nsum + nrm;
      psum = psum + pt;
      dsum += h.t;
      nhit++;
      if (smp == A.s0) mesh0 = mesh, tri0 = h.id - S.meshTriBegin[mesh];
    }
  }
  if (!in) return;
  const size_t p3 = 3 * (size_t)pix;
  if (A.albedo) A.albedo[p3] = alb.x, A.albedo[p3 + 1] = alb.y, A.albedo[p3 + 2] = alb.z;
  if (A.normal) A.normal[p3] = nsum.x, A.normal[p3 + 1] = nsum.y, A.normal[p3 + 2] = nsum.z;
  if (A.position) A.position[p3] = psum.x, A.position[p3 + 1] = psum.y, A.position[p3 + 2] = psum.z;
  if (A.depth) A.depth[pix] = dsum;
  if (A.hits) A.hits[pix] = nhit;
  if (A.mesh) A.mesh[pix] = mesh0;
  if (A.tri) A.tri[pix] = tri0;
}

hipError_t launch_aov(bool brute_force, const DevScene& S, const AovArgs& A, hipStream_t stream) {
  const uint32_t tiles = ((A.width + 7u) / 8u) * ((A.height + 7u) / 8u);
  if (tiles == 0 || A.s1 <= A.s0) return hipSuccess;
  if (brute_force) hipLaunchKernelGGL(k_aov<true>, dim3(tiles), dim3(64), 0, stream, S, A);
  else hipLaunchKernelGGL(k_aov<false>, dim3(tiles), dim3(64), 0, stream, S, A);
  return hipGetLastError();
}
