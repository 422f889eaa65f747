// rays_kernels.h — the integrator over ray batches of the caller's: rt_render_rays.
//
// Row r of the accumulator is what pixel (0, 0) of a frame holds whose camera_ray returned (o_r, unit3(d_r)) for every
// sample and whose pixel index in the RNG stream is the row's key: sample i seeds rt_stream_seed(seed, RT_STREAM_PIXEL,
// key, i), draws jitter_sample and discards it, and from the primary cast on runs render_tile's own device functions —
// cast, vertex_setup_ray, the light samples in light order, hemisphere_sample after every shaded vertex, c0 + (c1 +
// (c2 + 0)), clamp01 — so the bits are the frame's.  One lane owns one ray and loops over the sample range: its sums are
// float32 adds in sample order and no hand-over between lanes is needed.  64 consecutive rays make a wave; nothing is
// assumed about their coherence.
//
// POOLED = true (BVH, at most POOL_L lights): the shadow and bounce rays of the wave's vertices go through vertex_pool's
// LT_NONE instance, as the frame's pooled branch sends them.  POOLED = false (the exhaustive loop, more lights, or
// rt_params.reserved[1] bit 0): every vertex is shaded by its own lane, one light after the other (shade_direct_seq), and
// the bounce ray is cast by the same lane.  The two give the same bits.  Measured on 2^20 rays the pool
// takes 0.68 of the sequential body's time on a frame's own primary rays and 0.59 on rays that leave surfaces in
// hemisphere directions: the secondary rays of 64 unrelated vertices end at very different times, which is the case the
// pool's hand-out and stealing exist for.
// A primary ray that starts beyond S.originBound takes the exhaustive loop (k_trace's rule); a row whose direction is
// degenerate (not finite, or null after unit3: ao_finite's test) is a primary miss that casts nothing.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

template <bool BRUTE, bool POOLED, bool STATS>
__global__ __launch_bounds__(BLOCK, STATS ? 1 : 4) void k_render_rays(DevScene S, RaysArgs A, float4* __restrict__ accum,
                                                                     unsigned long long* __restrict__ counters) {
  static_assert(!POOLED || !BRUTE, "the vertex pool serves BVH direct lighting");
  // dynamic LDS: [A.stackLevels][64] traversal stack, then (POOLED) the ray pool
  uint32_t* stack = g_lds + (threadIdx.x & 63u);
  uint32_t* pool = g_lds + A.stackLevels * BLOCK;
  const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;  // (n < 2^31: no wrap)
  const bool in = r < A.n;
  f3 o0 = mk(0.f, 0.f, 0.f), d0 = o0;
  uint32_t key = r;
  if (in) {
    o0 = ld(A.rays[r].origin), d0 = unit3(ld(A.rays[r].direction));
    if (A.streamIndex) key = A.streamIndex[r];
  }
  const bool ok = in && ao_finite(d0) && (d0.x != 0.f || d0.y != 0.f || d0.z != 0.f);
  // origins beyond the range the box padding was derived for are outside the exactness argument of the slab test
  // (k_trace): the exhaustive loop for the primary ray; every later ray starts on a surface
  const bool far = !BRUTE && ok && fmaxf(fmaxf(fabsf(o0.x), fabsf(o0.y)), fabsf(o0.z)) > S.originBound;
  float4 sum = in ? accum[r] : make_float4(0.f, 0.f, 0.f, 0.f);
  LaneStats st;
  const int nvert = A.mode == RT_MODE_PATH ? (int)A.max_depth : 1;
  for (uint32_t i = A.s0; i < A.s1; i++) {  // (wave-uniform: the walks below need every lane of the wave)
    Rng g{rt_stream_seed(A.seed, RT_STREAM_PIXEL, key, i)};
    float sx, sy;
    jitter_sample(g, (int)i, (int)A.spp, sx, sy);  // (discarded: the stream is then where the frame's is)
    f3 o = o0, d = d0;
    f3 c0 = mk(0.f, 0.f, 0.f), c1 = c0, c2 = c0;
    bool primary = true, alive = ok;
    HitRec h;
    if (alive) st.closest++;
    bool hit0 = cast<BRUTE, false, STATS>(S, alive && !far, o, d, stack, h, st);
    if (far) hit0 = brute<false, STATS>(S, o, d, h, st);
    if (alive && !hit0) primary = false, alive = false;
    for (int depth = 0; depth < nvert; depth++) {
      if (wave_ballot(alive) == 0) break;
      const bool bounce = A.mode == RT_MODE_PATH && depth + 1 < nvert;  // wave-uniform
      f3 nrm = mk(0.f, 0.f, 0.f), pt = nrm, bdir = nrm, c = nrm;
      uint32_t mesh = 0;
      if (alive) vertex_setup_ray(S, h.id, o, d, nrm, pt, mesh);
      HitRec nh;
      bool nfound = false;
      if constexpr (POOLED) {
        c = vertex_pool<STATS, LT_NONE, true>(S, alive, bounce, g, d, mesh, nrm, pt, bdir, stack, pool, nh, nfound, st);
      } else {
        if (alive) {
          h.mesh = mesh;
          c = shade_direct_seq<BRUTE, STATS>(S, g, d, h, stack, nrm, pt, st);
          // drawn after every shaded vertex (Renderer.cpp:164); after the last one the stream ends
          if (bounce) bdir = hemisphere_sample(g, nrm), st.closest++;
        }
        if (bounce) nfound = cast<BRUTE, false, STATS>(S, alive, pt, bdir, stack, nh, st);
      }
      if (alive) {
        if (depth == 0) c0 = c;
        else if (depth == 1) c1 = c;
        else c2 = c;
        o = pt, d = bdir, h = nh;
        if (!nfound) alive = false;
      }
    }
    // calculateColorPath returns c0 + (c1 + (c2 + 0)) for finalDepth <= 3
    const f3 total = c0 + (c1 + (c2 + mk(0.f, 0.f, 0.f)));
    if (ok) {
      sum.x += clamp01(total.x), sum.y += clamp01(total.y), sum.z += clamp01(total.z);
      if (primary) sum.w += 1.f;
    }
  }
  if (in) accum[r] = sum;
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_render_rays folds the stripes)
}

hipError_t launch_render_rays(bool brute_force, bool stats, const DevScene& S, const RaysArgs& A, float4* accum,
                              unsigned long long* counters, hipStream_t stream) {
  if (A.n == 0 || A.s1 <= A.s0) return hipSuccess;
  const dim3 grid((A.n + BLOCK - 1) / BLOCK), block(BLOCK);
  // the vertex pool handles up to POOL_L lights, as in launch_render
  const bool pooled = !brute_force && (A.flags & 1u) && S.n_lights <= (uint32_t)POOL_L;
  const size_t ldsBytes = 4u * ((size_t)A.stackLevels * BLOCK + (pooled ? VP_WORDS : 0));
#define RT_LAUNCH_RAYS(BR, PL)                                                                                            \
  do {                                                                                                                    \
    if (stats) hipLaunchKernelGGL((k_render_rays<BR, PL, true>), grid, block, ldsBytes, stream, S, A, accum, counters);  \
    else hipLaunchKernelGGL((k_render_rays<BR, PL, false>), grid, block, ldsBytes, stream, S, A, accum, counters);       \
  } while (0)
  if (brute_force) RT_LAUNCH_RAYS(true, false);
  else if (pooled) RT_LAUNCH_RAYS(false, true);
  else RT_LAUNCH_RAYS(false, false);
#undef RT_LAUNCH_RAYS
  if (!stats) hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  return hipGetLastError();
}
