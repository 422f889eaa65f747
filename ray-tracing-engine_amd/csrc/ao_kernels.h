// ao_kernels.h — ambient occlusion and bent normals at the first hit: rt_render_ao.
//
// The primary rays and hits of k_aov (aov_kernels.h), and at every hit n_rays occlusion rays: ray j of sample i of pixel
// pix draws its direction with hemisphere_sample from a stream of its own, rt_stream_seed(seed, RT_STREAM_AO, pix,
// i * n_rays + j), starts at X + bias * d and is occluded iff a triangle passes the walker's test with t > 0 (and, BOUNDED,
// t < maxDistance: the closest-hit walker with its bound preset, so Trav is untouched).  Per pixel: the rays that escaped
// (integer), the hit samples (integer), and the float32 sum of the escaped directions in (sample, j) order.
//
// One wave owns an 8x8 tile, one lane a pixel, the full-depth LDS stack of k_aov.  A lane loops over the rays of its own
// vertex, every lane of the wave in every walk; lanes whose primary ray missed sit the walks out.  (A pooled schedule —
// the wave's nhit * n_rays rays of a sample dealt over all 64 lanes through LDS, which the per-ray streams allow — was
// built, gave the same bits and lost on every measured frame: DESIGN.md §6j has its numbers.)
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

// Is the ray (o, d) of a lane that is `on` occluded?  Wave-uniform call sites: every lane of the wave takes part in the walk.
template <bool BRUTE, bool BOUNDED>
RT_DEV bool ao_occluded(const DevScene& S, bool on, f3 o, f3 d, float maxDistance, uint32_t* stack) {
  HitRec h;
  LaneStats st;
  if constexpr (BRUTE) {
    if (BOUNDED) return on && brute<false, false>(S, o, d, h, st) && h.t < maxDistance;
    return on && brute<true, false>(S, o, d, h, st);
  } else if constexpr (!BOUNDED) {
    return traverse<true, false, LT_NONE>(S, on, o, d, stack, h, st);
  } else {
    // the closest-hit walker accepts t < best only (on t == best the lower id, and no id is below bestId = 0): with best
    // preset it finds a hit iff one exists with 0 < t < maxDistance, and culls every box that starts beyond
    Trav<TRAV_CLOSEST, LT_NONE> T;
    T.idle(stack);
    if (on) T.start(o, d, S.invBoxScale), T.best = maxDistance;
    while (wave_ballot(T.live()) != 0) T.template round<false>(S, st);
    return T.found;
  }
}

RT_DEV bool ao_finite(f3 d) { return fabsf(d.x) < INFINITY && fabsf(d.y) < INFINITY && fabsf(d.z) < INFINITY; }

template <bool BRUTE, bool BOUNDED>
__global__ __launch_bounds__(64) void k_ao(DevScene S, AoArgs A) {
  __shared__ uint32_t lds[(rtbvh::kMaxDepth + 1) * 64];
  const uint32_t tilesX = (A.width + 7u) / 8u;
  const uint32_t tile = blockIdx.x;
  const uint32_t px = (tile % tilesX) * 8u + (threadIdx.x & 7u), py = (tile / tilesX) * 8u + (threadIdx.x >> 3);
  const bool in = px < A.width && py < A.height;
  const uint32_t pix = py * A.width + px;
  float bias = A.bias;
  if (bias == 0.f) {  // 1e-4 of the diagonal of the referenced vertices' box (launch_ref_extent has reduced it on this stream)
    const float dx = o2f(A.ext[3]) - o2f(A.ext[0]), dy = o2f(A.ext[4]) - o2f(A.ext[1]), dz = o2f(A.ext[5]) - o2f(A.ext[2]);
    bias = 1e-4f * __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
  }
  f3 bent = mk(0.f, 0.f, 0.f);
  uint32_t nhit = 0, unocc = 0;
  for (uint32_t smp = A.s0; smp < A.s1; smp++) {  // (wave-uniform: the walks below need every lane of the wave)
    Rng g{rt_stream_seed(A.seed, RT_STREAM_PIXEL, pix, smp)};
    float sx, sy;
    jitter_sample(g, (int)smp, (int)A.spp, sx, sy);
    f3 o, d;
    camera_ray(S.cam, ((float)px + sx) / (float)A.width, 1.f - ((float)py + sy) / (float)A.height, o, d);
    HitRec h;
    LaneStats st;
    const bool has = cast<BRUTE, false, false, LT_NONE>(S, in, o, d, lds + threadIdx.x, h, st) && in;
    f3 nrm = mk(0.f, 0.f, 0.f), pt = mk(0.f, 0.f, 0.f);
    if (has) {
      uint32_t mesh;
      vertex_setup_ray(S, h.id, o, d, nrm, pt, mesh);
      nhit++;
    }
    for (uint32_t j = 0; j < A.nRays; j++) {  // (wave-uniform too)
      f3 ad = mk(0.f, 0.f, 0.f), ao = ad;
      if (has) {
        Rng ga{rt_stream_seed(A.seed, RT_STREAM_AO, pix, smp * A.nRays + j)};
        ad = hemisphere_sample(ga, nrm);
        ao = pt + bias * ad;
      }
      const bool occ = ao_occluded<BRUTE, BOUNDED>(S, has, ao, ad, A.maxDistance, lds + threadIdx.x);
      if (has && !occ) {
        unocc++;
        if (ao_finite(ad)) bent = bent + ad;  // (a direction that is not finite is counted and adds nothing)
      }
    }
  }
  if (!in) return;
  if (A.unoccluded) A.unoccluded[pix] = unocc;
  if (A.hits) A.hits[pix] = nhit;
  if (A.bent) A.bent[3 * (size_t)pix] = bent.x, A.bent[3 * (size_t)pix + 1] = bent.y, A.bent[3 * (size_t)pix + 2] = bent.z;
}

hipError_t launch_ao(bool brute_force, const DevScene& S, const AoArgs& A, hipStream_t stream) {
  const uint32_t tiles = ((A.width + 7u) / 8u) * ((A.height + 7u) / 8u);
  if (tiles == 0 || A.s1 <= A.s0) return hipSuccess;
  const bool bounded = A.maxDistance > 0.f;
  if (brute_force) {
    if (bounded) hipLaunchKernelGGL((k_ao<true, true>), dim3(tiles), dim3(64), 0, stream, S, A);
    else hipLaunchKernelGGL((k_ao<true, false>), dim3(tiles), dim3(64), 0, stream, S, A);
  } else {
    if (bounded) hipLaunchKernelGGL((k_ao<false, true>), dim3(tiles), dim3(64), 0, stream, S, A);
    else hipLaunchKernelGGL((k_ao<false, false>), dim3(tiles), dim3(64), 0, stream, S, A);
  }
  return hipGetLastError();
}

// RT_UNIT_HEMISPHERE (rt_test_unit): hemisphere_sample from a given engine state.  in: state, normal xyz; out: direction
// xyz, end state.  (a kernel of its own: k_unit stays the kernel it was)
__global__ void k_unit_hemisphere(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* a = in + 4 * (size_t)i;
  Rng g{a[0]};
  const f3 d = hemisphere_sample(g, mk(__uint_as_float(a[1]), __uint_as_float(a[2]), __uint_as_float(a[3])));
  uint32_t* o = out + 4 * (size_t)i;
  o[0] = __float_as_uint(d.x), o[1] = __float_as_uint(d.y), o[2] = __float_as_uint(d.z), o[3] = g.s;
}
