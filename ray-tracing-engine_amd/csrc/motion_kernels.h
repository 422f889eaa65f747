// motion_kernels.h — where was this pixel's surface point last frame: rt_render_motion, and rt_render_motion_views for the
// frames of many cameras in one launch.
//
// One ray per pixel: the primary ray of sample s0 of the frame (the sample rt_aov.mesh / .tri describe: same stream seed,
// jitter_sample, camera_ray), cast as k_aov casts it.  At the hit, (u, v) as the frame shades with them, the hit point X
// over the context's positions and the same float32 expression X' over LAST frame's positions; both projected to the
// screen in float64 (the inverse of camera_ray by Cramer's rule, rt_amd.h states the order) under their own cameras;
// motion = previous minus current screen position, in pixels.  A wave owns an 8x8-pixel tile, one lane one pixel.
// Channels whose pointer is null are not written.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

// vertex_setup_ray's sibling for the motion pass: the same (u, v) — tri_test on the same operands — and the same hit
// point, and the triangle's vertex ids and (u, v) for the caller; no normal.
RT_DEV void vertex_setup_ray_uv(const DevScene& S, uint32_t id, f3 o, f3 d, uint4& tv, float& u, float& v, f3& point) {
  tv = S.triShade[id];
  const f3 p0 = ld(S.vpos + 3 * (size_t)tv.x), p1 = ld(S.vpos + 3 * (size_t)tv.y), p2 = ld(S.vpos + 3 * (size_t)tv.z);
  float t;
  tri_test(o, d, p0, p1 - p0, p2 - p0, u, v, t, true);
  const float w = 1.f - u - v;
  point = w * p0 + u * p1 + v * p2;
}

struct d3 {
  double x, y, z;
};
RT_DEV d3 dsub(const float* a, const float* b) { return d3{(double)a[0] - (double)b[0], (double)a[1] - (double)b[1], (double)a[2] - (double)b[2]}; }
RT_DEV d3 dld(const float* a) { return d3{(double)a[0], (double)a[1], (double)a[2]}; }
RT_DEV double ddot(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_DEV d3 dcross(d3 a, d3 b) { return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// Screen position (pixels) of the point Y under camera c; false: Y is not in front of the camera.
RT_DEV bool screen_pos(const rt_camera& c, f3 Y, double width, double height, double& sx, double& sy) {
  const float y[3] = {Y.x, Y.y, Y.z};
  const d3 q = dsub(y, c.position), a = dsub(c.lower_left, c.position), H = dld(c.horizontal), V = dld(c.vertical);
  const d3 hv = dcross(H, V);
  const double qn = ddot(q, hv), den = ddot(a, hv);
  const double s = ddot(a, dcross(q, V)) / qn, t = ddot(a, dcross(H, q)) / qn;
  sx = s * width, sy = (1.0 - t) * height;
  return qn / den > 0.0;
}

// VIEWS = false: the frame of S.cam, A.seed and A.prevCam, one workgroup per tile (rt_render_motion; the instance reads
// none of the view fields).  VIEWS = true: n_views x A.tilesPerView workgroups, view-major (aov_kernels.h view_of_wave): the wave's
// view gives the tile, the camera and the seed, A.prevCams[view] last frame's camera (48 bytes, read by scalar loads as the
// view's record is; A.seed and A.prevCam are not read), the pixel index that feeds the RNG stream is local to the view and
// every channel is written into the view's slice.
template <bool BRUTE, bool VIEWS>
__global__ __launch_bounds__(64) void k_motion(DevScene S, MotionArgs A) {
  __shared__ uint32_t lds[(rtbvh::kMaxDepth + 1) * 64];
  ViewOfWave vw;
  rt_camera vprev;
  if constexpr (VIEWS) {
    vw = view_of_wave(A.views, A.tilesPerView);
    typedef const __attribute__((address_space(4))) rt_camera* const_cam_ptr;
    const const_cam_ptr P = (const_cam_ptr)A.prevCams + vw.view;
    for (int j = 0; j < 3; ++j)
      vprev.position[j] = P->position[j], vprev.lower_left[j] = P->lower_left[j], vprev.horizontal[j] = P->horizontal[j],
      vprev.vertical[j] = P->vertical[j];
  }
  const uint32_t tilesX = (A.width + 7u) / 8u;
  const uint32_t tile = VIEWS ? vw.tile : blockIdx.x;
  const uint32_t px = (tile % tilesX) * 8u + (threadIdx.x & 7u), py = (tile / tilesX) * 8u + (threadIdx.x >> 3);
  const bool in = px < A.width && py < A.height;
  const uint32_t pix = py * A.width + px;
  Rng g{rt_stream_seed(VIEWS ? vw.seed : A.seed, RT_STREAM_PIXEL, pix, A.s0)};
  float jx, jy;
  jitter_sample(g, (int)A.s0, (int)A.spp, jx, jy);
  f3 o, d;
  camera_ray(VIEWS ? vw.cam : S.cam, ((float)px + jx) / (float)A.width, 1.f - ((float)py + jy) / (float)A.height, o, d);
  HitRec h;
  LaneStats st;
  const bool hit = cast<BRUTE, false, false, LT_NONE>(S, in, o, d, lds + threadIdx.x, h, st);
  if (!in) return;
  f3 X = mk(0.f, 0.f, 0.f), Xp = mk(0.f, 0.f, 0.f);
  float mx = 0.f, my = 0.f;
  uint32_t mesh = 0xffffffffu;
  if (hit) {
    uint4 tv;
    float u, v;
    vertex_setup_ray_uv(S, h.id, o, d, tv, u, v, X);
    mesh = tv.w;
    const float w = 1.f - u - v;
    Xp = w * ld(A.prevVpos + 3 * (size_t)tv.x) + u * ld(A.prevVpos + 3 * (size_t)tv.y) + v * ld(A.prevVpos + 3 * (size_t)tv.z);
    if (A.motion) {
      const double W = (double)A.width, H = (double)A.height;
      double cx, cy, qx, qy;
      const bool fc = screen_pos(VIEWS ? vw.cam : S.cam, X, W, H, cx, cy), fp = screen_pos(VIEWS ? vprev : A.prevCam, Xp, W, H, qx, qy);
      const bool ok = fc && fp && isfinite(cx) && isfinite(cy) && isfinite(qx) && isfinite(qy);
      mx = ok ? (float)(qx - cx) : INFINITY;
      my = ok ? (float)(qy - cy) : INFINITY;
    }
  }
  const size_t p1 = (VIEWS ? view_slice(vw.view, A.width, A.height, 1) : 0) + pix, p3 = 3 * p1;
  if (A.motion) A.motion[2 * p1] = mx, A.motion[2 * p1 + 1] = my;
  if (A.position) A.position[p3] = X.x, A.position[p3 + 1] = X.y, A.position[p3 + 2] = X.z;
  if (A.prevPosition) A.prevPosition[p3] = Xp.x, A.prevPosition[p3 + 1] = Xp.y, A.prevPosition[p3 + 2] = Xp.z;
  if (A.mesh) A.mesh[p1] = mesh;
}

hipError_t launch_motion(bool brute_force, const DevScene& S, const MotionArgs& A, hipStream_t stream) {
  const uint32_t tiles = ((A.width + 7u) / 8u) * ((A.height + 7u) / 8u);
  if (tiles == 0) return hipSuccess;
  if (brute_force) hipLaunchKernelGGL((k_motion<true, false>), dim3(tiles), dim3(64), 0, stream, S, A);
  else hipLaunchKernelGGL((k_motion<false, false>), dim3(tiles), dim3(64), 0, stream, S, A);
  return hipGetLastError();
}

hipError_t launch_motion_views(bool brute_force, const DevScene& S, const MotionArgs& A, const ViewRec* views, const rt_camera* prevCams,
                               uint32_t nViews, hipStream_t stream) {
  MotionArgs V = A;
  V.views = views, V.prevCams = prevCams, V.tilesPerView = ((A.width + 7u) / 8u) * ((A.height + 7u) / 8u);
  if (V.tilesPerView == 0 || nViews == 0) return hipSuccess;
  if ((uint64_t)V.tilesPerView * nViews > 0x7fffffffull) return hipErrorInvalidValue;  // (a tile holds a pixel: n w h < 2^31 keeps it below)
  if (brute_force) hipLaunchKernelGGL((k_motion<true, true>), dim3(V.tilesPerView * nViews), dim3(64), 0, stream, S, V);
  else hipLaunchKernelGGL((k_motion<false, true>), dim3(V.tilesPerView * nViews), dim3(64), 0, stream, S, V);
  return hipGetLastError();
}
