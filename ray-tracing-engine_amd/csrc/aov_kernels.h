// aov_kernels.h — first-hit AOVs (arbitrary output variables) of a frame's primary rays: rt_render_aov, and of the frames
// of many cameras in one launch: rt_render_aov_views.
//
// The primary rays of wf_generate (RNG stream of (pixel, sample), jitter_sample, camera_ray), cast through the same
// closest-hit walk (or the exhaustive loop), and at the hit vertex_setup_ray: the shading normal, the hit point and the
// mesh exactly as the frame shades them (Renderer.cpp:42-43).  One lane owns one pixel and loops over the sample range,
// so every sum is formed in float32 in sample order; a wave owns an 8x8-pixel tile, so its rays share nodes.  A miss adds
// nothing.  Channels whose pointer is null are not written.
// (included by rt_kernels.hip inside namespace rtk: shares its device functions)

// The view of a wave of a multi-view pass (k_aov<.., true>, k_motion<.., true>): workgroup b of the launch is tile
// b % tilesPerView of view b / tilesPerView.  The block index is wave-uniform, so the view's record is read with scalar
// loads through the constant address space and stays in SGPRs, as render_tile reads it.
struct ViewOfWave {
  uint32_t view, tile;
  rt_camera cam;
  uint32_t seed;
};
RT_DEV ViewOfWave view_of_wave(const ViewRec* views, uint32_t tilesPerView) {
  typedef const __attribute__((address_space(4))) ViewRec* const_view_ptr;
  ViewOfWave w;
  w.view = blockIdx.x / tilesPerView, w.tile = blockIdx.x - w.view * tilesPerView;
  const const_view_ptr R = (const_view_ptr)views + w.view;
  for (int j = 0; j < 3; ++j)
    w.cam.position[j] = R->cam.position[j], w.cam.lower_left[j] = R->cam.lower_left[j],
    w.cam.horizontal[j] = R->cam.horizontal[j], w.cam.vertical[j] = R->cam.vertical[j];
  w.seed = R->seed;
  return w;
}

// VIEWS = false: the frame of S.cam and A.seed, one workgroup per tile (rt_render_aov; the instance reads none of the view
// fields and is the kernel it was before they existed).  VIEWS = true: n_views x A.tilesPerView workgroups, view-major; the tile,
// the camera and the seed are the wave's view's, the pixel index that feeds the RNG stream is local to the view, and every
// channel is written into the view's slice (view_slice, in 64 bits).
// VCOL (rt_render_aov_colors): the albedo channel sums the colour interpolated from A.vcol at the hit (vertex_color)
// instead of the mesh's albedo; the other instances do not read A.vcol and are the kernels they were before it existed.
// TEX (rt_render_aov_textured): the albedo channel sums the sample of the hit mesh's texture (tex_color), or the mesh's
// albedo where it has none, from A's four tex* tables; the other instances do not read them.
// VIEWS with VCOL or TEX (rt_render_aov_views_albedo): both at once, each as above.
// launch_aov (below) picks the instance: views null is the single-view form, the surface part of `surface` the channel.
template <bool BRUTE, bool VIEWS, bool VCOL = false, bool TEX = false>
__global__ __launch_bounds__(64) void k_aov(DevScene S, AovArgs A) {
  __shared__ uint32_t lds[(rtbvh::kMaxDepth + 1) * 64];
  ViewOfWave vw;
  if constexpr (VIEWS) vw = view_of_wave(A.views, A.tilesPerView);
  const uint32_t tilesX = (A.width + 7u) / 8u;
  const uint32_t tile = VIEWS ? vw.tile : blockIdx.x;
  const uint32_t px = (tile % tilesX) * 8u + (threadIdx.x & 7u), py = (tile / tilesX) * 8u + (threadIdx.x >> 3);
  const bool in = px < A.width && py < A.height;
  const uint32_t pix = py * A.width + px;
  f3 alb = mk(0.f, 0.f, 0.f), nsum = mk(0.f, 0.f, 0.f), psum = mk(0.f, 0.f, 0.f);
  float dsum = 0.f;
  uint32_t nhit = 0, mesh0 = 0xffffffffu, tri0 = 0xffffffffu;
  for (uint32_t smp = A.s0; smp < A.s1; smp++) {  // (wave-uniform: the walk below needs every lane of the wave)
    Rng g{rt_stream_seed(VIEWS ? vw.seed : A.seed, RT_STREAM_PIXEL, pix, smp)};
    float sx, sy;
    jitter_sample(g, (int)smp, (int)A.spp, sx, sy);
    f3 o, d;
    camera_ray(VIEWS ? vw.cam : S.cam, ((float)px + sx) / (float)A.width, 1.f - ((float)py + sy) / (float)A.height, o, d);
    HitRec h;
    LaneStats st;
    const bool hit = cast<BRUTE, false, false, LT_NONE>(S, in, o, d, lds + threadIdx.x, h, st);
    if (in && hit) {
      f3 nrm, pt;
      uint32_t mesh;
      if constexpr (VCOL) {
        uint4 tv;
        float u, v;
        vertex_setup_ray(S, h.id, o, d, nrm, pt, tv, u, v);
        mesh = tv.w;
        alb = alb + vertex_color(A.vcol, tv, u, v);
      } else if constexpr (TEX) {
        uint4 tv;
        float u, v;
        vertex_setup_ray(S, h.id, o, d, nrm, pt, tv, u, v);
        mesh = tv.w;
        bool textured;
        const f3 c = tex_color(TexRec{A.texUv, A.texMesh, A.texDesc, A.texels}, tv, u, v, textured);
        const rt_material& m = S.mats[mesh];
        alb = alb + (textured ? c : mk(m.albedo[0], m.albedo[1], m.albedo[2]));
      } else {
        vertex_setup_ray(S, h.id, o, d, nrm, pt, mesh);
        const rt_material& m = S.mats[mesh];
        alb = alb + mk(m.albedo[0], m.albedo[1], m.albedo[2]);
      }
      nsum = nsum + nrm;
      psum = psum + pt;
      dsum += h.t;
      nhit++;
      if (smp == A.s0) mesh0 = mesh, tri0 = h.id - S.meshTriBegin[mesh];
    }
  }
  if (!in) return;
  const size_t p1 = (VIEWS ? view_slice(vw.view, A.width, A.height, 1) : 0) + pix, p3 = 3 * p1;
  if (A.albedo) A.albedo[p3] = alb.x, A.albedo[p3 + 1] = alb.y, A.albedo[p3 + 2] = alb.z;
  if (A.normal) A.normal[p3] = nsum.x, A.normal[p3 + 1] = nsum.y, A.normal[p3 + 2] = nsum.z;
  if (A.position) A.position[p3] = psum.x, A.position[p3 + 1] = psum.y, A.position[p3 + 2] = psum.z;
  if (A.depth) A.depth[p1] = dsum;
  if (A.hits) A.hits[p1] = nhit;
  if (A.mesh) A.mesh[p1] = mesh0;
  if (A.tri) A.tri[p1] = tri0;
}

template <bool VCOL, bool TEX>
static void launch_aov_instance(bool brute_force, dim3 grid, hipStream_t stream, const DevScene& S, const AovArgs& A) {
  if (A.views) {
    if (brute_force) hipLaunchKernelGGL((k_aov<true, true, VCOL, TEX>), grid, dim3(64), 0, stream, S, A);
    else hipLaunchKernelGGL((k_aov<false, true, VCOL, TEX>), grid, dim3(64), 0, stream, S, A);
  } else {
    if (brute_force) hipLaunchKernelGGL((k_aov<true, false, VCOL, TEX>), grid, dim3(64), 0, stream, S, A);
    else hipLaunchKernelGGL((k_aov<false, false, VCOL, TEX>), grid, dim3(64), 0, stream, S, A);
  }
}

hipError_t launch_aov(bool brute_force, const DevScene& S, const AovArgs& A, const ViewRec* views, uint32_t nViews,
                      const FrameVariant& surface, hipStream_t stream) {
  AovArgs C = A;
  // the albedo channel's tables: a record with a null one is refused whatever the launch's size
  if (surface.surface == FrameVariant::VCOL) {
    const VColRec* R = static_cast<const VColRec*>(surface.rec);
    if (!R || SurfVCol::refused(*R)) return hipErrorInvalidValue;
    C.vcol = R->vcol;
  } else if (surface.surface == FrameVariant::TEX) {
    const TexRec* T = static_cast<const TexRec*>(surface.rec);
    if (!T || SurfTex::refused(*T)) return hipErrorInvalidValue;
    C.texUv = T->uv, C.texMesh = T->meshTex, C.texDesc = T->desc, C.texels = T->texels;
  } else if (surface.surface != FrameVariant::NONE) return hipErrorInvalidValue;  // (no albedo channel of material maps)
  const uint32_t tiles = ((A.width + 7u) / 8u) * ((A.height + 7u) / 8u);
  if (views) C.views = views, C.tilesPerView = tiles;
  if (tiles == 0 || (views && nViews == 0) || A.s1 <= A.s0) return hipSuccess;
  if (views && (uint64_t)tiles * nViews > 0x7fffffffull) return hipErrorInvalidValue;  // (a tile holds a pixel: n w h < 2^31 keeps it below)
  const dim3 grid(views ? tiles * nViews : tiles);
  if (surface.surface == FrameVariant::VCOL) launch_aov_instance<true, false>(brute_force, grid, stream, S, C);
  else if (surface.surface == FrameVariant::TEX) launch_aov_instance<false, true>(brute_force, grid, stream, S, C);
  else launch_aov_instance<false, false>(brute_force, grid, stream, S, C);
  return hipGetLastError();
}
