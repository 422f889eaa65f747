// aov_views_host_check.cpp — the host side of rt_render_aov_views, rt_render_motion_views and rt_denoise_batch as a
// stand-alone program, for sanitizer runs on the CPU (no GPU, no Python).  It covers what runs without a device: every
// validation path of the six entry points (a rejected call must write nothing: the buffers are filled first and compared
// after; a valid call answers RT_ERR_NO_DEVICE and the context handle is never looked at), and the slice-offset arithmetic
// of the outputs of stacks just below n * w * h = 2^31, computed and checked against 128-bit arithmetic but never dereferenced.  The
// staging of the host forms (device allocations and copies) needs a device and is not covered here.
//
// rt_api.cpp and bvh_build.cpp are compiled with the sanitizers; the kernels' objects come from the product's build
// (make -C ray-tracing-engine_amd) through an archive, from the repository root:
//   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/aov_views_host_check.cpp ray-tracing-engine_amd/csrc/rt_api.cpp ray-tracing-engine_amd/csrc/bvh_build.cpp; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -ffp-contract=off -pthread -Iinclude -Iray-tracing-engine_amd/csrc \
//         -c $f -o $(basename $f).o; done
//   ar rcs kernels.a ray-tracing-engine_amd/build/*.hip.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -pthread aov_views_host_check.cpp.o rt_api.cpp.o bvh_build.cpp.o \
//       -Wl,--whole-archive kernels.a -Wl,--no-whole-archive -o aov_views_host_check
//   ./aov_views_host_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_amd.h"
#include "rt_kernels.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, rt_last_error()); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

constexpr uint32_t W = 12, H = 8, N = 3;
constexpr size_t PX = (size_t)W * H * N;

struct Buffers {
  std::vector<float> f3a, f3b, f3c, f1, f2;
  std::vector<uint32_t> u1, u2, u3;
  Buffers() : f3a(3 * PX, 3.f), f3b(3 * PX, 3.f), f3c(3 * PX, 3.f), f1(PX, 3.f), f2(2 * PX, 3.f), u1(PX, 3u), u2(PX, 3u), u3(PX, 3u) {}
  bool untouched() const {
    for (const auto* v : {&f3a, &f3b, &f3c, &f1, &f2})
      for (float x : *v)
        if (x != 3.f) return false;
    for (const auto* v : {&u1, &u2, &u3})
      for (uint32_t x : *v)
        if (x != 3u) return false;
    return true;
  }
  rt_aov aov() {
    rt_aov a = {};
    a.albedo = f3a.data(), a.normal = f3b.data(), a.position = f3c.data(), a.depth = f1.data();
    a.hits = u1.data(), a.mesh = u2.data(), a.tri = u3.data();
    return a;
  }
  rt_motion motion() {
    rt_motion m = {};
    m.motion = f2.data(), m.position = f3a.data(), m.prev_position = f3b.data(), m.mesh = u1.data();
    return m;
  }
};

rt_params params() {
  rt_params p = {};
  p.width = W, p.height = H, p.spp = 4, p.mode = RT_MODE_PATH, p.max_depth = 3, p.seed = 1, p.rng_mode = RT_RNG_PIXEL, p.world = 1;
  p.tile = 8;
  return p;
}

std::vector<rt_camera> cameras(uint32_t n) {
  std::vector<rt_camera> c(n);
  for (uint32_t j = 0; j < n; ++j)
    for (int k = 0; k < 3; ++k)
      c[j].position[k] = 1.f + j + k, c[j].lower_left[k] = 2.f + j + k, c[j].horizontal[k] = 3.f + k, c[j].vertical[k] = 4.f + k;
  return c;
}

void check_slices() {
  // stacks just below the 2^31 pixels the checks admit (65,535 x 32,767 in one frame, 4,681 x 1,057 x 434,
  // 65,535 x 181 x 181, 32,767 x 65,535 x 1): every slice offset in 64 bits, against 128-bit arithmetic
  struct Case {
    uint32_t n, w, h;
  };
  const Case cases[] = {{1, 65535, 32767}, {4681, 1057, 434}, {65535, 181, 181}, {32767, 65535, 1}};
  for (const Case& c : cases) {
    const unsigned __int128 all = (unsigned __int128)c.n * c.w * c.h;
    EXPECT(all < ((unsigned __int128)1 << 31));
    for (uint32_t ch = 1; ch <= 4; ++ch) {
      const uint32_t views[] = {0, c.n / 2, c.n - 1, c.n};
      for (uint32_t j : views) {
        const unsigned __int128 want = (unsigned __int128)j * c.w * c.h * ch;
        EXPECT((unsigned __int128)rtk::view_slice(j, c.w, c.h, ch) == want);
      }
    }
    // the last element of the last slice of a 3-float channel lies beyond 32 bits' reach whenever the stack is that large
    const size_t last = rtk::view_slice(c.n - 1, c.w, c.h, 3) + 3 * ((size_t)c.w * c.h) - 1;
    EXPECT(last == (size_t)(3 * all - 1));
  }
  EXPECT(rtk::view_slice(1, 65535, 32767, 3) > 0xffffffffull);
}

void check_aov_and_motion() {
  Buffers b;
  rt_ctx* fake = reinterpret_cast<rt_ctx*>(1);
  rt_params p = params();
  std::vector<rt_camera> cams = cameras(N), prevCams = cameras(N);
  const uint32_t seeds[N] = {1, 2, 40000};
  rt_views v = {};
  v.n_views = N, v.cameras = cams.data(), v.seeds = seeds;
  rt_aov a = b.aov();
  rt_motion m = b.motion();
  rt_motion_prev_views pv = {};
  pv.cameras = prevCams.data();

  auto aov = [&](rt_ctx* c, const rt_params* pp, const rt_views* vv, const rt_aov* aa, int want) {
    EXPECT(rt_render_aov_views(c, pp, vv, aa) == want);
    EXPECT(rt_render_aov_views_device(c, pp, vv, aa, nullptr) == want);
  };
  auto mot = [&](rt_ctx* c, const rt_params* pp, const rt_views* vv, const rt_motion_prev_views* pr, const rt_motion* mm, int want) {
    EXPECT(rt_render_motion_views(c, pp, vv, pr, mm) == want);
    EXPECT(rt_render_motion_views_device(c, pp, vv, pr, mm, nullptr) == want);
  };
  auto both = [&](const rt_params* pp, const rt_views* vv, int want) {
    aov(fake, pp, vv, &a, want);
    mot(fake, pp, vv, &pv, &m, want);
  };

  aov(nullptr, &p, &v, &a, RT_ERR_INVALID), aov(fake, nullptr, &v, &a, RT_ERR_INVALID), aov(fake, &p, nullptr, &a, RT_ERR_INVALID);
  aov(fake, &p, &v, nullptr, RT_ERR_INVALID);
  mot(nullptr, &p, &v, &pv, &m, RT_ERR_INVALID), mot(fake, &p, &v, nullptr, &m, RT_ERR_INVALID), mot(fake, &p, &v, &pv, nullptr, RT_ERR_INVALID);
  {
    rt_views x = v;
    x.cameras = nullptr;
    both(&p, &x, RT_ERR_INVALID);
    x = v, x.reserved0 = 1;
    both(&p, &x, RT_ERR_INVALID);
    x = v, x.reserved[5] = 1;
    both(&p, &x, RT_ERR_INVALID);
    x = v, x.n_views = 0;
    both(&p, &x, RT_ERR_INVALID);
    x = v, x.n_views = 65536;  // (rejected before cameras[3..] would be read)
    both(&p, &x, RT_ERR_INVALID);
  }
  {
    rt_aov x = a;
    x.reserved[3] = 1;
    aov(fake, &p, &v, &x, RT_ERR_INVALID);
    rt_motion y = m;
    y.reserved[0] = 1;
    mot(fake, &p, &v, &pv, &y, RT_ERR_INVALID);
    rt_motion_prev_views z = pv;
    z.reserved[1] = 1;
    mot(fake, &p, &v, &z, &m, RT_ERR_INVALID);
  }
  {
    rt_params x = p;
    x.width = 0;
    both(&x, &v, RT_ERR_INVALID);
    x = p, x.height = 65536;
    both(&x, &v, RT_ERR_INVALID);
    x = p, x.spp = 0;
    both(&x, &v, RT_ERR_INVALID);
    x = p, x.spp_begin = 3, x.spp_count = 2;
    both(&x, &v, RT_ERR_INVALID);
    x = p, x.tile = 4;
    both(&x, &v, RT_ERR_INVALID);
    x = p, x.world = 2;
    both(&x, &v, RT_ERR_UNSUPPORTED);
    x = p, x.rng_mode = RT_RNG_LEGACY;
    both(&x, &v, RT_ERR_UNSUPPORTED);
    // 2^31 pixels over the views: rejected before cameras[3..] would be read
    rt_views many = v;
    many.n_views = 40000;
    x = p, x.width = 256, x.height = 256;
    both(&x, &many, RT_ERR_INVALID);
  }
  for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
    std::vector<rt_camera> c2 = cams;
    c2[2].vertical[1] = bad;
    rt_views x = v;
    x.cameras = c2.data();
    both(&p, &x, RT_ERR_INVALID);
    EXPECT(strstr(rt_last_error(), "view 2") != nullptr);
    std::vector<rt_camera> p2 = prevCams;
    p2[1].position[2] = -bad;
    rt_motion_prev_views z = pv;
    z.cameras = p2.data();
    mot(fake, &p, &v, &z, &m, RT_ERR_INVALID);
    EXPECT(strstr(rt_last_error(), "view 1") != nullptr);
  }
  // valid calls, the fields the passes ignore set to values rt_render would refuse: no device here
  rt_params q = p;
  q.mode = 7, q.max_depth = 9, q.use_photons = 1, q.k = 300, q.reserved[2] = 1;
  both(&p, &v, RT_ERR_NO_DEVICE), both(&q, &v, RT_ERR_NO_DEVICE);
  rt_motion_prev_views none = {};
  mot(fake, &p, &v, &none, &m, RT_ERR_NO_DEVICE);
  EXPECT(b.untouched());
}

void check_denoise() {
  Buffers b;
  rt_ctx* fake = reinterpret_cast<rt_ctx*>(1);
  rt_denoise_params d = {};
  d.width = W, d.height = H;
  rt_aov a = b.aov();
  float *rgb = b.f3a.data(), *out = b.f3b.data();
  auto call = [&](rt_ctx* c, const rt_denoise_params* dd, uint32_t n, const float* r, const rt_aov* aa, float* o, int want) {
    EXPECT(rt_denoise_batch(c, dd, n, r, aa, o) == want);
    EXPECT(rt_denoise_batch_device(c, dd, n, r, aa, o, nullptr) == want);
  };
  call(nullptr, &d, N, rgb, &a, out, RT_ERR_INVALID), call(fake, nullptr, N, rgb, &a, out, RT_ERR_INVALID);
  call(fake, &d, N, nullptr, &a, out, RT_ERR_INVALID), call(fake, &d, N, rgb, nullptr, out, RT_ERR_INVALID);
  call(fake, &d, N, rgb, &a, nullptr, RT_ERR_INVALID);
  rt_aov x = a;
  x.hits = nullptr;
  call(fake, &d, N, rgb, &x, out, RT_ERR_INVALID);
  x = a, x.reserved[0] = 1;
  call(fake, &d, N, rgb, &x, out, RT_ERR_INVALID);
  rt_denoise_params y = d;
  y.reserved[4] = 1;
  call(fake, &y, N, rgb, &a, out, RT_ERR_INVALID);
  y = d, y.width = 0;
  call(fake, &y, N, rgb, &a, out, RT_ERR_INVALID);
  y = d, y.iterations = 9;
  call(fake, &y, N, rgb, &a, out, RT_ERR_INVALID);
  y = d, y.sigma_normal = std::numeric_limits<float>::quiet_NaN();
  call(fake, &y, N, rgb, &a, out, RT_ERR_INVALID);
  call(fake, &d, 0, rgb, &a, out, RT_ERR_INVALID);
  y = d, y.width = 32768, y.height = 32768;
  call(fake, &y, 2, rgb, &a, out, RT_ERR_INVALID);
  y = d, y.width = 1, y.height = 1;
  call(fake, &y, 1u << 31, rgb, &a, out, RT_ERR_INVALID);
  call(fake, &y, 0xffffffffu, rgb, &a, out, RT_ERR_INVALID);
  // valid, the largest stack included (nothing is dereferenced without a device), rgb == out
  call(fake, &d, N, rgb, &a, out, RT_ERR_NO_DEVICE), call(fake, &d, N, rgb, &a, rgb, RT_ERR_NO_DEVICE);
  call(fake, &y, (1u << 31) - 1, rgb, &a, out, RT_ERR_NO_DEVICE);
  EXPECT(b.untouched());
}

}  // namespace

int main() {
  int n = 0;
  if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
    fprintf(stderr, "this program is for machines without a GPU: with one, the fake context handle would be dereferenced\n");
    return 2;
  }
  check_slices();
  check_aov_and_motion();
  check_denoise();
  if (failures) {
    fprintf(stderr, "FAILED: %d checks\n", failures);
    return 1;
  }
  printf("aov_views_host_check: validation paths and slice offsets ok\n");
  return 0;
}
