// TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT.
//
// Driver that compiles the *reference's own sources where they lie* under
// /root/reference/source (via -I, nothing is copied) and exercises their public
// and — through the `private -> public` macro below — private interfaces, so
// that the restatement in oracle/rt_oracle.cpp and the HIP path can be pinned
// to the real thing.  Build recipe: oracle/Makefile (target _ref/ref_harness).
// The produced binary lives in oracle/_ref/ (git-ignored) and is only ever
// executed by tests/, bench.py's cpu_baseline leg and tests/golden/make_golden.py.
//
// Everything in this file is our own code; the scene script below restates the
// constants of reference source/Main.cpp:26-151,165-208 and
// is validated by reproducing the md5 of the stock binary's output (App. C).
//
// Sub-commands
//   render  <meshdir> <scene> <w> <h> <mode> <N> <p> <k> <out.ppm>
//   vectors <meshdir> <out.json>
//   knn     <out.json>                                        (tie-heavy k-NN maps)
//   time    <meshdir> <scene> <w> <h> <mode> <N> <p> <k>     (prints seconds)
//   shading <meshdir> <in.bin> <out.json> <ppm_prefix>        (swept materials, lights, frames: tests/shading_sweep.py)
#define _USE_MATH_DEFINES
#include <assert.h>
// NB: <math.h> must NOT be pre-included: libstdc++'s wrapper would pull the float
// overloads into :: and change what `tan(...)` in Camera.h:15 resolves to.

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

// open the reference classes up for white-box dumps (std headers above are
// already include-guarded, so the macro only touches the reference headers)
#define private public
#define protected public
// same include order as reference source/Main.cpp:13-22 (it decides which
// cmath overloads are visible where)
#include "Camera.h"
#include "CommandLine.h"
#include "Image.cpp"
#include "LightSource.h"
#include "Material.h"
#include "Mesh.h"
#include "Ray.h"
#include "RayTracer.h"
#include "Renderer.cpp"
#include "Scene.h"
#undef private
#undef protected

namespace {

uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// ---------------------------------------------------------------- scene script
void addQuad(Mesh& m, const Vec3f& a, const Vec3f& b, const Vec3f& c,
             const Vec3f& d, const Vec3f& n) {
  int base = (int)m.vertexPositions().size();
  for (const Vec3f& p : {a, b, c, d}) {
    m.vertexPositions().push_back(p);
    m.vertexNormals().push_back(n);
  }
  m.indexedTriangles().push_back(Vec3i(base, base + 1, base + 3));
  m.indexedTriangles().push_back(Vec3i(base, base + 2, base + 3));
}

void spinY(Mesh& m, float phi) {
  // Main.cpp:88-99 — positions only; cos/sin resolve to the float overloads
  // because `using namespace std` (CommandLine.h) is in force here as there.
  float c = cos(phi), s = sin(phi);
  Vec3f r0(c, 0, s), r1(0, 1, 0), r2(-s, 0, c);
  for (Vec3f& p : m.vertexPositions()) {
    Vec3f q(dot(r0, p), dot(r1, p), dot(r2, p));
    p = q;
  }
}

Scene buildScene(const std::string& meshdir, const std::string& kind, size_t w,
                 size_t h) {
  Scene scene;
  scene.camera() = Camera(Vec3f(0.3f, 0.6f, 2.3f), Vec3f(), Vec3f(0.f, 1.f, 0.f),
                          60.f, float(w) / h);
  scene.lightsources().push_back(LightSource(Vec3f(-1.4f, 1.f, 2.9f),
                                             Vec3f(1.f, 1.f, 1.f),
                                             Vec3f(0.3f, 0.f, -1.f), 0.85f, 0.01f));
  scene.lightsources().push_back(LightSource(Vec3f(1.4f, 1.f, 2.9f),
                                             Vec3f(1.f, 1.f, 1.f),
                                             Vec3f(-0.3f, 0.f, -1.f), 0.85f, 0.01f));
  scene.lightsources().push_back(LightSource(Vec3f(0.f, -0.3f, 1.1f),
                                             Vec3f(1.f, 1.f, 1.f),
                                             Vec3f(0.f, 0.f, -1.f), 0.85f, 0.1f));
  Mesh walls, left, right, slot3, slot4;
  Vec3f wallsF0(0.5f, 0.5f, 0.5f);
  walls.material() = Material(0.6f, 0.3f, Vec3f(0.96f, 0.96f, 0.86f), wallsF0);
  left.material() = Material(0.6f, 0.3f, Vec3f(0.9f, 0.3f, 0.3f), wallsF0);
  right.material() = Material(0.6f, 0.3f, Vec3f(0.3f, 0.9f, 0.3f), wallsF0);
  slot3.material() =
      Material(0.1f, 0.1f, Vec3f(0.9f, 0.9f, 0.9f), Vec3f(1.0f, 0.86f, 0.57f));
  slot4.material() =
      Material(0.8f, 0.9f, Vec3f(0.4f, 0.4f, 0.9f), Vec3f(0.3, 0.3, 0.3));

  std::string f3 = "cube_tri.off";
  if (kind == "lowres") f3 = "example_low_res.off";
  else if (kind == "hires") f3 = "example.off";
  else if (kind != "cubes") throw std::runtime_error("unknown scene " + kind);
  slot3.loadOFF(meshdir + "/" + f3);
  slot4.loadOFF(meshdir + "/cube_tri2.off");

  const float B = 1.51f, C = 1.5f;
  addQuad(walls, Vec3f(B, -1.f, B), Vec3f(B, -1.f, -B), Vec3f(-B, -1.f, B),
          Vec3f(-B, -1.f, -B), Vec3f(0.f, 1.f, 0.f));
  addQuad(walls, Vec3f(-B, -1.f, -B), Vec3f(B, -1.f, -B), Vec3f(-B, C, -B),
          Vec3f(B, C, -B), Vec3f(0.f, 0.f, 1.f));
  addQuad(walls, Vec3f(B, C, B), Vec3f(B, C, -B), Vec3f(-B, C, B),
          Vec3f(-B, C, -B), Vec3f(0.f, -1.f, 0.f));
  // left wall x=-B (Main.cpp:64-71), right wall x=+B (:73-81)
  addQuad(left, Vec3f(-B, -1.f, B), Vec3f(-B, -1.f, -B), Vec3f(-B, C, B),
          Vec3f(-B, C, -B), Vec3f(1.f, 0.f, 0.f));
  addQuad(right, Vec3f(B, -1.f, B), Vec3f(B, -1.f, -B), Vec3f(B, C, B),
          Vec3f(B, C, -B), Vec3f(-1.f, 0.f, 0.f));

  spinY(slot3, M_PI / 4.5f);
  spinY(slot4, -M_PI / 4.5f);
  scene.meshes().push_back(walls);
  scene.meshes().push_back(left);
  scene.meshes().push_back(right);
  scene.meshes().push_back(slot3);
  scene.meshes().push_back(slot4);
  return scene;
}

// ------------------------------------------------------------------ JSON bits
struct J {
  std::ostringstream o;
  bool first = true;
  void key(const char* k) {
    if (!first) o << ",\n";
    first = false;
    o << "\"" << k << "\":";
  }
  template <class It>
  void arr(It b, It e) {
    o << "[";
    for (It i = b; i != e; ++i) {
      if (i != b) o << ",";
      o << *i;
    }
    o << "]";
  }
  void u32(const char* k, const std::vector<uint32_t>& v) {
    key(k);
    arr(v.begin(), v.end());
  }
  void i64(const char* k, const std::vector<long long>& v) {
    key(k);
    arr(v.begin(), v.end());
  }
};

void push3(std::vector<uint32_t>& v, const Vec3f& p) {
  v.push_back(fbits(p[0]));
  v.push_back(fbits(p[1]));
  v.push_back(fbits(p[2]));
}

void dumpScene(J& j, const std::string& tag, const Scene& sc) {
  std::vector<uint32_t> pos, nrm, mat, tri, toff, voff;
  uint32_t to = 0, vo = 0;
  for (const Mesh& m : sc.meshes()) {
    toff.push_back(to);
    voff.push_back(vo);
    for (auto& p : m.vertexPositions()) push3(pos, p);
    for (auto& n : m.vertexNormals()) push3(nrm, n);
    for (auto& t : m.indexedTriangles()) {
      tri.push_back(t[0]);
      tri.push_back(t[1]);
      tri.push_back(t[2]);
    }
    to += m.indexedTriangles().size();
    vo += m.vertexPositions().size();
    const Material& M = m.material();
    mat.push_back(fbits(M.m_kd));
    mat.push_back(fbits(M.m_alpha));
    push3(mat, M.m_albedo);
    push3(mat, M.m_F0);
  }
  toff.push_back(to);
  voff.push_back(vo);
  j.u32((tag + "_pos").c_str(), pos);
  j.u32((tag + "_nrm").c_str(), nrm);
  j.u32((tag + "_tri_local").c_str(), tri);
  j.u32((tag + "_tri_off").c_str(), toff);
  j.u32((tag + "_vtx_off").c_str(), voff);
  j.u32((tag + "_mat").c_str(), mat);
  std::vector<uint32_t> cam, lights;
  const Camera& c = sc.camera();
  push3(cam, c.m_position);
  push3(cam, c.m_lowerLeftCorner);
  push3(cam, c.m_horizontal);
  push3(cam, c.m_vertical);
  j.u32((tag + "_cam").c_str(), cam);
  for (const LightSource& l : sc.lightsources()) {
    push3(lights, l.m_position);
    push3(lights, l.m_color);
    push3(lights, l.m_vertical);
    push3(lights, l.m_horizontal);
    push3(lights, l.m_normal);
    lights.push_back(fbits(l.m_intensity));
    lights.push_back(fbits(l.m_sideLength));
    lights.push_back(fbits(l.m_factor));
    lights.push_back(fbits(l.ac));
    lights.push_back(fbits(l.al));
    lights.push_back(fbits(l.aq));
  }
  j.u32((tag + "_lights").c_str(), lights);
}

// deterministic helper stream for building test inputs (NOT the engine `gen`)
struct Lcg {
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed) {}
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  float uni(float a, float b) { return a + (b - a) * (next() / 2147483648.0f); }
};

int cmdVectors(const std::string& meshdir, const std::string& out) {
  J j;
  j.o << "{\n";
  // ---- scenes (cubes in full; lowres in full too: 641 verts, small)
  Scene cubes = buildScene(meshdir, "cubes", 256, 256);
  Scene lowres = buildScene(meshdir, "lowres", 256, 256);
  dumpScene(j, "cubes", cubes);
  dumpScene(j, "lowres", lowres);
  {
    // non-square aspect camera frame
    Scene s = buildScene(meshdir, "cubes", 380, 270);
    std::vector<uint32_t> cam;
    push3(cam, s.camera().m_position);
    push3(cam, s.camera().m_lowerLeftCorner);
    push3(cam, s.camera().m_horizontal);
    push3(cam, s.camera().m_vertical);
    j.u32("cam_380x270", cam);
  }

  // ---- Camera::rayAt on a grid (Camera.h:27-30)
  {
    std::vector<uint32_t> v;
    for (int a = 0; a <= 8; a++)
      for (int b = 0; b <= 8; b++) {
        float u = a / 8.f, w = b / 8.f;
        Ray r = cubes.camera().rayAt(u, w);
        v.push_back(fbits(u));
        v.push_back(fbits(w));
        push3(v, r.origin());
        push3(v, r.direction());
      }
    j.u32("rayAt", v);
  }

  // ---- Ray::triangleIntersect (Ray.cpp:9-24): random, grazing, degenerate
  {
    std::vector<uint32_t> v;
    Lcg g(12345);
    for (int i = 0; i < 600; i++) {
      Vec3f p0(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
      Vec3f p1(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
      Vec3f p2(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
      Vec3f o(g.uni(-2, 2), g.uni(-2, 2), g.uni(-2, 2));
      Vec3f d;
      int kind = i % 6;
      if (kind == 0) {  // aim at the interior
        float a = g.uni(0, 1), b = g.uni(0, 1 - a);
        d = (p0 * (1 - a - b) + p1 * a + p2 * b) - o;
      } else if (kind == 1) {  // aim exactly at an edge point
        float a = g.uni(0, 1);
        d = (p0 * (1 - a) + p1 * a) - o;
      } else if (kind == 2) {  // aim exactly at a vertex
        d = p2 - o;
      } else if (kind == 3) {  // origin on the triangle (self-hit acne case)
        float a = g.uni(0, 1), b = g.uni(0, 1 - a);
        o = p0 * (1 - a - b) + p1 * a + p2 * b;
        d = Vec3f(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
      } else if (kind == 4) {  // nearly parallel to the plane
        Vec3f e = normalize(p1 - p0);
        d = e + normalize(cross(p1 - p0, p2 - p0)) * g.uni(-2e-6f, 2e-6f);
      } else {
        d = Vec3f(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
      }
      if (i % 50 == 49) p2 = p1;  // degenerate triangle
      if (i % 2) d = normalize(d);
      float u = -7.f, w = -7.f, t = -7.f;  // sentinel: outputs may stay unwritten
      bool hit = Ray(o, d).triangleIntersect(p0, p1, p2, u, w, t);
      push3(v, p0);
      push3(v, p1);
      push3(v, p2);
      push3(v, o);
      push3(v, d);
      v.push_back(hit ? 1u : 0u);
      v.push_back(fbits(u));
      v.push_back(fbits(w));
      v.push_back(fbits(t));
    }
    j.u32("triangleIntersect", v);
  }

  // ---- RayTracer::rayTrace (RayTracer.h:27-53): camera, bounce and shadow rays
  auto traceSet = [&](const char* name, const Scene& sc, int n) {
    std::vector<uint32_t> v;
    RayTracer rt;
    Lcg g(777);
    for (int i = 0; i < n; i++) {
      Ray r = sc.camera().rayAt(g.uni(0, 1), g.uni(0, 1));
      for (int hop = 0; hop < 3; hop++) {
        size_t mi = 9999;
        Vec3i tri(-1, -1, -1);
        float u = -7.f, w = -7.f, d = -7.f;
        bool hit = rt.rayTrace(r, sc, mi, tri, u, w, d);
        push3(v, r.origin());
        push3(v, r.direction());
        v.push_back(hit);
        v.push_back((uint32_t)mi);
        v.push_back(tri[0]);
        v.push_back(tri[1]);
        v.push_back(tri[2]);
        v.push_back(fbits(u));
        v.push_back(fbits(w));
        v.push_back(fbits(d));
        if (!hit) break;
        const Mesh& m = sc.meshes()[mi];
        float ww = 1.f - u - w;
        Vec3f p = ww * m.vertexPositions()[tri[0]] + u * m.vertexPositions()[tri[1]] +
                  w * m.vertexPositions()[tri[2]];
        // next ray starts exactly on the surface (no epsilon) like the reference
        Vec3f nd;
        if (hop == 0)
          nd = Vec3f(0.f, -0.3f, 1.1f) - p;  // un-normalised, towards light 2
        else
          nd = normalize(Vec3f(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)));
        r = Ray(p, nd);
      }
    }
    j.u32(name, v);
  };
  traceSet("rayTrace_cubes", cubes, 400);
  traceSet("rayTrace_lowres", lowres, 250);

  // ---- Material::evaluateColorResponse (Material.h:25-70)
  {
    std::vector<uint32_t> v;
    Lcg g(4242);
    for (const Mesh& m : cubes.meshes()) {
      Material M = m.material();
      for (int i = 0; i < 60; i++) {
        Vec3f n(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
        Vec3f wi(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
        Vec3f wo(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
        if (i % 10 == 7) wo = wi * -1.f;            // wh = 0
        if (i % 10 == 8) wi = cross(n, wo);         // grazing n.wi = 0
        if (i % 10 == 9) n = Vec3f(0, 1, 0), wi = Vec3f(0.3f, 0.8f, 0.1f), wo = Vec3f(-0.2f, 0.5f, 0.4f);
        Vec3f r = M.evaluateColorResponse(n, wi, wo);
        push3(v, n);
        push3(v, wi);
        push3(v, wo);
        v.push_back(fbits(M.m_kd));
        v.push_back(fbits(M.m_alpha));
        push3(v, M.m_albedo);
        push3(v, M.m_F0);
        push3(v, r);
      }
    }
    j.u32("bsdf", v);
  }

  // ---- LightSource::evaluateLight (LightSource.h:51-59)
  {
    std::vector<uint32_t> v;
    Lcg g(99);
    for (LightSource l : cubes.lightsources())
      for (int i = 0; i < 20; i++) {
        Vec3f p(g.uni(-1.5f, 1.5f), g.uni(-1.f, 1.5f), g.uni(-1.5f, 1.5f));
        push3(v, p);
        push3(v, l.evaluateLight(p));
      }
    j.u32("evaluateLight", v);
  }

  // ---- the engine and the three samplers, from a fresh seed-1 engine
  {
    gen.seed(1);
    std::vector<uint32_t> raw;
    for (int i = 0; i < 8; i++) raw.push_back((uint32_t)gen());
    j.u32("engine_first8", raw);

    gen.seed(1);
    RayTracer rt;
    std::vector<uint32_t> v;
    for (int N : {1, 2, 4, 8, 16, 128})
      for (int i = 0; i < std::min(N, 12); i++) {
        Vec3f s = rt.jitterSample(i, N);
        v.push_back(N);
        v.push_back(i);
        v.push_back(fbits(s[0]));
        v.push_back(fbits(s[1]));
      }
    j.u32("jitterSample_seq", v);

    gen.seed(1);
    std::vector<uint32_t> a;
    for (int rep = 0; rep < 4; rep++)
      for (LightSource l : cubes.lightsources()) push3(a, l.randAreaPosition());
    j.u32("randAreaPosition_seq", a);

    gen.seed(1);
    std::vector<uint32_t> hs;
    Lcg g(31337);
    for (int i = 0; i < 200; i++) {
      Vec3f n(g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1));
      if (i % 7 == 0) n = Vec3f(0, 1, 0);
      if (i % 7 == 1) n = Vec3f(0, 0, -1);
      if (i % 7 == 2) n = Vec3f(1, 0, 0);
      Vec3f d = rt.hsphereUniformSample(n, M_PI / 2.f);
      push3(hs, n);
      push3(hs, d);
    }
    j.u32("hsphere_seq", hs);
  }

  // ---- photon map (PhotonMap.h:14-50,92-155) + kd-tree order + knearest
  {
    gen.seed(1);
    RayTracer rt;
    PhotonMap pm(cubes, 3000, rt);
    std::vector<uint32_t> ph;
    for (const Particle& p : pm.list()) {
      push3(ph, p.position());
      push3(ph, p.incomeDirection());
      ph.push_back(fbits(p.weight()));
    }
    j.u32("photons_cubes_3000", ph);
    std::vector<uint32_t> after;
    for (int i = 0; i < 4; i++) after.push_back((uint32_t)gen());
    j.u32("photons_cubes_3000_engine_after", after);

    kdtree tree(pm.list().begin(), pm.list().end());
    std::vector<uint32_t> order;  // node array order after make_tree
    for (auto& n : tree.m_nodes) push3(order, n.m_point.position());
    j.u32("kdtree_order_pos", order);

    std::vector<uint32_t> q;
    Lcg g(2024);
    for (int i = 0; i < 300; i++) {
      Particle t;
      if (i % 3 == 0) {
        const Particle& s = pm.list()[g.next() % pm.list().size()];
        t.position() = s.position() + Vec3f(g.uni(-0.05f, 0.05f), g.uni(-0.05f, 0.05f), g.uni(-0.05f, 0.05f));
      } else if (i % 3 == 1) {
        t.position() = Vec3f(g.uni(-1.5f, 1.5f), -1.f, g.uni(-1.5f, 1.5f));
      } else {
        t.position() = Vec3f(g.uni(-1.5f, 1.5f), g.uni(-1.f, 1.5f), g.uni(-1.5f, 1.5f));
      }
      if (i == 299) t.position() = pm.list()[5].position();  // exact hit: bestdist==0 path
      for (int k : {1, 5, 10}) {
        std::vector<Particle> res;
        tree.knearest(t, k, res);
        push3(q, t.position());
        q.push_back(k);
        q.push_back((uint32_t)tree.m_visited);
        for (auto& r : res) {
          push3(q, r.position());
          push3(q, r.incomeDirection());
        }
      }
    }
    j.u32("knearest", q);
  }

  j.o << "\n}\n";
  std::ofstream f(out);
  f << j.o.str();
  return 0;
}

int cmdRender(int argc, char** argv, bool timeOnly) {
  std::string meshdir = argv[2], kind = argv[3];
  size_t w = atoi(argv[4]), h = atoi(argv[5]);
  int mode = atoi(argv[6]), N = atoi(argv[7]), p = atoi(argv[8]), k = atoi(argv[9]);
  std::cout.setstate(std::ios::failbit);  // silence the progress bar
  Scene scene = buildScene(meshdir, kind, w, h);
  Image image(w, h);
  RayTracer rt;
  Renderer renderer;
  if (p > 0)
    renderer = Renderer(scene, N, mode, rt, p, k);
  else
    renderer = Renderer(scene, N, mode, rt);
  image.fillBackground();
  auto t0 = std::chrono::steady_clock::now();
  renderer.render(image);  // writes update.ppm into CWD every pass (Renderer.cpp:268)
  double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout.clear();
  if (!timeOnly) image.savePPM(argv[10]);
  printf("{\"seconds\": %.6f, \"samples\": %zu}\n", s, w * h * (size_t)N);
  return 0;
}

// ---------------------------------------------------------------- k-NN tie maps
// Photon maps on a grid of spacing 1/8 (exact in float), built so that equal
// coordinates and equal distances are the rule: a lattice, repeated positions,
// axis-aligned walls, a line, one point, tiny maps, and the lattice scaled by powers
// of two whose squares underflow, go subnormal, approach FLT_MAX or overflow.
// Photon i of a map has direction (i / 2, 1, n - i): unique, so a result identifies
// its photon even where positions repeat.
struct KnnMap {
  std::string name;
  int scaleExp;
  std::vector<Vec3f> pos;
};

std::vector<KnnMap> knnMaps(Lcg& g) {
  const float s = 0.125f;
  auto shuffle = [&](std::vector<Vec3f>& v) {
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[g.next() % i]);
  };
  auto lattice = [&](int a) {
    std::vector<Vec3f> v;
    for (int x = 0; x < a; x++)
      for (int y = 0; y < a; y++)
        for (int z = 0; z < a; z++) v.push_back(Vec3f(x * s, y * s, z * s));
    shuffle(v);
    return v;
  };
  auto grid = [&](int lo, int hi) { return (float)((int)(g.next() % (uint32_t)(hi - lo + 1)) + lo) * s; };
  // (one draw per statement: the order of a constructor's arguments is unspecified)
  auto grid3 = [&](int lo0, int hi0, int lo1, int hi1, int lo2, int hi2) {
    Vec3f p;
    p[0] = grid(lo0, hi0);
    p[1] = grid(lo1, hi1);
    p[2] = grid(lo2, hi2);
    return p;
  };
  std::vector<KnnMap> m;
  m.push_back({"lattice", 0, lattice(10)});
  {
    std::vector<Vec3f> v;
    for (const Vec3f& p : lattice(7))
      for (int r = 0, reps = 2 + (int)(g.next() % 2); r < reps; r++) v.push_back(p);
    shuffle(v);
    m.push_back({"duplicates", 0, v});
  }
  {
    std::vector<Vec3f> v;
    for (int i = 0; i < 600; i++) {
      Vec3f p = grid3(-12, 12, -8, 12, -12, 12);
      switch (g.next() % 5) {
        case 0: p[1] = -1.f; break;
        case 1: p[0] = -1.5f; break;
        case 2: p[0] = 1.5f; break;
        case 3: p[2] = -1.5f; break;
        default: break;
      }
      v.push_back(p);
    }
    m.push_back({"walls", 0, v});
  }
  {
    std::vector<Vec3f> v;
    for (int i = 0; i < 300; i++) v.push_back(Vec3f(0.25f, grid(-20, 19), -0.5f));
    m.push_back({"line", 0, v});
  }
  m.push_back({"point", 0, std::vector<Vec3f>(100, Vec3f(0.375f, -0.25f, 0.5f))});
  for (int n = 1; n <= 5; n++) {
    std::vector<Vec3f> v;
    for (int i = 0; i < n; i++) v.push_back(grid3(-2, 2, -2, 2, -2, 2));
    m.push_back({"tiny" + std::to_string(n), 0, v});
  }
  for (int e : {-80, -70, 62, 64}) m.push_back({"lattice_2^" + std::to_string(e), e, lattice(6)});
  return m;
}

// Queries on the map's own grid (before scaling): photon positions, cell centres, face
// centres and edge midpoints (exact equal-distance ties), points on a photon's split
// coordinate, random points, and points 10^3 x the map's extent away.
std::vector<Vec3f> knnQueries(Lcg& g, const std::vector<Vec3f>& pos) {
  const float h = 0.0625f;
  Vec3f lo = pos[0], hi = pos[0];
  for (const Vec3f& p : pos)
    for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], p[a]), hi[a] = std::max(hi[a], p[a]);
  float ext = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), std::max(hi[2] - lo[2], 0.125f));
  auto any = [&]() { return pos[g.next() % pos.size()]; };
  auto sgn = [&]() { return g.next() % 2 ? h : -h; };
  auto sgn3 = [&]() {
    Vec3f d;
    for (int a = 0; a < 3; a++) d[a] = sgn();
    return d;
  };
  auto inBox = [&]() {
    Vec3f p;
    for (int a = 0; a < 3; a++) p[a] = g.uni(lo[a] - 0.125f, hi[a] + 0.125f);
    return p;
  };
  std::vector<Vec3f> q;
  for (int i = 0; i < 8; i++) q.push_back(any());
  for (int i = 0; i < 8; i++) {
    const Vec3f p = any();
    q.push_back(p + sgn3());
  }
  for (int i = 0; i < 8; i++) {
    Vec3f p = any();
    const int a = (int)(g.next() % 3);
    p[a] += sgn();
    if (i % 2) p[(a + 1) % 3] += sgn();
    q.push_back(p);
  }
  for (int i = 0; i < 6; i++) {
    Vec3f p = inBox();
    const uint32_t a = g.next() % 3;
    p[a] = any()[a];
    q.push_back(p);
  }
  for (int i = 0; i < 6; i++) q.push_back(inBox());
  const Vec3f c = (lo + hi) * 0.5f;
  for (const Vec3f& d : {Vec3f(-1.f, -1.f, -1.f), Vec3f(1.f, 1.f, 1.f), Vec3f(-1.f, 1.f, -1.f), Vec3f(1.f, -1.f, 0.5f)})
    q.push_back(c + d * (1000.f * ext));
  return q;
}

// knn <out.json>: the maps, the reference's kdtree order of each, and kdtree::knearest
// for every query and every k in 1..min(16, n): m_visited and the results as slots of
// the tree order (found by exact position + direction).
int cmdKnn(const std::string& out) {
  Lcg g(8128);
  std::ostringstream o;
  o << "{\"maps\":[\n";
  bool firstMap = true;
  for (KnnMap& m : knnMaps(g)) {
    const size_t n = m.pos.size();
    std::vector<Vec3f> qs = knnQueries(g, m.pos);
    for (std::vector<Vec3f>* v : {&m.pos, &qs})
      for (Vec3f& p : *v)
        for (int a = 0; a < 3; a++) p[a] = std::ldexp(p[a], m.scaleExp);  // exact: a power of two
    std::vector<Particle> list;
    for (size_t i = 0; i < n; i++) list.push_back(Particle(m.pos[i], Vec3f(0.5f * i, 1.f, float(n - i)), 1.f));
    kdtree tree(list.begin(), list.end());
    std::unordered_map<uint32_t, uint32_t> slotOf;  // direction x bits -> tree slot
    std::vector<uint32_t> given, order, qv, res;
    for (const Particle& p : list) push3(given, p.position()), push3(given, p.incomeDirection());
    for (size_t i = 0; i < n; i++) {
      const Particle& p = tree.m_nodes[i].m_point;
      push3(order, p.position());
      push3(order, p.incomeDirection());
      slotOf[fbits(p.incomeDirection()[0])] = (uint32_t)i;
    }
    for (size_t qi = 0; qi < qs.size(); qi++) {
      push3(qv, qs[qi]);
      Particle t;
      t.position() = qs[qi];
      for (int k = 1; k <= (int)std::min<size_t>(16, n); k++) {
        std::vector<Particle> r;
        tree.knearest(t, k, r);
        res.push_back((uint32_t)qi);
        res.push_back((uint32_t)k);
        res.push_back((uint32_t)tree.m_visited);
        for (const Particle& p : r) {
          const uint32_t slot = slotOf.at(fbits(p.incomeDirection()[0]));
          const Particle& s = tree.m_nodes[slot].m_point;
          if (fbits(s.position()[0]) != fbits(p.position()[0]) || fbits(s.position()[1]) != fbits(p.position()[1]) ||
              fbits(s.position()[2]) != fbits(p.position()[2]))
            throw std::runtime_error("knn result not found in the tree order");
          res.push_back(slot);
        }
      }
    }
    J j;
    j.o << (firstMap ? "{" : ",\n{");
    firstMap = false;
    j.key("name");
    j.o << "\"" << m.name << "\"";
    j.i64("scale_exp", {m.scaleExp});
    j.u32("given", given);
    j.u32("tree", order);
    j.u32("queries", qv);
    j.u32("knn", res);
    o << j.o.str() << "}";
  }
  o << "\n]}\n";
  std::ofstream f(out);
  f << o.str();
  return 0;
}

// ---------------------------------------------------------------- shading sweep
// shading <meshdir> <in.bin> <out.json> <ppm_prefix>: the inputs tests/golden/make_shading_golden.py wrote from
// tests/shading_sweep.py, through the reference's own Material, LightSource and Renderer.  in.bin (little endian):
//   uint32 header[8] = 'SHAD', n_bsdf, n_eval, n_basis, n_frames, 0, 0, 0
//   float  bsdf[n_bsdf][17]   kd alpha albedo3 f03 n3 wi3 wo3
//   float  eval[n_eval][19]   light spec (position3 color3 direction3 intensity side factor ac al aq 0), point3
//   float  basis[n_basis][6]  position3 direction3
//   per frame: uint32 {w, h, mode, N, n_lights, 0}, float materials[5][8], float lights[n_lights][16] (specs)
// out.json: "bsdf" [n][3], "evaluateLight" [n][3], "basis" [n][9] = m_vertical m_horizontal m_normal, as bit patterns;
// frame i (cubes geometry, legacy serial RNG from a seed-1 engine) goes to <ppm_prefix><i>.ppm.
LightSource lightOf(const float* s) {
  LightSource l(Vec3f(s[0], s[1], s[2]), Vec3f(s[3], s[4], s[5]), Vec3f(s[6], s[7], s[8]), s[9], s[10]);
  l.m_factor = s[11], l.ac = s[12], l.al = s[13], l.aq = s[14];
  return l;
}

int cmdShading(const std::string& meshdir, const std::string& in, const std::string& out, const std::string& prefix) {
  std::ifstream f(in, std::ios::binary);
  if (!f) throw std::runtime_error("cannot open " + in);
  uint32_t hdr[8];
  f.read((char*)hdr, sizeof(hdr));
  if (!f || hdr[0] != 0x44414853u) throw std::runtime_error("not a shading sweep file: " + in);
  auto floats = [&](size_t n) {
    std::vector<float> v(n);
    f.read((char*)v.data(), (std::streamsize)(n * sizeof(float)));
    if (!f) throw std::runtime_error("short shading sweep file");
    return v;
  };
  const uint32_t nBsdf = hdr[1], nEval = hdr[2], nBasis = hdr[3], nFrames = hdr[4];
  std::vector<float> bsdf = floats((size_t)nBsdf * 17), eval = floats((size_t)nEval * 19), basis = floats((size_t)nBasis * 6);
  J j;
  j.o << "{\n";
  {
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < nBsdf; i++) {
      const float* a = &bsdf[(size_t)i * 17];
      Material M(a[0], a[1], Vec3f(a[2], a[3], a[4]), Vec3f(a[5], a[6], a[7]));
      push3(v, M.evaluateColorResponse(Vec3f(a[8], a[9], a[10]), Vec3f(a[11], a[12], a[13]), Vec3f(a[14], a[15], a[16])));
    }
    j.u32("bsdf", v);
  }
  {
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < nEval; i++) {
      const float* a = &eval[(size_t)i * 19];
      LightSource l = lightOf(a);
      push3(v, l.evaluateLight(Vec3f(a[16], a[17], a[18])));
    }
    j.u32("evaluateLight", v);
  }
  {
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < nBasis; i++) {
      const float* a = &basis[(size_t)i * 6];
      LightSource l(Vec3f(a[0], a[1], a[2]), Vec3f(1.f, 1.f, 1.f), Vec3f(a[3], a[4], a[5]), 1.f, 0.f);
      push3(v, l.m_vertical);
      push3(v, l.m_horizontal);
      push3(v, l.m_normal);
    }
    j.u32("basis", v);
  }
  j.o << "\n}\n";
  std::ofstream(out) << j.o.str();
  std::cout.setstate(std::ios::failbit);  // silence the progress bar
  for (uint32_t i = 0; i < nFrames; i++) {
    uint32_t fh[6];
    f.read((char*)fh, sizeof(fh));
    if (!f) throw std::runtime_error("short shading sweep file (frame)");
    std::vector<float> mats = floats(40), lights = floats((size_t)fh[4] * 16);
    Scene scene = buildScene(meshdir, "cubes", fh[0], fh[1]);
    for (int m = 0; m < 5; m++) {
      const float* a = &mats[(size_t)m * 8];
      scene.meshes()[m].material() = Material(a[0], a[1], Vec3f(a[2], a[3], a[4]), Vec3f(a[5], a[6], a[7]));
    }
    scene.lightsources().clear();
    for (uint32_t l = 0; l < fh[4]; l++) scene.lightsources().push_back(lightOf(&lights[(size_t)l * 16]));
    gen.seed(1);  // every frame from the engine state a fresh process has
    Image image(fh[0], fh[1]);
    RayTracer rt;
    Renderer renderer(scene, (int)fh[3], (int)fh[2], rt);
    image.fillBackground();
    renderer.render(image);
    image.savePPM(prefix + std::to_string(i) + ".ppm");
  }
  std::cout.clear();
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 6 && !strcmp(argv[1], "shading")) return cmdShading(argv[2], argv[3], argv[4], argv[5]);
  if (argc >= 4 && !strcmp(argv[1], "vectors")) return cmdVectors(argv[2], argv[3]);
  if (argc >= 3 && !strcmp(argv[1], "knn")) return cmdKnn(argv[2]);
  if (argc >= 11 && !strcmp(argv[1], "render")) return cmdRender(argc, argv, false);
  if (argc >= 10 && !strcmp(argv[1], "time")) return cmdRender(argc, argv, true);
  fprintf(stderr, "usage: see header of oracle/ref_harness.cpp\n");
  return 2;
}
