// rt_kernels.hip — gfx950 kernels of the path-tracing hot path.
//
// Execution model (wave64, CDNA4):
//   * one lane = one (pixel, sample) pair in every render kernel: a wave integrates
//     S = 1 << sshift consecutive samples of P = 64 >> sshift pixels side by side and the
//     pixel's owner lane adds them in sample order, so every pixel's float sum is formed
//     in exactly the order the reference forms it (Renderer.cpp:219-258) whatever S, the
//     number of launches or the number of GPUs the frame is split over;
//   * BVH traversal keeps a per-lane stack in LDS laid out [level][thread]
//     (ds_read/write_b32, lane-contiguous => bank-conflict free), node records are
//     32 B (12 binary16 box planes + 2 child refs: 2 x dwordx4 per lane per step),
//     triangle records 48 B (3 x dwordx4);
//   * the photon k-NN keeps its k-heap in LDS ([slot][thread]) and re-uses the
//     traversal stack region for the kd-tree's per-level split distances;
//   * the pooled integrator (BVH direct lighting) runs as ONE persistent workgroup of 16
//     waves per CU (fewer when deep stacks fill the LDS): its LDS holds every wave's private
//     stack and ray pool plus the whole BVH when it fits, else its most-visited prefix;
//     waves draw wave tiles from a global counter; after the tree copy no wave ever
//     synchronises with another (wave-scope fences only), counters leave through one atomic
//     per wave;
//   * a wave issues one instruction of ANY kind per 4 cycles, so the hot loops are written for
//     instruction COUNT: wave-uniform loops around predicated regions, lane masks made by hand
//     (ballot / inverse ballot + scalar bit operations) where the compiler would add compares,
//     and s_setprio by phase (the descent's dependent LDS round trips go first).
// Built with -ffp-contract=off (bit parity with the x86-64 oracle, no FMA).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "bvh_build.h"
#include "filters.h"
#include "rt_device.h"
#include "rt_kernels.h"

using namespace rtd;

namespace rtk {

constexpr int BLOCK = 64;
constexpr int STACK = rtbvh::kMaxDepth;  // 32 words per lane
constexpr int KMAX = RTK_KMAX;           // photon heap capacity per lane

struct Lds {
  uint32_t* stack;  // [STACK][BLOCK] this thread's column: stack[level * BLOCK]
  uint2* heap;      // [KMAX][BLOCK] {distance bits, photon index}
};

// Diagnostic build only (-DRT_PHASE_TIMING, tools/phase_timing.sh): wave-level shader-clock
// time per section of the pooled k_render, accumulated in LDS by lane 0 at wave-uniform
// points and flushed to counters[16..].  Never compiled into the product library.
#ifdef RT_PHASE_TIMING
__shared__ unsigned long long g_phAcc[24];
__shared__ unsigned long long g_phT0;
#define PH(p)                                                  \
  do {                                                         \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    if (threadIdx.x == 0) g_phAcc[p] += t_ - g_phT0, g_phT0 = t_; \
  } while (0)
#define PHC(p) do { if (threadIdx.x == 0) g_phAcc[p] += 1; } while (0)
#else
#define PH(p) do { } while (0)
#define PHC(p) do { } while (0)
#endif
enum { PH_SETUP = 0, PH_PRIMARY, PH_VSETUP, PH_FILL, PH_HANDOUT, PH_STEAL, PH_DESCENT, PH_LEAF, PH_POOLMISC, PH_BSDF,
       PH_ACCUM, PH_N_ROUNDS, PH_N_STEPS, PH_N_POOLS, PH_TAIL, PH_FOREIGN, PH_COUNT };

struct LaneStats {
  uint32_t closest = 0, shadow = 0, knn = 0, nodes = 0, tris = 0, kd = 0;
  uint32_t wnode = 0, wleaf = 0;  // wave-level node steps / leaf phases (counted by the first active lane)
  uint32_t lwait = 0, lidle = 0;  // lanes holding a leaf / no ray during those node steps
  uint32_t frames = 0;            // Q8: block frames fetched
};

struct HitRec {
  float t, u, v;
  uint32_t id, mesh;
};

RT_DEV float safe_inv(float d) {
  // finite stand-in for 1/0 so that lo * inv - o * inv never forms 0 * inf.  The
  // reciprocal only feeds the (padded, conservative) slab test, never a reference
  // expression, so the 1-ulp hardware v_rcp_f32 is enough: its error is four orders
  // below the box padding in t units.
  // (clamped, not selected: rcp(+-0) and rcp(denormal) are +-inf, med3 brings them to +-1e20 —
  // two instructions instead of compare + copysign + select)
  return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d), -1e20f, 1e20f);
}

RT_DEV f3 f4xyz(const float4& a) { return mk(a.x, a.y, a.z); }

// Conservative slab test of one padded child box.  Returns entry distance in tn.
// t = lo*inv - o*inv as ONE fma per plane (this is our own box arithmetic, not a
// reference expression, so contraction is allowed here): its absolute error is
// ~ulp(o*inv) = 6e-8*|o|*|inv|, three orders below the box padding expressed in t
// units (pad*|inv|, pad >= 6e-5*|o|max), so no padded box is ever wrongly culled.
RT_DEV float h2f_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
RT_DEV float h2f_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
// byte k of a word as a float: the compiler selects v_cvt_f32_ubyteK (extract + convert, one instruction)
RT_DEV float ub0(uint32_t w) { return (float)(w & 0xffu); }
RT_DEV float ub1(uint32_t w) { return (float)((w >> 8) & 0xffu); }
RT_DEV float ub2(uint32_t w) { return (float)((w >> 16) & 0xffu); }
RT_DEV float ub3(uint32_t w) { return (float)(w >> 24); }

RT_DEV bool slab(float lx, float ly, float lz, float hx, float hy, float hz, f3 inv, f3 oi, float tmax,
                 float& tn) {
  float ax = __builtin_fmaf(lx, inv.x, -oi.x), bx = __builtin_fmaf(hx, inv.x, -oi.x);
  float ay = __builtin_fmaf(ly, inv.y, -oi.y), by = __builtin_fmaf(hy, inv.y, -oi.y);
  float az = __builtin_fmaf(lz, inv.z, -oi.z), bz = __builtin_fmaf(hz, inv.z, -oi.z);
  float tnear = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.f));
  float tfar = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
  tn = tnear;
  return tnear <= fminf(tfar, tmax);
}

// The same test with the planes already ordered along the ray: `n*` = the plane the ray
// crosses first on that axis (lo when the direction component is >= 0, else hi), `f*` the
// other one.  t is monotone in the plane coordinate (one correctly rounded fma, inv fixed and
// finite: safe_inv), so near/far selected by the sign of inv ARE min/max of the pair — same
// tnear, tfar, same decision, six instructions fewer per child pair.
RT_DEV bool slab_ordered(float nx, float fx, float ny, float fy, float nz, float fz, f3 inv, f3 oi, float tmax, float& tn) {
  const float ax = __builtin_fmaf(nx, inv.x, -oi.x), bx = __builtin_fmaf(fx, inv.x, -oi.x);
  const float ay = __builtin_fmaf(ny, inv.y, -oi.y), by = __builtin_fmaf(fy, inv.y, -oi.y);
  const float az = __builtin_fmaf(nz, inv.z, -oi.z), bz = __builtin_fmaf(fz, inv.z, -oi.z);
  const float tnear = fmaxf(fmaxf(ax, ay), fmaxf(az, 0.f));
  const float tfar = fminf(fminf(bx, by), bz);
  tn = tnear;
  return tnear <= fminf(tfar, tmax);
}
// (lo, hi) f16 pair -> (near, far): rotate by 16 when the ray runs against the axis
RT_DEV uint32_t order_planes(uint32_t w, uint32_t rot) { return __builtin_amdgcn_alignbit(w, w, rot); }

// lane mask of a predicate (HIP's __ballot(int) goes through a 0/1 register and a compare where
// the compiler does not fold it: two vector instructions per use)
RT_DEV uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

constexpr int32_t TERM = (int32_t)0x80000000;  // "this lane holds no live ray"

// Every LDS exchange in this file is between lanes of ONE wave (a wave owns its stack,
// heap and pool regions), so no s_barrier is ever needed: a wave's DS operations are
// executed in issue order, and this keeps the compiler from moving them across the
// hand-over point.  (With one wave per workgroup __syncthreads() compiled to the same
// thing; the persistent kernel runs 16 waves per workgroup, where it would not.)
RT_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// byte offset of g_lds inside the workgroup's LDS segment (static __shared__ objects of
// the diagnostic build come first)
RT_DEV uint32_t ldsNodeBase();

// Dynamic LDS of the render kernels.  The persistent pooled kernel keeps the TOP of the
// BVH here — node records [0, topK), which bvh_build lays out most-visited first — in
// front of the per-wave regions: one copy per CU, shared by all of its waves.
extern __shared__ uint32_t g_lds[];
RT_DEV uint32_t ldsNodeBase() { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)g_lds; }

// One lane's ray in flight.  round() advances every lane of the wave that holds a
// live ray by one "while-while" round: first the wave descends inner nodes until only a
// few lanes are still descending (lanes that already hold a leaf sit out, masked; the
// stragglers sit out the leaf phase), then all held leaves are intersected together —
// each wave iteration runs one kind of work instead of the union of both (the
// single-loop form measured 34 % lane utilisation on incoherent rays).  Between rounds
// a caller may hand finished lanes new rays or parts of other lanes' rays (vertex pool
// below).
constexpr int TRAV_CLOSEST = 0, TRAV_ANY = 1, TRAV_MIXED = 2;  // MIXED: per-lane `anyHit` flag

// LT: where node records live.  LT_NONE: HBM/L2 through the vector L1; LT_TOP: records
// [0, S.topK) in LDS (g_lds), the rest in HBM/L2; LT_ALL: the whole tree in LDS.
constexpr int LT_NONE = 0, LT_TOP = 1, LT_ALL = 2;
// + LT_Q8: the ONE-REQUEST node (rtbvh::Slot16, bvh_build.h): a 16-byte record — 12 8-bit box planes in the frame of the
// record's 16-KiB block + one word that locates both children — in ONE array with the triangle records.  A visit is one
// dwordx4 instead of two; a lane that enters a record of another block fetches that block's frame {origin, step} with it
// (one more request, in flight together with the record) and rebuilds its two slab constants: t = q * (step / d) +
// (origin - o) / d, so the 8-bit plane goes into the same fma the binary16 plane went into (v_cvt_f32_ubyteN extracts
// and converts in one instruction, v_perm_b32 orders a word's two (lo, hi) pairs along the ray).
constexpr int LT_Q8 = 4;
// Wave priority by phase (s_setprio): a wave in the DESCENT (a chain of dependent LDS round trips
// and short instruction runs) or in the pool bookkeeping issues ahead of waves that stream through
// shading arithmetic or triangle tests, instead of queueing behind them by age.  Measured: C2
// +5.1 %, C4 +2.2 % (descent 2, pool 1, leaf and shading 0; 1..3 in the descent are alike, a raised
// LEAF phase costs 2 %); on the 1 M-triangle scene, where the waves wait on memory rather than on
// each other, it costs 1 % — LT_NOPRIO (trees beyond kPrioMaxNodes) leaves everything at 0.
constexpr int LT_NOPRIO = 8;
// Compact ray pool (scenes whose stacks fill the LDS): per light the pool keeps the two
// parameters of the light sample instead of the direction to it — 2 words instead of 3 per lane and
// light, 768 B per wave with three lights — and the direction is rebuilt where it is needed by the
// arithmetic light_sample() performs (LightSource.h:46-49, the same operations in the same order:
// the same bits).  On the 1 M-triangle scene that is the sixteenth wave.
constexpr int LT_COMPACT = 16;
// ... and without the bounce directions either (another 768 B per wave; implies LT_COMPACT): every
// bounce ray is handed to its OWN pixel lane in the first hand-out and starts from the register that
// holds the direction anyway; a lane that steals part of a bounce ray takes the direction from the
// victim's registers.  The eight-million-triangle scene's sixteenth wave.
constexpr int LT_COMPACT2 = 32;
// ... and without the light samples' parameters or the vertex positions either (implies LT_COMPACT2): the pixel lane keeps its
// vertex and its RNG state from before its light draws in registers, a worker lane fetches both by lane shuffle and re-draws
// the light sample from the state — the same engine calls, the same bits.  168 words instead of 744 (the bounce keys, the
// hand-out list, the result bits): with 28 stack rows that is 7,840 B per wave — five workgroups of four waves fit a CU's LDS,
// which is handed out in 1,280-byte units —, TWENTY waves per CU for trees of up to 27 levels, and the instance is compiled
// for five waves per SIMD (96 VGPRs).
constexpr int LT_COMPACT3 = 64;
// The resident tree's leaves hold at most two records (rt_options.bvh_leaf_max <= 2, the default): the leaf phase is
// test_pair alone — no loop over records 3 .. leaf_max, none of its masks.  The launcher picks these instances per launch
// from RenderArgs::flags bit 1 (the timed single-view LT_ALL, LT_TOP and four-wave instances; RT_LEAF2=0 forces the
// general ones).
constexpr int LT_LEAF2 = 128;
// 1 / det of the triangle test by rtd::recip_fast (3 instructions, the division's bits for |det| < 2^100) instead of the
// division: only the instances the launcher picks when the host has bounded |det| for the launch's rays (DevScene::slowRecip == 0).
constexpr int LT_FASTDET = 256;
// A multi-view frame (rt_render_views): RenderArgs::tileView / views give every wave tile its view's camera, stream key
// and accumulator slice.  Only render_tile reads it (it strips the bit before it passes LT on).  Its own instances: read
// at run time, the choice costs every single-view instance SGPR spills and one of them a wave.
constexpr int LT_VIEWS = 512;
// The frame's variants (frame_variants.h).  Only render_tile reads these bits, and it takes the one record that goes with
// them (frame_rec_t); the record-carrying instances are k_render_rec's.
// A frame through a thin lens (rt_render_lens): render_tile takes a LensRec and, where its aperture is not zero, forms the
// primary ray by lens_ray instead of camera_ray.
constexpr int LT_LENS = 1024;
// A frame under an open shutter (rt_render_shutter): render_tile takes a ShutterRec and forms every sample's camera, then
// its primary ray, by shutter_ray.  With LT_VIEWS (rt_render_views_shutter): the record is the view's, from
// RenderArgs::viewShutters, and shutter_ray runs on the view's camera and seed; no record argument, so these are k_render
// instances.
constexpr int LT_SHUTTER = 2048;
// A frame split by light group (rt_render_lights): render_tile takes a LightGroupsRec, keeps one colour per group and
// vertex and adds every sample into one accumulator slice per group; the vertex pool and shade_direct_seq form the
// per-group sums (their GROUPS switch).
constexpr int LT_LIGHTS = 4096;
// A frame with sampled direct lighting (rt_render_pick): render_tile takes a PickRec and draws every sample's m light
// indices from a stream of its own before the primary cast; the vertex pool and shade_direct_seq then run over those m
// slots of the record's scaled lights instead of the scene's list (their PICK switch).
constexpr int LT_PICK = 8192;
// A frame with per-vertex albedo (rt_render_colors): render_tile takes a VColRec and forms every vertex's kdDiffuse from
// the colours of the hit triangle's three vertices; the vertex pool and shade_direct_seq shade with it in place of the
// mesh's (their VC switch: ParkKd, the value the surface policy SurfVCol parks).
constexpr int LT_VCOL = 16384;
// A frame with image-textured albedo (rt_render_textured): render_tile takes a TexRec and forms every vertex's kdDiffuse
// from the texture sample at the hit's uv (tex_kd); it reaches the vertex pool and shade_direct_seq as the coloured
// frame's does (SurfTex: the same three parked rows).
constexpr int LT_TEX = 32768;
// A frame with textured material maps (rt_render_material): render_tile takes a MatRec and forms every vertex's whole
// material from the samples at the hit's uv (tex_mat); it reaches the vertex pool and shade_direct_seq through their VC
// switch as SurfMat's ParkMat, which shades with bsdf_base(const rt_material&) in place of the mesh's DevMat.
constexpr int LT_MAT = 65536;
// A frame with tangent-space normal maps (rt_render_normal_mapped): render_tile takes a NrmRec, forms every vertex's
// material as the material-map frame does (SurfNrm parks SurfMat's ParkMat) and, before anything reads the shading
// normal, replaces it by the perturbed one (nmap_bend): the light terms, the BSDF and the bounce then use that.
constexpr int LT_NMAP = 131072;
constexpr int LT_SURFACES = LT_VCOL | LT_TEX | LT_MAT | LT_NMAP;  // (the bits surface_t reads)
// The descent loop of Trav::round as the compiler writes it, in an instance that would otherwise take the hand-written
// loop (Trav::DESCENT): the launcher's RT_DESCENT=0 twin of the timed LT_ALL | LT_FASTDET | LT_LEAF2 instance.
constexpr int LT_CLOOP = 262144;
constexpr uint32_t kPrioMaxNodes = 65536;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) u32x4* lds_u4_ptr;

// POOL: the walker of a vertex pool (its rounds end at the pool loop's wave priority); the mixed walker always is, the
// any-hit one when the pool holds shadow rays only.
template <int MODE, int LTX = LT_NONE, bool POOL = (MODE == TRAV_MIXED)>
struct Trav {
  static constexpr int LT = LTX & 3;
  static constexpr bool PRIO = (LTX & LT_NOPRIO) == 0;
  static constexpr bool DIVIDE = (LTX & LT_FASTDET) == 0;
  static constexpr bool Q8 = (LTX & LT_Q8) != 0;
  static constexpr bool LEAF2 = (LTX & LT_LEAF2) != 0;
  static constexpr bool KEYED = LEAF2;  // test_pair accepts by one compare of hit_key (see there)
  // round()'s descent loop as one assembly block that only ever NARROWS exec (descent_asm): the timed whole-tree-in-LDS
  // two-record-leaf instance, in the three walkers it was written for and read back in (closest-hit, mixed, any-hit of a
  // shadow-only pool); LT_CLOOP keeps the compiler's loop.  So does the diagnostic build (RT_PHASE_TIMING): the block takes
  // a node's offset for its LDS address, which holds only without static LDS in front of g_lds (the step in round()),
  // and it does not count PH_N_STEPS.
#ifdef RT_PHASE_TIMING
  static constexpr bool DESCENT = false;
#else
  static constexpr bool DESCENT = LT == LT_ALL && LEAF2 && !DIVIDE && !Q8 && (LTX & LT_CLOOP) == 0 && (MODE != TRAV_ANY || POOL);
#endif
  static_assert(!Q8 || LT == LT_NONE, "Q8 records are fetched from HBM / L2");
  // any-hit rays enter child 0 (the smaller box) first: the big-scene instances and the whole-tree-in-LDS ones (measured:
  // C5 -2.5 %, C5x8 -1.9 %, C2 -0.7 %, C1 -3 %; the partial-top instance of C4 loses 0.7 % to the extra scalar op and keeps
  // the distance order)
  static constexpr bool ANYORD = (LTX & LT_NOPRIO) != 0 || LT == LT_ALL;
  f3 o, d, inv, oi;
  uint32_t rotX, rotY, rotZ;  // 16 where the direction component is negative (order_planes); Q8: the v_perm_b32 selectors of the three plane words
  // Q8: 1 / d (inv and oi then hold the slab constants IN THE HELD FRAME: step / d and (o - origin) / d) and the block
  // whose frame that is
  f3 inv0;
  uint32_t fblk;
  float best;
  uint32_t bestId;
  bool found, anyHit;
  // LDS stack of this lane: row 0 holds a TERM sentinel, entries live in rows 1..depth;
  // `top` points at the top entry (or at the sentinel: an empty stack pops TERM by itself,
  // so no step ever tests for emptiness or clamps an index)
  uint32_t* top;
  uint32_t* base;
  int32_t cur;
  HitRec hit;
  // pool mode (TRAV_MIXED): several lanes may walk disjoint subtrees of ONE ray
  // (vertex_pool: work stealing).  `stolen` = bottom stack entries handed to other
  // lanes; closest-hit candidates are published to shared[0..1] = 64-bit key
  // (t bits << 32 | triangle id: unsigned min == closest t, lowest id on ties —
  // RayTracer.h:40's rule); the pixel lane recomputes u, v of the winner.
  int stolen;
  bool shared;  // this ray is (or was) walked by more than one lane
  unsigned long long* sharedKey;
  uint32_t pj;

  // entries on the stack (live lanes only: top >= base there, so the byte distance is unsigned —
  // a signed 64-bit pointer difference and division cost seven instructions)
  RT_DEV int depth() const {
    return (int)(((uint32_t)(uintptr_t)top - (uint32_t)(uintptr_t)base) / (4u * BLOCK));
  }
  RT_DEV void idle(uint32_t* stack) { cur = TERM, found = false, base = top = stack, stolen = 0, shared = false; }
  RT_DEV uint32_t peek() const { return *top; }
  RT_DEV void pop() { top -= BLOCK; }
  RT_DEV void start(f3 o_, f3 d_, float invScale) {
    o = o_, d = d_;
    const f3 i1 = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    if (Q8) {
      inv0 = i1, fblk = ~0u;  // (no frame held: the first step fetches the root block's)
      inv = oi = mk(0.f, 0.f, 0.f);
      // a plane word holds two (lo, hi) byte pairs — (x, y) of child 0, (z of child 0, x of child 1), (y, z) of child 1 —
      // and v_perm_b32 swaps the bytes of a pair whose axis the ray runs against
      const uint32_t nx = __float_as_uint(i1.x) >> 31, ny = __float_as_uint(i1.y) >> 31, nz = __float_as_uint(i1.z) >> 31;
      rotX = 0x03020100u ^ (nx * 0x00000101u) ^ (ny * 0x01010000u);
      rotY = 0x03020100u ^ (nz * 0x00000101u) ^ (nx * 0x01010000u);
      rotZ = 0x03020100u ^ (ny * 0x00000101u) ^ (nz * 0x01010000u);
    } else {
      oi = mk(o.x * i1.x, o.y * i1.y, o.z * i1.z);
      // boxes are stored as coordinate * boxScale (a power of two): fold 1/boxScale in
      inv = mk(i1.x * invScale, i1.y * invScale, i1.z * invScale);
      rotX = (__float_as_uint(i1.x) >> 31) << 4, rotY = (__float_as_uint(i1.y) >> 31) << 4, rotZ = (__float_as_uint(i1.z) >> 31) << 4;
    }
    best = 3.402823466e+38f;  // numeric_limits<float>::max(), RayTracer.h:30
    bestId = 0, found = false, top = base, cur = Q8 ? (int32_t)rtbvh::kQ8RootOffset : 0, stolen = 0, shared = false;
    *base = (uint32_t)TERM;
    // A ray with a NaN component cannot hit anything: Ray.cpp:9-24 then yields NaN u
    // or v for every triangle and every comparison fails (hemisphere samples are NaN
    // with p ~ 3e-8).  The slab test, built from min/max that drop
    // NaNs, would instead accept every box: ONE such ray walks all 500k nodes of the
    // 1M-triangle scene (measured: +0.6 s on a 50 ms frame).  Same result, no walk:
    // (three two-operand unordered tests)
    if (__builtin_isunordered(o.x, o.y) | __builtin_isunordered(o.z, d.x) | __builtin_isunordered(d.y, d.z)) cur = TERM;
  }
  RT_DEV bool live() const { return cur != TERM; }

  // The descent loop of round() for the DESCENT instances, exit rule and step as in the loop there (its comments apply):
  // the same vector and LDS instructions per step, taken from the compiler's own body, under five control instructions
  // instead of eight.  The lanes of successive steps are nested — a lane that stops descending never resumes inside the
  // loop — so exec is only narrowed (s_mov exec, vcc: a compare under exec writes 0 for the lanes that are off, which is
  // what they are) and restored once, after the loop; the compiler re-enters and leaves the step's region every step
  // (s_or exec / s_and_saveexec / a never-taken execz branch / a branch back to the latch).
  // Every adjacent pair of the control sequence occurs in the compiler's output for these kernels (a compare into vcc and
  // s_bcnt1 of vcc; a scalar write of exec and a DS or vector instruction), no vector instruction reads a mask that a vector
  // instruction wrote (they pass through a scalar operation, as in the compiler's step), and the scalar unit writes
  // registers only.  The waits count LDS operations, which return in order: the block opens with lgkmcnt(0) because
  // scalar loads share the counter and do not.  It leaves with the last step's stack write in flight, as the compiler's
  // loop does.  The two 16-byte halves of the node need register tuples whose elements the text can name: v[16:19] and
  // v[2:5], with the scalar temporaries beside them (the registers the compiler's mixed walker uses for them).
#define RT_DESCENT_HEAD                                                         \
  "s_waitcnt lgkmcnt(0)\n\t"                                                    \
  "v_cmp_lt_i32_e32 vcc, -1, %[cur]\n\t"                                        \
  "s_and_saveexec_b64 %[save], vcc\n\t"                                         \
  "s_cbranch_execz 2f\n"                                                        \
  "1:\n\t"                                                                      \
  "ds_read_b128 v[16:19], %[cur]\n\t"                                           \
  "ds_read_b128 v[2:5], %[cur] offset:16\n\t"                                   \
  "ds_read_b32 v6, %[top]\n\t"                                                  \
  "s_waitcnt lgkmcnt(2)\n\t"                                                    \
  "v_alignbit_b32 v7, v16, v16, %[rx]\n\t"                                      \
  "v_alignbit_b32 v16, v17, v17, %[ry]\n\t"                                     \
  "v_alignbit_b32 v17, v18, v18, %[rz]\n\t"                                     \
  "v_fma_mix_f32 v21, v17, %[iz], -%[oz] op_sel_hi:[1,0,0]\n\t"                 \
  "v_alignbit_b32 v18, v19, v19, %[rx]\n\t"                                     \
  "s_waitcnt lgkmcnt(1)\n\t"                                                    \
  "v_alignbit_b32 v3, v3, v3, %[rz]\n\t"                                        \
  "v_fma_mix_f32 v19, v7, %[ix], -%[ox] op_sel_hi:[1,0,0]\n\t"                  \
  "v_fma_mix_f32 v7, v7, %[ix], -%[ox] op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"    \
  "v_fma_mix_f32 v20, v16, %[iy], -%[oy] op_sel_hi:[1,0,0]\n\t"                 \
  "v_fma_mix_f32 v16, v16, %[iy], -%[oy] op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"  \
  "v_max_f32_e32 v21, 0, v21\n\t"                                               \
  "v_alignbit_b32 v2, v2, v2, %[ry]\n\t"                                        \
  "v_fma_mix_f32 v17, v17, %[iz], -%[oz] op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"  \
  "v_max3_f32 v19, v19, v20, v21\n\t"                                           \
  "v_min_f32_e32 v7, v7, v16\n\t"                                               \
  "v_fma_mix_f32 v20, v3, %[iz], -%[oz] op_sel_hi:[1,0,0]\n\t"                  \
  "v_min3_f32 v7, v7, v17, %[best]\n\t"                                         \
  "v_fma_mix_f32 v16, v18, %[ix], -%[ox] op_sel_hi:[1,0,0]\n\t"                 \
  "v_fma_mix_f32 v17, v18, %[ix], -%[ox] op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"  \
  "v_fma_mix_f32 v18, v2, %[iy], -%[oy] op_sel_hi:[1,0,0]\n\t"                  \
  "v_max_f32_e32 v20, 0, v20\n\t"                                               \
  "v_fma_mix_f32 v2, v2, %[iy], -%[oy] op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"    \
  "v_max3_f32 v16, v16, v18, v20\n\t"                                           \
  "v_fma_mix_f32 v3, v3, %[iz], -%[oz] op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"    \
  "v_min_f32_e32 v2, v17, v2\n\t"
  // (v19 / v7: child 0's entry and exit distance, v16 / v2: child 1's.  vcc = m0, %[m1] = m1, %[ty] = takeY)
#define RT_DESCENT_TAIL                                                         \
  "v_cndmask_b32_e64 v20, v5, v4, %[ty]\n\t"                                    \
  "ds_write_b32 %[top], v20 offset:%[row]\n\t"                                  \
  "v_cndmask_b32_e64 v20, v4, v5, %[ty]\n\t"                                    \
  "s_or_b64 %[ty], %[m1], vcc\n\t"                                              \
  "s_waitcnt lgkmcnt(1)\n\t"                                                    \
  "v_cndmask_b32_e64 %[cur], v6, v20, %[ty]\n\t"                                \
  "v_cndmask_b32_e64 v20, %[pop], 0, %[ty]\n\t"                                 \
  "s_and_b64 %[m1], %[m1], vcc\n\t"                                             \
  "v_cndmask_b32_e64 v20, v20, %[blk], %[m1]\n\t"                               \
  "v_lshl_add_u32 %[top], v20, 2, %[top]\n\t"                                   \
  "v_cmp_lt_i32_e32 vcc, -1, %[cur]\n\t"                                        \
  "s_bcnt1_i32_b64 %[n], vcc\n\t"                                               \
  "s_cmp_le_u32 %[exitBelow], %[n]\n\t"                                         \
  "s_mov_b64 exec, vcc\n\t"                                                     \
  "s_cbranch_scc1 1b\n"                                                         \
  "2:\n\t"                                                                      \
  "s_or_b64 exec, exec, %[save]"
#define RT_DESCENT_OUT [cur] "+v"(cur), [top] "+v"(t), [save] "=&s"(save), [ty] "=&s"(ty), [m1] "=&s"(m1), [n] "=&s"(n)
#define RT_DESCENT_IN                                                                                                  \
  [ix] "v"(inv.x), [iy] "v"(inv.y), [iz] "v"(inv.z), [ox] "v"(oi.x), [oy] "v"(oi.y), [oz] "v"(oi.z), [rx] "v"(rotX),   \
      [ry] "v"(rotY), [rz] "v"(rotZ), [best] "v"(best), [pop] "v"(-BLOCK), [exitBelow] "s"(exitBelow), [blk] "i"(BLOCK), \
      [row] "i"(4 * BLOCK)
#define RT_DESCENT_CLOBBER "v2", "v3", "v4", "v5", "v6", "v7", "v16", "v17", "v18", "v19", "v20", "v21", "vcc", "scc", "memory"
  RT_DEV void descent_asm(int exitBelow, uint64_t anyFirst) {
    typedef __attribute__((address_space(3))) uint32_t* lds_u32_ptr;
    lds_u32_ptr t = (lds_u32_ptr)top;
    uint64_t save, ty, m1;
    uint32_t n;
    if constexpr (MODE == TRAV_MIXED) {
      // takeY = m1 & ~(m0 & (t0 <= t1 | anyFirst))
      asm volatile(RT_DESCENT_HEAD
                   "v_cmp_le_f32_e64 %[ty], v19, v16\n\t"
                   "v_min3_f32 v2, v2, v3, %[best]\n\t"
                   "v_cmp_le_f32_e32 vcc, v19, v7\n\t"
                   "s_or_b64 %[ty], %[ty], %[anyFirst]\n\t"
                   "v_cmp_le_f32_e64 %[m1], v16, v2\n\t"
                   "s_and_b64 %[ty], %[ty], vcc\n\t"
                   "s_andn2_b64 %[ty], %[m1], %[ty]\n\t" RT_DESCENT_TAIL
                   : RT_DESCENT_OUT
                   : RT_DESCENT_IN, [anyFirst] "s"(anyFirst)
                   : RT_DESCENT_CLOBBER);
    } else if constexpr (MODE == TRAV_ANY) {
      // (ANYORD: every ray enters child 0 whenever it is hit) takeY = m1 & ~m0
      static_assert(ANYORD, "the any-hit block is the ANYORD step");
      asm volatile(RT_DESCENT_HEAD
                   "v_min3_f32 v2, v2, v3, %[best]\n\t"
                   "v_cmp_le_f32_e32 vcc, v19, v7\n\t"
                   "v_cmp_le_f32_e64 %[m1], v16, v2\n\t"
                   "s_andn2_b64 %[ty], %[m1], vcc\n\t" RT_DESCENT_TAIL
                   : RT_DESCENT_OUT
                   : RT_DESCENT_IN
                   : RT_DESCENT_CLOBBER);
    } else {
      // takeY = m1 & ~(m0 & t0 <= t1)
      asm volatile(RT_DESCENT_HEAD
                   "v_cmp_le_f32_e64 %[ty], v19, v16\n\t"
                   "v_min3_f32 v2, v2, v3, %[best]\n\t"
                   "v_cmp_le_f32_e32 vcc, v19, v7\n\t"
                   "v_cmp_le_f32_e64 %[m1], v16, v2\n\t"
                   "s_and_b64 %[ty], %[ty], vcc\n\t"
                   "s_andn2_b64 %[ty], %[m1], %[ty]\n\t" RT_DESCENT_TAIL
                   : RT_DESCENT_OUT
                   : RT_DESCENT_IN
                   : RT_DESCENT_CLOBBER);
    }
    top = (uint32_t*)t;
  }
#undef RT_DESCENT_HEAD
#undef RT_DESCENT_TAIL
#undef RT_DESCENT_OUT
#undef RT_DESCENT_IN
#undef RT_DESCENT_CLOBBER

  template <bool STATS>
  RT_DEV void round(const DevScene& S, LaneStats& st) {
    const int live0 = __popcll(wave_ballot(cur != TERM));
    // (at least 1: the loop below leaves when FEWER lanes than this descend, so 0 would never leave)
    const int exitBelow = max(1, min((int)S.leafT, (live0 * (int)S.leafMul) >> 6));
    uint32_t statWait = 0, statIdle = 0;
    if (STATS) statWait = (uint32_t)__popcll(wave_ballot(cur < 0 && cur != TERM)), statIdle = (uint32_t)__popcll(wave_ballot(cur == TERM));
    PHC(PH_N_ROUNDS);
    // The loop is WAVE-UNIFORM (a ballot decides, every lane leaves together) and the step a
    // plain predicated region inside it: with the lane condition as the loop condition the
    // compiler keeps per-lane exit masks (20 scalar instructions + 4 branches per step, and a
    // wave issues one instruction of ANY kind per 4 cycles).
    // (the lanes of a step are the ballot the loop control has just counted: the mask goes
    // straight back into exec — no second compare, no vector-to-scalar hand-over at the loop top)
    uint64_t inner = __builtin_amdgcn_ballot_w64(cur >= 0);
    // Any-hit rays (Renderer.cpp:54 only uses the bool) do not need the nearer child first: where ANYORD is set they
    // enter child 0 whenever it is hit — the builders put the SMALLER box there, the likelier place to find an occluder
    // close to the ray.  Same booleans, fewer visits: 1 M triangles 34.96 -> 33.54 nodes and 4.04 -> 3.50 triangle tests
    // per ray, 357 -> 348 ms; 8 M triangles 58.7 -> 57.6 ms; C2 3.17 -> 2.99 triangle tests per ray, 50.9 -> 50.6 ms.
    // (Denser-subtree-first, larger-box-first and the RTSAH rule lose: profiles/r03_anyhit_order_ab.txt.)
    const uint64_t anyFirst = !ANYORD ? 0ull : MODE == TRAV_ANY ? ~0ull : MODE == TRAV_MIXED ? __builtin_amdgcn_ballot_w64(anyHit) : 0ull;
    if (PRIO) __builtin_amdgcn_s_setprio(2);
    if constexpr (DESCENT && !STATS) descent_asm(exitBelow, anyFirst);
    else if (inner) for (;;) {
     if (__builtin_amdgcn_inverse_ballot_w64(inner)) {
      {
      float t0, t1;
      bool h0, h1;
      int2 ch;
      int32_t below;
      if (STATS) {
        st.nodes++;
        if (__ffsll((long long)wave_ballot(true)) - 1 == (int)(threadIdx.x & 63)) st.wnode++, st.lwait += statWait, st.lidle += statIdle;
      }
      if constexpr (Q8) {
        // ONE request: the 16-byte record; plus its block's frame when the lane last decoded a record of another block
        const char* const q8 = reinterpret_cast<const char*>(S.q8);
        const uint4 r = *reinterpret_cast<const uint4*>(q8 + (uint32_t)cur);
        const uint32_t blk = (uint32_t)cur >> S.q8ShiftBytes;
        if (blk != fblk) {
          const float4 fr = *reinterpret_cast<const float4*>(q8 + (blk << S.q8ShiftBytes));
          inv = mk(inv0.x * fr.w, inv0.y * fr.w, inv0.z * fr.w);
          oi = mk((o.x - fr.x) * inv0.x, (o.y - fr.y) * inv0.y, (o.z - fr.z) * inv0.z);
          fblk = blk;
          if (STATS) st.frames++;
        }
        PHC(PH_N_STEPS);
        below = (int32_t)peek();
        // both children's items are adjacent, child 0's first: one word locates them (bvh_build.h Slot16)
        const uint32_t ref = r.w, base0 = ref & ~15u;
        const uint32_t base1 = base0 + ((ref & 1u) ? ((ref & 4u) ? 96u : 48u) : 16u);
        ch.x = (ref & 1u) ? (int32_t)~(base0 | ((ref >> 2) & 1u)) : (int32_t)base0;
        ch.y = (ref & 2u) ? (int32_t)~(base1 | ((ref >> 3) & 1u)) : (int32_t)base1;
        const uint32_t w0 = __builtin_amdgcn_perm(r.x, r.x, rotX), w1 = __builtin_amdgcn_perm(r.y, r.y, rotY), w2 = __builtin_amdgcn_perm(r.z, r.z, rotZ);
        h0 = slab_ordered(ub0(w0), ub1(w0), ub2(w0),
                          ub3(w0), ub0(w1), ub1(w1), inv, oi, best, t0);
        h1 = slab_ordered(ub2(w1), ub3(w1), ub0(w2),
                          ub1(w2), ub2(w2), ub3(w2), inv, oi, best, t1);
      } else {
      // 32-B packed node: 12 x f16 planes + 2 refs (32-bit byte offset from a uniform base:
      // the load takes the base from SGPRs)
      uint4 a, b;
      // (`cur` of an inner node is the byte offset of its record)
      if (LT == LT_ALL || (LT == LT_TOP && (uint32_t)cur < S.topK * 32u)) {
        // from LDS (the tree copy starts at LDS byte offset 0 of the dynamic segment): a
        // divergent 32-B read costs the LDS a few cycles per wave where the vector L1 spends
        // one tag lookup per lane and dwordx4
        uint32_t off = (uint32_t)cur;
        if (LT == LT_TOP) asm volatile("" : "+v"(off));  // keep the two address spaces on separate paths (else: one flat load)
#ifdef RT_PHASE_TIMING
        lds_u4_ptr n = (lds_u4_ptr)(uintptr_t)(off + ldsNodeBase());
#else
        // (no static LDS in the product build: the dynamic segment, i.e. the tree copy, starts at LDS
        // address 0 — checked once on the host, launch_render2 — so a node's offset IS its address)
        lds_u4_ptr n = (lds_u4_ptr)(uintptr_t)off;
#endif
        const u32x4 va = n[0], vb = n[1];
        a = make_uint4(va.x, va.y, va.z, va.w), b = make_uint4(vb.x, vb.y, vb.z, vb.w);
      } else {
        const uint4* n = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(S.nodes) + (uint32_t)cur);
        a = n[0], b = n[1];
      }
      PHC(PH_N_STEPS);
      // the entry a miss would pop, fetched with the node (its latency hides behind the
      // node's; a read in the divergent pop branch made every step wait for LDS)
      below = (int32_t)peek();
      ch = make_int2((int)b.z, (int)b.w);
      const uint32_t x0 = order_planes(a.x, rotX), y0 = order_planes(a.y, rotY), z0 = order_planes(a.z, rotZ);
      const uint32_t x1 = order_planes(a.w, rotX), y1 = order_planes(b.x, rotY), z1 = order_planes(b.y, rotZ);
      h0 = slab_ordered(h2f_lo(x0), h2f_hi(x0), h2f_lo(y0), h2f_hi(y0), h2f_lo(z0), h2f_hi(z0), inv, oi, best, t0);
      h1 = slab_ordered(h2f_lo(x1), h2f_hi(x1), h2f_lo(y1), h2f_hi(y1), h2f_lo(z1), h2f_hi(z1), inv, oi, best, t1);
      }
      // select-based step: one divergent branch (the pop) instead of a four-way chain;
      // the far child is stored unconditionally (the slot is simply not claimed unless
      // both children were hit)
      // which child to enter: child 1 unless child 0 is hit and not farther.  Lane masks by hand
      // (ballots and scalar bit operations: three compares, and / and-not / or / and) — left to
      // the compiler the negation becomes a fourth compare.
      const uint64_t m0 = __builtin_amdgcn_ballot_w64(h0), m1 = __builtin_amdgcn_ballot_w64(h1);
      const uint64_t mle = ANYORD ? (__builtin_amdgcn_ballot_w64(t0 <= t1) | anyFirst) : __builtin_amdgcn_ballot_w64(t0 <= t1);
      const bool takeY = __builtin_amdgcn_inverse_ballot_w64(m1 & ~(m0 & mle));
      const bool both = __builtin_amdgcn_inverse_ballot_w64(m0 & m1), any = __builtin_amdgcn_inverse_ballot_w64(m0 | m1);
      top[BLOCK] = (uint32_t)(takeY ? ch.x : ch.y);
      cur = any ? (takeY ? ch.y : ch.x) : below;
      top += both ? BLOCK : any ? 0 : -BLOCK;  // (a lane that pops the sentinel is dead until start())
      // leave the descent early once only a few lanes are still descending: they
      // sit out one leaf phase (masked) instead of making everyone else wait for them
      // (only when the lanes that would otherwise wait clearly outnumber them: in the
      // tail of a pool, with a handful of live rays, a round must not shrink to one step)
      // (desc < leafT and desc < live0 * leafMul / 64, folded into one threshold)
      }
     }
      inner = __builtin_amdgcn_ballot_w64(cur >= 0);
      if (__popcll(inner) < exitBelow) break;
    }
    if (PRIO) __builtin_amdgcn_s_setprio(0);
    PH(PH_DESCENT);
    if (cur < 0 && cur != TERM) {
      const uint32_t code = ~(uint32_t)cur;
      // (byte offset of the leaf's first record | count - 1: the loads take the base from SGPRs)
      const uint32_t cnt = (code & 7u) + 1u;
      const char* const leaf = reinterpret_cast<const char*>(Q8 ? reinterpret_cast<const float4*>(S.q8) : S.tris) + (code & ~7u);
      if (STATS) st.wleaf += (uint32_t)(__ffsll((long long)wave_ballot(true)) - 1 == (int)(threadIdx.x & 63));
      // leaves hold 1..leaf_max (default 2) records: the first two are tested in
      // straight-line code with both records' loads in flight together
      const float4* r = reinterpret_cast<const float4*>(leaf);
      const uint32_t second = cnt > 1 ? 3u : 0u;  // a 1-triangle leaf re-reads its only record
      const float4 a0 = r[0], a1 = r[1], a2 = r[2];
      const float4 b0 = r[second + 0], b1 = r[second + 1], b2 = r[second + 2];
      bool stop = test_pair<STATS>(a0, a1, a2, b0, b1, b2, cnt > 1, st);
      // (LEAF2: no leaf of the tree holds a third record — no loop, none of its guard and mask bookkeeping)
      if constexpr (!LEAF2) {
        for (uint32_t i = 2; i < cnt && !stop; i++) {
          const float4* q = reinterpret_cast<const float4*>(leaf + 48u * i);
          stop = test_record<STATS>(q[0], q[1], q[2], st);
        }
      }
      cur = stop ? TERM : (int32_t)peek();
      pop();
    }
    if (PRIO && POOL) __builtin_amdgcn_s_setprio(1);  // back in the pool loop
    PH(PH_LEAF);
  }

  // The first two records of a leaf at once and without a branch: both tests run, every
  // acceptance is a select (RayTracer.h:40's rule applied to A, then to B), so the leaf
  // phase stays one basic block instead of a dozen exec-mask regions.  `two` = the leaf
  // holds a second record (else B is a re-read of A and is ignored).
  // That sentence is the intent; what the compiler makes of `ta < best || (ta == best && ida < bestId)` is an exec-mask
  // region per short-circuit operand, each around one or two vector instructions (about 100 lines of assembly for A and B).
  // KEYED instances therefore state the SAME rule as one unsigned compare of hit_key — the order publish and refresh_best
  // keep — with the booleans combined bitwise, and take tri_test's predicate as masks too (C2 -1.1 %: DESIGN.md §4.3,
  // profiles/leaf_accept/).  Why the keys order as the rule does: ha / hb contain t > 0, so an accepted t is a positive
  // float and no NaN; best is FLT_MAX, an accepted t or a published key's t (and, were a general instance keyed,
  // ao_occluded's finite maxDistance > 0) — never negative, never -0, never NaN.  Positive floats order as their bit
  // patterns do and equal ones have equal bits, so kA < k0 is the rule for every candidate that ha lets through; the key
  // of a rejected one may hold anything (NaN, negative t), and its mask discards it (tests/test_leaf_accept_rule.py).
  // KEYED is the LT_LEAF2 instances, which it was measured in; the others keep the text and the registers they had (keyed,
  // k_ao<false, true> would lose a wave per SIMD and some counted instances spill more).
  template <bool STATS>
  RT_DEV bool test_pair(const float4& p0, const float4& p1, const float4& p2, const float4& q0, const float4& q1,
                        const float4& q2, bool two, LaneStats& st) {
    if (STATS) st.tris += two ? 2u : 1u;
    float ua, va, ta, ub, vb, tb;
    const bool ha = tri_test(o, d, mk(p0.x, p0.y, p0.z), mk(p0.w, p1.x, p1.y), mk(p1.z, p1.w, p2.x), ua, va, ta, DIVIDE, KEYED) && ta > 0.f;
    const bool hb = tri_test(o, d, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), ub, vb, tb, DIVIDE, KEYED) && tb > 0.f && two;
    const bool isAny = MODE == TRAV_ANY || (MODE == TRAV_MIXED && anyHit);
    const uint32_t ida = __float_as_uint(p2.y), idb = __float_as_uint(q2.y);
    bool ba, bb;
    if constexpr (KEYED) {
      const unsigned long long k0 = hit_key(best, bestId), kA = hit_key(ta, ida), kB = hit_key(tb, idb);
      ba = (bool)((int)!isAny & (int)ha & (int)(kA < k0));
      const unsigned long long k1 = ba ? kA : k0;
      bb = (bool)((int)!isAny & (int)hb & (int)(kB < k1));
      const unsigned long long k2 = bb ? kB : k1;
      best = __uint_as_float((uint32_t)(k2 >> 32)), bestId = (uint32_t)k2;
    } else {
      ba = !isAny && ha && (ta < best || (ta == best && ida < bestId));
      const float b1 = ba ? ta : best;
      const uint32_t i1 = ba ? ida : bestId;
      bb = !isAny && hb && (tb < b1 || (tb == b1 && idb < i1));
      best = bb ? tb : b1, bestId = bb ? idb : i1;
    }
    if (MODE == TRAV_CLOSEST) {  // (pool mode recomputes u, v from the id: vertex_setup_ray)
      hit.u = bb ? ub : ba ? ua : hit.u, hit.v = bb ? vb : ba ? va : hit.v;
      hit.mesh = bb ? __float_as_uint(q2.z) : ba ? __float_as_uint(p2.z) : hit.mesh;
    }
    hit.t = best, hit.id = bestId;
    // (these three as mask arithmetic too were measured and lose: profiles/leaf_accept/)
    found = found || (isAny ? (ha || hb) : (ba || bb));
    if (MODE == TRAV_MIXED && shared && (ba || bb)) publish();
    return isAny && (ha || hb);
  }

  // Ray.cpp:9-24 on one 48-B record + the acceptance rule of RayTracer.h:40 (leaves with
  // more than two records: rt_options.bvh_leaf_max > 2).
  // Returns true when the ray is decided (any-hit rays only).
  template <bool STATS>
  RT_DEV bool test_record(const float4& q0, const float4& q1, const float4& q2, LaneStats& st) {
    if (STATS) st.tris++;
    float u, v, t;
    if (tri_test(o, d, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), u, v, t, DIVIDE) && t > 0.f) {
      if (MODE == TRAV_ANY || (MODE == TRAV_MIXED && anyHit)) {
        found = true;
        return true;
      }
      const uint32_t id = __float_as_uint(q2.y);
      if (t < best || (t == best && id < bestId)) {
        best = t, bestId = id, found = true;
        hit.t = t, hit.u = u, hit.v = v, hit.id = id, hit.mesh = __float_as_uint(q2.z);
        if (MODE == TRAV_MIXED && shared) publish();
      }
    }
    return false;
  }

  // the order of hits as one unsigned number: t bits << 32 | triangle id
  static RT_DEV unsigned long long hit_key(float t, uint32_t id) { return ((unsigned long long)__float_as_uint(t) << 32) | id; }

  // pool mode: make this lane's closest hit visible to the other lanes / the pixel lane
  RT_DEV void publish() {
    atomicMin(sharedKey + (int32_t)pj, hit_key(hit.t, hit.id));
  }

  // pool mode: adopt a closer hit another lane has published for the same ray
  RT_DEV void refresh_best() {
    const unsigned long long key = sharedKey[(int32_t)pj];
    const float kt = __uint_as_float((uint32_t)(key >> 32));
    const uint32_t kid = (uint32_t)key;
    if (key != ~0ull && (kt < best || (kt == best && kid < bestId))) best = kt, bestId = kid;
  }
};

// RayTracer::rayTrace (RayTracer.h:27-53) through the flattened BVH.
//   ANY = false: closest positive t; on equal t the lowest global triangle id wins
//                (== the reference's strict '<' in mesh-then-triangle order)
//   ANY = true : stops at the first accepted triangle with t > 0 (Renderer.cpp:54
//                only uses the bool)
// `on` = this lane has a ray; lanes without one still take part in the wave loop.
template <bool ANY, bool STATS, int LT = LT_NONE>
RT_DEV bool traverse(const DevScene& S, bool on, f3 o, f3 d, uint32_t* stack, HitRec& hit, LaneStats& st) {
  Trav<ANY ? TRAV_ANY : TRAV_CLOSEST, LT> T;
  T.idle(stack);
  if (on) T.start(o, d, S.invBoxScale);
  PH(PH_SETUP);
  while (wave_ballot(T.live()) != 0) {
    T.template round<STATS>(S, st);
    PH(PH_PRIMARY);  // (round() itself books descent and leaf time; the primary cast is coherent)
  }
  if (!ANY && T.found) hit = T.hit;
  return T.found;
}

// The reference algorithm itself: every triangle, reference order (RayTracer.h:32-51).
template <bool ANY, bool STATS>
RT_DEV bool brute(const DevScene& S, f3 o, f3 d, HitRec& hit, LaneStats& st) {
  float best = 3.402823466e+38f;
  bool found = false;
  for (uint32_t i = 0; i < S.n_tris; i++) {
    const float4* r = S.trisRef + 3 * (size_t)i;  // wave-uniform address -> scalar loads
    const float4 q0 = r[0], q1 = r[1], q2 = r[2];
    float u, v, t;
    if (tri_test(o, d, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), u, v, t, true)) {
      if (t > 0.f && t < best) {
        if (ANY) return true;
        best = t, found = true;
        hit.t = t, hit.u = u, hit.v = v, hit.id = i, hit.mesh = __float_as_uint(q2.z);
      }
    }
  }
  if (STATS) st.tris += S.n_tris;
  return found;
}

// `on`: lanes without a ray pass false (wave-uniform call sites, no early exits).
template <bool BRUTE, bool ANY, bool STATS, int LT = LT_NONE>
RT_DEV bool cast(const DevScene& S, bool on, f3 o, f3 d, uint32_t* stack, HitRec& hit, LaneStats& st) {
  if (BRUTE) return on && brute<ANY, STATS>(S, o, d, hit, st);
  return traverse<ANY, STATS, LT>(S, on, o, d, stack, hit, st);
}

// Renderer.cpp:274-277 dotArr: (w*a + u*b) + v*c per component
RT_DEV f3 interp3(const float* arr, uint4 tv, float w, float u, float v) {
  return w * ld(arr + 3 * (size_t)tv.x) + u * ld(arr + 3 * (size_t)tv.y) + v * ld(arr + 3 * (size_t)tv.z);
}

// ---------------------------------------------------------------- photon k-NN
// kdtree::knearest (kdtree.h:87-107 recursion, :180-195 driver) on the implicit
// median tree, restated step for step INCLUDING its quirks:
// heap seeded with array nodes [0,k), lagging m_bestdist, squared-vs-plain prune.
// std::make_heap/pop_heap/push_heap/sort_heap are restated from libstdc++
// (bits/stl_heap.h: __push_heap / __adjust_heap) because result ORDER feeds a
// float sum (Renderer.cpp:93-96).
// The entry accessors of a layout; HeapOps is the heap on top of them.
struct HeapInterleaved {
  uint2* e;  // [slot * BLOCK]: {distance bits, photon index} in one 8-byte word (one LDS op per move)
  RT_DEV float D(int s) const { return __uint_as_float(e[s * BLOCK].x); }
  RT_DEV uint32_t I(int s) const { return e[s * BLOCK].y; }
  RT_DEV void set(int s, float dv, uint32_t iv) const { e[s * BLOCK] = make_uint2(__float_as_uint(dv), iv); }
  RT_DEV void move(int dst, int src) const { e[dst * BLOCK] = e[src * BLOCK]; }
  // the heap of a lane whose Lds was carved for k slots (carve_lds puts it there)
  RT_DEV static HeapInterleaved at(const Lds& L, int) { return HeapInterleaved{L.heap}; }
};

// The wide k-NN (17 <= k <= RT_KNN_KMAX: k_render_wide, k_knn_wide) runs the same heap on one of two layouts
// (launcher: wide_layout):
//   HEAP_WIDE8:   the interleaved 8-byte entries above (one LDS op per move);
//   HEAP_SPLIT16: a plane of float distances [k][64], then a plane of 16-bit indices [k][64] (maps of fewer than
//                 65,535 photons, the rule kd_stack applies to the walk's stack): 6 bytes per slot, two ops per move.
enum { HEAP_WIDE8 = 0, HEAP_SPLIT16 = 1 };
template <int HL>
struct HeapPlanes {
  static_assert(HL == HEAP_SPLIT16, "the planes hold 16-bit indices");
  using Idx = uint16_t;
  float* d;  // [slot * BLOCK]
  Idx* i;    // [slot * BLOCK]
  RT_DEV float D(int s) const { return d[s * BLOCK]; }
  RT_DEV uint32_t I(int s) const { return i[s * BLOCK]; }
  RT_DEV void set(int s, float dv, uint32_t iv) const { d[s * BLOCK] = dv, i[s * BLOCK] = (Idx)iv; }
  RT_DEV void move(int dst, int src) const { d[dst * BLOCK] = d[src * BLOCK], i[dst * BLOCK] = i[src * BLOCK]; }
  // (carve_lds points a lane at its column of the heap region: the region starts 2 words per lane below)
  RT_DEV static HeapPlanes at(const Lds& L, int k) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* region = reinterpret_cast<uint32_t*>(L.heap - lane);
    return HeapPlanes{reinterpret_cast<float*>(region) + lane, reinterpret_cast<Idx*>(region + (size_t)k * BLOCK) + lane};
  }
};

template <class E>
struct HeapOps : E {
  using E::D;
  using E::I;
  using E::set;
  using E::move;
  RT_DEV static HeapOps at(const Lds& L, int k) { return HeapOps{E::at(L, k)}; }
  RT_DEV void push_up(int hole, int top, float vd, uint32_t vi) const {
    int parent = (hole - 1) / 2;
    while (hole > top && D(parent) < vd) {
      move(hole, parent);
      hole = parent;
      parent = (hole - 1) / 2;
    }
    set(hole, vd, vi);
  }
  RT_DEV void adjust(int hole, int len, float vd, uint32_t vi) const {
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
      child = 2 * (child + 1);
      if (D(child) < D(child - 1)) child--;
      move(hole, child);
      hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
      child = 2 * (child + 1);
      move(hole, child - 1);
      hole = child - 1;
    }
    push_up(hole, top, vd, vi);
  }
  // std::pop_heap on [0,len): max goes to slot len-1, [0,len-1) stays a heap
  RT_DEV void pop(int len) const {
    if (len > 1) {
      const float vd = D(len - 1);
      const uint32_t vi = I(len - 1);
      move(len - 1, 0);
      adjust(0, len - 1, vd, vi);
    }
  }
  RT_DEV void make(int len) const {
    if (len < 2) return;
    for (int parent = (len - 2) / 2;; parent--) {
      adjust(parent, len, D(parent), I(parent));
      if (parent == 0) return;
    }
  }
  RT_DEV void sort(int len) const {
    while (len > 1) {
      pop(len);
      len--;
    }
  }
};
using Heap = HeapOps<HeapInterleaved>;  // k <= 16 (k_render, k_knn)
template <int HL>
using WideHeap = HeapOps<typename std::conditional<HL == HEAP_WIDE8, HeapInterleaved, HeapPlanes<HL>>::type>;
// LDS rows (64 words) of a k-slot heap on layout HL
constexpr uint32_t heap_rows(int hl, uint32_t k) { return hl == HEAP_SPLIT16 ? k + (k + 1u) / 2u : 2u * k; }

RT_DEV float photon_dist(const DevScene& S, uint32_t n, f3 p, float4& pos) {
  pos = S.phPos[n];
  return dist3(mk(pos.x, pos.y, pos.z), p);
}

// kdtree::knearest (kdtree.h:87-107 recursion, :180-195 driver) over the tree's EXPLICIT topology (kd_build.hip
// k_kd_topology: child indices, axis and the parent's split in a record per photon).  One flat loop, one node per
// iteration, the same code for a lane that descends and a lane that comes back up:
//   * visit (kdtree.h:88-99): distance, insert if d < m_bestdist; stop below a zero m_bestdist (:101);
//   * descend into the near child (:102-104) and leave the far child on the lane's LDS stack — one word, its index;
//   * a lane with nowhere to descend pops the next far child and, in the next iteration, FIRST applies kdtree.h:105
//     (dx * dx >= m_bestdist, squared against plain, as there) with the m_bestdist of that moment and the split distance
//     rebuilt from the child's own record (parent's coordinate - query coordinate: the float subtraction the parent's
//     visit made) — a rejected child costs one iteration, nothing is unwound level by level.
// Round 3's walk carried the implicit tree's (b, e, depth, pending / side / parity bit masks) and spent a third of its
// vector instructions on range arithmetic, in two nested data-dependent loops whose trip counts the whole wave paid.
// Result-preserving extra prune, as before (546 -> ~1/6 of the node visits on C3): every photon of a far subtree lies
// beyond the split plane, so its float distance is >= |dx| * (1 - 1.5e-7) (monotone float subtraction; three roundings
// under the square root, one on it), and m_bestdist never increases for k >= 2 (the new value is the second largest of
// the old heap plus the new point): if |dx| * (1 - 4.8e-7) already reaches it, no node of that subtree can pass
// d < m_bestdist (kdtree.h:92) and the heap — hence the result — is the same whether or not the subtree is walked.
// (With k = 1 "the remaining k - 1" is empty and front() is the PREVIOUS insert, which may be larger than the one
// before: there only the reference's own test runs.)  The reference's own test is much weaker whenever m_bestdist < 1.
// After the call the heap holds the k results in ascending distance order.
// S16: the pending far children as 16-bit indices (maps of fewer than 65,535 photons: config 3's 35,744): half the stack's LDS,
// which with the k-heap is what caps the photon kernel's waves per CU.
constexpr uint32_t KD_NONE = 0x3fffffffu;
template <bool S16, class HP>
RT_DEV uint32_t knn_query(const DevScene& S, f3 p, int k, const HP& H, uint32_t* stack) {
  using Entry = typename std::conditional<S16, uint16_t, uint32_t>::type;
  constexpr uint32_t NONE_E = S16 ? 0xffffu : KD_NONE;
  float4 pos;
  for (int j = 0; j < k; j++) H.set(j, photon_dist(S, (uint32_t)j, p, pos), (uint32_t)j);
  H.make(k);
  double bestdist = (double)H.D(0);
  float skip2 = (float)(bestdist * bestdist * (1.0 + 1e-6));
  uint32_t visited = 0;
  const bool mono = k >= 2;  // m_bestdist is non-increasing
  // (this lane's column: [row][lane] entries; 16-bit entries pack two rows into one of the stack's 256-byte rows)
  Entry* top = S16 ? reinterpret_cast<Entry*>(stack - (threadIdx.x & 63u)) + (threadIdx.x & 63u) : reinterpret_cast<Entry*>(stack);
  *top = (Entry)NONE_E;  // row 0: the sentinel an empty stack pops
  uint32_t cur = S.n_photons / 2u;  // the root: the median of [0, n)
  bool popped = false;
  while (cur != KD_NONE) {
    // the node's record: {position, left | axis << 30}{right, parent's split, parent's axis, -}: both halves in one line
    const uint4 ra = S.phTopo[2 * (size_t)cur], rb = S.phTopo[2 * (size_t)cur + 1];
    const float4 P = make_float4(__uint_as_float(ra.x), __uint_as_float(ra.y), __uint_as_float(ra.z), 0.f);
    const uint4 T = make_uint4(ra.w, rb.x, rb.y, rb.z);
    bool go = true;
    if (popped) {  // kdtree.h:105 for the activation that left this child behind, and the geometric prune
      const float pc = T.w == 0u ? p.x : T.w == 1u ? p.y : p.z;
      const double dxp = (double)(__uint_as_float(T.z) - pc);
      go = !(dxp * dxp >= bestdist) && !(mono && (dxp < 0 ? -dxp : dxp) * (1.0 - 4.8e-7) >= bestdist);
    }
    uint32_t next = KD_NONE;
    if (go) {
      ++visited;
      // kdtree.h:90-92 compares the fp32 distance sqrt(d2), widened, with m_bestdist.  The correctly rounded root is
      // only taken when d2 is not clearly out: d2 >= skip2 = m_bestdist^2 * (1 + 1e-6) rounded to float implies
      // sqrtf(d2) >= m_bestdist (a correctly rounded sqrt is monotone and within 6e-8 relative), i.e. no insert.
      const f3 dv = mk(P.x, P.y, P.z) - p;
      const float d2 = dot3(dv, dv);
      if (!(d2 >= skip2)) {
        const float dn = __builtin_sqrtf(d2);
        if ((double)dn < bestdist) {
          H.pop(k);                       // pop_heap
          bestdist = (double)H.D(0);      // front() of the remaining k-1, then pop_back
          H.set(k - 1, dn, cur);          // push_back(*root)
          H.push_up(k - 1, 0, dn, cur);   // push_heap
          skip2 = (float)(bestdist * bestdist * (1.0 + 1e-6));
        }
      }
      if (bestdist != 0) {
        const uint32_t axis = T.x >> 30;
        const float dx = axis == 0u ? dv.x : axis == 1u ? dv.y : dv.z;  // node coordinate - query coordinate (kdtree.h:102)
        const bool left = dx > 0.f;
        const uint32_t l = T.x & KD_NONE, r = T.y;
        const uint32_t far = left ? r : l;
        next = left ? l : r;
        // m_bestdist never increases (k >= 2), so a far side that both tests already reject now stays rejected: it is
        // not even recorded
        // (the entry is stored above the top unconditionally and claimed by a select, as Trav::round does: one row
        // beyond the deepest pending entry exists — the stack has a row per tree level plus the sentinel's)
        const double dxd = (double)dx;
        const bool out1 = dxd * dxd >= bestdist, out2 = (dxd < 0 ? -dxd : dxd) * (1.0 - 4.8e-7) >= bestdist;
        const bool record = (far != KD_NONE) & (!mono | !(out1 | out2));
        top[BLOCK] = (Entry)far;  // (KD_NONE truncates to the 16-bit sentinel)
        top += record ? BLOCK : 0;
      }
    }
    popped = next == KD_NONE;
    if (popped) {
      const uint32_t e = *top;
      next = e == NONE_E ? KD_NONE : e;
      if (e != NONE_E) top -= BLOCK;  // (the sentinel stays)
    }
    cur = next;
  }
  H.sort(k);
  return visited;
}

// ---------------------------------------------------------------- shading
constexpr int POOL_L = 3;                              // lights handled by the shadow-ray pool

RT_DEV uint32_t lanes_below(uint64_t m) {  // number of set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Renderer.cpp:42-43: interpolated shading normal and hit point
template <bool FAST = false>
RT_DEV void vertex_setup(const DevScene& S, const HitRec& h, f3& hitNormal, f3& point) {
  const float w = 1.f - h.u - h.v;
  const uint4 tv = S.triShade[h.id];
  hitNormal = unit3<FAST>(interp3(S.vnrm, tv, w, h.u, h.v));
  point = interp3(S.vpos, tv, w, h.u, h.v);
}

// The same from the triangle id alone (vertex pool: a bounce hit comes back as a
// (t, id) key).  u, v are recomputed by Ray.cpp:9-24 on exactly the operands the
// walker's record holds — p0 and the float edge differences bvh_build.cpp stores —
// so they are the bits the walker had; the vertex loads are the ones the
// interpolation needs anyway.
// (tv, u, v: the triangle's record and the barycentrics, for the callers that interpolate more than the normal)
template <bool FAST = false>
RT_DEV void vertex_setup_ray(const DevScene& S, uint32_t id, f3 o, f3 d, f3& hitNormal, f3& point, uint4& tv, float& u, float& v) {
  tv = S.triShade[id];
  const f3 p0 = ld(S.vpos + 3 * (size_t)tv.x), p1 = ld(S.vpos + 3 * (size_t)tv.y), p2 = ld(S.vpos + 3 * (size_t)tv.z);
  float t;
  tri_test(o, d, p0, p1 - p0, p2 - p0, u, v, t, true);  // (once per vertex: the division; the same bits as the walker's)
  const float w = 1.f - u - v;
  hitNormal = unit3<FAST>(interp3(S.vnrm, tv, w, u, v));
  point = w * p0 + u * p1 + v * p2;
}
// (... and e1 = p1 - p0, e2 = p2 - p0, the edges the test ran on, for the caller that forms a tangent frame: the
// positions are loaded once)
template <bool FAST = false>
RT_DEV void vertex_setup_ray(const DevScene& S, uint32_t id, f3 o, f3 d, f3& hitNormal, f3& point, uint4& tv, float& u, float& v,
                             f3& e1, f3& e2) {
  tv = S.triShade[id];
  const f3 p0 = ld(S.vpos + 3 * (size_t)tv.x), p1 = ld(S.vpos + 3 * (size_t)tv.y), p2 = ld(S.vpos + 3 * (size_t)tv.z);
  e1 = p1 - p0, e2 = p2 - p0;
  float t;
  tri_test(o, d, p0, e1, e2, u, v, t, true);
  const float w = 1.f - u - v;
  hitNormal = unit3<FAST>(interp3(S.vnrm, tv, w, u, v));
  point = w * p0 + u * p1 + v * p2;
}
template <bool FAST = false>
RT_DEV void vertex_setup_ray(const DevScene& S, uint32_t id, f3 o, f3 d, f3& hitNormal, f3& point, uint32_t& mesh) {
  uint4 tv;
  float u, v;
  vertex_setup_ray<FAST>(S, id, o, d, hitNormal, point, tv, u, v);
  mesh = tv.w;
}

// Per-vertex albedo (rt_render_colors, rt_amd.h): the colour of the hit from the three vertices' colours,
// c = (c0 + u (c1 - c0)) + v (c2 - c0) per component, every operation rounded on its own — three equal colours give c0
// exactly — gathered per lane by vertex id as the normals are ...
RT_DEV f3 vertex_color(const float* vcol, uint4 tv, float u, float v) {
  const f3 c0 = ld(vcol + 3 * (size_t)tv.x), c1 = ld(vcol + 3 * (size_t)tv.y), c2 = ld(vcol + 3 * (size_t)tv.z);
  return (c0 + u * (c1 - c0)) + v * (c2 - c0);
}
// ... and the kdDiffuse the vertex shades with: make_dev_mat's two operations on c in place of the mesh's albedo
RT_DEV f3 vertex_kd(const DevScene& S, const float* vcol, uint4 tv, float u, float v) {
  const f3 diffuse = vertex_color(vcol, tv, u, v) / 3.14159274f;  // c / float(M_PI)
  return S.mats[tv.w].kd * diffuse;
}
// Image-textured albedo (rt_render_textured, rt_amd.h's sampler).  gfx950 has no image instructions: a sample is plain
// loads and float32 arithmetic, every operation rounded on its own.
// tex_wrap: the texel index of the integer coordinate i on an axis of n texels — REPEAT: the non-negative remainder,
// ((i % n) + n) % n; CLAMP: min(max(i, 0), n - 1).
RT_DEV int tex_wrap(int i, int n, bool clamp) {
  if (clamp) return min(max(i, 0), n - 1);
  const int r = i % n;
  return r < 0 ? r + n : r;
}
// the sample of texture D at (s, t).  int(floorf(.)) stays far inside int32: |uv| <= 1024 at the vertices and u, v in
// [0, 1] give |s| <= 1024 + 2 * 2048 = 5120, and 5120 * 16384 + 1 < 2^27.  The bilinear filter samples row by row (a, then
// b): six texel floats are live at most.
RT_DEV f3 tex_sample(const float* __restrict__ texels, TexDesc D, float s, float t) {
  const int W = (int)D.width, H = (int)D.height;
  const bool cs = (D.bits & TEX_CLAMP_S) != 0, ct = (D.bits & TEX_CLAMP_T) != 0;
  const float* base = texels + 3 * (size_t)D.offset;
  if (!(D.bits & TEX_BILINEAR)) {
    const int i = tex_wrap((int)floorf(s * (float)W), W, cs), j = tex_wrap((int)floorf(t * (float)H), H, ct);
    return ld(base + 3 * ((size_t)j * (size_t)W + (size_t)i));
  }
  const float x = s * (float)W - 0.5f, y = t * (float)H - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int i0 = tex_wrap((int)xf, W, cs), i1 = tex_wrap((int)xf + 1, W, cs);
  const int j0 = tex_wrap((int)yf, H, ct), j1 = tex_wrap((int)yf + 1, H, ct);
  const float* r0 = base + 3 * (size_t)j0 * (size_t)W;
  const float* r1 = base + 3 * (size_t)j1 * (size_t)W;
  const f3 t00 = ld(r0 + 3 * i0), t01 = ld(r0 + 3 * i1);
  const f3 a = t00 + fx * (t01 - t00);
  const f3 t10 = ld(r1 + 3 * i0), t11 = ld(r1 + 3 * i1);
  const f3 b = t10 + fx * (t11 - t10);
  return a + fy * (b - a);
}
// the hit's texture coordinate on one axis, vertex_color's form: three equal values give s0 exactly
RT_DEV float tex_coord(float s0, float s1, float s2, float u, float v) { return (s0 + u * (s1 - s0)) + v * (s2 - s0); }
// The albedo a vertex of a textured frame shades with: the sample of its mesh's texture at the hit's uv, or (no texture)
// the mesh's own.  found: the mesh has a texture.  The three uv gathers and the mesh's texture index are independent of
// each other and go out together.
RT_DEV f3 tex_color(const TexRec& T, uint4 tv, float u, float v, bool& found) {
  const float2* uv = reinterpret_cast<const float2*>(T.uv);
  const uint32_t ti = T.meshTex[tv.w];
  const float2 a = uv[tv.x], b = uv[tv.y], c = uv[tv.z];
  found = ti != kTexNone;
  if (!found) return mk(0.f, 0.f, 0.f);
  const TexDesc D = T.desc[ti];
  return tex_sample(T.texels, D, tex_coord(a.x, b.x, c.x, u, v), tex_coord(a.y, b.y, c.y, u, v));
}
// ... and the kdDiffuse: vertex_kd's two operations on the sample; a mesh without a texture keeps its DevMat's
RT_DEV f3 tex_kd(const DevScene& S, const TexRec& T, uint4 tv, float u, float v) {
  bool found;
  const f3 c = tex_color(T, tv, u, v, found);
  if (!found) return ld(S.matsDev[tv.w].kdDiffuse);
  const f3 diffuse = c / 3.14159274f;  // c / float(M_PI)
  return S.mats[tv.w].kd * diffuse;
}

// The material a vertex of a material-map frame shades with (rt_render_material): the hit mesh's, with albedo, f0 and
// (kd, alpha) replaced by the samples of the mesh's three textures at the hit's one uv, each under its own texture's
// filter and wraps; kTexNone keeps the mesh's field.  The three per-mesh indices and the three uv gathers are independent
// of each other and go out together, the descriptors follow their indices, and the maps are sampled one after the other:
// one map's six texel floats are live at most.  (The descriptor of a map that is kTexNone is texture 0's, which a
// resident set always has, and is not used.)
RT_DEV rt_material tex_mat(const DevScene& S, const MatRec& M, uint4 tv, float u, float v) {
  const float2* uv = reinterpret_cast<const float2*>(M.uv);
  const uint32_t ta = M.meshTex[tv.w], tf = M.meshF0[tv.w], tk = M.meshKdAlpha[tv.w];
  const float2 a = uv[tv.x], b = uv[tv.y], c = uv[tv.z];
  rt_material m = S.mats[tv.w];
  const TexDesc Da = M.desc[ta != kTexNone ? ta : 0u], Df = M.desc[tf != kTexNone ? tf : 0u], Dk = M.desc[tk != kTexNone ? tk : 0u];
  const float s = tex_coord(a.x, b.x, c.x, u, v), t = tex_coord(a.y, b.y, c.y, u, v);
  if (ta != kTexNone) {
    const f3 x = tex_sample(M.texels, Da, s, t);
    m.albedo[0] = x.x, m.albedo[1] = x.y, m.albedo[2] = x.z;
  }
  if (tf != kTexNone) {
    const f3 x = tex_sample(M.texels, Df, s, t);
    m.f0[0] = x.x, m.f0[1] = x.y, m.f0[2] = x.z;
  }
  if (tk != kTexNone) {
    const f3 x = tex_sample(M.texels, Dk, s, t);
    m.kd = x.x, m.alpha = x.y;
  }
  return m;
}
// The shading normal a vertex of a normal-mapped frame shades and bounces with (rt_render_normal_mapped): N, the
// interpolated unit normal, turned by the sample of the mesh's normal map in the tangent frame of the hit triangle.  The
// frame is formed here, from the triangle's CURRENT edges e1, e2 (p1 - p0, p2 - p0) and its three uvs: nothing of it is
// cached, so it follows every update.  The operations are rt_amd.h's list, one by one, every one rounded on its own.  N
// comes back untouched — no arithmetic on it — where the mesh has no map, where the sample's x and y are both 0 (a flat
// texel), and where the frame or the result degenerates.  The uv gathers and the map's index are tex_mat's loads again
// (the same addresses, no store between: the compiler keeps one copy), and the map is sampled behind tex_mat's three.
RT_DEV f3 nmap_bend(const NrmRec& R, uint4 tv, float u, float v, f3 e1, f3 e2, f3 N) {
  const float2* uv = reinterpret_cast<const float2*>(R.mat.uv);
  const uint32_t tn = R.meshNormal[tv.w];
  const float2 a = uv[tv.x], b = uv[tv.y], c = uv[tv.z];
  if (tn == kTexNone) return N;
  const TexDesc D = R.mat.desc[tn];
  const float a1 = b.x - a.x, a2 = c.x - a.x, b1 = b.y - a.y, b2 = c.y - a.y;
  const float r = a1 * b2 - a2 * b1;
  if (!(r != 0.f)) return N;  // (zero or NaN: the uvs span no area)
  f3 Tr = b2 * e1 - b1 * e2, Br = a1 * e2 - a2 * e1;
  if (r < 0.f) Tr = -Tr, Br = -Br;
  const f3 Tp = Tr - dot3(N, Tr) * N;
  if (!(dot3(Tp, Tp) > 0.f)) return N;
  const f3 T = unit3(Tp);
  f3 B = cross3(N, T);
  if (dot3(B, Br) < 0.f) B = -B;
  const f3 m = tex_sample(R.mat.texels, D, tex_coord(a.x, b.x, c.x, u, v), tex_coord(a.y, b.y, c.y, u, v));
  const float x = 2.f * m.x - 1.f, y = 2.f * m.y - 1.f, z = 2.f * m.z - 1.f;
  if (x == 0.f && y == 0.f) return N;
  const f3 V = (x * T + y * B) + z * N;
  const float vv = dot3(V, V);
  if (!(vv > 0.f) || !(vv < __builtin_inff())) return N;  // (not finite and positive)
  return unit3(V);
}
// What a vertex shades with in place of its mesh's DevMat, while the wave traverses: the value (v) and the rows of LDS
// where it is parked over every walk (ROWS of [64] floats, the wave's, behind its stack rows and pool, allocated for these
// instances alone: held in registers, it would cost the timed instances, which sit at their budget, as many more of
// them).  WHOLE says how the read-back value enters the light-independent half of the BSDF: a kdDiffuse overwrites the
// mesh's; a whole material forms the half anew by bsdf_base(const rt_material&) (the same operands every time, so the
// same bits).  ParkNone: a frame without a surface — an empty argument, so that its instances keep the signatures (and
// the code) they had.
struct ParkNone {
  static constexpr int ROWS = 0;
};
struct ParkKd {  // a kdDiffuse, in three rows
  static constexpr int ROWS = 3;
  static constexpr bool WHOLE = false;
  f3 v;
  float* park;
  RT_DEV void store(uint32_t lane) const { park[lane] = v.x, park[64 + lane] = v.y, park[128 + lane] = v.z; }
  RT_DEV f3 load(uint32_t lane) const { return mk(park[lane], park[64 + lane], park[128 + lane]); }
};
struct ParkMat {  // a material, in eight rows in rt_material's field order
  static constexpr int ROWS = 8;
  static constexpr bool WHOLE = true;
  rt_material v;
  float* park;
  RT_DEV void store(uint32_t lane) const {
    park[lane] = v.kd, park[64 + lane] = v.alpha;
    for (int c = 0; c < 3; ++c) park[(2 + c) * 64 + lane] = v.albedo[c], park[(5 + c) * 64 + lane] = v.f0[c];
  }
  RT_DEV rt_material load(uint32_t lane) const {
    rt_material m;
    m.kd = park[lane], m.alpha = park[64 + lane];
    for (int c = 0; c < 3; ++c) m.albedo[c] = park[(2 + c) * 64 + lane], m.f0[c] = park[(5 + c) * 64 + lane];
    return m;
  }
};
// The surface policies, one per surface a frame can carry (surface_t picks it by the frame's LT_* bits): the record its
// frames take (Rec), what a vertex parks (Parked), how that value is formed from the hit's (tv, u, v) (form), whether
// the surface replaces the vertex's shading normal before anything reads it (BENDS, then by bend), and the records the
// launcher answers hipErrorInvalidValue to (refused).  A new surface is one more policy here, its bit in surface_t and
// its row in frame_variants.h.
struct NoRec {};
struct SurfNone {
  using Rec = NoRec;
  using Parked = ParkNone;
  static constexpr int LT = 0;
  static constexpr bool BENDS = false;
  static bool refused(const Rec&) { return false; }
};
struct SurfVCol {  // rt_render_colors
  using Rec = VColRec;
  using Parked = ParkKd;
  static constexpr int LT = LT_VCOL;
  static constexpr bool BENDS = false;
  static RT_DEV f3 form(const DevScene& S, const Rec& R, uint4 tv, float u, float v) { return vertex_kd(S, R.vcol, tv, u, v); }
  static bool refused(const Rec& R) { return !R.vcol; }
};
struct SurfTex {  // rt_render_textured
  using Rec = TexRec;
  using Parked = ParkKd;
  static constexpr int LT = LT_TEX;
  static constexpr bool BENDS = false;
  static RT_DEV f3 form(const DevScene& S, const Rec& R, uint4 tv, float u, float v) { return tex_kd(S, R, tv, u, v); }
  static bool refused(const Rec& R) { return !R.uv || !R.meshTex || !R.desc || !R.texels; }
};
struct SurfMat {  // rt_render_material
  using Rec = MatRec;
  using Parked = ParkMat;
  static constexpr int LT = LT_MAT;
  static constexpr bool BENDS = false;
  static RT_DEV rt_material form(const DevScene& S, const Rec& R, uint4 tv, float u, float v) { return tex_mat(S, R, tv, u, v); }
  static bool refused(const Rec& R) { return !R.uv || !R.meshTex || !R.desc || !R.texels || !R.meshF0 || !R.meshKdAlpha; }
};
struct SurfNrm {  // rt_render_normal_mapped: the material-map frame's value and rows, and a bent normal
  using Rec = NrmRec;
  using Parked = ParkMat;
  static constexpr int LT = LT_NMAP;
  static constexpr bool BENDS = true;
  static RT_DEV rt_material form(const DevScene& S, const Rec& R, uint4 tv, float u, float v) { return tex_mat(S, R.mat, tv, u, v); }
  static RT_DEV f3 bend(const Rec& R, uint4 tv, float u, float v, f3 e1, f3 e2, f3 N) { return nmap_bend(R, tv, u, v, e1, e2, N); }
  static bool refused(const Rec& R) { return SurfMat::refused(R.mat) || !R.meshNormal; }
};
template <int LTV>
using surface_t = std::conditional_t<(LTV & LT_VCOL) != 0, SurfVCol,
                  std::conditional_t<(LTV & LT_TEX) != 0, SurfTex,
                  std::conditional_t<(LTV & LT_MAT) != 0, SurfMat,
                  std::conditional_t<(LTV & LT_NMAP) != 0, SurfNrm, SurfNone>>>>;

// Renderer.cpp:63-104: photon-map radiance estimate at the vertex (HP: the heap's layout, WideHeap for k > 16)
template <bool STATS, class HP = Heap>
RT_DEV f3 shade_photon(const DevScene& S, const RenderArgs& A, f3 rayDir, const HitRec& h, const Lds& L, f3 hitNormal,
                       f3 point, LaneStats& st) {
  const rt_material mat = S.mats[h.mesh];
  const HP H = HP::at(L, (int)A.k);
  const int k = (int)A.k;
  st.knn++;
  const uint32_t vis = A.kd16 ? knn_query<true>(S, point, k, H, L.stack) : knn_query<false>(S, point, k, H, L.stack);
  if (STATS) st.kd += vis;
  const float4 far = S.phPos[H.I(k - 1)];
  const float r = dist3(mk(far.x, far.y, far.z), point);
  const float area = (float)(3.14159265358979323846 * (double)r * (double)r);
  f3 avg = mk(0.f, 0.f, 0.f), radiance = mk(0.f, 0.f, 0.f);
  for (int j = 0; j < k; j++) {
    avg = avg + f4xyz(S.phDir[H.I(j)]);
    radiance = radiance + mk(1.f, 1.f, 1.f);
  }
  radiance = radiance / area;
  radiance = radiance / (float)(int)A.photons_requested;
  radiance = radiance * 100.f;  // Renderer.h:45
  const f3 bsdf = bsdf_eval(mat, hitNormal, unit3(avg), -rayDir);
  return mk(0.f, 0.f, 0.f) + radiance * bsdf;
}

// A vertex's colour per light group (rt_render_lights): c[g] = the sum, from +0 and in light order, of the unoccluded
// terms of the lights in masks[g].  Only ever indexed by the constants of a fully unrolled loop: registers, no scratch.
struct GroupCols {
  f3 c[RT_LIGHT_GROUPS_MAX];
};
RT_DEV void group_cols_zero(GroupCols& q) {
#pragma unroll
  for (int g = 0; g < RT_LIGHT_GROUPS_MAX; ++g) q.c[g] = mk(0.f, 0.f, 0.f);
}
// one unoccluded light's term into the groups that hold light l (G is a kernel argument and l wave-uniform: scalar tests)
RT_DEV void group_cols_add(GroupCols& q, const LightGroupsRec& G, uint32_t l, f3 term) {
#pragma unroll
  for (int g = 0; g < RT_LIGHT_GROUPS_MAX; ++g)
    if ((G.masks[g] >> l) & 1u) q.c[g] = q.c[g] + term;
}

// A sample's light indices (rt_render_pick): slot j < R.m holds pick(u_j).  Read by slot through selects (pick_at), never
// indexed: registers, no scratch.
struct Picks {
  uint32_t k0, k1, k2;
};
static_assert(RT_PICK_SLOTS_MAX == 3 && RT_PICK_SLOTS_MAX == POOL_L, "a picked frame's slots are the pool's lights");
RT_DEV uint32_t pick_at(const Picks& p, uint32_t slot) { return slot == 0u ? p.k0 : slot == 1u ? p.k1 : p.k2; }
// pick(u): the smallest k with u < thresholds[k] — it exists for every u in [0, 1): thresholds[n - 1] is 1.0f.  The
// index differs from lane to lane: vector loads, of a table that stays cache-resident.
RT_DEV uint32_t pick_light(const PickRec& R, float u) {
  uint32_t lo = 0u, hi = R.n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (u < R.thresholds[mid]) hi = mid;
    else lo = mid + 1u;
  }
  return lo;
}
// the m picks of sample i of pixel pix, from the sample's own stream (one draw per slot, in slot order)
RT_DEV Picks draw_picks(const PickRec& R, uint32_t seed, uint32_t pix, uint32_t i) {
  Rng e{rt_stream_seed(seed, RT_STREAM_PICK, pix, i)};
  Picks p{0u, 0u, 0u};
  p.k0 = pick_light(R, e.canonF());
  if (R.m > 1u) p.k1 = pick_light(R, e.canonF());
  if (R.m > 2u) p.k2 = pick_light(R, e.canonF());
  return p;
}
// What the light loops of a picked frame take in place of the scene's list: the record and the lane's picks.  NoPick:
// every other frame — an empty argument, so that the instances without picks keep the signatures (and the code) they had.
struct NoPick {};
struct PickArgs {
  const PickRec* R;
  Picks k;
};
template <class PK>
constexpr bool is_pick = std::is_same_v<PK, PickArgs>;
// light `slot` of the loop: the scene's, or the scaled light of the lane's slot — six 16-byte loads at most, of which the
// compiler keeps what the caller reads
RT_DEV rt_light loop_light(const DevScene& S, NoPick, uint32_t slot) { return S.lights[slot]; }
RT_DEV rt_light loop_light(const DevScene&, const PickArgs& a, uint32_t slot) { return a.R->lights[pick_at(a.k, slot)].l; }
RT_DEV uint32_t loop_lights(const DevScene& S, NoPick) { return S.n_lights; }
RT_DEV uint32_t loop_lights(const DevScene&, const PickArgs& a) { return a.R->m; }

// Renderer.cpp:49-60, one light after the other (brute-force variant and scenes
// with more than POOL_L lights).  Called by lanes that own a vertex only.
// GROUPS (rt_render_lights): the terms go into *gc by group instead of into the returned colour, which stays 0.
// PK = PickArgs (rt_render_pick): the light list is the sample's picked lights, in slot order, instead of the scene's.
// VC with rows (ParkKd, ParkMat: the coloured, textured and material-map frames): the vertex's own value in place of
// the mesh's, parked in LDS over every walk and entered into the light-independent half behind each.
template <bool BRUTE, bool STATS, bool GROUPS = false, class PK = NoPick, class VC = ParkNone>
RT_DEV f3 shade_direct_seq(const DevScene& S, Rng& g, f3 rayDir, const HitRec& h, uint32_t* stack, f3 hitNormal,
                           f3 point, LaneStats& st, const LightGroupsRec* G = nullptr, GroupCols* gc = nullptr, PK pk = PK(),
                           VC vc = VC()) {
  BsdfBase base = bsdf_base(S.matsDev[h.mesh], hitNormal, -rayDir);  // the light-independent half, once
  if constexpr (VC::ROWS != 0) vc.store(threadIdx.x & 63u);
  f3 color = mk(0.f, 0.f, 0.f);
  if constexpr (GROUPS) group_cols_zero(*gc);
  for (uint32_t li = 0; li < loop_lights(S, pk); li++) {
    const rt_light Lt = loop_light(S, pk, li);
    const f3 toLight = light_sample(g, Lt) - point;
    HitRec tmp;
    st.shadow++;
    if (cast<BRUTE, true, STATS>(S, true, point, toLight, stack, tmp, st)) continue;
    if constexpr (VC::ROWS != 0) {
      asm volatile("" ::: "memory");  // (read back behind the walk, not held over it)
      if constexpr (VC::WHOLE) base = bsdf_base(vc.load(threadIdx.x & 63u), hitNormal, -rayDir);
      else base.kdDiffuse = vc.load(threadIdx.x & 63u);
    }
    const f3 bsdf = bsdf_apply(base, toLight);
    f3 radiance;
    if constexpr (is_pick<PK>) {
      // (the lane's own light is fetched again behind the walk, as the pool's colour loop does: held, its eleven words
      // that light_eval reads would sit in VGPRs across the traversal)
      asm volatile("" ::: "memory");
      radiance = light_eval(loop_light(S, pk, li), point);
    } else radiance = light_eval(Lt, point);
    if constexpr (GROUPS) group_cols_add(*gc, *G, li, radiance * bsdf);
    else color = color + radiance * bsdf;
  }
  return color;
}

// ---------------------------------------------------------------- vertex pool
// Everything a path vertex sends out is known as soon as the vertex exists: the
// n_lights shadow rays (Renderer.cpp:52-54: the light samples are drawn
// unconditionally, in light order) AND the bounce ray (Renderer.cpp:164-166: the
// hemisphere sample depends on the normal and the stream only).  So all
// (n_lights + 1) x (lanes with a vertex) rays of a wave go into one LDS pool and the
// 64 lanes work through it as WORKERS — a lane whose ray is decided fetches the next
// undecided one (ballot + mbcnt compaction, no atomics) instead of idling until
// the slowest of 64 rays ends.  Per pixel lane the pool holds: vertex position (3
// words), one direction per light (3 x POOL_L), the bounce direction (3), the bounce
// result as a 64-bit key (t, id).  Shadow results are one bit per (light, lane).  Arithmetic and draw order per pixel are exactly those of
// the sequential code, so results are bit-identical.
constexpr int VP_PT = 0, VP_DIR = 192, VP_BDIR = VP_DIR + 192 * POOL_L, VP_KEY = VP_BDIR + 192, VP_LIST = VP_KEY + 128,
              VP_RES = VP_LIST + 32;
constexpr int VP_WORDS = VP_RES + 2 * POOL_L + 2;
constexpr int VP_COMPACT_SAVES = 64 * POOL_L;  // words a compact pool is shorter by
// offsets of everything behind the per-light block, by layout
template <int CP> struct VpLayout {  // CP = 0: full, 1: light parameters, 2: ... and no bounce directions, 3: keys, list and result bits only
  static constexpr int PER_LIGHT = CP ? 128 : 192;
  static constexpr int BDIR = CP == 3 ? 0 : VP_DIR + PER_LIGHT * POOL_L, KEY = BDIR + (CP >= 2 ? 0 : 192), LIST = KEY + 128, RES = LIST + 32;
  static constexpr int WORDS = RES + 2 * POOL_L + 2;
};
static_assert(VpLayout<3>::WORDS == (int)rtbvh::kWavePoolWordsMin && VpLayout<3>::KEY % 2 == 0, "the smallest pool (bvh_build.h sizes the depth cap with it)");
static_assert(VpLayout<0>::WORDS == VP_WORDS && VpLayout<1>::WORDS == VP_WORDS - VP_COMPACT_SAVES &&
              VpLayout<2>::WORDS == VP_WORDS - 2 * VP_COMPACT_SAVES, "pool layouts");
static_assert(VpLayout<1>::KEY % 2 == 0 && VpLayout<2>::KEY % 2 == 0, "64-bit keys need 8-byte alignment");
static_assert(VP_KEY % 2 == 0, "64-bit keys need 8-byte alignment");
static_assert(VP_WORDS == (int)rtbvh::kWavePoolWords && BLOCK == (int)rtbvh::kStackRowWords, "bvh_build.h sizes the depth cap with these");

// BOUNCE = false: the body for a pool that is known to hold shadow rays only — the pool of a path's deepest vertex, and
// every pool of a frame without bounces (`bounceRay` is false and not read).  Its walker is the any-hit one (no candidate
// distance or id, no acceptance chains, no keys to publish or adopt) and the bounce kind is gone from the rank arithmetic,
// the hand-out and the direction fetch; hand-out order, thresholds, stealing and the shared result bits are the same code,
// so the schedule — and the counted pass's node and triangle totals — are the same.  BOUNCE = true is the general body:
// `bounceRay` says at run time whether a bounce ray is sent.
// GROUPS (rt_render_lights): the loop after the pool adds every unoccluded term into *gc by group (G's masks) instead of
// into the returned colour, which stays 0; nothing before that loop differs.
// PK = PickArgs (rt_render_pick): the pool's lights are the lane's picked ones, in slot order: the fill loop samples
// them and the colour loop evaluates them, each lane fetching its own from the record's table.  The workers read the full
// layout's toLight directions only, so the rounds, the hand-out, the stealing and the result bits are the same code.
// VC with rows (ParkKd, ParkMat): the vertex's own value in place of the mesh's.  It is parked in VC::ROWS rows of LDS
// behind the pool's words (the launcher allocates them for these instances alone) as the point is in the pool, and read
// back behind the rounds as the point is: nothing more of the vertex is live while the wave traverses.
template <bool STATS, int LT, bool BOUNCE, bool GROUPS = false, class PK = NoPick, class VC = ParkNone>
RT_DEV f3 vertex_pool(const DevScene& S, bool alive, bool bounceRay, Rng& g, f3 rayDir, uint32_t mesh, f3 hitNormal,
                      f3& point, f3& bdir, uint32_t* stack, uint32_t* pool, HitRec& next, bool& nextFound, LaneStats& st,
                      const LightGroupsRec* G = nullptr, GroupCols* gc = nullptr, PK pk = PK(), VC vc = VC()) {
  const bool bounce = BOUNCE && bounceRay;
  if constexpr (GROUPS) group_cols_zero(*gc);
  constexpr bool FR = (LT & LT_FASTDET) != 0;  // 1 / length by rtd::recip_fast (see rtd::unit3)
  const uint32_t lane = threadIdx.x & 63u, nl = loop_lights(S, pk);
  constexpr bool CP3 = (LT & LT_COMPACT3) != 0, CP2 = CP3 || (LT & LT_COMPACT2) != 0, CP = CP2 || (LT & LT_COMPACT) != 0;
  static_assert(!is_pick<PK> || !CP, "the picked frames' instances use the full pool layout: workers read directions, never a light");
  static_assert(VC::ROWS == 0 || !CP, "a surface that parks its value uses the full pool layout, with the parked rows behind it");
  using VP = VpLayout<CP3 ? 3 : CP2 ? 2 : CP ? 1 : 0>;
  float* fp = reinterpret_cast<float*>(pool);
  // 32 words: rank -> pixel lane (64 bytes) while rays are handed out; then rank -> victim
  // word while stealing (min(victims, free lanes) <= 32 entries)
  uint32_t* list = pool + VP::LIST;
  uint8_t* listB = reinterpret_cast<uint8_t*>(list);
  uint32_t* res = pool + VP::RES;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(pool + VP::KEY);
  const uint64_t amask = wave_ballot(alive);
  const uint32_t n = (uint32_t)__popcll(amask);
  f3 color = mk(0.f, 0.f, 0.f);
  nextFound = false;
  uint32_t gsave = 0;  // (LT_COMPACT3) this lane's engine state before its light draws
  if (n == 0) return color;
  PH(PH_VSETUP);
  PHC(PH_N_POOLS);
  if (alive) {
    if (!CP3) fp[VP_PT + lane] = point.x, fp[VP_PT + 64 + lane] = point.y, fp[VP_PT + 128 + lane] = point.z;
    if constexpr (VC::ROWS != 0) vc.store(lane);
    // draw order of the reference: the light samples in light order (Renderer.cpp:52),
    // then the hemisphere sample (Renderer.cpp:164)
    if (CP3) gsave = g.s;  // (the light samples are re-drawn from here wherever they are needed)
    for (uint32_t l = 0; l < nl; l++) {
      if (CP3) {
        g.next(), g.next();  // (light_sample_params' two engine calls)
      } else if (CP) {
        float rh, rv;
        light_sample_params(g, S.lights[l], rh, rv);
        fp[VP_DIR + (2 * l + 0) * 64 + lane] = rh, fp[VP_DIR + (2 * l + 1) * 64 + lane] = rv;
      } else {
        f3 tl;
        if constexpr (is_pick<PK>) tl = light_sample(g, loop_light(S, pk, l)) - point;
        else tl = light_sample(g, S.lights[l]) - point;
        fp[VP_DIR + (3 * l + 0) * 64 + lane] = tl.x, fp[VP_DIR + (3 * l + 1) * 64 + lane] = tl.y, fp[VP_DIR + (3 * l + 2) * 64 + lane] = tl.z;
      }
    }
    if (bounce) {
      // (the caller's copy is read back from the pool after the loop: `point` and the bounce
      // direction do not occupy registers while the wave traverses)
      const f3 bd = hemisphere_sample<FR>(g, hitNormal);
      if (CP2) bdir = bd;  // (stays in the caller's registers)
      else fp[VP::BDIR + lane] = bd.x, fp[VP::BDIR + 64 + lane] = bd.y, fp[VP::BDIR + 128 + lane] = bd.z;
      keys[lane] = ~0ull;
    }
    listB[lanes_below(amask)] = (uint8_t)lane;
    st.shadow += nl;
    if (bounce) st.closest++;
  }
  if (lane < 2 * POOL_L) res[lane] = 0;
  wave_sync();
  PH(PH_FILL);
  const uint32_t kinds = nl + (bounce ? 1u : 0u), R = n * kinds;
  uint32_t head = 0, myK = 0, myJ = 0;
  Trav<BOUNCE ? TRAV_MIXED : TRAV_ANY, LT, true> T;
  T.idle(stack);
  if constexpr (BOUNCE) T.sharedKey = keys, T.pj = 0;
  uint32_t* stackBase = stack - lane;
  if (!(LT & LT_NOPRIO)) __builtin_amdgcn_s_setprio(1);
  for (;;) {
    const uint64_t idle = wave_ballot(!T.live());
    const int nIdle = __popcll(idle);
    // a lane may be given a ray (hand-out) or a subtree of one (stealing); the ray is
    // started in ONE place below, so that the traversal state has a single definition
    // point per iteration (two start sites cost ~25 register copies per round)
    bool newRay = false, newShared = false;
    uint32_t newK = 0, newJ = 0;
    int32_t newNode = (LT & LT_Q8) ? (int32_t)rtbvh::kQ8RootOffset : 0;  // (the root's record)
    f3 dv = mk(0.f, 0.f, 0.f);  // (CP2) direction of the ray a thief joins, from the victim's registers
    if (CP2 && bounce && head == 0) {
      // first hand-out (every lane is free): each bounce ray to its own pixel lane, the first
      // shadow rays to the lanes without a vertex — the same 64 ranks as below, dealt differently
      if (alive) {
        newRay = true, newK = nl, newJ = lane;
      } else {
        const uint32_t r = n + lanes_below(~amask);
        if (r < R) {
          const uint32_t k = (r >= n) + (r >= 2 * n) + (r >= 3 * n);  // >= 1 here
          newRay = true, newK = k - 1u, newJ = listB[r - k * n];
        }
      }
      head = 64;
    } else if (head < R) {
      if (nIdle >= (int)S.refillT || nIdle == 64) {
        const uint32_t r = head + lanes_below(idle);
        if (!T.live() && r < R) {
          // the bounce rays (closest hit: the longest walks) are handed out first
          uint32_t k = (r >= n) + (r >= 2 * n) + (r >= 3 * n);  // r / n for kinds <= POOL_L + 1
          const uint32_t j = listB[r - k * n];
          k = bounce ? (k == 0 ? nl : k - 1) : k;
          newRay = true, newK = k, newJ = j;
        }
        head += (uint32_t)nIdle;
      }
      PH(PH_HANDOUT);
    } else if (nIdle >= (int)S.stealT) {
      // The pool is empty and many workers are free: the tail.  A few long rays would
      // now keep 64 lanes waiting (measured: 75 % of the rounds ran with 8 live lanes).
      // Free lanes take over the BOTTOM pending subtree of a busy lane's stack (the
      // farthest, usually largest one) and walk it for the same ray.  The victim's slot
      // is overwritten with TERM, which is what it must pop there anyway; any-hit rays
      // share one result bit, closest-hit rays one atomic-min key, so the outcome is
      // the one a single walker produces.
      // One steal event hands out up to four bottom entries per busy lane (pass p takes
      // every victim's next one), so that a single long ray with a deep stack refills the
      // wave at once instead of doubling its walkers round by round.  list16[slot] =
      // victim lane | entry index << 6; the thief fetches (kind, pixel lane) from the
      // victim's registers.
      uint16_t* list16 = reinterpret_cast<uint16_t*>(list);
      uint32_t given = 0;
      // entries this lane could hand over
      const int avail = T.live() ? T.depth() - T.stolen : 0;
      // (the passes only write the list; the lane's own state changes once, after them —
      // per-lane flags updated inside a loop with exits cost a dozen mask instructions per pass)
      int gave = 0;
      for (int pass = 0; pass < 4; pass++) {
        const bool canGive = avail > pass;
        const uint64_t vmask = wave_ballot(canGive);
        if (vmask == 0 || given >= (uint32_t)nIdle) break;
        const uint32_t slot = given + lanes_below(vmask);
        const bool gives = canGive && slot < (uint32_t)nIdle;
        if (gives) list16[slot] = (uint16_t)(lane | ((uint32_t)(T.stolen + pass) << 6));
        gave += gives ? 1 : 0;
        given += (uint32_t)__popcll(vmask);
      }
      if (gave) {
        if constexpr (BOUNCE) {
          if (!T.shared && !T.anyHit && T.found) T.publish();  // what it has found so far
        }
        T.shared = true;
        T.stolen += gave;
      }
      if (given != 0) {
        given = given < (uint32_t)nIdle ? given : (uint32_t)nIdle;
        wave_sync();
        const uint32_t q = lanes_below(idle);
        const bool thief = !T.live() && q < given;
        const uint32_t w = thief ? (uint32_t)list16[q] : lane;
        const uint32_t v = w & 63u, e = w >> 6;
        const uint32_t kj = (uint32_t)__shfl((int)(myK | (myJ << 8)), (int)v, 64);  // (all lanes take part)
        if (CP2 && BOUNCE) dv = mk(__shfl(T.d.x, (int)v, 64), __shfl(T.d.y, (int)v, 64), __shfl(T.d.z, (int)v, 64));
        if (thief) {
          uint32_t* slot = stackBase + (e + 1u) * BLOCK + v;  // (row 0 is the sentinel)
          newNode = (int32_t)*slot;
          *slot = (uint32_t)TERM;
          newRay = true, newShared = true, newK = kj & 255u, newJ = kj >> 8;
        }
        wave_sync();
      }
      PH(PH_STEAL);
    }
    const uint32_t gsj = CP3 ? (uint32_t)__shfl((int)gsave, (int)newJ, 64) : 0u;  // (all lanes take part)
    const f3 pj3 = CP3 ? mk(__shfl(point.x, (int)newJ, 64), __shfl(point.y, (int)newJ, 64), __shfl(point.z, (int)newJ, 64)) : mk(0.f, 0.f, 0.f);
    if (newRay) {
      const f3 pj = CP3 ? pj3 : mk(fp[VP_PT + newJ], fp[VP_PT + 64 + newJ], fp[VP_PT + 128 + newJ]);
      f3 dj;
      if (CP) {
        if (!BOUNCE || newK < nl) {  // rebuild the direction from the light sample's two parameters
          const rt_light& Lt = S.lights[newK];
          float rh, rv;
          if (CP3) {  // ... which are re-drawn: the pixel lane's engine state before its light draws, 2 calls per earlier light
            Rng t{gsj};
            for (uint32_t q = 0; q < 2u * newK; ++q) t.next();
            light_sample_params(t, Lt, rh, rv);
          } else {
            rh = fp[VP_DIR + (2 * newK + 0) * 64 + newJ], rv = fp[VP_DIR + (2 * newK + 1) * 64 + newJ];
          }
          dj = light_point(Lt, rh, rv) - pj;
        } else if (CP2) {
          dj = newShared ? dv : bdir;  // a bounce ray: stolen (the victim's direction) or this lane's own
        } else {
          dj = mk(fp[VP::BDIR + newJ], fp[VP::BDIR + 64 + newJ], fp[VP::BDIR + 128 + newJ]);
        }
      } else {
        const uint32_t src = !BOUNCE || newK < nl ? VP_DIR + 192 * newK : VP::BDIR;
        dj = mk(fp[src + newJ], fp[src + 64 + newJ], fp[src + 128 + newJ]);
      }
      T.start(pj, dj, S.invBoxScale);
      if (T.live()) T.cur = newNode;  // (a NaN ray stays dead)
      if constexpr (BOUNCE) T.anyHit = newK < nl, T.pj = newJ;
      T.shared = newShared;
      myK = newK, myJ = newJ;
    }
    if (wave_ballot(T.live()) == 0) break;
    // Rounds until enough lanes are free for the next hand-out or steal (the same
    // thresholds as above, so the schedule is the one a check per round gives — without
    // walking through the bookkeeping in the rounds where it cannot do anything)
    const int need = min(64, head < R ? (int)S.refillT : (int)S.stealT);
    for (;;) {
      if (T.shared && T.live()) {
        // several lanes may now serve this ray: stop at a decided any-hit
        // ray, prune with the closest hit anyone has found so far
        if (!BOUNCE || T.anyHit) {
          if ((res[myK * 2 + (myJ >> 5)] >> (myJ & 31)) & 1u) T.cur = TERM;
        } else {
          T.refresh_best();
        }
      }
      const bool was = T.live();
      PH(PH_POOLMISC);
      if (head >= R) PHC(PH_TAIL);
      T.template round<STATS>(S, st);
      if (was && !T.live() && T.found) {
        if (!BOUNCE || myK < nl) atomicOr(&res[myK * 2 + (myJ >> 5)], 1u << (myJ & 31));
        else if (!T.shared) T.publish();  // shared rays publish every improvement as it happens
      }
      if (__popcll(wave_ballot(!T.live())) >= need) break;
    }
  }
  if (!(LT & LT_NOPRIO)) __builtin_amdgcn_s_setprio(0);
  wave_sync();
  PH(PH_POOLMISC);
  // `point` and the bounce direction come back from the pool (the same bits; lanes without a
  // vertex read stale words nobody uses): nothing of them is live while the wave traverses
  const f3 pt = CP3 ? point : mk(fp[VP_PT + lane], fp[VP_PT + 64 + lane], fp[VP_PT + 128 + lane]);
  point = pt;
  if (bounce && !CP2) bdir = mk(fp[VP::BDIR + lane], fp[VP::BDIR + 64 + lane], fp[VP::BDIR + 128 + lane]);
  if (alive) {
    BsdfBase base = bsdf_base<FR>(S.matsDev[mesh], hitNormal, -rayDir);  // the light-independent half, once
    if constexpr (VC::ROWS != 0) {  // (in place of the mesh's)
      if constexpr (VC::WHOLE) base = bsdf_base<FR>(vc.load(lane), hitNormal, -rayDir);
      else base.kdDiffuse = vc.load(lane);
    }
    Rng relight{gsave};
    for (uint32_t l = 0; l < nl; l++) {
      float rh3 = 0.f, rv3 = 0.f;
      if (CP3) light_sample_params(relight, S.lights[l], rh3, rv3);  // (every light: the stream moves on whether it is occluded or not)
      if ((res[l * 2 + (lane >> 5)] >> (lane & 31)) & 1u) continue;  // occluded (Renderer.cpp:54-55)
      const f3 toLight = CP3 ? light_point(S.lights[l], rh3, rv3) - pt
                         : CP ? light_point(S.lights[l], fp[VP_DIR + (2 * l + 0) * 64 + lane], fp[VP_DIR + (2 * l + 1) * 64 + lane]) - pt
                              : mk(fp[VP_DIR + (3 * l + 0) * 64 + lane], fp[VP_DIR + (3 * l + 1) * 64 + lane], fp[VP_DIR + (3 * l + 2) * 64 + lane]);
      const f3 bsdf = bsdf_apply<FR>(base, toLight);
      f3 radiance;
      if constexpr (is_pick<PK>) radiance = light_eval(loop_light(S, pk, l), pt);
      else radiance = light_eval(S.lights[l], pt);
      if constexpr (GROUPS) group_cols_add(*gc, *G, l, radiance * bsdf);
      else color = color + radiance * bsdf;
    }
    if (bounce) {
      const unsigned long long key = keys[lane];
      nextFound = key != ~0ull;
      next.t = __uint_as_float((uint32_t)(key >> 32)), next.id = (uint32_t)key;
      next.u = next.v = 0.f, next.mesh = 0u;  // vertex_setup_ray works from the id
    }
  }
  wave_sync();  // the pool is rewritten by the next vertex
  PH(PH_BSDF);
  return color;
}

RT_DEV uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

RT_DEV void flush_stats(const LaneStats& st, unsigned long long* counters, bool stats) {
  const uint32_t c = wave_sum(st.closest), s = wave_sum(st.shadow), q = wave_sum(st.knn);
  uint32_t n = 0, t = 0, kd = 0;
  uint32_t wn = 0, wl = 0;
  uint32_t lw = 0, li = 0, fr = 0;
  if (stats) fr = wave_sum(st.frames), n = wave_sum(st.nodes), t = wave_sum(st.tris), kd = wave_sum(st.kd), wn = wave_sum(st.wnode), wl = wave_sum(st.wleaf), lw = wave_sum(st.lwait), li = wave_sum(st.lidle);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counters[RTK_CNT_CLOSEST], (unsigned long long)c);
    atomicAdd(&counters[RTK_CNT_SHADOW], (unsigned long long)s);
    if (q) atomicAdd(&counters[RTK_CNT_KNN], (unsigned long long)q);
    if (stats) {
      atomicAdd(&counters[RTK_CNT_NODES], (unsigned long long)n);
      atomicAdd(&counters[RTK_CNT_TRIS], (unsigned long long)t);
      if (kd) atomicAdd(&counters[RTK_CNT_KD], (unsigned long long)kd);
      atomicAdd(&counters[RTK_CNT_WNODE], (unsigned long long)wn);
      atomicAdd(&counters[RTK_CNT_WLEAF], (unsigned long long)wl);
      atomicAdd(&counters[RTK_CNT_LWAIT], (unsigned long long)lw);
      atomicAdd(&counters[RTK_CNT_LIDLE], (unsigned long long)li);
      if (fr) atomicAdd(&counters[RTK_CNT_FRAMES], (unsigned long long)fr);
    }
  }
}

// The same for the one-wave-per-workgroup kernels, whose frames have up to hundreds of thousands of waves: the three
// ray / query counts go to 1,024 striped slots behind the counter block (counters + RTK_CNT_COUNT: [1024][4]) and
// k_fold_stripes adds them up after the kernel — 262 k waves adding to ONE address each spent 4 of the photon frame's
// 17 ms queueing at the memory side (same-address atomics serialise there).
RT_DEV void flush_stats_striped(const LaneStats& st, unsigned long long* counters) {
  const uint32_t c = wave_sum(st.closest), s = wave_sum(st.shadow), q = wave_sum(st.knn);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* stripe = counters + RTK_CNT_COUNT + 4u * (blockIdx.x & 1023u);
    if (c) atomicAdd(&stripe[0], (unsigned long long)c);
    if (s) atomicAdd(&stripe[1], (unsigned long long)s);
    if (q) atomicAdd(&stripe[2], (unsigned long long)q);
  }
}
__global__ __launch_bounds__(1024) void k_fold_stripes(unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long sh[3][16];
  unsigned long long* stripe = counters + RTK_CNT_COUNT + 4u * threadIdx.x;
  unsigned long long v[3] = {stripe[0], stripe[1], stripe[2]};
  stripe[0] = stripe[1] = stripe[2] = 0;  // ready for the next launch
  for (int j = 0; j < 3; ++j) {
    for (int off = 32; off > 0; off >>= 1) v[j] += __shfl_xor(v[j], off, 64);
    if ((threadIdx.x & 63u) == 0) sh[j][threadIdx.x >> 6] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
    for (int i = 0; i < 16; i++) t += sh[threadIdx.x][i];
    const int which = threadIdx.x == 0 ? RTK_CNT_CLOSEST : threadIdx.x == 1 ? RTK_CNT_SHADOW : RTK_CNT_KNN;
    if (t) atomicAdd(&counters[which], t);
  }
}

// [levels][64] stack, then (photon variants) [k][64] heap distances and [k][64] heap ids
template <bool PHOTON>
RT_DEV Lds carve_lds(uint32_t* base, uint32_t levels = STACK, uint32_t kslots = KMAX) {
  Lds L;
  L.stack = base + (threadIdx.x & 63u);
  L.heap = PHOTON ? reinterpret_cast<uint2*>(base + levels * BLOCK) + (threadIdx.x & 63u) : nullptr;
  return L;
}

// ---------------------------------------------------------------- integrate
// Renderer::render's per-sample body (Renderer.cpp:227-258) + calculateColorRay /
// calculateColorPath (:106-201) with the recursion unrolled to a loop.  Control
// flow is wave-uniform (per-lane `alive` flags instead of early exits) because the
// direct-lighting step exchanges rays between lanes through LDS.
// One wave tile: lane = (pixel pl of the tile, sample slot sj).  The wave integrates
// S = 1 << sshift consecutive samples of P = 64 >> sshift pixels side by side.

// The primary ray of a sample through a thin lens (rt_amd.h, rt_render_lens; R.aperture > 0): from a point of the lens
// disc, drawn by rejection from a stream of its own, through the point where the pinhole ray of (u, v) meets the plane
// of focus.  Float32, nothing fused; the direction by the division and the square root (rt_render_rays' rule).
RT_DEV void lens_ray(const rt_camera& c, const LensRec& R, uint32_t lensSeed, float u, float v, f3& o, f3& d) {
  const f3 pos = ld(c.position);
  const f3 q = ld(c.lower_left) + u * ld(c.horizontal) + v * ld(c.vertical) - pos;  // camera_ray's operand
  const f3 F = pos + R.fs * q;
  Rng e{lensSeed};
  float lx = 0.f, ly = 0.f;
  for (int t = 0; t < 32; ++t) {  // (a pair is accepted with probability pi / 4)
    const float x = e.uniformF(-1.f, 1.f);
    const float y = e.uniformF(-1.f, 1.f);
    if (x * x + y * y <= 1.f) {
      lx = x, ly = y;
      break;
    }
  }
  o = (pos + (R.aperture * lx) * ld(R.hu)) + (R.aperture * ly) * ld(R.vu);
  d = unit3(F - o);
}

// The primary ray of a sample under an open shutter (rt_amd.h, rt_render_shutter): the sample's time t from a stream of
// its own, its camera c + t D in registers, then the dividing camera_ray on that camera or, with a lens, lens_ray with
// the axes and the focus scale of that time.  Float32, nothing fused.  t, the camera and the engine die here.
RT_DEV void shutter_ray(const rt_camera& c, const ShutterRec& R, uint32_t seed, uint32_t pix, uint32_t i, float u, float v,
                        f3& o, f3& d) {
  Rng e{rt_stream_seed(seed, RT_STREAM_SHUTTER, pix, i)};
  const float t = e.uniformF(R.open, R.close);
  rt_camera ct;
  for (int k = 0; k < 3; ++k) {
    ct.position[k] = c.position[k] + t * R.d[k];
    ct.lower_left[k] = c.lower_left[k] + t * R.d[3 + k];
    ct.horizontal[k] = c.horizontal[k] + t * R.d[6 + k];
    ct.vertical[k] = c.vertical[k] + t * R.d[9 + k];
  }
  // (wave-uniform: the record is a kernel argument)
  if (R.aperture > 0.f) {
    LensRec l;
    l.aperture = R.aperture, l.fs = R.fs0 + t * R.dfs;
    const f3 hu = unit3(ld(ct.horizontal)), vu = unit3(ld(ct.vertical));
    l.hu[0] = hu.x, l.hu[1] = hu.y, l.hu[2] = hu.z;
    l.vu[0] = vu.x, l.vu[1] = vu.y, l.vu[2] = vu.z;
    lens_ray(ct, l, rt_stream_seed(seed, RT_STREAM_LENS, pix, i), u, v, o, d);
  } else camera_ray<false>(ct, u, v, o, d);
}

// (LT_LIGHTS) One sample group of a frame split by light group into the accumulator: per group g < G.n the sample is
// c0[g] + (c1[g] + (c2[g] + 0)), clamped, and the pixel's owner lane adds the wave's samples in sample order into slice g
// (accum + g * width * height), with the hit count into .w — render_tile's own adds, once per slice.  The hand-over area
// is (3 RT_LIGHT_GROUPS_MAX + 1) rows of ex: the colours of group g in rows 3 g .. 3 g + 2, the hit flag in the last.  The
// owner reads its pixel of a slice, adds and writes it back here, per sample group, instead of carrying G float4 sums
// across the vertex pools: the same float32 adds in the same order, one 16-byte load and store per slice.
constexpr int LG_EX_ROWS = 3 * RT_LIGHT_GROUPS_MAX + 1;
RT_DEV void group_samples_add(const RenderArgs& A, const LightGroupsRec& G, float4* __restrict__ accum, float* ex, const GroupCols& g0,
                              const GroupCols& g1, const GroupCols& g2, bool primary, bool active, bool owner, uint32_t pix,
                              uint32_t pl, uint32_t base) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t S_ = 1u << A.sshift, P_ = 64u >> A.sshift;
  const size_t slice = (size_t)A.width * A.height;
  constexpr int HIT = 3 * RT_LIGHT_GROUPS_MAX * 64;
  if (A.sshift == 0) {
#pragma unroll
    for (int g = 0; g < RT_LIGHT_GROUPS_MAX; ++g) {
      if ((uint32_t)g < G.n && active) {
        const f3 total = g0.c[g] + (g1.c[g] + (g2.c[g] + mk(0.f, 0.f, 0.f)));
        float4 s = accum[g * slice + pix];
        s.x += clamp01(total.x), s.y += clamp01(total.y), s.z += clamp01(total.z);
        if (primary) s.w += 1.f;
        accum[g * slice + pix] = s;
      }
    }
    return;
  }
#pragma unroll
  for (int g = 0; g < RT_LIGHT_GROUPS_MAX; ++g) {
    if ((uint32_t)g < G.n) {
      const f3 total = g0.c[g] + (g1.c[g] + (g2.c[g] + mk(0.f, 0.f, 0.f)));
      ex[(3 * g + 0) * 64 + lane] = clamp01(total.x), ex[(3 * g + 1) * 64 + lane] = clamp01(total.y), ex[(3 * g + 2) * 64 + lane] = clamp01(total.z);
    }
  }
  ex[HIT + lane] = primary ? 1.f : 0.f;
  wave_sync();
  if (owner) {
    const uint32_t cnt = A.s1 - base < S_ ? A.s1 - base : S_;
#pragma unroll
    for (int g = 0; g < RT_LIGHT_GROUPS_MAX; ++g) {
      if ((uint32_t)g < G.n) {
        float4 s = accum[g * slice + pix];
        for (uint32_t jj = 0; jj < cnt; jj++) {
          const uint32_t q = jj * P_ + pl;
          s.x += ex[(3 * g + 0) * 64 + q], s.y += ex[(3 * g + 1) * 64 + q], s.z += ex[(3 * g + 2) * 64 + q];
          s.w += ex[HIT + q];  // adds 1.0 or an exact 0.0
        }
        accum[g * slice + pix] = s;
      }
    }
  }
  wave_sync();
}

// The record a frame variant's instances take as a kernel argument of their own, by its LT_* bits: the lens, the shutter
// of a single-view frame (a multi-view one reads its records from RenderArgs' tables), the light groups, the light
// picks — or, whatever the generator, the surface's (surface_t<LTV>::Rec) — or none.  park: the wave's parked rows of
// LDS (surface_t<LTV>::Parked::ROWS of them), from the kernel that lays its LDS out.
template <int LTV>
using frame_rec_t = std::conditional_t<(LTV & LT_LENS) != 0, LensRec,
                    std::conditional_t<(LTV & LT_LIGHTS) != 0, LightGroupsRec,
                    std::conditional_t<(LTV & LT_PICK) != 0, PickRec,
                    std::conditional_t<surface_t<LTV>::LT != 0, typename surface_t<LTV>::Rec,
                    std::conditional_t<(LTV & LT_SHUTTER) != 0 && (LTV & LT_VIEWS) == 0, ShutterRec, NoRec>>>>>;
// (what the instances without a record leave out; the others do not compile without theirs)
template <int LTV>
constexpr const frame_rec_t<LTV>* no_record() {
  static_assert(std::is_same_v<frame_rec_t<LTV>, NoRec>, "this variant's instances pass their record to render_tile");
  return nullptr;
}

// FINE (k_render_persist's plain single-view instances): the list may end in a fine tail (RenderArgs::fineFrom), whose items
// take their samples per wave and their footprint from A.sshiftFine: wave-uniform values, read once per item here.
template <bool BRUTE, bool PHOTON, bool POOLED, bool STATS, int LTV, class HP = Heap, bool FINE = false>
RT_DEV void render_tile(const DevScene& S, const RenderArgs& A, float4* __restrict__ accum, const Lds& L, uint32_t* pool,
                        float* ex, uint32_t wave, LaneStats& st, const frame_rec_t<LTV>* rec = no_record<LTV>(),
                        float* park = nullptr) {
  constexpr int LT = LTV & ~(LT_VIEWS | LT_LENS | LT_SHUTTER | LT_LIGHTS | LT_PICK | LT_SURFACES);
  constexpr bool VIEWS = (LTV & LT_VIEWS) != 0;
  constexpr bool LENS = (LTV & LT_LENS) != 0;
  constexpr bool SHUTTER = (LTV & LT_SHUTTER) != 0;
  constexpr bool LIGHTS = (LTV & LT_LIGHTS) != 0;
  constexpr bool PICK = (LTV & LT_PICK) != 0;
  constexpr bool VCOL = (LTV & LT_VCOL) != 0;
  constexpr bool TEX = (LTV & LT_TEX) != 0;
  constexpr bool MAT = (LTV & LT_MAT) != 0;
  constexpr bool NMAP = (LTV & LT_NMAP) != 0;
  // (the surface side and the camera side are orthogonal — below, the surface is SF alone and meets the generator
  // nowhere: a record of colours or textures goes with the plain generator or with the multi-view shutter's, the general
  // camera form, whose tables come from RenderArgs)
  using SF = surface_t<LTV>;
  using PV = typename SF::Parked;
  static_assert(!VCOL || (VIEWS == SHUTTER && !LENS && !LIGHTS && !PICK && !PHOTON), "vertex colours go with the plain frame or the multi-view shutter frame");
  static_assert(!TEX || (VIEWS == SHUTTER && !LENS && !LIGHTS && !PICK && !VCOL && !PHOTON), "textures go with the plain frame or the multi-view shutter frame");
  static_assert(!MAT || (!VIEWS && !LENS && !SHUTTER && !LIGHTS && !PICK && !VCOL && !TEX && !PHOTON), "material maps go with the plain frame only");
  static_assert(!NMAP || (!VIEWS && !LENS && !SHUTTER && !LIGHTS && !PICK && !VCOL && !TEX && !MAT && !PHOTON), "normal maps go with the plain frame only");
  static_assert(!LIGHTS || (!VIEWS && !LENS && !SHUTTER && !PHOTON), "light groups go with the plain frame only");
  static_assert(!PICK || (!VIEWS && !LENS && !SHUTTER && !LIGHTS && !PHOTON), "light picks go with the plain frame only");
  static_assert(!LENS || !VIEWS, "no multi-view lens frames");
  static_assert(!SHUTTER || !LENS, "the shutter's lens is its own: LT_SHUTTER does not go with LT_LENS");
  constexpr bool FR = (LT & LT_FASTDET) != 0;  // 1 / length by rtd::recip_fast (see rtd::unit3)
  const uint32_t lane = threadIdx.x & 63u;
  // lane = (pixel pl of the wave tile, sample slot sj): the wave integrates
  // S = 1 << sshift consecutive samples of P = 64 >> sshift pixels side by side
  const uint32_t tile = A.tiles[wave];
  // A multi-view frame: the tile's view picks the camera, the stream key and the accumulator slice.  `wave` is wave-
  // uniform (a block index, or readfirstlane of the tile counter), so the view index and its record are read with scalar
  // loads through the constant address space and stay in SGPRs.
  // (single-view instances read S.cam and A.seed as they always did)
  rt_camera cam;
  uint32_t seed = A.seed;
  ShutterRec vsh;  // (LT_VIEWS | LT_SHUTTER) the view's shutter record, from the table parallel to views, in SGPRs too
  if constexpr (VIEWS) {
    typedef const __attribute__((address_space(4))) uint32_t* const_u32_ptr;
    typedef const __attribute__((address_space(4))) ViewRec* const_view_ptr;
    typedef const __attribute__((address_space(4))) ViewShutterRec* const_shutter_ptr;
    const uint32_t view = ((const_u32_ptr)A.tileView)[wave];
    const const_view_ptr R = (const_view_ptr)A.views + view;
    for (int j = 0; j < 3; ++j)
      cam.position[j] = R->cam.position[j], cam.lower_left[j] = R->cam.lower_left[j],
      cam.horizontal[j] = R->cam.horizontal[j], cam.vertical[j] = R->cam.vertical[j];
    seed = R->seed;
    accum += R->accumOff;
    if constexpr (SHUTTER) {
      const const_shutter_ptr Q = (const_shutter_ptr)A.viewShutters + view;
      for (int j = 0; j < 12; ++j) vsh.d[j] = Q->d[j];
      vsh.open = Q->open, vsh.close = Q->close, vsh.aperture = Q->aperture, vsh.fs0 = Q->fs0, vsh.dfs = Q->dfs;
    }
  }
  uint32_t sshift = A.sshift, tileW = A.tileW;
  if constexpr (FINE) {
    static_assert(POOLED && LTV == LT, "the fine tail goes with the plain pooled frame only");
    if (wave >= A.fineFrom) {
      // (the footprints of rt_api.cpp wave_tile_shape: 8, 8, 4, 4, 2, 2, 1 pixels wide)
      sshift = A.sshiftFine, tileW = 8u >> (A.sshiftFine >> 1);
    }
  }
  const uint32_t S_ = 1u << sshift, P_ = 64u >> sshift;
  const uint32_t pl = lane & (P_ - 1u), sj = lane >> (6u - sshift);
  const uint32_t wsh = (uint32_t)__builtin_ctz(tileW);
  const uint32_t px = (tile & 0xffffu) + (pl & (tileW - 1u)), py = (tile >> 16) + (pl >> wsh);
  const bool inImage = px < A.width && py < A.height;
  const bool owner = inImage && sj == 0;  // adds this pixel's samples, in order
  const uint32_t pix = inImage ? py * A.width + px : 0u;
  float4 sum = owner ? accum[pix] : make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr bool pooled = POOLED;  // chosen by the launcher: BVH, direct lighting, n_lights <= POOL_L
  const int nvert = A.mode == RT_MODE_PATH ? (int)A.max_depth : 1;
  for (uint32_t base = A.s0; base < A.s1; base += S_) {
    const uint32_t i = base + sj;
    const bool active = inImage && i < A.s1;
    Rng g{rt_stream_seed(VIEWS ? seed : A.seed, RT_STREAM_PIXEL, pix, i)};
    float sx, sy;
    jitter_sample(g, (int)i, (int)A.spp, sx, sy);
    f3 o, d;
    const float cu = ((float)px + sx) / (float)A.width, cv = 1.f - ((float)py + sy) / (float)A.height;
    if constexpr (VIEWS && SHUTTER) shutter_ray(cam, vsh, seed, pix, i, cu, cv, o, d);
    else if constexpr (VIEWS) camera_ray<FR>(cam, cu, cv, o, d);
    else if constexpr (LENS) {
      // (wave-uniform: the record is a kernel argument)
      if (rec->aperture > 0.f) lens_ray(S.cam, *rec, rt_stream_seed(A.seed, RT_STREAM_LENS, pix, i), cu, cv, o, d);
      else camera_ray<FR>(S.cam, cu, cv, o, d);
    } else if constexpr (SHUTTER) shutter_ray(S.cam, *rec, A.seed, pix, i, cu, cv, o, d);
    else camera_ray<FR>(S.cam, cu, cv, o, d);
    f3 c0 = mk(0.f, 0.f, 0.f), c1 = c0, c2 = c0;
    GroupCols g0, g1, g2, gv;  // (LT_LIGHTS) the three vertices' colours per group, and the current vertex's
    if constexpr (LIGHTS) group_cols_zero(g0), group_cols_zero(g1), group_cols_zero(g2);
    bool primary = true, alive = active;
    // (LT_PICK) the sample's light indices: drawn once, before the primary cast, for all of its vertices
    Picks pk{0u, 0u, 0u};
    if constexpr (PICK) pk = draw_picks(*rec, A.seed, pix, i);
    if constexpr (pooled) {
      // primary ray (coherent: traced in lock step), then one pool per vertex
      HitRec h;
      if (alive) st.closest++;
      const bool hit0 = cast<false, false, STATS, LT>(S, alive, o, d, L.stack, h, st);
      if (alive && !hit0) primary = false, alive = false;
      for (int depth = 0; depth < nvert; depth++) {
        if (wave_ballot(alive) == 0) break;
        const bool bounce = A.mode == RT_MODE_PATH && depth + 1 < nvert;  // wave-uniform
        f3 nrm = mk(0.f, 0.f, 0.f), pt = nrm, bdir = nrm;
        uint32_t mesh = 0;
        PV sf;  // the vertex's surface value (zero without a vertex) with the wave's rows; ParkNone: empty
        if constexpr (PV::ROWS != 0) sf = PV{{}, park};
        // (the vertex set-up is three dependent loads deep: it goes out ahead of other waves'
        // arithmetic, like the pool loop that follows; +0.4 % on C2)
        if (!(LT & LT_NOPRIO)) __builtin_amdgcn_s_setprio(1);
        if constexpr (PV::ROWS != 0) {
          if (alive) {
            uint4 tv;
            float u, v;
            [[maybe_unused]] f3 e1, e2;  // (a surface that bends the normal: the triangle's edges, from the same loads)
            if constexpr (SF::BENDS) vertex_setup_ray<FR>(S, h.id, o, d, nrm, pt, tv, u, v, e1, e2);
            else vertex_setup_ray<FR>(S, h.id, o, d, nrm, pt, tv, u, v);
            mesh = tv.w, sf.v = SF::form(S, *rec, tv, u, v);
            // (the bent normal replaces the interpolated one here, before the pool's light terms, its BSDF half and its
            // hemisphere sample see nrm; only nrm survives the set-up)
            if constexpr (SF::BENDS) nrm = SF::bend(*rec, tv, u, v, e1, e2, nrm);
          }
        } else
        if (alive) vertex_setup_ray<FR>(S, h.id, o, d, nrm, pt, mesh);
        // (Renderer.cpp:164: the hemisphere sample is drawn after every shaded vertex;
        // after the LAST one the reference draws it too but never traces it, and the
        // stream ends there — the pool only draws it when a bounce ray follows)
        HitRec nh;
        bool nfound;
        // A pool without a bounce ray holds any-hit rays only and runs the body compiled for that — in the instances
        // with the whole tree in LDS (LT_ALL: plan_persist's class of the small scenes, whose frames are bound by
        // instruction issue).  In the other instances (a partial top, trees in HBM / L2, the compact pools) the
        // second body costs the timed kernels registers they do not have: `<false, 257>` and `<false, 280>` spill
        // with it where they have no scratch without, `k_render_persist5<false, 328>` spills more; they keep the
        // general body alone.
        constexpr bool SHADOW_BODY = (LT & 3) == LT_ALL;
        f3 c;
        if constexpr (LIGHTS) {
          static_assert(!SHADOW_BODY, "the light-group instances keep their trees in HBM / L2");
          c = vertex_pool<STATS, LT, true, true>(S, alive, bounce, g, d, mesh, nrm, pt, bdir, L.stack, pool, nh, nfound, st, rec, &gv);
        } else if constexpr (PICK) {
          static_assert(!SHADOW_BODY, "the light-pick instances keep their trees in HBM / L2");
          c = vertex_pool<STATS, LT, true, false, PickArgs>(S, alive, bounce, g, d, mesh, nrm, pt, bdir, L.stack, pool, nh, nfound, st, nullptr, nullptr, PickArgs{rec, pk});
        } else if constexpr (PV::ROWS != 0) {
          static_assert(!SHADOW_BODY, "the instances with a surface keep their trees in HBM / L2");
          c = vertex_pool<STATS, LT, true, false, NoPick, PV>(S, alive, bounce, g, d, mesh, nrm, pt, bdir, L.stack, pool, nh, nfound, st, nullptr, nullptr, NoPick(), sf);
        } else
        c = SHADOW_BODY && !bounce
                         ? vertex_pool<STATS, LT, false>(S, alive, false, g, d, mesh, nrm, pt, bdir, L.stack, pool, nh, nfound, st)
                         : vertex_pool<STATS, LT, true>(S, alive, bounce, g, d, mesh, nrm, pt, bdir, L.stack, pool, nh, nfound, st);
        if (alive) {
          if (depth == 0) c0 = c;
          else if (depth == 1) c1 = c;
          else c2 = c;
          if constexpr (LIGHTS) {
            if (depth == 0) g0 = gv;
            else if (depth == 1) g1 = gv;
            else g2 = gv;
          }
          o = pt, d = bdir, h = nh;
          if (!nfound) alive = false;
        }
      }
    } else
    for (int depth = 0; depth < nvert; depth++) {
      HitRec h;
      if (alive) st.closest++;
      const bool hitv = cast<BRUTE, false, STATS>(S, alive, o, d, L.stack, h, st);
      if (alive && !hitv) {
        if (depth == 0) primary = false;
        alive = false;
      }
      if (wave_ballot(alive) == 0) break;
      f3 nrm = mk(0.f, 0.f, 0.f), pt = nrm, c = nrm;
      if (alive) vertex_setup<FR>(S, h, nrm, pt);
      if constexpr (SF::BENDS) {
        // (before shade_direct_seq and the hemisphere sample below read nrm; the positions are vertex_setup's loads)
        if (alive) {
          const uint4 tv = S.triShade[h.id];
          const f3 p0 = ld(S.vpos + 3 * (size_t)tv.x), p1 = ld(S.vpos + 3 * (size_t)tv.y), p2 = ld(S.vpos + 3 * (size_t)tv.z);
          nrm = SF::bend(*rec, tv, h.u, h.v, p1 - p0, p2 - p0, nrm);
        }
      }
      if (PHOTON) {
        if (alive) c = shade_photon<STATS, HP>(S, A, d, h, L, nrm, pt, st);
      } else if constexpr (LIGHTS) {
        if (alive) c = shade_direct_seq<BRUTE, STATS, true>(S, g, d, h, L.stack, nrm, pt, st, rec, &gv);
      } else if constexpr (PICK) {
        if (alive) c = shade_direct_seq<BRUTE, STATS, false, PickArgs>(S, g, d, h, L.stack, nrm, pt, st, nullptr, nullptr, PickArgs{rec, pk});
      } else if constexpr (PV::ROWS != 0) {
        if (alive)
          c = shade_direct_seq<BRUTE, STATS, false, NoPick, PV>(S, g, d, h, L.stack, nrm, pt, st, nullptr, nullptr, NoPick(),
                                                                PV{SF::form(S, *rec, S.triShade[h.id], h.u, h.v), park});
      } else {
        if (alive) c = shade_direct_seq<BRUTE, STATS>(S, g, d, h, L.stack, nrm, pt, st);
      }
      if (alive) {
        if (depth == 0) c0 = c;
        else if (depth == 1) c1 = c;
        else c2 = c;
        if constexpr (LIGHTS) {
          if (depth == 0) g0 = gv;
          else if (depth == 1) g1 = gv;
          else g2 = gv;
        }
      }
      if (A.mode != RT_MODE_PATH) break;
      if (alive) {
        d = hemisphere_sample(g, nrm);  // drawn after every shaded vertex (Renderer.cpp:164)
        o = pt;
      }
    }
    // calculateColorPath returns c0 + (c1 + (c2 + 0)) for finalDepth <= 3
    PH(PH_VSETUP);
    if constexpr (LIGHTS) {
      group_samples_add(A, *rec, accum, ex, g0, g1, g2, primary, active, owner, pix, pl, base);
      continue;
    }
    const f3 total = c0 + (c1 + (c2 + mk(0.f, 0.f, 0.f)));
    const float r0 = clamp01(total.x), r1 = clamp01(total.y), r2 = clamp01(total.z);
    if (sshift == 0) {
      if (active) {
        sum.x += r0, sum.y += r1, sum.z += r2;
        if (primary) sum.w += 1.f;
      }
    } else {
      // hand the sample to the pixel's owner lane, which adds samples base.. in order
      // (Renderer.cpp:258: updateImage += colorResponse, i = 0..N-1)
      ex[lane] = r0, ex[64 + lane] = r1, ex[128 + lane] = r2, ex[192 + lane] = primary ? 1.f : 0.f;
      wave_sync();
      if (owner) {
        const uint32_t cnt = A.s1 - base < S_ ? A.s1 - base : S_;
        for (uint32_t jj = 0; jj < cnt; jj++) {
          const uint32_t q = jj * P_ + pl;
          sum.x += ex[q], sum.y += ex[64 + q], sum.z += ex[128 + q];
          sum.w += ex[192 + q];  // adds 1.0 or an exact 0.0
        }
      }
      wave_sync();
    }
    PH(PH_ACCUM);
  }
  if constexpr (LIGHTS) return;  // (group_samples_add has written every slice)
  if (owner) accum[pix] = sum;
}

template <bool BRUTE, bool PHOTON, bool POOLED, bool STATS, int MINW, int LTV = LT_NONE>
__global__ __launch_bounds__(BLOCK, MINW) void k_render(DevScene S, RenderArgs A, float4* __restrict__ accum,
                                                  unsigned long long* __restrict__ counters) {
  static_assert(BLOCK == 64, "one wave per workgroup");
  static_assert(!POOLED || (!BRUTE && !PHOTON), "the vertex pool serves BVH direct lighting");
  // dynamic LDS (render_lds_bytes): [levels][64] traversal stack, sized from the
  // depth of THIS scene's trees so that LDS does not cap occupancy; then the photon
  // k-heap or the shadow-ray pool
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<PHOTON>(lds, A.stackLevels, A.k);
  uint32_t* pool = lds + (A.stackLevels + (PHOTON ? 2 * A.k : 0)) * BLOCK;
  // [4][64] sample results: share the pool's words, or (no pool) the first four stack
  // levels — both idle when a sample is handed over
  float* ex = reinterpret_cast<float*>(POOLED ? pool : lds);
  LaneStats st;
  // A.tilesPerBlock consecutive wave tiles per workgroup (1 unless RT_TILES_PER_BLOCK says otherwise: more of them
  // unbalance the grid — C3 13.7 / 14.8 / 17.8 ms at 4 / 8 / 16)
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t) render_tile<BRUTE, PHOTON, POOLED, STATS, LTV>(S, A, accum, L, pool, ex, t, st);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);  // (launch_render2 folds the stripes)
}

// Photon frames with 17 <= k <= RT_KNN_KMAX: k_render's photon path with the k-heap on layout HL (heap_rows(HL, k) rows
// above the stack rows).  LDS, not registers, sets these kernels' waves (a k-slot heap is 6 or 8 x 64 x k bytes per
// wave): MINW is the occupancy the smallest of them reaches, so the walk has every register it can use.
template <bool BRUTE, bool STATS, int MINW, int HL, int LTV = LT_NONE>
__global__ __launch_bounds__(BLOCK, MINW) void k_render_wide(DevScene S, RenderArgs A, float4* __restrict__ accum,
                                                          unsigned long long* __restrict__ counters) {
  uint32_t* lds = g_lds;
  const Lds L = carve_lds<true>(lds, A.stackLevels, A.k);
  float* ex = reinterpret_cast<float*>(lds);  // (the first four stack rows, idle when a sample is handed over)
  LaneStats st;
  const uint32_t t0 = blockIdx.x * A.tilesPerBlock, t1 = min(A.n_tiles, t0 + A.tilesPerBlock);
  for (uint32_t t = t0; t < t1; ++t)
    render_tile<BRUTE, true, false, STATS, LTV, WideHeap<HL>>(S, A, accum, L, nullptr, ex, t, st);
  if (STATS) flush_stats(st, counters, true);
  else flush_stats_striped(st, counters);
}

// The pooled integrator as PERSISTENT workgroups: one workgroup of up to 16 waves per CU
// for the whole launch.  Its LDS holds ONE copy of the top of the BVH (node records
// [0, topK), breadth-first) in front of the waves' private regions (traversal stack +
// vertex pool), and every wave draws wave tiles from a global counter until none is
// left — so a CU never idles behind a slow neighbour wave, and the node fetches of the
// upper tree levels (all of them for the 1.2k-triangle scene) never touch the vector L1.
// Waves never synchronise with each other after the tree copy.
template <bool STATS, int LT, bool FINE = false>
RT_DEV void persist_body(const DevScene& S, const RenderArgs& A, float4* __restrict__ accum, unsigned long long* __restrict__ counters) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  {
    uint4* dst = reinterpret_cast<uint4*>(g_lds);
    for (uint32_t i = threadIdx.x; i < 2u * S.topK; i += blockDim.x) dst[i] = S.nodes[i];
  }
  __syncthreads();  // the only workgroup-wide barrier
  uint32_t* mine = g_lds + 8u * S.topK + wv * A.waveWords;
  Lds L = carve_lds<false>(mine, A.stackLevels, 0);
  uint32_t* pool = mine + A.stackLevels * BLOCK;
  // (the 256-word exchange area of the sample adds: in the pool — or, where the pool is smaller than that, in the stack rows,
  // which are idle between two vertices; Trav::start rewrites the sentinel row)
  float* ex = reinterpret_cast<float*>((LT & LT_COMPACT3) ? mine : pool);
  LaneStats st;
#ifdef RT_PHASE_TIMING
  if (threadIdx.x < 24) g_phAcc[threadIdx.x] = 0;
  if (threadIdx.x == 0) g_phT0 = __builtin_amdgcn_s_memtime();
  __syncthreads();
#endif
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(A.tileCounter, 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (t >= A.n_tiles) break;
    render_tile<false, false, true, STATS, LT, Heap, FINE>(S, A, accum, L, pool, ex, t, st);
  }
#ifdef RT_PHASE_TIMING
  __syncthreads();
  if (threadIdx.x < PH_COUNT) atomicAdd(&counters[16 + threadIdx.x], g_phAcc[threadIdx.x]);
#endif
  flush_stats(st, counters, STATS);
}

template <bool STATS, int LT>
__global__ __launch_bounds__(1024) void k_render_persist(DevScene S, RenderArgs A, float4* __restrict__ accum,
                                                         unsigned long long* __restrict__ counters) {
  persist_body<STATS, LT, (LT & LT_VIEWS) == 0>(S, A, accum, counters);
}
// The same for the trees that leave the LDS to the stacks (LT_COMPACT3: the 424-word pool): workgroups of FOUR waves, one per
// SIMD, five of them per CU — 20 waves at 96 VGPRs (the compiler spills 28 registers, outside the descent: 1.4 % at equal
// occupancy on the 1 M-triangle scene, against what the four extra waves hide of its memory latency).
template <bool STATS, int LT>
__global__ __launch_bounds__(256, 5) void k_render_persist5(DevScene S, RenderArgs A, float4* __restrict__ accum,
                                                            unsigned long long* __restrict__ counters) {
  persist_body<STATS, LT>(S, A, accum, counters);
}

// Renderer.cpp:262-265
__global__ void k_resolve(uint32_t n_pixels, float spp, const float4* __restrict__ accum,
                          const float* __restrict__ bg, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pixels) return;
  const float4 a = accum[i];
  const float miss = (float)((int)spp - (int)a.w);
  out[3 * i + 0] = a.x / spp + bg[3 * i + 0] * miss / spp;
  out[3 * i + 1] = a.y / spp + bg[3 * i + 1] * miss / spp;
  out[3 * i + 2] = a.z / spp + bg[3 * i + 2] * miss / spp;
}

// ---------------------------------------------------------------- ray streams (wavefront stage T)
// RayTracer::rayTrace (RayTracer.h:27-53) over a QUEUE of rays in HBM instead of the rays of
// one wave's pixels: persistent waves draw rays from a global counter — whenever enough
// lanes have finished, they are refilled in one step (ballot + mbcnt compaction, one atomic
// per refill) — so the 64 lanes of a wave stay busy however unequal the rays are, and the
// kernel carries no shading state: 64 VGPRs, 8 waves per SIMD.
//   rayO[i] = origin xyz, w = kind bits (bit 0: any-hit);  rayD[i] = direction xyz
//   res[i]  = closest: {t bits, triangle id} or {~0, ~0};  any-hit: {hit ? 1 : 0, 0}
constexpr int STREAM_CHUNK = 2048;
template <int LT>
__global__ __launch_bounds__(1024, 8) void k_trace_stream(DevScene S, const float4* __restrict__ rayO,
                                                          const float4* __restrict__ rayD, uint32_t n,
                                                          uint2* __restrict__ res, uint32_t* __restrict__ counter,
                                                          uint32_t stackLevels) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (LT != LT_NONE) {
    uint4* dst = reinterpret_cast<uint4*>(g_lds);
    for (uint32_t i = threadIdx.x; i < 2u * S.topK; i += blockDim.x) dst[i] = S.nodes[i];
    __syncthreads();
  }
  uint32_t* stack = g_lds + 8u * S.topK + wv * stackLevels * BLOCK + lane;
  Trav<TRAV_MIXED, LT> T;
  T.idle(stack);
  T.sharedKey = nullptr, T.pj = 0;
  LaneStats st;
  uint32_t mine = ~0u;
  // A wave reserves STREAM_CHUNK rays at a time (one atomic on the shared counter per chunk:
  // every wave of the chip hitting ONE address per refill was the bottleneck, 3 Grays/s) and
  // STAGES them 64 at a time in registers: lane L holds ray (block + L), loaded one refill
  // before it is needed, so the HBM/L2 latency of a ray record hides behind a traversal
  // round.  Lanes that finished take the staged rays in order, through a lane shuffle.
  uint32_t cur = 0, end = 0;      // unstaged rest of the chunk
  uint32_t sBase = 0, sHead = 64;  // staged block: ray index of entry 0, next entry to hand out
  uint32_t sCount = 0;             // entries of the staged block that exist
  float4 so = make_float4(0.f, 0.f, 0.f, 0.f), sd = so;
  bool more = true;  // rays left to stage
  for (;;) {
    const uint64_t idle = wave_ballot(!T.live());
    const int nIdle = __popcll(idle);
    if ((nIdle >= (int)S.refillT || nIdle == 64) && (sHead < sCount || more)) {
      if (sHead < sCount) {
        const uint32_t r = sHead + lanes_below(idle);
        const bool take = !T.live() && r < sCount;
        const int src = take ? (int)r : (int)lane;
        const float ox = __shfl(so.x, src, 64), oy = __shfl(so.y, src, 64), oz = __shfl(so.z, src, 64), ow = __shfl(so.w, src, 64);
        const float dx = __shfl(sd.x, src, 64), dy = __shfl(sd.y, src, 64), dz = __shfl(sd.z, src, 64);
        if (take) {
          T.start(mk(ox, oy, oz), mk(dx, dy, dz), S.invBoxScale);
          T.anyHit = (__float_as_uint(ow) & 1u) != 0u;
          mine = sBase + r;
          // (a ray with a NaN component is dead on arrival: Trav::start — it hits nothing)
          if (!T.live()) res[mine] = T.anyHit ? make_uint2(0u, 0u) : make_uint2(~0u, ~0u), mine = ~0u;
        }
        sHead = sHead + (uint32_t)nIdle < sCount ? sHead + (uint32_t)nIdle : sCount;
      }
      if (sHead >= sCount && more) {  // stage the next 64 (consumed at a later refill)
        if (cur == end) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(counter, (uint32_t)STREAM_CHUNK);
          cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
          end = cur + (uint32_t)STREAM_CHUNK < n ? cur + (uint32_t)STREAM_CHUNK : n;
          if (cur >= n) cur = end = n, more = false;
        }
        if (more) {
          sBase = cur, sHead = 0, sCount = end - cur < 64u ? end - cur : 64u;
          if (lane < sCount) so = rayO[cur + lane], sd = rayD[cur + lane];
          cur += sCount;
        }
      }
    }
    if (wave_ballot(T.live()) == 0) {
      if (!more) break;
      continue;
    }
    const bool was = T.live();
    T.template round<false>(S, st);
    if (was && !T.live()) {
      res[mine] = T.anyHit ? make_uint2(T.found ? 1u : 0u, 0u)
                           : (T.found ? make_uint2(__float_as_uint(T.hit.t), T.hit.id) : make_uint2(~0u, ~0u));
      mine = ~0u;
    }
  }
}

// ---------------------------------------------------------------- wavefront integrator
#include "wavefront_kernels.h"

// ---------------------------------------------------------------- first-hit AOVs (rt_render_aov)
#include "aov_kernels.h"

// ---------------------------------------------------------------- motion vectors (rt_render_motion)
#include "motion_kernels.h"

// ---------------------------------------------------------------- ambient occlusion (rt_render_ao)
#include "ao_kernels.h"

// ---------------------------------------------------------------- ray batches (rt_render_rays)
#include "rays_kernels.h"

// ---------------------------------------------------------------- the frame's generator variants (rt_render_lens,
// rt_render_shutter, rt_render_views_shutter, rt_render_lights, rt_render_pick, rt_render_colors, rt_render_textured, rt_render_material)
#include "frame_variants.h"

// ---------------------------------------------------------------- frame assembly (multi-GPU)
// A rank's owned 8x8-pixel granules, packed [granule][64 pixels] (row-major inside the
// granule; slots outside the image are never read back), and the inverse on the rank
// that assembles the frame.  gran[g] = x8 | y8 << 16 (granule coordinates).
__global__ void k_pack_owned(const float4* __restrict__ accum, float4* __restrict__ packed, const uint32_t* __restrict__ gran,
                             uint32_t n, uint32_t width, uint32_t height) {
  const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (g >= n) return;
  const uint32_t x = (gran[g] & 0xffffu) * 8u + (l & 7u), y = (gran[g] >> 16) * 8u + (l >> 3);
  packed[(size_t)g * 64u + l] = (x < width && y < height) ? accum[(size_t)y * width + x] : make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ void k_unpack_owned(const float4* __restrict__ packed, float4* __restrict__ accum, const uint32_t* __restrict__ gran,
                               uint32_t n, uint32_t width, uint32_t height) {
  const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (g >= n) return;
  const uint32_t x = (gran[g] & 0xffffu) * 8u + (l & 7u), y = (gran[g] >> 16) * 8u + (l >> 3);
  if (x < width && y < height) accum[(size_t)y * width + x] = packed[(size_t)g * 64u + l];
}

// ---------------------------------------------------------------- test hooks
template <bool BRUTE, bool ANY, int LT = LT_NONE>
__global__ __launch_bounds__(BLOCK) void k_trace(DevScene S, const rt_ray* __restrict__ rays, uint32_t n,
                                                 rt_hit* __restrict__ hits, unsigned long long* counters) {
  __shared__ uint32_t lds[(STACK + 1) * BLOCK];  // (+1: the sentinel row)
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  LaneStats st;
  if (i < n) {
    HitRec h;
    const f3 o = ld(rays[i].origin), d = ld(rays[i].direction);
    // origins beyond the range the box padding was derived for (bvh_build.cpp: camera,
    // lights, geometry) are outside the exactness argument of the slab test: those rays
    // take the exhaustive loop (a NaN origin compares false and stays on the BVH path,
    // which ends it at once)
    const bool far = !BRUTE && fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) > S.originBound;
    bool found = cast<BRUTE, ANY, true, LT>(S, !far, o, d, lds + threadIdx.x, h, st);
    if (far) found = brute<ANY, true>(S, o, d, h, st);
    rt_hit r;
    r.hit = found, r.mesh = 0, r.tri = 0, r.vtx[0] = r.vtx[1] = r.vtx[2] = 0, r.u = r.v = r.d = 0.f;
    if (found && !ANY) {
      const uint4 tv = S.triShade[h.id];
      r.mesh = h.mesh;
      r.tri = h.id - S.meshTriBegin[h.mesh];
      const uint32_t vb = S.meshVtxBegin[h.mesh];
      r.vtx[0] = tv.x - vb, r.vtx[1] = tv.y - vb, r.vtx[2] = tv.z - vb;
      r.u = h.u, r.v = h.v, r.d = h.t;
    }
    hits[i] = r;
    if (ANY) st.shadow = 1;
    else st.closest = 1;
  }
  flush_stats(st, counters, true);
}

// The photon frames' walk on their tightest layout (k_render with a BVH shallower than the kd tree): S16 and
// stackLevels as launch_frame gives them (rt_api.cpp kd_stack), the k-slot heap directly above the stack rows.
template <bool S16>
__global__ __launch_bounds__(BLOCK) void k_knn(DevScene S, const float* __restrict__ q, uint32_t n, uint32_t k,
                                               uint32_t stackLevels, uint32_t* __restrict__ idx, float* __restrict__ dst,
                                               uint32_t* __restrict__ visited) {
  const Lds L = carve_lds<true>(g_lds, stackLevels, k);
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const Heap H{L.heap};
  const uint32_t vis = knn_query<S16>(S, ld(q + 3 * (size_t)i), (int)k, H, L.stack);
  for (uint32_t j = 0; j < k; j++) {
    idx[(size_t)i * k + j] = H.I((int)j);
    dst[(size_t)i * k + j] = H.D((int)j);
  }
  if (visited) visited[i] = vis;
}

// The wide frames' walk (k_render_wide) on their layout: the k-slot heap on layout HL above the stack rows.
template <bool S16, int MINW, int HL>
__global__ __launch_bounds__(BLOCK, MINW) void k_knn_wide(DevScene S, const float* __restrict__ q, uint32_t n, uint32_t k,
                                                       uint32_t stackLevels, uint32_t* __restrict__ idx,
                                                       float* __restrict__ dst, uint32_t* __restrict__ visited) {
  const Lds L = carve_lds<true>(g_lds, stackLevels, k);
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const WideHeap<HL> H = WideHeap<HL>::at(L, (int)k);
  const uint32_t vis = knn_query<S16>(S, ld(q + 3 * (size_t)i), (int)k, H, L.stack);
  for (uint32_t j = 0; j < k; j++) {
    idx[(size_t)i * k + j] = H.I((int)j);
    dst[(size_t)i * k + j] = H.D((int)j);
  }
  if (visited) visited[i] = vis;
}

// PhotonMap::PhotonMap + calculatePhotonPath (PhotonMap.h:14-50,92-155), one lane
// per emitted photon, stream key (seed, RT_STREAM_PHOTON, light*perLight + j).
// Each emitted photon stores at most ONE particle, so slot j of the output is
// either that particle or flagged empty: order is deterministic (stable compaction on the
// device: kd_build.hip k_photon_compact, rt_build_photon_map; rt_emit_photons compacts on the host).
template <bool BRUTE>
__global__ __launch_bounds__(BLOCK) void k_emit(DevScene S, uint32_t perLight, uint32_t seed,
                                                float4* __restrict__ outPos, float4* __restrict__ outDir,
                                                unsigned long long* counters) {
  __shared__ uint32_t lds[(STACK + 1) * BLOCK];
  uint32_t* stack = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
  LaneStats st;
  if (j < perLight * S.n_lights) {
    const uint32_t li = j / perLight;
    const rt_light Lt = S.lights[li];
    Rng g{rt_stream_seed(seed, RT_STREAM_PHOTON, j, 0)};
    const float lightPdf = 1.f / (float)S.n_lights;
    const f3 lsNormal = ld(Lt.normal);
    f3 o = light_sample(g, Lt);
    f3 d = hemisphere_sample(g, lsNormal);
    const float pdf0 = dot3(unit3(d), unit3(lsNormal));
    float weight = light_radiance(Lt, o) / (pdf0 * lightPdf);
    f3 ppos = mk(0.f, 0.f, 0.f), pdir = ppos;
    bool stored = false, exitNext = false;
    for (int depth = 0;; depth++) {
      if (exitNext) {
        stored = true;
        break;
      }
      if (depth >= 20) break;
      HitRec h;
      st.closest++;
      if (!cast<BRUTE, false, false>(S, true, o, d, stack, h, st)) {
        stored = depth != 0;
        break;
      }
      const float w = 1.f - h.u - h.v;
      const uint4 tv = S.triShade[h.id];
      const f3 nrm = unit3(interp3(S.vnrm, tv, w, h.u, h.v));
      const f3 pt = interp3(S.vpos, tv, w, h.u, h.v);
      ppos = pt, pdir = -d;
      const f3 rnd = hemisphere_sample(g, nrm);
      const f3 perfect = d - 2.f * (dot3(d, nrm)) * nrm;
      const float bsdf = len3(bsdf_eval(S.mats[h.mesh], nrm, d, rnd));
      const float pdf = (dot3(unit3(rnd), unit3(perfect)) + 1.f) / 2.f;
      weight *= bsdf / pdf;
      const float cont = fminf(weight, 1.f);
      if (g.uniformF(0.f, 1.f) > cont) exitNext = true;
      else weight /= cont;
      o = pt, d = rnd;
    }
    outPos[j] = make_float4(ppos.x, ppos.y, ppos.z, stored ? 1.f : 0.f);
    outDir[j] = make_float4(pdir.x, pdir.y, pdir.z, weight);
  }
  flush_stats(st, counters, false);
}

// Unit evaluations of the device building blocks (parity hooks, rt_test_unit).
__global__ void k_unit(uint32_t which, const void* __restrict__ in, void* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (which) {
    case RT_UNIT_ASIN:
      ((double*)out)[i] = rt_asin(((const double*)in)[i]);
      break;
    case RT_UNIT_SINF:
      ((float*)out)[i] = rt_sinf(((const float*)in)[i]);
      break;
    case RT_UNIT_COSF:
      ((float*)out)[i] = rt_cosf(((const float*)in)[i]);
      break;
    case RT_UNIT_STREAM_SEED: {
      const uint32_t* a = (const uint32_t*)in + 4 * (size_t)i;
      ((uint32_t*)out)[i] = rt_stream_seed(a[0], a[1], a[2], a[3]);
      break;
    }
    case RT_UNIT_TRIANGLE: {  // in: p0 p1 p2 o d (15 floats); out: hit u v t (4 floats)
      const float* a = (const float*)in + 15 * (size_t)i;
      float* o = (float*)out + 4 * (size_t)i;
      const f3 p0 = ld(a), p1 = ld(a + 3), p2 = ld(a + 6);
      float u = o[1], v = o[2], t = o[3];  // outputs may stay unwritten (Ray.cpp:14)
      const bool hit = tri_test_ref_order(ld(a + 9), ld(a + 12), p0, p1 - p0, p2 - p0, u, v, t);
      o[0] = hit ? 1.f : 0.f, o[1] = u, o[2] = v, o[3] = t;
      break;
    }
    case RT_UNIT_BSDF: {  // in: kd alpha albedo3 f03 n3 wi3 wo3 (17 floats); out: 3 floats
      const float* a = (const float*)in + 17 * (size_t)i;
      rt_material m;
      m.kd = a[0], m.alpha = a[1];
      for (int c = 0; c < 3; c++) m.albedo[c] = a[2 + c], m.f0[c] = a[5 + c];
      const f3 r = bsdf_eval(m, ld(a + 8), ld(a + 11), ld(a + 14));
      float* o = (float*)out + 3 * (size_t)i;
      o[0] = r.x, o[1] = r.y, o[2] = r.z;
      break;
    }
    case RT_UNIT_RAY_AT: {  // in: camera(12) u v (14 floats); out: o3 d3
      const float* a = (const float*)in + 14 * (size_t)i;
      rt_camera c;
      for (int k = 0; k < 3; k++)
        c.position[k] = a[k], c.lower_left[k] = a[3 + k], c.horizontal[k] = a[6 + k], c.vertical[k] = a[9 + k];
      f3 o, d;
      camera_ray(c, a[12], a[13], o, d);
      float* q = (float*)out + 6 * (size_t)i;
      q[0] = o.x, q[1] = o.y, q[2] = o.z, q[3] = d.x, q[4] = d.y, q[5] = d.z;
      break;
    }
    case RT_UNIT_LIGHT_EVAL: {  // in: rt_light(21 floats) p3; out: 3
      const float* a = (const float*)in + 24 * (size_t)i;
      rt_light l;
      memcpy(&l, a, sizeof(rt_light));
      const f3 r = light_eval(l, ld(a + 21));
      float* o = (float*)out + 3 * (size_t)i;
      o[0] = r.x, o[1] = r.y, o[2] = r.z;
      break;
    }
    case RT_UNIT_SAMPLERS: {
      // in (28 words): state, idx, n, pad, normal3, pad, rt_light(21 floats).
      // out (12 words): jitter x y, hemisphere dir3, light sample3, end state, pad3.
      // Draw order: jitter, hemisphere, light — each from the running state.
      const uint32_t* a = (const uint32_t*)in + 28 * (size_t)i;
      const float* af = (const float*)a;
      Rng g{a[0]};
      float* o = (float*)out + 12 * (size_t)i;
      jitter_sample(g, (int)a[1], (int)a[2], o[0], o[1]);
      const f3 h = hemisphere_sample(g, ld(af + 4));
      rt_light l;
      memcpy(&l, af + 7, sizeof(rt_light));
      const f3 p = light_sample(g, l);
      o[2] = h.x, o[3] = h.y, o[4] = h.z, o[5] = p.x, o[6] = p.y, o[7] = p.z;
      ((uint32_t*)o)[8] = g.s;
      o[9] = o[10] = o[11] = 0.f;
      break;
    }
    case RT_UNIT_LIGHT_SAMPLE: {  // in (22 words): state, rt_light(21 floats); out: sample3, end state
      const uint32_t* a = (const uint32_t*)in + 22 * (size_t)i;
      Rng g{a[0]};
      rt_light l;
      memcpy(&l, a + 1, sizeof(rt_light));
      const f3 p = light_sample(g, l);
      float* o = (float*)out + 4 * (size_t)i;
      o[0] = p.x, o[1] = p.y, o[2] = p.z;
      ((uint32_t*)o)[3] = g.s;
      break;
    }
    case RT_UNIT_POW: {  // in: double x; out: double rt_pow2(x), rt_pow5(x)
      const double x = ((const double*)in)[i];
      ((double*)out)[2 * (size_t)i] = rt_pow2(x), ((double*)out)[2 * (size_t)i + 1] = rt_pow5(x);
      break;
    }
    case RT_UNIT_RECIP: {  // in: float x; out: rtd::recip_fast(x), 1.0f / x, rtd::sqrt_fast(x), sqrtf(x)
      const float x = ((const float*)in)[i];
      float* o = (float*)out + 4 * (size_t)i;
      o[0] = rtd::recip_fast(x), o[1] = 1.0f / x, o[2] = rtd::sqrt_fast(x), o[3] = __builtin_sqrtf(x);
      break;
    }
    case RT_UNIT_BSDF_HOISTED: {
      // in (33 floats): the 17 of RT_UNIT_BSDF, then the rtd::DevMat the host made of the material (rt_api.cpp);
      // out: the hoisted form, the hoisted form FAST, the rt_material form FAST (9 floats)
      const float* a = (const float*)in + 33 * (size_t)i;
      rt_material m;
      m.kd = a[0], m.alpha = a[1];
      for (int c = 0; c < 3; c++) m.albedo[c] = a[2 + c], m.f0[c] = a[5 + c];
      DevMat dm;
      memcpy(&dm, a + 17, sizeof(DevMat));
      const f3 n = ld(a + 8), wi = ld(a + 11), wo = ld(a + 14);
      const f3 r0 = bsdf_apply<false>(bsdf_base<false>(dm, n, wo), wi);
      const f3 r1 = bsdf_apply<true>(bsdf_base<true>(dm, n, wo), wi);
      const f3 r2 = bsdf_apply<true>(bsdf_base<true>(m, n, wo), wi);
      float* o = (float*)out + 9 * (size_t)i;
      o[0] = r0.x, o[1] = r0.y, o[2] = r0.z, o[3] = r1.x, o[4] = r1.y, o[5] = r1.z, o[6] = r2.x, o[7] = r2.y, o[8] = r2.z;
      break;
    }
    default:
      break;
  }
}

// ---------------------------------------------------------------- launchers
// Dynamic LDS beyond 64 KiB must be allowed per kernel AND per device (one process may drive
// several devices: rt_group): `done` is the caller's per-kernel bit mask of devices already set.
template <class K>
static bool allow_big_lds(K kernel, unsigned long long& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 0;
  if (done & (1ull << dev)) return true;
#ifndef RT_PHASE_TIMING
  // Trav::round takes a node's byte offset as its LDS address: the tree copy must start at LDS
  // address 0, i.e. the kernel must not have static LDS in front of the dynamic segment
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) != hipSuccess || fa.sharedSizeBytes != 0) return false;
#endif
  // (the diagnostic build stays 256 B short of the CU's 160 KiB for its static LDS: the attribute
  // is refused when static + dynamic exceed the CU)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             4 * rtbvh::kLdsWordsPerCU);
  done |= 1ull << dev;
  return true;
}

// LDS plan of the persistent pooled kernel: W waves per workgroup (one workgroup per CU),
// topK tree-top nodes in front of W private regions of waveWords each.  160 KiB per CU.
struct PersistPlan {
  uint32_t waves, topK, waveWords, ldsBytes;
  int compact = 0;  // 1: LT_COMPACT pool layout, 2: LT_COMPACT2, 3: LT_COMPACT3 (workgroups of 4 waves, 5 per CU)
};
static PersistPlan plan_persist(const DevScene& S, const RenderArgs& A) {
  const uint32_t total = rtbvh::kLdsWordsPerCU;  // words
  const uint32_t waveWords = A.stackLevels * BLOCK + VP_WORDS;
  static const int wEnv = getenv("RT_PERSIST_WAVES") ? atoi(getenv("RT_PERSIST_WAVES")) : 0;
  static const int kEnv = getenv("RT_TOPK") ? atoi(getenv("RT_TOPK")) : -1;
  const uint32_t cap = S.n_nodes < rtbvh::kTopNodes ? S.n_nodes : rtbvh::kTopNodes;
  // Measured (MI355X, Grays/s): occupancy comes first — 12 instead of 16 waves costs 15-17 %
  // on every scene; the whole tree in LDS (LT_ALL, no branch) gives C2 +5.6 %.  So: as many
  // waves as fit (at most 16), then as much of the tree as fits beside them.
  // RT_PERSIST_WAVES / RT_TOPK override.
  uint32_t w = wEnv > 0 ? (uint32_t)wEnv : 16u;
  while (w > 1u && w * waveWords > total) --w;
  if (w * waveWords > total) return PersistPlan{0, 0, waveWords, 0};
  // big trees whose stacks leave fewer than 16 waves: the compact pool, if it buys a wave
  static const int cpEnv = getenv("RT_COMPACT") ? atoi(getenv("RT_COMPACT")) : -1;
  // ... and if the smallest pool makes room for TWENTY waves (five workgroups of four per CU, 96 VGPRs): the 1 M-triangle
  // scene's 25 stack rows + 424 words = 8,096 B per wave
  if ((cpEnv < 0 || cpEnv == 3) && S.n_nodes > kPrioMaxNodes && !S.q8 && wEnv <= 0 && kEnv < 0) {
    // (the LDS is handed out in units of 1,280 bytes: five workgroups of four waves must fit with their sizes rounded up)
    const uint32_t ww3 = A.stackLevels * BLOCK + (uint32_t)VpLayout<3>::WORDS;
    if (5u * ((16u * ww3 + rtbvh::kLdsGrainBytes - 1u) / rtbvh::kLdsGrainBytes * rtbvh::kLdsGrainBytes) <= 4u * total) {
      PersistPlan cp{4u, 0u, ww3, 4u * 4u * ww3};
      cp.compact = 3;
      return cp;
    }
  }
  if (cpEnv != 0 && (S.n_nodes > kPrioMaxNodes || S.q8) && w < 16u && kEnv < 0) {
    // (the smallest step that buys the most waves; RT_COMPACT = 1 / 2 forces a level)
    uint32_t bestW = w;
    int level = 0;
    for (int lv = 1; lv <= 2; ++lv) {
      const uint32_t ww = waveWords - (uint32_t)(lv * VP_COMPACT_SAVES);
      uint32_t w2 = wEnv > 0 ? (uint32_t)wEnv : 16u;
      while (w2 > 1u && w2 * ww > total) --w2;
      if (cpEnv > 0 ? lv == cpEnv : w2 > bestW) bestW = w2, level = lv;
    }
    if (level) {
      const uint32_t ww = waveWords - (uint32_t)(level * VP_COMPACT_SAVES);
      PersistPlan cp{bestW, 0, ww, 4u * bestW * ww};
      cp.compact = level;
      return cp;
    }
  }
  uint32_t k = S.q8 ? 0u : (total - w * waveWords) / 8u;  // (Q8 records are not copied into LDS)
  k = k < cap ? k : cap;
  // (a PARTIAL top — a prefix of the area-ordered node array — costs the step a second load path;
  // with the step as lean as it is now it pays from a few hundred nodes up: the 11.7 k-triangle
  // mesh keeps 688 of its 6,003 nodes in LDS beside 16 waves, +1.8 %; 256 nodes +0.7 %)
  if (kEnv >= 0) k = (uint32_t)kEnv < k ? (uint32_t)kEnv : k;
  else if (k < S.n_nodes && k < 256u) k = 0;
  return PersistPlan{w, k, waveWords, 4u * (8u * k + w * waveWords)};
}

// The wide k-heap's layout (DESIGN.md "Photon k up to 256"; measured on config 3's frame at k = 17 .. 256): the 6-byte
// split planes where the indices fit in 16 bits (kd16: fewer than 65,535 photons) AND they give the CU more waves than
// the 8-byte entries — 11.65 / 28.2 / 99.8 / 307 ms against 12.4 / 33.2 / 116.9 / 425 ms at k = 17 / 32 / 64 / 128;
// at equal waves the interleaved entries' one LDS op per move wins (k = 256, one wave per CU either way: 1593 against
// 1686 ms).  RT_KNN_WIDE_LAYOUT=8 / 16 forces a layout (16: where the indices fit; tools/knn_wide_bench.py's A/B).
static int wide_layout(bool kd16, uint32_t stackLevels, uint32_t k) {
  static const int forced = getenv("RT_KNN_WIDE_LAYOUT") ? atoi(getenv("RT_KNN_WIDE_LAYOUT")) : 0;
  if (!kd16 || forced == 8) return HEAP_WIDE8;
  if (forced == 16) return HEAP_SPLIT16;
  const uint32_t cu = rtbvh::kLdsWordsPerCU / BLOCK;  // LDS rows per CU
  return cu / (stackLevels + heap_rows(HEAP_SPLIT16, k)) > cu / (stackLevels + heap_rows(HEAP_WIDE8, k)) ? HEAP_SPLIT16
                                                                                                        : HEAP_WIDE8;
}
// Occupancy target (waves per SIMD) of the timed wide instances: what k = 17 reaches on config 3's layout (split planes,
// 10 stack rows + 26 heap rows: 16 waves per CU); larger k hold fewer waves, bound by LDS
constexpr int MINW_WIDE = 4;

// RT_KNN_VERBOSE: one line on stderr per photon-frame or wide k-NN launch — the instance, its heap layout (-1: k_render's),
// its LDS per wave and the waves per CU the runtime reports for it (tools/knn_wide_bench.py)
template <class K>
static void knn_report(K kernel, const char* name, int hl, uint32_t k, size_t ldsBytes) {
  static const bool verbose = getenv("RT_KNN_VERBOSE") != nullptr;
  if (!verbose) return;
  int blocks = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, BLOCK, ldsBytes) != hipSuccess) blocks = -1;
  fprintf(stderr, "{\"knn_kernel\": \"%s\", \"layout\": %d, \"k\": %u, \"lds_bytes\": %zu, \"waves_per_cu\": %d}\n", name, hl, k,
          ldsBytes, blocks);
}

template <bool BRUTE>
static hipError_t launch_render_wide(bool stats, const DevScene& S, const RenderArgs& A, float4* accum,
                                     unsigned long long* counters, hipStream_t stream) {
  const int hl = wide_layout(A.kd16 != 0, A.stackLevels, A.k);
  const size_t ldsBytes = 4u * (size_t)(A.stackLevels + heap_rows(hl, A.k)) * BLOCK;
  if (A.k > (uint32_t)RT_KNN_KMAX || ldsBytes > 4u * (size_t)rtbvh::kLdsWordsPerCU) return hipErrorInvalidValue;
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;
#define RT_LAUNCH_WIDE1(ST, MW, HLV, LTV)                                                                             \
  do {                                                                                                                \
    static unsigned long long done = 0;                                                                               \
    if (!allow_big_lds(&k_render_wide<BRUTE, ST, MW, HLV, LTV>, done)) return hipErrorInvalidConfiguration;            \
    knn_report(k_render_wide<BRUTE, ST, MW, HLV, LTV>, "k_render_wide", HLV, A.k, ldsBytes);                          \
    hipLaunchKernelGGL((k_render_wide<BRUTE, ST, MW, HLV, LTV>), dim3(A.n_tiles), dim3(BLOCK), ldsBytes, stream, S, A1, \
                       accum, counters);                                                                              \
  } while (0)
#define RT_LAUNCH_WIDE(ST, MW, HLV)                        \
  do {                                                     \
    if (A.tileView) RT_LAUNCH_WIDE1(ST, MW, HLV, LT_VIEWS); \
    else RT_LAUNCH_WIDE1(ST, MW, HLV, LT_NONE);            \
  } while (0)
#define RT_LAUNCH_WIDE_HL(ST, MW)                                   \
  do {                                                              \
    if (hl == HEAP_SPLIT16) RT_LAUNCH_WIDE(ST, MW, HEAP_SPLIT16);   \
    else RT_LAUNCH_WIDE(ST, MW, HEAP_WIDE8);                        \
  } while (0)
  if (stats) RT_LAUNCH_WIDE_HL(true, 1);
  else {
    RT_LAUNCH_WIDE_HL(false, MINW_WIDE);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
#undef RT_LAUNCH_WIDE_HL
#undef RT_LAUNCH_WIDE
#undef RT_LAUNCH_WIDE1
  return hipGetLastError();
}

static bool persist_wanted(const RenderArgs& A) {
  static const bool noPersist = getenv("RT_NO_PERSIST") != nullptr;
  return !noPersist && A.tileCounter && A.numCUs;
}
static bool pool_wanted(const DevScene& S, const RenderArgs& A) { return (A.flags & 1u) && S.n_lights <= (uint32_t)POOL_L; }

uint32_t persist_fine_waves(bool brute_force, bool photon, const DevScene& S, const RenderArgs& A) {
  if (brute_force || photon || !pool_wanted(S, A) || !persist_wanted(A) || A.tileView) return 0;
  const PersistPlan P = plan_persist(S, A);
  return P.compact == 3 ? 0u : P.waves * A.numCUs;  // (the four-wave flavour keeps the coarse list)
}

template <bool BRUTE, bool PHOTON, bool POOLED>
static hipError_t launch_render2(bool stats, const DevScene& S, const RenderArgs& A, float4* accum,
                                 unsigned long long* counters, hipStream_t stream) {
  const uint32_t blocks = A.n_tiles;
  if (blocks == 0) return hipSuccess;
  // (a list with a fine tail is k_render_persist's alone: persist_fine_waves says 0 for every other launch)
  if (A.fineFrom < A.n_tiles && !(POOLED && persist_fine_waves(false, false, S, A))) return hipErrorInvalidValue;
  if (POOLED && persist_wanted(A)) {
    const PersistPlan P = plan_persist(S, A);
    if (P.waves) {
      DevScene S2 = S;
      RenderArgs A2 = A;
      S2.topK = P.topK, A2.waveWords = P.waveWords;
      hipError_t e = hipMemsetAsync(A.tileCounter, 0, sizeof(uint32_t), stream);
      if (e != hipSuccess) return e;
      const uint32_t perCU = P.waves;                                    // waves one workgroup brings
      const uint32_t slots = P.compact == 3 ? 5u * A.numCUs : A.numCUs;  // workgroups the device holds at once
      const uint32_t wgs = (blocks + perCU - 1) / perCU < slots ? (blocks + perCU - 1) / perCU : slots;
#define RT_LAUNCH_PERSIST1(ST, LTV)                                                                         \
  do {                                                                                                      \
    static unsigned long long done = 0;                                                                     \
    if (!allow_big_lds(&k_render_persist<ST, LTV>, done)) return hipErrorInvalidConfiguration;              \
    hipLaunchKernelGGL((k_render_persist<ST, LTV>), dim3(wgs), dim3(64u * P.waves), P.ldsBytes, stream, S2, \
                       A2, accum, counters);                                                                \
  } while (0)
#define RT_LAUNCH_PERSIST(ST, LTV)                                \
  do {                                                            \
    if (A.tileView) RT_LAUNCH_PERSIST1(ST, (LTV) | LT_VIEWS);     \
    else RT_LAUNCH_PERSIST1(ST, LTV);                             \
  } while (0)
      // Two instances per layout: the timed one, with the three-instruction 1 / det and 1 / length (the host has bounded
      // their operands: DevScene::slowRecip == 0), and the COUNTED one, which divides — and which also serves the rare
      // scene beyond those bounds (same frame: the short forms give the division's bits).
#define RT_LAUNCH_EITHER(LTV)                                    \
  do {                                                           \
    if (stats || S.slowRecip) RT_LAUNCH_PERSIST(true, LTV);      \
    else RT_LAUNCH_PERSIST(false, (LTV) | LT_FASTDET);           \
  } while (0)
      // ... and, of the layouts the BASELINE configs run in, a second timed instance for trees whose leaves hold at most
      // two records (LT_LEAF2: RenderArgs::flags bit 1, set per launch from the resident tree).  RT_LEAF2=0 forces the
      // general instances; it is read at every launch, so one process can compare the two.
      const char* const leaf2Env = getenv("RT_LEAF2");
      const bool leaf2 = (A.flags & 2u) && !(leaf2Env && atoi(leaf2Env) == 0) && !stats && !S.slowRecip && !A.tileView;
      // ... and of the LT_ALL one a twin with the compiler's descent loop (LT_CLOOP; Trav::DESCENT): RT_DESCENT=0, read at
      // every launch like RT_LEAF2.
      const char* const descentEnv = getenv("RT_DESCENT");
      const bool cloop = descentEnv && atoi(descentEnv) == 0;
#define RT_LAUNCH_LEAF2(LTV)                                                                               \
  do {                                                                                                     \
    if (leaf2 && cloop && ((LTV) & 3) == LT_ALL) RT_LAUNCH_PERSIST1(false, LT_ALL | LT_FASTDET | LT_LEAF2 | LT_CLOOP); \
    else if (leaf2) RT_LAUNCH_PERSIST1(false, (LTV) | LT_FASTDET | LT_LEAF2);                              \
    else RT_LAUNCH_EITHER(LTV);                                                                            \
  } while (0)
      const int lt = P.topK == 0 ? LT_NONE : P.topK >= S.n_nodes ? LT_ALL : LT_TOP;
      if (P.compact == 3) {
#define RT_LAUNCH_PERSIST5(ST, LTV)                                                                                       \
  do {                                                                                                                    \
    static unsigned long long done = 0;                                                                                   \
    if (!allow_big_lds(&k_render_persist5<ST, LTV>, done)) return hipErrorInvalidConfiguration;                           \
    hipLaunchKernelGGL((k_render_persist5<ST, LTV>), dim3(wgs), dim3(256), P.ldsBytes, stream, S2, A2, accum, counters); \
  } while (0)
        constexpr int C3 = LT_NONE | LT_NOPRIO | LT_COMPACT3;
        if (leaf2) RT_LAUNCH_PERSIST5(false, C3 | LT_FASTDET | LT_LEAF2);
        else if (stats || S.slowRecip) {
          if (A.tileView) RT_LAUNCH_PERSIST5(true, C3 | LT_VIEWS);
          else RT_LAUNCH_PERSIST5(true, C3);
        } else {
          if (A.tileView) RT_LAUNCH_PERSIST5(false, C3 | LT_FASTDET | LT_VIEWS);
          else RT_LAUNCH_PERSIST5(false, C3 | LT_FASTDET);
        }
#undef RT_LAUNCH_PERSIST5
      } else if (S.q8) {  // the one-request records (the context chose them: rt_api.cpp create_ctx)
        if (P.compact == 2) RT_LAUNCH_EITHER(LT_Q8 | LT_NOPRIO | LT_COMPACT2);
        else if (P.compact) RT_LAUNCH_EITHER(LT_Q8 | LT_NOPRIO | LT_COMPACT);
        else RT_LAUNCH_EITHER(LT_Q8 | LT_NOPRIO);
      } else if (P.compact == 2) RT_LAUNCH_EITHER(LT_NONE | LT_NOPRIO | LT_COMPACT2);
      else if (P.compact) RT_LAUNCH_EITHER(LT_NONE | LT_NOPRIO | LT_COMPACT);
      else if (lt == LT_ALL) RT_LAUNCH_LEAF2(LT_ALL);
      else if (lt == LT_TOP) RT_LAUNCH_LEAF2(LT_TOP);
      else RT_LAUNCH_EITHER(LT_NONE | LT_NOPRIO);  // (a small tree beside stacks that leave no room for 256 of its nodes: rare)
#undef RT_LAUNCH_LEAF2
#undef RT_LAUNCH_EITHER
#undef RT_LAUNCH_PERSIST
#undef RT_LAUNCH_PERSIST1
      return hipGetLastError();
    }
  }
  if (PHOTON && A.k > (uint32_t)KMAX) return launch_render_wide<BRUTE>(stats, S, A, accum, counters, stream);
  const uint32_t rows = A.stackLevels + (PHOTON ? 2 * A.k : 0);
  const size_t ldsBytes = 4u * ((rows < 4u ? 4u : rows) * BLOCK + (POOLED ? VP_WORDS : 0));
  RenderArgs A1 = A;
  A1.tilesPerBlock = 1u;  // (more wave tiles per workgroup unbalance the grid: C3 13.7 / 14.8 / 17.8 ms at 4 / 8 / 16 in round 3)
  const uint32_t nBlocks = blocks;
  // Occupancy target (waves per SIMD) of the one-wave-per-workgroup kernels.
  // (the photon kernel at 5 waves per SIMD: its walk waits on L1-hit loads half of its life; 96 VGPRs cost 12 spilled registers
  // outside the walk, and the 16-bit stack makes the LDS room — measured: C3 7.3 -> see DESIGN.md 4.6)
  constexpr int MINW = PHOTON ? 5 : 4;
  if (PHOTON) knn_report(stats ? k_render<BRUTE, PHOTON, POOLED, true, 1> : k_render<BRUTE, PHOTON, POOLED, false, MINW>,
                         "k_render", -1, A.k, ldsBytes);
  if (stats) {
    if (A.tileView) hipLaunchKernelGGL((k_render<BRUTE, PHOTON, POOLED, true, 1, LT_VIEWS>), dim3(nBlocks), dim3(BLOCK), ldsBytes, stream, S, A1, accum, counters);
    else hipLaunchKernelGGL((k_render<BRUTE, PHOTON, POOLED, true, 1>), dim3(nBlocks), dim3(BLOCK), ldsBytes, stream, S, A1, accum, counters);
  } else {
    if (A.tileView) hipLaunchKernelGGL((k_render<BRUTE, PHOTON, POOLED, false, MINW, LT_VIEWS>), dim3(nBlocks), dim3(BLOCK), ldsBytes, stream, S, A1, accum, counters);
    else hipLaunchKernelGGL((k_render<BRUTE, PHOTON, POOLED, false, MINW>), dim3(nBlocks), dim3(BLOCK), ldsBytes, stream, S, A1, accum, counters);
    hipLaunchKernelGGL(k_fold_stripes, dim3(1), dim3(1024), 0, stream, counters);
  }
  return hipGetLastError();
}

hipError_t launch_render(bool brute_force, bool photon, bool stats, const DevScene& S, const RenderArgs& A,
                         float4* accum, unsigned long long* counters, hipStream_t stream) {
  if (brute_force) return photon ? launch_render2<true, true, false>(stats, S, A, accum, counters, stream)
                                 : launch_render2<true, false, false>(stats, S, A, accum, counters, stream);
  if (photon) return launch_render2<false, true, false>(stats, S, A, accum, counters, stream);
  // direct lighting through the BVH: the vertex pool handles up to POOL_L lights
  if (pool_wanted(S, A)) return launch_render2<false, false, true>(stats, S, A, accum, counters, stream);
  return launch_render2<false, false, false>(stats, S, A, accum, counters, stream);
}

hipError_t launch_resolve(uint32_t n_pixels, uint32_t spp, const float4* accum, const float* bg, float* out,
                          hipStream_t stream) {
  if (n_pixels == 0) return hipSuccess;
  hipLaunchKernelGGL(k_resolve, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, (float)spp, accum,
                     bg, out);
  return hipGetLastError();
}

hipError_t launch_trace_stream(const DevScene& S, const float4* rayO, const float4* rayD, uint32_t n, uint2* res,
                               uint32_t* counter, uint32_t stackLevels, uint32_t numCUs, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(counter, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  // LDS: [tree, if all of it fits beside the stacks][16 waves x stack]; two workgroups per CU
  const uint32_t total = 160u * 1024u / 4u / 2u - 32u;  // words per workgroup
  uint32_t wpw = 16u;                                   // waves per workgroup: as many as the stacks allow
  while (wpw > 1u && wpw * stackLevels * BLOCK > total) --wpw;
  const uint32_t stackWords = wpw * stackLevels * BLOCK;
  static const int kEnv = getenv("RT_STREAM_TOPK") ? atoi(getenv("RT_STREAM_TOPK")) : -1;
  DevScene S2 = S;
  S2.topK = 0;
  if (stackWords > total) return hipErrorInvalidValue;
  if (stackWords + 8u * S.n_nodes <= total) S2.topK = S.n_nodes;
  if (kEnv >= 0) S2.topK = (uint32_t)kEnv < S2.topK ? (uint32_t)kEnv : S2.topK;
  const uint32_t ldsBytes = 4u * (8u * S2.topK + stackWords);
  const uint32_t waves = (n + 63u) / 64u;
  uint32_t wgs = (waves + wpw - 1u) / wpw;
  static const uint32_t perCU = getenv("RT_STREAM_WGS") ? (uint32_t)atoi(getenv("RT_STREAM_WGS")) : 2u;
  wgs = wgs < perCU * numCUs ? wgs : perCU * numCUs;
  if (S2.topK >= S.n_nodes && S2.topK) {
    static unsigned long long done = 0;
    if (!allow_big_lds(&k_trace_stream<LT_ALL>, done)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((k_trace_stream<LT_ALL>), dim3(wgs), dim3(64u * wpw), ldsBytes, stream, S2, rayO, rayD, n, res, counter, stackLevels);
  } else {
    static unsigned long long done = 0;
    if (!allow_big_lds(&k_trace_stream<LT_NONE>, done)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((k_trace_stream<LT_NONE>), dim3(wgs), dim3(64u * wpw), ldsBytes, stream, S2, rayO, rayD, n, res, counter, stackLevels);
  }
  return hipGetLastError();
}

hipError_t launch_pack(bool unpack, const float4* src, float4* dst, const uint32_t* gran, uint32_t n, uint32_t width,
                       uint32_t height, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + 3) / 4), block(256);
  if (unpack) hipLaunchKernelGGL(k_unpack_owned, grid, block, 0, stream, src, dst, gran, n, width, height);
  else hipLaunchKernelGGL(k_pack_owned, grid, block, 0, stream, src, dst, gran, n, width, height);
  return hipGetLastError();
}


hipError_t launch_trace(bool brute_force, bool any, const DevScene& S, const rt_ray* rays, uint32_t n,
                        rt_hit* hits, unsigned long long* counters, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (brute_force) {
    if (any) hipLaunchKernelGGL((k_trace<true, true>), grid, block, 0, stream, S, rays, n, hits, counters);
    else hipLaunchKernelGGL((k_trace<true, false>), grid, block, 0, stream, S, rays, n, hits, counters);
  } else if (S.q8) {  // the context traverses the one-request records
    if (any) hipLaunchKernelGGL((k_trace<false, true, LT_Q8>), grid, block, 0, stream, S, rays, n, hits, counters);
    else hipLaunchKernelGGL((k_trace<false, false, LT_Q8>), grid, block, 0, stream, S, rays, n, hits, counters);
  } else {
    if (any) hipLaunchKernelGGL((k_trace<false, true>), grid, block, 0, stream, S, rays, n, hits, counters);
    else hipLaunchKernelGGL((k_trace<false, false>), grid, block, 0, stream, S, rays, n, hits, counters);
  }
  return hipGetLastError();
}

hipError_t launch_knn(const DevScene& S, const float* q, uint32_t n, uint32_t k, bool kd16, uint32_t stackLevels,
                      uint32_t* idx, float* dist, uint32_t* visited, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (k < 1 || k > (uint32_t)KMAX || stackLevels < 2 || stackLevels > (uint32_t)STACK + 1) return hipErrorInvalidValue;
  const size_t ldsBytes = 4u * (size_t)(stackLevels + 2 * k) * BLOCK;
  if (kd16)
    hipLaunchKernelGGL(k_knn<true>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), ldsBytes, stream, S, q, n, k, stackLevels,
                       idx, dist, visited);
  else
    hipLaunchKernelGGL(k_knn<false>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), ldsBytes, stream, S, q, n, k, stackLevels,
                       idx, dist, visited);
  return hipGetLastError();
}

hipError_t launch_knn_wide(const DevScene& S, const float* q, uint32_t n, uint32_t k, bool kd16, uint32_t stackLevels,
                           uint32_t* idx, float* dist, uint32_t* visited, hipStream_t stream) {
  if (k <= (uint32_t)KMAX) return launch_knn(S, q, n, k, kd16, stackLevels, idx, dist, visited, stream);  // (the same instance)
  if (n == 0) return hipSuccess;
  if (k > (uint32_t)RT_KNN_KMAX || stackLevels < 2 || stackLevels > (uint32_t)STACK + 1) return hipErrorInvalidValue;
  const int hl = wide_layout(kd16, stackLevels, k);
  const size_t ldsBytes = 4u * (size_t)(stackLevels + heap_rows(hl, k)) * BLOCK;
  const dim3 grid((n + BLOCK - 1) / BLOCK);
#define RT_LAUNCH_KNN_WIDE(S16, HLV)                                                                                  \
  do {                                                                                                                \
    static unsigned long long done = 0;                                                                               \
    if (!allow_big_lds(&k_knn_wide<S16, MINW_WIDE, HLV>, done)) return hipErrorInvalidConfiguration;                  \
    knn_report(k_knn_wide<S16, MINW_WIDE, HLV>, "k_knn_wide", HLV, k, ldsBytes);                                     \
    hipLaunchKernelGGL((k_knn_wide<S16, MINW_WIDE, HLV>), grid, dim3(BLOCK), ldsBytes, stream, S, q, n, k, stackLevels, \
                       idx, dist, visited);                                                                           \
  } while (0)
  if (!kd16) RT_LAUNCH_KNN_WIDE(false, HEAP_WIDE8);
  else if (hl == HEAP_SPLIT16) RT_LAUNCH_KNN_WIDE(true, HEAP_SPLIT16);
  else RT_LAUNCH_KNN_WIDE(true, HEAP_WIDE8);
#undef RT_LAUNCH_KNN_WIDE
  return hipGetLastError();
}

hipError_t launch_emit(const DevScene& S, uint32_t perLight, uint32_t seed, float4* outPos, float4* outDir,
                       unsigned long long* counters, hipStream_t stream) {
  const uint32_t n = perLight * S.n_lights;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_emit<false>), dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, S, perLight, seed,
                     outPos, outDir, counters);
  return hipGetLastError();
}

// recip_fast / sqrt_fast against the division and sqrtf on THIS device: every mantissa (2^23) in two neighbouring
// binades (both signs for the reciprocal) — v_rcp_f32 and v_rsq_f32 work on the mantissa and the exponent's parity, and
// scaling by powers of four is exact on both sides of the comparison away from the denormals, so this covers what the
// exhaustive check of tools/microbench/recip_exact.hip found to be the whole in-range behaviour.  *bad != 0: a mismatch.
__global__ void k_selfcheck_recip(uint32_t* bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // 2^25: sign | binade | mantissa
  const uint32_t bits = ((i >> 24) << 31) | ((127u + ((i >> 23) & 1u)) << 23) | (i & 0x7fffffu);
  const float x = __uint_as_float(bits);
  bool ok = __float_as_uint(rtd::recip_fast(x)) == __float_as_uint(1.0f / x);
  if (!(i >> 24)) ok = ok && __float_as_uint(rtd::sqrt_fast(x)) == __float_as_uint(__builtin_sqrtf(x));
  if (!ok) atomicOr(bad, 1u);
}
hipError_t launch_selfcheck_recip(uint32_t* dBad, hipStream_t stream) {
  hipLaunchKernelGGL(k_selfcheck_recip, dim3(1u << 17), dim3(256), 0, stream, dBad);
  return hipGetLastError();
}

hipError_t launch_unit(uint32_t which, const void* in, void* out, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (which == RT_UNIT_HEMISPHERE) {
    hipLaunchKernelGGL(k_unit_hemisphere, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t*)in, (uint32_t*)out, n);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_unit, dim3((n + 255) / 256), dim3(256), 0, stream, which, in, out, n);
  return hipGetLastError();
}

}  // namespace rtk
