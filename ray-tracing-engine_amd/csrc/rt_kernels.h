// rt_kernels.h — host<->device argument blocks and kernel launchers
// (implemented in rt_kernels.hip, called from rt_api.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "bvh_build.h"
#include "rt_amd.h"
#include "rt_device.h"

#define RTK_KMAX 16  // photon k-heap slots per lane of k_render / k_knn (LDS budget, rt_kernels.hip); up to RT_KNN_KMAX
                     // (rt_amd.h) the wide instances k_render_wide / k_knn_wide serve

enum {
  RTK_CNT_CLOSEST = 0,
  RTK_CNT_SHADOW,
  RTK_CNT_KNN,
  RTK_CNT_NODES,
  RTK_CNT_TRIS,
  RTK_CNT_KD,
  RTK_CNT_WNODE,  // wave-level node steps (a step = one descent iteration of a wave)
  RTK_CNT_WLEAF,  // wave-level leaf phases
  RTK_CNT_LWAIT,  // lanes holding a leaf, summed over the wave-level node steps
  RTK_CNT_LIDLE,  // lanes without a ray, summed over the wave-level node steps
  RTK_CNT_FRAMES, // Q8 node format: block frames fetched
  RTK_CNT_COUNT = 32  // [16..31]: section clocks of the diagnostic build (RT_PHASE_TIMING)
};

namespace rtk {

// Device-resident flattened scene (all pointers are HBM allocations of rt_ctx).
struct DevScene {
  const uint4* nodes;      // n_nodes x 32 B: 12 x f16 box planes ((lo, hi) per axis, child 0 then child 1, scaled) + 2 child refs
  const uint4* q8;         // the one-request form (rtbvh::Slot16: frames, 16-B node records and triangle records in one array), or null:
                           // when set, the pooled render kernel and k_trace traverse it instead of nodes / tris
  uint32_t q8ShiftBytes;   // log2 of a block's BYTES (rtbvh::Built::q8Shift + 4)
  const float4* tris;      // n_tris x 48 B, BVH leaf order: {p0,e1.x}{e1.yz,e2.xy}{e2.z,id,mesh,-}
  const float4* trisRef;   // same records in reference (mesh,tri) order (brute-force path)
  const uint4* triShade;   // per global triangle id: {v0,v1,v2 (global vertex ids), mesh}
  const float* vpos;       // [n_vertices][3]
  const float* vnrm;       // [n_vertices][3]
  const rt_material* mats; // [n_meshes]
  const rtd::DevMat* matsDev;  // [n_meshes] the same with the per-material constants of Material.h:25-70 worked out (rt_device.h)
  const rt_light* lights;  // [n_lights]
  const uint32_t* meshTriBegin;
  const uint32_t* meshVtxBegin;
  const float4* phPos;     // photons in kd-tree order: xyz + pad
  const float4* phDir;     // income direction xyz + weight
  const uint4* phTopo;     // per photon, 32 B: {position xyz, left child | axis << 30}{right child, parent's split coordinate, parent's axis, 0} (kd_build.hip k_kd_topology)
  uint32_t n_tris, n_nodes, n_lights, n_photons;
  float invBoxScale;       // 1 / rtbvh::Built::boxScale
  uint32_t topK;           // node records [0, topK) are LDS-resident in the persistent kernel (set per launch)
  float originBound;       // k_trace: rays starting farther out run the exhaustive loop (rtbvh::Built)
  uint32_t leafT;          // Trav::round leaves its descent when fewer lanes than this still descend ...
  uint32_t leafMul;        // ... and fewer than leafMul/64 of the wave's live lanes
  uint32_t slowRecip;      // 1: 1 / det by division (rays of unknown length); 0: rtd::recip_fast — |det| < 2^100 is guaranteed
  uint32_t refillT;        // vertex_pool hands out rays once this many workers are free
  uint32_t stealT;         // ... and splits the stacks of the last long rays once this many are free
  rt_camera cam;
};

// One view of a multi-view frame (rt_render_views): what the wave tiles of that view render with in place of DevScene::cam,
// RenderArgs::seed and the accumulator's base.  64 bytes, read by scalar loads.
struct ViewRec {
  rt_camera cam;
  uint32_t seed;      // stream key of the view's pixels
  uint32_t accumOff;  // first float4 of the view's accumulator slice (view * width * height)
  uint32_t pad[2];
};
static_assert(sizeof(ViewRec) == 64, "ViewRec is four 16-byte scalar loads");

// The shutter of one view of a multi-view shutter frame (rt_render_views_shutter): ShutterRec's host-derived constants
// (below) with the view's camera in the place of the context's, in a table parallel to the views' (ViewRec stays 64
// bytes).  80 bytes, read by scalar loads.
struct ViewShutterRec {
  float d[12];        // camera_close - cameras[view], component by component (position, lower_left, H, V)
  float open, close;  // the exposure: t = uniformF(open, close)
  float aperture;     // lens radius, 0 = pinhole (fs0 and dfs are then not read)
  float fs0, dfs;     // fs of cameras[view], and fs of camera_close minus it
  uint32_t pad[3];
};
static_assert(sizeof(ViewShutterRec) == 80 && sizeof(ViewShutterRec) % 16 == 0, "ViewShutterRec is five 16-byte scalar loads");

struct RenderArgs {
  const uint32_t* tiles;  // owned wave tiles: x0 | y0 << 16 (pixels, top-left corner)
  uint32_t n_tiles;
  uint32_t width, height, spp, s0, s1, mode, max_depth, seed, k, photons_requested;
  uint32_t flags;         // bit 0: shadow rays through the wave-level pool; bit 1: no leaf of the resident tree holds more
                          // than two records (the launcher's LT_LEAF2 instances)
  uint32_t stackLevels;   // LDS traversal-stack rows (64 words each) per wave: BVH depth + 1; with photons also the kd walk's
                          // pending entries (kd depth + 2: 32-bit, or two 16-bit entries per word when kd16)
  uint32_t kd16;          // the k-NN walk keeps 16-bit stack entries (fewer than 65,535 photons)
  uint32_t sshift;        // a wave = (64 >> sshift) pixels x (1 << sshift) samples side by side
  uint32_t tileW, tileH;  // pixel footprint of one wave (tileW * tileH == 64 >> sshift)
  uint32_t tilesPerBlock; // one-wave-per-workgroup kernels (k_render): consecutive wave tiles a workgroup renders (launcher)
  // persistent pooled kernel (k_render_persist)
  uint32_t* tileCounter;  // next wave tile to hand out (zeroed before the launch)
  uint32_t waveWords;     // LDS words per wave (stack levels x 64 + pool), set by the launcher
  uint32_t numCUs;        // workgroups to launch (one per CU)
  // multi-view frames (rt_render_views): the view of each wave tile (an index into views, parallel to tiles) and the
  // views' records; null: one view, S.cam, seed and accum as given
  const uint32_t* tileView;
  const ViewRec* views;
  // multi-view shutter frames (rt_render_views_shutter): the views' shutter records, indexed as views; else null
  const ViewShutterRec* viewShutters;
  // the fine tail of a plain single-view frame's list (k_render_persist): items [fineFrom, n_tiles) are the last coarse
  // tiles' pixels again at sshiftFine >= sshift — more samples of fewer pixels side by side, so shorter items — for the
  // end of the launch, where every wave is inside its last item.  fineFrom == n_tiles: none (every other launch).
  uint32_t fineFrom = ~0u, sshiftFine = 0;
};

// Waves the device holds at once if launch_render runs this frame in k_render_persist, the kernel that takes a fine tail;
// 0 if it runs in another kernel (k_render, k_render_persist5, k_render_wide), whose lists have none.
uint32_t persist_fine_waves(bool brute_force, bool photon, const DevScene& S, const RenderArgs& A);
hipError_t launch_render(bool brute_force, bool photon, bool stats, const DevScene& S, const RenderArgs& A,
                         float4* accum, unsigned long long* counters, hipStream_t stream);
hipError_t launch_resolve(uint32_t n_pixels, uint32_t spp, const float4* accum, const float* bg, float* out,
                          hipStream_t stream);
// The wavefront integrator (wavefront.hip): path state of one batch, SoA in HBM
struct WfArgs {
  const uint32_t* gran;  // owned 8x8 granules (x8 | y8 << 16), row-major: path = (sample slot, granule, pixel)
  uint32_t nGran, width, height, spp, seed;
  uint32_t s0, s1;       // sample range still to do
  uint32_t batch;        // samples per batch
  uint32_t nPaths;       // paths of this batch (set by the launcher)
  uint32_t* rng;         // [P] engine state
  float4 *org, *dir;     // [P] current ray
  uint2* key;            // [P] current hit {t bits, triangle id}; {~0, ~0}: the path has ended
  float4 *nrm, *pnt;     // [P] vertex normal (+ mesh in w), point
  float4* col;           // [3][P] vertex colours; col[0].w: primary hit, col[1].w: slot holds a sample
  float4 *rayO, *rayD;   // [4P] ray queue
  uint2* res;            // [4P] results
  unsigned long long* stripes;  // [1024][2] striped ray counters (closest, shadow), zero between frames
};
hipError_t launch_wavefront(const DevScene& S, const WfArgs& W, uint32_t mode, uint32_t maxDepth, float4* accum,
                            unsigned long long* counters, uint32_t* queueCounter, uint32_t stackLevels, uint32_t numCUs,
                            hipStream_t stream);
// first-hit AOVs of a frame's primary rays (aov_kernels.h, rt_render_aov): sums over the samples [s0, s1) of every pixel;
// null channels are not written
struct TexDesc;  // (with TexRec, among the frame's variants below)
struct AovArgs {
  float *albedo, *normal, *position, *depth;  // [h][w][3], [h][w][3], [h][w][3], [h][w]
  uint32_t *hits, *mesh, *tri;                // [h][w] each
  uint32_t width, height, spp, seed, s0, s1;
  // multi-view launches only (launch_aov sets them; the single-view instances do not read them)
  const ViewRec* views = nullptr;
  uint32_t tilesPerView = 0;
  // coloured launches only (launch_aov sets it; the other instances do not read it)
  const float* vcol = nullptr;
  // textured launches only (launch_aov sets them; the other instances do not read them): TexRec's four tables
  const float* texUv = nullptr;
  const uint32_t* texMesh = nullptr;
  const TexDesc* texDesc = nullptr;
  const float* texels = nullptr;
};
// (launch_aov: below FrameVariant, whose surface part says what the albedo channel sums)
// ambient occlusion and bent normals at the first hit (ao_kernels.h, rt_render_ao): per pixel, over the samples [s0, s1),
// the occlusion rays that escaped, the hit samples, and the float32 sum of the escaped directions; null channels are not written
struct AoArgs {
  uint32_t *unoccluded, *hits;  // [h][w] each
  float* bent;                  // [h][w][3]
  uint32_t width, height, spp, seed, s0, s1;
  uint32_t nRays;               // occlusion rays per primary hit
  float bias;                   // 0: 1e-4 of the diagonal of the box in ext
  float maxDistance;            // 0: unbounded
  const uint32_t* ext;          // the referenced vertices' box as launch_ref_extent leaves it (read when bias == 0)
};
hipError_t launch_ao(bool brute_force, const DevScene& S, const AoArgs& A, hipStream_t stream);
// the integrator over a batch of the caller's rays (rays_kernels.h, rt_render_rays): row r of accum gains the samples
// [s0, s1) of ray r, whose RNG stream is keyed by streamIndex[r] (null: r)
struct RaysArgs {
  const rt_ray* rays;           // [n], device memory; directions of any length
  const uint32_t* streamIndex;  // [n] or null
  uint32_t n;                   // 1 .. 2^31 - 1
  uint32_t spp, s0, s1, mode, max_depth, seed;
  uint32_t flags;               // bit 0: shadow and bounce rays through the wave-level pool (RenderArgs::flags)
  uint32_t stackLevels;         // LDS traversal-stack rows per wave (RenderArgs::stackLevels)
};
hipError_t launch_render_rays(bool brute_force, bool stats, const DevScene& S, const RaysArgs& A, float4* accum,
                              unsigned long long* counters, hipStream_t stream);
// ---- the frame's generator variants (frame_variants.h): the frame integrator with another generator or another split of
// its samples.  What a variant's kernels read beyond the frame's arguments travels as one record, by value.
// the frame through a thin lens (rt_render_lens): the host-derived constants of rt_amd.h.
// aperture == 0: the frame's own camera_ray (a wave-uniform test on the record), the other fields are not read.
struct LensRec {
  float aperture, fs;  // lens radius; focus_distance / distance of the image plane
  float hu[3], vu[3];  // unit3(cam.horizontal), unit3(cam.vertical)
};
// the frame under an open shutter (rt_render_shutter): the host-derived constants of rt_amd.h.  The camera of a sample
// is S.cam + t d, t drawn in [open, close]; aperture > 0 puts rt_render_lens' lens on it.
struct ShutterRec {
  float d[12];          // camera_close - the context's camera, component by component (position, lower_left, H, V)
  float open, close;    // the exposure: t = uniformF(open, close)
  float aperture;       // lens radius, 0 = pinhole (fs0 and dfs are then not read)
  float fs0, dfs;       // fs of the context's camera, and fs of camera_close minus it
};
// the frame split by light group (rt_render_lights): rt_light_groups' count and masks — a kernel argument, so every
// mask test is a scalar one.  masks[g] is 0 for g >= n.
struct LightGroupsRec {
  uint32_t n;
  uint32_t masks[RT_LIGHT_GROUPS_MAX];
};
// the frame with sampled direct lighting (rt_render_pick): every sample picks m of the context's n lights by the host's
// threshold table and shades all of its vertices with those, each scaled by 1 / (m p_k) on the host.  PickLight is
// rt_light padded to 24 floats: the index differs from lane to lane, so a lane fetches its light in 16-byte vector loads
// (the table stays cache-resident).  Both tables are device memory that the launch reads in stream order.
struct alignas(16) PickLight {
  rt_light l;  // L_k with color[c] = w_k * color[c]
  float pad[3];
};
static_assert(sizeof(PickLight) == 96, "PickLight is six 16-byte loads");
struct PickRec {
  uint32_t m, n;            // light samples per path vertex (1..RT_PICK_SLOTS_MAX); the context's light count
  const float* thresholds;  // [n] t_k = (float)C_k, 1.0f from the last light with q_k > 0 onwards: pick(u) = the smallest k with u < t_k
  const PickLight* lights;  // [n]
};
// the frame with per-vertex albedo (rt_render_colors): every shaded vertex takes its material's albedo from the colours of
// the hit triangle's three vertices (rt_amd.h's interpolation); the array is device memory the launch reads in stream
// order, gathered per lane by vertex id as the normals are.
struct VColRec {
  const float* vcol;  // [n_vertices][3]
};
// the frame with image-textured albedo (rt_render_textured): every shaded vertex of a mesh with a texture takes its
// material's albedo from the texture's sample at the hit's interpolated uv (rt_amd.h's sampler); a mesh whose meshTex
// entry is kTexNone shades with its own material.  All four tables are device memory the launch reads in stream order.
// TexDesc is one 16-byte load: where the texture's texels start in the pool (in texels), its size and its wrap/filter bits.
struct alignas(16) TexDesc {
  uint32_t offset, width, height, bits;  // bits: TEX_CLAMP_S | TEX_CLAMP_T | TEX_BILINEAR
};
constexpr uint32_t TEX_CLAMP_S = 1u, TEX_CLAMP_T = 2u, TEX_BILINEAR = 4u;
constexpr uint32_t kTexNone = 0xffffffffu;  // RT_TEX_NONE
struct TexRec {
  const float* uv;           // [n_vertices][2]
  const uint32_t* meshTex;   // [n_meshes]: an index into desc, or kTexNone
  const TexDesc* desc;       // [n_textures]
  const float* texels;       // the pool: every texture's [height][width][3], one behind the other
};
// the frame with textured material maps (rt_render_material): TexRec's frame in which, beside the albedo, f0 and
// (kd, alpha) of every shaded vertex come from textures of the same set, sampled at the same hit coordinate: meshF0's
// texture gives f0 from its rgb, meshKdAlpha's gives kd from r and alpha from g (b is not read); kTexNone keeps the mesh's
// own.  The first four pointers are TexRec's; the two tables are device memory the launch reads in stream order.
struct MatRec {
  const float* uv;              // [n_vertices][2]
  const uint32_t* meshTex;      // [n_meshes]: the albedo's texture, or kTexNone
  const TexDesc* desc;          // [n_textures]
  const float* texels;          // the pool
  const uint32_t* meshF0;       // [n_meshes]: f0's texture, or kTexNone
  const uint32_t* meshKdAlpha;  // [n_meshes]: (kd, alpha)'s texture, or kTexNone
};
// the frame with tangent-space normal maps (rt_render_normal_mapped): MatRec's frame (mat: its six fields; a context
// without resident material maps passes tables of kTexNone for the last two) in which the shading normal of every shaded
// vertex of a mesh with a normal map is turned by the map's sample at the same hit coordinate, in the tangent frame formed
// from the triangle's current positions and uvs (rt_amd.h's operations); kTexNone keeps the interpolated normal.
struct NrmRec {
  MatRec mat;
  const uint32_t* meshNormal;  // [n_meshes]: the normal map's texture, or kTexNone
};
// Which variant a frame is: a generator part (what forms its primary rays, splits its samples or lists its lights) and
// a surface part (what its vertices shade with), with the one record of the pair (which the caller keeps alive over the
// launch call): the generator's LensRec, ShutterRec, LightGroupsRec or PickRec, or the surface's VColRec, TexRec,
// MatRec or NrmRec.  VIEWS_SHUTTER, many views each under its own open shutter (rt_render_views_shutter), has no record of its own
// — tile t renders with views[tileView[t]]'s camera, seed and slice under viewShutters[tileView[t]], from RenderArgs'
// three tables — so it carries a surface's.
struct FrameVariant {
  enum Gen { PLAIN, LENS, SHUTTER, LIGHTS, PICK, VIEWS_SHUTTER };
  enum Surface { NONE, VCOL, TEX, MAT, NMAP };
  Gen gen = PLAIN;
  Surface surface = NONE;
  const void* rec = nullptr;
  FrameVariant() = default;
  FrameVariant(const LensRec& r) : gen(LENS), rec(&r) {}
  FrameVariant(const ShutterRec& r) : gen(SHUTTER), rec(&r) {}
  FrameVariant(const LightGroupsRec& r) : gen(LIGHTS), rec(&r) {}
  FrameVariant(const PickRec& r) : gen(PICK), rec(&r) {}
  FrameVariant(const VColRec& r) : surface(VCOL), rec(&r) {}
  FrameVariant(const TexRec& r) : surface(TEX), rec(&r) {}
  FrameVariant(const MatRec& r) : surface(MAT), rec(&r) {}
  FrameVariant(const NrmRec& r) : surface(NMAP), rec(&r) {}
  // F's surface under the multi-view shutter's generator (rt_render_views_shutter_albedo; a plain F: the multi-view
  // shutter frame itself), with RenderArgs' three tables
  static FrameVariant under_views_shutter(FrameVariant F) {
    F.gen = VIEWS_SHUTTER;
    return F;
  }
  explicit operator bool() const { return gen != PLAIN || surface != NONE; }
  // the variant in an error message: "<name> render launch failed"
  std::string name() const {
    static const char* const gens[] = {"", "lens", "shutter", "light-group", "light-pick", "multi-view shutter"};
    static const char* const surfaces[] = {"", "vertex-colour", "textured", "material-map", "normal-mapped"};
    return std::string(gens[gen]) + (gen != PLAIN && surface != NONE ? " " : "") + surfaces[surface];
  }
};
// launch_render's one-wave-per-workgroup family (brute, sequential, pooled; counted or timed) for a variant F (not the
// plain frame, which is launch_render's).  The pairs that exist: every generator without a surface, every surface under
// the plain generator, and VCOL and TEX under VIEWS_SHUTTER; hipErrorInvalidValue for every other pair, and where A, the
// record or the scene's light count do not fit the variant.
// The generator decides what A is: launch_render's with tileView null, but for VIEWS_SHUTTER a multi-view frame's with
// the three tables set.  LIGHTS: accum is [G.n][height][width], slice g at accum + g * width * height.  PICK: pooled
// whenever A.flags bit 0 is set, whatever the scene's light count (a vertex sends m <= POOL_L shadow rays).
// The surface decides the LDS a launch allocates per wave beyond the generator's: the rows its policy parks a vertex's
// value in (VCOL and TEX three, the kdDiffuse; MAT and NMAP eight, the material).
hipError_t launch_render_variant(const FrameVariant& F, bool brute_force, bool stats, const DevScene& S, const RenderArgs& A,
                                 float4* accum, unsigned long long* counters, hipStream_t stream);
// The AOV pass.  views null: the frame of S.cam and A.seed; else the same pass over nViews views in one launch
// (rt_render_aov_views): view j renders with views[j]'s camera and seed (A.seed is not read) into slice j of every channel.
// surface (its surface part alone is read): what the albedo channel sums at the first hit — NONE the mesh's albedo, VCOL
// the colour interpolated from the VColRec's array (rt_render_aov_colors), TEX the TexRec's texture sample, or the mesh's
// albedo on a mesh without a texture (rt_render_aov_textured); instances of their own each.  hipErrorInvalidValue for a
// record with a null table, for MAT, and for views of 2^31 tiles or more together; an empty launch is a success.
hipError_t launch_aov(bool brute_force, const DevScene& S, const AovArgs& A, const ViewRec* views, uint32_t nViews,
                      const FrameVariant& surface, hipStream_t stream);
// First element of view j's slice of a per-view output with c floats or words per pixel (rt_render_aov_views,
// rt_render_motion_views, rt_denoise_batch): formed in 64 bits — n w h may reach 2^31 - 1 and 3 x that is not 32-bit.
__host__ __device__ inline size_t view_slice(uint32_t j, uint32_t width, uint32_t height, uint32_t c) {
  return (size_t)j * width * height * c;
}
// the motion pass (motion_kernels.h, rt_render_motion): per pixel, for the primary ray of sample s0, the hit point over the
// context's positions and over prevVpos (never null: the context's own when the geometry did not move), and the screen
// motion between prevCam and S.cam; null channels are not written
struct MotionArgs {
  float *motion, *position, *prevPosition;  // [h][w][2], [h][w][3], [h][w][3]
  uint32_t* mesh;                           // [h][w]
  const float* prevVpos;                    // [n_vertices][3]
  rt_camera prevCam;
  uint32_t width, height, spp, seed, s0;
  // multi-view launches only (launch_motion_views sets them; the single-view instances do not read them)
  const ViewRec* views = nullptr;
  const rt_camera* prevCams = nullptr;
  uint32_t tilesPerView = 0;
};
hipError_t launch_motion(bool brute_force, const DevScene& S, const MotionArgs& A, hipStream_t stream);
// the same pass over nViews views in one launch (rt_render_motion_views): view j with views[j]'s camera and seed and
// prevCams[j] as last frame's camera (a device table of its own: ViewRec stays 64 bytes) into slice j of every channel
hipError_t launch_motion_views(bool brute_force, const DevScene& S, const MotionArgs& A, const ViewRec* views, const rt_camera* prevCams,
                               uint32_t nViews, hipStream_t stream);
// adaptive sampling (adaptive.hip, rt_render_adaptive): per-pixel running moments and per-granule pass counts, the
// compaction of the active granules into the next pass's wave tiles, and the resolve with per-pixel sample counts
enum { ADAPT_CNT_GRANULES = 0, ADAPT_CNT_PIXELS = 1, ADAPT_CNT_TILES = 2, ADAPT_CNT_WORDS = 16 };  // counts[2 + sshift]
struct AdaptArgs {
  uint32_t width, height, gx, gy;  // image; granules per row / column
  uint32_t P;                      // samples per pass
  uint32_t minPasses;              // passes before a pixel may converge (>= 2 applied on the device)
  float threshold, floor;          // the retirement rule (threshold 0: never)
  const float4* accum;             // [h][w] the frame's accumulator
  const float* bg;                 // [h][w][3]
  float4* prev;                    // [h][w] accum after the previous pass
  double2* mom;                    // [h][w] {S1, S2}
  uint32_t* passes;                // [granules] passes run
  uint32_t* retired;               // [granules] 1 = retired
  uint32_t* list;                  // [granules] the active granules (x8 + y8 * gx), row-major
  uint32_t* tiles;                 // [granules * 64] their wave tiles (x0 | y0 << 16)
  uint32_t* counts;                // [ADAPT_CNT_WORDS]
};
// list + counts from retired (one workgroup)
hipError_t launch_adapt_compact(const AdaptArgs& A, hipStream_t stream);
// tiles from the first nAct entries of list for a wave footprint tw x th (one workgroup)
hipError_t launch_adapt_expand(const AdaptArgs& A, uint32_t nAct, uint32_t tw, uint32_t th, hipStream_t stream);
// the rule over the first nAct entries of list after a pass: moments, passes, retired
hipError_t launch_adapt_update(const AdaptArgs& A, uint32_t nAct, hipStream_t stream);
// out = k_resolve's expression with spp = passes[granule] * P per pixel; spp (may be null) = that count
hipError_t launch_resolve_adaptive(const AdaptArgs& A, float* out, uint32_t* spp, hipStream_t stream);
// ray queue in HBM -> results (wavefront stage T)
hipError_t launch_trace_stream(const DevScene& S, const float4* rayO, const float4* rayD, uint32_t n, uint2* res,
                               uint32_t* counter, uint32_t stackLevels, uint32_t numCUs, hipStream_t stream);
// multi-GPU frame assembly: pack (unpack = false) a rank's owned granules out of a full-frame
// accumulator, or scatter a packed buffer back into one
hipError_t launch_pack(bool unpack, const float4* src, float4* dst, const uint32_t* gran, uint32_t n, uint32_t width,
                       uint32_t height, hipStream_t stream);
hipError_t launch_trace(bool brute_force, bool any, const DevScene& S, const rt_ray* rays, uint32_t n,
                        rt_hit* hits, unsigned long long* counters, hipStream_t stream);
// the photon frames' k-NN walk (knn_query<kd16>) on their layout: stackLevels rows of LDS stack, the k-slot heap above
hipError_t launch_knn(const DevScene& S, const float* q, uint32_t n, uint32_t k, bool kd16, uint32_t stackLevels,
                      uint32_t* idx, float* dist, uint32_t* visited, hipStream_t stream);
// the same for k in 1..RT_KNN_KMAX: k <= RTK_KMAX runs launch_knn's instance, larger k the wide frames' walk on their layout
hipError_t launch_knn_wide(const DevScene& S, const float* q, uint32_t n, uint32_t k, bool kd16, uint32_t stackLevels,
                           uint32_t* idx, float* dist, uint32_t* visited, hipStream_t stream);
hipError_t launch_emit(const DevScene& S, uint32_t perLight, uint32_t seed, float4* outPos, float4* outDir,
                       unsigned long long* counters, hipStream_t stream);
// scene BVH on the device (bvh_gpu.hip): arrays are hipMalloc'ed by the builder, owned by the caller
struct GpuBvh {
  uint4* nodes16 = nullptr;   // n_nodes x 32 B (what the kernels traverse)
  float4* nodesF = nullptr;   // n_nodes x 64 B (rtbvh::Node: inspection / export)
  float4* tris = nullptr;     // leaf order
  float4* trisRef = nullptr;  // reference order
  uint32_t n_nodes = 0, maxDepth = 0;
};
// the exact build: the host builder's split rules as kernels above the exact subtrees (hSizeKey: rtbvh::planSceneExact)
hipError_t gpu_bvh_build_exact(const float* dVpos, const uint4* dTriShade, const float* hSizeKey, uint32_t n_tris, const rtbvh::ScenePlan& plan,
                               GpuBvh* out, hipStream_t stream);
// the hybrid build: the host builder's top (rtbvh::buildTop), exact subtrees of its parts on the device
hipError_t gpu_bvh_build_over_top(const float* dVpos, const uint4* dTriShade, const float* hSizeKey, uint32_t n_tris, const rtbvh::TopBuilt& top,
                                  GpuBvh* out, hipStream_t stream);
// refit of a built tree to new vertex positions (bvh_gpu.hip, rt_update): dOut3 = max |x| bits of the positions the
// triangles reference, of all positions, of all normals (0 where pos / nrm is null; NaN and infinities compare above every
// finite value); the depth of every node (*maxDepthOut = the deepest; synchronises); and the refit itself — records: the
// triangle records in both orders anew from dVpos — then every box bottom-up, one launch per depth, and the packed records
// with boxScale (slot order, refs and numbering untouched)
hipError_t launch_magnitudes(const float* dPos, const float* dNrm, const uint4* dTriShade, uint32_t nTris, uint32_t nVerts,
                             uint32_t* dOut3, hipStream_t stream);
// rt_update_transforms: dOutPos / dOutNrm = the rest arrays under the per-mesh records of dTable (rt_amd.h's arithmetic;
// RT_XF_STATIC meshes copied), and dOut3 = launch_magnitudes' three words of the result, positions and normals folded in
// the same pass.  The out arrays must not alias the rest arrays.
hipError_t launch_transform(const float* dRestPos, const float* dRestNrm, const rt_mesh_transform* dTable, const uint32_t* dMeshVtxBegin,
                            uint32_t nMeshes, uint32_t nVerts, float* dOutPos, float* dOutNrm, const uint4* dTriShade, uint32_t nTris,
                            uint32_t* dOut3, hipStream_t stream);
// rt_update_skin: dOutPos / dOutNrm = the rest arrays blended under the bone records of dTable by the resident skin
// (dBone [nVerts][4] indices into dTable, dWeight [nVerts][4], both 16-byte aligned; rt_amd.h's arithmetic, vertices of
// four zero weights copied), and dOut3 as launch_transform's.  The out arrays must not alias the rest arrays.
hipError_t launch_skin(const float* dRestPos, const float* dRestNrm, const uint16_t* dBone, const float* dWeight,
                       const rt_mesh_transform* dTable, uint32_t nVerts, float* dOutPos, float* dOutNrm, const uint4* dTriShade,
                       uint32_t nTris, uint32_t* dOut3, hipStream_t stream);
hipError_t gpu_bvh_depths(const float4* nodesF, uint32_t n, uint8_t* dDepth, uint32_t* maxDepthOut, hipStream_t stream);
hipError_t gpu_bvh_refit(const float* dVpos, const uint4* dTriShade, uint32_t nTris, bool records, float4* tris, float4* trisRef,
                         float4* nodesF, uint4* nodes16, uint32_t nNodes, const uint8_t* dDepth, uint32_t maxDepth, float pad,
                         float boxScale, hipStream_t stream);
// the surface-area cost of a resident tree (rt_bvh_quality_get): dOut2 = {sum over inner slots of A / A_root, sum over leaf
// slots of cnt A / A_root} in double, through dPartial (2 x kQualityPartials doubles, 16-byte aligned as dOut2); the same
// records give the same bits (fixed summation shape, no atomics)
constexpr uint32_t kQualityPartials = 1024;
hipError_t gpu_bvh_quality(const float4* nodesF, uint32_t nNodes, double* dPartial, double* dOut2, hipStream_t stream);
// photon map on the device (kd_build.hip)
hipError_t launch_photon_compact(const float4* slots, uint32_t n, float4* items, uint32_t* count, hipStream_t stream);
hipError_t launch_kd_build(float4* items, uint32_t n, int depthOverride, hipStream_t stream);
// explicit child / parent-split records of the median-implicit tree over phPos (what knn_query walks)
hipError_t launch_kd_topology(const float4* phPos, uint32_t n, uint4* topo, hipStream_t stream);
hipError_t launch_photon_gather(const float4* items, const float4* slotDir, uint32_t n, float4* phPos, float4* phDir,
                                uint32_t* perm, hipStream_t stream);
hipError_t launch_unit(uint32_t which, const void* in, void* out, uint32_t n, hipStream_t stream);
// *dBad (zeroed by the caller) != 0 afterwards: rtd::recip_fast / sqrt_fast differ from the division / sqrtf on this device
hipError_t launch_selfcheck_recip(uint32_t* dBad, hipStream_t stream);

}  // namespace rtk
