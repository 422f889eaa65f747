// rt_api.cpp — the C ABI declared in include/rt_amd.h: context lifetime, HBM
// residency of the flattened scene, launch orchestration.  All arithmetic of the
// hot path lives in rt_kernels.hip; nothing here computes radiance on the host
// and nothing falls back to the CPU when a device is missing.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "bvh_build.h"
#include "filters.h"
#include "material_maps.h"
#include "normal_maps.h"
#include "rt_amd.h"
#include "rt_kernels.h"
#include "wave_tiles.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(RT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Picks the device and refuses anything that is not a gfx950 part.
int select_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(RT_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(RT_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, n - 1);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(RT_ERR_NO_DEVICE, "device %d is %s; kernels are built for gfx950 only", device, prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  return RT_OK;
}

// Owners of device memory, events and streams.  Where a failed hipFree must be reported, the caller
// releases the owner and checks: HIP_TRY(hipFree(p.release())).
struct HipFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
template <class T>
using DevBuf = std::unique_ptr<T, HipFree>;
struct HipHostFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};
template <class T>
using PinnedBuf = std::unique_ptr<T, HipHostFree>;
struct EventDestroy {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
struct StreamDestroy {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

template <class T>
hipError_t dev_alloc(DevBuf<T>* out, size_t count) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, count * sizeof(T));
  out->reset(e == hipSuccess ? static_cast<T*>(p) : nullptr);
  return e;
}
hipError_t make_event(Event* out, unsigned flags = hipEventDefault) {
  hipEvent_t e = nullptr;
  const hipError_t r = hipEventCreateWithFlags(&e, flags);
  out->reset(r == hipSuccess ? e : nullptr);
  return r;
}
hipError_t make_stream(Stream* out) {
  hipStream_t s = nullptr;
  const hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  out->reset(r == hipSuccess ? s : nullptr);
  return r;
}

// A device copy of count elements of src (none when count is 0)
template <class T>
int upload(DevBuf<T>* out, const void* src, size_t count) {
  out->reset();
  if (count == 0) return RT_OK;
  HIP_TRY(dev_alloc(out, count));
  HIP_TRY(hipMemcpy(out->get(), src, count * sizeof(T), hipMemcpyHostToDevice));
  return RT_OK;
}

template <class T>
hipError_t pinned_alloc(PinnedBuf<T>* out, size_t count) {
  void* h = nullptr;
  const hipError_t e = hipHostMalloc(&h, count * sizeof(T));
  out->reset(e == hipSuccess ? static_cast<T*>(h) : nullptr);
  return e;
}

// Scratch that grows on demand: *buf gets room for `need` elements when *cap is less (*grew says whether it did).  *cap is
// 0 while there is no valid buffer; a device buffer is freed first and a failing hipFree reported, a pinned one goes once
// its successor is there.
template <class T>
int renew(DevBuf<T>* buf, size_t count) {
  if (*buf) HIP_TRY(hipFree(buf->release()));
  HIP_TRY(dev_alloc(buf, count));
  return RT_OK;
}
template <class T>
int renew(PinnedBuf<T>* buf, size_t count) {
  HIP_TRY(pinned_alloc(buf, count));
  return RT_OK;
}
template <class Owner, class Cap>
int grow(Owner* buf, Cap* cap, size_t need, bool* grew = nullptr) {
  const bool g = need > *cap;
  if (grew) *grew = g;
  if (!g) return RT_OK;
  *cap = 0;
  const int rc = renew(buf, need);
  if (rc != RT_OK) return rc;
  *cap = static_cast<Cap>(need);
  return RT_OK;
}

// Device copies of a host form's buffers, freed with the scope.  in() uploads an input; out() makes room for an output
// the caller asked for (null otherwise); work() makes room the device form needs either way and zeroed() fills it with
// zeros (an integrator's accumulator); inout() uploads what the device form updates in place.  download() copies back
// every one of these whose host pointer was given, in() apart.  After a failure they all answer null and rc holds what the
// entry point returns; it is looked at once, after the last of them.
struct Staging {
  struct Out {
    void* host;
    const void* dev;
    size_t bytes;
  };
  std::vector<DevBuf<char>> bufs;
  std::vector<Out> outs;
  int rc = RT_OK;

  int stage(void** d, const void* src, void* dst, size_t bytes, bool zero) {
    DevBuf<char> b;
    HIP_TRY(dev_alloc(&b, bytes));
    if (src) HIP_TRY(hipMemcpy(b.get(), src, bytes, hipMemcpyHostToDevice));
    if (zero) HIP_TRY(hipMemset(b.get(), 0, bytes));
    *d = b.get();
    bufs.push_back(std::move(b));
    if (dst) outs.push_back({dst, *d, bytes});
    return RT_OK;
  }
  template <class T>
  T* staged(const void* src, void* dst, size_t count, bool zero = false) {
    void* d = nullptr;
    if (rc == RT_OK) rc = stage(&d, src, dst, count * sizeof(T), zero);
    return static_cast<T*>(d);
  }
  template <class T>
  T* in(const T* host, size_t count) { return staged<T>(host, nullptr, count); }
  template <class T>
  T* out(T* host, size_t count) { return host ? staged<T>(nullptr, host, count) : nullptr; }
  template <class T>
  T* work(void* host, size_t count) { return staged<T>(nullptr, host, count); }
  template <class T>
  T* zeroed(void* host, size_t count) { return staged<T>(nullptr, host, count, true); }
  template <class T>
  T* inout(void* host, size_t count) { return staged<T>(host, host, count); }
  int download() {
    for (const Out& o : outs) HIP_TRY(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    return RT_OK;
  }
};

// A list of words that the host makes and kernels read (wave tiles, granules), sent on the CALLER's stream through a pinned
// copy that lives as long as the device copy.  upload() would not do on the asynchronous paths: its blocking copy runs on
// the null stream, and the runtime multiplexes streams onto a few hardware queues — when the null stream and the caller's
// share one, the copy waits for everything the caller has queued (DESIGN.md "Stream order").  `ready` is recorded behind
// the copy: a launch that reads the list on another stream waits for it on the device (use_on).
struct StreamList {
  DevBuf<uint32_t> d;
  PinnedBuf<uint32_t> h;
  Event ready;
  hipStream_t on = nullptr;
  uint32_t n = 0;
};
// (releases what L held: hipFree waits for the launches that may still read it)
int stream_upload(StreamList* L, const std::vector<uint32_t>& v, hipStream_t stream) {
  L->n = 0;
  if (L->d) {
    HIP_TRY(hipEventSynchronize(L->ready.get()));  // the copy has read the pinned words
    HIP_TRY(hipFree(L->d.release()));
  }
  L->h.reset();
  if (v.empty()) return RT_OK;
  HIP_TRY(dev_alloc(&L->d, v.size()));
  HIP_TRY(pinned_alloc(&L->h, v.size()));
  memcpy(L->h.get(), v.data(), v.size() * sizeof(uint32_t));
  if (!L->ready) HIP_TRY(make_event(&L->ready, hipEventDisableTiming));
  HIP_TRY(hipMemcpyAsync(L->d.get(), L->h.get(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(L->ready.get(), stream));
  L->on = stream, L->n = static_cast<uint32_t>(v.size());
  return RT_OK;
}
int use_on(const StreamList& L, hipStream_t stream) {
  if (L.d && stream != L.on) HIP_TRY(hipStreamWaitEvent(stream, L.ready.get(), 0));
  return RT_OK;
}

using rtl::owned_granules;
using rtl::TileKey;
using rtl::wave_tile_shape;
using rtl::wave_tiles;

constexpr int kEventPairs = 256;

}  // namespace

// Releasing a context frees everything it owns on the current device: rt_destroy selects the context's first.
struct rt_ctx {
  int device = 0;
  rtk::DevScene S{};  // the kernels' argument: views of the buffers below
  rtbvh::Built bvh;  // host copy kept for rt_bvh_export
  // the scene's arrays (S's fields of the same names)
  DevBuf<uint4> triShade, nodes, q8;
  DevBuf<float> vpos, vnrm;
  DevBuf<float4> tris, trisRef;
  DevBuf<rt_material> mats;
  DevBuf<rtd::DevMat> matsDev;
  DevBuf<rt_light> lights;
  DevBuf<uint32_t> meshTriBegin, meshVtxBegin;
  // device-built BVH (rt_options.bvh_builder / RT_BVH_GPU): the float form of the nodes stays
  // on the device for rt_bvh_export
  DevBuf<float4> nodesF;
  // the photon map (install_photons / drop_photons)
  DevBuf<float4> phPos, phDir;
  DevBuf<uint4> phTopo;  // explicit kd topology over phPos (rtk::launch_kd_topology)
  StreamList tiles;  // the frame's wave tiles, for tileKey
  TileKey tileKey;
  uint32_t tilesFineFrom = 0;  // index of the list's first fine item (== tiles.n: none)
  DevBuf<unsigned long long> dCounters;
  DevBuf<uint32_t> dTileCounter;  // work queue head of the persistent render kernel
  // owned-granule lists of the ranks of a tile-sharded frame (multi-GPU assembly), by key
  using GranList = StreamList;
  std::map<std::string, GranList> granules;
  // path state + ray queues of the wavefront integrator (allocated on first use)
  rtk::WfArgs wf{};
  size_t wfCap = 0;  // bytes of wfBlock
  DevBuf<char> wfBlock;
  uint32_t builder = RT_BVH_HOST;
  bool broken = false;  // the device tree is in an unknown state (rt_bvh_tune could not restore it, rt_update failed partway): launches are refused
  uint32_t recipCheck = 0;  // 0: short reciprocal forms not wanted (operand bounds), 1: verified on this device, 2: self-check FAILED (dividing)
  uint32_t nodeFormat = RT_NODES_F16;  // what the pooled render kernel and rt_trace traverse
  float buildMs = 0.f;
  uint32_t numCUs = 0;
  Event ev[kEventPairs][2];
  int evUsed = 0;
  // what the rules of rt_update read besides the scene's arrays (the camera is S.cam): the lights, and the magnitude
  // summaries — max |x| bits of the positions the triangles reference (the padding rule), of all positions and of all
  // normals (vouch_short_forms)
  std::vector<rt_light> hostLights;
  uint32_t nMeshes = 0, nVertices = 0;
  uint32_t magRef = 0, magPos = 0, magNrm = 0;
  // refit state (rt_update, allocated on first use): the depth of every node of nodesF (a host-built tree's nodes are
  // uploaded to nodesF then and kept), and scratch for host-given arrays and the magnitude read-back
  DevBuf<uint8_t> refitDepth;
  uint32_t refitMaxDepth = 0;
  // rt_rebuild builds under the rt_options the context was created with
  uint32_t optLeafMax = 0, optBuilder = RT_BVH_AUTO, optNodeFormat = RT_NODES_AUTO;
  // rt_bvh_quality_get: the cost of the tree as last built (taken before the first refit that follows a build, or at the
  // first quality call), the refits since, and the reduction's block (2 x kQualityPartials partial sums, then the pair of
  // the tree as it is and the pair of the baseline; allocated on first use)
  double costBuilt = 0.0;
  bool costBuiltValid = false;
  uint32_t refits = 0;
  DevBuf<double> dQuality;
  DevBuf<float> updPos, updNrm;
  DevBuf<uint32_t> dMag;
  // rt_update_transforms (allocated on first use): the rest pose — a snapshot of vpos / vnrm taken at the first transforms
  // call after a call that gave vertex arrays (restValid) — and the per-mesh records
  DevBuf<float> restPos, restNrm;
  bool restValid = false;
  DevBuf<rt_mesh_transform> xfTable;
  // rt_set_skin / rt_update_skin: the resident skin — [nVertices][4] bone indices and weights, as the caller laid them out —
  // and the table the bone records of a call go to (skinBones of them; 0 = no skin)
  DevBuf<uint16_t> skinBone;
  DevBuf<float> skinWeight;
  DevBuf<rt_mesh_transform> skinTable;
  uint32_t skinBones = 0;
  // rt_set_vertex_colors: the resident [nVertices][3] colours that rt_render_colors and rt_render_aov_colors interpolate
  // (null: none); nothing else reads them, and no update touches them
  DevBuf<float> vcol;
  // rt_set_textures: the resident texture set that rt_render_textured and rt_render_aov_textured sample (texels null:
  // none) — the uvs by global vertex id, every mesh's texture index, one descriptor per texture and the texel pool;
  // nothing else reads them, and no update touches them
  struct TexSet {
    DevBuf<float> uv, texels;
    DevBuf<uint32_t> meshTex;
    DevBuf<rtk::TexDesc> desc;
    explicit operator bool() const { return (bool)texels; }
    rtk::TexRec rec() const { return rtk::TexRec{uv.get(), meshTex.get(), desc.get(), texels.get()}; }
    // how many sets (and releases) this context has seen: every rt_set_textures that replaces or releases moves it on,
    // so that what was checked against one set (rt_set_material_maps' indices) can tell that it has gone
    uint64_t generation = 0;
    uint32_t nTextures = 0;
  } tex;
  // rt_set_material_maps: every mesh's f0 and (kd, alpha) texture index into the set of generation texGeneration (f0
  // null: none); rt_render_material alone reads them, and no update touches them
  struct MatMaps {
    DevBuf<uint32_t> f0, kdAlpha;
    uint64_t texGeneration = 0;
    explicit operator bool() const { return (bool)f0; }
  } matMaps;
  // rt_set_normal_maps: every mesh's normal map, a texture index into the set of generation texGeneration (normal null:
  // none); rt_render_normal_mapped alone reads it, and no update touches it.  noMaps: [nMeshes] RT_TEX_NONE, which that
  // frame reads in place of the two material tables while no material maps are resident (made with the first table)
  struct NrmMaps {
    DevBuf<uint32_t> normal;
    uint64_t texGeneration = 0;
    explicit operator bool() const { return (bool)normal; }
  } nrmMaps;
  DevBuf<uint32_t> noMaps;
  // scratch of rt_denoise_device and rt_svgf_device (rtk::filter_scratch; grows on demand: ensure_filter_scratch)
  DevBuf<float4> dnScratch;
  size_t dnCap = 0;
  // scratch of the motion pass and the temporal accumulation (allocated on first use): last frame's positions as the
  // host form of rt_render_motion uploads them, and the accumulation's own block for its sigma_position (not a part of
  // dnScratch: the accumulation and the denoiser may run on different streams)
  DevBuf<float> mvPrev;
  DevBuf<rtk::FilterBlock> tpScratch;
  // scratch of rt_render_adaptive_device (moments, granule state and lists, tile list, counts; grows on demand)
  DevBuf<char> adScratch;
  size_t adCap = 0;
  // scratch of rt_render_views_device: the view-major wave tiles and their views (for vwKey and vwViews views) and the view
  // records
  StreamList vwTiles, vwTileView;
  uint32_t vwNTiles = 0, vwViews = 0;
  TileKey vwKey;
  DevBuf<rtk::ViewRec> vwRecs;
  uint32_t vwCap = 0;
  // rt_render_motion_views_device: last frame's camera of every view, a table beside vwRecs (ViewRec stays 64 bytes),
  // uploaded ahead of the view records on the same stream
  DevBuf<rt_camera> vwPrevCams;
  uint32_t vwPrevCap = 0;
  // rt_render_views_shutter_device: the shutter record of every view, one more table beside vwRecs, uploaded the same way
  DevBuf<rtk::ViewShutterRec> vwShutters;
  uint32_t vwShutterCap = 0;
  // The pinned copies those uploads read, a ring of kViewStages: a call takes the next slot and waits only for the uploads
  // of the call kViewStages back (`read`: recorded behind the uploads that last read the slot), so back-to-back calls on
  // a busy stream do not wait for one another (DESIGN.md "Stream order")
  struct ViewStage {
    PinnedBuf<rtk::ViewRec> recs;
    PinnedBuf<rt_camera> prevCams;
    PinnedBuf<rtk::ViewShutterRec> shutters;
    uint32_t cap = 0, prevCap = 0, shutterCap = 0;
    Event read;
    bool readSet = false;
  };
  static constexpr uint32_t kViewStages = 4;
  ViewStage vwStage[kViewStages];
  uint32_t vwStageNext = 0;
  // rt_render_ao_device with the default bias (allocated on first use): the box of the referenced vertices, reduced on the
  // call's stream and read by the kernel behind it
  DevBuf<uint32_t> aoExt;
  // scratch of rt_render_rays' host form (grows on demand): the batch's rays and stream indices on the device
  DevBuf<rt_ray> rbRays;
  DevBuf<uint32_t> rbIndex;
  size_t rbCap = 0, rbIndexCap = 0;
  // rt_render_pick (allocated on first use, grows with the light count): the call's table on the device — n PickLight
  // records, then n thresholds — written and read in stream order, and the ring of pinned copies its uploads read
  // (vwStage's rule: a call waits only for the upload of the call kViewStages back)
  DevBuf<char> pkTable;
  size_t pkCap = 0;
  struct PickStage {
    PinnedBuf<char> h;
    size_t cap = 0;
    Event read;
    bool readSet = false;
  };
  PickStage pkStage[kViewStages];
  uint32_t pkStageNext = 0;
};

namespace {

// The device scene forgets the photon map BEFORE it is freed: a failure anywhere after leaves "no photons"
// behind (check_params then refuses use_photons), never dangling pointers.
int drop_photons(rt_ctx* c) {
  c->S.phPos = c->S.phDir = nullptr, c->S.phTopo = nullptr, c->S.n_photons = 0;
  if (c->phPos) HIP_TRY(hipFree(c->phPos.release()));
  if (c->phDir) HIP_TRY(hipFree(c->phDir.release()));
  if (c->phTopo) HIP_TRY(hipFree(c->phTopo.release()));
  return RT_OK;
}
void install_photons(rt_ctx* c, DevBuf<float4> pos, DevBuf<float4> dir, DevBuf<uint4> topo, uint32_t n) {
  c->phPos = std::move(pos), c->phDir = std::move(dir), c->phTopo = std::move(topo);
  c->S.phPos = c->phPos.get(), c->S.phDir = c->phDir.get(), c->S.phTopo = c->phTopo.get(), c->S.n_photons = n;
}
// PhotonMap.h:19-20: lightPdf = 1.f / #lights; photonsPerLS = (int)(n * lightPdf)
uint32_t photons_per_light(uint32_t n_requested, uint32_t n_lights) {
  const float lightPdf = 1.f / static_cast<float>(n_lights);
  return static_cast<uint32_t>(static_cast<int>(static_cast<float>(static_cast<int>(n_requested)) * lightPdf));
}

// How many samples of a pixel one wave integrates side by side.  A pixel's float
// sum must be formed in sample order, but only the ADDS are ordered: the samples
// themselves are independent streams, so the 64 lanes of a wave can hold
// (pixel, sample) pairs and hand their results to the pixel's owner lane, which adds
// them in order.  More samples per wave = more, shorter work items: the grid no longer
// quantises into ~3 rounds of 16k tile-sized items, and a rank that owns 1/8 of the
// pixels still fills the GPU.
// `pixels`: the pixels the launch renders (choose_sshift: the rank's share of the frame; an adaptive pass: its active
// granules' in-image pixels).
// `pick`: a frame of rt_render_pick, whose vertices send m <= 3 shadow rays whatever the context's light count.
uint32_t choose_sshift_px(const rt_ctx* c, const rt_params* p, uint64_t pixels, uint32_t spp_count, bool pick = false) {
  if (p->reserved[0]) {  // explicit lanes-per-pixel (tests, experiments)
    uint32_t s = 0;
    while ((1u << (s + 1)) <= p->reserved[0] && s < 6) ++s;
    return s;
  }
  // measured on C2 (1024^2 x 128 spp), samples per wave 1/2/4/8/16/64:
  // 12.3 / 12.8 / 13.4 / 13.6 / 13.7 / 13.6 Grays/s -> aim for >= 32 rounds of a
  // 256-CU x 16-wave chip
  const uint64_t target = 32ull * 256 * 16;
  uint32_t s = 0;
  while (s < 6 && (pixels << s) / 64 < target && (2u << s) <= spp_count) ++s;
  // The pooled BVH kernel (persistent workgroups: no grid quantisation to balance) wants MORE samples of a pixel side by
  // side than that: their vertices lie close together, so the wave's rays share nodes and triangle lines.  Measured in
  // round 3 (profiles/r03_samples_per_wave.txt), frame ms at 1 / 4 / 8 / 16 / 32 / 64 samples of a pixel per wave:
  // C2 56.1 / 51.2 / 50.4 / 50.3 / 50.6 / 51.4, C4 - / 937.6 / 934.0 / 931.5 / - / 951.8 (the old rule gave it 2: 946),
  // and the scenes that sit on the vector L1's request roof, where coalescing is worth most: 1 M triangles 407 / 358 /
  // 348 / 339 / 334 / 328, 8 M triangles (32 spp) - / 59.7 / 57.6 / 55.8 / 55.1.  So: 16 on cache-resident scenes, as
  // many as the frame has (<= 64) beyond 65,536 nodes.  (The owner lane's in-order adds grow with the count: that is
  // what turns C2 and C4 around after 16.)  The image does not depend on it (test_frame_independent_of_samples_per_wave).
  const bool pooled = !p->use_photons && p->accel != RT_ACCEL_BRUTE && (pick || c->S.n_lights <= 3u) && !(p->reserved[1] & 1u) &&
                      !(p->reserved[2] & 1u);
  if (pooled) {
    const uint32_t want = c->S.n_nodes > 65536u ? 6u : 4u;
    while (s < want && (2u << s) <= spp_count) ++s;
  }
  // Photon-map shading: the k-NN walks of a pixel's samples run almost in step (their queries lie within one pixel's
  // footprint), and a wave issues every branch any of its lanes is in — C3 at 1 / 2 / 4 / 8 / 16 samples of a pixel per
  // wave: 26.3 / 19.6 / 15.7 / 13.7 / 12.4 ms (16 was 17.0 ms until the waves' counts went to striped slots:
  // rt_kernels.hip flush_stats_striped); at 64 spp, 16 / 32 / 64: 46.6 / 43.9 / 42.8 ms (profiles/r03_c3_samples_per_wave.txt)
  if (p->use_photons && p->accel != RT_ACCEL_BRUTE)
    while (s < 6u && (2u << s) <= spp_count) ++s;
  return s;
}
uint32_t choose_sshift(const rt_ctx* c, const rt_params* p, uint32_t spp_count, bool pick = false) {
  const uint64_t world = p->world ? p->world : 1;
  return choose_sshift_px(c, p, (uint64_t)p->width * p->height / world, spp_count, pick);
}

TileKey tile_key(const rt_params* p, uint32_t sshift) {
  TileKey k;
  k.w = p->width, k.h = p->height, k.rank = p->rank, k.world = p->world ? p->world : 1;
  k.tile = p->tile ? p->tile : 8;
  k.sshift = sshift;
  return k;
}

// fine, sshiftFine: the list's fine tail (TileKey); 0: none
int ensure_tiles(rt_ctx* c, const rt_params* p, uint32_t sshift, hipStream_t stream, uint32_t fine = 0, uint32_t sshiftFine = 0) {
  TileKey k = tile_key(p, sshift);
  if (fine && sshiftFine > sshift) k.fine = fine, k.sshiftFine = sshiftFine;
  if (c->tiles.d && k == c->tileKey) return use_on(c->tiles, stream);
  uint32_t from = 0;
  const int rc = stream_upload(&c->tiles, wave_tiles(k, &from), stream);
  if (rc != RT_OK) return rc;
  c->tileKey = k, c->tilesFineFrom = from;
  return RT_OK;
}

// How many coarse tiles of a plain frame's list are split for the end of the launch: one per wave the device holds at
// once (rtk::persist_fine_waves: 0 where the frame does not run in k_render_persist; measured on C2 at 0 / 1 / 2 / 4 per
// wave: 42.83 / 42.63 / 42.67 / 42.72 ms, profiles/fine_tail/).  RT_FINE_TAIL, read per launch: 0 none, n that many,
// "all" the whole list.
uint32_t fine_tail_tiles(uint32_t waves) {
  if (!waves) return 0;
  const char* const e = getenv("RT_FINE_TAIL");
  if (!e || !*e) return waves;
  if (!strcmp(e, "all")) return ~0u;
  const long n = atol(e);
  return n <= 0 ? 0u : (uint32_t)std::min<long>(n, 0x7fffffff);
}

int ensure_granules(rt_ctx* c, const rt_params* p, uint32_t rank, hipStream_t stream, const rt_ctx::GranList** out) {
  char key[96];
  snprintf(key, sizeof key, "%u.%u.%u.%u.%u", p->width, p->height, rank, p->world ? p->world : 1, p->tile ? p->tile : 8);
  auto it = c->granules.find(key);
  if (it == c->granules.end()) {
    std::vector<uint32_t> g;
    owned_granules(p->width, p->height, rank, p->world, p->tile, [&](uint32_t x8, uint32_t y8) { g.push_back(x8 | (y8 << 16)); });
    rt_ctx::GranList L;
    int rc = stream_upload(&L, g, stream);
    if (rc != RT_OK) return rc;
    it = c->granules.emplace(key, std::move(L)).first;
  } else {
    const int rc = use_on(it->second, stream);
    if (rc != RT_OK) return rc;
  }
  *out = &it->second;
  return RT_OK;
}

// The checks of check_params that look at p alone (the multi-view passes answer them before they look at the context).
int check_params_shape(const rt_params* p) {
  if (p->width == 0 || p->height == 0 || p->width > 65535u || p->height > 65535u)
    return fail(RT_ERR_INVALID, "image size %ux%u out of range", p->width, p->height);
  if (p->spp == 0) return fail(RT_ERR_INVALID, "spp must be >= 1");
  if (p->mode != RT_MODE_RAY && p->mode != RT_MODE_PATH) return fail(RT_ERR_INVALID, "mode must be 0 or 1");
  if (p->rng_mode != RT_RNG_PIXEL)
    return fail(RT_ERR_UNSUPPORTED,
                "rng_mode legacy is one global serial engine (reference LightSource.h:6) and cannot run in "
                "parallel; the GPU path implements RT_RNG_PIXEL only");
  if (p->max_depth < 1 || p->max_depth > 3) return fail(RT_ERR_UNSUPPORTED, "max_depth must be in 1..3");
  if (p->world > 1 && p->rank >= p->world) return fail(RT_ERR_INVALID, "rank %u >= world %u", p->rank, p->world);
  if (p->tile % 8 != 0) return fail(RT_ERR_INVALID, "tile must be a multiple of 8");
  if (p->spp_count && (uint64_t)p->spp_begin + p->spp_count > p->spp)
    return fail(RT_ERR_INVALID, "sample range [%u,+%u) exceeds spp %u", p->spp_begin, p->spp_count, p->spp);
  return RT_OK;
}

int check_params(const rt_ctx* c, const rt_params* p) {
  if (!p) return fail(RT_ERR_INVALID, "params is null");
  if (c->broken) return fail(RT_ERR_STATE, "the context's device tree is in an unknown state (a failed rt_bvh_tune or rt_update): destroy it");
  const int rc = check_params_shape(p);
  if (rc != RT_OK) return rc;
  if (p->use_photons) {
    if (c->S.n_photons == 0) return fail(RT_ERR_STATE, "use_photons set but no photons were uploaded (rt_set_photons)");
    if (p->k < 1 || p->k > RT_KNN_KMAX) return fail(RT_ERR_UNSUPPORTED, "k must be in 1..%d", RT_KNN_KMAX);
    // kdtree.h:182-183 throws std::logic_error here
    if (p->k > c->S.n_photons) return fail(RT_ERR_STATE, "k is greater than the number of nodes");
    if (p->photons_requested == 0) return fail(RT_ERR_INVALID, "photons_requested must be > 0 with use_photons");
  }
  return RT_OK;
}

// The samples of a pixel a call integrates: [s0, s1), all spp of them unless p gives a range
struct SampleRange {
  uint32_t s0, s1, count;
};
SampleRange sample_range(const rt_params& p) {
  if (p.spp_count) return {p.spp_begin, p.spp_begin + p.spp_count, p.spp_count};
  return {0u, p.spp, p.spp};
}

// *st zeroed but for the device counters
int read_counters(rt_ctx* c, rt_stats* st) {
  memset(st, 0, sizeof *st);
  unsigned long long h[RTK_CNT_COUNT];
  HIP_TRY(hipMemcpy(h, c->dCounters.get(), sizeof h, hipMemcpyDeviceToHost));
  st->rays_closest = h[RTK_CNT_CLOSEST];
  st->rays_shadow = h[RTK_CNT_SHADOW];
  st->knn_queries = h[RTK_CNT_KNN];
  st->nodes_visited = h[RTK_CNT_NODES];
  st->tris_tested = h[RTK_CNT_TRIS];
  st->kd_visited = h[RTK_CNT_KD];
  st->frame_fetches = h[RTK_CNT_FRAMES];
  st->reserved[0] = h[RTK_CNT_WNODE];  // diagnostics (collect_stats): wave-level node steps,
  st->reserved[1] = h[RTK_CNT_WLEAF];  // wave-level leaf phases -> lane utilisation of the traversal
  st->reserved[2] = h[RTK_CNT_LWAIT];  // lanes holding a leaf / lanes without a ray at the START of the round,
  st->reserved[3] = h[RTK_CNT_LIDLE];  // summed over that round's node steps
#ifdef RT_PHASE_TIMING  // diagnostic build (tools/phase_timing.sh): section clocks of the pooled kernel
  if (getenv("RT_PHASE_DUMP")) {
    fprintf(stderr, "{\"phase_clocks\": [");
    for (int i = 16; i < RTK_CNT_COUNT; ++i) fprintf(stderr, "%llu%s", h[i], i + 1 < RTK_CNT_COUNT ? ", " : "]}\n");
  }
#endif
  return RT_OK;
}

// The ring of event pairs that time the integrators' launches (rt_profile_collect reads pairs 0 .. evUsed - 1): the next
// pair is recorded on `stream` around what `launch` queues there; *evIndex gets its index.
template <class Launch>
int timed_launch(rt_ctx* c, hipStream_t stream, int* evIndex, Launch launch) {
  const int e = c->evUsed % kEventPairs;
  HIP_TRY(hipEventRecord(c->ev[e][0].get(), stream));
  const int rc = launch();
  if (rc != RT_OK) return rc;
  HIP_TRY(hipEventRecord(c->ev[e][1].get(), stream));
  c->evUsed++;
  if (evIndex) *evIndex = e;
  return RT_OK;
}
hipError_t event_pair_ms(const rt_ctx* c, int e, float* ms) {
  return hipEventElapsedTime(ms, c->ev[e][0].get(), c->ev[e][1].get());
}
// *stats of the launch that event pair e brackets, once `stream` has run it: the counters, the kernel time and the
// caller's count of samples
int frame_stats(rt_ctx* c, hipStream_t stream, int e, uint64_t samples, rt_stats* stats) {
  HIP_TRY(hipStreamSynchronize(stream));
  const int rc = read_counters(c, stats);
  if (rc != RT_OK) return rc;
  float ms = 0.f;
  HIP_TRY(event_pair_ms(c, e, &ms));
  stats->kernel_ms = ms, stats->samples = samples;
  return RT_OK;
}

// The photon k-NN walk's LDS stack (rt_kernels.hip knn_query) over a map of n photons: its entry width and the
// rows it needs.  The walk's stack holds a sentinel + at most one pending far child per tree level + the entry written
// ahead of the top; 16-bit entries (two per row) when every photon index fits below the 16-bit sentinel 0xffff.
// Photon frames and rt_knn both size the walk by this rule.
struct KdStack {
  bool kd16;
  uint32_t rows;
};
KdStack kd_stack(uint32_t n_photons) {
  uint32_t kd = 1;  // levels of the median tree over n_photons
  while ((1ull << kd) <= n_photons) ++kd;
  const bool kd16 = n_photons < 65535u;
  return {kd16, kd16 ? (kd + 2u + 1u) / 2u : kd + 1u};
}
// A lane's stack rows for a walk that needs `levels` of them (+1: row 0 of a lane's stack is the TERM sentinel,
// rt_kernels.hip Trav)
uint32_t stack_levels(uint32_t levels) {
  return (levels > (uint32_t)rtbvh::kMaxDepth ? (uint32_t)rtbvh::kMaxDepth : levels) + 1u;
}

// The wavefront integrator's arguments for p: rank p->rank's granules and its path state + ray queues, carved from
// one block that grows with the batch.  *out keeps nGran 0 when the rank owns no pixel: there is nothing to launch.
int wavefront_args(rt_ctx* c, const rt_params* p, const rtk::RenderArgs& A, uint32_t sppCount, hipStream_t stream,
                   rtk::WfArgs* out) {
  const rt_ctx::GranList* G = nullptr;
  int rc = ensure_granules(c, p, p->rank, stream, &G);
  if (rc != RT_OK) return rc;
  const size_t perSample = (size_t)G->n * 64u;
  if (perSample == 0) return RT_OK;
  size_t batch = (4u << 20) / perSample;  // ~4 M paths per batch (1.1 GB of state + queues)
  batch = batch < 1 ? 1 : batch > sppCount ? sppCount : batch;
  const size_t P = batch * perSample;
  // rng 4, org 16, dir 16, key 8, nrm 16, pnt 16, col 48, rayO 64, rayD 64, res 32 = 284 B per path
  bool grew = false;
  if ((rc = grow(&c->wfBlock, &c->wfCap, P * 284 + 4096 + 2048 * sizeof(unsigned long long), &grew)) != RT_OK) return rc;
  if (grew) {  // carved again for P paths
    char* q = c->wfBlock.get();
    auto take = [&](size_t n) {
      char* r = q;
      q += (n + 255) / 256 * 256;
      return r;
    };
    rtk::WfArgs& W = c->wf;
    W.rayO = reinterpret_cast<float4*>(take(P * 64)), W.rayD = reinterpret_cast<float4*>(take(P * 64));
    W.col = reinterpret_cast<float4*>(take(P * 48));
    W.org = reinterpret_cast<float4*>(take(P * 16)), W.dir = reinterpret_cast<float4*>(take(P * 16));
    W.nrm = reinterpret_cast<float4*>(take(P * 16)), W.pnt = reinterpret_cast<float4*>(take(P * 16));
    W.res = reinterpret_cast<uint2*>(take(P * 32)), W.key = reinterpret_cast<uint2*>(take(P * 8));
    W.rng = reinterpret_cast<uint32_t*>(take(P * 4));
    W.stripes = reinterpret_cast<unsigned long long*>(take(2048 * sizeof(unsigned long long)));
    const hipError_t he = hipMemsetAsync(W.stripes, 0, 2048 * sizeof(unsigned long long), stream);
    if (he != hipSuccess) {
      c->wfCap = 0;  // (the block is not usable before its stripes are zero)
      return fail(RT_ERR_HIP, "wavefront stripes reset failed: %s", hipGetErrorString(he));
    }
  }
  rtk::WfArgs W = c->wf;
  W.gran = G->d.get(), W.nGran = G->n, W.width = p->width, W.height = p->height, W.spp = p->spp, W.seed = p->seed;
  W.s0 = A.s0, W.s1 = A.s1, W.batch = (uint32_t)batch, W.nPaths = 0;
  *out = W;
  return RT_OK;
}

// A wave-tile list of the caller's (an adaptive pass, a multi-view frame) instead of the frame's cached one: device
// memory, for `sshift`; a multi-view frame also gives each tile's view and the view records (rtk::RenderArgs), and a
// multi-view shutter frame the views' shutter records beside them.
struct TileList {
  const uint32_t* tiles;
  uint32_t n, sshift;
  const uint32_t* tileView = nullptr;
  const rtk::ViewRec* views = nullptr;
  const rtk::ViewShutterRec* viewShutters = nullptr;
};

// What forms or splits a frame's samples in place of the plain frame, if anything: the thin lens of rt_render_lens, the
// open shutter of rt_render_shutter, the light groups of rt_render_lights (dAccum then holds one slice per group) or the
// light picks of rt_render_pick — and what its vertices shade with in place of their meshes' materials: the vertex colours
// of rt_render_colors, the textures of rt_render_textured, the material maps of rt_render_material or the normal maps of
// rt_render_normal_mapped — with the record
// its kernels take; their callers have refused photons and the wavefront bit (frame_params_checks).  A multi-view
// shutter frame carries its records in its TileList instead: launch_frame tells it from them.
using FrameGen = rtk::FrameVariant;

// What every such frame refuses of a p of the right shape; noun names the frames in the messages.
int frame_params_checks(const rt_params* p, const char* noun) {
  if (p->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded %s frames (world %u) are not supported", noun, p->world);
  if (p->use_photons) return fail(RT_ERR_UNSUPPORTED, "%s frames do not shade from the photon map", noun);
  if (p->reserved[2] & 1u) return fail(RT_ERR_UNSUPPORTED, "%s frames do not run the wavefront integrator", noun);
  return RT_OK;
}

// Launch the integrate kernel for p on `stream`, bracketed by an event pair.  own: render those wave tiles only.
// gen: the frame's variant, if any.
int launch_frame(rt_ctx* c, const rt_params* p, float4* dAccum, hipStream_t stream, int* evIndex,
                 const TileList* own = nullptr, const FrameGen& gen = FrameGen()) {
  const SampleRange sr = sample_range(*p);
  const uint32_t sshift = own ? own->sshift : choose_sshift(c, p, sr.count, gen.gen == FrameGen::PICK);
  int rc = RT_OK;
  rtk::RenderArgs A;
  A.sshift = sshift;
  wave_tile_shape(sshift, A.tileW, A.tileH);
  A.tileView = own ? own->tileView : nullptr, A.views = own ? own->views : nullptr;
  A.viewShutters = own ? own->viewShutters : nullptr;
  A.width = p->width, A.height = p->height, A.spp = p->spp;
  A.s0 = sr.s0, A.s1 = sr.s1;
  A.mode = p->mode, A.max_depth = p->max_depth, A.seed = p->seed;
  A.k = p->k, A.photons_requested = p->photons_requested;
  static const bool noPool = getenv("RT_NO_POOL") != nullptr;
  A.flags = (noPool || (p->reserved[1] & 1u)) ? 0u : 1u;
  if (c->bvh.leafMax <= 2u) A.flags |= 2u;  // (the resident tree's, whoever built it last: rt_create, rt_rebuild)
  // stack entries: one per inner level on a root-to-leaf path; the photon k-NN
  // keeps one split distance per kd level in the same region
  // a root-to-leaf path of depth d passes d inner nodes and each stacks at most one
  // far child, so d entries suffice
  uint32_t levels = c->bvh.maxDepth > 1 ? c->bvh.maxDepth : 1;
  A.kd16 = 0;
  if (p->use_photons) {
    const KdStack ks = kd_stack(c->S.n_photons);
    A.kd16 = ks.kd16 ? 1u : 0u;
    levels = levels > ks.rows ? levels : ks.rows;
  }
  A.stackLevels = stack_levels(levels);
  A.tileCounter = c->dTileCounter.get(), A.numCUs = c->numCUs, A.waveWords = 0, A.tilesPerBlock = 1;
  // rt_params.reserved[2] bit 0: the queue-based (wavefront) integrator — BVH direct lighting with
  // at most 3 lights, like the pooled kernel; same frame bit for bit
  const bool wavefront = (p->reserved[2] & 1u) && !p->use_photons && p->accel != RT_ACCEL_BRUTE && c->S.n_lights <= 3u;
  // The wave tiles: the caller's, or the context's list — with a fine tail where the plain frame runs in k_render_persist:
  // the same pixels at up to four times the samples per wave (<= 64, and no more than the launch has: choose_sshift_px's rule)
  uint32_t fine = 0, sshiftFine = std::min(6u, sshift + 2u);
  while (sshiftFine > sshift && (1u << sshiftFine) > sr.count) --sshiftFine;
  if (!own && !gen && !wavefront)
    fine = fine_tail_tiles(rtk::persist_fine_waves(p->accel == RT_ACCEL_BRUTE, p->use_photons != 0, c->S, A));
  if (!own && (rc = ensure_tiles(c, p, sshift, stream, fine, sshiftFine)) != RT_OK) return rc;
  A.tiles = own ? own->tiles : c->tiles.d.get(), A.n_tiles = own ? own->n : c->tiles.n;
  A.fineFrom = own ? A.n_tiles : c->tilesFineFrom, A.sshiftFine = own ? sshift : c->tileKey.sshiftFine;
  rtk::WfArgs W{};
  if (wavefront && (rc = wavefront_args(c, p, A, sr.count, stream, &W)) != RT_OK) return rc;
  return timed_launch(c, stream, evIndex, [&] {
    // (a multi-view shutter frame keeps the surface record of a coloured or textured gen: rt_render_views_shutter_albedo)
    if (const FrameGen V = A.viewShutters ? FrameGen::under_views_shutter(gen) : gen) {
      hipError_t he = rtk::launch_render_variant(V, p->accel == RT_ACCEL_BRUTE, p->collect_stats != 0, c->S, A, dAccum,
                                                 c->dCounters.get(), stream);
      if (he != hipSuccess) return fail(RT_ERR_HIP, "%s render launch failed: %s", V.name().c_str(), hipGetErrorString(he));
    } else if (!wavefront) {
      hipError_t he = rtk::launch_render(p->accel == RT_ACCEL_BRUTE, p->use_photons != 0, p->collect_stats != 0, c->S, A,
                                         dAccum, c->dCounters.get(), stream);
      if (he != hipSuccess) return fail(RT_ERR_HIP, "render launch failed: %s", hipGetErrorString(he));
    } else if (W.nGran) {
      hipError_t hw = rtk::launch_wavefront(c->S, W, p->mode, p->max_depth, dAccum, c->dCounters.get(), c->dTileCounter.get(),
                                            A.stackLevels, c->numCUs, stream);
      if (hw != hipSuccess) return fail(RT_ERR_HIP, "wavefront launch failed: %s", hipGetErrorString(hw));
    }
    return (int)RT_OK;
  });
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_err.c_str(); }

}  // extern "C"

namespace {
// rt_create with an optional host-built tree to copy instead of building one (rt_group: every
// device gets the same tree, built once)
int create_ctx(const rt_scene_desc* sc, const rt_options* opt, const rtbvh::Built* prebuilt, rt_ctx** out);
}  // namespace

extern "C" {

int rt_create(const rt_scene_desc* sc, const rt_options* opt, rt_ctx** out) { return create_ctx(sc, opt, nullptr, out); }

}  // extern "C"

namespace {
// f(thread, begin, end) over contiguous chunks of [b, e): up to 16 threads, one per 2^18 elements
template <class F>
void par_chunks(size_t b, size_t e, F f) {
  static const uint32_t hw = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  const size_t n = e > b ? e - b : 0;
  const uint32_t T = (uint32_t)std::max<size_t>(1, std::min<size_t>(hw, n >> 18));
  if (T <= 1u) {
    f(0u, b, e);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(T - 1u);
  for (uint32_t t = 1; t < T; ++t) th.emplace_back([&f, b, n, t, T] { f(t, b + n * t / T, b + n * (t + 1) / T); });
  f(0u, b, b + n / T);
  for (std::thread& x : th) x.join();
}

// A built tree before it belongs to a context (build_tree makes it, install_tree hands it over): the host copy kept for
// rt_bvh_export, the device arrays (DevScene's fields of the same names) and what rt_bvh_info reports of it
struct Tree {
  rtbvh::Built bvh;
  DevBuf<uint4> nodes, q8;
  DevBuf<float4> tris, trisRef, nodesF;
  uint32_t nNodes = 0, builder = RT_BVH_HOST, nodeFormat = RT_NODES_F16, q8ShiftBytes = 0;
  float buildMs = 0.f, planMs = 0.f;  // planMs: the host passes' share of buildMs
};

// The tree the device builder left on the device, read back into t->bvh: its float nodes, and with nTris > 0 its
// triangle records in both orders (throws: the callers report it as their step's failure)
void read_back_tree(Tree* t, uint32_t nTris) {
  const size_t nn = t->nNodes;
  t->bvh.nodes.resize(nn), t->bvh.tris.resize(nTris), t->bvh.trisRef.resize(nTris);
  if (hipMemcpy(t->bvh.nodes.data(), t->nodesF.get(), nn * sizeof(rtbvh::Node), hipMemcpyDeviceToHost) != hipSuccess ||
      (nTris && (hipMemcpy(t->bvh.tris.data(), t->tris.get(), (size_t)nTris * sizeof(rtbvh::TriRec), hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(t->bvh.trisRef.data(), t->trisRef.get(), (size_t)nTris * sizeof(rtbvh::TriRec), hipMemcpyDeviceToHost) != hipSuccess)))
    throw std::runtime_error("reading the device-built tree back failed");
}

// The short reciprocal (rt_device.h recip_fast: v_rcp_f32 + one Newton step, the division's bits for 2^-100 <= |x| < 2^101
// — exhaustive check, tools/microbench/recip_exact.hip) replaces the division in the default render instances
// (rt_kernels.hip LT_FASTDET) in two places, and the host vouches for the range here:
//  * 1 / det of the triangle test: |det| = |e1 . (d x e2)| <= |e1| |e2| |d|; edges are at most 2 sqrt(3) maxAbs long, and
//    the rays the RENDER kernels make are unit vectors (camera, bounce) or run from a surface point to a light sample;
//  * length and 1 / length in normalisations (sqrt_fast: the same check, 2^-100 <= x < 2^101): every vector the kernels
//    normalise is a small sum of scene inputs, so |input| <= 1e14 keeps the squared length below 2^100 (the lower end
//    is tested per lane: rt_device.h unit3).
// Outside these bounds — or with any non-finite input — the kernels divide.  (User rays, rt_trace /
// rt_trace_stream_device, always divide.)  Sets c->S.slowRecip and c->recipCheck.  rt_create and rt_update run it.
// max |x| over n floats as bits (a non-finite value has all exponent bits set: its magnitude bits compare above every
// finite float's)
uint32_t max_abs_bits(const float* p, size_t n) {
  uint32_t top[64] = {0};
  par_chunks(0, n, [&](uint32_t th, size_t b, size_t e) {
    uint32_t m = 0;
    for (size_t i = b; i < e; ++i) {
      uint32_t u;
      memcpy(&u, p + i, 4);
      u &= 0x7fffffffu;
      m = u > m ? u : m;
    }
    top[th] = m;
  });
  uint32_t m = 0;
  for (uint32_t t : top) m = t > m ? t : m;
  return m;
}
float bits_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// The operand bounds of the short forms for the context's positions, normals and lights with camera `cam` (reads the
// magnitude summaries c->magPos / c->magNrm and the lights c->hostLights)
bool short_forms_bound(const rt_ctx* c, const rt_camera& cam) {
  double maxAbs = 0, maxLight = 0, maxAny = 0;
  bool finite = true;
  auto eat = [&](uint32_t m) {
    if (m >= 0x7f800000u) finite = false;
    else maxAny = std::max(maxAny, (double)bits_float(m));
    return m >= 0x7f800000u ? 0.0 : (double)bits_float(m);
  };
  maxAbs = eat(c->magPos);
  eat(c->magNrm);
  eat(max_abs_bits(cam.position, 12));
  for (const rt_light& L : c->hostLights) {
    eat(max_abs_bits(L.position, 15));
    eat(max_abs_bits(&L.intensity, 6));
    double pos = 0, ver = 0, hor = 0;
    for (int a = 0; a < 3; ++a) pos += (double)L.position[a] * L.position[a], ver += (double)L.vertical[a] * L.vertical[a], hor += (double)L.horizontal[a] * L.horizontal[a];
    maxLight = std::max(maxLight, std::sqrt(pos) + std::fabs((double)L.side) * (std::sqrt(ver) + std::sqrt(hor)));
  }
  const double edge = 2.0 * 1.7320508 * maxAbs, dir = 1.7320508 * maxAbs + maxLight + 2.0;
  const double detBound = 1.01 * edge * edge * dir;
  return finite && maxAny <= 1e14 && maxLight <= 1e14 && std::isfinite(detBound) && detBound < 1.2676506e30;
}

// (reads the magnitude summaries c->magPos / c->magNrm, the camera S.cam and the lights c->hostLights)
void vouch_short_forms(rt_ctx* c) {
  rtk::DevScene& S = c->S;
  S.slowRecip = short_forms_bound(c, S.cam) ? 0u : 1u;
  if (getenv("RT_SLOW_RECIP")) S.slowRecip = 1u;  // (A/B and the parity tests of the division path)
  // ... and the device vouches for the short forms itself, once per process and device (2^25 inputs, well under a
  // millisecond): the exhaustive check ran on one MI355X; a part whose v_rcp_f32 / v_rsq_f32 rounded differently would
  // show here, and its contexts divide.
  if (S.slowRecip) return;
  static std::mutex mu;
  static std::map<int, bool> verified;
  std::lock_guard<std::mutex> lock(mu);
  auto it = verified.find(c->device);
  if (it == verified.end()) {
    bool ok = false;
    {
      DevBuf<uint32_t> dBad;
      uint32_t bad = 1u;
      if (dev_alloc(&dBad, 1) == hipSuccess && hipMemset(dBad.get(), 0, sizeof(uint32_t)) == hipSuccess &&
          rtk::launch_selfcheck_recip(dBad.get(), nullptr) == hipSuccess &&
          hipMemcpy(&bad, dBad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess)
        ok = bad == 0u;
    }
    it = verified.emplace(c->device, ok).first;
    if (getenv("RT_BVH_VERBOSE")) fprintf(stderr, "short reciprocal / square root self-check on device %d: %s\n", c->device, ok ? "bit-identical" : "MISMATCH, dividing");
  }
  if (!it->second) S.slowRecip = 1u;
  c->recipCheck = it->second ? 1u : 2u;
}

// The tree part of rt_create, which rt_rebuild runs again: the builder choice, the host passes over the description
// (validation, the host build, the hybrid top or the size keys), then — `resident` gives the positions and the shading
// records on the device: rt_create uploads them there, a rebuild has them — the device build, the renumbering and the
// node format.  Everything lands in *t; no context is touched.
template <class Resident>
int build_tree(const rt_scene_desc* sc, uint32_t leafMax, uint32_t builderOpt, uint32_t nodeFormatOpt, const rtbvh::Built* prebuilt,
               Resident resident, Tree* t) {
  int rc = RT_OK;
  // the tree: host SAH builder, or the device builder (tiny scenes always take the host's
  // special cases)
  // (RT_BVH_GPU=1 / 2 / 3: the device / hybrid / host builder whatever the options say — the test suites run whole on each)
  const char* gpuEnv = getenv("RT_BVH_GPU");
  uint32_t wantBuilder = gpuEnv ? (uint32_t)atoi(gpuEnv) : builderOpt;
  if (wantBuilder > RT_BVH_HOST) return fail(RT_ERR_INVALID, "unknown bvh_builder %u", wantBuilder);
  // AUTO: the device builder gives the host builder's tree (tests/treedigest.py; profiles/r04_builders.txt) 2 ... 14 x sooner,
  // so every scene it is faster on takes it (from 8,192 triangles: below that a build is 1-3 ms either way and the host needs no
  // device round trip); a group of contexts given a host-built tree shares it
  static const uint32_t autoFrom = getenv("RT_BVH_AUTO_FROM") ? (uint32_t)atoi(getenv("RT_BVH_AUTO_FROM")) : 8192u;
  if (wantBuilder == RT_BVH_AUTO) wantBuilder = (sc->n_triangles >= autoFrom && !prebuilt) ? (uint32_t)RT_BVH_DEVICE : (uint32_t)RT_BVH_HOST;
  // (a scene of a single part has no top to build on the host: the device builder's own path handles it)
  const bool hybrid = wantBuilder == RT_BVH_HYBRID && sc->n_triangles > 1024u;
  const bool gpuBuild = (wantBuilder == RT_BVH_DEVICE || wantBuilder == RT_BVH_HYBRID) && sc->n_triangles >= 16;
  rtbvh::TopBuilt topBuilt;
  rtbvh::ScenePlan plan;
  std::vector<float> sizeKey;
  const auto tBuild0 = std::chrono::steady_clock::now();
  auto msSince = [&tBuild0] { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tBuild0).count(); };
  try {
    if (hybrid) {
      rtbvh::buildTop(*sc, leafMax, 1024u, topBuilt);
      if (getenv("RT_BVH_VERBOSE"))
        fprintf(stderr, "hybrid builder: host top of %zu nodes over %zu parts in %.1f ms\n", topBuilt.nodes.size(), topBuilt.parts.size(), msSince());
      t->bvh.leafMax = topBuilt.leafMax, t->bvh.pad = topBuilt.pad, t->bvh.originBound = topBuilt.originBound, t->bvh.boxScale = topBuilt.boxScale;
      t->bvh.maxAbs = topBuilt.maxAbs;
      t->bvh.depthCap = topBuilt.depthCap;
      (void)rtbvh::planSceneExact(*sc, leafMax, sizeKey);  // (the size keys of the subtrees' sweeps)
    } else if (gpuBuild) {
      // (the device build restates the host builder's splits: it takes the host's depth cap and size keys)
      plan = rtbvh::planSceneExact(*sc, leafMax, sizeKey);
      if (getenv("RT_BVH_VERBOSE")) fprintf(stderr, "device builder: validation + size keys in %.2f ms\n", msSince());
      t->bvh.leafMax = plan.leafMax, t->bvh.pad = plan.pad, t->bvh.originBound = plan.originBound, t->bvh.boxScale = plan.boxScale;
      t->bvh.maxAbs = plan.maxAbs;
      t->bvh.depthCap = plan.depthCap;
    } else if (prebuilt) {
      t->bvh = *prebuilt;
    } else {
      rtbvh::build(*sc, leafMax, t->bvh);
    }
  } catch (const std::exception& e) {
    return fail(RT_ERR_INVALID, "scene rejected: %s", e.what());
  }
  t->planMs = msSince();
  static_assert(sizeof(rtbvh::Node16) == 2 * sizeof(uint4), "node layout");
  static_assert(sizeof(rtbvh::TriRec) == 3 * sizeof(float4), "triangle layout");
  const float* dVpos = nullptr;
  const uint4* dTriShade = nullptr;
  if ((rc = resident(&dVpos, &dTriShade)) != RT_OK) return rc;
  if (gpuBuild) {
    if (getenv("RT_BVH_VERBOSE")) fprintf(stderr, "scene arrays on the device %.2f ms after the start\n", msSince());
    rtk::GpuBvh G;
    hipError_t he = hipSuccess;
    if (hybrid) {
      he = rtk::gpu_bvh_build_over_top(dVpos, dTriShade, sizeKey.data(), sc->n_triangles, topBuilt, &G, nullptr);
    } else {
      he = rtk::gpu_bvh_build_exact(dVpos, dTriShade, sizeKey.data(), sc->n_triangles, plan, &G, nullptr);
    }
    if (he != hipSuccess) return fail(RT_ERR_HIP, "device BVH build failed: %s", hipGetErrorString(he));
    t->nodes.reset(G.nodes16), t->tris.reset(G.tris), t->trisRef.reset(G.trisRef), t->nodesF.reset(G.nodesF);
    t->bvh.maxDepth = G.maxDepth;
    t->nNodes = G.n_nodes;
    t->builder = hybrid ? RT_BVH_HYBRID : RT_BVH_DEVICE;
    // Trees whose top the render kernel may keep in LDS (rt_kernels.hip plan_persist: a prefix of the node array) get the host
    // builder's final numbering — the most-visited nodes first, greedily by box area from the root (bvh_build.cpp
    // relayoutTop) — instead of the device's pre-order: C4 loses 2 % on a pre-order tree.  64 KB ... 4 MB back and forth.
    if (t->nNodes >= 2u && t->nNodes <= 65536u) {
      try {
        read_back_tree(t, 0);
        rtbvh::relayoutAndPack(t->bvh);
        if (hipMemcpy(t->nodesF.get(), t->bvh.nodes.data(), (size_t)t->nNodes * sizeof(rtbvh::Node), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(t->nodes.get(), t->bvh.nodes16.data(), (size_t)t->nNodes * sizeof(rtbvh::Node16), hipMemcpyHostToDevice) != hipSuccess)
          throw std::runtime_error("writing the renumbered tree failed");
        t->bvh.nodes.clear(), t->bvh.nodes16.clear();  // (rt_bvh_export reads the device copies)
      } catch (const std::exception& e) {
        return fail(RT_ERR_HIP, "device BVH build: %s", e.what());
      }
    }
  } else {
    if ((rc = upload(&t->nodes, t->bvh.nodes16.data(), t->bvh.nodes16.size() * 2)) != RT_OK ||
        (rc = upload(&t->tris, t->bvh.tris.data(), t->bvh.tris.size() * 3)) != RT_OK ||
        (rc = upload(&t->trisRef, t->bvh.trisRef.data(), t->bvh.trisRef.size() * 3)) != RT_OK)
      return rc;
    t->nNodes = static_cast<uint32_t>(t->bvh.nodes.size());
  }
  // The node records the pooled render kernel and rt_trace traverse (rt_options.node_format; RT_NODES=f16|q8 overrides).
  // RT_NODES_Q8 — 16-byte records, ONE vector-memory request per visit (bvh_build.h Slot16) — is for trees the caches do
  // not hold, where the traversal sits on the vector L1's request rate.  The other kernels (photon emission, ray streams,
  // the wavefront integrator, the one-wave-per-workgroup render instances) keep the 32-byte records, so both forms are resident.
  uint32_t wantNodes = nodeFormatOpt;
  if (const char* e = getenv("RT_NODES")) wantNodes = !strcmp(e, "q8") ? (uint32_t)RT_NODES_Q8 : !strcmp(e, "f16") ? (uint32_t)RT_NODES_F16 : wantNodes;
  if (wantNodes > RT_NODES_Q8) return fail(RT_ERR_INVALID, "unknown node_format %u", wantNodes);
  if (wantNodes == RT_NODES_Q8) {
    try {
      if (gpuBuild) read_back_tree(t, sc->n_triangles);  // the packer works from the float records
      if (t->bvh.q8.empty()) rtbvh::packQ8(t->bvh);
      if (gpuBuild) t->bvh.nodes.clear(), t->bvh.tris.clear(), t->bvh.trisRef.clear();  // (rt_bvh_export reads the device copies)
    } catch (const std::exception& e) {
      return fail(RT_ERR_UNSUPPORTED, "node_format RT_NODES_Q8: %s", e.what());
    }
    static_assert(sizeof(rtbvh::Slot16) == sizeof(uint4), "slot layout");
    if ((rc = upload(&t->q8, t->bvh.q8.data(), t->bvh.q8.size())) != RT_OK) return rc;
    t->q8ShiftBytes = t->bvh.q8Shift + 4u;
    t->nodeFormat = RT_NODES_Q8;
    std::vector<rtbvh::Slot16>().swap(t->bvh.q8);  // (the host copy is not needed again)
  }
  t->buildMs = msSince();
  if (getenv("RT_BVH_VERBOSE")) fprintf(stderr, "tree resident %.2f ms after the start\n", t->buildMs);
  return RT_OK;
}

// *t becomes the context's tree, with every value derived from it; the tree it replaces (a rebuild) is freed, and what
// was derived from that one's topology — the refit depth table, the quality baseline — goes with it.  Nothing here can fail.
void install_tree(rt_ctx* c, Tree* t) {
  rtk::DevScene& S = c->S;
  c->bvh = std::move(t->bvh);
  c->nodes = std::move(t->nodes), c->q8 = std::move(t->q8), c->tris = std::move(t->tris), c->trisRef = std::move(t->trisRef);
  c->nodesF = std::move(t->nodesF);
  c->builder = t->builder, c->nodeFormat = t->nodeFormat, c->buildMs = t->buildMs;
  S.nodes = c->nodes.get(), S.q8 = c->q8.get(), S.tris = c->tris.get(), S.trisRef = c->trisRef.get();
  S.n_nodes = t->nNodes, S.q8ShiftBytes = t->q8ShiftBytes;
  S.invBoxScale = 1.f / c->bvh.boxScale;
  S.originBound = c->bvh.originBound;
  memcpy(&c->magRef, &c->bvh.maxAbs, 4);
  // Pool thresholds (Trav::round's descent early exit, the steal and refill levels).  Two scene
  // classes, as for the samples-of-a-pixel-per-wave rule: trees the caches hold (<= 65,536 nodes)
  // are issue-bound and want long descents (12 / 8 / 24: C2 50.5 ms; 16 or 24 lanes cost 0.2-1 %);
  // beyond that every step waits on the vector L1, and leaving the descent with up to 24 lanes still
  // in it plus refilling at 32 hands out work sooner (C5 328.5 -> 317.4 ms, C5x8 55.0 -> 52.4 ms;
  // profiles/r03_pool_thresholds.txt).
  const bool bigTree = S.n_nodes > 65536;
  S.leafT = getenv("RT_LEAFT") ? atoi(getenv("RT_LEAFT")) : bigTree ? 32 : 12;
  S.leafMul = getenv("RT_LEAFMUL") ? atoi(getenv("RT_LEAFMUL")) : bigTree ? 32 : 22;
  S.stealT = getenv("RT_STEALT") ? atoi(getenv("RT_STEALT")) : 8;
  S.refillT = getenv("RT_REFILLT") ? atoi(getenv("RT_REFILLT")) : bigTree ? 32 : 24;
  c->refitDepth.reset(), c->refitMaxDepth = 0;
  c->costBuiltValid = false, c->refits = 0;
}

int create_ctx(const rt_scene_desc* sc, const rt_options* opt, const rtbvh::Built* prebuilt, rt_ctx** out) {
  if (!sc || !out) return fail(RT_ERR_INVALID, "scene/out is null");
  *out = nullptr;
  if (!sc->vertex_pos || !sc->vertex_nrm || !sc->tri_vtx || !sc->mesh_tri_begin || !sc->mesh_vtx_begin ||
      !sc->materials || (sc->n_lights && !sc->lights))
    return fail(RT_ERR_INVALID, "scene descriptor has null arrays");
  if (sc->n_meshes == 0 || sc->n_vertices == 0 || sc->n_triangles == 0)
    return fail(RT_ERR_INVALID, "empty scene");
  // (node and leaf refs are 31-bit byte offsets of 32-B node / 48-B triangle records)
  if (sc->n_triangles >= (1u << 25)) return fail(RT_ERR_UNSUPPORTED, "more than 2^25 - 1 triangles");
  int rc = select_device(opt ? opt->device : 0);
  if (rc != RT_OK) return rc;

  // (every exit before the release at the end frees what the context holds so far, on this device)
  std::unique_ptr<rt_ctx> c(new rt_ctx());
  c->device = opt ? opt->device : 0;
  c->optLeafMax = opt ? opt->bvh_leaf_max : 0u, c->optBuilder = opt ? opt->bvh_builder : (uint32_t)RT_BVH_AUTO;
  c->optNodeFormat = opt ? opt->node_format : (uint32_t)RT_NODES_AUTO;
  rtk::DevScene& S = c->S;
  Tree tree;
  // (the scene's arrays go to the device once the host passes have accepted the description)
  rc = build_tree(sc, c->optLeafMax, c->optBuilder, c->optNodeFormat, prebuilt, [&](const float** dVpos, const uint4** dTriShade) {
    // (big scenes: the per-triangle and per-vertex host passes of rt_create are shared by a few threads — 8 M triangles
    // spent 60 ms in them on one)
    std::unique_ptr<uint4[]> shade(new uint4[sc->n_triangles]);
    for (uint32_t m = 0; m < sc->n_meshes; ++m)
      par_chunks(sc->mesh_tri_begin[m], sc->mesh_tri_begin[m + 1], [&](uint32_t, size_t tb, size_t te) {
        for (size_t t = tb; t < te; ++t) shade[t] = make_uint4(sc->tri_vtx[3 * t], sc->tri_vtx[3 * t + 1], sc->tri_vtx[3 * t + 2], m);
      });
    int r = upload(&c->triShade, shade.get(), (size_t)sc->n_triangles);
    shade.reset();
    if (r != RT_OK || (r = upload(&c->vpos, sc->vertex_pos, (size_t)sc->n_vertices * 3)) != RT_OK ||
        (r = upload(&c->vnrm, sc->vertex_nrm, (size_t)sc->n_vertices * 3)) != RT_OK)
      return r;
    *dVpos = c->vpos.get(), *dTriShade = c->triShade.get();
    return (int)RT_OK;
  }, &tree);
  if (rc != RT_OK) return rc;
  install_tree(c.get(), &tree);
  std::vector<rtd::DevMat> dm(sc->n_meshes);
  for (uint32_t m = 0; m < sc->n_meshes; ++m) dm[m] = rtd::make_dev_mat(sc->materials[m]);
  if ((rc = upload(&c->mats, sc->materials, sc->n_meshes)) != RT_OK || (rc = upload(&c->matsDev, dm.data(), dm.size())) != RT_OK ||
      (rc = upload(&c->lights, sc->lights, sc->n_lights)) != RT_OK ||
      (rc = upload(&c->meshTriBegin, sc->mesh_tri_begin, sc->n_meshes + 1)) != RT_OK ||
      (rc = upload(&c->meshVtxBegin, sc->mesh_vtx_begin, sc->n_meshes + 1)) != RT_OK)
    return rc;
  S.triShade = c->triShade.get(), S.vpos = c->vpos.get(), S.vnrm = c->vnrm.get();
  S.mats = c->mats.get(), S.matsDev = c->matsDev.get(), S.lights = c->lights.get();
  S.meshTriBegin = c->meshTriBegin.get(), S.meshVtxBegin = c->meshVtxBegin.get();
  S.n_tris = sc->n_triangles;
  S.n_lights = sc->n_lights;
  S.n_photons = 0;
  S.cam = sc->camera;
  c->hostLights.assign(sc->lights, sc->lights + sc->n_lights);
  c->nMeshes = sc->n_meshes, c->nVertices = sc->n_vertices;
  c->magPos = max_abs_bits(sc->vertex_pos, 3 * (size_t)sc->n_vertices);
  c->magNrm = max_abs_bits(sc->vertex_nrm, 3 * (size_t)sc->n_vertices);
  vouch_short_forms(c.get());
  S.phPos = S.phDir = nullptr, S.phTopo = nullptr;
  S.topK = 0;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && cus > 0) c->numCUs = (uint32_t)cus;
  if (dev_alloc(&c->dTileCounter, 1) != hipSuccess) return fail(RT_ERR_HIP, "tile counter allocation failed");
  if (c->numCUs == 0) return fail(RT_ERR_HIP, "device %d reports no compute units", c->device);
  // (the counter block + 1,024 striped slots x 4 for the one-wave-per-workgroup kernels: rt_kernels.hip flush_stats_striped)
  if (dev_alloc(&c->dCounters, RTK_CNT_COUNT + 4096) != hipSuccess ||
      hipMemset(c->dCounters.get(), 0, (RTK_CNT_COUNT + 4096) * sizeof(unsigned long long)) != hipSuccess)
    return fail(RT_ERR_HIP, "counter allocation failed");
  for (auto& pr : c->ev)
    if (make_event(&pr[0]) != hipSuccess || make_event(&pr[1]) != hipSuccess) return fail(RT_ERR_HIP, "event creation failed");
  *out = c.release();
  return RT_OK;
}

// The image of a host form of an integrator, when the caller asked for one: bg goes up, the n slices of npx pixels of
// dAccum are resolved at spp samples over it, each into its slice of the staged out_rgb.
int stage_resolve(Staging* st, const float* bg, float* out_rgb, const float4* dAccum, uint32_t n, size_t npx, uint32_t spp) {
  if (!out_rgb) return RT_OK;
  const float* dBg = st->in(bg, 3 * npx);
  float* dOut = st->out(out_rgb, 3 * n * npx);
  if (st->rc != RT_OK) return st->rc;
  for (uint32_t j = 0; j < n; ++j) {
    const hipError_t he = rtk::launch_resolve((uint32_t)npx, spp, dAccum + j * npx, dBg, dOut + 3 * j * npx, nullptr);
    if (he != hipSuccess) return fail(RT_ERR_HIP, "resolve launch failed: %s", hipGetErrorString(he));
  }
  return RT_OK;
}

// The frame of a checked p into d_accum on `stream`, with a frame's stats: rt_render_device, and (gen) rt_render_lens_device
// and rt_render_shutter_device.
int frame_device(rt_ctx* c, const rt_params* p, const FrameGen& gen, void* d_accum, void* stream, rt_stats* stats) {
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (stats) HIP_TRY(hipMemsetAsync(c->dCounters.get(), 0, RTK_CNT_COUNT * sizeof(unsigned long long), s));
  int e = 0;
  const int rc = launch_frame(c, p, static_cast<float4*>(d_accum), s, &e, nullptr, gen);
  if (rc != RT_OK) return rc;
  if (!stats) return RT_OK;
  // samples of the pixels this rank owns: its granules, clipped to the image
  uint64_t px = 0;
  owned_granules(p->width, p->height, p->rank, p->world, p->tile, [&](uint32_t x8, uint32_t y8) {
    px += (uint64_t)std::min(8u, p->width - x8 * 8) * std::min(8u, p->height - y8 * 8);
  });
  return frame_stats(c, s, e, px * sample_range(*p).count, stats);
}

// What a host form that may return the image, the accumulator or both refuses about its outputs (else null): the
// `outputs` text its checks report in their place.
const char* outputs_refused(const float* bg, const float* out_rgb, const float* accum_out) {
  return !out_rgb && !accum_out ? "neither out_rgb nor accum_out is given"
         : out_rgb && !bg       ? "out_rgb requested without a background image"
                                : nullptr;
}

// The host form of a frame, after its checks: frame_device into a zeroed accumulator of nSlices slices (accum_out's
// staging), every slice resolved over bg where out_rgb is asked for, and the results brought down.
int frame_host(rt_ctx* c, const rt_params* p, const FrameGen& gen, uint32_t nSlices, const float* bg, float* out_rgb,
               float* accum_out, rt_stats* stats) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)p->width * p->height;
  Staging st;
  float4* dAccum = st.zeroed<float4>(accum_out, nSlices * npx);
  if (st.rc != RT_OK) return st.rc;
  rt_stats local;
  int rc = frame_device(c, p, gen, dAccum, nullptr, stats ? stats : &local);
  if (rc != RT_OK) return rc;
  if ((rc = stage_resolve(&st, bg, out_rgb, dAccum, nSlices, npx, p->spp)) != RT_OK) return rc;
  return st.download();
}
}  // namespace

extern "C" {

void rt_destroy(rt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

int rt_set_photons(rt_ctx* c, const float* pos3, const float* dir3, uint32_t n) {
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  if (n && (!pos3 || !dir3)) return fail(RT_ERR_INVALID, "photon arrays are null");
  if (n >= (1u << 30)) return fail(RT_ERR_UNSUPPORTED, "too many photons");
  HIP_TRY(hipSetDevice(c->device));
  int rc = drop_photons(c);
  if (rc != RT_OK) return rc;
  std::vector<float4> p(n), d(n);
  for (uint32_t i = 0; i < n; ++i) {
    p[i] = make_float4(pos3[3 * (size_t)i], pos3[3 * (size_t)i + 1], pos3[3 * (size_t)i + 2], 0.f);
    d[i] = make_float4(dir3[3 * (size_t)i], dir3[3 * (size_t)i + 1], dir3[3 * (size_t)i + 2], 0.f);
  }
  DevBuf<float4> pos, dir;
  DevBuf<uint4> topo;
  if ((rc = upload(&pos, p.data(), n)) != RT_OK || (rc = upload(&dir, d.data(), n)) != RT_OK) return rc;
  if (n) {  // the arrays come in tree order (kdtree.h:60-69): the explicit topology follows from it
    hipError_t he = dev_alloc(&topo, 2 * (size_t)n);
    if (he == hipSuccess) he = rtk::launch_kd_topology(pos.get(), n, topo.get(), nullptr);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return fail(RT_ERR_HIP, "photon topology failed: %s", hipGetErrorString(he));
  }
  install_photons(c, std::move(pos), std::move(dir), std::move(topo), n);
  return RT_OK;
}

int rt_emit_photons(rt_ctx* c, uint32_t n_requested, uint32_t seed, float* pos3, float* dir3, float* weight,
                    uint32_t* n_out) {
  if (!c || !n_out) return fail(RT_ERR_INVALID, "ctx/n_out is null");
  *n_out = 0;
  if (n_requested == 0 || c->S.n_lights == 0) return RT_OK;
  if (!pos3 || !dir3) return fail(RT_ERR_INVALID, "output arrays are null");
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t perLight = photons_per_light(n_requested, c->S.n_lights);
  const uint32_t n = perLight * c->S.n_lights;
  if (n == 0) return RT_OK;
  DevBuf<float4> dPos, dDir;
  HIP_TRY(dev_alloc(&dPos, n));
  if (dev_alloc(&dDir, n) != hipSuccess) return fail(RT_ERR_HIP, "photon buffer allocation failed");
  hipError_t he = rtk::launch_emit(c->S, perLight, seed, dPos.get(), dDir.get(), c->dCounters.get(), nullptr);
  std::vector<float4> hp(n), hd(n);
  if (he == hipSuccess) he = hipMemcpy(hp.data(), dPos.get(), n * sizeof(float4), hipMemcpyDeviceToHost);
  if (he == hipSuccess) he = hipMemcpy(hd.data(), dDir.get(), n * sizeof(float4), hipMemcpyDeviceToHost);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "photon emission failed: %s", hipGetErrorString(he));
  uint32_t m = 0;
  for (uint32_t j = 0; j < n; ++j) {
    if (hp[j].w == 0.f) continue;  // this emitted photon stored no particle
    pos3[3 * (size_t)m] = hp[j].x, pos3[3 * (size_t)m + 1] = hp[j].y, pos3[3 * (size_t)m + 2] = hp[j].z;
    dir3[3 * (size_t)m] = hd[j].x, dir3[3 * (size_t)m + 1] = hd[j].y, dir3[3 * (size_t)m + 2] = hd[j].z;
    if (weight) weight[m] = hd[j].w;
    ++m;
  }
  *n_out = m;
  return RT_OK;
}

int rt_render_device(rt_ctx* c, const rt_params* p, void* d_accum, void* stream, rt_stats* stats) {
  if (!c || !d_accum) return fail(RT_ERR_INVALID, "ctx/d_accum is null");
  const int rc = check_params(c, p);
  if (rc != RT_OK) return rc;
  return frame_device(c, p, FrameGen(), d_accum, stream, stats);
}

int rt_resolve_device(rt_ctx* c, uint32_t width, uint32_t height, uint32_t spp, const void* d_accum,
                      const void* d_bg, void* d_out, void* stream) {
  if (!c || !d_accum || !d_bg || !d_out) return fail(RT_ERR_INVALID, "null argument");
  if (spp == 0) return fail(RT_ERR_INVALID, "spp must be >= 1");
  HIP_TRY(hipSetDevice(c->device));
  hipError_t he = rtk::launch_resolve(width * height, spp, static_cast<const float4*>(d_accum),
                                      static_cast<const float*>(d_bg), static_cast<float*>(d_out),
                                      static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "resolve launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_render(rt_ctx* c, const rt_params* p, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  int rc = check_params(c, p);
  if (rc != RT_OK) return rc;
  if (out_rgb && !bg) return fail(RT_ERR_INVALID, "out_rgb requested without a background image");
  return frame_host(c, p, FrameGen(), 1, bg, out_rgb, accum_out, stats);
}

int rt_render_passes(rt_ctx* c, const rt_params* p, const float* bg, float* accum_io, float* out_rgb, rt_stats* stats) {
  if (!c || !accum_io || !bg || !out_rgb) return fail(RT_ERR_INVALID, "null argument");
  int rc = check_params(c, p);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)p->width * p->height;
  Staging st;
  float4* dAccum = st.inout<float4>(accum_io, npx);
  if (st.rc != RT_OK) return st.rc;
  rt_stats local;
  if ((rc = rt_render_device(c, p, dAccum, nullptr, stats ? stats : &local)) != RT_OK) return rc;
  // (resolved over the samples the accumulator holds so far)
  if ((rc = stage_resolve(&st, bg, out_rgb, dAccum, 1, npx, sample_range(*p).s1)) != RT_OK) return rc;
  return st.download();
}

int rt_trace(rt_ctx* c, const rt_ray* rays, uint32_t n, uint32_t accel, uint32_t kind, rt_hit* hits) {
  if (!c || (n && (!rays || !hits))) return fail(RT_ERR_INVALID, "null argument");
  if (n == 0) return RT_OK;
  HIP_TRY(hipSetDevice(c->device));
  Staging st;
  const rt_ray* dR = st.in(rays, n);
  rt_hit* dH = st.out(hits, n);
  if (st.rc != RT_OK) return st.rc;
  rtk::DevScene Su = c->S;
  Su.slowRecip = 1u;  // the caller's rays: any length
  const hipError_t he = rtk::launch_trace(accel == RT_ACCEL_BRUTE, kind == RT_TRACE_ANY, Su, dR, n, dH, c->dCounters.get(), nullptr);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "trace failed: %s", hipGetErrorString(he));
  return st.download();
}

// rt_knn (k in 1..RTK_KMAX) and rt_knn_wide (1..RT_KNN_KMAX) differ in the cap only: launch_knn_wide runs rt_knn's
// instance for k <= RTK_KMAX
static int knn_common(rt_ctx* c, const float* q3, uint32_t n, uint32_t k, uint32_t kmax, uint32_t* idx, float* dist,
                      uint32_t* visited) {
  if (!c || (n && (!q3 || !idx || !dist))) return fail(RT_ERR_INVALID, "null argument");
  if (c->S.n_photons == 0) return fail(RT_ERR_STATE, "tree is empty");              // kdtree.h:181
  if (k < 1 || k > kmax) return fail(RT_ERR_UNSUPPORTED, "k must be in 1..%u", kmax);
  if (k > c->S.n_photons) return fail(RT_ERR_STATE, "k is greater than the number of nodes");  // kdtree.h:182-183
  if (n == 0) return RT_OK;
  HIP_TRY(hipSetDevice(c->device));
  Staging st;
  const float* dQ = st.in(q3, (size_t)n * 3);
  uint32_t* dI = st.out(idx, (size_t)n * k);
  float* dD = st.out(dist, (size_t)n * k);
  uint32_t* dV = st.work<uint32_t>(visited, n);  // (the walk counts its visits either way)
  if (st.rc != RT_OK) return st.rc;
  // the walk a photon frame runs, on the frame's layout when the BVH is shallower than the kd tree (the tightest one)
  const KdStack ks = kd_stack(c->S.n_photons);
  const hipError_t he = rtk::launch_knn_wide(c->S, dQ, n, k, ks.kd16, stack_levels(ks.rows), dI, dD, dV, nullptr);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "knn failed: %s", hipGetErrorString(he));
  return st.download();
}

int rt_knn(rt_ctx* c, const float* q3, uint32_t n, uint32_t k, uint32_t* idx, float* dist, uint32_t* visited) {
  return knn_common(c, q3, n, k, RTK_KMAX, idx, dist, visited);
}

int rt_knn_wide(rt_ctx* c, const float* q3, uint32_t n, uint32_t k, uint32_t* idx, float* dist, uint32_t* visited) {
  return knn_common(c, q3, n, k, RT_KNN_KMAX, idx, dist, visited);
}

int rt_bvh_info_get(rt_ctx* c, rt_bvh_info* out) {
  if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
  memset(out, 0, sizeof *out);
  out->n_nodes = c->S.n_nodes;
  out->n_tri_records = c->S.n_tris;
  out->max_depth = c->bvh.maxDepth;
  out->leaf_max = c->bvh.leafMax;
  out->pad = c->bvh.pad;
  out->build_ms = c->buildMs;
  out->builder = c->builder;
  out->node_format = c->nodeFormat;
  out->flags = (c->S.slowRecip ? 0u : (uint32_t)RT_BVH_FLAG_SHORT_RECIP) | (c->recipCheck == 2u ? (uint32_t)RT_BVH_FLAG_RECIP_CHECK_FAILED : 0u);
  return RT_OK;
}

int rt_bvh_export(rt_ctx* c, void* nodes64, void* tris48) {
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  if (c->builder != RT_BVH_HOST) {  // the arrays only exist on the device
    HIP_TRY(hipSetDevice(c->device));
    if (nodes64) HIP_TRY(hipMemcpy(nodes64, c->nodesF.get(), (size_t)c->S.n_nodes * sizeof(rtbvh::Node), hipMemcpyDeviceToHost));
    if (tris48) HIP_TRY(hipMemcpy(tris48, c->S.tris, (size_t)c->S.n_tris * sizeof(rtbvh::TriRec), hipMemcpyDeviceToHost));
    return RT_OK;
  }
  if (nodes64) memcpy(nodes64, c->bvh.nodes.data(), c->bvh.nodes.size() * sizeof(rtbvh::Node));
  if (tris48) memcpy(tris48, c->bvh.tris.data(), c->bvh.tris.size() * sizeof(rtbvh::TriRec));
  return RT_OK;
}

int rt_bvh_build_host(const rt_scene_desc* sc, uint32_t leaf_max, uint32_t threads, rt_bvh_info* info,
                      uint64_t* digest, double* seconds) {
  if (!sc || !info || !digest) return fail(RT_ERR_INVALID, "null argument");
  try {
    rtbvh::Built b;
    const auto t0 = std::chrono::steady_clock::now();
    rtbvh::build(*sc, leaf_max, b, threads);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    info->n_nodes = (uint32_t)b.nodes.size(), info->n_tri_records = (uint32_t)b.tris.size();
    info->max_depth = b.maxDepth, info->leaf_max = b.leafMax, info->pad = b.pad;
    uint64_t h = 1469598103934665603ull;  // FNV-1a over float nodes, packed nodes, triangle records
    auto eat = [&h](const void* p, size_t n) {
      const unsigned char* q = static_cast<const unsigned char*>(p);
      for (size_t i = 0; i < n; ++i) h = (h ^ q[i]) * 1099511628211ull;
    };
    eat(b.nodes.data(), b.nodes.size() * sizeof(rtbvh::Node));
    eat(b.nodes16.data(), b.nodes16.size() * sizeof(rtbvh::Node16));
    eat(b.tris.data(), b.tris.size() * sizeof(rtbvh::TriRec));
    *digest = h;
  } catch (const std::exception& e) {
    return fail(RT_ERR_INVALID, "BVH build failed: %s", e.what());
  }
  return RT_OK;
}

int rt_bvh_check_host(const rt_scene_desc* sc, uint32_t leaf_max, uint32_t node_format, uint32_t* out8, double* est2) {
  if (!sc || !out8) return fail(RT_ERR_INVALID, "null argument");
  if (node_format != RT_NODES_F16 && node_format != RT_NODES_Q8) return fail(RT_ERR_INVALID, "node_format must be RT_NODES_F16 or RT_NODES_Q8");
  try {
    rtbvh::Built b;
    rtbvh::build(*sc, leaf_max, b, 0);
    const bool q8 = node_format == RT_NODES_Q8;
    if (q8) rtbvh::packQ8(b);
    const size_t nn = b.nodes16.size();
    if (nn == 0 || nn != b.nodes.size()) return fail(RT_ERR_STATE, "the build produced no packed nodes");
    const float inv = 1.f / b.boxScale;
    std::vector<uint32_t> seen(b.tris.size(), 0);
    std::vector<uint8_t> visited(q8 ? b.q8.size() : nn, 0);
    uint32_t depthSeen = 0;
    double areaSum = 0;  // inner children's decoded box areas (the visit estimate of the packed form)
    // depth-first over the packed tree; returns the float box of the geometry below a child ref
    struct Bx { float lo[3], hi[3]; };
    struct Walker {
      const rt_scene_desc& sc; const rtbvh::Built& b; std::vector<uint32_t>& seen; std::vector<uint8_t>& visited;
      uint32_t& depthSeen; double& areaSum; float inv; bool q8; uint64_t nodes; std::string err;
      Bx walk(int32_t ref, uint32_t depth) {
        Bx r;
        for (int a = 0; a < 3; ++a) r.lo[a] = 3e38f, r.hi[a] = -3e38f;
        depthSeen = std::max(depthSeen, depth);
        if (ref < 0) {  // leaf: ~(byte offset of the first record | count - 1)
          const uint32_t code = ~(uint32_t)ref, cnt = (code & 7u) + 1u;
          if (cnt > b.leafMax) err = "leaf holds more records than leaf_max";
          for (uint32_t t = 0; t < cnt && err.empty(); ++t) {
            rtbvh::TriRec rec;
            if (q8) {  // the records sit in the unified array: identify them by their id, compare with the leaf-order array
              const size_t slot = ((size_t)(code & ~7u) >> 4) + 3u * t;
              if (((code & ~7u) & 15u) || slot + 3 > b.q8.size()) { err = "leaf offset outside the unified array"; break; }
              for (int k = 0; k < 3; ++k)
                if (visited[slot + k]++) err = "a triangle slot is referenced twice";
              memcpy(&rec, &b.q8[slot], sizeof rec);
              if (rec.id >= seen.size() || memcmp(&rec, &b.trisRef[rec.id], sizeof rec) != 0) { err = "a triangle record of the unified array is not the scene's"; break; }
              seen[rec.id]++;
            } else {
              const uint32_t i = (code & ~7u) / 48u + t;
              if ((code & ~7u) % 48u) err = "leaf offset is not a multiple of 48";
              if (i >= seen.size()) { err = "leaf range beyond the triangle array"; break; }
              seen[i]++;
              rec = b.tris[i];
            }
            for (int k = 0; k < 3; ++k) {
              const float* q = sc.vertex_pos + 3 * (size_t)sc.tri_vtx[3 * (size_t)rec.id + k];
              for (int a = 0; a < 3; ++a) r.lo[a] = std::min(r.lo[a], q[a]), r.hi[a] = std::max(r.hi[a], q[a]);
            }
          }
          return r;
        }
        float lo[2][3], hi[2][3];
        int32_t child[2];
        if (q8) {
          if ((size_t)((uint32_t)ref >> 4) >= visited.size()) { err = "inner ref beyond the unified array"; return r; }
          if (visited[(uint32_t)ref >> 4]++) { err = "node reached twice"; return r; }
          rtbvh::decodeQ8(b, (uint32_t)ref, lo, hi, child);
        } else {
          if (ref % 32) { err = "inner ref is not a multiple of 32"; return r; }
          const uint32_t idx = (uint32_t)ref / 32u;
          if (idx >= visited.size()) { err = "inner ref beyond the node array"; return r; }
          if (visited[idx]++) { err = "node reached twice"; return r; }
          const rtbvh::Node16& n = b.nodes16[idx];
          for (int i = 0; i < 2; ++i) {
            const uint16_t* q = i ? n.box1 : n.box0;
            for (int a = 0; a < 3; ++a) lo[i][a] = rtbvh::halfToFloat(q[2 * a]) * inv, hi[i][a] = rtbvh::halfToFloat(q[2 * a + 1]) * inv;
            child[i] = n.child[i];
          }
        }
        ++nodes;
        for (int i = 0; i < 2 && err.empty(); ++i) {
          const Bx c = walk(child[i], depth + 1u);
          if (child[i] >= 0) {
            const double dx = (double)hi[i][0] - lo[i][0], dy = (double)hi[i][1] - lo[i][1], dz = (double)hi[i][2] - lo[i][2];
            areaSum += dx * dy + dy * dz + dz * dx;
          }
          for (int a = 0; a < 3; ++a) {
            // the stored box must contain the geometry below it, padded
            if (!(lo[i][a] <= c.lo[a] - 0.999f * b.pad && hi[i][a] >= c.hi[a] + 0.999f * b.pad)) err = "a child box does not contain its padded geometry";
            r.lo[a] = std::min(r.lo[a], c.lo[a]), r.hi[a] = std::max(r.hi[a], c.hi[a]);
          }
        }
        return r;
      }
    } W{*sc, b, seen, visited, depthSeen, areaSum, inv, q8, 0, {}};
    W.walk(q8 ? (int32_t)rtbvh::kQ8RootOffset : 0, 0);
    if (!W.err.empty()) return fail(RT_ERR_STATE, "BVH check: %s", W.err.c_str());
    // (a one-triangle scene has that triangle under both children of its root: bvh_build.cpp build())
    for (uint32_t v : seen)
      if (v != 1 && !(sc->n_triangles == 1 && v == 2)) return fail(RT_ERR_STATE, "BVH check: a triangle record is referenced %u times", v);
    if (W.nodes != nn) return fail(RT_ERR_STATE, "BVH check: %llu of %zu nodes reachable", (unsigned long long)W.nodes, nn);
    if (depthSeen != b.maxDepth) return fail(RT_ERR_STATE, "BVH check: deepest leaf at level %u, builder says %u", depthSeen, b.maxDepth);
    if ((int)depthSeen > b.depthCap) return fail(RT_ERR_STATE, "BVH check: depth %u exceeds the cap %d", depthSeen, b.depthCap);
    out8[0] = (uint32_t)nn, out8[1] = (uint32_t)b.q8.size(), out8[2] = b.q8Blocks, out8[3] = b.maxDepth;
    out8[4] = out8[5] = out8[6] = out8[7] = 0;
    // the surface-area estimate of node visits per random ray: the root plus every inner child by its box area
    if (est2) {
      auto area = [](const float* lo, const float* hi) {
        const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
      };
      const rtbvh::Node& n0 = b.nodes[0];
      float lo[3], hi[3];
      for (int a = 0; a < 3; ++a) lo[a] = std::min(n0.lo0[a], n0.lo1[a]), hi[a] = std::max(n0.hi0[a], n0.hi1[a]);
      const double rootArea = std::max(area(lo, hi), 1e-300);
      double v = 0;
      for (const rtbvh::Node& n : b.nodes) {
        if (n.child[0] >= 0) v += area(n.lo0, n.hi0);
        if (n.child[1] >= 0) v += area(n.lo1, n.hi1);
      }
      est2[0] = 1.0 + v / rootArea, est2[1] = 1.0 + areaSum / rootArea;
    }
  } catch (const std::exception& e) {
    return fail(RT_ERR_INVALID, "BVH check failed: %s", e.what());
  }
  return RT_OK;
}

int rt_bvh_top_check_host(const rt_scene_desc* sc, uint32_t leaf_max, uint32_t cutoff, uint32_t* out8) {
  if (!sc || !out8) return fail(RT_ERR_INVALID, "null argument");
  try {
    rtbvh::TopBuilt t;
    rtbvh::buildTop(*sc, leaf_max, cutoff, t);
    const uint32_t n = sc->n_triangles;
    if (t.order.size() != n) return fail(RT_ERR_STATE, "top check: the order has %zu entries for %u triangles", t.order.size(), n);
    std::vector<uint8_t> seenTri(n, 0), covered(n, 0), partRef(t.parts.size(), 0);
    for (uint32_t id : t.order) {
      if (id >= n || seenTri[id]++) return fail(RT_ERR_STATE, "top check: the order is not a permutation");
    }
    auto geomBox = [&](uint32_t b, uint32_t e, float* lo, float* hi) {
      for (int a = 0; a < 3; ++a) lo[a] = 3e38f, hi[a] = -3e38f;
      for (uint32_t i = b; i < e; ++i)
        for (int k = 0; k < 3; ++k) {
          const float* q = sc->vertex_pos + 3 * (size_t)sc->tri_vtx[3 * (size_t)t.order[i] + k];
          for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], q[a]), hi[a] = std::max(hi[a], q[a]);
        }
    };
    uint32_t largest = 0, deepest = 0, topLeaves = 0;
    for (uint32_t i = 0; i < t.nodes.size(); ++i)
      for (int c = 0; c < 2; ++c) {
        const int32_t ref = t.nodes[i].child[c];
        const float* blo = c ? t.nodes[i].lo1 : t.nodes[i].lo0;
        const float* bhi = c ? t.nodes[i].hi1 : t.nodes[i].hi0;
        uint32_t b = 0, e = 0;
        if (ref >= 0) {
          if ((uint32_t)ref >= t.nodes.size() || (uint32_t)ref == i) return fail(RT_ERR_STATE, "top check: bad inner ref");
          continue;
        }
        const uint32_t code = ~(uint32_t)ref;
        if (code & rtbvh::kPartFlag) {
          const uint32_t k = code & (rtbvh::kPartFlag - 1u);
          if (k >= t.parts.size() || partRef[k]++) return fail(RT_ERR_STATE, "top check: part %u referred to twice or out of range", k);
          const rtbvh::TopBuilt::Part& P = t.parts[k];
          if (P.parent != i || P.slot != (uint32_t)c) return fail(RT_ERR_STATE, "top check: part %u names another referrer", k);
          b = P.b, e = P.e;
          if (e <= b || e > n || e - b > cutoff || e - b <= t.leafMax) return fail(RT_ERR_STATE, "top check: part %u has %u triangles", k, e - b);
          largest = std::max(largest, e - b), deepest = std::max(deepest, P.depth);
          // its subtree must still fit below: ceil(log2(triangles / leafMax)) more levels at least
          uint32_t need = 0;
          for (uint32_t m = e - b; m > t.leafMax; m = (m + 1) / 2) ++need;
          if ((int)(P.depth + need) > t.depthCap) return fail(RT_ERR_STATE, "top check: part %u at depth %u cannot be split within the cap %d", k, P.depth, t.depthCap);
        } else {
          b = code >> 3, e = b + (code & 7u) + 1u;
          if (e > n || e - b > t.leafMax) return fail(RT_ERR_STATE, "top check: bad leaf");
          ++topLeaves;
        }
        for (uint32_t j = b; j < e; ++j)
          if (covered[j]++) return fail(RT_ERR_STATE, "top check: position %u of the order is covered twice", j);
        float lo[3], hi[3];
        geomBox(b, e, lo, hi);
        for (int a = 0; a < 3; ++a)
          if (!(blo[a] <= lo[a] - 0.999f * t.pad && bhi[a] >= hi[a] + 0.999f * t.pad)) return fail(RT_ERR_STATE, "top check: a child box does not contain its padded geometry");
      }
    for (uint32_t j = 0; j < n; ++j)
      if (covered[j] != 1) return fail(RT_ERR_STATE, "top check: position %u of the order is not covered", j);
    for (size_t k = 0; k + 1 < t.parts.size(); ++k)
      if (t.parts[k].b >= t.parts[k + 1].b) return fail(RT_ERR_STATE, "top check: parts are not in order");
    out8[0] = (uint32_t)t.nodes.size(), out8[1] = (uint32_t)t.parts.size(), out8[2] = largest, out8[3] = deepest;
    out8[4] = (uint32_t)t.depthCap, out8[5] = topLeaves, out8[6] = out8[7] = 0;
  } catch (const std::exception& e) {
    return fail(RT_ERR_INVALID, "top check failed: %s", e.what());
  }
  return RT_OK;
}

int rt_bvh_tune(rt_ctx* c, const rt_params* probe, double budget_seconds, uint32_t max_probes, rt_tune_report* out) {
  if (!c || !probe) return fail(RT_ERR_INVALID, "ctx/probe is null");
  if (out) memset(out, 0, sizeof *out);
  if (c->builder != RT_BVH_HOST || c->bvh.nodes.empty() || c->nodeFormat != RT_NODES_F16)
    return fail(RT_ERR_STATE, "rt_bvh_tune needs a host-built tree in the RT_NODES_F16 format");
  if (probe->use_photons || probe->accel != RT_ACCEL_BVH) return fail(RT_ERR_INVALID, "the probe must be a BVH render without the photon map");
  int rc = check_params(c, probe);
  if (rc != RT_OK) return rc;
  if (!(budget_seconds > 0)) return RT_OK;
  HIP_TRY(hipSetDevice(c->device));
  // (the tree may change: rt_update uploads it again)
  c->nodesF.reset(), c->refitDepth.reset();
  if (c->refits == 0) c->costBuiltValid = false;  // (rt_bvh_quality's baseline of a tree never refit is taken again: the numbering may change)
  DevBuf<float4> dAcc;
  HIP_TRY(dev_alloc(&dAcc, (size_t)probe->width * probe->height));
  rt_params p = *probe;
  p.collect_stats = 1;
  const size_t nodeBytes = c->bvh.nodes.size() * sizeof(rtbvh::Node16);
  std::string err;
  auto upload = [&]() -> bool {
    if (hipMemcpy(c->nodes.get(), c->bvh.nodes16.data(), nodeBytes, hipMemcpyHostToDevice) != hipSuccess) {
      err = "node upload failed";
      return false;
    }
    return true;
  };
  auto measure = [&]() -> double {
    if (!err.empty()) return 1e300;
    rtbvh::packNodes(c->bvh);
    if (!upload()) return 1e300;
    if (hipMemset(dAcc.get(), 0, (size_t)p.width * p.height * sizeof(float4)) != hipSuccess) {
      err = "probe accumulator reset failed";
      return 1e300;
    }
    rt_stats st;
    if (rt_render_device(c, &p, dAcc.get(), nullptr, &st) != RT_OK) {
      err = std::string("probe render failed: ") + rt_last_error();
      return 1e300;
    }
    return (double)st.nodes_visited + 1.5 * (double)st.tris_tested;
  };
  // A second probe (another seed: other jitter, other light samples, other bounce directions) is the referee: a tuned
  // tree that does not also beat the original on rays it was not tuned on is dropped (over-fitting shows on scenes
  // whose probe is too small for their triangle count).
  rtbvh::TuneReport rep;
  bool kept = true;
  const std::vector<rtbvh::Node> original = c->bvh.nodes;
  const uint32_t depth0 = c->bvh.maxDepth;
  try {
    rt_params pv = p;
    pv.seed = p.seed ^ 0x9e3779b9u;
    auto referee = [&]() {
      const rt_params keep = p;
      p = pv;
      const double v = measure();
      p = keep;
      return v;
    };
    const double v0 = referee();
    rep = rtbvh::tuneMeasured(c->bvh, measure, budget_seconds, max_probes, getenv("RT_BVH_VERBOSE") != nullptr);
    const double v1 = referee();
    if (getenv("RT_BVH_VERBOSE")) fprintf(stderr, "tune referee probe: %.6g -> %.6g\n", v0, v1);
    if (!(v1 < v0)) c->bvh.nodes = original, c->bvh.maxDepth = depth0, kept = false;
    // final numbering (the LDS-resident prefix is chosen by area from the root) and the device copy
    rtbvh::relayoutAndPack(c->bvh);
  } catch (const std::exception& e) {
    err = e.what();
  }
  if (!err.empty()) {
    // a failed probe, upload or builder step: the context goes back to the tree it came with, host AND device side
    // (the device may hold whichever candidate was uploaded last)
    const std::string why = err;
    err.clear();
    try {
      c->bvh.nodes = original, c->bvh.maxDepth = depth0;
      rtbvh::relayoutAndPack(c->bvh);
    } catch (const std::exception& e) {
      err = e.what();
    }
    if (err.empty()) upload();
    if (!err.empty()) {  // not even that: the device tree is unknown, the context must not render again
      c->broken = true;
      return fail(RT_ERR_STATE, "rt_bvh_tune: %s; restoring the original tree failed too (%s): the context is unusable", why.c_str(), err.c_str());
    }
    return fail(RT_ERR_HIP, "rt_bvh_tune: %s (the original tree is back in place)", why.c_str());
  }
  upload();
  if (!err.empty()) {
    c->broken = true;
    return fail(RT_ERR_STATE, "rt_bvh_tune: %s: the context is unusable", err.c_str());
  }
  if (kept && rep.accepted) c->costBuiltValid = false, c->refits = 0;  // an accepted tuning is a build (rt_bvh_quality)
  if (out) out->probes = rep.probes, out->accepted = kept ? rep.accepted : 0u, out->cost_before = rep.cost0, out->cost_after = kept ? rep.cost1 : rep.cost0, out->seconds = rep.seconds;
  return RT_OK;
}

int rt_profile_reset(rt_ctx* c) {
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  c->evUsed = 0;
  return RT_OK;
}

int rt_profile_collect(rt_ctx* c, double* total_ms, uint32_t* launches) {
  if (!c || !total_ms || !launches) return fail(RT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const int n = c->evUsed < kEventPairs ? c->evUsed : kEventPairs;
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    HIP_TRY(event_pair_ms(c, i, &ms));
    sum += ms;
  }
  *total_ms = sum, *launches = static_cast<uint32_t>(n);
  return RT_OK;
}

int rt_test_unit(int32_t device, uint32_t which, const void* in, void* out, uint32_t n) {
  static const uint32_t inBytes[] = {8, 4, 4, 16, 60, 68, 56, 96, 112, 88, 8, 4, 68, 16};
  static const uint32_t outBytes[] = {8, 4, 4, 4, 16, 12, 24, 12, 48, 16, 16, 16, 36, 16};
  if (which > RT_UNIT_HEMISPHERE) return fail(RT_ERR_INVALID, "unknown unit %u", which);
  if (n && (!in || !out)) return fail(RT_ERR_INVALID, "null argument");
  if (n == 0) return RT_OK;
  int rc = select_device(device);
  if (rc != RT_OK) return rc;
  // RT_UNIT_BSDF_HOISTED: the device reads each row followed by the record rt_create would make of its material
  std::vector<float> hoisted;
  size_t devInBytes = inBytes[which];
  if (which == RT_UNIT_BSDF_HOISTED) {
    static_assert(sizeof(rtd::DevMat) == 16 * sizeof(float) && sizeof(rt_material) == 8 * sizeof(float), "unit row layout");
    devInBytes = (17 + 16) * sizeof(float);
    hoisted.resize((size_t)n * 33);
    for (uint32_t i = 0; i < n; ++i) {
      const float* row = static_cast<const float*>(in) + 17 * (size_t)i;
      rt_material m;
      memcpy(&m, row, sizeof(m));  // kd alpha albedo3 f03
      const rtd::DevMat dm = rtd::make_dev_mat(m);
      memcpy(&hoisted[33 * (size_t)i], row, 17 * sizeof(float));
      memcpy(&hoisted[33 * (size_t)i + 17], &dm, sizeof(dm));
    }
    in = hoisted.data();
  }
  DevBuf<char> dIn, dOut;
  HIP_TRY(dev_alloc(&dIn, (size_t)n * devInBytes));
  hipError_t he = dev_alloc(&dOut, (size_t)n * outBytes[which]);
  if (he == hipSuccess) he = hipMemcpy(dIn.get(), in, (size_t)n * devInBytes, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(dOut.get(), out, (size_t)n * outBytes[which], hipMemcpyHostToDevice);
  if (he == hipSuccess) he = rtk::launch_unit(which, dIn.get(), dOut.get(), n, nullptr);
  if (he == hipSuccess) he = hipMemcpy(out, dOut.get(), (size_t)n * outBytes[which], hipMemcpyDeviceToHost);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "unit kernel failed: %s", hipGetErrorString(he));
  return RT_OK;
}

// ------------------------------------------------------------------ ray streams
int rt_trace_stream_device(rt_ctx* c, const void* d_ray_o, const void* d_ray_d, uint32_t n, void* d_res, void* stream) {
  if (!c || (n && (!d_ray_o || !d_ray_d || !d_res))) return fail(RT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t levels = (c->bvh.maxDepth > 1 ? c->bvh.maxDepth : 1) + 1u;
  rtk::DevScene Su = c->S;
  Su.slowRecip = 1u;  // the caller's rays: any length
  hipError_t he = rtk::launch_trace_stream(Su, static_cast<const float4*>(d_ray_o), static_cast<const float4*>(d_ray_d), n,
                                           static_cast<uint2*>(d_res), c->dTileCounter.get(), levels, c->numCUs,
                                           static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "stream trace launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

// ------------------------------------------------------------------ photon map on the device
int rt_build_photon_map(rt_ctx* c, uint32_t n_requested, uint32_t seed, uint32_t* n_stored, double* ms_out) {
  if (!c || !n_stored) return fail(RT_ERR_INVALID, "ctx/n_stored is null");
  *n_stored = 0;
  HIP_TRY(hipSetDevice(c->device));
  (void)drop_photons(c);  // forget the old map first (a failed free does not stop the new one)
  if (n_requested == 0 || c->S.n_lights == 0) return RT_OK;
  const uint32_t perLight = photons_per_light(n_requested, c->S.n_lights);
  const uint32_t n = perLight * c->S.n_lights;
  if (n == 0) return RT_OK;
  DevBuf<float4> slotPos, slotDir, items, phPos, phDir;
  DevBuf<uint4> phTopo;
  DevBuf<uint32_t> dCount;
  Event ev[3];
  hipError_t he = dev_alloc(&slotPos, n);
  if (he == hipSuccess) he = dev_alloc(&slotDir, n);
  if (he == hipSuccess) he = dev_alloc(&items, n);
  if (he == hipSuccess) he = dev_alloc(&dCount, 1);
  for (Event& e : ev)
    if (he == hipSuccess) he = make_event(&e);
  if (he == hipSuccess) he = hipEventRecord(ev[0].get(), nullptr);
  if (he == hipSuccess) he = rtk::launch_emit(c->S, perLight, seed, slotPos.get(), slotDir.get(), c->dCounters.get(), nullptr);
  if (he == hipSuccess) he = rtk::launch_photon_compact(slotPos.get(), n, items.get(), dCount.get(), nullptr);
  if (he == hipSuccess) he = hipEventRecord(ev[1].get(), nullptr);
  uint32_t m = 0;
  if (he == hipSuccess) he = hipMemcpy(&m, dCount.get(), sizeof m, hipMemcpyDeviceToHost);  // (the count only)
  if (he == hipSuccess && m) {
    he = rtk::launch_kd_build(items.get(), m, -1, nullptr);
    if (he == hipSuccess) he = dev_alloc(&phPos, m);
    if (he == hipSuccess) he = dev_alloc(&phDir, m);
    if (he == hipSuccess) he = dev_alloc(&phTopo, 2 * (size_t)m);
    if (he == hipSuccess) he = rtk::launch_photon_gather(items.get(), slotDir.get(), m, phPos.get(), phDir.get(), nullptr, nullptr);
    if (he == hipSuccess) he = rtk::launch_kd_topology(phPos.get(), m, phTopo.get(), nullptr);
  }
  if (he == hipSuccess) he = hipEventRecord(ev[2].get(), nullptr);
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(RT_ERR_HIP, "photon map build failed: %s", hipGetErrorString(he));
  if (ms_out) {
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, ev[0].get(), ev[1].get());
    (void)hipEventElapsedTime(&b, ev[1].get(), ev[2].get());
    ms_out[0] = a, ms_out[1] = b;  // emission + compaction, kd order + gather
  }
  install_photons(c, std::move(phPos), std::move(phDir), std::move(phTopo), m);
  *n_stored = m;
  return RT_OK;
}

int rt_get_photons(rt_ctx* c, float* pos3, float* dir3, float* weight, uint32_t cap, uint32_t* n_out) {
  if (!c || !n_out) return fail(RT_ERR_INVALID, "ctx/n_out is null");
  const uint32_t n = c->S.n_photons;
  *n_out = n;
  if (n == 0) return RT_OK;
  if (cap < n) return fail(RT_ERR_INVALID, "capacity %u < %u photons", cap, n);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<float4> p(n), d(n);
  HIP_TRY(hipMemcpy(p.data(), c->phPos.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(d.data(), c->phDir.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    if (pos3) pos3[3 * (size_t)i] = p[i].x, pos3[3 * (size_t)i + 1] = p[i].y, pos3[3 * (size_t)i + 2] = p[i].z;
    if (dir3) dir3[3 * (size_t)i] = d[i].x, dir3[3 * (size_t)i + 1] = d[i].y, dir3[3 * (size_t)i + 2] = d[i].z;
    if (weight) weight[i] = d[i].w;
  }
  return RT_OK;
}

int rt_test_kd_order(int32_t device, const float* pos3, uint32_t n, int32_t depth_limit, uint32_t* perm_out, double* ms_out) {
  if (n && (!pos3 || !perm_out)) return fail(RT_ERR_INVALID, "null argument");
  if (n == 0) return RT_OK;
  int rc = select_device(device);
  if (rc != RT_OK) return rc;
  std::vector<float4> h(n);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t bits = i;
    float f;
    memcpy(&f, &bits, 4);
    h[i] = make_float4(pos3[3 * (size_t)i], pos3[3 * (size_t)i + 1], pos3[3 * (size_t)i + 2], f);
  }
  DevBuf<float4> items, scratch;
  DevBuf<uint32_t> dPerm;
  Event e0, e1;
  rc = upload(&items, h.data(), n);
  if (rc != RT_OK) return rc;
  hipError_t he = dev_alloc(&scratch, n);
  if (he == hipSuccess) he = dev_alloc(&dPerm, n);
  if (he == hipSuccess) he = make_event(&e0);
  if (he == hipSuccess) he = make_event(&e1);
  if (he == hipSuccess) he = hipEventRecord(e0.get(), nullptr);
  if (he == hipSuccess) he = rtk::launch_kd_build(items.get(), n, depth_limit, nullptr);
  if (he == hipSuccess) he = hipEventRecord(e1.get(), nullptr);
  if (he == hipSuccess) he = rtk::launch_photon_gather(items.get(), nullptr, n, scratch.get(), nullptr, dPerm.get(), nullptr);
  if (he == hipSuccess) he = hipMemcpy(perm_out, dPerm.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (he == hipSuccess && ms_out) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0.get(), e1.get());
    *ms_out = ms;
  }
  if (he != hipSuccess) return fail(RT_ERR_HIP, "kd order failed: %s", hipGetErrorString(he));
  return RT_OK;
}

// ------------------------------------------------------------------ multi-GPU frame assembly
int rt_owned_granules(const rt_params* p, uint32_t rank, uint32_t* n_out) {
  if (!p || !n_out) return fail(RT_ERR_INVALID, "null argument");
  if (p->tile % 8 != 0) return fail(RT_ERR_INVALID, "tile must be a multiple of 8");
  *n_out = 0;
  owned_granules(p->width, p->height, rank, p->world, p->tile, [&](uint32_t, uint32_t) { ++*n_out; });
  return RT_OK;
}

int rt_pack_owned_device(rt_ctx* c, const rt_params* p, const void* d_accum, void* d_packed, void* stream) {
  if (!c || !p || !d_accum || !d_packed) return fail(RT_ERR_INVALID, "null argument");
  if (p->tile % 8 != 0 || (p->world > 1 && p->rank >= p->world)) return fail(RT_ERR_INVALID, "bad rank/world/tile");
  HIP_TRY(hipSetDevice(c->device));
  const rt_ctx::GranList* L = nullptr;
  int rc = ensure_granules(c, p, p->rank, static_cast<hipStream_t>(stream), &L);
  if (rc != RT_OK) return rc;
  hipError_t he = rtk::launch_pack(false, static_cast<const float4*>(d_accum), static_cast<float4*>(d_packed), L->d.get(), L->n, p->width,
                                   p->height, static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "pack launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_unpack_owned_device(rt_ctx* c, const rt_params* p, uint32_t from_rank, const void* d_packed, void* d_accum, void* stream) {
  if (!c || !p || !d_accum || !d_packed) return fail(RT_ERR_INVALID, "null argument");
  if (p->tile % 8 != 0 || from_rank >= (p->world ? p->world : 1)) return fail(RT_ERR_INVALID, "bad rank/world/tile");
  HIP_TRY(hipSetDevice(c->device));
  const rt_ctx::GranList* L = nullptr;
  int rc = ensure_granules(c, p, from_rank, static_cast<hipStream_t>(stream), &L);
  if (rc != RT_OK) return rc;
  hipError_t he = rtk::launch_pack(true, static_cast<const float4*>(d_packed), static_cast<float4*>(d_accum), L->d.get(), L->n, p->width,
                                   p->height, static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "unpack launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ rt_group: N devices, one process
// RCCL is reached through dlopen: single-GPU users of librt_amd.so never load it.
namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool load() {
    if (lib) return true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) return false;
#define SYM(field, name) field = reinterpret_cast<decltype(field)>(dlsym(lib, name))
    SYM(CommInitAll, "ncclCommInitAll");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(Send, "ncclSend");
    SYM(Recv, "ncclRecv");
    SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    return CommInitAll && CommDestroy && Send && Recv && GroupStart && GroupEnd && GetErrorString;
  }
};
Rccl g_rccl;
}  // namespace

struct rt_group {
  std::vector<rt_ctx*> ctx;
  std::vector<int> dev;
  std::vector<Stream> stream;
  Stream xstream;   // device 0: receives and scatters the other ranks' granules beside rank 0's own render
  Event assembled;  // ... and tells stream[0] when the frame is whole
  std::vector<Event> packed_ready;
  std::vector<DevBuf<float4>> accum;   // [rank] full frame on that rank's device
  std::vector<DevBuf<float4>> packed;  // [rank] owned granules, on that rank's device (rank > 0)
  std::vector<DevBuf<float4>> recv;    // [rank] the same bytes on device 0 (rank > 0)
  std::vector<ncclComm_t> comm; // RCCL communicators (all devices distinct), else empty: peer copies
  DevBuf<float> dBg, dOut;
  size_t npx = 0;
  uint32_t fw = 0, fh = 0, ftile = 0;  // what the frame buffers are sized for
  uint32_t tile = 32;
  bool rccl = false;
};

namespace {
// (each rank's resources are released with that rank's device current)
void group_free_frame(rt_group* g) {
  for (size_t r = 0; r < g->ctx.size(); ++r) {
    (void)hipSetDevice(g->dev[r]);
    g->accum[r].reset(), g->packed[r].reset();
  }
  (void)hipSetDevice(g->dev[0]);
  for (auto& p : g->recv) p.reset();
  g->dBg.reset(), g->dOut.reset();
  g->npx = 0, g->fw = g->fh = g->ftile = 0;
}
}  // namespace

extern "C" {

int rt_group_create(const rt_scene_desc* scene, const int32_t* devices, uint32_t n, const rt_options* opt, rt_group** out) {
  if (!scene || !devices || !out || n == 0) return fail(RT_ERR_INVALID, "scene/devices/out is null or n == 0");
  if (n > 64) return fail(RT_ERR_INVALID, "at most 64 devices");
  *out = nullptr;
  // (a failure below releases the group by rt_group_destroy, and the failing rank's own stream, event and context by
  // scope: none of them touches the g_err message the caller reads)
  std::unique_ptr<rt_group, void (*)(rt_group*)> g(new rt_group(), rt_group_destroy);
  bool distinct = true;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t q = 0; q < r; ++q) distinct = distinct && devices[r] != devices[q];
  // (sized before the first context exists: rt_group_destroy -> group_free_frame walks these for every context so far)
  g->accum.resize(n), g->packed.resize(n), g->recv.resize(n);
  for (uint32_t r = 0; r < n; ++r) {
    rt_options o{};
    if (opt) o = *opt;
    o.device = devices[r];
    rt_ctx* created = nullptr;
    // the host tree is built by the first context and copied by the others
    const rtbvh::Built* shared = (r > 0 && g->ctx[0]->builder == RT_BVH_HOST) ? &g->ctx[0]->bvh : nullptr;
    int rc = create_ctx(scene, &o, shared, &created);
    if (rc != RT_OK) return rc;
    std::unique_ptr<rt_ctx> c(created);  // (create_ctx left its device current)
    Stream s;
    Event e;
    if (make_stream(&s) != hipSuccess || make_event(&e, hipEventDisableTiming) != hipSuccess)
      return fail(RT_ERR_HIP, "stream/event creation failed on device %d", devices[r]);
    g->ctx.push_back(c.release()), g->dev.push_back(devices[r]), g->stream.push_back(std::move(s)), g->packed_ready.push_back(std::move(e));
  }
  (void)hipSetDevice(g->dev[0]);
  if (make_stream(&g->xstream) != hipSuccess || make_event(&g->assembled, hipEventDisableTiming) != hipSuccess)
    return fail(RT_ERR_HIP, "exchange stream creation failed on device %d", devices[0]);
  // exchange path: RCCL send/recv when every rank has its own device (ncclCommInitAll refuses
  // duplicates); ranks sharing a device (rehearsal on one GPU) use peer copies
  if (((n > 1 && distinct) || (n == 1 && getenv("RT_GROUP_FORCE_RCCL"))) && !getenv("RT_GROUP_NO_RCCL")) {
    if (!g_rccl.load())
      return fail(RT_ERR_UNSUPPORTED, "librccl.so could not be loaded (%s); set RT_GROUP_NO_RCCL=1 for peer copies", dlerror());
    g->comm.assign(n, nullptr);
    ncclResult_t nr = g_rccl.CommInitAll(g->comm.data(), static_cast<int>(n), g->dev.data());
    if (nr != ncclSuccess) {
      g->comm.clear();
      return fail(RT_ERR_HIP, "ncclCommInitAll failed: %s", g_rccl.GetErrorString(nr));
    }
    g->rccl = true;
  }
  *out = g.release();
  return RT_OK;
}

void rt_group_destroy(rt_group* g) {
  if (!g) return;
  if (!g->ctx.empty()) group_free_frame(g);
  for (ncclComm_t c : g->comm)
    if (c) (void)g_rccl.CommDestroy(c);
  if (!g->dev.empty()) (void)hipSetDevice(g->dev[0]);
  g->xstream.reset(), g->assembled.reset();
  for (size_t r = 0; r < g->ctx.size(); ++r) {
    (void)hipSetDevice(g->dev[r]);
    g->stream[r].reset(), g->packed_ready[r].reset();
    rt_destroy(g->ctx[r]);
  }
  delete g;
}

uint32_t rt_group_size(const rt_group* g) { return g ? static_cast<uint32_t>(g->ctx.size()) : 0; }
int rt_group_uses_rccl(const rt_group* g) { return g && g->rccl ? 1 : 0; }
rt_ctx* rt_group_ctx(rt_group* g, uint32_t rank) { return g && rank < g->ctx.size() ? g->ctx[rank] : nullptr; }

int rt_group_set_photons(rt_group* g, const float* pos3, const float* dir3, uint32_t n) {
  if (!g) return fail(RT_ERR_INVALID, "group is null");
  for (rt_ctx* c : g->ctx) {
    int rc = rt_set_photons(c, pos3, dir3, n);
    if (rc != RT_OK) return rc;
  }
  return RT_OK;
}

int rt_group_render(rt_group* g, const rt_params* p, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  if (!g) return fail(RT_ERR_INVALID, "group is null");
  const uint32_t n = static_cast<uint32_t>(g->ctx.size());
  int rc = check_params(g->ctx[0], p);
  if (rc != RT_OK) return rc;
  if (out_rgb && !bg) return fail(RT_ERR_INVALID, "out_rgb requested without a background image");
  const size_t npx = (size_t)p->width * p->height;
  rt_params base = *p;
  base.world = n, base.tile = p->tile ? p->tile : g->tile;
  std::vector<uint32_t> cnt(n, 0);
  for (uint32_t r = 0; r < n; ++r) owned_granules(p->width, p->height, r, n, base.tile, [&](uint32_t, uint32_t) { ++cnt[r]; });
  if (p->width != g->fw || p->height != g->fh || base.tile != g->ftile) {  // frame buffers for this image size and sharding
    group_free_frame(g);
    for (uint32_t r = 0; r < n; ++r) {
      HIP_TRY(hipSetDevice(g->dev[r]));
      HIP_TRY(dev_alloc(&g->accum[r], npx));
      if (r > 0 && cnt[r]) HIP_TRY(dev_alloc(&g->packed[r], (size_t)cnt[r] * 64));
    }
    HIP_TRY(hipSetDevice(g->dev[0]));
    for (uint32_t r = 1; r < n; ++r)
      if (cnt[r]) HIP_TRY(dev_alloc(&g->recv[r], (size_t)cnt[r] * 64));
    HIP_TRY(dev_alloc(&g->dBg, npx * 3));
    HIP_TRY(dev_alloc(&g->dOut, npx * 3));
    g->npx = npx, g->fw = p->width, g->fh = p->height, g->ftile = base.tile;
  }
  // 1. every rank integrates its tiles (asynchronously, each on its own device and stream)
  std::vector<int> ev(n, 0);
  for (uint32_t r = 0; r < n; ++r) {
    rt_params pr = base;
    pr.rank = r;
    HIP_TRY(hipSetDevice(g->dev[r]));
    hipStream_t s = g->stream[r].get();
    HIP_TRY(hipMemsetAsync(g->accum[r].get(), 0, npx * sizeof(float4), s));
    if (r == 0) {  // the exchange stream scatters into this buffer: only after it has been zeroed
      HIP_TRY(hipEventRecord(g->assembled.get(), s));
      HIP_TRY(hipStreamWaitEvent(g->xstream.get(), g->assembled.get(), 0));
    }
    HIP_TRY(hipMemsetAsync(g->ctx[r]->dCounters.get(), 0, RTK_CNT_COUNT * sizeof(unsigned long long), s));
    rc = launch_frame(g->ctx[r], &pr, g->accum[r].get(), s, &ev[r]);
    if (rc != RT_OK) return rc;
    if (r > 0 && cnt[r]) {
      rc = rt_pack_owned_device(g->ctx[r], &pr, g->accum[r].get(), g->packed[r].get(), s);
      if (rc != RT_OK) return rc;
      HIP_TRY(hipEventRecord(g->packed_ready[r].get(), s));
    }
  }
  // 2. owned granules travel to rank 0's device: 1/N of the frame per rank, nothing else.  Device 0
  // receives and scatters them on its EXCHANGE stream, beside its own render on stream[0] (the
  // pixels are disjoint), so a rank that finishes early is assembled while the others still render.
  if (g->rccl) {
    ncclResult_t nr = g_rccl.GroupStart();
    for (uint32_t r = 1; r < n && nr == ncclSuccess; ++r) {
      if (!cnt[r]) continue;
      const size_t floats = (size_t)cnt[r] * 64 * 4;
      nr = g_rccl.Send(g->packed[r].get(), floats, ncclFloat, 0, g->comm[r], g->stream[r].get());
      if (nr == ncclSuccess) nr = g_rccl.Recv(g->recv[r].get(), floats, ncclFloat, static_cast<int>(r), g->comm[0], g->xstream.get());
    }
    const ncclResult_t ne = g_rccl.GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return fail(RT_ERR_HIP, "RCCL exchange failed: %s", g_rccl.GetErrorString(nr));
  } else {
    HIP_TRY(hipSetDevice(g->dev[0]));
    for (uint32_t r = 1; r < n; ++r) {
      if (!cnt[r]) continue;
      HIP_TRY(hipStreamWaitEvent(g->xstream.get(), g->packed_ready[r].get(), 0));
      HIP_TRY(hipMemcpyPeerAsync(g->recv[r].get(), g->dev[0], g->packed[r].get(), g->dev[r], (size_t)cnt[r] * 64 * sizeof(float4),
                                 g->xstream.get()));
    }
  }
  // 3. rank 0 scatters them into its frame, resolves (Renderer.cpp:262-265) and hands the image back
  HIP_TRY(hipSetDevice(g->dev[0]));
  for (uint32_t r = 1; r < n; ++r) {
    if (!cnt[r]) continue;
    rc = rt_unpack_owned_device(g->ctx[0], &base, r, g->recv[r].get(), g->accum[0].get(), g->xstream.get());
    if (rc != RT_OK) return rc;
  }
  hipStream_t s0 = g->stream[0].get();
  HIP_TRY(hipEventRecord(g->assembled.get(), g->xstream.get()));
  HIP_TRY(hipStreamWaitEvent(s0, g->assembled.get(), 0));
  hipError_t he = hipSuccess;
  if (out_rgb) {
    he = hipMemcpyAsync(g->dBg.get(), bg, npx * 3 * sizeof(float), hipMemcpyHostToDevice, s0);
    if (he == hipSuccess) rc = rt_resolve_device(g->ctx[0], p->width, p->height, p->spp, g->accum[0].get(), g->dBg.get(), g->dOut.get(), s0);
    if (rc != RT_OK) return rc;
    if (he == hipSuccess) he = hipMemcpyAsync(out_rgb, g->dOut.get(), npx * 3 * sizeof(float), hipMemcpyDeviceToHost, s0);
  }
  if (he == hipSuccess && accum_out) he = hipMemcpyAsync(accum_out, g->accum[0].get(), npx * sizeof(float4), hipMemcpyDeviceToHost, s0);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "frame read-back failed: %s", hipGetErrorString(he));
  for (uint32_t r = 0; r < n; ++r) {
    HIP_TRY(hipSetDevice(g->dev[r]));
    HIP_TRY(hipStreamSynchronize(g->stream[r].get()));
  }
  HIP_TRY(hipSetDevice(g->dev[0]));
  HIP_TRY(hipStreamSynchronize(g->xstream.get()));
  if (stats) {
    *stats = rt_stats{};
    for (uint32_t r = 0; r < n; ++r) {
      HIP_TRY(hipSetDevice(g->dev[r]));
      rt_stats s;
      rc = read_counters(g->ctx[r], &s);
      if (rc != RT_OK) return rc;
      float ms = 0.f;
      HIP_TRY(event_pair_ms(g->ctx[r], ev[r], &ms));
      stats->rays_closest += s.rays_closest, stats->rays_shadow += s.rays_shadow, stats->knn_queries += s.knn_queries;
      stats->nodes_visited += s.nodes_visited, stats->tris_tested += s.tris_tested, stats->kd_visited += s.kd_visited;
      stats->kernel_ms = ms > stats->kernel_ms ? ms : stats->kernel_ms;  // the slowest rank
    }
    stats->samples = (uint64_t)npx * sample_range(*p).count;
  }
  return RT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- rt_update: a resident scene follows its description
namespace {

// rt_bvh_quality_get's reduction over the context's float nodes, queued on `stream`: the pair {inner-slot sum, leaf-slot
// sum} lands in c->dQuality at kQualityNow (the tree as it is) or kQualityBuilt (the baseline rt_update takes before its
// first refit).  A host-built or tuned tree's float nodes go to the device first, as for a refit, and stay.
constexpr size_t kQualityNow = 2 * (size_t)rtk::kQualityPartials, kQualityBuilt = kQualityNow + 2;
int queue_quality(rt_ctx* c, size_t slot, hipStream_t stream) {
  int rc = RT_OK;
  if (!c->nodesF && (rc = upload(&c->nodesF, c->bvh.nodes.data(), c->bvh.nodes.size() * 4)) != RT_OK) return rc;
  if (!c->dQuality) HIP_TRY(dev_alloc(&c->dQuality, kQualityBuilt + 2));
  HIP_TRY(rtk::gpu_bvh_quality(c->nodesF.get(), c->S.n_nodes, c->dQuality.get(), c->dQuality.get() + slot, stream));
  return RT_OK;
}
// cost = nodes + 1.5 tris of a pair read back from c->dQuality (the stream that wrote it has been synchronised)
int read_quality(rt_ctx* c, size_t slot, rt_bvh_quality* q) {
  double h[2];
  HIP_TRY(hipMemcpy(h, c->dQuality.get() + slot, sizeof h, hipMemcpyDeviceToHost));
  q->nodes = 1.0 + h[0], q->tris = h[1];
  q->cost = q->nodes + 1.5 * q->tris;
  return RT_OK;
}
// the whole call, after the argument checks: one launch bracketed by an event pair like a frame's, then the baseline rule
int tree_quality(rt_ctx* c, rt_bvh_quality* q) {
  rt_bvh_quality r{};
  const int e = c->evUsed % kEventPairs;
  HIP_TRY(hipEventRecord(c->ev[e][0].get(), nullptr));
  int rc = queue_quality(c, kQualityNow, nullptr);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipEventRecord(c->ev[e][1].get(), nullptr));
  c->evUsed++;
  HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = read_quality(c, kQualityNow, &r)) != RT_OK) return rc;
  // (no refit since the build: the tree as it is IS the tree as built)
  if (!c->costBuiltValid && c->refits == 0) c->costBuilt = r.cost, c->costBuiltValid = true;
  r.cost_built = c->costBuilt;
  r.ratio = r.cost / r.cost_built;
  r.n_nodes = c->S.n_nodes, r.refits = c->refits;
  *q = r;
  return RT_OK;
}

// what an update changes; positions / normals already on the device (the caller's arrays or the context's scratch)
struct Update {
  const float* dPos = nullptr;
  const float* dNrm = nullptr;
  const rt_camera* camera = nullptr;
  const rt_light* lights = nullptr;
  uint32_t nLights = 0;
  const rt_material* materials = nullptr;
  const rtbvh::Padding* padding = nullptr;  // rt_render_views: its farthest view's padding in place of the camera's rule
  // rt_update_transforms: dPos / dNrm come from the rest pose (which stays), their summary is already on its way into
  // c->dMag on the stream, and the positions the update replaces go to dPrevPos first
  bool fromRest = false, magQueued = false;
  void* dPrevPos = nullptr;
};

int update_checks(rt_ctx* c, const rt_light* lights, uint32_t nLights) {
  if (!lights && nLights) return fail(RT_ERR_INVALID, "update: lights is null but n_lights is %u", nLights);
  if (c->nodeFormat == RT_NODES_Q8) return fail(RT_ERR_UNSUPPORTED, "update: RT_NODES_Q8 contexts cannot be refit (create the context again)");
  if (c->broken) return fail(RT_ERR_STATE, "the context is in an unknown state (a failed rt_bvh_tune or rt_update): destroy it");
  return RT_OK;
}

// The rules rt_create applies, on the updated description: validation and every derived value first (nothing visible
// changes), then the arrays, the refit and the derived state.  `stream` orders the work on the caller's arrays.
int update_ctx(rt_ctx* c, const Update& u, hipStream_t stream, std::chrono::steady_clock::time_point t0, rt_update_report* rep) {
  rtk::DevScene& S = c->S;
  rt_update_report r{};
  // 1. the magnitude summaries of the new arrays (the finiteness check, the padding rule, vouch_short_forms)
  uint32_t magRef = c->magRef, magPos = c->magPos, magNrm = c->magNrm;
  if (u.dPos || u.dNrm) {
    if (!c->dMag) HIP_TRY(dev_alloc(&c->dMag, 3));
    uint32_t h[3] = {0, 0, 0};
    hipError_t he = u.magQueued ? hipSuccess : rtk::launch_magnitudes(u.dPos, u.dNrm, c->triShade.get(), S.n_tris, c->nVertices, c->dMag.get(), stream);
    if (he == hipSuccess) he = hipMemcpyAsync(h, c->dMag.get(), sizeof h, hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return fail(RT_ERR_HIP, "update: magnitude pass failed: %s", hipGetErrorString(he));
    if (u.dPos) magRef = h[0], magPos = h[1];
    if (u.dNrm) magNrm = h[2];
    if (magRef >= 0x7f800000u) return fail(RT_ERR_INVALID, "update rejected: non-finite vertex position");
  }
  const rt_camera cam = u.camera ? *u.camera : S.cam;
  const std::vector<rt_light> lights = u.lights ? std::vector<rt_light>(u.lights, u.lights + u.nLights) : c->hostLights;
  const rtbvh::Padding P = u.padding ? *u.padding : rtbvh::paddingRule(bits_float(magRef), cam, lights.data(), (uint32_t)lights.size());
  const bool refit = u.dPos || P.pad != c->bvh.pad || P.boxScale != c->bvh.boxScale;
  // 2. staging: new light and material arrays, the refit's float nodes and depth table (the context still renders as before)
  int rc = RT_OK;
  DevBuf<rt_light> dLights;
  DevBuf<rt_material> dMats;
  DevBuf<rtd::DevMat> dMatsDev;
  if (u.lights && (rc = upload(&dLights, lights.data(), lights.size())) != RT_OK) return rc;
  if (u.materials) {
    std::vector<rtd::DevMat> dm(c->nMeshes);
    for (uint32_t m = 0; m < c->nMeshes; ++m) dm[m] = rtd::make_dev_mat(u.materials[m]);
    if ((rc = upload(&dMats, u.materials, c->nMeshes)) != RT_OK || (rc = upload(&dMatsDev, dm.data(), dm.size())) != RT_OK) return rc;
  }
  Event e0, e1;
  if (refit) {
    // (a host-built tree's float nodes go to the device on the first refit and stay; rt_bvh_tune drops them)
    if (!c->nodesF && (rc = upload(&c->nodesF, c->bvh.nodes.data(), c->bvh.nodes.size() * 4)) != RT_OK) return rc;
    if (!c->refitDepth) {
      HIP_TRY(dev_alloc(&c->refitDepth, S.n_nodes));
      const hipError_t he = rtk::gpu_bvh_depths(c->nodesF.get(), S.n_nodes, c->refitDepth.get(), &c->refitMaxDepth, stream);
      if (he != hipSuccess) {
        c->refitDepth.reset();
        return fail(RT_ERR_HIP, "update: node depths failed: %s", hipGetErrorString(he));
      }
    }
    HIP_TRY(make_event(&e0));
    HIP_TRY(make_event(&e1));
    // (the first refit after a build: the cost of the tree as built, rt_bvh_quality's baseline, while its boxes still stand)
    if (!c->costBuiltValid && (rc = queue_quality(c, kQualityBuilt, stream)) != RT_OK) return rc;
  }
  const bool baseline = refit && !c->costBuiltValid;
  // 3. the context changes: a failure from here on leaves it refusing launches
  c->broken = true;
  const size_t nv = 3 * (size_t)c->nVertices;
  hipError_t he = hipSuccess;
  if (u.dPrevPos) he = hipMemcpyAsync(u.dPrevPos, c->vpos.get(), nv * sizeof(float), hipMemcpyDeviceToDevice, stream);
  if (he == hipSuccess && u.dPos && u.dPos != c->vpos.get()) he = hipMemcpyAsync(c->vpos.get(), u.dPos, nv * sizeof(float), hipMemcpyDeviceToDevice, stream);
  if (he == hipSuccess && u.dNrm && u.dNrm != c->vnrm.get())
    he = hipMemcpyAsync(c->vnrm.get(), u.dNrm, nv * sizeof(float), hipMemcpyDeviceToDevice, stream);
  if (refit) {
    if (he == hipSuccess) he = hipEventRecord(e0.get(), stream);
    if (he == hipSuccess)
      he = rtk::gpu_bvh_refit(c->vpos.get(), c->triShade.get(), S.n_tris, u.dPos != nullptr, c->tris.get(), c->trisRef.get(), c->nodesF.get(),
                              c->nodes.get(), S.n_nodes, c->refitDepth.get(), c->refitMaxDepth, P.pad, P.boxScale, stream);
    if (he == hipSuccess) he = hipEventRecord(e1.get(), stream);
  }
  if (he == hipSuccess) he = hipStreamSynchronize(stream);
  if (he == hipSuccess && refit) {
    float ms = 0.f;
    he = hipEventElapsedTime(&ms, e0.get(), e1.get());
    r.refit_ms = ms;
  }
  // a host-built tree's host copy (rt_bvh_export, rt_bvh_tune) follows
  if (he == hipSuccess && refit && c->builder == RT_BVH_HOST) {
    rtbvh::Built& b = c->bvh;
    he = hipMemcpy(b.nodes.data(), c->nodesF.get(), b.nodes.size() * sizeof(rtbvh::Node), hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(b.nodes16.data(), c->nodes.get(), b.nodes16.size() * sizeof(rtbvh::Node16), hipMemcpyDeviceToHost);
    if (he == hipSuccess && u.dPos) he = hipMemcpy(b.tris.data(), c->tris.get(), b.tris.size() * sizeof(rtbvh::TriRec), hipMemcpyDeviceToHost);
    if (he == hipSuccess && u.dPos) he = hipMemcpy(b.trisRef.data(), c->trisRef.get(), b.trisRef.size() * sizeof(rtbvh::TriRec), hipMemcpyDeviceToHost);
  }
  if (he != hipSuccess) return fail(RT_ERR_HIP, "update failed after the context had started to change (%s): it refuses launches", hipGetErrorString(he));
  if (baseline) {
    rt_bvh_quality built{};
    if ((rc = read_quality(c, kQualityBuilt, &built)) != RT_OK) return rc;
    c->costBuilt = built.cost, c->costBuiltValid = true;
  }
  if (refit) c->refits++;
  c->bvh.maxAbs = bits_float(magRef), c->bvh.pad = P.pad, c->bvh.originBound = P.originBound, c->bvh.boxScale = P.boxScale;
  S.invBoxScale = 1.f / P.boxScale, S.originBound = P.originBound;
  c->magRef = magRef, c->magPos = magPos, c->magNrm = magNrm;
  S.cam = cam;
  if (u.lights) {
    c->lights = std::move(dLights), c->hostLights = lights;
    S.lights = c->lights.get(), S.n_lights = (uint32_t)lights.size();
  }
  if (u.materials) {
    c->mats = std::move(dMats), c->matsDev = std::move(dMatsDev);
    S.mats = c->mats.get(), S.matsDev = c->matsDev.get();
  }
  vouch_short_forms(c);
  if ((u.dPos || u.dNrm) && !u.fromRest) c->restValid = false;  // the live arrays are the new rest pose of rt_update_transforms
  // the photon map was emitted from the old geometry, normals, lights and materials
  if (u.dPos || u.dNrm || u.lights || u.materials) {
    r.photons_dropped = S.n_photons > 0 ? 1u : 0u;
    if ((rc = drop_photons(c)) != RT_OK) return rc;
  }
  c->broken = false;
  r.refitted = refit ? 1u : 0u;
  r.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rep) *rep = r;
  return RT_OK;
}

// rt_update_transforms and rt_update_skin, before their kernel: the rest pose — a copy of the live arrays, taken on `stream`
// when none is valid —, the scratch of rt_update's host form that the result goes to, and the magnitude block.  Nothing
// here is visible until update_ctx's own validation has passed.
int prepare_rest_pose(rt_ctx* c, hipStream_t stream) {
  const size_t nv = 3 * (size_t)c->nVertices;
  if (!c->restPos) HIP_TRY(dev_alloc(&c->restPos, nv));
  if (!c->restNrm) HIP_TRY(dev_alloc(&c->restNrm, nv));
  if (!c->updPos) HIP_TRY(dev_alloc(&c->updPos, nv));
  if (!c->updNrm) HIP_TRY(dev_alloc(&c->updNrm, nv));
  if (!c->dMag) HIP_TRY(dev_alloc(&c->dMag, 3));
  if (!c->restValid) {
    HIP_TRY(hipMemcpyAsync(c->restPos.get(), c->vpos.get(), nv * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c->restNrm.get(), c->vnrm.get(), nv * sizeof(float), hipMemcpyDeviceToDevice, stream));
    c->restValid = true;
  }
  return RT_OK;
}
// ... and after it: the posed arrays wait in the scratch and their summary is on its way into c->dMag
int update_from_rest(rt_ctx* c, const rt_camera* camera, const rt_light* lights, uint32_t nLights, void* dPrevPos, hipStream_t stream,
                     std::chrono::steady_clock::time_point t0, rt_update_report* rep) {
  Update x;
  x.dPos = c->updPos.get(), x.dNrm = c->updNrm.get();
  x.camera = camera, x.lights = lights, x.nLights = nLights;
  x.fromRest = x.magQueued = true, x.dPrevPos = dPrevPos;
  return update_ctx(c, x, stream, t0, rep);
}
// the entries of a record that its call reads, all finite
bool finite_record(const rt_mesh_transform& t) {
  bool finite = true;
  for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(t.m[i / 4][i % 4]);
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(t.n[i / 3][i % 3]);
  return finite;
}

}  // namespace

extern "C" {

int rt_update(rt_ctx* c, const rt_scene_update* u, rt_update_report* rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (rep) memset(rep, 0, sizeof *rep);
  if (!c || !u) return fail(RT_ERR_INVALID, "ctx/update is null");
  int rc = update_checks(c, u->lights, u->n_lights);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  // the host form: the arrays go to the context's scratch, then the device form runs on them
  const size_t nv = 3 * (size_t)c->nVertices;
  Update x;
  if (u->vertex_pos) {
    if (!c->updPos) HIP_TRY(dev_alloc(&c->updPos, nv));
    HIP_TRY(hipMemcpy(c->updPos.get(), u->vertex_pos, nv * sizeof(float), hipMemcpyHostToDevice));
    x.dPos = c->updPos.get();
  }
  if (u->vertex_nrm) {
    if (!c->updNrm) HIP_TRY(dev_alloc(&c->updNrm, nv));
    HIP_TRY(hipMemcpy(c->updNrm.get(), u->vertex_nrm, nv * sizeof(float), hipMemcpyHostToDevice));
    x.dNrm = c->updNrm.get();
  }
  x.camera = u->camera, x.lights = u->lights, x.nLights = u->n_lights, x.materials = u->materials;
  return update_ctx(c, x, nullptr, t0, rep);
}

int rt_update_vertices_device(rt_ctx* c, const void* d_pos, const void* d_nrm, void* stream, rt_update_report* rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (rep) memset(rep, 0, sizeof *rep);
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  int rc = update_checks(c, nullptr, 0);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  Update x;
  x.dPos = static_cast<const float*>(d_pos), x.dNrm = static_cast<const float*>(d_nrm);
  return update_ctx(c, x, static_cast<hipStream_t>(stream), t0, rep);
}

int rt_update_transforms(rt_ctx* c, const rt_transform_update* u, void* stream_, rt_update_report* rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (rep) memset(rep, 0, sizeof *rep);
  // what the update says of itself comes before anything of the context
  if (!u) return fail(RT_ERR_INVALID, "ctx/update is null");
  if (!u->transforms) return fail(RT_ERR_INVALID, "update: transforms is null");
  for (uint32_t r : u->reserved)
    if (r) return fail(RT_ERR_INVALID, "update: reserved words must be zero");
  for (uint32_t j = 0; j < u->n_meshes; ++j) {
    const rt_mesh_transform& t = u->transforms[j];
    if (t.flags & ~(uint32_t)RT_XF_STATIC) return fail(RT_ERR_INVALID, "update: mesh %u: unknown transform flags 0x%x", j, t.flags);
    if (t.flags & RT_XF_STATIC) continue;
    if (!finite_record(t)) return fail(RT_ERR_INVALID, "update: mesh %u: non-finite entry in its transform", j);
  }
  if (!u->lights && u->n_lights) return fail(RT_ERR_INVALID, "update: lights is null but n_lights is %u", u->n_lights);
  if (!c) return fail(RT_ERR_INVALID, "ctx/update is null");
  if (u->n_meshes != c->nMeshes) return fail(RT_ERR_INVALID, "update: %u transforms for a context of %u meshes", u->n_meshes, c->nMeshes);
  int rc = update_checks(c, u->lights, u->n_lights);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if ((rc = prepare_rest_pose(c, stream)) != RT_OK) return rc;
  if (!c->xfTable) HIP_TRY(dev_alloc(&c->xfTable, c->nMeshes));
  HIP_TRY(hipMemcpyAsync(c->xfTable.get(), u->transforms, c->nMeshes * sizeof(rt_mesh_transform), hipMemcpyHostToDevice, stream));
  HIP_TRY(rtk::launch_transform(c->restPos.get(), c->restNrm.get(), c->xfTable.get(), c->meshVtxBegin.get(), c->nMeshes, c->nVertices,
                                c->updPos.get(), c->updNrm.get(), c->triShade.get(), c->S.n_tris, c->dMag.get(), stream));
  return update_from_rest(c, u->camera, u->lights, u->n_lights, u->d_prev_pos, stream, t0, rep);
}

int rt_set_skin(rt_ctx* c, const rt_skin* s) {
  if (!s) {
    if (!c) return fail(RT_ERR_INVALID, "ctx/skin is null");
    HIP_TRY(hipSetDevice(c->device));
    c->skinBone.reset(), c->skinWeight.reset(), c->skinTable.reset();
    c->skinBones = 0;
    return RT_OK;
  }
  // what the skin says of itself comes before anything of the context
  if (!s->bone || !s->weight) return fail(RT_ERR_INVALID, "skin: bone/weight is null");
  for (uint32_t r : s->reserved)
    if (r) return fail(RT_ERR_INVALID, "skin: reserved words must be zero");
  if (s->n_bones < 1 || s->n_bones > 65536) return fail(RT_ERR_INVALID, "skin: n_bones is %u, outside 1..65536", s->n_bones);
  for (uint32_t v = 0; v < s->n_vertices; ++v) {
    const size_t at = RT_SKIN_INFLUENCES * (size_t)v;
    for (uint32_t k = 0; k < RT_SKIN_INFLUENCES; ++k)
      if (!std::isfinite(s->weight[at + k])) return fail(RT_ERR_INVALID, "skin: vertex %u: non-finite weight", v);
    for (uint32_t k = 0; k < RT_SKIN_INFLUENCES; ++k)
      if (s->bone[at + k] >= s->n_bones)
        return fail(RT_ERR_INVALID, "skin: vertex %u slot %u: bone index %u of %u bones", v, k, (uint32_t)s->bone[at + k], s->n_bones);
  }
  if (!c) return fail(RT_ERR_INVALID, "ctx/skin is null");
  if (s->n_vertices != c->nVertices) return fail(RT_ERR_INVALID, "skin: %u vertices for a context of %u", s->n_vertices, c->nVertices);
  int rc = update_checks(c, nullptr, 0);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  // the new skin replaces the old one only when all of it is resident
  DevBuf<uint16_t> bone;
  DevBuf<float> weight;
  DevBuf<rt_mesh_transform> table;
  const size_t n = RT_SKIN_INFLUENCES * (size_t)c->nVertices;
  if ((rc = upload(&bone, s->bone, n)) != RT_OK || (rc = upload(&weight, s->weight, n)) != RT_OK) return rc;
  HIP_TRY(dev_alloc(&table, s->n_bones));
  c->skinBone = std::move(bone), c->skinWeight = std::move(weight), c->skinTable = std::move(table);
  c->skinBones = s->n_bones;
  return RT_OK;
}

int rt_update_skin(rt_ctx* c, const rt_skin_update* u, void* stream_, rt_update_report* rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (rep) memset(rep, 0, sizeof *rep);
  // what the update says of itself comes before anything of the context
  if (!u) return fail(RT_ERR_INVALID, "ctx/update is null");
  if (!u->bones) return fail(RT_ERR_INVALID, "update: bones is null");
  for (uint32_t r : u->reserved)
    if (r) return fail(RT_ERR_INVALID, "update: reserved words must be zero");
  for (uint32_t j = 0; j < u->n_bones; ++j) {
    const rt_mesh_transform& t = u->bones[j];
    if (t.flags) return fail(RT_ERR_INVALID, "update: bone %u: flags must be zero (0x%x)", j, t.flags);
    if (!finite_record(t)) return fail(RT_ERR_INVALID, "update: bone %u: non-finite entry in its transform", j);
  }
  if (!u->lights && u->n_lights) return fail(RT_ERR_INVALID, "update: lights is null but n_lights is %u", u->n_lights);
  if (!c) return fail(RT_ERR_INVALID, "ctx/update is null");
  if (!c->skinBones) return fail(RT_ERR_STATE, "update: the context has no resident skin (rt_set_skin)");
  if (u->n_bones != c->skinBones) return fail(RT_ERR_INVALID, "update: %u bones for a skin of %u bones", u->n_bones, c->skinBones);
  int rc = update_checks(c, u->lights, u->n_lights);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if ((rc = prepare_rest_pose(c, stream)) != RT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->skinTable.get(), u->bones, c->skinBones * sizeof(rt_mesh_transform), hipMemcpyHostToDevice, stream));
  HIP_TRY(rtk::launch_skin(c->restPos.get(), c->restNrm.get(), c->skinBone.get(), c->skinWeight.get(), c->skinTable.get(), c->nVertices,
                           c->updPos.get(), c->updNrm.get(), c->triShade.get(), c->S.n_tris, c->dMag.get(), stream));
  return update_from_rest(c, u->camera, u->lights, u->n_lights, u->d_prev_pos, stream, t0, rep);
}

int rt_group_update(rt_group* g, const rt_scene_update* u, rt_update_report* rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (rep) memset(rep, 0, sizeof *rep);
  if (!g || !u) return fail(RT_ERR_INVALID, "group/update is null");
  rt_update_report first{};
  for (size_t r = 0; r < g->ctx.size(); ++r) {
    rt_update_report mine{};
    const int rc = rt_update(g->ctx[r], u, r == 0 ? &first : &mine);
    if (rc != RT_OK) return rc;
  }
  (void)hipSetDevice(g->dev[0]);
  first.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rep) *rep = first;
  return RT_OK;
}

}  // extern "C"

// ---- rt_bvh_quality_get / rt_rebuild: a refit tree measured, and built again in place ---------------------------------
extern "C" {

int rt_bvh_quality_get(rt_ctx* c, rt_bvh_quality* out) {
  if (!c || !out) return fail(RT_ERR_INVALID, "quality: ctx/out is null");
  memset(out, 0, sizeof *out);
  if (c->nodeFormat == RT_NODES_Q8) return fail(RT_ERR_UNSUPPORTED, "quality: RT_NODES_Q8 contexts keep no float nodes to measure");
  if (c->broken) return fail(RT_ERR_STATE, "the context is in an unknown state (a failed rt_bvh_tune or rt_update): destroy it");
  HIP_TRY(hipSetDevice(c->device));
  return tree_quality(c, out);
}

int rt_rebuild(rt_ctx* c, const rt_rebuild_params* p, rt_rebuild_report* rep) {
  const auto t0 = std::chrono::steady_clock::now();
  auto msSince = [&t0] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  if (rep) memset(rep, 0, sizeof *rep);
  // what the parameters say of themselves comes before anything of the context
  if (p) {
    for (uint32_t r : p->reserved)
      if (r) return fail(RT_ERR_INVALID, "rebuild: reserved words must be zero");
    if (p->min_ratio != 0.f && !(std::isfinite(p->min_ratio) && p->min_ratio >= 1.f))
      return fail(RT_ERR_INVALID, "rebuild: min_ratio must be 0 or finite and >= 1");
  }
  if (!c) return fail(RT_ERR_INVALID, "rebuild: ctx is null");
  if (c->nodeFormat == RT_NODES_Q8) return fail(RT_ERR_UNSUPPORTED, "rebuild: RT_NODES_Q8 contexts cannot be rebuilt (create the context again)");
  if (c->broken) return fail(RT_ERR_STATE, "the context is in an unknown state (a failed rt_bvh_tune or rt_update): destroy it");
  HIP_TRY(hipSetDevice(c->device));
  rt_rebuild_report r{};
  const float minRatio = p ? p->min_ratio : 0.f;
  int rc = RT_OK;
  if (minRatio > 0.f || rep) {
    rt_bvh_quality q;
    if ((rc = tree_quality(c, &q)) != RT_OK) return rc;
    r.ratio_before = q.ratio;
    if (minRatio > 0.f && !(q.ratio >= (double)minRatio)) {
      r.total_ms = msSince();
      if (rep) *rep = r;
      return RT_OK;
    }
  }
  // the description the host passes read: positions, vertex ids and mesh tables come back for the duration of the call (the
  // builders read neither normals nor materials); the lights and the camera are the context's
  const rtk::DevScene& S = c->S;
  const double tRead0 = msSince();
  std::vector<float> pos(3 * (size_t)c->nVertices);
  std::vector<uint32_t> triVtx, meshTriBegin(c->nMeshes + 1u), meshVtxBegin(c->nMeshes + 1u);
  {
    std::vector<uint4> shade(S.n_tris);
    HIP_TRY(hipMemcpy(shade.data(), c->triShade.get(), shade.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pos.data(), c->vpos.get(), pos.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(meshTriBegin.data(), c->meshTriBegin.get(), meshTriBegin.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(meshVtxBegin.data(), c->meshVtxBegin.get(), meshVtxBegin.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    rtbvh::triVtxFromShade(reinterpret_cast<const uint32_t*>(shade.data()), S.n_tris, triVtx);
  }
  const rt_scene_desc sc = rtbvh::residentDesc(c->nMeshes, c->nVertices, S.n_tris, pos.data(), triVtx.data(), meshTriBegin.data(),
                                               meshVtxBegin.data(), c->hostLights.data(), (uint32_t)c->hostLights.size(), S.cam);
  r.readback_ms = msSince() - tRead0;
  // the new tree, beside the one the context renders with; a failure up to here leaves the context as it was
  Tree tree;
  rc = build_tree(&sc, c->optLeafMax, c->optBuilder, c->optNodeFormat, nullptr, [&](const float** dVpos, const uint4** dTriShade) {
    *dVpos = c->vpos.get(), *dTriShade = c->triShade.get();
    return (int)RT_OK;
  }, &tree);
  if (rc != RT_OK) return rc;
  if (tree.nodeFormat != RT_NODES_F16) return fail(RT_ERR_UNSUPPORTED, "rebuild: the build produced RT_NODES_Q8 records (RT_NODES changed since rt_create)");
  HIP_TRY(hipDeviceSynchronize());
  r.build_ms = tree.buildMs, r.plan_ms = tree.planMs;
  // the swap: moves only, then the values derived from the tree by rt_create's rules
  install_tree(c, &tree);
  vouch_short_forms(c);
  r.rebuilt = 1u, r.builder = c->builder;
  if (rep) {
    // (from here on a failure is a failed quality call on a whole context)
    rt_bvh_quality q;
    if ((rc = tree_quality(c, &q)) != RT_OK) return rc;
    r.cost_after = q.cost;
    r.total_ms = msSince();
    *rep = r;
  }
  return RT_OK;
}

}  // extern "C"

// ---- first-hit AOVs and the a-trous denoiser -------------------------------------------------------------------------
namespace {

// the defaults of rt_denoise_params (rt_amd.h, DESIGN.md "AOVs and the a-trous denoiser": chosen on C1 / C2 frames)
constexpr uint32_t kDenoiseIterations = 5;
constexpr float kDenoiseSigmaColor = 2.f, kDenoiseSigmaNormal = 0.5f;

// checks the three filters share (the texts are part of what the callers see)
int check_image_size(uint32_t w, uint32_t h) {
  return w == 0 || h == 0 || w > 65535u || h > 65535u ? fail(RT_ERR_INVALID, "image size %ux%u out of range", w, h) : RT_OK;
}
int check_sigmas(std::initializer_list<float> sigmas) {
  for (float s : sigmas)
    if (!(s >= 0.f) || !std::isfinite(s)) return fail(RT_ERR_INVALID, "sigmas must be finite and >= 0");
  return RT_OK;
}
int check_aov_channels(const rt_aov* aov, const char* who) {
  return aov->albedo && aov->normal && aov->position && aov->hits
             ? RT_OK
             : fail(RT_ERR_INVALID, "the %s needs the albedo, normal, position and hits channels", who);
}
int check_motion_channels(const rt_motion* cur) {
  return cur->motion && cur->prev_position && cur->mesh
             ? RT_OK
             : fail(RT_ERR_INVALID, "the current frame needs the motion, prev_position and mesh channels");
}
int check_not_broken(const rt_ctx* c) {
  return c->broken ? fail(RT_ERR_STATE, "the context's device tree is in an unknown state: destroy it") : RT_OK;
}

// (a context exists only where a device does: the entry points that take a handle unchecked up to here ask this first)
int check_device_present() {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(RT_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  return RT_OK;
}

// Everything rt_denoise and rt_denoise_device check before they look at the context.
int denoise_checks(const rt_ctx* c, const rt_denoise_params* d, const void* rgb, const rt_aov* aov, const void* out) {
  if (!c || !d || !rgb || !aov || !out) return fail(RT_ERR_INVALID, "null argument");
  return check_aov_channels(aov, "denoiser");
}

// ... and what they check in d's numbers (both after their own earlier checks: the header gives each form's order)
int denoise_param_checks(const rt_denoise_params* d) {
  int rc = check_image_size(d->width, d->height);
  if (rc != RT_OK) return rc;
  if (d->iterations > 8) return fail(RT_ERR_INVALID, "iterations %u > 8", d->iterations);
  return check_sigmas({d->sigma_color, d->sigma_normal, d->sigma_position});
}

// c->dnScratch with room for `need` float4 (rt_denoise_device and rt_svgf_device: one call at a time)
int ensure_filter_scratch(rt_ctx* c, size_t need) {
  return grow(&c->dnScratch, &c->dnCap, need);
}

// rt_render_aov's own view of p: the fields that do not affect the pass are neutralised before rt_render's checks
rt_params aov_params(const rt_params& p) {
  rt_params q = p;
  q.mode = RT_MODE_RAY, q.max_depth = 1, q.use_photons = 0, q.k = 0, q.photons_requested = 0;
  return q;
}
int aov_checks(const rt_ctx* c, const rt_params* p, rt_params* q) {
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  if (!p) return fail(RT_ERR_INVALID, "params is null");
  *q = aov_params(*p);
  int rc = check_params(c, q);
  if (rc != RT_OK) return rc;
  if (q->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded AOVs (world %u) are not supported", q->world);
  return RT_OK;
}

// The denoiser's arguments (one frame or a stack of them) with d's defaults applied; the scratch is the context's
rtk::DenoiseArgs denoise_args(const rt_ctx* c, const rt_denoise_params* d, const void* d_rgb, const rt_aov* aov, void* d_out) {
  rtk::DenoiseArgs D;
  D.width = d->width, D.height = d->height;
  D.iterations = d->iterations ? d->iterations : kDenoiseIterations;
  D.sigma_color = d->sigma_color > 0.f ? d->sigma_color : kDenoiseSigmaColor;
  D.sigma_normal = d->sigma_normal > 0.f ? d->sigma_normal : kDenoiseSigmaNormal;
  D.sigma_position = d->sigma_position;  // 0: the device derives it from the scene's extent (once for a stack)
  D.rgb = static_cast<const float*>(d_rgb), D.albedo = aov->albedo, D.normal = aov->normal, D.position = aov->position;
  D.hits = aov->hits, D.out = static_cast<float*>(d_out), D.scratch = c->dnScratch.get();
  return D;
}

rtk::AovArgs aov_args(const rt_params& q, const rt_aov& out) {
  rtk::AovArgs A;
  A.albedo = out.albedo, A.normal = out.normal, A.position = out.position, A.depth = out.depth;
  A.hits = out.hits, A.mesh = out.mesh, A.tri = out.tri;
  A.width = q.width, A.height = q.height, A.spp = q.spp, A.seed = q.seed;
  A.s0 = sample_range(q).s0, A.s1 = sample_range(q).s1;
  return A;
}

// What the vertices of a frame shade with, or the albedo channel of an AOV pass sums, in place of the meshes' own: the
// record its kernels take, built from the context's resident data, and the FrameGen that names it (gen points into this
// object, which its owner keeps alive over the launch call).
struct SurfaceGen {
  rtk::VColRec vcol{};
  rtk::TexRec tex{};
  rtk::MatRec mat{};
  rtk::NrmRec nrm{};
  FrameGen gen;
  SurfaceGen() = default;
  SurfaceGen(const SurfaceGen&) = delete;
  SurfaceGen& operator=(const SurfaceGen&) = delete;
};
// (of a checked `albedo` argument of the *_albedo forms)
inline FrameGen::Surface albedo_surface(uint32_t albedo) {
  return albedo == RT_ALBEDO_COLORS ? FrameGen::VCOL : albedo == RT_ALBEDO_TEXTURES ? FrameGen::TEX : FrameGen::NONE;
}
// G for surface `kind`, or RT_ERR_STATE where the context lacks what it reads: the colours; the textures, then the maps,
// then maps that were set for these textures (NMAP: the normal maps, then material maps if any are resident — without
// them the frame reads noMaps, RT_TEX_NONE on every mesh, for both material tables)
int resident_surface(const rt_ctx* c, FrameGen::Surface kind, SurfaceGen* G) {
  if (kind == FrameGen::VCOL && !c->vcol) return fail(RT_ERR_STATE, "the context has no resident vertex colours (rt_set_vertex_colors)");
  if ((kind == FrameGen::TEX || kind == FrameGen::MAT || kind == FrameGen::NMAP) && !c->tex) return fail(RT_ERR_STATE, "the context has no resident textures (rt_set_textures)");
  if (kind == FrameGen::MAT && !c->matMaps) return fail(RT_ERR_STATE, "the context has no resident material maps (rt_set_material_maps)");
  if (kind == FrameGen::MAT && c->matMaps.texGeneration != c->tex.generation)
    return fail(RT_ERR_STATE, "the material maps were set for another texture set (rt_set_material_maps after rt_set_textures)");
  if (kind == FrameGen::NMAP && !c->nrmMaps) return fail(RT_ERR_STATE, "the context has no resident normal maps (rt_set_normal_maps)");
  if (kind == FrameGen::NMAP && c->nrmMaps.texGeneration != c->tex.generation)
    return fail(RT_ERR_STATE, "the normal maps were set for another texture set (rt_set_normal_maps after rt_set_textures)");
  if (kind == FrameGen::NMAP && c->matMaps && c->matMaps.texGeneration != c->tex.generation)
    return fail(RT_ERR_STATE, "the material maps were set for another texture set (rt_set_material_maps after rt_set_textures)");
  const rtk::TexRec T = c->tex.rec();
  switch (kind) {
    case FrameGen::NONE: G->gen = FrameGen(); break;
    case FrameGen::VCOL: G->vcol = rtk::VColRec{c->vcol.get()}, G->gen = FrameGen(G->vcol); break;
    case FrameGen::TEX: G->tex = T, G->gen = FrameGen(G->tex); break;
    case FrameGen::MAT:
      G->mat = rtk::MatRec{T.uv, T.meshTex, T.desc, T.texels, c->matMaps.f0.get(), c->matMaps.kdAlpha.get()}, G->gen = FrameGen(G->mat);
      break;
    case FrameGen::NMAP: {
      const uint32_t* f0 = c->matMaps ? c->matMaps.f0.get() : c->noMaps.get();
      const uint32_t* kdAlpha = c->matMaps ? c->matMaps.kdAlpha.get() : c->noMaps.get();
      G->nrm = rtk::NrmRec{rtk::MatRec{T.uv, T.meshTex, T.desc, T.texels, f0, kdAlpha}, c->nrmMaps.normal.get()}, G->gen = FrameGen(G->nrm);
      break;
    }
  }
  return RT_OK;
}

// rt_render_aov_device, rt_render_aov_colors_device or rt_render_aov_textured_device
int aov_device(rt_ctx* c, const rt_params* p, const rt_aov* out, void* stream, FrameGen::Surface alb) {
  rt_params q;
  int rc = aov_checks(c, p, &q);
  if (rc != RT_OK) return rc;
  if (!out) return fail(RT_ERR_INVALID, "aov is null");
  SurfaceGen G;
  if ((rc = resident_surface(c, alb, &G)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const rtk::AovArgs A = aov_args(q, *out);
  const bool brute = q.accel == RT_ACCEL_BRUTE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t he = rtk::launch_aov(brute, c->S, A, nullptr, 0, G.gen, s);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "AOV launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

// the host form of each
int aov_host(rt_ctx* c, const rt_params* p, const rt_aov* out, FrameGen::Surface alb) {
  rt_params q;
  int rc = aov_checks(c, p, &q);
  if (rc != RT_OK) return rc;
  if (!out) return fail(RT_ERR_INVALID, "aov is null");
  SurfaceGen G;
  if ((rc = resident_surface(c, alb, &G)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)q.width * q.height;
  Staging st;
  rt_aov d = {};
  d.albedo = st.out(out->albedo, 3 * npx), d.normal = st.out(out->normal, 3 * npx), d.position = st.out(out->position, 3 * npx);
  d.depth = st.out(out->depth, npx), d.hits = st.out(out->hits, npx), d.mesh = st.out(out->mesh, npx), d.tri = st.out(out->tri, npx);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = aov_device(c, &q, &d, nullptr, alb)) != RT_OK) return rc;
  return st.download();
}

}  // namespace

extern "C" {

int rt_render_aov_device(rt_ctx* c, const rt_params* p, const rt_aov* out, void* stream) { return aov_device(c, p, out, stream, FrameGen::NONE); }
int rt_render_aov(rt_ctx* c, const rt_params* p, const rt_aov* out) { return aov_host(c, p, out, FrameGen::NONE); }
int rt_render_aov_colors_device(rt_ctx* c, const rt_params* p, const rt_aov* out, void* stream) { return aov_device(c, p, out, stream, FrameGen::VCOL); }
int rt_render_aov_colors(rt_ctx* c, const rt_params* p, const rt_aov* out) { return aov_host(c, p, out, FrameGen::VCOL); }
int rt_render_aov_textured_device(rt_ctx* c, const rt_params* p, const rt_aov* out, void* stream) { return aov_device(c, p, out, stream, FrameGen::TEX); }
int rt_render_aov_textured(rt_ctx* c, const rt_params* p, const rt_aov* out) { return aov_host(c, p, out, FrameGen::TEX); }

int rt_denoise_device(rt_ctx* c, const rt_denoise_params* d, const void* d_rgb, const rt_aov* aov, void* d_out, void* stream) {
  int rc = denoise_checks(c, d, d_rgb, aov, d_out);
  if (rc != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  if ((rc = denoise_param_checks(d)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_filter_scratch(c, rtk::filter_scratch(d->width, d->height))) != RT_OK) return rc;
  const hipError_t he = rtk::launch_denoise(c->S, denoise_args(c, d, d_rgb, aov, d_out), static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "denoise launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_denoise(rt_ctx* c, const rt_denoise_params* d, const float* rgb, const rt_aov* aov, float* out) {
  int rc = denoise_checks(c, d, rgb, aov, out);
  if (rc != RT_OK) return rc;
  if ((rc = check_image_size(d->width, d->height)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)d->width * d->height;
  Staging st;
  const float* dRgb = st.in(rgb, 3 * npx);
  rt_aov da = {};
  da.albedo = st.in(aov->albedo, 3 * npx), da.normal = st.in(aov->normal, 3 * npx), da.position = st.in(aov->position, 3 * npx);
  da.hits = st.in(aov->hits, npx);
  float* dOut = st.out(out, 3 * npx);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = rt_denoise_device(c, d, dRgb, &da, dOut, nullptr)) != RT_OK) return rc;
  return st.download();
}

}  // extern "C"

// ---- motion vectors and temporal accumulation -------------------------------------------------------------------------
namespace {

// the defaults of rt_temporal_params (rt_amd.h, DESIGN.md "Motion vectors and temporal accumulation": chosen on two
// turntable sequences)
constexpr uint32_t kTemporalMaxHistory = 16;
constexpr float kTemporalSigmaScale = 0.02f;  // of the diagonal of the referenced vertices' box

bool any_set(const uint32_t* w, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (w[i]) return true;
  return false;
}

// Everything rt_render_motion checks before it touches the device; *q gets rt_render_aov's view of p.
int motion_checks(const rt_ctx* c, const rt_params* p, const rt_motion_prev* prev, const rt_motion* out, rt_params* q) {
  if (!c || !p || !prev || !out) return fail(RT_ERR_INVALID, "null argument");
  if (any_set(prev->reserved, 6) || any_set(out->reserved, 4)) return fail(RT_ERR_INVALID, "reserved words must be zero");
  if (prev->camera) {
    const float* f = prev->camera->position;  // (the four vectors are contiguous: 12 floats)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(f[i])) return fail(RT_ERR_INVALID, "the previous camera is not finite");
  }
  return aov_checks(c, p, q);
}

rtk::MotionArgs motion_args(const rt_ctx* c, const rt_params& q, const rt_motion_prev* prev, const float* dPrevPos, const rt_motion& out) {
  rtk::MotionArgs A;
  A.motion = out.motion, A.position = out.position, A.prevPosition = out.prev_position, A.mesh = out.mesh;
  A.prevVpos = dPrevPos ? dPrevPos : c->S.vpos;
  A.prevCam = prev->camera ? *prev->camera : c->S.cam;
  A.width = q.width, A.height = q.height, A.spp = q.spp, A.seed = q.seed;
  A.s0 = sample_range(q).s0;
  return A;
}

// Last frame's positions as a host form was given them (null: the scene's own), in the context's copy on the device
int upload_prev_positions(rt_ctx* c, const float* hostPos, const float** dPos) {
  *dPos = nullptr;
  if (!hostPos) return RT_OK;
  const size_t nv = 3 * (size_t)c->nVertices;
  if (!c->mvPrev) HIP_TRY(dev_alloc(&c->mvPrev, nv));
  HIP_TRY(hipMemcpy(c->mvPrev.get(), hostPos, nv * sizeof(float), hipMemcpyHostToDevice));
  *dPos = c->mvPrev.get();
  return RT_OK;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *x = static_cast<const char*>(a), *y = static_cast<const char*>(b);
  return x < y + nb && y < x + na;
}

// Everything rt_temporal_accumulate checks before it touches the device (and before it looks at the context).
int temporal_checks(const rt_ctx* c, const rt_temporal_params* t, const float* cur_rgb, const rt_motion* cur, const rt_history* prev,
                    const float* out_rgb, const float* out_length) {
  if (!c || !t || !cur_rgb || !cur || !prev || !out_rgb || !out_length) return fail(RT_ERR_INVALID, "null argument");
  int rc = check_motion_channels(cur);
  if (rc != RT_OK) return rc;
  if (!prev->rgb || !prev->position || !prev->mesh || !prev->length)
    return fail(RT_ERR_INVALID, "the history needs rgb, position, mesh and length");
  if ((rc = check_image_size(t->width, t->height)) != RT_OK) return rc;
  if (!(t->sigma_position >= 0.f) || !std::isfinite(t->sigma_position))
    return fail(RT_ERR_INVALID, "sigma_position must be finite and >= 0");
  if (!(t->alpha_min >= 0.f) || !(t->alpha_min <= 1.f)) return fail(RT_ERR_INVALID, "alpha_min must be 0 or in (0, 1]");
  if (any_set(t->reserved, 6) || any_set(cur->reserved, 4)) return fail(RT_ERR_INVALID, "reserved words must be zero");
  const size_t px = (size_t)t->width * t->height * sizeof(float);
  const void* const hist[4] = {prev->rgb, prev->position, prev->mesh, prev->length};
  const size_t histBytes[4] = {3 * px, 3 * px, px, px};
  for (int i = 0; i < 4; ++i)
    if (overlap(out_rgb, 3 * px, hist[i], histBytes[i]) || overlap(out_length, px, hist[i], histBytes[i]))
      return fail(RT_ERR_INVALID, "the outputs must not alias the history (taps read neighbouring pixels)");
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_motion_device(rt_ctx* c, const rt_params* p, const rt_motion_prev* prev, const rt_motion* out, void* stream) {
  rt_params q;
  int rc = motion_checks(c, p, prev, out, &q);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const rtk::MotionArgs A = motion_args(c, q, prev, prev->vertex_pos, *out);
  const hipError_t he = rtk::launch_motion(q.accel == RT_ACCEL_BRUTE, c->S, A, static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "motion launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_render_motion(rt_ctx* c, const rt_params* p, const rt_motion_prev* prev, const rt_motion* out) {
  rt_params q;
  int rc = motion_checks(c, p, prev, out, &q);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)q.width * q.height;
  const float* dPrevPos = nullptr;
  if ((rc = upload_prev_positions(c, prev->vertex_pos, &dPrevPos)) != RT_OK) return rc;
  Staging st;
  rt_motion d = {};
  d.motion = st.out(out->motion, 2 * npx), d.position = st.out(out->position, 3 * npx);
  d.prev_position = st.out(out->prev_position, 3 * npx), d.mesh = st.out(out->mesh, npx);
  if (st.rc != RT_OK) return st.rc;
  const rtk::MotionArgs A = motion_args(c, q, prev, dPrevPos, d);
  const hipError_t he = rtk::launch_motion(q.accel == RT_ACCEL_BRUTE, c->S, A, nullptr);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "motion launch failed: %s", hipGetErrorString(he));
  return st.download();
}

int rt_temporal_accumulate_device(rt_ctx* c, const rt_temporal_params* t, const void* d_cur_rgb, const rt_motion* cur,
                                  const rt_history* prev, void* d_out_rgb, void* d_out_length, void* stream) {
  int rc = temporal_checks(c, t, static_cast<const float*>(d_cur_rgb), cur, prev, static_cast<const float*>(d_out_rgb),
                           static_cast<const float*>(d_out_length));
  if (rc != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->tpScratch) HIP_TRY(dev_alloc(&c->tpScratch, 1));
  rtk::TemporalArgs T;
  T.width = t->width, T.height = t->height;
  T.maxHistory = t->max_history ? t->max_history : kTemporalMaxHistory;
  T.alphaMin = t->alpha_min, T.sigmaPosition = t->sigma_position, T.sigmaScale = kTemporalSigmaScale;
  T.curRgb = static_cast<const float*>(d_cur_rgb), T.motion = cur->motion, T.prevPosition = cur->prev_position, T.mesh = cur->mesh;
  T.hRgb = prev->rgb, T.hPosition = prev->position, T.hLength = prev->length, T.hMesh = prev->mesh;
  T.outRgb = static_cast<float*>(d_out_rgb), T.outLength = static_cast<float*>(d_out_length), T.block = c->tpScratch.get();
  const hipError_t he = rtk::launch_temporal(c->S, T, static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "temporal launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_temporal_accumulate(rt_ctx* c, const rt_temporal_params* t, const float* cur_rgb, const rt_motion* cur,
                           const rt_history* prev, float* out_rgb, float* out_length) {
  int rc = temporal_checks(c, t, cur_rgb, cur, prev, out_rgb, out_length);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)t->width * t->height;
  Staging st;
  const float* dRgb = st.in(cur_rgb, 3 * npx);
  rt_motion dc = {};
  dc.motion = st.in(cur->motion, 2 * npx), dc.prev_position = st.in(cur->prev_position, 3 * npx), dc.mesh = st.in(cur->mesh, npx);
  rt_history dh = {};
  dh.rgb = st.in(prev->rgb, 3 * npx), dh.position = st.in(prev->position, 3 * npx), dh.length = st.in(prev->length, npx);
  dh.mesh = st.in(prev->mesh, npx);
  float *dOut = st.out(out_rgb, 3 * npx), *dLen = st.out(out_length, npx);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = rt_temporal_accumulate_device(c, t, dRgb, &dc, &dh, dOut, dLen, nullptr)) != RT_OK) return rc;
  return st.download();
}

}  // extern "C"

// ---- variance-guided spatiotemporal filtering --------------------------------------------------------------------------
namespace {

// the defaults of rt_svgf_params (rt_amd.h, DESIGN.md "Variance-guided spatiotemporal filtering": chosen on two turntable
// sequences); the two position sigmas default to the denoiser's and the accumulation's fraction of the box diagonal
constexpr uint32_t kSvgfIterations = 5, kSvgfMaxHistory = 2;
constexpr float kSvgfSigmaLuminance = 2.f, kSvgfSigmaNormal = 0.5f, kSvgfSigmaScale = 0.02f;

// Everything rt_svgf checks before it touches the device (and before it looks at the context).
int svgf_checks(const rt_ctx* c, const rt_svgf_params* s, const float* cur_rgb, const rt_aov* aov, const rt_motion* cur,
                const rt_svgf_history* prev, const rt_svgf_out* out) {
  if (!c || !s || !cur_rgb || !aov || !cur || !prev || !out) return fail(RT_ERR_INVALID, "null argument");
  int rc = check_aov_channels(aov, "filter");
  if (rc != RT_OK) return rc;
  if ((rc = check_motion_channels(cur)) != RT_OK) return rc;
  if (!prev->color || !prev->moments || !prev->position || !prev->mesh || !prev->length)
    return fail(RT_ERR_INVALID, "the history needs color, moments, position, mesh and length");
  if (!out->rgb || !out->color || !out->moments || !out->length)
    return fail(RT_ERR_INVALID, "the outputs rgb, color, moments and length are required");
  if ((rc = check_image_size(s->width, s->height)) != RT_OK) return rc;
  if (s->iterations > 8) return fail(RT_ERR_INVALID, "iterations %u > 8", s->iterations);
  if ((rc = check_sigmas({s->sigma_luminance, s->sigma_normal, s->sigma_position, s->sigma_reproject})) != RT_OK) return rc;
  const float al[2] = {s->alpha_min, s->alpha_min_moments};
  for (float v : al)
    if (!(v >= 0.f) || !(v <= 1.f)) return fail(RT_ERR_INVALID, "alpha_min and alpha_min_moments must be 0 or in (0, 1]");
  if (any_set(s->reserved, 6) || any_set(aov->reserved, 4) || any_set(cur->reserved, 4) || any_set(out->reserved, 4))
    return fail(RT_ERR_INVALID, "reserved words must be zero");
  const size_t px = (size_t)s->width * s->height * sizeof(float);
  const void* const hist[5] = {prev->color, prev->moments, prev->position, prev->mesh, prev->length};
  const size_t histBytes[5] = {3 * px, 2 * px, 3 * px, px, px};
  const void* const outs[6] = {out->rgb, out->color, out->moments, out->length, out->accum, out->variance};
  const size_t outBytes[6] = {3 * px, 3 * px, 2 * px, px, 3 * px, px};
  for (int i = 0; i < 6; ++i) {
    if (!outs[i]) continue;
    for (int j = 0; j < 5; ++j)
      if (overlap(outs[i], outBytes[i], hist[j], histBytes[j]))
        return fail(RT_ERR_INVALID, "the outputs must not alias the history (taps read neighbouring pixels)");
    for (int j = i + 1; j < 6; ++j)
      if (outs[j] && overlap(outs[i], outBytes[i], outs[j], outBytes[j])) return fail(RT_ERR_INVALID, "the outputs must not alias one another");
  }
  // (the context exists only where a device does; a handle is not looked at before this)
  return check_device_present();
}

}  // namespace

extern "C" {

int rt_svgf_device(rt_ctx* c, const rt_svgf_params* s, const void* d_cur_rgb, const rt_aov* aov, const rt_motion* cur,
                   const rt_svgf_history* prev, const rt_svgf_out* out, void* stream) {
  int rc = svgf_checks(c, s, static_cast<const float*>(d_cur_rgb), aov, cur, prev, out);
  if (rc != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_filter_scratch(c, rtk::filter_scratch(s->width, s->height))) != RT_OK) return rc;
  rtk::SvgfArgs A;
  A.width = s->width, A.height = s->height;
  A.iterations = s->iterations ? s->iterations : kSvgfIterations;
  A.maxHistory = s->max_history ? s->max_history : kSvgfMaxHistory;
  A.alphaMin = s->alpha_min, A.alphaMinMoments = s->alpha_min_moments;
  A.sigmaLuminance = s->sigma_luminance > 0.f ? s->sigma_luminance : kSvgfSigmaLuminance;
  A.sigmaNormal = s->sigma_normal > 0.f ? s->sigma_normal : kSvgfSigmaNormal;
  A.sigmaPosition = s->sigma_position, A.sigmaReproject = s->sigma_reproject, A.sigmaScale = kSvgfSigmaScale;
  A.curRgb = static_cast<const float*>(d_cur_rgb), A.albedo = aov->albedo, A.normal = aov->normal, A.position = aov->position;
  A.hits = aov->hits, A.motion = cur->motion, A.prevPosition = cur->prev_position, A.mesh = cur->mesh;
  A.hColor = prev->color, A.hMoments = prev->moments, A.hPosition = prev->position, A.hLength = prev->length, A.hMesh = prev->mesh;
  A.outRgb = out->rgb, A.outColor = out->color, A.outMoments = out->moments, A.outLength = out->length;
  A.outAccum = out->accum, A.outVariance = out->variance, A.scratch = c->dnScratch.get();
  const hipError_t he = rtk::launch_svgf(c->S, A, static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "svgf launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_svgf(rt_ctx* c, const rt_svgf_params* s, const float* cur_rgb, const rt_aov* aov, const rt_motion* cur,
            const rt_svgf_history* prev, const rt_svgf_out* out) {
  int rc = svgf_checks(c, s, cur_rgb, aov, cur, prev, out);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)s->width * s->height;
  Staging st;
  const float* dRgb = st.in(cur_rgb, 3 * npx);
  rt_aov da = {};
  da.albedo = st.in(aov->albedo, 3 * npx), da.normal = st.in(aov->normal, 3 * npx), da.position = st.in(aov->position, 3 * npx);
  da.hits = st.in(aov->hits, npx);
  rt_motion dc = {};
  dc.motion = st.in(cur->motion, 2 * npx), dc.prev_position = st.in(cur->prev_position, 3 * npx), dc.mesh = st.in(cur->mesh, npx);
  rt_svgf_history dh = {};
  dh.color = st.in(prev->color, 3 * npx), dh.moments = st.in(prev->moments, 2 * npx), dh.position = st.in(prev->position, 3 * npx);
  dh.length = st.in(prev->length, npx), dh.mesh = st.in(prev->mesh, npx);
  rt_svgf_out dout = {};
  dout.rgb = st.out(out->rgb, 3 * npx), dout.color = st.out(out->color, 3 * npx), dout.moments = st.out(out->moments, 2 * npx);
  dout.length = st.out(out->length, npx), dout.accum = st.out(out->accum, 3 * npx), dout.variance = st.out(out->variance, npx);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = rt_svgf_device(c, s, dRgb, &da, &dc, &dh, &dout, nullptr)) != RT_OK) return rc;
  return st.download();
}

}  // extern "C"

// ---- adaptive sampling ----------------------------------------------------------------------------------------------
namespace {

// the defaults of rt_adaptive_params (rt_amd.h, DESIGN.md "Adaptive sampling")
constexpr uint32_t kAdaptiveMinPasses = 4;
constexpr float kAdaptiveFloor = 0.01f;

struct AdaptiveRule {
  uint32_t maxPasses, minPasses;
  float threshold, floor;
};

int adaptive_rule_checks(const rt_params* p, const rt_adaptive_params* a, AdaptiveRule* r);
// Everything an adaptive frame checks before it touches the device; *r gets the rule with its defaults applied.
int adaptive_checks(const rt_ctx* c, const rt_params* p, const rt_adaptive_params* a, AdaptiveRule* r) {
  if (!c) return fail(RT_ERR_INVALID, "ctx is null");
  if (!p) return fail(RT_ERR_INVALID, "params is null");
  if (!a) return fail(RT_ERR_INVALID, "adaptive params are null");
  const int rc = check_params(c, p);
  if (rc != RT_OK) return rc;
  return adaptive_rule_checks(p, a, r);
}
// ... of them, what p and a alone decide once p has a frame's shape (rt_render_adaptive_shutter asks this before the device)
int adaptive_rule_checks(const rt_params* p, const rt_adaptive_params* a, AdaptiveRule* r) {
  if (p->spp_begin || p->spp_count)
    return fail(RT_ERR_INVALID, "an adaptive frame runs whole passes of spp samples: spp_begin and spp_count must be 0");
  if (a->max_passes == 0) return fail(RT_ERR_INVALID, "max_passes must be >= 1");
  if ((uint64_t)a->max_passes * p->spp > 0x7fffffffull)
    return fail(RT_ERR_INVALID, "max_passes %u x spp %u exceeds 2^31 - 1 samples per pixel", a->max_passes, p->spp);
  if (a->min_passes && (a->min_passes < 2 || a->min_passes > a->max_passes))
    return fail(RT_ERR_INVALID, "min_passes %u outside 2..max_passes (%u)", a->min_passes, a->max_passes);
  if (!std::isfinite(a->threshold) || !(a->threshold >= 0.f)) return fail(RT_ERR_INVALID, "threshold must be finite and >= 0");
  const float fl = a->floor == 0.f ? kAdaptiveFloor : a->floor;
  if (!std::isfinite(fl) || !(fl > 0.f)) return fail(RT_ERR_INVALID, "floor must be finite and > 0");
  for (uint32_t v : a->reserved)
    if (v) return fail(RT_ERR_INVALID, "rt_adaptive_params.reserved must be zero");
  if (p->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded adaptive frames (world %u) are not supported", p->world);
  if (p->reserved[2] & 1u) return fail(RT_ERR_UNSUPPORTED, "adaptive frames do not run the wavefront integrator");
  r->maxPasses = a->max_passes;
  r->minPasses = a->min_passes ? a->min_passes : std::min(kAdaptiveMinPasses, a->max_passes);
  r->threshold = a->threshold, r->floor = fl;
  return RT_OK;
}

// The pass loop behind every adaptive entry point, on device buffers, after the checks: rule R over passes of the frame p
// describes, its primary rays formed by gen (rt_render_adaptive_shutter: the open shutter; else the frame's own).
int adaptive_run(rt_ctx* c, const rt_params* p, const AdaptiveRule& R, const FrameGen& gen, const void* d_bg, void* d_accum,
                 void* d_out, void* d_spp, void* stream, rt_adaptive_report* rep, rt_stats* stats,
                 std::chrono::steady_clock::time_point t0) {
  int rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t W = p->width, H = p->height, gx = (W + 7) / 8, gy = (H + 7) / 8, nG = gx * gy;
  const size_t npx = (size_t)W * H;
  // scratch: prev [npx] float4, moments [npx] double2, passes / retired / list [nG], tiles [64 nG], counts
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t oMom = up(npx * sizeof(float4)), oPass = oMom + up(npx * sizeof(double2)), oRet = oPass + up(nG * 4ull);
  const size_t oList = oRet + up(nG * 4ull), oTiles = oList + up(nG * 4ull), oCnt = oTiles + up(nG * 64ull * 4);
  const size_t need = oCnt + rtk::ADAPT_CNT_WORDS * 4;
  if ((rc = grow(&c->adScratch, &c->adCap, need)) != RT_OK) return rc;
  char* b = c->adScratch.get();
  rtk::AdaptArgs A;
  A.width = W, A.height = H, A.gx = gx, A.gy = gy, A.P = p->spp, A.minPasses = R.minPasses;
  A.threshold = R.threshold, A.floor = R.floor;
  A.accum = static_cast<const float4*>(d_accum), A.bg = static_cast<const float*>(d_bg);
  A.prev = reinterpret_cast<float4*>(b), A.mom = reinterpret_cast<double2*>(b + oMom);
  A.passes = reinterpret_cast<uint32_t*>(b + oPass), A.retired = reinterpret_cast<uint32_t*>(b + oRet);
  A.list = reinterpret_cast<uint32_t*>(b + oList), A.tiles = reinterpret_cast<uint32_t*>(b + oTiles);
  A.counts = reinterpret_cast<uint32_t*>(b + oCnt);
  Event ev[6];
  for (Event& e : ev) HIP_TRY(make_event(&e));
  HIP_TRY(hipMemsetAsync(b, 0, oList, s));  // prev, moments, passes, retired
  HIP_TRY(hipMemsetAsync(d_accum, 0, npx * sizeof(float4), s));
  if (stats) HIP_TRY(hipMemsetAsync(c->dCounters.get(), 0, RTK_CNT_COUNT * sizeof(unsigned long long), s));
  rt_adaptive_report out = {};
  out.granules = nG;
  double renderMs = 0., adaptMs = 0.;
  auto elapsed = [&](int i, int j, double* acc) {
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, ev[i].get(), ev[j].get());
    *acc += ms;
    return e;
  };
  bool pending = false;  // a pass whose events are not read yet
  rt_params q = *p;
  hipError_t he;
  // pass k: compaction of the active granules -> counts read back -> wave tiles for the pass's sshift -> the render
  // pass over them -> the rule over the granules it rendered
  for (uint32_t k = 0; k < R.maxPasses; ++k) {
    HIP_TRY(hipEventRecord(ev[0].get(), s));
    if ((he = rtk::launch_adapt_compact(A, s)) != hipSuccess) return fail(RT_ERR_HIP, "adaptive compaction failed: %s", hipGetErrorString(he));
    HIP_TRY(hipEventRecord(ev[1].get(), s));
    uint32_t cnt[rtk::ADAPT_CNT_WORDS];
    HIP_TRY(hipMemcpyAsync(cnt, A.counts, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(elapsed(0, 1, &adaptMs));
    if (pending) {
      HIP_TRY(elapsed(2, 3, &adaptMs));
      HIP_TRY(elapsed(3, 4, &renderMs));
      HIP_TRY(elapsed(4, 5, &adaptMs));
      pending = false;
    }
    const uint32_t nAct = cnt[rtk::ADAPT_CNT_GRANULES];
    if (nAct == 0) break;
    if (k < 64) out.active[k] = nAct;
    q.seed = p->seed + k;
    const uint32_t sshift = choose_sshift_px(c, &q, cnt[rtk::ADAPT_CNT_PIXELS], p->spp);
    uint32_t tw, th;
    wave_tile_shape(sshift, tw, th);
    HIP_TRY(hipEventRecord(ev[2].get(), s));
    if ((he = rtk::launch_adapt_expand(A, nAct, tw, th, s)) != hipSuccess) return fail(RT_ERR_HIP, "adaptive tile list failed: %s", hipGetErrorString(he));
    HIP_TRY(hipEventRecord(ev[3].get(), s));
    const TileList own = {A.tiles, cnt[rtk::ADAPT_CNT_TILES + sshift], sshift};
    if ((rc = launch_frame(c, &q, static_cast<float4*>(d_accum), s, nullptr, &own, gen)) != RT_OK) return rc;
    HIP_TRY(hipEventRecord(ev[4].get(), s));
    if ((he = rtk::launch_adapt_update(A, nAct, s)) != hipSuccess) return fail(RT_ERR_HIP, "adaptive update failed: %s", hipGetErrorString(he));
    HIP_TRY(hipEventRecord(ev[5].get(), s));
    pending = true;
    out.passes++;
    out.pixel_samples += (uint64_t)cnt[rtk::ADAPT_CNT_PIXELS] * p->spp;
  }
  he = rtk::launch_resolve_adaptive(A, static_cast<float*>(d_out), static_cast<uint32_t*>(d_spp), s);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "adaptive resolve failed: %s", hipGetErrorString(he));
  if (rep || stats) {
    HIP_TRY(hipStreamSynchronize(s));
    if (pending) {
      HIP_TRY(elapsed(2, 3, &adaptMs));
      HIP_TRY(elapsed(3, 4, &renderMs));
      HIP_TRY(elapsed(4, 5, &adaptMs));
    }
  }
  if (stats) {
    if ((rc = read_counters(c, stats)) != RT_OK) return rc;
    stats->kernel_ms = renderMs;
    stats->samples = out.pixel_samples;
  }
  if (rep) {
    out.render_ms = renderMs, out.adapt_ms = adaptMs;
    out.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *rep = out;
  }
  return RT_OK;
}

// The host forms: adaptive_run on device copies of the caller's buffers, on the null stream
int adaptive_host(rt_ctx* c, const rt_params* p, const AdaptiveRule& R, const FrameGen& gen, const float* bg, float* out_rgb,
                  float* accum_out, uint32_t* spp_out, rt_adaptive_report* rep, rt_stats* stats,
                  std::chrono::steady_clock::time_point t0) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)p->width * p->height;
  Staging st;
  float4* dAccum = st.work<float4>(accum_out, npx);  // (the pass loop zeroes it)
  const float* dBg = st.in(bg, 3 * npx);
  float* dOut = st.out(out_rgb, 3 * npx);
  uint32_t* dSpp = st.out(spp_out, npx);
  if (st.rc != RT_OK) return st.rc;
  int rc = adaptive_run(c, p, R, gen, dBg, dAccum, dOut, dSpp, nullptr, rep, stats, t0);
  if (rc != RT_OK) return rc;
  if ((rc = st.download()) != RT_OK) return rc;
  if (rep) rep->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RT_OK;
}

int shutter_record_checks(const rt_shutter* s, const char* who);
int shutter_params_checks(const rt_params* p);
int shutter_camera_checks(const rt_camera& A, float originBound, const rt_shutter* s, const char* who, rtk::ShutterRec* R);

// Everything both forms of rt_render_adaptive_shutter check, in the header's order: the arguments alone (rt_render_shutter's
// of the record and of p, then rt_render_adaptive's of p and a, then the form's own buffers), the device, then the context
// (rt_render's state checks) and its camera.
int adaptive_shutter_checks(const rt_ctx* c, const rt_params* p, const rt_adaptive_params* a, const rt_shutter* sh, bool buffers,
                            AdaptiveRule* r, rtk::ShutterRec* S) {
  if (!c || !p || !a || !sh) return fail(RT_ERR_INVALID, "ctx/params/adaptive params/shutter is null");
  int rc = shutter_record_checks(sh, "");
  if (rc != RT_OK) return rc;
  if ((rc = shutter_params_checks(p)) != RT_OK) return rc;
  if ((rc = adaptive_rule_checks(p, a, r)) != RT_OK) return rc;
  if (!buffers) return fail(RT_ERR_INVALID, "null argument");
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_params(c, p)) != RT_OK) return rc;
  return shutter_camera_checks(c->S.cam, c->bvh.originBound, sh, "", S);
}

}  // namespace

extern "C" {

int rt_render_adaptive_device(rt_ctx* c, const rt_params* p, const rt_adaptive_params* a, const void* d_bg, void* d_accum,
                              void* d_out, void* d_spp, void* stream, rt_adaptive_report* rep, rt_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  AdaptiveRule R;
  const int rc = adaptive_checks(c, p, a, &R);
  if (rc != RT_OK) return rc;
  if (!d_bg || !d_accum || !d_out) return fail(RT_ERR_INVALID, "null argument");
  return adaptive_run(c, p, R, FrameGen(), d_bg, d_accum, d_out, d_spp, stream, rep, stats, t0);
}

int rt_render_adaptive(rt_ctx* c, const rt_params* p, const rt_adaptive_params* a, const float* bg, float* out_rgb,
                       float* accum_out, uint32_t* spp_out, rt_adaptive_report* rep, rt_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  AdaptiveRule R;
  const int rc = adaptive_checks(c, p, a, &R);
  if (rc != RT_OK) return rc;
  if (!bg || !out_rgb) return fail(RT_ERR_INVALID, "null argument");
  return adaptive_host(c, p, R, FrameGen(), bg, out_rgb, accum_out, spp_out, rep, stats, t0);
}

// ---- adaptive frames under an open shutter
int rt_render_adaptive_shutter_device(rt_ctx* c, const rt_params* p, const rt_adaptive_params* a, const rt_shutter* sh,
                                      const void* d_bg, void* d_accum, void* d_out, void* d_spp, void* stream,
                                      rt_adaptive_report* rep, rt_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  AdaptiveRule R;
  rtk::ShutterRec S;
  const int rc = adaptive_shutter_checks(c, p, a, sh, d_bg && d_accum && d_out, &R, &S);
  if (rc != RT_OK) return rc;
  return adaptive_run(c, p, R, S, d_bg, d_accum, d_out, d_spp, stream, rep, stats, t0);
}

int rt_render_adaptive_shutter(rt_ctx* c, const rt_params* p, const rt_adaptive_params* a, const rt_shutter* sh, const float* bg,
                               float* out_rgb, float* accum_out, uint32_t* spp_out, rt_adaptive_report* rep, rt_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  AdaptiveRule R;
  rtk::ShutterRec S;
  const int rc = adaptive_shutter_checks(c, p, a, sh, bg && out_rgb, &R, &S);
  if (rc != RT_OK) return rc;
  return adaptive_host(c, p, R, S, bg, out_rgb, accum_out, spp_out, rep, stats, t0);
}

}  // extern "C"

// ---- many views of one scene (DESIGN.md "Multi-view frames") --------------------------------------------------------
namespace {

// What a multi-view frame checks in p and v alone ...
int views_shape_checks(const rt_params* p, const rt_views* v) {
  if (v->reserved0) return fail(RT_ERR_INVALID, "rt_views.reserved0 must be zero");
  for (uint32_t r : v->reserved)
    if (r) return fail(RT_ERR_INVALID, "rt_views.reserved must be zero");
  if (v->n_views == 0 || v->n_views > 65535u) return fail(RT_ERR_INVALID, "n_views %u out of range 1..65535", v->n_views);
  if ((uint64_t)v->n_views * p->width * p->height >= (1ull << 31))
    return fail(RT_ERR_INVALID, "%u views of %ux%u pixels: 2^31 pixels or more", v->n_views, p->width, p->height);
  if (p->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded multi-view frames (world %u) are not supported", p->world);
  if (p->reserved[2] & 1u) return fail(RT_ERR_UNSUPPORTED, "multi-view frames do not run the wavefront integrator");
  return RT_OK;
}
// ... and everything it checks before it touches the device, and the padding its farthest view needs:
// *refit = true when that is wider than the context's (rt_amd.h: the camera rule).
int views_checks(rt_ctx* c, const rt_params* p, const rt_views* v, rtbvh::Padding* pad, bool* refit) {
  if (!c || !p || !v || !v->cameras) return fail(RT_ERR_INVALID, "ctx/params/views/cameras is null");
  int rc = check_params(c, p);
  if (rc != RT_OK) return rc;
  if ((rc = views_shape_checks(p, v)) != RT_OK) return rc;
  // rt_update's rules, per view camera in place of the context's
  const float magRef = bits_float(c->magRef);
  *pad = rtbvh::Padding{c->bvh.pad, c->bvh.originBound, c->bvh.boxScale};
  *refit = false;
  for (uint32_t j = 0; j < v->n_views; ++j) {
    const rt_camera& cam = v->cameras[j];
    if (max_abs_bits(cam.position, 12) >= 0x7f800000u) return fail(RT_ERR_INVALID, "view %u: non-finite camera", j);
    if (c->S.slowRecip == 0u && !short_forms_bound(c, cam))
      return fail(RT_ERR_INVALID, "view %u: camera beyond the short forms' operand bounds (rt_update to it instead)", j);
    const rtbvh::Padding P = rtbvh::paddingRule(magRef, cam, c->hostLights.data(), (uint32_t)c->hostLights.size());
    if (P.pad > pad->pad) *pad = P, *refit = true;
  }
  if (*refit && c->nodeFormat == RT_NODES_Q8)
    return fail(RT_ERR_UNSUPPORTED, "views need a wider box padding (%g) and RT_NODES_Q8 contexts cannot be refit", pad->pad);
  return RT_OK;
}

// A camera-only rt_update on `stream` to the padding the farthest view of a multi-view call needs; the context does not
// take that view's camera.
int refit_to_padding(rt_ctx* c, const rtbvh::Padding& pad, hipStream_t stream) {
  const int rc = update_checks(c, nullptr, 0);
  if (rc != RT_OK) return rc;
  Update x;
  x.padding = &pad;
  return update_ctx(c, x, stream, std::chrono::steady_clock::now(), nullptr);
}

// The view-major wave tiles of n views (each view's as a single-view frame has them) and each tile's view, cached on the
// context by (frame, sshift, n)
int ensure_view_tiles(rt_ctx* c, const rt_params* p, uint32_t sshift, uint32_t n, hipStream_t stream) {
  const TileKey k = tile_key(p, sshift);
  if (c->vwTiles.d && k == c->vwKey && n == c->vwViews) {
    const int rc = use_on(c->vwTiles, stream);
    return rc != RT_OK ? rc : use_on(c->vwTileView, stream);
  }
  c->vwNTiles = 0, c->vwViews = 0;
  const std::vector<uint32_t> one = wave_tiles(k);
  std::vector<uint32_t> tiles, view;
  tiles.reserve(one.size() * n), view.reserve(one.size() * n);
  for (uint32_t j = 0; j < n; ++j) {
    tiles.insert(tiles.end(), one.begin(), one.end());
    view.insert(view.end(), one.size(), j);
  }
  int rc = stream_upload(&c->vwTiles, tiles, stream);
  if (rc == RT_OK) rc = stream_upload(&c->vwTileView, view, stream);
  if (rc != RT_OK) return rc;
  c->vwNTiles = static_cast<uint32_t>(tiles.size()), c->vwViews = n, c->vwKey = k;
  return RT_OK;
}

// The view records — and, for the motion pass, last frame's camera of every view (prevCams, else null), ahead of them —
// to the device on `stream`, through the next slot of the ring of pinned copies: the host waits only until the uploads that
// last read that slot, kViewStages calls ago, have finished.  The device tables are written and read in stream order;
// where they grow, the old ones are freed under launches that may still read them, which hipFree waits for.
// shutters: the views' shutter records of a multi-view shutter frame (else null), a third table through the same slot.
int upload_views(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_camera* prevCams, hipStream_t stream,
                 const rtk::ViewShutterRec* shutters = nullptr) {
  const uint32_t n = v->n_views;
  rt_ctx::ViewStage& g = c->vwStage[c->vwStageNext++ % rt_ctx::kViewStages];
  if (!g.read) HIP_TRY(make_event(&g.read, hipEventDisableTiming));
  if (g.readSet) HIP_TRY(hipEventSynchronize(g.read.get()));
  g.readSet = false;
  int rc = grow(&g.recs, &g.cap, n);
  if (rc == RT_OK && prevCams) rc = grow(&g.prevCams, &g.prevCap, n);
  if (rc == RT_OK) rc = grow(&c->vwRecs, &c->vwCap, n);
  if (rc == RT_OK && prevCams) rc = grow(&c->vwPrevCams, &c->vwPrevCap, n);
  if (rc == RT_OK && shutters) rc = grow(&g.shutters, &g.shutterCap, n);
  if (rc == RT_OK && shutters) rc = grow(&c->vwShutters, &c->vwShutterCap, n);
  if (rc != RT_OK) return rc;
  if (shutters) {
    memcpy(g.shutters.get(), shutters, n * sizeof(rtk::ViewShutterRec));
    HIP_TRY(hipMemcpyAsync(c->vwShutters.get(), g.shutters.get(), n * sizeof(rtk::ViewShutterRec), hipMemcpyHostToDevice, stream));
  }
  if (prevCams) {
    memcpy(g.prevCams.get(), prevCams, n * sizeof(rt_camera));
    HIP_TRY(hipMemcpyAsync(c->vwPrevCams.get(), g.prevCams.get(), n * sizeof(rt_camera), hipMemcpyHostToDevice, stream));
  }
  rtk::ViewRec* h = g.recs.get();
  const uint32_t px = p->width * p->height;
  for (uint32_t j = 0; j < n; ++j) {
    h[j] = rtk::ViewRec{};
    h[j].cam = v->cameras[j];
    h[j].seed = v->seeds ? v->seeds[j] : p->seed;
    h[j].accumOff = j * px;
  }
  HIP_TRY(hipMemcpyAsync(c->vwRecs.get(), h, n * sizeof(rtk::ViewRec), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(g.read.get(), stream));
  g.readSet = true;
  return RT_OK;
}

// The multi-view frame of checked p and v into d_accum on `stream`, behind rt_render_views_device and both forms of
// rt_render_views_shutter: pad and refit as views_checks (or views_shutter_checks) left them; shutters: the views'
// shutter records, the third table of a multi-view shutter frame, or null.  gen: with shutters, the colours or textures
// the frame shades with (rt_render_views_shutter_albedo), else none.
int views_frame_device(rt_ctx* c, const rt_params* p, const rt_views* v, const rtk::ViewShutterRec* shutters, const rtbvh::Padding& pad,
                       bool refit, void* d_accum, void* stream, rt_stats* stats, const FrameGen& gen = FrameGen()) {
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  if (refit && (rc = refit_to_padding(c, pad, s)) != RT_OK) return rc;
  const uint32_t n = v->n_views;
  const uint32_t sppCount = sample_range(*p).count;
  const uint32_t sshift = choose_sshift_px(c, p, (uint64_t)n * p->width * p->height, sppCount);
  if ((rc = ensure_view_tiles(c, p, sshift, n, s)) != RT_OK) return rc;
  if ((rc = upload_views(c, p, v, nullptr, s, shutters)) != RT_OK) return rc;
  if (stats) HIP_TRY(hipMemsetAsync(c->dCounters.get(), 0, RTK_CNT_COUNT * sizeof(unsigned long long), s));
  TileList own = {c->vwTiles.d.get(), c->vwNTiles, sshift};
  own.tileView = c->vwTileView.d.get(), own.views = c->vwRecs.get(), own.viewShutters = shutters ? c->vwShutters.get() : nullptr;
  int e = 0;
  if ((rc = launch_frame(c, p, static_cast<float4*>(d_accum), s, &e, &own, gen)) != RT_OK) return rc;
  return stats ? frame_stats(c, s, e, (uint64_t)n * p->width * p->height * sppCount, stats) : (int)RT_OK;
}

// The host form of such a frame, after its checks: frame_host's steps over one accumulator slice per view, each view
// resolved over its slice with the shared background.
int views_frame_host(rt_ctx* c, const rt_params* p, const rt_views* v, const rtk::ViewShutterRec* shutters, const rtbvh::Padding& pad,
                     bool refit, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats, const FrameGen& gen = FrameGen()) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)p->width * p->height, all = npx * v->n_views;
  Staging st;
  float4* dAccum = st.zeroed<float4>(accum_out, all);
  if (st.rc != RT_OK) return st.rc;
  rt_stats local;
  int rc = views_frame_device(c, p, v, shutters, pad, refit, dAccum, nullptr, stats ? stats : &local, gen);
  if (rc != RT_OK) return rc;
  if ((rc = stage_resolve(&st, bg, out_rgb, dAccum, v->n_views, npx, p->spp)) != RT_OK) return rc;
  return st.download();
}

}  // namespace

extern "C" {

int rt_render_views_device(rt_ctx* c, const rt_params* p, const rt_views* v, void* d_accum, void* stream, rt_stats* stats) {
  rtbvh::Padding pad;
  bool refit = false;
  int rc = views_checks(c, p, v, &pad, &refit);
  if (rc != RT_OK) return rc;
  if (!d_accum) return fail(RT_ERR_INVALID, "d_accum is null");
  return views_frame_device(c, p, v, nullptr, pad, refit, d_accum, stream, stats);
}

int rt_render_views(rt_ctx* c, const rt_params* p, const rt_views* v, const float* bg, float* out_rgb, float* accum_out,
                    rt_stats* stats) {
  rtbvh::Padding pad;
  bool refit = false;
  int rc = views_checks(c, p, v, &pad, &refit);
  if (rc != RT_OK) return rc;
  if (out_rgb && !bg) return fail(RT_ERR_INVALID, "out_rgb requested without a background image");
  return views_frame_host(c, p, v, nullptr, pad, refit, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- ambient occlusion and bent normals at the first hit ----------------------------------------------
namespace {

// Everything rt_render_ao checks, in the header's order.  What can be told from the arguments alone is answered before
// the context is looked at, and a context exists only where a device does.  *q: p as rt_render_aov sees it (the wavefront
// bit selects an integrator and does not matter here either).
int ao_checks(const rt_ctx* c, const rt_params* p, const rt_ao_params* a, const rt_ao* out, rt_params* q) {
  if (!c || !p || !a || !out) return fail(RT_ERR_INVALID, "ctx/params/ao params/ao is null");
  if (any_set(a->reserved, 5) || any_set(out->reserved, 4)) return fail(RT_ERR_INVALID, "reserved words must be zero");
  if (a->n_rays == 0 || a->n_rays > RT_AO_MAX_RAYS) return fail(RT_ERR_INVALID, "n_rays %u outside 1..%d", a->n_rays, RT_AO_MAX_RAYS);
  if ((uint64_t)p->spp * a->n_rays >= (1ull << 32)) return fail(RT_ERR_INVALID, "spp * n_rays (%u * %u) does not fit 32 bits", p->spp, a->n_rays);
  if (!(a->bias >= 0.f) || !std::isfinite(a->bias)) return fail(RT_ERR_INVALID, "bias must be finite and >= 0");
  if (!(a->max_distance >= 0.f) || !std::isfinite(a->max_distance)) return fail(RT_ERR_INVALID, "max_distance must be finite and >= 0");
  *q = aov_params(*p);
  q->reserved[2] &= ~1u;
  int rc = check_params_shape(q);
  if (rc != RT_OK) return rc;
  if (q->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded ambient occlusion (world %u) is not supported", q->world);
  if ((rc = check_device_present()) != RT_OK) return rc;
  return check_not_broken(c);
}

// The launch behind both forms: q and a have passed ao_checks, out holds device pointers.
int ao_launch(rt_ctx* c, const rt_params& q, const rt_ao_params* a, const rt_ao* out, hipStream_t s) {
  HIP_TRY(hipSetDevice(c->device));
  rtk::AoArgs A{};
  A.unoccluded = out->unoccluded, A.hits = out->hits, A.bent = out->bent;
  A.width = q.width, A.height = q.height, A.spp = q.spp, A.seed = q.seed;
  A.s0 = sample_range(q).s0, A.s1 = sample_range(q).s1;
  A.nRays = a->n_rays, A.bias = a->bias, A.maxDistance = a->max_distance;
  if (a->bias == 0.f) {
    if (!c->aoExt) HIP_TRY(dev_alloc(&c->aoExt, 6));
    const hipError_t he = rtk::launch_ref_extent(c->S, c->aoExt.get(), s);
    if (he != hipSuccess) return fail(RT_ERR_HIP, "extent reduction failed: %s", hipGetErrorString(he));
    A.ext = c->aoExt.get();
  }
  const hipError_t he = rtk::launch_ao(q.accel == RT_ACCEL_BRUTE, c->S, A, s);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "ambient occlusion launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_ao_device(rt_ctx* c, const rt_params* p, const rt_ao_params* a, const rt_ao* out, void* stream) {
  rt_params q;
  const int rc = ao_checks(c, p, a, out, &q);
  if (rc != RT_OK) return rc;
  return ao_launch(c, q, a, out, static_cast<hipStream_t>(stream));
}

int rt_render_ao(rt_ctx* c, const rt_params* p, const rt_ao_params* a, const rt_ao* out) {
  rt_params q;
  int rc = ao_checks(c, p, a, out, &q);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)q.width * q.height;
  Staging st;
  rt_ao d = {};
  d.unoccluded = st.out(out->unoccluded, npx), d.hits = st.out(out->hits, npx), d.bent = st.out(out->bent, 3 * npx);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = ao_launch(c, q, a, &d, nullptr)) != RT_OK) return rc;
  return st.download();
}

}  // extern "C"

// ---- the integrator over ray batches of the caller's --------------------------------------------------
namespace {

// Everything both forms of rt_render_rays check in their arguments, in the header's order; the device is asked for by
// the caller, behind its own checks.  *q: p with the ignored size neutralised.
int rays_checks(const rt_ctx* c, const rt_params* p, const rt_ray_batch* b, rt_params* q) {
  if (!c || !p || !b || !b->rays) return fail(RT_ERR_INVALID, "ctx/params/batch/rays is null");
  if (b->reserved0 || any_set(b->reserved, 6)) return fail(RT_ERR_INVALID, "rt_ray_batch: reserved words must be zero");
  if (b->n == 0 || b->n >= (1u << 31)) return fail(RT_ERR_INVALID, "n %u outside 1..2^31-1", b->n);
  *q = *p;
  q->width = q->height = 1;
  const int rc = check_params_shape(q);
  if (rc != RT_OK) return rc;
  if (q->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded ray batches (world %u) are not supported", q->world);
  if (q->use_photons) return fail(RT_ERR_UNSUPPORTED, "ray batches do not shade from the photon map");
  if (q->reserved[2] & 1u) return fail(RT_ERR_UNSUPPORTED, "ray batches do not run the wavefront integrator");
  return RT_OK;
}

// unit3(d) (rt_device.h) has a non-finite component or is the null vector: d is null or not finite, or its squared
// length — (x x + y y) + z z in float32, as dot3 forms it — overflows
bool degenerate_direction(const float* d) {
  if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) return true;
  if (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f) return true;
  const float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
  const float xy = xx + yy;
  const float len2 = xy + zz;
  return !std::isfinite(len2);
}

// The launch behind both forms: q and b have passed rays_checks, b holds device pointers.  Bracketed by an event pair.
int rays_launch(rt_ctx* c, const rt_params& q, const rt_ray_batch& b, float4* dAccum, hipStream_t s, rt_stats* stats) {
  if (stats) HIP_TRY(hipMemsetAsync(c->dCounters.get(), 0, RTK_CNT_COUNT * sizeof(unsigned long long), s));
  rtk::RaysArgs A{};
  A.rays = b.rays, A.streamIndex = b.stream_index, A.n = b.n;
  A.spp = q.spp, A.mode = q.mode, A.max_depth = q.max_depth, A.seed = q.seed;
  A.s0 = sample_range(q).s0, A.s1 = sample_range(q).s1;
  A.flags = (q.reserved[1] & 1u) ? 0u : 1u;
  A.stackLevels = stack_levels(c->bvh.maxDepth > 1 ? c->bvh.maxDepth : 1);
  int e = 0;
  const int rc = timed_launch(c, s, &e, [&] {
    const hipError_t he = rtk::launch_render_rays(q.accel == RT_ACCEL_BRUTE, q.collect_stats != 0, c->S, A, dAccum, c->dCounters.get(), s);
    return he != hipSuccess ? fail(RT_ERR_HIP, "ray batch launch failed: %s", hipGetErrorString(he)) : (int)RT_OK;
  });
  if (rc != RT_OK || !stats) return rc;
  return frame_stats(c, s, e, (uint64_t)b.n * (A.s1 - A.s0), stats);
}

}  // namespace

extern "C" {

int rt_render_rays_device(rt_ctx* c, const rt_params* p, const rt_ray_batch* b, void* d_accum, void* stream, rt_stats* stats) {
  rt_params q;
  int rc = rays_checks(c, p, b, &q);
  if (rc != RT_OK) return rc;
  if (!d_accum) return fail(RT_ERR_INVALID, "d_accum is null");
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return rays_launch(c, q, *b, static_cast<float4*>(d_accum), static_cast<hipStream_t>(stream), stats);
}

int rt_render_rays(rt_ctx* c, const rt_params* p, const rt_ray_batch* b, const float* bg, float* out_rgb, float* accum_out,
                   rt_stats* stats) {
  rt_params q;
  int rc = rays_checks(c, p, b, &q);
  if (rc != RT_OK) return rc;
  if (!out_rgb && !accum_out) return fail(RT_ERR_INVALID, "neither out_rgb nor accum_out is given");
  if (out_rgb && !bg) return fail(RT_ERR_INVALID, "out_rgb requested without a background");
  const size_t n = b->n;
  for (size_t r = 0; r < n; ++r) {
    const rt_ray& ray = b->rays[r];
    if (!std::isfinite(ray.origin[0]) || !std::isfinite(ray.origin[1]) || !std::isfinite(ray.origin[2]))
      return fail(RT_ERR_INVALID, "ray %zu: non-finite origin", r);
    if (degenerate_direction(ray.direction))
      return fail(RT_ERR_INVALID, "ray %zu: direction (%g, %g, %g) cannot be normalised", r, ray.direction[0], ray.direction[1], ray.direction[2]);
  }
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = grow(&c->rbRays, &c->rbCap, n)) != RT_OK) return rc;
  if (b->stream_index && (rc = grow(&c->rbIndex, &c->rbIndexCap, n)) != RT_OK) return rc;
  HIP_TRY(hipMemcpy(c->rbRays.get(), b->rays, n * sizeof(rt_ray), hipMemcpyHostToDevice));
  if (b->stream_index) HIP_TRY(hipMemcpy(c->rbIndex.get(), b->stream_index, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  rt_ray_batch d = *b;
  d.rays = c->rbRays.get(), d.stream_index = b->stream_index ? c->rbIndex.get() : nullptr;
  Staging st;
  float4* dAccum = st.zeroed<float4>(accum_out, n);
  if (st.rc != RT_OK) return st.rc;
  rt_stats local;
  if ((rc = rays_launch(c, q, d, dAccum, nullptr, stats ? stats : &local)) != RT_OK) return rc;
  // the batch as an image n wide and 1 high
  if ((rc = stage_resolve(&st, bg, out_rgb, dAccum, 1, n, q.spp)) != RT_OK) return rc;
  return st.download();
}

}  // extern "C"

// ---- the frame through a thin lens --------------------------------------------------------------------
namespace {

// Vec3.h:170-178 in float32 as the device forms it (rt_device.h unit3); false for a null or non-finite vector
bool unit3_host(const float* a, float* u) {
  const float xx = a[0] * a[0], yy = a[1] * a[1], zz = a[2] * a[2];
  const float xy = xx + yy;
  const float l = std::sqrt(xy + zz);
  if (!(l > 0.f) || !std::isfinite(l)) return false;
  const float inv = 1.0f / l;
  for (int k = 0; k < 3; ++k) u[k] = a[k] * inv;
  return true;
}

// The fs rule of rt_amd.h for one camera: the distance of the image plane along the optical axis in float64 (the header
// states the order), focus_distance over it rounded to float32; RT_ERR_INVALID unless that is finite and > 0.
int focus_scale(const rt_camera& cam, float focus_distance, float* fs, const char* who = "") {
  double cc[3], H[3], V[3];
  for (int k = 0; k < 3; ++k) {
    H[k] = cam.horizontal[k], V[k] = cam.vertical[k];
    cc[k] = (((double)cam.lower_left[k] + 0.5 * H[k]) + 0.5 * V[k]) - (double)cam.position[k];
  }
  const double n[3] = {H[1] * V[2] - H[2] * V[1], H[2] * V[0] - H[0] * V[2], H[0] * V[1] - H[1] * V[0]};
  const double cn = (cc[0] * n[0] + cc[1] * n[1]) + cc[2] * n[2], nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  const double plane = std::fabs(cn) / std::sqrt(nn);
  *fs = (float)((double)focus_distance / plane);
  if (!(*fs > 0.f) || !std::isfinite(*fs))
    return fail(RT_ERR_INVALID, "%sfocus_distance %g over the image plane's distance %g is not a finite positive float", who, focus_distance, plane);
  return RT_OK;
}

// Everything both forms of rt_render_lens check, in the header's order, and the record the kernels take.  outputs: what is
// wrong with the form's own buffers, or null.  What can be told from the arguments alone is answered before the device is
// asked for, and the camera is read last: a context exists only where a device does.
int lens_checks(const rt_ctx* c, const rt_params* p, const rt_lens* l, const char* outputs, rtk::LensRec* R) {
  if (!c || !p || !l) return fail(RT_ERR_INVALID, "ctx/params/lens is null");
  if (outputs) return fail(RT_ERR_INVALID, "%s", outputs);
  if (any_set(l->reserved, 5)) return fail(RT_ERR_INVALID, "rt_lens: reserved words must be zero");
  if (l->model != RT_LENS_THIN) return fail(RT_ERR_INVALID, "unknown lens model %u", l->model);
  if (!(l->aperture >= 0.f) || !std::isfinite(l->aperture)) return fail(RT_ERR_INVALID, "aperture must be finite and >= 0");
  const bool open = l->aperture > 0.f;
  if (open && (!(l->focus_distance > 0.f) || !std::isfinite(l->focus_distance)))
    return fail(RT_ERR_INVALID, "focus_distance must be finite and > 0");
  int rc = check_params_shape(p);
  if (rc != RT_OK) return rc;
  if ((rc = frame_params_checks(p, "lens")) != RT_OK) return rc;
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  const rt_camera& cam = c->S.cam;
  float m = 0.f;
  for (int k = 0; k < 3; ++k) m = std::max(m, std::fabs(cam.position[k]));
  const float reach = m + 2.f * l->aperture;
  if (reach > c->bvh.originBound)
    return fail(RT_ERR_INVALID, "the lens reaches %g from the origin, beyond the context's origin bound %g", reach, c->bvh.originBound);
  *R = rtk::LensRec{};
  R->aperture = l->aperture;
  if (!open) return RT_OK;  // (the frame's own camera_ray: fs is neither computed nor checked)
  if (!unit3_host(cam.horizontal, R->hu) || !unit3_host(cam.vertical, R->vu))
    return fail(RT_ERR_INVALID, "the camera's horizontal or vertical axis cannot be normalised");
  return focus_scale(cam, l->focus_distance, &R->fs);
}

// max_c |a_c| of a 3-vector
float max_abs3(const float* a) { return std::max(std::fabs(a[0]), std::max(std::fabs(a[1]), std::fabs(a[2]))); }

// rt_render_shutter's checks in three parts, so that rt_render_views_shutter applies them per view: who prefixes every
// message ("" or "view j: ").  First what the record alone decides ...
int shutter_record_checks(const rt_shutter* s, const char* who) {
  if (any_set(s->reserved, 4)) return fail(RT_ERR_INVALID, "%srt_shutter: reserved words must be zero", who);
  const float* b = reinterpret_cast<const float*>(&s->camera_close);  // (the twelve components: rt_camera is four float[3])
  static_assert(sizeof(rt_camera) == 12 * sizeof(float), "rt_camera is twelve floats");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(b[k])) return fail(RT_ERR_INVALID, "%scamera_close: component %d is not finite", who, k);
  if (!std::isfinite(s->open) || !std::isfinite(s->close) || !(0.f <= s->open && s->open <= s->close && s->close <= 1.f))
    return fail(RT_ERR_INVALID, "%sthe exposure must be finite with 0 <= open <= close <= 1", who);
  if (!(s->aperture >= 0.f) || !std::isfinite(s->aperture)) return fail(RT_ERR_INVALID, "%saperture must be finite and >= 0", who);
  if (s->aperture > 0.f && (!(s->focus_distance > 0.f) || !std::isfinite(s->focus_distance)))
    return fail(RT_ERR_INVALID, "%sfocus_distance must be finite and > 0", who);
  return RT_OK;
}
// ... then what p alone decides ...
int shutter_params_checks(const rt_params* p) {
  const int rc = check_params_shape(p);
  return rc != RT_OK ? rc : frame_params_checks(p, "shutter");
}
// ... and last what reads the camera A the shutter opens on (the context's, or a view's) and the origin bound the frame
// runs under, and the record the kernels take.
int shutter_camera_checks(const rt_camera& A, float originBound, const rt_shutter* s, const char* who, rtk::ShutterRec* R) {
  const rt_camera& B = s->camera_close;
  const float *a = reinterpret_cast<const float*>(&A), *b = reinterpret_cast<const float*>(&B);
  *R = rtk::ShutterRec{};
  for (int k = 0; k < 12; ++k) R->d[k] = b[k] - a[k];  // (finite: both ends are, and the open camera lies within the scene's input bound)
  R->open = s->open, R->close = s->close, R->aperture = s->aperture;
  // pos(t) = posA + t D may pass an end point by one rounding: one float above the larger end covers every value
  const float reach = std::nextafter(std::max(max_abs3(A.position), max_abs3(B.position)), INFINITY) + 2.f * s->aperture;
  if (reach > originBound)
    return fail(RT_ERR_INVALID, "%sthe moving camera reaches %g from the origin, beyond the context's origin bound %g", who, reach, originBound);
  float u[3];
  if (!unit3_host(A.horizontal, u) || !unit3_host(A.vertical, u) || !unit3_host(B.horizontal, u) || !unit3_host(B.vertical, u))
    return fail(RT_ERR_INVALID, "%sa horizontal or vertical axis of the open camera or of camera_close cannot be normalised", who);
  double hh = 0., vv = 0.;
  for (int k = 0; k < 3; ++k) hh += (double)A.horizontal[k] * (double)B.horizontal[k], vv += (double)A.vertical[k] * (double)B.vertical[k];
  if (!(hh > 0.) || !(vv > 0.))
    return fail(RT_ERR_INVALID, "%sthe camera's horizontal or vertical axis turns by 90 degrees or more between open and close: an interpolated axis could vanish", who);
  if (!(s->aperture > 0.f)) return RT_OK;
  float fs1;
  int rc;
  if ((rc = focus_scale(A, s->focus_distance, &R->fs0, who)) != RT_OK || (rc = focus_scale(B, s->focus_distance, &fs1, who)) != RT_OK) return rc;
  R->dfs = fs1 - R->fs0;
  return RT_OK;
}

// Everything both forms of rt_render_shutter check, in the header's order, and the record the kernels take (lens_checks'
// shape: the arguments alone first, then the device, the context's camera last).
int shutter_checks(const rt_ctx* c, const rt_params* p, const rt_shutter* s, const char* outputs, rtk::ShutterRec* R) {
  if (!c || !p || !s) return fail(RT_ERR_INVALID, "ctx/params/shutter is null");
  if (outputs) return fail(RT_ERR_INVALID, "%s", outputs);
  int rc = shutter_record_checks(s, "");
  if (rc != RT_OK) return rc;
  if ((rc = shutter_params_checks(p)) != RT_OK) return rc;
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  return shutter_camera_checks(c->S.cam, c->bvh.originBound, s, "", R);
}

}  // namespace

extern "C" {

int rt_render_lens_device(rt_ctx* c, const rt_params* p, const rt_lens* l, void* d_accum, void* stream, rt_stats* stats) {
  rtk::LensRec R;
  const int rc = lens_checks(c, p, l, d_accum ? nullptr : "d_accum is null", &R);
  if (rc != RT_OK) return rc;
  return frame_device(c, p, R, d_accum, stream, stats);
}

int rt_render_lens(rt_ctx* c, const rt_params* p, const rt_lens* l, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  rtk::LensRec R;
  const int rc = lens_checks(c, p, l, outputs_refused(bg, out_rgb, accum_out), &R);
  if (rc != RT_OK) return rc;
  return frame_host(c, p, R, 1, bg, out_rgb, accum_out, stats);
}

// ---- the frame under an open shutter
int rt_render_shutter_device(rt_ctx* c, const rt_params* p, const rt_shutter* sh, void* d_accum, void* stream, rt_stats* stats) {
  rtk::ShutterRec R;
  const int rc = shutter_checks(c, p, sh, d_accum ? nullptr : "d_accum is null", &R);
  if (rc != RT_OK) return rc;
  return frame_device(c, p, R, d_accum, stream, stats);
}

int rt_render_shutter(rt_ctx* c, const rt_params* p, const rt_shutter* sh, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  rtk::ShutterRec R;
  const int rc = shutter_checks(c, p, sh, outputs_refused(bg, out_rgb, accum_out), &R);
  if (rc != RT_OK) return rc;
  return frame_host(c, p, R, 1, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- the frame split by light group -------------------------------------------------------------------
namespace {

// Everything both forms of rt_render_lights check, in the header's order, and the record the kernels take (lens_checks'
// shape: the arguments alone first, then the device, the context's lights last).
int lights_checks(const rt_ctx* c, const rt_params* p, const rt_light_groups* g, const char* outputs, rtk::LightGroupsRec* R) {
  if (!c || !p || !g) return fail(RT_ERR_INVALID, "ctx/params/groups is null");
  if (g->n_groups < 1 || g->n_groups > RT_LIGHT_GROUPS_MAX)
    return fail(RT_ERR_INVALID, "n_groups %u is not in 1..%d", g->n_groups, RT_LIGHT_GROUPS_MAX);
  if (any_set(g->reserved, 3)) return fail(RT_ERR_INVALID, "rt_light_groups: reserved words must be zero");
  for (uint32_t j = g->n_groups; j < RT_LIGHT_GROUPS_MAX; ++j)
    if (g->masks[j]) return fail(RT_ERR_INVALID, "masks[%u] = 0x%x is set beyond n_groups %u", j, g->masks[j], g->n_groups);
  if (outputs) return fail(RT_ERR_INVALID, "%s", outputs);
  int rc = check_params_shape(p);
  if (rc != RT_OK) return rc;
  if ((rc = frame_params_checks(p, "light-group")) != RT_OK) return rc;
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  const uint32_t nl = c->S.n_lights;
  if (nl > 32u) return fail(RT_ERR_UNSUPPORTED, "the context has %u lights: a group mask holds 32", nl);
  *R = rtk::LightGroupsRec{};
  R->n = g->n_groups;
  for (uint32_t j = 0; j < g->n_groups; ++j) {
    if (nl < 32u && (g->masks[j] >> nl))
      return fail(RT_ERR_INVALID, "group %u: mask 0x%x names a light at or above the context's n_lights %u", j, g->masks[j], nl);
    R->masks[j] = g->masks[j];
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_lights_device(rt_ctx* c, const rt_params* p, const rt_light_groups* g, void* d_accum, void* stream, rt_stats* stats) {
  rtk::LightGroupsRec R;
  const int rc = lights_checks(c, p, g, d_accum ? nullptr : "d_accum is null", &R);
  if (rc != RT_OK) return rc;
  return frame_device(c, p, R, d_accum, stream, stats);
}

int rt_render_lights(rt_ctx* c, const rt_params* p, const rt_light_groups* g, const float* bg, float* out_rgb, float* accum_out,
                     rt_stats* stats) {
  rtk::LightGroupsRec R;
  const int rc = lights_checks(c, p, g, outputs_refused(bg, out_rgb, accum_out), &R);
  if (rc != RT_OK) return rc;
  return frame_host(c, p, R, R.n, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- sampled direct lighting for scenes of many lights ------------------------------------------------
namespace {

// The table of a call (rt_amd.h): the scaled lights L'_k and the thresholds t_k.
struct PickTable {
  std::vector<rtk::PickLight> lights;
  std::vector<float> thresholds;
};

// Everything both forms of rt_render_pick check, in the header's order (lights_checks' shape: the arguments alone first,
// then the device, the context's lights last), and the table the kernels read.
int pick_checks(const rt_ctx* c, const rt_params* p, const rt_light_pick* k, const char* outputs, PickTable* T) {
  if (!c || !p || !k) return fail(RT_ERR_INVALID, "ctx/params/pick is null");
  if (k->slots < 1 || k->slots > RT_PICK_SLOTS_MAX) return fail(RT_ERR_INVALID, "slots %u is not in 1..%d", k->slots, RT_PICK_SLOTS_MAX);
  if (any_set(k->reserved, 5)) return fail(RT_ERR_INVALID, "rt_light_pick: reserved words must be zero");
  if (k->importance && !k->n_importance) return fail(RT_ERR_INVALID, "importance is given with n_importance 0");
  if (!k->importance && k->n_importance) return fail(RT_ERR_INVALID, "n_importance is %u and importance is null", k->n_importance);
  bool anyPositive = false;
  for (uint32_t j = 0; j < k->n_importance; ++j) {
    const float q = k->importance[j];
    if (!std::isfinite(q) || q < 0.f) return fail(RT_ERR_INVALID, "importance[%u] = %g is negative or not finite", j, (double)q);
    anyPositive = anyPositive || q > 0.f;
  }
  if (k->importance && !anyPositive) return fail(RT_ERR_INVALID, "all %u importance values are zero", k->n_importance);
  if (outputs) return fail(RT_ERR_INVALID, "%s", outputs);
  int rc = check_params_shape(p);
  if (rc != RT_OK) return rc;
  if ((rc = frame_params_checks(p, "light-pick")) != RT_OK) return rc;
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  const uint32_t n = (uint32_t)c->hostLights.size(), m = k->slots;
  if (n == 0) return fail(RT_ERR_INVALID, "the context has no lights to pick from");
  if (k->importance && k->n_importance != n) return fail(RT_ERR_INVALID, "n_importance %u is not the context's n_lights %u", k->n_importance, n);
  // the importance q_k: the caller's, or the lights' power proxy
  std::vector<double> q(n);
  if (k->importance) {
    for (uint32_t j = 0; j < n; ++j) q[j] = (double)k->importance[j];
  } else {
    bool any = false;
    for (uint32_t j = 0; j < n; ++j) {
      const rt_light& L = c->hostLights[j];
      const double v = (double)L.intensity * (double)L.factor * (((double)L.color[0] + L.color[1]) + L.color[2]) * (double)L.side * (double)L.side;
      q[j] = std::isfinite(v) && v > 0. ? v : 0.;
      any = any || q[j] > 0.;
    }
    if (!any) std::fill(q.begin(), q.end(), 1.);
  }
  double Q = 0.;
  uint32_t last = 0;  // the last light that can be picked
  for (uint32_t j = 0; j < n; ++j) {
    Q += q[j];
    if (q[j] > 0.) last = j;
  }
  T->lights.assign(n, rtk::PickLight{});
  T->thresholds.resize(n);
  double C = 0.;
  for (uint32_t j = 0; j < n; ++j) {
    const double pj = q[j] / Q;
    C += pj;
    T->thresholds[j] = j >= last ? 1.0f : (float)C;
    rt_light L = c->hostLights[j];
    if (pj > 0.) {
      const float w = (float)(1.0 / ((double)m * pj));
      if (!std::isfinite(w))
        return fail(RT_ERR_INVALID, "light %u: probability %g with %u slots gives a weight that is not finite", j, pj, m);
      for (float& x : L.color) x = w * x;
    }
    T->lights[j].l = L;
  }
  return RT_OK;
}

// The table to the device on `stream` through the next slot of the ring of pinned copies (upload_views' rule), and the
// record the kernels take.  The device block is written and read in stream order; where it grows, the old one is freed
// under launches that may still read it, which hipFree waits for.
int stage_pick(rt_ctx* c, const rt_light_pick* k, const PickTable& T, hipStream_t stream, rtk::PickRec* R) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = T.lights.size(), lightBytes = n * sizeof(rtk::PickLight), bytes = lightBytes + n * sizeof(float);
  rt_ctx::PickStage& g = c->pkStage[c->pkStageNext++ % rt_ctx::kViewStages];
  if (!g.read) HIP_TRY(make_event(&g.read, hipEventDisableTiming));
  if (g.readSet) HIP_TRY(hipEventSynchronize(g.read.get()));
  g.readSet = false;
  int rc = grow(&g.h, &g.cap, bytes);
  if (rc == RT_OK) rc = grow(&c->pkTable, &c->pkCap, bytes);
  if (rc != RT_OK) return rc;
  memcpy(g.h.get(), T.lights.data(), lightBytes);
  memcpy(g.h.get() + lightBytes, T.thresholds.data(), n * sizeof(float));
  HIP_TRY(hipMemcpyAsync(c->pkTable.get(), g.h.get(), bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(g.read.get(), stream));
  g.readSet = true;
  R->m = k->slots, R->n = (uint32_t)n;
  R->lights = reinterpret_cast<const rtk::PickLight*>(c->pkTable.get());
  R->thresholds = reinterpret_cast<const float*>(c->pkTable.get() + lightBytes);
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_pick_device(rt_ctx* c, const rt_params* p, const rt_light_pick* k, void* d_accum, void* stream, rt_stats* stats) {
  PickTable T;
  int rc = pick_checks(c, p, k, d_accum ? nullptr : "d_accum is null", &T);
  if (rc != RT_OK) return rc;
  rtk::PickRec R;
  if ((rc = stage_pick(c, k, T, static_cast<hipStream_t>(stream), &R)) != RT_OK) return rc;
  return frame_device(c, p, R, d_accum, stream, stats);
}

int rt_render_pick(rt_ctx* c, const rt_params* p, const rt_light_pick* k, const float* bg, float* out_rgb, float* accum_out,
                   rt_stats* stats) {
  PickTable T;
  int rc = pick_checks(c, p, k, outputs_refused(bg, out_rgb, accum_out), &T);
  if (rc != RT_OK) return rc;
  rtk::PickRec R;
  if ((rc = stage_pick(c, k, T, nullptr, &R)) != RT_OK) return rc;
  return frame_host(c, p, R, 1, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- per-vertex albedo ---------------------------------------------------------------------------------
namespace {

// Everything both forms of rt_render_colors, rt_render_textured, rt_render_material and rt_render_normal_mapped check, in the header's order
// (lens_checks' shape: the arguments alone first, then the device, the context last), and the surface the kernels take.
int surface_checks(const rt_ctx* c, const rt_params* p, const char* outputs, FrameGen::Surface kind, SurfaceGen* G) {
  static const char* const nouns[] = {"", "coloured", "textured", "material-map", "normal-mapped"};
  if (!c || !p) return fail(RT_ERR_INVALID, "ctx/params is null");
  if (outputs) return fail(RT_ERR_INVALID, "%s", outputs);
  int rc = check_params_shape(p);
  if (rc != RT_OK) return rc;
  if ((rc = frame_params_checks(p, nouns[kind])) != RT_OK) return rc;
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = check_not_broken(c)) != RT_OK) return rc;
  return resident_surface(c, kind, G);
}

// the device and the host form of each
int surface_frame_device(rt_ctx* c, const rt_params* p, FrameGen::Surface kind, void* d_accum, void* stream, rt_stats* stats) {
  SurfaceGen G;
  const int rc = surface_checks(c, p, d_accum ? nullptr : "d_accum is null", kind, &G);
  if (rc != RT_OK) return rc;
  return frame_device(c, p, G.gen, d_accum, stream, stats);
}
int surface_frame_host(rt_ctx* c, const rt_params* p, FrameGen::Surface kind, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  SurfaceGen G;
  const int rc = surface_checks(c, p, outputs_refused(bg, out_rgb, accum_out), kind, &G);
  if (rc != RT_OK) return rc;
  return frame_host(c, p, G.gen, 1, bg, out_rgb, accum_out, stats);
}

}  // namespace

extern "C" {

int rt_set_vertex_colors(rt_ctx* c, const float* rgb, uint32_t n_vertices) {
  if (!rgb) {
    if (!c) return fail(RT_ERR_INVALID, "ctx/rgb is null");
    HIP_TRY(hipSetDevice(c->device));
    c->vcol.reset();
    return RT_OK;
  }
  // what the array says of itself comes before anything of the context
  for (size_t j = 0; j < 3 * (size_t)n_vertices; ++j)
    if (!std::isfinite(rgb[j]))
      return fail(RT_ERR_INVALID, "vertex colours: rgb[%zu] (vertex %zu, component %zu) is not finite", j, j / 3, j % 3);
  if (!c) return fail(RT_ERR_INVALID, "ctx/rgb is null");
  if (n_vertices != c->nVertices) return fail(RT_ERR_INVALID, "vertex colours: %u vertices for a context of %u", n_vertices, c->nVertices);
  int rc = check_not_broken(c);  // (as rt_set_skin: nothing is uploaded to a context that refuses launches)
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  // the new colours replace the old ones only when all of them are resident; the old array is then freed under launches
  // that may still read it, which hipFree waits for
  DevBuf<float> fresh;
  if ((rc = upload(&fresh, rgb, 3 * (size_t)n_vertices)) != RT_OK) return rc;
  c->vcol = std::move(fresh);
  return RT_OK;
}

int rt_render_colors_device(rt_ctx* c, const rt_params* p, void* d_accum, void* stream, rt_stats* stats) {
  return surface_frame_device(c, p, FrameGen::VCOL, d_accum, stream, stats);
}
int rt_render_colors(rt_ctx* c, const rt_params* p, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  return surface_frame_host(c, p, FrameGen::VCOL, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- image-textured albedo ------------------------------------------------------------------------------
namespace {

constexpr uint32_t kTexMaxSide = 16384u;       // with |uv| <= kTexMaxUv: int(floorf(s * W)) stays far inside int32 (rt_kernels.hip tex_sample)
constexpr float kTexMaxUv = 1024.f;
constexpr uint64_t kTexMaxTexels = 1ull << 28;  // 3 floats each: the pool's float index stays below 2^32

// What a texture set says of itself, before anything of a context: the headers of all textures, then the total, then
// the texels (so no texel of a refused header is read), the meshes' indices and the uvs.
int texture_set_checks(const rt_texture_set* t) {
  if (!t->textures || !t->mesh_texture || !t->vertex_uv) return fail(RT_ERR_INVALID, "textures: textures/mesh_texture/vertex_uv is null");
  if (t->n_textures == 0) return fail(RT_ERR_INVALID, "textures: n_textures is 0");
  for (int k = 0; k < 4; ++k)
    if (t->reserved[k]) return fail(RT_ERR_INVALID, "textures: reserved[%d] of the set is %u, not 0", k, t->reserved[k]);
  uint64_t total = 0;
  for (uint32_t i = 0; i < t->n_textures; ++i) {
    const rt_texture& x = t->textures[i];
    if (x.width < 1u || x.width > kTexMaxSide) return fail(RT_ERR_INVALID, "textures: texture %u: width %u is outside 1..%u", i, x.width, kTexMaxSide);
    if (x.height < 1u || x.height > kTexMaxSide) return fail(RT_ERR_INVALID, "textures: texture %u: height %u is outside 1..%u", i, x.height, kTexMaxSide);
    if (x.wrap_s > (uint32_t)RT_TEX_CLAMP) return fail(RT_ERR_INVALID, "textures: texture %u: wrap_s %u is unknown", i, x.wrap_s);
    if (x.wrap_t > (uint32_t)RT_TEX_CLAMP) return fail(RT_ERR_INVALID, "textures: texture %u: wrap_t %u is unknown", i, x.wrap_t);
    if (x.filter > (uint32_t)RT_TEX_BILINEAR) return fail(RT_ERR_INVALID, "textures: texture %u: filter %u is unknown", i, x.filter);
    for (int k = 0; k < 3; ++k)
      if (x.reserved[k]) return fail(RT_ERR_INVALID, "textures: texture %u: reserved[%d] is %u, not 0", i, k, x.reserved[k]);
    if (!x.texels) return fail(RT_ERR_INVALID, "textures: texture %u: texels is null", i);
    total += (uint64_t)x.width * x.height;
    if (total > kTexMaxTexels) return fail(RT_ERR_INVALID, "textures: %llu texels up to texture %u, more than %llu", (unsigned long long)total, i, (unsigned long long)kTexMaxTexels);
  }
  for (uint32_t i = 0; i < t->n_textures; ++i) {
    const rt_texture& x = t->textures[i];
    const size_t n = 3 * (size_t)x.width * x.height;
    for (size_t j = 0; j < n; ++j)
      if (!std::isfinite(x.texels[j]))
        return fail(RT_ERR_INVALID, "textures: texture %u: texels[%zu] (row %zu, column %zu, component %zu) is not finite", i, j,
                    j / 3 / x.width, j / 3 % x.width, j % 3);
  }
  for (uint32_t m = 0; m < t->n_meshes; ++m)
    if (t->mesh_texture[m] != RT_TEX_NONE && t->mesh_texture[m] >= t->n_textures)
      return fail(RT_ERR_INVALID, "textures: mesh_texture[%u] is %u: neither one of %u textures nor RT_TEX_NONE", m, t->mesh_texture[m], t->n_textures);
  for (size_t j = 0; j < 2 * (size_t)t->n_vertices; ++j)
    if (!std::isfinite(t->vertex_uv[j]) || std::fabs(t->vertex_uv[j]) > kTexMaxUv)
      return fail(RT_ERR_INVALID, "textures: vertex_uv[%zu] (vertex %zu, component %zu) is %g: not finite or beyond %g", j, j / 2, j % 2,
                  (double)t->vertex_uv[j], (double)kTexMaxUv);
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_set_textures(rt_ctx* c, const rt_texture_set* t) {
  if (!t) {
    if (!c) return fail(RT_ERR_INVALID, "ctx/textures is null");
    HIP_TRY(hipSetDevice(c->device));
    rt_ctx::TexSet none;
    none.generation = c->tex.generation + 1;  // (resident material maps are stale from here on)
    c->tex = std::move(none);
    return RT_OK;
  }
  int rc = texture_set_checks(t);
  if (rc != RT_OK) return rc;
  if (!c) return fail(RT_ERR_INVALID, "ctx/textures is null");
  if (t->n_meshes != c->nMeshes) return fail(RT_ERR_INVALID, "textures: %u meshes for a context of %u", t->n_meshes, c->nMeshes);
  if (t->n_vertices != c->nVertices) return fail(RT_ERR_INVALID, "textures: %u vertices for a context of %u", t->n_vertices, c->nVertices);
  if ((rc = check_not_broken(c)) != RT_OK) return rc;  // (as rt_set_vertex_colors: nothing is uploaded to a context that refuses launches)
  HIP_TRY(hipSetDevice(c->device));
  // the pool: every texture's texels one behind the other, and where each starts
  std::vector<rtk::TexDesc> desc(t->n_textures);
  size_t total = 0;
  for (uint32_t i = 0; i < t->n_textures; ++i) {
    const rt_texture& x = t->textures[i];
    desc[i] = rtk::TexDesc{(uint32_t)total, x.width, x.height,
                           (x.wrap_s == RT_TEX_CLAMP ? rtk::TEX_CLAMP_S : 0u) | (x.wrap_t == RT_TEX_CLAMP ? rtk::TEX_CLAMP_T : 0u) |
                               (x.filter == RT_TEX_BILINEAR ? rtk::TEX_BILINEAR : 0u)};
    total += (size_t)x.width * x.height;
  }
  // the new set replaces the old one only when all of it is resident; the old arrays are then freed under launches that
  // may still read them, which hipFree waits for
  rt_ctx::TexSet fresh;
  HIP_TRY(dev_alloc(&fresh.texels, 3 * total));
  for (uint32_t i = 0; i < t->n_textures; ++i)
    HIP_TRY(hipMemcpy(fresh.texels.get() + 3 * (size_t)desc[i].offset, t->textures[i].texels,
                      3 * sizeof(float) * (size_t)desc[i].width * desc[i].height, hipMemcpyHostToDevice));
  if ((rc = upload(&fresh.uv, t->vertex_uv, 2 * (size_t)t->n_vertices)) != RT_OK ||
      (rc = upload(&fresh.meshTex, t->mesh_texture, t->n_meshes)) != RT_OK || (rc = upload(&fresh.desc, desc.data(), desc.size())) != RT_OK)
    return rc;
  fresh.generation = c->tex.generation + 1, fresh.nTextures = t->n_textures;  // (resident material maps are stale from here on)
  c->tex = std::move(fresh);
  return RT_OK;
}

int rt_render_textured_device(rt_ctx* c, const rt_params* p, void* d_accum, void* stream, rt_stats* stats) {
  return surface_frame_device(c, p, FrameGen::TEX, d_accum, stream, stats);
}
int rt_render_textured(rt_ctx* c, const rt_params* p, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  return surface_frame_host(c, p, FrameGen::TEX, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- textured material maps -----------------------------------------------------------------------------
extern "C" {

int rt_set_material_maps(rt_ctx* c, const rt_material_maps* m) {
  if (!m) {
    if (!c) return fail(RT_ERR_INVALID, "ctx/maps is null");
    HIP_TRY(hipSetDevice(c->device));
    c->matMaps = rt_ctx::MatMaps();
    return RT_OK;
  }
  const int word = rtmat::first_reserved(*m);
  if (word >= 0) return fail(RT_ERR_INVALID, "material maps: reserved[%d] is %u, not 0", word, m->reserved[word]);
  if (!c) return fail(RT_ERR_INVALID, "ctx/maps is null");
  if (m->n_meshes != c->nMeshes) return fail(RT_ERR_INVALID, "material maps: %u meshes for a context of %u", m->n_meshes, c->nMeshes);
  int rc = check_not_broken(c);  // (as rt_set_textures: nothing is uploaded to a context that refuses launches)
  if (rc != RT_OK) return rc;
  if (!c->tex) return fail(RT_ERR_STATE, "the context has no resident textures (rt_set_textures)");
  rtmat::Tables tables;
  std::string why;
  if (!rtmat::build_tables(*m, c->tex.nTextures, &tables, &why)) return fail(RT_ERR_INVALID, "%s", why.c_str());
  HIP_TRY(hipSetDevice(c->device));
  // the new tables replace the old ones only when both are resident; the old ones are then freed under launches that may
  // still read them, which hipFree waits for
  rt_ctx::MatMaps fresh;
  if ((rc = upload(&fresh.f0, tables.f0.data(), tables.f0.size())) != RT_OK ||
      (rc = upload(&fresh.kdAlpha, tables.kdAlpha.data(), tables.kdAlpha.size())) != RT_OK)
    return rc;
  fresh.texGeneration = c->tex.generation;
  c->matMaps = std::move(fresh);
  return RT_OK;
}

int rt_render_material_device(rt_ctx* c, const rt_params* p, void* d_accum, void* stream, rt_stats* stats) {
  return surface_frame_device(c, p, FrameGen::MAT, d_accum, stream, stats);
}
int rt_render_material(rt_ctx* c, const rt_params* p, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  return surface_frame_host(c, p, FrameGen::MAT, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- tangent-space normal maps ---------------------------------------------------------------------------
extern "C" {

int rt_set_normal_maps(rt_ctx* c, const rt_normal_maps* m) {
  if (!m) {
    if (!c) return fail(RT_ERR_INVALID, "ctx/maps is null");
    HIP_TRY(hipSetDevice(c->device));
    c->nrmMaps = rt_ctx::NrmMaps();
    return RT_OK;
  }
  const int word = rtnrm::first_reserved(*m);
  if (word >= 0) return fail(RT_ERR_INVALID, "normal maps: reserved[%d] is %u, not 0", word, m->reserved[word]);
  if (!c) return fail(RT_ERR_INVALID, "ctx/maps is null");
  if (m->n_meshes != c->nMeshes) return fail(RT_ERR_INVALID, "normal maps: %u meshes for a context of %u", m->n_meshes, c->nMeshes);
  int rc = check_not_broken(c);  // (as rt_set_material_maps: nothing is uploaded to a context that refuses launches)
  if (rc != RT_OK) return rc;
  if (!c->tex) return fail(RT_ERR_STATE, "the context has no resident textures (rt_set_textures)");
  std::vector<uint32_t> table;
  std::string why;
  if (!rtnrm::build_table(*m, c->tex.nTextures, &table, &why)) return fail(RT_ERR_INVALID, "%s", why.c_str());
  HIP_TRY(hipSetDevice(c->device));
  // the table of RT_TEX_NONE a frame without material maps reads: made once, never written again
  if (!c->noMaps) {
    const std::vector<uint32_t> none(c->nMeshes, RT_TEX_NONE);
    if ((rc = upload(&c->noMaps, none.data(), none.size())) != RT_OK) return rc;
  }
  // the new table replaces the old one only when it is resident; the old one is then freed under launches that may still
  // read it, which hipFree waits for
  rt_ctx::NrmMaps fresh;
  if ((rc = upload(&fresh.normal, table.data(), table.size())) != RT_OK) return rc;
  fresh.texGeneration = c->tex.generation;
  c->nrmMaps = std::move(fresh);
  return RT_OK;
}

int rt_render_normal_mapped_device(rt_ctx* c, const rt_params* p, void* d_accum, void* stream, rt_stats* stats) {
  return surface_frame_device(c, p, FrameGen::NMAP, d_accum, stream, stats);
}
int rt_render_normal_mapped(rt_ctx* c, const rt_params* p, const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  return surface_frame_host(c, p, FrameGen::NMAP, bg, out_rgb, accum_out, stats);
}

}  // extern "C"

// ---- many views, each under its own open shutter ------------------------------------------------------
namespace {

// Everything both forms of rt_render_views_shutter check, in the header's order.  The arguments alone first: p and v as
// rt_render_views checks them, the view cameras' finiteness, then rt_render_shutter's checks of p and, view by view, of the
// record; then the device; then the context: rt_render_views' camera rule with every camera_close counted in the padding,
// and rt_render_shutter's camera checks per view with cameras[j] in the place of the context's camera, under the origin
// bound the frame runs with (*pad's).  recs: the records the kernels take.
// albedo (rt_render_views_shutter_albedo; RT_ALBEDO_MATERIAL is the plain form): a value that is none of the three is
// refused among the arguments, and data the context does not hold last of all.  G: the surface the frame shades with.
int views_shutter_checks(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_shutter* sh, const char* outputs,
                         rtbvh::Padding* pad, bool* refit, std::vector<rtk::ViewShutterRec>* recs, uint32_t albedo,
                         SurfaceGen* G) {
  if (!c || !p || !v || !v->cameras) return fail(RT_ERR_INVALID, "ctx/params/views/cameras is null");
  if (!sh) return fail(RT_ERR_INVALID, "shutters is null");
  if (outputs) return fail(RT_ERR_INVALID, "%s", outputs);
  if (albedo > RT_ALBEDO_TEXTURES) return fail(RT_ERR_INVALID, "albedo %u is none of RT_ALBEDO_MATERIAL, RT_ALBEDO_COLORS, RT_ALBEDO_TEXTURES", albedo);
  int rc = check_params_shape(p);
  if (rc != RT_OK) return rc;
  if ((rc = views_shape_checks(p, v)) != RT_OK) return rc;
  if ((rc = shutter_params_checks(p)) != RT_OK) return rc;
  char who[32];
  for (uint32_t j = 0; j < v->n_views; ++j) {
    if (max_abs_bits(v->cameras[j].position, 12) >= 0x7f800000u) return fail(RT_ERR_INVALID, "view %u: non-finite camera", j);
    snprintf(who, sizeof who, "view %u: ", j);
    if ((rc = shutter_record_checks(&sh[j], who)) != RT_OK) return rc;
  }
  if ((rc = check_device_present()) != RT_OK) return rc;
  if ((rc = views_checks(c, p, v, pad, refit)) != RT_OK) return rc;
  const float magRef = bits_float(c->magRef);
  for (uint32_t j = 0; j < v->n_views; ++j) {
    const rtbvh::Padding P = rtbvh::paddingRule(magRef, sh[j].camera_close, c->hostLights.data(), (uint32_t)c->hostLights.size());
    if (P.pad > pad->pad) *pad = P, *refit = true;
  }
  if (*refit && c->nodeFormat == RT_NODES_Q8)
    return fail(RT_ERR_UNSUPPORTED, "views need a wider box padding (%g) and RT_NODES_Q8 contexts cannot be refit", pad->pad);
  recs->resize(v->n_views);
  for (uint32_t j = 0; j < v->n_views; ++j) {
    snprintf(who, sizeof who, "view %u: ", j);
    rtk::ShutterRec R;
    if ((rc = shutter_camera_checks(v->cameras[j], pad->originBound, &sh[j], who, &R)) != RT_OK) return rc;
    rtk::ViewShutterRec& Q = (*recs)[j];
    Q = rtk::ViewShutterRec{};
    memcpy(Q.d, R.d, sizeof Q.d);
    Q.open = R.open, Q.close = R.close, Q.aperture = R.aperture, Q.fs0 = R.fs0, Q.dfs = R.dfs;
  }
  return resident_surface(c, albedo_surface(albedo), G);
}

}  // namespace

extern "C" {

int rt_render_views_shutter_device(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_shutter* shutters, void* d_accum,
                                   void* stream, rt_stats* stats) {
  return rt_render_views_shutter_albedo_device(c, p, v, shutters, RT_ALBEDO_MATERIAL, d_accum, stream, stats);
}
int rt_render_views_shutter(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_shutter* shutters, const float* bg,
                            float* out_rgb, float* accum_out, rt_stats* stats) {
  return rt_render_views_shutter_albedo(c, p, v, shutters, RT_ALBEDO_MATERIAL, bg, out_rgb, accum_out, stats);
}

int rt_render_views_shutter_albedo_device(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_shutter* shutters, uint32_t albedo,
                                          void* d_accum, void* stream, rt_stats* stats) {
  rtbvh::Padding pad;
  bool refit = false;
  std::vector<rtk::ViewShutterRec> recs;
  SurfaceGen G;
  const int rc = views_shutter_checks(c, p, v, shutters, d_accum ? nullptr : "d_accum is null", &pad, &refit, &recs, albedo, &G);
  if (rc != RT_OK) return rc;
  return views_frame_device(c, p, v, recs.data(), pad, refit, d_accum, stream, stats, G.gen);
}

int rt_render_views_shutter_albedo(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_shutter* shutters, uint32_t albedo,
                                   const float* bg, float* out_rgb, float* accum_out, rt_stats* stats) {
  rtbvh::Padding pad;
  bool refit = false;
  std::vector<rtk::ViewShutterRec> recs;
  SurfaceGen G;
  const int rc = views_shutter_checks(c, p, v, shutters, outputs_refused(bg, out_rgb, accum_out), &pad, &refit, &recs, albedo, &G);
  if (rc != RT_OK) return rc;
  return views_frame_host(c, p, v, recs.data(), pad, refit, bg, out_rgb, accum_out, stats, G.gen);
}

}  // extern "C"

// ---- per-view AOVs and motion vectors, and the batched denoiser (DESIGN.md "Multi-view frames") ----------------------
namespace {

// What rt_render_aov_views and rt_render_motion_views check once their own pointers and reserved words are in order: p
// as rt_render_aov sees it (*q; the wavefront bit selects an integrator and does not matter here either), then
// rt_render_views' checks.  Everything that can be told from the arguments alone is answered before the context is looked
// at, and a context exists only where a device does.  prevCams: last frame's camera of each view, or null.
int views_pass_checks(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_camera* prevCams, rt_params* q, rtbvh::Padding* pad,
                      bool* refit) {
  *q = aov_params(*p);
  q->reserved[2] &= ~1u;
  int rc = check_params_shape(q);
  if (rc != RT_OK) return rc;
  if (q->world > 1) return fail(RT_ERR_UNSUPPORTED, "tile-sharded AOVs (world %u) are not supported", q->world);
  if ((rc = views_shape_checks(q, v)) != RT_OK) return rc;
  for (uint32_t j = 0; j < v->n_views; ++j) {
    if (max_abs_bits(v->cameras[j].position, 12) >= 0x7f800000u) return fail(RT_ERR_INVALID, "view %u: non-finite camera", j);
    if (prevCams && max_abs_bits(prevCams[j].position, 12) >= 0x7f800000u)
      return fail(RT_ERR_INVALID, "view %u: the previous camera is not finite", j);
  }
  if ((rc = check_device_present()) != RT_OK) return rc;
  return views_checks(c, q, v, pad, refit);
}

// alb: what the albedo channel sums (rt_render_aov_views_albedo; RT_ALBEDO_MATERIAL for rt_render_aov_views) — an unknown
// value is refused among the arguments, data the context does not hold last of all.  G: the surface the channel reads.
int aov_views_checks(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_aov* out, rt_params* q, rtbvh::Padding* pad, bool* refit,
                     uint32_t alb, SurfaceGen* G) {
  if (!c || !p || !v || !v->cameras || !out) return fail(RT_ERR_INVALID, "ctx/params/views/cameras/aov is null");
  if (any_set(out->reserved, 4)) return fail(RT_ERR_INVALID, "reserved words must be zero");
  if (alb > RT_ALBEDO_TEXTURES) return fail(RT_ERR_INVALID, "albedo %u is none of RT_ALBEDO_MATERIAL, RT_ALBEDO_COLORS, RT_ALBEDO_TEXTURES", alb);
  const int rc = views_pass_checks(c, p, v, nullptr, q, pad, refit);
  return rc != RT_OK ? rc : resident_surface(c, albedo_surface(alb), G);
}

int motion_views_checks(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_motion_prev_views* prev, const rt_motion* out,
                        rt_params* q, rtbvh::Padding* pad, bool* refit) {
  if (!c || !p || !v || !v->cameras || !prev || !out) return fail(RT_ERR_INVALID, "ctx/params/views/cameras/prev/out is null");
  if (any_set(prev->reserved, 6) || any_set(out->reserved, 4)) return fail(RT_ERR_INVALID, "reserved words must be zero");
  return views_pass_checks(c, p, v, prev->cameras, q, pad, refit);
}

// What the device forms do between their checks and their launch: the refit a farther view asks for (as
// rt_render_views_device: the context keeps the padding, not the camera), last frame's cameras when the motion pass runs
// (prev: null for the AOV pass), and the view records.
int stage_views(rt_ctx* c, const rt_params* q, const rt_views* v, const rt_motion_prev_views* prev, const rtbvh::Padding& pad, bool refit,
                hipStream_t s) {
  int rc;
  if (refit && (rc = refit_to_padding(c, pad, s)) != RT_OK) return rc;
  return upload_views(c, q, v, prev ? (prev->cameras ? prev->cameras : v->cameras) : nullptr, s);
}

// rt_render_aov_views_device and rt_render_aov_views_albedo_device: the multi-view forms of aov_device, the albedo
// channel by `alb`
int aov_views_device(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_aov* out, void* stream, uint32_t alb) {
  rt_params q;
  rtbvh::Padding pad;
  bool refit = false;
  SurfaceGen G;
  int rc = aov_views_checks(c, p, v, out, &q, &pad, &refit, alb, &G);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = stage_views(c, &q, v, nullptr, pad, refit, s)) != RT_OK) return rc;
  const bool brute = q.accel == RT_ACCEL_BRUTE;
  const rtk::AovArgs A = aov_args(q, *out);
  const hipError_t he = rtk::launch_aov(brute, c->S, A, c->vwRecs.get(), v->n_views, G.gen, s);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "AOV launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

// ... and of aov_host
int aov_views_host(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_aov* out, uint32_t alb) {
  rt_params q;
  rtbvh::Padding pad;
  bool refit = false;
  SurfaceGen G;
  int rc = aov_views_checks(c, p, v, out, &q, &pad, &refit, alb, &G);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t all = rtk::view_slice(v->n_views, q.width, q.height, 1);
  Staging st;
  rt_aov d = {};
  d.albedo = st.out(out->albedo, 3 * all), d.normal = st.out(out->normal, 3 * all), d.position = st.out(out->position, 3 * all);
  d.depth = st.out(out->depth, all), d.hits = st.out(out->hits, all), d.mesh = st.out(out->mesh, all), d.tri = st.out(out->tri, all);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = aov_views_device(c, &q, v, &d, nullptr, alb)) != RT_OK) return rc;
  return st.download();
}

// Everything rt_denoise_batch checks, the context last (it exists only where a device does).
int denoise_batch_checks(const rt_ctx* c, const rt_denoise_params* d, uint32_t nFrames, const void* rgb, const rt_aov* aov, const void* out) {
  int rc = denoise_checks(c, d, rgb, aov, out);
  if (rc != RT_OK) return rc;
  if (any_set(d->reserved, 6) || any_set(aov->reserved, 4)) return fail(RT_ERR_INVALID, "reserved words must be zero");
  if ((rc = denoise_param_checks(d)) != RT_OK) return rc;
  if (nFrames == 0) return fail(RT_ERR_INVALID, "n_frames is 0");
  if ((uint64_t)nFrames * d->width * d->height >= (1ull << 31))
    return fail(RT_ERR_INVALID, "%u frames of %ux%u pixels: 2^31 pixels or more", nFrames, d->width, d->height);
  if ((rc = check_device_present()) != RT_OK) return rc;
  return check_not_broken(c);
}

}  // namespace

extern "C" {

int rt_render_aov_views_device(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_aov* out, void* stream) {
  return aov_views_device(c, p, v, out, stream, RT_ALBEDO_MATERIAL);
}
int rt_render_aov_views(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_aov* out) {
  return aov_views_host(c, p, v, out, RT_ALBEDO_MATERIAL);
}
int rt_render_aov_views_albedo_device(rt_ctx* c, const rt_params* p, const rt_views* v, uint32_t albedo, const rt_aov* out, void* stream) {
  return aov_views_device(c, p, v, out, stream, albedo);
}
int rt_render_aov_views_albedo(rt_ctx* c, const rt_params* p, const rt_views* v, uint32_t albedo, const rt_aov* out) {
  return aov_views_host(c, p, v, out, albedo);
}

int rt_render_motion_views_device(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_motion_prev_views* prev,
                                  const rt_motion* out, void* stream) {
  rt_params q;
  rtbvh::Padding pad;
  bool refit = false;
  int rc = motion_views_checks(c, p, v, prev, out, &q, &pad, &refit);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = stage_views(c, &q, v, prev, pad, refit, s)) != RT_OK) return rc;
  const rt_motion_prev one = {};  // (the launcher reads the cameras from the tables: only prevVpos matters below)
  const rtk::MotionArgs A = motion_args(c, q, &one, prev->vertex_pos, *out);
  const hipError_t he =
      rtk::launch_motion_views(q.accel == RT_ACCEL_BRUTE, c->S, A, c->vwRecs.get(), c->vwPrevCams.get(), v->n_views, s);
  if (he != hipSuccess) return fail(RT_ERR_HIP, "motion launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_render_motion_views(rt_ctx* c, const rt_params* p, const rt_views* v, const rt_motion_prev_views* prev, const rt_motion* out) {
  rt_params q;
  rtbvh::Padding pad;
  bool refit = false;
  int rc = motion_views_checks(c, p, v, prev, out, &q, &pad, &refit);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t all = rtk::view_slice(v->n_views, q.width, q.height, 1);
  rt_motion_prev_views dp = *prev;
  if ((rc = upload_prev_positions(c, prev->vertex_pos, &dp.vertex_pos)) != RT_OK) return rc;
  Staging st;
  rt_motion d = {};
  d.motion = st.out(out->motion, 2 * all), d.position = st.out(out->position, 3 * all);
  d.prev_position = st.out(out->prev_position, 3 * all), d.mesh = st.out(out->mesh, all);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = rt_render_motion_views_device(c, &q, v, &dp, &d, nullptr)) != RT_OK) return rc;
  return st.download();
}

int rt_denoise_batch_device(rt_ctx* c, const rt_denoise_params* d, uint32_t n_frames, const void* d_rgb, const rt_aov* aov, void* d_out,
                            void* stream) {
  int rc = denoise_batch_checks(c, d, n_frames, d_rgb, aov, d_out);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_filter_scratch(c, n_frames * rtk::filter_scratch(d->width, d->height))) != RT_OK) return rc;
  const hipError_t he = rtk::launch_denoise_batch(c->S, denoise_args(c, d, d_rgb, aov, d_out), n_frames, static_cast<hipStream_t>(stream));
  if (he != hipSuccess) return fail(RT_ERR_HIP, "denoise launch failed: %s", hipGetErrorString(he));
  return RT_OK;
}

int rt_denoise_batch(rt_ctx* c, const rt_denoise_params* d, uint32_t n_frames, const float* rgb, const rt_aov* aov, float* out) {
  int rc = denoise_batch_checks(c, d, n_frames, rgb, aov, out);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t all = rtk::view_slice(n_frames, d->width, d->height, 1);
  Staging st;
  const float* dRgb = st.in(rgb, 3 * all);
  rt_aov da = {};
  da.albedo = st.in(aov->albedo, 3 * all), da.normal = st.in(aov->normal, 3 * all), da.position = st.in(aov->position, 3 * all);
  da.hits = st.in(aov->hits, all);
  float* dOut = st.out(out, 3 * all);
  if (st.rc != RT_OK) return st.rc;
  if ((rc = rt_denoise_batch_device(c, d, n_frames, dRgb, &da, dOut, nullptr)) != RT_OK) return rc;
  return st.download();
}

}  // extern "C"
