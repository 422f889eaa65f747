/* rt_amd.h — C ABI of the MI355X (gfx950) path-tracing hot path.
 *
 * The reference (nikitakaraevv/ray-tracing-engine) has no plugin/FFI seam; the
 * natural boundary is `void Renderer::render(Image&)` (reference
 * source/Renderer.h:36, source/Renderer.cpp:203-272), called once from main
 * (source/Main.cpp:224).  Everything below is what a `Renderer::render` that
 * dispatches to the GPU binds to (see INTEGRATION.md for the host-side stub):
 *
 *   rt_create / rt_destroy      <- Renderer::Renderer(Scene&, ...) deep copy of the
 *                                  scene (Renderer.cpp:15-31): flattened snapshot
 *   rt_set_photons              <- PhotonMap + kdtree built in render()
 *                                  (Renderer.cpp:209-213; kdtree.h:60-69 order)
 *   rt_emit_photons             <- PhotonMap::PhotonMap (PhotonMap.h:14-50,92-155)
 *   rt_update                   <- a scene changed between frames (Main.cpp:88-99 rotationY, a moving
 *                                  camera or light): the resident context follows it, tree refit
 *   rt_update_transforms        <- the same with one matrix per mesh (Main.cpp:88-99): the device transforms a
 *                                  resident rest pose, nothing per vertex crosses the bus
 *   rt_set_skin / rt_update_skin <- (no counterpart) deforming meshes: the device blends the rest pose under up to four
 *                                  bones per vertex (linear blend skinning), one record per bone crosses the bus
 *   rt_bvh_quality_get / rt_rebuild <- (no counterpart) the surface-area cost of the refit tree against the tree as built,
 *                                  and the tree built again in place from the resident arrays when it has degraded
 *   rt_render                   <- the spp/y/x loop + resolve (Renderer.cpp:219-271)
 *   rt_render_device/_resolve_device : same, on caller-owned DEVICE buffers and a
 *                                  caller stream (multi-GPU tile sharding, bench)
 *   rt_render_aov / rt_denoise  <- (no counterpart) first-hit AOVs of a frame's primary rays, and the a-trous
 *                                  filter of a low-spp frame guided by them (+ _device forms)
 *   rt_render_motion / rt_temporal_accumulate <- (no counterpart) where each pixel's surface point was last frame, and
 *                                  the previous frame's history reprojected there and blended (+ _device forms)
 *   rt_render_adaptive          <- (no counterpart) passes of spp samples over the pixel granules whose estimate has
 *                                  not yet converged (+ _device form)
 *   rt_render_views             <- (no counterpart) the frames of many cameras of one resident scene in one launch
 *                                  (+ _device form)
 *   rt_render_ao                <- (no counterpart) ambient occlusion and bent normals at the frame's first hit
 *                                  (+ _device form)
 *   rt_render_rays              <- (no counterpart) the integrator over ray batches of the caller's: probes, baking,
 *                                  cameras of any kind (+ _device form)
 *   rt_render_lens              <- (no counterpart) the frame through a thin lens: depth of field, one lens sample
 *                                  per pixel sample (+ _device form)
 *   rt_render_shutter           <- (no counterpart) the frame under an open shutter while the camera moves: one time
 *                                  per pixel sample, with or without the lens (+ _device form)
 *   rt_render_views_shutter / rt_render_adaptive_shutter <- (no counterpart) that shutter per view of a multi-view
 *                                  frame, and in the passes of an adaptive frame (+ _device forms)
 *   rt_render_lights            <- (no counterpart) the frame split by light group: one accumulator per group of
 *                                  lights for the rays of one frame (+ _device form)
 *   rt_render_pick              <- (no counterpart) sampled direct lighting for scenes of many lights: m <= 3 lights per
 *                                  sample, picked by importance and weighted by 1 / (m p) (+ _device form)
 *   rt_set_vertex_colors / rt_render_colors / rt_render_aov_colors <- (no counterpart) per-vertex albedo: the frame and
 *                                  its first-hit AOVs with the colour interpolated at every shaded vertex (+ _device forms)
 *   rt_set_textures / rt_render_textured / rt_render_aov_textured <- (no counterpart) image-textured albedo: the frame and
 *                                  its first-hit AOVs with the hit mesh's texture sampled at every shaded vertex (+ _device forms)
 *   rt_set_material_maps / rt_render_material <- (no counterpart) textured kd, alpha and f0: the textured frame with the
 *                                  whole material of every shaded vertex sampled from the resident textures (+ _device form)
 *   rt_set_normal_maps / rt_render_normal_mapped <- (no counterpart) tangent-space normal maps: that frame with the shading
 *                                  normal of every shaded vertex turned by a texture of the resident set (+ _device form)
 *   rt_render_aov_views / rt_render_motion_views / rt_denoise_batch <- (no counterpart) the AOVs, motion vectors and
 *                                  denoised frames of those views, one launch each (+ _device forms)
 *   rt_trace                    <- RayTracer::rayTrace (RayTracer.h:27-53) test hook
 *   rt_knn / rt_knn_wide        <- kdtree::knearest (kdtree.h:180-195) test hooks
 *
 * Conventions: plain C, int status (0 = RT_OK), caller-owned buffers, no C++
 * types or exceptions across the boundary, one host thread per context and ONE LAUNCH IN
 * FLIGHT per context: a context owns one work-queue head, one counter block, one
 * wavefront state block and the scratch of its filters and passes, so the calls on one
 * context must be ordered on one stream (or synchronised) — use one context per stream.  There
 * is NO CPU fallback: every compute entry point fails with RT_ERR_NO_DEVICE if
 * no gfx950 device is usable.
 *
 * Stream order of the `_device` forms (tests/test_gpu_stream_order.py issues every one of them on a
 * non-blocking stream that is still busy, back to back; rt_render_lens_device: tests/test_gpu_lens.py;
 * rt_render_shutter_device: tests/test_gpu_shutter.py):
 *   ASYNCHRONOUS — everything the call does is queued on `stream`, device inputs are read and outputs
 *   written in stream order, and the call returns without waiting for the stream:
 *     rt_render_device, rt_render_views_device, rt_render_rays_device, rt_render_shutter_device,
 *     rt_render_views_shutter_device (tests/test_gpu_views_shutter.py), rt_render_lights_device
 *     (tests/test_gpu_lights.py), rt_render_pick_device (tests/test_gpu_pick.py), rt_render_colors_device
 *     (tests/test_gpu_vcol.py), rt_render_textured_device (tests/test_gpu_tex.py), rt_render_material_device
 *     (tests/test_gpu_mat.py), rt_render_normal_mapped_device (tests/test_gpu_nmap.py) and
 *     rt_render_lens_device with stats == NULL;
 *     rt_resolve_device;
 *     rt_render_aov_device, rt_render_aov_colors_device, rt_render_aov_textured_device, rt_render_ao_device, rt_render_motion_device; rt_temporal_accumulate_device,
 *     rt_svgf_device, rt_denoise_device, rt_denoise_batch_device; rt_render_aov_views_device,
 *     rt_render_motion_views_device; rt_pack_owned_device, rt_unpack_owned_device; rt_trace_stream_device.
 *     Host arguments (params, cameras, seeds, previous cameras, a pick's importance array) are copied before the call
 *     returns.
 *     Two exceptions, neither of which changes a result: a call that needs MORE scratch than the context holds
 *     (another frame size, rank or sample-per-wave choice for the tile list; more views; a larger frame for the
 *     filters; a larger wavefront batch; more lights for a pick table) frees the old block, and hipFree waits for the
 *     device; and the fifth multi-view call in a row waits for the upload of the first (four pinned staging copies), as
 *     does the fifth rt_render_pick_device call for the table of the first.
 *   SYNCHRONISE `stream`, and only it, before they return, because the host reads a result back:
 *     rt_render_device, rt_render_views_device, rt_render_rays_device, rt_render_shutter_device,
 *     rt_render_views_shutter_device, rt_render_lights_device, rt_render_pick_device, rt_render_colors_device,
 *     rt_render_textured_device, rt_render_material_device, rt_render_normal_mapped_device,
 *     rt_render_lens_device with stats != NULL;
 *     rt_render_adaptive_device and rt_render_adaptive_shutter_device (every pass); rt_update_vertices_device,
 *     rt_update_transforms and rt_update_skin (twice);
 *     the four multi-view forms when a view lies far enough out to need a wider box padding (a refit).
 *   HOST forms (rt_render, rt_render_aov, rt_denoise, rt_update, rt_trace, rt_knn, rt_bvh_quality_get, rt_rebuild,
 *     the photon calls ...) run on the NULL stream and return when their result is in host memory.  The null
 *     stream does not wait for a non-blocking stream: a host form must not follow an unfinished asynchronous call on
 *     such a stream without a synchronisation of that stream.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 2
/* largest photon-map k (rt_params.k, rt_knn_wide): the k-slot heap of a wave lives in LDS */
#define RT_KNN_KMAX 256

enum {
  RT_OK = 0,
  RT_ERR_INVALID = 1,   /* bad argument / inconsistent scene            */
  RT_ERR_NO_DEVICE = 2, /* no usable HIP device (never falls back to CPU) */
  RT_ERR_HIP = 3,       /* a HIP runtime call failed                      */
  RT_ERR_UNSUPPORTED = 4,
  RT_ERR_STATE = 5      /* e.g. photon shading requested without photons  */
};

/* Material.h:62-64 (m_kd, m_alpha, m_albedo, m_F0) */
typedef struct rt_material {
  float kd, alpha;
  float albedo[3];
  float f0[3];
} rt_material;

/* LightSource.h:61-65; basis from the ctor (:19-33) computed by the host */
typedef struct rt_light {
  float position[3], color[3], vertical[3], horizontal[3], normal[3];
  float intensity, side, factor, ac, al, aq;
} rt_light;

/* Camera.h:34-40 (m_position, m_lowerLeftCorner, m_horizontal, m_vertical) */
typedef struct rt_camera {
  float position[3], lower_left[3], horizontal[3], vertical[3];
} rt_camera;

/* Flattened Scene (Scene.h:27-31, Mesh.h:136-141).  Triangles are listed in the
 * reference's (mesh, triangle) iteration order (RayTracer.h:32-35): that order
 * is the tie-break for equal hit distances. */
typedef struct rt_scene_desc {
  uint32_t n_meshes, n_vertices, n_triangles, n_lights;
  const float* vertex_pos;        /* [n_vertices][3], meshes concatenated           */
  const float* vertex_nrm;        /* [n_vertices][3]                                */
  const uint32_t* tri_vtx;        /* [n_triangles][3] GLOBAL vertex ids             */
  const uint32_t* mesh_tri_begin; /* [n_meshes+1] first triangle of each mesh       */
  const uint32_t* mesh_vtx_begin; /* [n_meshes+1] first vertex of each mesh         */
  const rt_material* materials;   /* [n_meshes]                                     */
  const rt_light* lights;         /* [n_lights]                                     */
  rt_camera camera;
} rt_scene_desc;

enum { RT_MODE_RAY = 0, RT_MODE_PATH = 1 };   /* -m, Renderer.h:9-10            */
enum { RT_RNG_LEGACY = 0, RT_RNG_PIXEL = 1 }; /* legacy = global serial engine:
                                                 CPU oracle only, GPU refuses  */
enum { RT_ACCEL_BVH = 0, RT_ACCEL_BRUTE = 1 };
enum { RT_TRACE_CLOSEST = 0, RT_TRACE_ANY = 1 };

typedef struct rt_options {
  int32_t device;          /* HIP device ordinal                              */
  uint32_t bvh_leaf_max;   /* 0 = default (2), max 8                          */
  uint32_t bvh_builder;    /* RT_BVH_*; AUTO = the device builder for scenes of 8,192 triangles and
                              more (the same tree as the host builder's, 2-14 x sooner), the host
                              builder below (1-3 ms either way).  The environment variable
                              RT_BVH_GPU=1|2|3 forces DEVICE | HYBRID | HOST                        */
  uint32_t node_format;    /* RT_NODES_*: the node records the pooled render kernel and rt_trace
                              traverse.  AUTO picks per scene; the hits are the same either way  */
  uint32_t reserved[4];
} rt_options;
/* RT_BVH_HOST:   SAH on up to 16 host threads (binned above 4,096 triangles, exact sweeps below, size axis, rotations).
 * RT_BVH_DEVICE: the same split rules as kernels down to parts of <= 1,024 triangles, each part one exact SAH subtree (one
 *                workgroup), then the host's rotation passes and a pre-order numbering as kernels: the SAME tree as
 *                RT_BVH_HOST's (equal boxes and leaf sets on the four preset scenes: tests/treedigest.py), 1 M triangles
 *                in about 20 ms.
 * RT_BVH_HYBRID: the host builder's own top, stopped at the same parts; everything below as RT_BVH_DEVICE.                 */
enum { RT_BVH_AUTO = 0, RT_BVH_DEVICE = 1, RT_BVH_HYBRID = 2, RT_BVH_HOST = 3 };
/* RT_NODES_F16: 32-byte records, 12 binary16 box planes + 2 child refs (two 16-byte requests per visit).
 * RT_NODES_Q8:  16-byte records, 12 8-bit box planes in the frame of the record's 16-KiB block + one
 *               packed child word (ONE request per visit), nodes and triangle records in one array.   */
enum { RT_NODES_AUTO = 0, RT_NODES_F16 = 1, RT_NODES_Q8 = 2 };

typedef struct rt_params {
  uint32_t width, height;
  uint32_t spp;        /* -N: samples per pixel of the whole frame             */
  uint32_t mode;       /* RT_MODE_*                                            */
  uint32_t max_depth;  /* 3 in the reference (Renderer.cpp:245,248)            */
  uint32_t seed;       /* stream key, include/rt_pixelmode.h                   */
  uint32_t rng_mode;   /* RT_RNG_PIXEL                                         */
  uint32_t accel;      /* RT_ACCEL_*                                           */
  uint32_t use_photons;       /* 1: photon-map shading (Renderer.cpp:63-104)   */
  uint32_t k;                 /* -k: 1..RT_KNN_KMAX (<= photons)               */
  uint32_t photons_requested; /* -p: density denominator (Renderer.cpp:99)     */
  uint32_t spp_begin, spp_count; /* sample sub-range of this call; 0,0 = all   */
  uint32_t rank, world;       /* tile ownership: this call renders the 8x8-pixel
                                 tiles t with owner(t) == rank                 */
  uint32_t tile;              /* ownership granule in pixels (multiple of 8)   */
  uint32_t collect_stats;     /* 1: also count BVH nodes / triangle tests      */
  uint32_t reserved[7];       /* [0]: samples of a pixel one wave integrates side by
                                 side (power of two <= 64; 0 = chosen from the grid
                                 size).  [1] bit 0: shade vertices sequentially instead
                                 of through the wave's ray pool.  [2] bit 0: the queue-
                                 based (wavefront) integrator: path state and ray queues
                                 in HBM, one trace launch per path depth.  None of them
                                 changes the result, only the schedule.               */
} rt_params;

typedef struct rt_stats {
  uint64_t samples;        /* pixel-samples integrated                          */
  uint64_t rays_closest;   /* closest-hit casts (primary + bounce)              */
  uint64_t rays_shadow;    /* any-hit casts                                     */
  uint64_t knn_queries;
  uint64_t nodes_visited;  /* BVH node records fetched (collect_stats)          */
  uint64_t tris_tested;    /* 48-B triangle records tested (collect_stats)      */
  uint64_t kd_visited;     /* kd-tree nodes visited (collect_stats)             */
  uint64_t frame_fetches;  /* RT_NODES_Q8: block frames fetched (collect_stats) */
  double kernel_ms;        /* device time of the integrate kernel(s)            */
  uint64_t reserved[4];
} rt_stats;

typedef struct rt_ray {
  float origin[3], direction[3];
} rt_ray;

/* What RayTracer::rayTrace hands back (RayTracer.h:27-53) + the triangle id. */
typedef struct rt_hit {
  int32_t hit;         /* 0/1                                                   */
  uint32_t mesh;       /* meshIndex                                             */
  uint32_t tri;        /* triangle index inside the mesh                        */
  uint32_t vtx[3];     /* `triangle`: vertex ids LOCAL to the mesh              */
  float u, v, d;
} rt_hit;

typedef struct rt_bvh_info {
  uint32_t n_nodes, n_tri_records, max_depth, leaf_max;
  float pad;           /* absolute box padding used                             */
  float build_ms;      /* wall time of the build inside rt_create                */
  uint32_t builder;    /* RT_BVH_HOST / RT_BVH_DEVICE / RT_BVH_HYBRID            */
  uint32_t node_format;  /* RT_NODES_F16 / RT_NODES_Q8: what the pooled render kernel traverses */
  uint32_t flags;        /* RT_BVH_FLAG_*                                                         */
} rt_bvh_info;

/* SHORT_RECIP: the render instances take 1 / det and 1 / length in the three- / five-instruction forms that are
 * bit-identical to the IEEE operations inside the operand bounds rt_create checked (else they divide);
 * RECIP_CHECK_FAILED: this device's own check of those forms (2^25 inputs at its first rt_create) disagreed with
 * its division / sqrtf, so its contexts divide.  Same images either way.                                         */
enum { RT_BVH_FLAG_SHORT_RECIP = 1, RT_BVH_FLAG_RECIP_CHECK_FAILED = 2 };

typedef struct rt_ctx rt_ctx;

int rt_abi_version(void);
const char* rt_last_error(void);

/* Uploads the scene and builds its BVH.  RT_ERR_INVALID: null arrays / empty scene;
 * RT_ERR_UNSUPPORTED: 2^25 triangles or more (node and leaf refs are 31-bit byte offsets). */
int rt_create(const rt_scene_desc* scene, const rt_options* opt, rt_ctx** out);
void rt_destroy(rt_ctx* ctx);

/* ---- updating a resident scene (animation) --------------------------------------------------------------------------
 * After a successful update the context is what rt_create would make of the updated description, except for the tree's
 * TOPOLOGY, which stays: the same leaves, child refs and numbering, with every box recomputed from the new positions
 * (a refit).  The hits are exact on any tree whose boxes hold their padded triangles, so every frame is the frame of the
 * updated scene, bit for bit; only its speed depends on how far the geometry moved from the tree's (rt_create again when
 * that matters).  The box padding, the origin bound of rt_trace, the binary16 plane scale and the choice of the short
 * reciprocal forms (rt_bvh_info.pad / .flags) follow the updated description by rt_create's own rules.
 * Boxes are refit when positions are given or when the padding or the plane scale changed (a camera or a light moving
 * outwards can change the padding); a camera-only update that changes neither only moves the camera.
 * Any update that gives positions, normals, lights or materials releases the photon map: photon frames return
 * RT_ERR_STATE until rt_set_photons / rt_build_photon_map runs again.  A camera-only update keeps it.
 * Validation comes first and a rejected update leaves the context as it was: RT_ERR_INVALID for a null context or
 * update, lights NULL with n_lights > 0, or a non-finite position a triangle references ("non-finite", as rt_create);
 * RT_ERR_UNSUPPORTED for RT_NODES_Q8 contexts.  A HIP failure once the context has started to change leaves it refusing
 * launches (RT_ERR_STATE): destroy it.  An update is a launch: it must not overlap another launch on the context. */
typedef struct rt_scene_update {
  const float* vertex_pos;        /* [n_vertices][3] or NULL = unchanged (same count, same tri_vtx as rt_create's)   */
  const float* vertex_nrm;        /* [n_vertices][3] or NULL = unchanged                                           */
  const rt_camera* camera;        /* or NULL = unchanged                                                           */
  const rt_light* lights;         /* [n_lights] or NULL = unchanged; n_lights may differ from rt_create's          */
  uint32_t n_lights;
  const rt_material* materials;   /* [n_meshes] or NULL = unchanged                                                */
  uint32_t reserved[6];           /* zero                                                                          */
} rt_scene_update;

typedef struct rt_update_report {
  uint32_t refitted;        /* 1: boxes (and, with positions, triangle records) were recomputed           */
  uint32_t photons_dropped; /* 1: the context's photon map was released                                   */
  double refit_ms;          /* device time of the refit kernels (HIP events), 0 if none ran              */
  double total_ms;          /* wall time of the call                                                      */
  uint64_t reserved[4];
} rt_update_report;

int rt_update(rt_ctx* ctx, const rt_scene_update* u, rt_update_report* rep /* may be NULL */);
/* rt_update with positions / normals already in DEVICE memory (e.g. a torch tensor) on the context's device, ordered on
 * `stream` (a hipStream_t, may be NULL); either pointer may be NULL.  Synchronises once to read the magnitude summary
 * back (the finiteness check and the rules above need it) and once at the end. */
int rt_update_vertices_device(rt_ctx* ctx, const void* d_pos, const void* d_nrm, void* stream, rt_update_report* rep);

/* ---- animating rigid meshes by matrices (Main.cpp:88-99: "mesh 3 is now at this matrix") ---------------------------
 * rt_update whose positions and normals the DEVICE computes from a resident rest pose and one record per mesh: the host
 * sends 88 bytes per mesh instead of every vertex.
 * Rest pose: the context's positions and normals as the last call that was NOT rt_update_transforms left them — rt_create,
 * or an rt_update / rt_update_vertices_device that gave positions or normals (such a call makes the live arrays, both of
 * them, the new rest pose).  Transforms are absolute, from the rest pose, never cumulative: frame 100 carries no rounding
 * of frames 1-99, and the same records give the same bits whatever came between.
 * Per vertex of mesh j, rest position (x, y, z) and rest normal (a, b, c), all in float32, in this order, nothing fused:
 *   X'_i = ((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3]        N'_i = (n[i][0] a + n[i][1] b) + n[i][2] c
 * — the association of `dot` in the reference's Vec3.h, so m = n = rotationY's rows reproduces rotationY.  Normals are not
 * renormalised: n is the caller's normal matrix (identity = "normals are left as loaded").  An RT_XF_STATIC mesh keeps
 * its rest arrays bit for bit and its m and n are not read.  An identity matrix is NOT RT_XF_STATIC: -0 + 0 = +0, so a
 * rest coordinate of -0 comes out as +0.
 * After a successful call the context is, bit for bit, what rt_update with vertex_pos / vertex_nrm = those arrays and the
 * same camera and lights would leave (tree, rt_bvh_info, every frame and pass, the photon map released, the report); the
 * rules above apply through the same code.
 * Validation comes first and a rejected call leaves the context and d_prev_pos untouched.  RT_ERR_INVALID: a null ctx, u
 * or transforms; non-zero reserved words; unknown flag bits, or a non-finite entry of m or n of a mesh that is not
 * RT_XF_STATIC (rt_last_error names the mesh); lights NULL with n_lights > 0; n_meshes different from the context's; a
 * transformed position a triangle references coming out non-finite ("non-finite vertex position", as rt_update).
 * RT_ERR_UNSUPPORTED: RT_NODES_Q8 contexts.  RT_ERR_STATE: a context that refuses launches.
 * Ordered on `stream` (a hipStream_t, may be NULL); synchronises it as rt_update_vertices_device does, once for the
 * magnitude summary and once at the end. */
enum { RT_XF_STATIC = 1 };   /* flags bit 0: this mesh keeps its rest arrays, bits copied verbatim; m and n ignored */
typedef struct rt_mesh_transform {
  float m[3][4];       /* positions: row i = (m[i][0], m[i][1], m[i][2] | m[i][3])                                  */
  float n[3][3];       /* normals: the caller's normal matrix                                                       */
  uint32_t flags;      /* RT_XF_*; other bits zero                                                                  */
} rt_mesh_transform;
typedef struct rt_transform_update {
  const rt_mesh_transform* transforms;  /* [n_meshes], HOST memory, required                                       */
  uint32_t n_meshes;                    /* must equal the context's                                                */
  uint32_t n_lights;
  const rt_camera* camera;              /* or NULL = unchanged, as rt_scene_update                                 */
  const rt_light* lights;               /* [n_lights] or NULL = unchanged                                          */
  void* d_prev_pos;                     /* DEVICE [n_vertices][3] or NULL: receives the context's positions as they
                                           were BEFORE this call, ordered on `stream` (the prev->vertex_pos of
                                           rt_render_motion_device)                                                */
  uint32_t reserved[6];                 /* zero                                                                    */
} rt_transform_update;
int rt_update_transforms(rt_ctx* ctx, const rt_transform_update* u, void* stream, rt_update_report* rep /* may be NULL */);

/* ---- animating deforming meshes by bones: linear blend skinning (no counterpart) -----------------------
 * rt_update whose positions and normals the DEVICE blends from the resident rest pose, a resident skin — four bone
 * indices and four weights per vertex, sent once — and one rt_mesh_transform record per BONE: a frame sends 88 bytes per
 * bone instead of every vertex.
 *
 * rt_set_skin makes a skin resident (replacing the one before), or releases it (skin == NULL).  It changes nothing else
 * in the context: the same frames before and after, the photon map and the rest pose kept.  The resident skin survives
 * every update and rt_rebuild (the vertex count of a context never changes) until rt_set_skin replaces or releases it
 * or rt_destroy runs.  A host form: it runs on the NULL stream and returns when the arrays are in device memory.
 * Validation comes first and a rejected call leaves the skin that was resident in force.  In this order — what the
 * arguments alone decide is answered before the context or a device is asked for —:
 *   RT_ERR_INVALID  a null ctx with skin == NULL (nothing to release from);
 *   RT_ERR_INVALID  bone or weight null; non-zero reserved words; n_bones outside 1..65536;
 *   RT_ERR_INVALID  vertex by vertex, in order: a non-finite weight (rt_last_error names the vertex), then an index
 *                   >= n_bones (it names the vertex and the slot) — the index of a zero-weight slot is validated too;
 *   RT_ERR_INVALID  a null ctx; n_vertices different from the context's;
 *   RT_ERR_UNSUPPORTED  RT_NODES_Q8 contexts;   RT_ERR_STATE  a context that refuses launches.
 *
 * rt_update_skin poses the rest pose of rt_update_transforms — the same arrays, the same lazy snapshot: the two calls
 * share it.  Poses are absolute, from the rest pose, never cumulative; a transforms call between two skin calls changes
 * nothing about the second; a call that gives vertex arrays makes the live arrays the new rest pose, as above.
 * Per vertex, rest position (x, y, z) and rest normal (a, b, c), all in float32, every product and sum rounded, nothing
 * fused: X' = N' = (+0, +0, +0), then for each slot k = 0..3 IN SLOT ORDER whose weight[k] != 0 (a zero of either sign is
 * skipped and its bone's record is not read), with R = bones[bone[k]] and w = weight[k]:
 *   P_i = ((R.m[i][0] x + R.m[i][1] y) + R.m[i][2] z) + R.m[i][3]      Q_i = (R.n[i][0] a + R.n[i][1] b) + R.n[i][2] c
 *   X'_i = X'_i + (w P_i)                                              N'_i = N'_i + (w Q_i)
 * — P and Q are rt_update_transforms' expression, unchanged.  Normals are not renormalised (the shader normalises the
 * interpolated normal).  A vertex whose four weights are all zero keeps its rest arrays bit for bit, -0 included: the
 * analogue of RT_XF_STATIC.  A vertex with the single weight 1 is NOT that: +0 + (1 P) turns a P of -0 into +0.
 * After a successful call the context is, bit for bit, what rt_update with vertex_pos / vertex_nrm = those arrays and the
 * same camera and lights would leave (tree, rt_bvh_info, every frame and pass, the photon map released, the report).
 * Validation comes first and a rejected call leaves the context and d_prev_pos untouched.  In this order:
 *   RT_ERR_INVALID  a null u or bones; non-zero reserved words;
 *   RT_ERR_INVALID  bone by bone, in order: non-zero flags, then a non-finite entry of m or n (rt_last_error names the
 *                   bone);
 *   RT_ERR_INVALID  lights NULL with n_lights > 0;
 *   RT_ERR_INVALID  a null ctx;   RT_ERR_STATE  no resident skin;   RT_ERR_INVALID  n_bones different from the skin's;
 *   RT_ERR_UNSUPPORTED  RT_NODES_Q8 contexts;   RT_ERR_STATE  a context that refuses launches;
 *   RT_ERR_INVALID  a blended position a triangle references coming out non-finite ("non-finite vertex position").
 * Ordered on `stream` (a hipStream_t, may be NULL) and synchronises it as rt_update_transforms does, twice. */
#define RT_SKIN_INFLUENCES 4
typedef struct rt_skin {
  uint32_t n_vertices;    /* must equal the context's                                                               */
  uint32_t n_bones;       /* 1 .. 65536                                                                             */
  const uint16_t* bone;   /* [n_vertices][4], HOST memory: the bone index of each slot, all of them < n_bones       */
  const float* weight;    /* [n_vertices][4], HOST memory: the weight of each slot, finite; 0 = the slot is unused  */
  uint32_t reserved[6];   /* zero                                                                                   */
} rt_skin;
int rt_set_skin(rt_ctx* ctx, const rt_skin* skin /* NULL: release the resident skin */);

typedef struct rt_skin_update {
  const rt_mesh_transform* bones;  /* [n_bones], HOST memory, required: m for positions, n for normals; flags 0    */
  uint32_t n_bones;                /* must equal the resident skin's                                               */
  uint32_t n_lights;
  const rt_camera* camera;         /* or NULL = unchanged, as rt_transform_update                                  */
  const rt_light* lights;          /* [n_lights] or NULL = unchanged                                               */
  void* d_prev_pos;                /* DEVICE [n_vertices][3] or NULL, as rt_transform_update                       */
  uint32_t reserved[6];            /* zero                                                                         */
} rt_skin_update;
int rt_update_skin(rt_ctx* ctx, const rt_skin_update* u, void* stream, rt_update_report* rep /* may be NULL */);

/* ---- rebuilding a refit tree ----------------------------------------------------------------------------
 * A refit keeps the topology rt_create built, so over a long animation the tree drifts from the geometry.  The two calls
 * below measure that and undo it without rt_destroy + rt_create: nothing crosses the bus towards the device, and the
 * handle, the photon map, the rest pose of rt_update_transforms, the resident skin and the profile events stay.
 *
 * rt_bvh_quality_get: the surface-area cost of the resident tree, one device pass over its float node records (the
 * rt_bvh_export form: node i has two slots k with a box lo, hi in float32 and a ref child[k]; ref >= 0 an inner node,
 * ref < 0 a leaf of cnt = ((~ref) & 7) + 1 triangle records).  With A(lo, hi) = dx dy + dy dz + dz dx in double from
 * the float planes (dx = (double)hi.x - lo.x, ...) — the area measure of rt_bvh_check_host's est2 — and
 * A_root = max(A(union of node 0's two slots), 1e-300):
 *   nodes = 1 + sum over inner slots of A / A_root        tris = sum over leaf slots of (cnt A) / A_root
 *   cost  = nodes + 1.5 tris                              (the weights of rt_bvh_tune's probe cost)
 * The sums are double sums of fixed shape (no floating-point atomics): two calls on the same tree return the same bits.
 * cost_built is the same measure of the tree as last BUILT (rt_create, rt_rebuild, an accepted rt_bvh_tune) on the boxes
 * it was built with, taken lazily: right before the first refit that follows a build (that rt_update* gains one pass over
 * the nodes), or at the first quality call if none has run yet; rt_create, rt_bvh_tune and the render paths do no work
 * for it.  ratio = cost / cost_built is 1.0 exactly on a tree never refit.
 * A PROXY, NOT AN ORACLE: the ratio compares the refit tree on today's geometry with the built tree on the build's
 * geometry (the ratio renderers commonly use to decide on a rebuild); it is not the cost of a fresh tree of today's
 * geometry, which only a build can give.  It is a launch like any other (one in flight per context) and synchronises.
 * RT_ERR_INVALID: a null ctx or out; RT_ERR_UNSUPPORTED: RT_NODES_Q8 contexts (as rt_update); RT_ERR_STATE: a context
 * that refuses launches. */
typedef struct rt_bvh_quality {
  double cost;          /* of the tree as it is now                                                         */
  double nodes, tris;   /* its two parts                                                                    */
  double cost_built;    /* the same measure of this topology before its first refit                         */
  double ratio;         /* cost / cost_built; 1.0 exactly on a tree never refit                             */
  uint32_t n_nodes;
  uint32_t refits;      /* refits (updates that recomputed the boxes) since the last build                  */
  uint64_t reserved[4];
} rt_bvh_quality;
int rt_bvh_quality_get(rt_ctx* ctx, rt_bvh_quality* out);

/* rt_rebuild: the tree built again from the context's resident arrays.  After a successful rebuild the tree, the triangle
 * records, rt_bvh_info (except build_ms) and every derived value — padding, origin bound, plane scale, depth cap, the
 * short-form vouching, the pool thresholds, the most-visited-first numbering of trees of at most 65,536 nodes — are what
 * rt_create would produce from the context's CURRENT description (live positions and normals, camera, lights, materials)
 * and the rt_options it was created with, under rt_create's builder rule (bvh_builder, RT_BVH_GPU, RT_BVH_AUTO_FROM, the
 * 16- and 1,024-triangle special cases): the same code builds both.  The refit depth table and any rt_bvh_tune result are
 * dropped; cost_built and refits start again.  Hits do not depend on the tree, so — unlike an update — a rebuild KEEPS
 * the photon map, the rest pose of rt_update_transforms, the resident skin, the profile events and the handle: every frame and pass is
 * bit-identical before and after.
 * The host passes of a build (validation, the size keys from the host's log2, the host builder for small scenes) read the
 * positions, vertex ids and mesh tables back for the duration of the call; the new tree is built into staging buffers
 * and swapped in only when everything has succeeded, so TWO TREES ARE RESIDENT during the call and a failure leaves the
 * context exactly as it was.  The call synchronises and takes no stream: it reads only the context's own arrays.
 * min_ratio: 0 = always rebuild; otherwise finite and >= 1: rebuild only if rt_bvh_quality_get's ratio >= min_ratio.
 * RT_ERR_INVALID: non-zero reserved words, min_ratio non-finite or in (0, 1) (checked first), a null ctx;
 * RT_ERR_UNSUPPORTED: RT_NODES_Q8 contexts; RT_ERR_STATE: a context that refuses launches. */
typedef struct rt_rebuild_params {
  float min_ratio;
  uint32_t reserved[7];   /* zero */
} rt_rebuild_params;
typedef struct rt_rebuild_report {
  uint32_t rebuilt;       /* 0: the ratio was below min_ratio, nothing changed                                        */
  uint32_t builder;       /* RT_BVH_* that ran (0 when nothing was rebuilt)                                           */
  double ratio_before;    /* rt_bvh_quality.ratio on entry (computed only when min_ratio > 0 or the report is asked for) */
  double cost_after;      /* cost of the new tree (== its cost_built); 0 when nothing was rebuilt                      */
  double build_ms;        /* the build: host plan + device build + renumbering (rt_bvh_info.build_ms)                 */
  double total_ms;        /* wall time of the call                                                                    */
  double readback_ms;     /* of total_ms: reading the arrays of the host passes back                                  */
  double plan_ms;         /* of build_ms: the host passes (validation + size keys, the hybrid top, or the host build)  */
  uint64_t reserved[4];
} rt_rebuild_report;
int rt_rebuild(rt_ctx* ctx, const rt_rebuild_params* p /* NULL = always */, rt_rebuild_report* rep /* may be NULL */);

/* Photon arrays already in the host-built kd-tree (median-implicit) order. */
int rt_set_photons(rt_ctx* ctx, const float* pos3, const float* dir3, uint32_t n);
/* Emit photons on the GPU (pixel RNG mode, one stream per emitted photon), in
 * emission order; out arrays sized n_requested.  *n_out = stored photons. */
int rt_emit_photons(rt_ctx* ctx, uint32_t n_requested, uint32_t seed, float* pos3,
                    float* dir3, float* weight, uint32_t* n_out);

/* The whole photon map on the device (Renderer.cpp:209-213: PhotonMap + kdtree built inside
 * render()): emission (the rt_emit_photons kernel), stable compaction of the stored
 * particles, and the kd-tree order — the reference's recursive std::nth_element
 * (kdtree.h:60-69) restated for the GPU so that the array order, ties included, is the
 * library's (csrc/kd_build.hip) — installed as the context's photon map.  Photons never
 * visit the host; ms_out (optional, [2]) = {emission + compaction, kd order} device ms. */
int rt_build_photon_map(rt_ctx* ctx, uint32_t n_requested, uint32_t seed, uint32_t* n_stored,
                        double* ms_out);
/* The context's photon map in tree order (inspection / PhotonMap::saveToPCD). */
int rt_get_photons(rt_ctx* ctx, float* pos3, float* dir3, float* weight, uint32_t cap,
                   uint32_t* n_out);
/* Test hook: the device kd order of n host-given positions; perm_out[i] = input index of
 * tree slot i.  depth_limit < 0: std::nth_element's 2*lg(n); >= 0 forces the heap-select
 * path early (parity of __heap_select itself). */
int rt_test_kd_order(int32_t device, const float* pos3, uint32_t n, int32_t depth_limit,
                     uint32_t* perm_out, double* ms_out);

/* Whole frame on host buffers: background_rgb / out_rgb are [h][w][3] floats.
 * accum_out (optional, [h][w][4]) receives {sum r,g,b, primary-hit count}. */
int rt_render(rt_ctx* ctx, const rt_params* p, const float* background_rgb,
              float* out_rgb, float* accum_out, rt_stats* stats);

/* Progressive form of rt_render (Renderer.cpp:261-269: an image after every pass):
 * integrates the sample range p->spp_begin/spp_count on top of the caller-held host
 * accumulator accum_io ([h][w][4], zero before the first range) and resolves the
 * running estimate of the first spp_begin+spp_count samples into out_rgb. */
int rt_render_passes(rt_ctx* ctx, const rt_params* p, const float* background_rgb, float* accum_io,
                     float* out_rgb, rt_stats* stats);

/* Accumulate this rank's tiles / sample range into d_accum ([h][w][4] floats in
 * DEVICE memory, caller-zeroed) on `stream` (a hipStream_t, may be NULL). */
int rt_render_device(rt_ctx* ctx, const rt_params* p, void* d_accum, void* stream,
                     rt_stats* stats);
/* Renderer.cpp:262-265 on device buffers: out = sum/N + bg*(N-count)/N */
int rt_resolve_device(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp,
                      const void* d_accum, const void* d_background_rgb,
                      void* d_out_rgb, void* stream);

/* ---- first-hit AOVs and the a-trous denoiser (DESIGN.md "AOVs and the a-trous denoiser") ---------------------------
 * rt_render_aov casts exactly the primary rays of the frame p describes — sample i of pixel (x, y) for i in the sample
 * range (spp_begin / spp_count, or 0..spp), from the same stream seed, jitter_sample(i, spp) and camera_ray — through the
 * context's tree (or the exhaustive loop for RT_ACCEL_BRUTE), so its hit is the frame's primary hit, and sums per pixel,
 * in float32 in sample order (as rt_render forms accum), what the frame's first vertex sees.  A miss adds nothing.  Sums,
 * not means: ranges chain, and the caller divides by hits.  Every pointer may be NULL (channel not wanted); the others
 * are overwritten.  mode, max_depth, use_photons, k and photons_requested do not affect the pass; world > 1 returns
 * RT_ERR_UNSUPPORTED (tile-sharded AOVs are out of scope); sizes and ranges are checked as rt_render checks them.
 * RT_NODES_Q8 contexts run the pass on their 32-byte records (resident for the other kernels): the same hits.          */
typedef struct rt_aov {
  float* albedo;     /* [h][w][3] sum over hit samples of the hit mesh's material albedo                          */
  float* normal;     /* [h][w][3] sum of the shading normal (Renderer.cpp:42)                                     */
  float* position;   /* [h][w][3] sum of the hit point (Renderer.cpp:43)                                          */
  float* depth;      /* [h][w]    sum of the hit distance t (rt_hit.d)                                            */
  uint32_t* hits;    /* [h][w]    samples whose primary ray hit (== the w channel of rt_render's accum)           */
  uint32_t* mesh;    /* [h][w]    mesh of sample spp_begin's primary hit, 0xffffffff = miss                       */
  uint32_t* tri;     /* [h][w]    triangle within that mesh,              0xffffffff = miss                       */
  uint32_t reserved[4];
} rt_aov;
int rt_render_aov(rt_ctx* ctx, const rt_params* p, const rt_aov* host_out);
/* The same into DEVICE buffers (e.g. torch tensors) on `stream` (a hipStream_t, may be NULL); no synchronisation. */
int rt_render_aov_device(rt_ctx* ctx, const rt_params* p, const rt_aov* device_out, void* stream);

/* The edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) guided by the AOVs, with albedo demodulation.
 * Guides a = albedo/hits, n = normal/hits, x = position/hits where hits > 0; a pixel with hits == 0 passes through
 * unchanged and weighs 0 as a tap.  Filtered: c = rgb / max(a, 1e-3); iteration i (from 0) has step s = 2^i, taps
 * q = p + s(dx, dy), dx, dy in -2..2 inside the image, weights h[dx] h[dy] exp(-|c_p-c_q|^2/sc_i^2)
 * exp(-|n_p-n_q|^2/sn^2) exp(-|x_p-x_q|^2/sx^2) with h = {1/16, 1/4, 3/8, 1/4, 1/16} and sc_i = sc 2^-i, output
 * sum(w c_q) / sum(w), the next iteration's input; the result times max(a, 1e-3).
 * Defaults (0): iterations 5, sigma_color 2, sigma_normal 0.5, sigma_position 2 % of the diagonal of the bounding box
 * of the vertices the context's triangles reference.  RT_ERR_INVALID: null arguments or guides, a size outside
 * 1..65535, iterations above 8, a negative or non-finite sigma.                                                       */
typedef struct rt_denoise_params {
  uint32_t width, height;
  uint32_t iterations;                             /* 0 = 5; at most 8                 */
  float sigma_color, sigma_normal, sigma_position; /* 0 = the defaults above           */
  uint32_t reserved[6];
} rt_denoise_params;
/* rgb: a resolved frame [h][w][3] (rt_render's out_rgb); aov: the SUMS of rt_render_aov for the same params (albedo,
 * normal, position, hits required); out: [h][w][3].  rgb may equal out. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* d, const float* rgb, const rt_aov* aov, float* out);
/* The same on DEVICE buffers, ordered on `stream` (may be NULL); no synchronisation.  A launch like any other: the
 * context's scratch serves one call at a time. */
int rt_denoise_device(rt_ctx* ctx, const rt_denoise_params* d, const void* d_rgb, const rt_aov* d_aov, void* d_out,
                      void* stream);

/* ---- ambient occlusion and bent normals at the first hit ---------------------------------------------
 * rt_render_ao casts rt_render_aov's primary rays — the same stream, jitter_sample, camera_ray and walk (or the exhaustive
 * loop for RT_ACCEL_BRUTE), so the same hits, shading normal n and point X — and at every hit n_rays occlusion rays.  Ray
 * j of sample i of pixel pix draws d = hemisphere_sample(n), the frame's own bounce distribution, from a stream of its
 * own: rt_stream_seed(seed, RT_STREAM_AO, pix, i * n_rays + j).  It starts at o = X + bias * d (per component in float32:
 * the product, then the sum) and is occluded iff a triangle passes the library's triangle test with t > 0 and, when
 * max_distance > 0, t < max_distance.  A direction with a non-finite component is not occluded: it is counted, and adds
 * nothing to bent.  A miss of the primary ray adds nothing.  unoccluded and hits are counts, so sample ranges chain
 * exactly (occluded = hits * n_rays - unoccluded); bent is a float32 sum per component in (sample, j) order.  mode,
 * max_depth, the photon fields and the wavefront bit do not affect the pass; RT_NODES_Q8 contexts walk their resident
 * 32-byte records, as rt_render_aov does.
 * RT_ERR_INVALID, before any device work and with nothing written: a null ctx, p, a or output struct; non-zero reserved
 * words; n_rays 0 or above RT_AO_MAX_RAYS; spp * n_rays >= 2^32; a negative or non-finite bias or max_distance;
 * rt_render_aov's size and range checks.  RT_ERR_UNSUPPORTED: world > 1, the legacy RNG.                             */
#define RT_AO_MAX_RAYS 256
typedef struct rt_ao_params {
  uint32_t n_rays;       /* occlusion rays per primary hit: 1..RT_AO_MAX_RAYS                          */
  float bias;            /* 0 = 1e-4f x the diagonal of the bounding box of the vertices the context's
                            triangles reference (rt_denoise's reduction, float32); else finite, > 0   */
  float max_distance;    /* 0 = unbounded; else finite, > 0, measured from the biased origin          */
  uint32_t reserved[5];  /* zero */
} rt_ao_params;
typedef struct rt_ao {   /* every pointer may be NULL; the others are overwritten                     */
  uint32_t* unoccluded;  /* [h][w]    occlusion rays that escaped, over the hit samples of the range   */
  uint32_t* hits;        /* [h][w]    == rt_aov.hits for the same params                               */
  float* bent;           /* [h][w][3] float32 sum of the escaped rays' directions                      */
  uint32_t reserved[4];  /* zero */
} rt_ao;
int rt_render_ao(rt_ctx* ctx, const rt_params* p, const rt_ao_params* a, const rt_ao* host_out);
/* The same into DEVICE buffers on `stream` (may be NULL); no synchronisation.  With the default bias the box is reduced
 * on the stream into a block the context owns: such calls run one at a time, as rt_denoise_device's do.                */
int rt_render_ao_device(rt_ctx* ctx, const rt_params* p, const rt_ao_params* a, const rt_ao* device_out, void* stream);

/* ---- the integrator over ray batches of the caller's -------------------------------------------------
 * rt_render_rays integrates p->mode / p->max_depth along n primary rays that the caller gives, where every other entry
 * point casts a pinhole camera's: light probes, lightmap or per-vertex baking, orthographic, fisheye or thin-lens
 * cameras, a batch a pipeline already holds in device memory.
 *
 * Row r of the accumulator is, bit for bit, what pixel (0, 0) of a frame that rt_render_device renders for p holds if
 * that frame's camera_ray returned origin o_r and direction unit3(d_r) for every sample, the frame's pixel index in the
 * RNG stream was stream_index[r] (r when stream_index is NULL), and its sample range was p's.  Sample i
 *   - seeds the engine with rt_stream_seed(p->seed, RT_STREAM_PIXEL, stream_index[r], i),
 *   - draws jitter_sample(engine, i, p->spp) and DISCARDS the result, so that the stream is then where the frame's is,
 *   - casts the primary ray (o_r, unit3(d_r)) — Vec3.h:170-178 in float32: the division and the square root, never the
 *     short forms,
 *   - integrates exactly as the frame does: the vertices, the light samples in light order, the hemisphere draw after
 *     every shaded vertex, c0 + (c1 + (c2 + 0)) and the clamp to [0, 1],
 *   - adds in float32, in sample order: rgb into .xyz, and 1 into .w when the primary ray hit.
 * Resolve a batch with rt_resolve_device(ctx, n, 1, spp, ...): an image n wide and 1 high.
 * Far origins: a primary ray whose origin has a component beyond the context's origin bound (rt_trace's rule) takes
 * the exhaustive loop over the triangles; its secondary rays start on surfaces and walk the tree.
 * Degenerate directions — unit3(d_r) has a non-finite component or is the null vector: a zero direction, a non-finite
 * one, or a finite one so long that its squared length overflows float32 — hit nothing.  The host form refuses them
 * (RT_ERR_INVALID, naming the ray); the device form, which cannot look, counts the ray as a primary miss: it adds nothing
 * and casts nothing.
 * p->width and p->height are ignored; every other field of p is checked as rt_render checks it.  RT_NODES_Q8 contexts
 * walk their resident 32-byte records, as rt_render_aov does.  The call changes nothing in the context: not the camera,
 * not the box padding.
 * stats: samples = n * (samples of the range); rays_closest, rays_shadow, kernel_ms and, with collect_stats,
 * nodes_visited and tris_tested as for a frame; an exhaustive primary cast counts one closest ray and every triangle.
 * Validation comes first and a rejected call writes nothing.  RT_ERR_INVALID: a null ctx, p, b or rays; n of 0 or of
 * 2^31 and more; non-zero reserved words; rt_render's checks of p; host form: neither out_rgb nor accum_out, out_rgb
 * without background_rgb, a non-finite origin, a degenerate direction; device form: a null d_accum.
 * RT_ERR_UNSUPPORTED: world > 1, use_photons, the wavefront integrator (reserved[2] bit 0), the legacy RNG.
 * The host form stages rays and indices in scratch the context owns: one call at a time.                               */
typedef struct rt_ray_batch {
  uint32_t n;                    /* 1 .. 2^31 - 1                                                          */
  uint32_t reserved0;            /* zero                                                                   */
  const rt_ray* rays;            /* [n]; host form: HOST memory, device form: DEVICE memory                */
  const uint32_t* stream_index;  /* [n] or NULL = r; the same memory space as rays                         */
  uint32_t reserved[6];          /* zero                                                                   */
} rt_ray_batch;
/* background_rgb [n][3] (required when out_rgb is given, as rt_render); out_rgb [n][3] or NULL; accum_out [n][4] or
 * NULL; stats may be NULL. */
int rt_render_rays(rt_ctx* ctx, const rt_params* p, const rt_ray_batch* b, const float* background_rgb, float* out_rgb,
                   float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [n][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain.  The host waits only to read stats back. */
int rt_render_rays_device(rt_ctx* ctx, const rt_params* p, const rt_ray_batch* b, void* d_accum, void* stream,
                          rt_stats* stats);

/* ---- the frame through a thin lens: depth of field ---------------------------------------------------
 * rt_render_lens renders the frame p describes as rt_render does, except that the primary ray of every SAMPLE leaves a
 * point of its own on a lens disc of radius `aperture` around the camera position and passes through the point where the
 * pinhole ray of that sample meets the plane of focus.  Points at focus_distance (measured along the optical axis, the
 * normal of the image plane) are sharp; everything else is blurred by the disc.
 *
 * Host-derived constants, computed once per call from the context's camera (pos, ll, H, V; float32 inputs):
 *   Hu = unit3(H), Vu = unit3(V) in float32 (Vec3.h:170-178: l = sqrt((x x + y y) + z z), inv = 1 / l, a inv);
 *   in float64, with cross and dot associated as the motion-vector section below defines them:
 *     c = ((ll + 0.5 H) + 0.5 V) - pos;  n = cross(H, V);  plane = |dot(c, n)| / sqrt(dot(n, n));
 *     fs = (float)(focus_distance / plane).
 * Sample i of pixel (x, y), pix = y * width + x:
 *   1. g is seeded with rt_stream_seed(seed, RT_STREAM_PIXEL, pix, i); jitter_sample(g, i, spp) gives (cu, cv) exactly
 *      as the frame forms them.
 *   2. aperture == 0: the ray is the frame's own camera_ray(cam, cu, cv).  No lens stream is drawn; fs is neither
 *      computed nor checked.
 *   3. aperture > 0, all in float32, nothing fused:
 *        q = ((ll + cu H) + cv V) - pos               (camera_ray's operand before unit3)
 *        F = pos + fs q                               (per component: the product, then the sum)
 *        e is seeded with rt_stream_seed(seed, RT_STREAM_LENS, pix, i); up to 32 times: lx = e.uniformF(-1, 1), then
 *        ly = e.uniformF(-1, 1); the first pair with lx lx + ly ly <= 1 is taken; if none is, lx = ly = 0
 *        o' = (pos + (aperture lx) Hu) + (aperture ly) Vu   (per component)
 *        the primary ray is (o', unit3(F - o')) with the division and the square root, never the short forms
 *        (rt_render_rays' rule).
 *   4. From the primary cast on the sample is the frame's, and g is where the frame's stream is (the lens draws came from
 *      e): the vertices, the light samples in light order, the hemisphere draw after every shaded vertex, c0 + (c1 +
 *      (c2 + 0)), the clamp, the float32 adds in sample order into .xyz and the hit count into .w.
 * Guarantees:
 *   - aperture == 0: accum, out and the ray counts are bit-identical to rt_render / rt_render_device for the same p.
 *   - aperture > 0: what sample i adds to pixel pix is, bit for bit, row pix of rt_render_rays for the ray (o', F - o')
 *     with stream_index = pix, spp_begin = i, spp_count = 1.
 *   - sample ranges, reserved[0] (lanes per pixel) and reserved[1] bit 0 (no pool) change the schedule, never the bits,
 *     at either aperture.
 * RT_NODES_Q8 contexts walk their resident 32-byte records, as rt_render_aov does.  The call changes nothing in the
 * context.  Stats are a frame's.  The frame runs on the one-wave-per-workgroup kernel family of rt_render (there are no
 * persistent lens instances).
 * Validation comes first and a rejected call writes nothing.  RT_ERR_INVALID: a null ctx, p or lens; host form: neither
 * out_rgb nor accum_out, or out_rgb without background_rgb; device form: a null d_accum; non-zero reserved words; an
 * unknown model; a negative or non-finite aperture; with aperture > 0 a non-finite or non-positive focus_distance, a
 * null H or V, or an fs that is not finite or not > 0; max_c |pos_c| + 2 aperture above the context's origin bound
 * (16 x the padding reference: the bound of rt_trace and rt_render_rays, inside which every lens origin walks the tree
 * as a row of rt_render_rays does); every check rt_render applies to p.  RT_ERR_UNSUPPORTED: world > 1, use_photons, the
 * wavefront integrator (reserved[2] bit 0), the legacy RNG.  The checks that read the camera follow the others, and a
 * context exists only where a device does.                                                                              */
enum { RT_LENS_THIN = 0 };
typedef struct rt_lens {
  uint32_t model;          /* RT_LENS_THIN; anything else RT_ERR_INVALID                               */
  float aperture;          /* lens RADIUS in scene units; 0 = pinhole; finite, >= 0                    */
  float focus_distance;    /* along the optical axis; finite, > 0; ignored when aperture == 0          */
  uint32_t reserved[5];    /* zero */
} rt_lens;
/* buffers as rt_render's */
int rt_render_lens(rt_ctx* ctx, const rt_params* p, const rt_lens* lens, const float* background_rgb, float* out_rgb,
                   float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain.  p and lens are copied before the call returns; the host waits only to read stats back. */
int rt_render_lens_device(rt_ctx* ctx, const rt_params* p, const rt_lens* lens, void* d_accum, void* stream,
                          rt_stats* stats);

/* ---- the frame under an open shutter: camera motion blur ----------------------------------------------
 * rt_render_shutter renders the frame p describes as rt_render does, except that every SAMPLE draws a time of its own in
 * the shutter interval and sees the camera of that time: the context's camera A when the move begins (time 0),
 * camera_close B when it ends (time 1), every one of the twelve components interpolated linearly between them.  With
 * aperture > 0 the thin lens of rt_render_lens sits on that moving camera.  Geometry does not move.
 *
 * Host-derived constants, computed once per call (A, B: twelve float32 components each, position, lower_left,
 * horizontal, vertical):
 *   D = B - A per component in float32;
 *   with aperture > 0: fs0 and fs1 by rt_render_lens' fs rule (the plane distance in float64, focus_distance over it
 *   rounded to float32) for A and for B, and dfs = fs1 - fs0 in float32.
 * Sample i of pixel (x, y), pix = y * width + x, all in float32, nothing fused:
 *   1. g is seeded with rt_stream_seed(seed, RT_STREAM_PIXEL, pix, i); jitter_sample(g, i, spp) gives (cu, cv) exactly
 *      as the frame forms them.
 *   2. e is seeded with rt_stream_seed(seed, RT_STREAM_SHUTTER, pix, i); t = e.uniformF(open, close), one draw
 *      (canonF() * (close - open) + open).
 *   3. C(t): every component c is A_c + (t * D_c), the product, then the sum; pos(t), ll(t), H(t), V(t) are its parts.
 *   4. aperture == 0: the ray is (pos(t), unit3(((ll(t) + cu H(t)) + cv V(t)) - pos(t))), with the division and the
 *      square root, never the short reciprocal forms (the operand bounds rt_create proved hold for A only).
 *   5. aperture > 0:
 *        Hu = unit3(H(t)), Vu = unit3(V(t)) (division and square root);  fs = fs0 + (t * dfs);
 *        then steps 3 and 4 of the rt_render_lens contract over C(t) with these Hu, Vu and fs: q, F, the lens point
 *        (lx, ly) from rt_stream_seed(seed, RT_STREAM_LENS, pix, i) as there, o' and the ray (o', unit3(F - o')).
 *   6. From the primary cast on the sample is the frame's, and g is where the frame's stream is.
 * Guarantees:
 *   - G1, rows: what sample i adds to pixel pix is, bit for bit, row pix of rt_render_rays for that sample's (o, F - o)
 *     — at aperture 0 (pos(t), ((ll(t) + cu H(t)) + cv V(t)) - pos(t)) — with stream_index = pix, spp_begin = i,
 *     spp_count = 1.
 *   - G2, still shutter: open == close == s and aperture == 0: accum, out and both ray counts are bit-identical to
 *     rt_render on a context whose camera rt_update set to C(s), C(s) computed by step 3.  This holds for cameras A, B
 *     with no -0 component (A_c + 0 * D_c turns a -0 into +0).
 *   - G3, lens at rest: open == close == 0 and aperture > 0: bit-identical to rt_render_lens with the same aperture and
 *     focus_distance on the same context (under the same condition on A).
 *   - G4, schedule: sample ranges, reserved[0] (lanes per pixel) and reserved[1] bit 0 (no pool) change the schedule,
 *     never the bits.
 * RT_NODES_Q8 contexts walk their resident 32-byte records.  The call changes nothing in the context.  Stats are a
 * frame's.  The frame runs on the one-wave-per-workgroup kernel family of rt_render (no persistent instances).
 * Validation comes first and a rejected call writes nothing; what the arguments alone decide is answered before the
 * device is asked for, and the checks that read the context's camera come last.  RT_ERR_INVALID: a null ctx, p or
 * shutter; host form: neither out_rgb nor accum_out, or out_rgb without background_rgb; device form: a null d_accum;
 * non-zero reserved words; a non-finite component of camera_close; open or close not finite or outside
 * 0 <= open <= close <= 1; a negative or non-finite aperture; with aperture > 0 a non-finite or non-positive
 * focus_distance; every check rt_render applies to p.  RT_ERR_UNSUPPORTED: world > 1, use_photons, the wavefront
 * integrator (reserved[2] bit 0), the legacy RNG.  Then, reading the camera, RT_ERR_INVALID: the origin bound: nextafterf(max_c max(|posA_c|, |posB_c|), +inf) + 2 aperture above the context's origin
 * bound (the interpolation may overshoot an end point by one rounding); an H or V that cannot be normalised at either
 * end, or that turns by 90 degrees or more — in float64, dot(H_A, H_B) <= 0 or dot(V_A, V_B) <= 0: an interpolated axis
 * could then vanish; with aperture > 0 an fs0 or fs1 that is not finite and > 0.                                        */
typedef struct rt_shutter {
  rt_camera camera_close;  /* the camera when the shutter closes; the context's camera is the one when it opens */
  float open, close;       /* the exposure, as fractions of the move: finite, 0 <= open <= close <= 1            */
  float aperture;          /* thin-lens radius, 0 = pinhole (rt_lens.aperture's rules)                           */
  float focus_distance;    /* as rt_lens; ignored when aperture == 0                                             */
  uint32_t reserved[4];    /* zero */
} rt_shutter;
/* buffers as rt_render's */
int rt_render_shutter(rt_ctx* ctx, const rt_params* p, const rt_shutter* shutter, const float* background_rgb,
                      float* out_rgb, float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain.  p and shutter are copied before the call returns; the host waits only to read stats back. */
int rt_render_shutter_device(rt_ctx* ctx, const rt_params* p, const rt_shutter* shutter, void* d_accum, void* stream,
                             rt_stats* stats);

/* ---- the frame split by light group: per-light frames from one launch ---------------------------------
 * rt_render_lights renders the frame p describes as rt_render does and leaves, instead of one accumulator, one per LIGHT
 * GROUP: slice g holds the frame with only the lights of masks[g] lit.  Every primary, bounce and shadow ray and every
 * random draw of the frame is made ONCE, whatever the number of groups: a light that is not lit still has its sample
 * drawn and its shadow ray cast (Renderer.cpp:52-54), so the groups differ only in which terms a vertex adds.
 *
 * Sample i of pixel (x, y), pix = y * width + x, all in float32, nothing fused:
 *   1. Up to the light loop of each vertex the sample is rt_render's, once for all groups: g seeded with
 *      rt_stream_seed(seed, RT_STREAM_PIXEL, pix, i), jitter_sample, camera_ray, the primary cast; at every vertex the
 *      light samples drawn in light order, one shadow ray per light, then (path mode, not after the last vertex traced)
 *      the hemisphere draw and the bounce cast.
 *   2. For group g the colour of a vertex is the sum of radiance_l * bsdf_l (the component-wise product rt_render adds)
 *      over the lights l with bit l of masks[g] set whose shadow ray found nothing, started from +0 and added in light
 *      order: color = color + radiance_l * bsdf_l.
 *   3. Per group the sample is c0 + (c1 + (c2 + 0)) over the (up to three) vertices' colours of that group, clamped to
 *      [0, 1] per component, and added in float32, in sample order, into .xyz of pixel pix of slice g; 1 is added into .w
 *      of pixel pix of EVERY slice when the primary ray hit.  .w is therefore the same in every slice.  A slice resolves
 *      with rt_resolve_device; the host form resolves every slice over the one background_rgb.
 * Guarantees, all bit for bit, on accumulator words and on both ray counts:
 *   - L1, slices: slice g is what rt_render_device leaves for the same p on a context whose lights outside masks[g] were
 *     given color = (0, 0, 0) by rt_update — PROVIDED no unoccluded term radiance_l * bsdf_l of such a light is non-finite
 *     on that context: the zeroed light's term must be 0 * x = +-0, which a NaN or infinite x (a non-finite bsdf_l or
 *     attenuation) does not give.  x + +-0 = x and +0 + -0 = +0 do the rest.
 *   - L2: a mask of all the context's lights gives rt_render's frame, unconditionally; n_groups == 1 with that mask also
 *     reproduces rt_render's stats (samples and both ray counts).
 *   - L3, the point of the call: samples, rays_closest and rays_shadow are ONE frame's, whatever n_groups is.
 *   - L4, schedule: sample ranges chain (every slice, as rt_render_device's accumulator); reserved[0] (lanes per pixel)
 *     and reserved[1] bit 0 (no pool) change the schedule, never the bits.
 * RT_NODES_Q8 contexts walk their resident 32-byte records, as rt_render_lens does.  The call changes nothing in the
 * context.  The frame runs on the one-wave-per-workgroup kernel family of rt_render (no persistent instances).
 * Validation comes first and a rejected call writes nothing; what the arguments alone decide is answered before the
 * device is asked for.  RT_ERR_INVALID: a null ctx, p or groups; n_groups 0 or above RT_LIGHT_GROUPS_MAX; non-zero
 * reserved words; a non-zero masks[g] with g >= n_groups; host form: neither out_rgb nor accum_out, or out_rgb without
 * background_rgb; device form: a null d_accum; every check rt_render applies to p.  RT_ERR_UNSUPPORTED: world > 1,
 * use_photons, the wavefront integrator (reserved[2] bit 0), the legacy RNG.  Then the device (RT_ERR_NO_DEVICE); then,
 * reading the context: RT_ERR_UNSUPPORTED for a context with more than 32 lights, RT_ERR_INVALID for a mask with a bit at
 * or above the context's n_lights (rt_last_error names the group and the mask).
 * Out of scope: unclamped per-group sums, more than RT_LIGHT_GROUPS_MAX groups per launch, groups combined with the lens,
 * the shutter, views or adaptive passes, photon frames.                                                                  */
#define RT_LIGHT_GROUPS_MAX 4
typedef struct rt_light_groups {
  uint32_t n_groups;                    /* 1..RT_LIGHT_GROUPS_MAX                                                     */
  uint32_t masks[RT_LIGHT_GROUPS_MAX];  /* bit l: light l is lit in this group.  Masks may overlap, may be 0, may be
                                           all lights; entries >= n_groups must be 0                                  */
  uint32_t reserved[3];                 /* zero */
} rt_light_groups;
/* out_rgb [G][h][w][3] or NULL, accum_out [G][h][w][4] or NULL, G = n_groups; background_rgb [h][w][3] */
int rt_render_lights(rt_ctx* ctx, const rt_params* p, const rt_light_groups* groups, const float* background_rgb,
                     float* out_rgb, float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [G][h][w][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain.  p and groups are copied before the call returns; the host waits only to read stats back
 * (stats == NULL: asynchronous; stats != NULL: synchronises `stream`, and only it). */
int rt_render_lights_device(rt_ctx* ctx, const rt_params* p, const rt_light_groups* groups, void* d_accum, void* stream,
                            rt_stats* stats);

/* ---- sampled direct lighting for scenes of many lights --------------------------------------------------
 * rt_render casts one shadow ray per light and vertex.  rt_render_pick renders the frame p describes with m = slots light
 * samples per path vertex instead: every SAMPLE picks m of the context's n lights by importance, all of its vertices
 * shade with those m, and each picked light is weighted by 1 / (m p_k).  A vertex then casts m <= RT_PICK_SLOTS_MAX shadow
 * rays whatever n is, so the frame runs through the wave-level vertex pool.
 *
 * The table, derived by the host once per call, in float64 unless said otherwise; L_k are the context's lights:
 *   - importance q_k: importance[k] where the caller gives the array; else the light's power proxy
 *     (double)intensity * (double)factor * (((double)color[0] + color[1]) + color[2]) * (double)side * (double)side, where a
 *     value that is not finite or not > 0 counts as 0; if every default q_k is 0, all q_k = 1.
 *   - Q = the sum of q_k in index order, p_k = q_k / Q, C_k = the running sum of p in index order; the thresholds are
 *     t_k = (float)C_k, and from the last k with q_k > 0 onwards t_k = 1.0f.
 *   - pick(u) = the smallest k with u < t_k.  It exists for every u in [0, 1); a light with q_k = 0 shares its threshold
 *     with its predecessor and is never picked.
 *   - w_k = (float)(1.0 / ((double)m * p_k)) for p_k > 0; the picked light L'_k is L_k with color[c] = w_k * color[c], one
 *     float32 product per component, computed on the host.  The kernels read L'_k from a device table of the call's own.
 * Sample i of pixel (x, y), pix = y * width + x, all in float32, nothing fused:
 *   1. e is seeded with rt_stream_seed(seed, RT_STREAM_PICK, pix, i); for slot j = 0 .. m - 1: u_j = e.canonF(), k_j =
 *      pick(u_j).  The picks belong to the SAMPLE: all of its vertices use the same m slots.
 *   2. From there the sample is rt_render's sample on the light list (L'_{k_0}, .., L'_{k_{m-1}}): g seeded with
 *      rt_stream_seed(seed, RT_STREAM_PIXEL, pix, i), jitter_sample, camera_ray, the primary cast; at every vertex the m
 *      light samples drawn from g in slot order (two engine calls each, whatever the light), one shadow ray per slot, the
 *      unoccluded terms added from +0 in slot order, then the hemisphere draw.
 *   3. The sample is c0 + (c1 + (c2 + 0)), clamped to [0, 1] per component, and added in float32 in sample order; .w
 *      counts the primary hit.
 * The estimator is unbiased BEFORE the clamp.  The per-sample clamp to [0, 1] bites more often with weights above 1, as
 * with any such sampler: a picked frame of a scene whose samples come near 1 is darker there than rt_render's.
 * Guarantees, all bit for bit, on accumulator words and on both ray counts:
 *   - P1: what sample i adds to pixel pix is what rt_render_device adds to that pixel for the same p with spp_begin = i,
 *     spp_count = 1 on a context of the same geometry whose light list is that sample's tuple (L'_{k_0}, .., L'_{k_{m-1}}).
 *   - P2: with n = 1 and m = 1 the frame and the stats are rt_render's (w = 1).
 *   - P3: .w, samples, rays_closest and rays_shadow do not depend on the picks (the main stream advances two calls per
 *     slot whatever the light): they are those of rt_render on the same geometry with any m lights.
 *   - P4, schedule: sample ranges chain; reserved[0] (lanes per pixel), reserved[1] bit 0 (no pool), collect_stats and
 *     RT_ACCEL_BRUTE change the schedule, never the bits.
 * RT_NODES_Q8 contexts walk their resident 32-byte records, as rt_render_lens does.  The call changes nothing in the
 * context.  The frame runs on the one-wave-per-workgroup kernel family of rt_render (no persistent instances), pooled
 * whatever n is.
 * Validation comes first and a rejected call writes nothing; what the arguments alone decide is answered before the
 * device is asked for.  RT_ERR_INVALID: a null ctx, p or pick; slots 0 or above RT_PICK_SLOTS_MAX; non-zero reserved
 * words; importance without n_importance, or the reverse; a negative or non-finite importance[k] (rt_last_error names
 * k); an all-zero importance; host form: neither out_rgb nor accum_out, or out_rgb without background_rgb; device form: a
 * null d_accum; every check rt_render applies to p.  RT_ERR_UNSUPPORTED: world > 1, use_photons, the wavefront integrator
 * (reserved[2] bit 0), the legacy RNG.  Then the device (RT_ERR_NO_DEVICE); then, reading the context, RT_ERR_INVALID
 * for a context without lights, an n_importance that is not the context's n_lights, and a weight w_k that is not finite
 * (rt_last_error names the numbers).  There is no cap on n beyond rt_create's.
 * Out of scope: picks combined with the lens, the shutter, views, adaptive passes, light groups or rt_render_rays;
 * position-dependent importance (light trees); per-vertex picks; photon frames; more than RT_PICK_SLOTS_MAX slots.        */
#define RT_PICK_SLOTS_MAX 3          /* == the vertex pool's light count: a picked frame always fits the pool          */
typedef struct rt_light_pick {
  uint32_t slots;            /* m: light samples per path vertex, 1..RT_PICK_SLOTS_MAX           */
  uint32_t n_importance;     /* 0, or the context's n_lights                                     */
  const float* importance;   /* [n_importance] HOST memory or NULL = the default above           */
  uint32_t reserved[5];      /* zero */
} rt_light_pick;
/* out_rgb [h][w][3] or NULL, accum_out [h][w][4] or NULL, background_rgb [h][w][3]: as rt_render's */
int rt_render_pick(rt_ctx* ctx, const rt_params* p, const rt_light_pick* pick, const float* background_rgb, float* out_rgb,
                   float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain.  p, pick and the importance array are copied, and the table is staged, before the call
 * returns: the caller may overwrite the array at once.  The host waits only to read stats back (stats == NULL:
 * asynchronous; stats != NULL: synchronises `stream`, and only it). */
int rt_render_pick_device(rt_ctx* ctx, const rt_params* p, const rt_light_pick* pick, void* d_accum, void* stream,
                          rt_stats* stats);

/* ---- per-vertex albedo -------------------------------------------------------------------------------
 * rt_material is indexed by mesh: every surface rt_render draws has one albedo per mesh.  rt_set_vertex_colors makes one
 * colour per vertex resident — rgb [n_vertices][3] floats, indexed by the global vertex id as the normals are — and
 * rt_render_colors renders rt_render's frame with ONE substitution at every shaded vertex: the material is the hit mesh's
 * with albedo replaced, per component, by
 *     c = (c0 + u * (c1 - c0)) + v * (c2 - c0)
 * where c0, c1, c2 are the colours of the triangle's three vertices in the order of its index triple and u, v are the hit's
 * barycentrics (the bits the normal is interpolated with).  Every difference, product and sum is rounded on its own to
 * float32, nothing fused.  This form, not w c0 + u c1 + v c2, is the definition: three equal colours give c0 exactly.
 * From c the vertex forms kdDiffuse = kd * (c / float(M_PI)), the two float32 operations rt_render applies to albedo; every
 * other field is the mesh's material.  The RNG streams, the jitter, every ray, the hit selection, both ray counts, the
 * per-sample clamp and the accumulation are rt_render's: colours never move a ray.
 * Guarantees, bit for bit on accumulator, image, samples and both ray counts, for colours that are not -0:
 *   - C1: if every vertex of every mesh carries its mesh's albedo, the frame is rt_render's.
 *   - C2: if the three vertices of every triangle carry one colour, the frame is rt_render's on the scene in which every
 *     triangle is a mesh of its own (in the same order), with that colour as albedo.
 *   - C3: sample ranges chain.
 *   - C4: reserved[0] (lanes per pixel), reserved[1] bit 0 (no pool), collect_stats, RT_ACCEL_BRUTE and the node format
 *     change the schedule, never the bits.
 * rt_set_vertex_colors copies rgb to the context's device (replacing the colours before); rgb == NULL releases them
 * (n_vertices is then not read).  It changes nothing any other entry point reads; the colours stay across every update,
 * refit and rt_rebuild (the vertex count of a context never changes) and go with rt_destroy.  It is a host form: it
 * returns when the copy is done; the array it replaces is freed once the launches that read it have run.
 *   RT_ERR_INVALID  a null rgb with a null ctx; a value that is not finite (rt_last_error names the first bad index); a
 *   null ctx; n_vertices different from the context's.  No range is imposed, as none is on rt_material.albedo.
 *   RT_ERR_STATE  a context that refuses launches (nothing is uploaded to it).
 * rt_render_colors / rt_render_colors_device take rt_render's / rt_render_device's arguments.  Validation comes first and
 * a rejected call writes nothing; what the arguments alone decide is answered before the device is asked for.
 * RT_ERR_INVALID: a null ctx or p; host form: neither out_rgb nor accum_out, or out_rgb without background_rgb; device
 * form: a null d_accum; every check rt_render applies to p.  RT_ERR_UNSUPPORTED: world > 1, use_photons, the wavefront
 * integrator (reserved[2] bit 0), the legacy RNG.  Then the device (RT_ERR_NO_DEVICE); then the context: RT_ERR_STATE for
 * one that refuses launches or has no resident colours.  The frame runs on the one-wave-per-workgroup kernel family of
 * rt_render_lens (no persistent instances); RT_NODES_Q8 contexts walk their resident 32-byte records, as there.
 * rt_render_aov_colors / rt_render_aov_colors_device are rt_render_aov / rt_render_aov_device with the albedo channel
 * summing c at the first hit instead of the mesh's albedo (the guide rt_denoise and rt_svgf demodulate by); every other
 * channel is rt_render_aov's bit for bit.  rt_render_aov's checks, then RT_ERR_STATE without resident colours.
 * Out of scope: colours combined with the lens, the shutter, light groups, light picks, views, adaptive passes or
 * rt_render_rays; rt_group; image textures (they need texture coordinates, which nothing here loads).                   */
int rt_set_vertex_colors(rt_ctx* ctx, const float* rgb /* [n_vertices][3] HOST memory, NULL: release */, uint32_t n_vertices);
/* out_rgb [h][w][3] or NULL, accum_out [h][w][4] or NULL, background_rgb [h][w][3]: as rt_render's */
int rt_render_colors(rt_ctx* ctx, const rt_params* p, const float* background_rgb, float* out_rgb, float* accum_out,
                     rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain (stats == NULL: asynchronous; stats != NULL: synchronises `stream`, and only it). */
int rt_render_colors_device(rt_ctx* ctx, const rt_params* p, void* d_accum, void* stream, rt_stats* stats);
int rt_render_aov_colors(rt_ctx* ctx, const rt_params* p, const rt_aov* host_out);
int rt_render_aov_colors_device(rt_ctx* ctx, const rt_params* p, const rt_aov* device_out, void* stream);

/* ---- image-textured albedo ------------------------------------------------------------------------------
 * rt_set_textures makes a set of images resident — the textures, one texture index (or RT_TEX_NONE) per mesh and one
 * texture coordinate pair per vertex, indexed by the global vertex id as the normals are — and rt_render_textured renders
 * rt_render's frame with ONE substitution at every shaded vertex: on a mesh with a texture the material is the hit mesh's
 * with albedo replaced, per component, by the sample c of that texture at the hit; from c the vertex forms
 * kdDiffuse = kd * (c / float(M_PI)), as rt_render_colors does.  A mesh mapped to RT_TEX_NONE shades with its own material.
 * The RNG streams, the jitter, every ray, the hit selection, both ray counts, the per-sample clamp and the accumulation are
 * rt_render's: textures never move a ray.  Resident vertex colours are not read.
 * The sample is defined operation by operation (the device has no image instructions): all of it is float32, every
 * operation rounded on its own, nothing fused.
 *   coordinates, per axis, from the uvs of the triangle's three vertices in the order of its index triple and the hit's
 *   barycentrics:  s = (s0 + u * (s1 - s0)) + v * (s2 - s0)      (three equal uvs give s0 exactly); t likewise
 *   RT_TEX_NEAREST:   i = wrap(int(floorf(s * float(W))), W), j = wrap(int(floorf(t * float(H))), H);  c = texel[j][i]
 *   RT_TEX_BILINEAR:  x = s * float(W) - 0.5f; xf = floorf(x); fx = x - xf; i0 = wrap(int(xf), W); i1 = wrap(int(xf) + 1, W);
 *                     y, yf, fy, j0, j1 from t and H in the same way; per component
 *                     a = texel[j0][i0] + fx * (texel[j0][i1] - texel[j0][i0])
 *                     b = texel[j1][i0] + fx * (texel[j1][i1] - texel[j1][i0])
 *                     c = a + fy * (b - a)                        (four equal texels give that texel exactly)
 *   wrap(i, N):       RT_TEX_REPEAT: the non-negative remainder ((i % N) + N) % N in int32; RT_TEX_CLAMP: min(max(i, 0), N - 1)
 * Row j of a texture covers t in [j / H, (j + 1) / H): row 0 is t = 0.  |uv| <= 1024 and W, H <= 16384 keep int(...) far
 * inside int32 (|s| <= 5 * 1024, so |s * W| < 2^27).
 * Guarantees, bit for bit on accumulator, image, samples and both ray counts, for texels that are not -0:
 *   - T1: a set in which every mesh is RT_TEX_NONE gives rt_render's frame; so does a set in which every textured mesh's
 *     texels all equal its material's albedo, whatever the uvs, filters and wraps.
 *   - T2: on a scene in which triangle k of n owns its three vertices, all three with uv ((3k + 1.5) / (3n), 0.5), and a
 *     3n x 1 texture whose texels 3k .. 3k + 2 hold colour k, the frame under either filter is rt_render_colors' with colour k
 *     on the vertices of triangle k — and so (C2) rt_render's on the scene of one mesh per triangle: every texel a sample can
 *     touch holds the same colour, so the rounding of x cannot show.
 *   - T3: sample ranges chain (spp_begin / spp_count), and host and device forms agree.
 *   - T4: reserved[0] (lanes per pixel), reserved[1] bit 0 (no pool), collect_stats, RT_ACCEL_BRUTE and the node format
 *     change the schedule, never the bits.
 * rt_set_textures copies the whole set to the context's device, into fresh allocations, and then replaces the set before;
 * NULL releases it.  It changes nothing any other entry point reads; the set stays across every update, refit, rt_rebuild,
 * transform and skin (uvs go by global vertex id, and the vertex and mesh counts of a context never change) and goes with
 * rt_destroy.  It is a host form: it returns when the copies are done; the arrays it replaces are freed once the launches
 * that read them have run.
 *   RT_ERR_INVALID, with rt_last_error naming the first offending value, in this order: a null textures, mesh_texture or
 *   vertex_uv; n_textures == 0; a non-zero reserved word of the set; per texture, in index order: a width or height outside
 *   1..16384, an unknown wrap_s, wrap_t or filter, a non-zero reserved word, a null texels, a running total of texels above
 *   2^28; then a texel that is not finite; a mesh_texture entry that is neither an index nor RT_TEX_NONE; a uv that is not
 *   finite or beyond 1024 in magnitude; then a null ctx with a non-null set; n_meshes or n_vertices different from the
 *   context's.  A null set with a null ctx.
 *   RT_ERR_STATE  a context that refuses launches (nothing is uploaded to it).
 * rt_render_textured / rt_render_textured_device take rt_render's / rt_render_device's arguments and rt_render_colors'
 * checks in its order: RT_ERR_INVALID for what the arguments alone decide; RT_ERR_UNSUPPORTED: world > 1, use_photons, the
 * wavefront integrator (reserved[2] bit 0), the legacy RNG; then the device (RT_ERR_NO_DEVICE); then the context:
 * RT_ERR_STATE for one that refuses launches or has no resident set.  The frame runs on the one-wave-per-workgroup kernel
 * family of rt_render_lens (no persistent instances); RT_NODES_Q8 contexts walk their resident 32-byte records, as there.
 * rt_render_aov_textured / rt_render_aov_textured_device are rt_render_aov / rt_render_aov_device with the albedo channel
 * summing c at the first hit (the mesh's albedo on an RT_TEX_NONE mesh); every other channel is rt_render_aov's bit for
 * bit.  rt_render_aov's checks, then RT_ERR_STATE without a resident set.
 * Out of scope: mip maps and any filter that needs ray footprints; 8-bit or sRGB texel storage; textures on
 * kd, alpha and f0 and on normals here (rt_render_material and rt_render_normal_mapped below); textures combined with vertex colours, the lens, the shutter, light groups, light picks, views, adaptive passes
 * or rt_render_rays; rt_group; a device-memory form of the set.                                                          */
#define RT_TEX_NONE 0xffffffffu
enum { RT_TEX_REPEAT = 0, RT_TEX_CLAMP = 1 };
enum { RT_TEX_NEAREST = 0, RT_TEX_BILINEAR = 1 };
typedef struct rt_texture {
  uint32_t width, height;      /* 1..16384 each                                            */
  uint32_t wrap_s, wrap_t;     /* RT_TEX_REPEAT | RT_TEX_CLAMP                             */
  uint32_t filter;             /* RT_TEX_NEAREST | RT_TEX_BILINEAR                         */
  uint32_t reserved[3];        /* 0                                                        */
  const float* texels;         /* [height][width][3] HOST memory, linear rgb, any finite value;
                                  row j covers t in [j/height, (j+1)/height)               */
} rt_texture;
typedef struct rt_texture_set {
  uint32_t n_textures, n_meshes, n_vertices;   /* the last two must be the context's       */
  const rt_texture* textures;                  /* [n_textures]                             */
  const uint32_t* mesh_texture;                /* [n_meshes]: a texture index or RT_TEX_NONE */
  const float* vertex_uv;                      /* [n_vertices][2], global vertex ids, finite, |.| <= 1024 */
  uint32_t reserved[4];
} rt_texture_set;
int rt_set_textures(rt_ctx* ctx, const rt_texture_set* set /* NULL: release */);
/* out_rgb [h][w][3] or NULL, accum_out [h][w][4] or NULL, background_rgb [h][w][3]: as rt_render's */
int rt_render_textured(rt_ctx* ctx, const rt_params* p, const float* background_rgb, float* out_rgb, float* accum_out,
                       rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream` (a hipStream_t, may be NULL), as rt_render_device
 * does: sample ranges chain (stats == NULL: asynchronous; stats != NULL: synchronises `stream`, and only it). */
int rt_render_textured_device(rt_ctx* ctx, const rt_params* p, void* d_accum, void* stream, rt_stats* stats);
int rt_render_aov_textured(rt_ctx* ctx, const rt_params* p, const rt_aov* host_out);
int rt_render_aov_textured_device(rt_ctx* ctx, const rt_params* p, const rt_aov* device_out, void* stream);

/* ---- motion vectors and temporal accumulation (DESIGN.md "Motion vectors and temporal accumulation") ----------------
 * Two stateless calls for animated frames.  The library keeps nothing between frames: the caller hands in last frame's
 * vertex positions and camera (what it gave rt_update then) and last frame's history buffers.
 *
 * rt_render_motion casts ONE ray per pixel, whatever spp is: the primary ray of sample spp_begin of the frame p describes
 * (the sample rt_aov.mesh / .tri describe: same stream seed, jitter_sample, camera_ray, same tree walk, or the exhaustive
 * loop for RT_ACCEL_BRUTE; RT_NODES_Q8 contexts walk their resident 32-byte records as rt_render_aov does).
 *   Miss: motion = (0, 0), position = prev_position = 0, mesh = 0xffffffff.
 *   Hit on global triangle g with the barycentrics (u, v) the frame shades with: position is the frame's hit point
 *   (Renderer.cpp:43), float32: w = (1 - u) - v; X = (w P0 + u P1) + v P2 over the context's positions — rt_aov.position
 *   of a one-sample range, in value.  prev_position X' is the SAME float32 expression over prev->vertex_pos at g's three
 *   vertex ids.
 *   Screen position of a point Y under a camera c, in float64 from the float32 inputs, in this order, no contraction
 *   (cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z):
 *     q = Y - c.position;  a = c.lower_left - c.position;  H = c.horizontal;  V = c.vertical
 *     qn = dot(q, cross(H, V));  den = dot(a, cross(H, V))
 *     s = dot(a, cross(q, V)) / qn;  t = dot(a, cross(H, q)) / qn;  sx = s width;  sy = (1 - t) height
 *   (camera_ray inverted: Y - position = lambda (a + s H + t V) by Cramer's rule); Y is in front of c iff qn / den > 0.
 *   motion = ((float)(sx(X', prev camera) - sx(X, the context's camera)), (float)(sy(..) - sy(..))): previous minus
 *   current screen position, in pixels.  If either point is not in front of its camera, or one of the four coordinates
 *   is not finite: motion = (+inf, +inf).
 *   With NULL prev members (or the context's own arrays and camera) every hit pixel has motion == (0, 0) exactly and
 *   prev_position == position bit for bit.
 * Validation comes first and a rejected call writes nothing: RT_ERR_INVALID for a null ctx, p, prev or out, non-zero
 * reserved words, a non-finite prev->camera, and rt_render_aov's size and range checks; RT_ERR_UNSUPPORTED for world > 1.
 * mode, max_depth and the photon fields do not affect the pass.                                                        */
typedef struct rt_motion_prev {
  const float* vertex_pos;   /* [n_vertices][3] LAST frame's positions (host form: host memory; device form: device
                                memory on the context's device), or NULL = the context's own (geometry did not move) */
  const rt_camera* camera;   /* HOST memory; last frame's camera, or NULL = the context's own                        */
  uint32_t reserved[6];      /* zero */
} rt_motion_prev;
typedef struct rt_motion {   /* every pointer may be NULL (channel not wanted); the others are overwritten            */
  float* motion;             /* [h][w][2] previous minus current screen position of the surface point, in pixels     */
  float* position;           /* [h][w][3] the hit point X in THIS frame (float32)                                    */
  float* prev_position;      /* [h][w][3] the same surface point X' in LAST frame's positions (float32)              */
  uint32_t* mesh;            /* [h][w]    mesh of the hit, 0xffffffff = miss (== rt_aov.mesh for the same params)    */
  uint32_t reserved[4];      /* zero */
} rt_motion;
/* The host form uploads prev->vertex_pos into scratch the context owns. */
int rt_render_motion(rt_ctx* ctx, const rt_params* p, const rt_motion_prev* prev, const rt_motion* host_out);
/* The same into DEVICE buffers on `stream` (a hipStream_t, may be NULL): prev->vertex_pos is read on `stream`; no
 * synchronisation. */
int rt_render_motion_device(rt_ctx* ctx, const rt_params* p, const rt_motion_prev* prev, const rt_motion* device_out,
                            void* stream);

/* rt_temporal_accumulate reprojects last frame's history along the motion vectors and blends the current frame in.
 * Per pixel (px, py), float64, in this order, no contraction; c = cur_rgb at the pixel, (mx, my) = cur->motion there:
 *   1. No history if cur->mesh == 0xffffffff or a motion component is not finite: out = c, out_length = 1.
 *   2. rx = px + mx; ry = py + my (the pixel centres cancel).  rx < -1, rx >= width, ry < -1 or ry >= height: no
 *      history.  x0 = floor(rx), ax = rx - x0; likewise y0, ay.
 *   3. Taps (x0 + i, y0 + j) in the order (0,0), (1,0), (0,1), (1,1), weight wx_i wy_j with wx = (1 - ax, ax).  A tap
 *      counts iff its weight is > 0, it is inside the image, prev->length > 0 there, prev->mesh there == cur->mesh and
 *      (dx dx + dy dy) + dz dz <= sigma_position^2 for d = prev->position[tap] - cur->prev_position[pixel].
 *   4. W = the sum of the counted weights.  W <= 0: no history.  Otherwise h = sum(w rgb_tap) / W per channel,
 *      L = sum(w length_tap) / W, Ln = min(L + 1, max_history), alpha = max(1 / Ln, alpha_min),
 *      out = (float)(h + alpha (c - h)), out_length = (float)Ln.
 * (sigma_position is a float; its square is formed in float64.)  The next frame's history is {out_rgb, cur->position,
 * cur->mesh, out_length}: the caller ping-pongs two sets.  The first frame of a sequence passes a history whose length
 * is all 0.  Defaults (0), chosen on two turntable sequences: max_history 16; sigma_position 2 % of the
 * diagonal of the bounding box of the vertices the context's triangles reference, in float32 (rt_denoise's default and
 * reduction).  RT_ERR_INVALID: null arguments or required channels, a size outside 1..65535, a negative or non-finite
 * sigma or alpha, alpha_min > 1, non-zero reserved words, out_rgb or out_length overlapping a history buffer (taps read
 * neighbouring pixels).  out_rgb may equal cur_rgb.                                                                    */
typedef struct rt_temporal_params {
  uint32_t width, height;
  uint32_t max_history;     /* 0 = default; the history length saturates here                          */
  float alpha_min;          /* 0 = none: pure 1 / length; otherwise finite, in (0, 1]                  */
  float sigma_position;     /* 0 = default: rt_denoise's default sigma_position (same reduction)       */
  uint32_t reserved[6];     /* zero */
} rt_temporal_params;
typedef struct rt_history {  /* one frame's history; all four required                                 */
  float* rgb;        /* [h][w][3] accumulated colour                                                   */
  float* position;   /* [h][w][3] rt_motion.position of the frame that wrote it                       */
  uint32_t* mesh;    /* [h][w]    rt_motion.mesh of that frame                                         */
  float* length;     /* [h][w]    frames accumulated in rgb; 0 = no history                            */
} rt_history;
/* cur: motion, prev_position and mesh required.  Host buffers. */
int rt_temporal_accumulate(rt_ctx* ctx, const rt_temporal_params* t, const float* cur_rgb, const rt_motion* cur,
                           const rt_history* prev, float* out_rgb, float* out_length);
/* The same on DEVICE buffers, ordered on `stream` (may be NULL); no synchronisation. */
int rt_temporal_accumulate_device(rt_ctx* ctx, const rt_temporal_params* t, const void* d_cur_rgb, const rt_motion* d_cur,
                                  const rt_history* d_prev, void* d_out_rgb, void* d_out_length, void* stream);

/* ---- variance-guided spatiotemporal filtering (DESIGN.md "Variance-guided spatiotemporal filtering") ----------------
 * rt_svgf (Schied et al., HPG 2017) accumulates the demodulated frame and its luminance moments in time, turns the moments
 * into a per-pixel variance and lets that variance steer an a-trous filter.  Stateless like the calls above: the caller
 * ping-pongs two rt_svgf_history sets.  Guides n = normal/hits, x = position/hits (float32); a pixel is VALID iff hits > 0.
 *
 * Stage A, per pixel, every pixel alike; float64 from the float32 inputs, in this order, no contraction:
 *   f = max(albedo/hits, 1e-3) per channel and d = cur_rgb / f, both in float32 (rt_denoise's); hits == 0: f = 1, d = cur_rgb.
 *   l = (0.2126 d.r + 0.7152 d.g) + 0.0722 d.b.
 *   Steps 1-4 of rt_temporal_accumulate with sigma_reproject for its sigma_position and prev->color for its rgb: the same
 *   tap order, acceptance test and W.  No history: accum = d, moments = (l, l l), length = 1.  Otherwise, h, hm1, hm2, L the
 *   weighted means sum(w tap) / W of prev->color, prev->moments and prev->length:
 *     Ln = min(L + 1, max_history);  alpha = max(1 / Ln, alpha_min);  alpha_m = max(1 / Ln, alpha_min_moments)
 *     accum = h + alpha (d - h);  m1 = hm1 + alpha_m (l - hm1);  m2 = hm2 + alpha_m (l l - hm2);  length = Ln
 *   out->accum, out->moments = (m1, m2) and out->length are these values rounded to float32, never filtered in space.
 * Stage B, float32 from here on, from the float32 m1, m2, Ln of stage A; sums run in tap order, rows first (dy outer):
 *   not VALID: var = 0.  Ln >= 4: var = max(0, m2 - m1 m1).  Otherwise over the taps q = p + (dx, dy), dx, dy in -3..3,
 *   inside the image and VALID: w = expf(-(|n_p-n_q|^2 / sn^2 + |x_p-x_q|^2 / sx^2)), M1 = sum(w m1_q) / sum(w), M2 likewise,
 *   var = max(0, M2 - M1 M1) * (4 / Ln).   (|a|^2 = (a.x a.x + a.y a.y) + a.z a.z; 1 / sn^2 = 1 / (sn sn), 1 / sx^2 likewise,
 *   formed once and multiplied.)
 * Stage C: iteration i (from 0) has step s = 2^i and works on (c, var), at first (accum, var).  A pixel that is not VALID
 *   keeps (c, var).  Otherwise g = sum(k var_q) / sum(k) over q = p + (dx, dy), dx, dy in -1..1 (whatever s is), inside the
 *   image and VALID, k = {1/4, 1/2, 1/4}[dx] {1/4, 1/2, 1/4}[dy]; lum(c) = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b; over the
 *   taps q = p + s (dx, dy), dx, dy in -2..2, inside the image and VALID, h = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *     w = (h[dx] h[dy]) expf(-((|n_p-n_q|^2 / sn^2 + |x_p-x_q|^2 / sx^2) + |lum(c_p) - lum(c_q)| / (sl sqrtf(g) + 1e-4)))
 *     c' = sum(w c_q) / sum(w);  var' = sum((w w) var_q) / (sum(w) sum(w))
 *   out->color is iteration 0's c' (the history the next frame accumulates onto: the paper's feedback), out->rgb the last
 *   c' times f, out->variance the last var'.
 * The next frame's history is {out->color, out->moments, cur->position, cur->mesh, out->length}; the first frame of a
 * sequence passes a history whose length is all 0.  Defaults (0), chosen on two turntable sequences:
 * iterations 5, max_history 2, sigma_luminance 2, sigma_normal 0.5, sigma_position and sigma_reproject 2 % of the diagonal
 * of the bounding box of the vertices the context's triangles reference (rt_denoise's and rt_temporal_accumulate's).
 * Validation comes first and a rejected call writes nothing: RT_ERR_INVALID for null arguments, required channels or
 * required outputs, a size outside 1..65535, iterations above 8, a negative or non-finite sigma or alpha, an alpha above 1,
 * non-zero reserved words, an output overlapping a history buffer or another output.  out->rgb may equal cur_rgb.  A call
 * that passes them answers RT_ERR_NO_DEVICE where there is no HIP device.                                              */
typedef struct rt_svgf_params {
  uint32_t width, height;
  uint32_t iterations;        /* 0 = 5; at most 8                                                            */
  uint32_t max_history;       /* 0 = default; the history length saturates here                              */
  float alpha_min;            /* colour: 0 = none: pure 1 / length; otherwise finite, in (0, 1]              */
  float alpha_min_moments;    /* the same for the two moments                                                */
  float sigma_luminance;      /* 0 = default; in standard deviations of the pixel's luminance                */
  float sigma_normal;         /* 0 = default                                                                 */
  float sigma_position;       /* the spatial guide; 0 = rt_denoise's default                                 */
  float sigma_reproject;      /* the tap acceptance; 0 = rt_temporal_accumulate's default                    */
  uint32_t reserved[6];       /* zero */
} rt_svgf_params;
typedef struct rt_svgf_history {  /* one frame's history; all five required                                  */
  float* color;      /* [h][w][3] DEMODULATED colour (rt_svgf_out.color)                                    */
  float* moments;    /* [h][w][2] first and second luminance moment                                         */
  float* position;   /* [h][w][3] rt_motion.position of the frame that wrote it                            */
  uint32_t* mesh;    /* [h][w]    rt_motion.mesh of that frame                                              */
  float* length;     /* [h][w]    frames accumulated; 0 = no history                                        */
} rt_svgf_history;
typedef struct rt_svgf_out {
  float* rgb;        /* [h][w][3] the filtered frame, required                                              */
  float* color;      /* [h][w][3] required: the next history's colour                                       */
  float* moments;    /* [h][w][2] required: the next history's moments                                      */
  float* length;     /* [h][w]    required: the next history's length                                       */
  float* accum;      /* [h][w][3] optional: stage A's colour, before any spatial filter                     */
  float* variance;   /* [h][w]    optional: the variance after the last iteration                           */
  uint32_t reserved[4];  /* zero */
} rt_svgf_out;
/* cur_rgb: a resolved frame [h][w][3]; aov_sums: the SUMS of rt_render_aov for the same params (albedo, normal, position,
 * hits required); cur: rt_render_motion's channels for it (motion, prev_position, mesh required; position is what the
 * caller keeps for the next history).  Host buffers. */
int rt_svgf(rt_ctx* ctx, const rt_svgf_params* s, const float* cur_rgb, const rt_aov* aov_sums, const rt_motion* cur,
            const rt_svgf_history* prev, const rt_svgf_out* out);
/* The same on DEVICE buffers, ordered on `stream` (may be NULL); no synchronisation.  The context's scratch serves one
 * call at a time. */
int rt_svgf_device(rt_ctx* ctx, const rt_svgf_params* s, const void* d_cur_rgb, const rt_aov* d_aov_sums,
                   const rt_motion* d_cur, const rt_svgf_history* d_prev, const rt_svgf_out* d_out, void* stream);

/* ---- adaptive sampling (DESIGN.md "Adaptive sampling") -----------------------------------------------------------
 * A frame of passes of P = p->spp samples per pixel.  Pass k renders the frame rt_render renders for p with seed
 * p->seed + k (uint32 wrap-around), over the 8x8-pixel granules still active only; each pass is a full stratified set
 * (jitter_sample(i, P), i in 0..P-1).  A granule that ran K passes holds in accum exactly what K calls of
 * rt_render_passes leave on a zero accumulator (call j: seed p->seed + j, spp P, spp_begin = spp_count = 0), bit for
 * bit; spp[pixel] = K * P, and out_rgb is rt_resolve_device of that accumulator with spp = K * P, pixel by pixel.
 * After every pass, per in-image pixel of a granule it rendered (float64, in this order, no contraction):
 *   d = accum - prev (float32);  prev = accum;  miss = P - d.w
 *   y = (0.2126 (d.x + bg_r miss) + 0.7152 (d.y + bg_g miss) + 0.0722 (d.z + bg_b miss)) / P;  S1 += y;  S2 += y y
 *   converged: K >= max(min_passes, 2) and v / K <= (threshold (m + floor))^2, m = S1 / K,
 *              v = max(0, (S2 - S1 m) / (K - 1))
 * A granule retires when every in-image pixel of it has converged, and stays retired.  The run ends after max_passes
 * passes or when no granule is active.  threshold 0: nothing retires (every granule runs max_passes).
 * Validation comes first and a rejected call changes nothing: RT_ERR_INVALID for null arguments, spp_begin / spp_count
 * not 0, a bad rt_adaptive_params or max_passes * spp above 2^31 - 1, and rt_render's checks; RT_ERR_UNSUPPORTED for
 * world > 1 (tile-sharded adaptive frames) and the wavefront integrator (reserved[2] bit 0).                          */
typedef struct rt_adaptive_params {
  uint32_t max_passes;   /* >= 1                                                                                 */
  uint32_t min_passes;   /* 0 = min(4, max_passes); otherwise 2..max_passes                                       */
  float threshold;       /* relative standard error of a pixel's mean luminance; 0 = never retire; finite, >= 0 */
  float floor;           /* 0 = 0.01; finite, > 0: keeps dark pixels from demanding unlimited samples             */
  uint32_t reserved[6];  /* zero                                                                                 */
} rt_adaptive_params;
typedef struct rt_adaptive_report {
  uint32_t passes;             /* passes run                                                                    */
  uint32_t granules;           /* 8x8 granules of the frame                                                     */
  uint64_t pixel_samples;      /* sum over pixels of spp                                                        */
  uint32_t active[64];         /* granules rendered by pass k (k < 64)                                          */
  double render_ms, adapt_ms;  /* device time: the render passes / the statistics and compaction kernels        */
  double total_ms;             /* wall time of the call                                                         */
  uint64_t reserved[4];
} rt_adaptive_report;
/* Host buffers: background_rgb / out_rgb [h][w][3]; accum_out [h][w][4] or NULL; spp_out [h][w] or NULL; rep, stats
 * may be NULL (stats: summed over the passes, samples = rep->pixel_samples). */
int rt_render_adaptive(rt_ctx* ctx, const rt_params* p, const rt_adaptive_params* a, const float* background_rgb,
                       float* out_rgb, float* accum_out, uint32_t* spp_out, rt_adaptive_report* rep, rt_stats* stats);
/* The same on DEVICE buffers, ordered on `stream` (may be NULL).  d_accum ([h][w][4]) is overwritten; d_spp may be
 * NULL.  The pass loop reads the active-granule counts back to the host: one synchronisation of `stream` per pass
 * (and one more at the end when rep or stats is given).  The context's adaptive scratch serves one call at a time. */
int rt_render_adaptive_device(rt_ctx* ctx, const rt_params* p, const rt_adaptive_params* a, const void* d_bg,
                              void* d_accum, void* d_out, void* d_spp, void* stream, rt_adaptive_report* rep,
                              rt_stats* stats);

/* ---- many views of one scene (DESIGN.md "Multi-view frames") -------------------------------------------------------
 * One launch renders n_views frames of the same p, view j with camera cameras[j] and stream key seeds[j] (p->seed for
 * every view when seeds is NULL).  Slice j of the accumulator is, bit for bit, what rt_render_device leaves for the same
 * p on this context after a camera-only rt_update to cameras[j] (with p->seed replaced by seeds[j]); the resolved image
 * is rt_resolve_device of that slice.  stats: rays_closest, rays_shadow and knn_queries are the sums of the per-view
 * frames' counts, samples covers every view, kernel_ms is the one launch.  The context's own camera does not change.
 * Cameras the tree must cover (rt_update's rules, per view camera): a non-finite view camera, or one beyond the operand
 * bounds of a context that takes the short reciprocal forms (rt_bvh_info.flags), is RT_ERR_INVALID, naming the view in
 * rt_last_error; a view camera that needs a wider box padding than the context has makes the call refit the boxes first
 * to the widest padding any view needs, which the context keeps (rt_bvh_info.pad; the photon map stays, as after a
 * camera-only update) — RT_ERR_UNSUPPORTED on RT_NODES_Q8 contexts.  The frames do not depend on the padding.
 * Validation comes first and a rejected call writes nothing: RT_ERR_INVALID for a null ctx, p, v or cameras, n_views
 * of 0 or above 65535, n_views * width * height of 2^31 or more, non-zero reserved fields, the camera rule and
 * rt_render's checks; RT_ERR_UNSUPPORTED for world > 1 and the wavefront integrator (reserved[2] bit 0); RT_ERR_STATE
 * for the photon cases, as rt_render.  The context's view scratch serves one call at a time.                        */
typedef struct rt_views {
  uint32_t n_views;            /* 1..65535; n_views * width * height < 2^31                       */
  uint32_t reserved0;          /* zero                                                            */
  const rt_camera* cameras;    /* [n_views], HOST memory                                          */
  const uint32_t* seeds;       /* [n_views] HOST memory, or NULL = p->seed for every view         */
  uint32_t reserved[6];        /* zero                                                            */
} rt_views;
/* background_rgb [h][w][3] shared by every view (required when out_rgb is given, as rt_render);
 * out_rgb [n][h][w][3] or NULL; accum_out [n][h][w][4] or NULL; stats summed over the views. */
int rt_render_views(rt_ctx* ctx, const rt_params* p, const rt_views* v, const float* background_rgb,
                    float* out_rgb, float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [n][h][w][4] on `stream` (a hipStream_t, may be NULL), as
 * rt_render_device does (sample ranges chain). To resolve view j, call rt_resolve_device on
 * d_accum + j*h*w*4 floats.  The host waits only to refit (a wider padding), to read stats back, and for the previous
 * call's upload of the view records. */
int rt_render_views_device(rt_ctx* ctx, const rt_params* p, const rt_views* v, void* d_accum, void* stream,
                           rt_stats* stats);

/* ---- lens and shutter per view, and in adaptive passes ------------------------------------------------
 * rt_render_views_shutter is rt_render_views with an open shutter of its own on every view: view j sees cameras[j] when
 * its shutter opens and shutters[j].camera_close when it closes, with shutters[j]'s exposure and lens.  shutters is HOST
 * memory, [n_views] records; rt_views, rt_shutter and their rules are the ones above.  A lens without motion is a record
 * with camera_close == cameras[j], open == close == 0 and aperture > 0 (rt_render_shutter's G3): there is no separate lens
 * variant, and views with and without a lens share the launch.
 * Host-derived constants, per view, in rt_render_shutter's arithmetic with A = cameras[j], B = shutters[j].camera_close:
 * D = B - A in float32; with aperture > 0, fs0 and fs1 by the fs rule in float64, rounded, and dfs = fs1 - fs0 in float32.
 * Every sample of view j is then formed by steps 1 to 6 of the rt_render_shutter contract with seed seeds[j] (p->seed when
 * seeds is NULL), pix local to the view, and these constants.
 * Guarantees (all bit for bit: accumulator words and both ray counts):
 *   - V1, slices: slice j of the accumulator is what rt_render_shutter_device leaves for the same p with p->seed replaced
 *     by seeds[j] and the record shutters[j], on this context after a camera-only rt_update to cameras[j]; the image is
 *     rt_resolve_device of that slice.  Through G1 every sample is a row of rt_render_rays.
 *   - V2, no optics: if every shutters[j] has camera_close == cameras[j], open == close == 0 and aperture == 0, the call
 *     equals rt_render_views / rt_render_views_device (cameras with no -0 component: G2's condition).
 *   - V3, schedule: sample ranges chain; reserved[0] (lanes per pixel) and reserved[1] bit 0 (no pool) never change the
 *     bits.
 *   - V4: n_views == 1 with cameras[0] equal to the context's camera is rt_render_shutter.
 * Stats are sums over the views, as for rt_render_views.  The context's camera does not change.  The frame runs on the
 * one-wave-per-workgroup kernel family (no persistent instances); RT_NODES_Q8 contexts walk their resident 32-byte
 * records.
 * The camera rule is rt_render_views', applied to cameras[j] in full and to camera_close for finiteness and for the
 * padding: the call refits once, to the widest padding any end camera of any view needs, which the context keeps —
 * RT_ERR_UNSUPPORTED on RT_NODES_Q8 contexts.
 * Validation comes first and a rejected call writes nothing; what the arguments alone decide is answered before the
 * device is asked for, in this order.  RT_ERR_INVALID: a null ctx, p, v or cameras; a null shutters; host form: neither
 * out_rgb nor accum_out, or out_rgb without background_rgb; device form: a null d_accum; every check rt_render applies to
 * p; rt_render_views' checks of v (reserved words, n_views 1..65535, n_views * width * height < 2^31) — with
 * RT_ERR_UNSUPPORTED for world > 1, the wavefront integrator (reserved[2] bit 0), use_photons and the legacy RNG, as
 * rt_render_shutter; then view by view, naming the view in rt_last_error ("view j: ..."): a non-finite cameras[j], and
 * rt_render_shutter's checks of shutters[j] (reserved words, a non-finite camera_close, the open / close range, aperture,
 * focus_distance).  Then the device: RT_ERR_NO_DEVICE.  Then, reading the context: rt_render_views' camera rule with the
 * padding as above; and view by view, naming the view, rt_render_shutter's camera checks with cameras[j] in the place of
 * the context's camera: the origin bound over both ends plus 2 aperture (against the bound the frame runs under: the
 * context's, or the refit's), the axes (an H or V that cannot be normalised, or dot(H_A, H_B) <= 0 or dot(V_A, V_B) <= 0),
 * and with aperture > 0 the fs rule at both ends.
 * Buffers as rt_render_views': background_rgb [h][w][3] shared by every view; out_rgb [n][h][w][3] or NULL; accum_out
 * [n][h][w][4] or NULL. */
int rt_render_views_shutter(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_shutter* shutters,
                            const float* background_rgb, float* out_rgb, float* accum_out, rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [n][h][w][4] on `stream` (may be NULL), as rt_render_views_device does:
 * sample ranges chain, and the view and shutter records go up through the same ring of pinned copies.  The host waits only
 * to refit, to read stats back, and for the upload of the call four multi-view calls back. */
int rt_render_views_shutter_device(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_shutter* shutters,
                                   void* d_accum, void* stream, rt_stats* stats);
/* rt_render_adaptive_shutter is rt_render_adaptive whose passes are rt_render_shutter frames: the context's camera when
 * the shutter opens, shutter->camera_close when it closes.
 *   - A1: a granule that ran K passes holds in accum exactly what K calls of rt_render_shutter_device leave on a zero
 *     accumulator (call k: seed p->seed + k, spp P, the whole range, the same shutter), bit for bit.
 * Retirement, spp_out, out_rgb and the report are rt_render_adaptive's rule over those passes.  A record that changes
 * nothing (camera_close equal to the context's camera, aperture 0; cameras with no -0 component) makes the call
 * rt_render_adaptive itself.  Validation comes first and a rejected call writes nothing: RT_ERR_INVALID for a null ctx, p,
 * a or shutter; then rt_render_shutter's checks of the record and of p (RT_ERR_UNSUPPORTED for world > 1, use_photons, the
 * wavefront bit, the legacy RNG); rt_render_adaptive's checks of p and a; null buffers (background_rgb / out_rgb; d_bg /
 * d_accum / d_out); then the device (RT_ERR_NO_DEVICE); then the context's state and rt_render_shutter's camera checks.
 * Buffers, the synchronisation per pass and the scratch are rt_render_adaptive's / rt_render_adaptive_device's. */
int rt_render_adaptive_shutter(rt_ctx* ctx, const rt_params* p, const rt_adaptive_params* a, const rt_shutter* shutter,
                               const float* background_rgb, float* out_rgb, float* accum_out, uint32_t* spp_out,
                               rt_adaptive_report* rep, rt_stats* stats);
int rt_render_adaptive_shutter_device(rt_ctx* ctx, const rt_params* p, const rt_adaptive_params* a,
                                      const rt_shutter* shutter, const void* d_bg, void* d_accum, void* d_out,
                                      void* d_spp, void* stream, rt_adaptive_report* rep, rt_stats* stats);

/* Per-view AOVs, motion vectors and a batched denoiser for the same views: one launch each where a caller would loop over
 * the views with rt_update(camera), rt_render_aov, rt_render_motion and rt_denoise.  Every output is [n_views] slices of
 * its single-view shape: slice j of a channel of c floats or words per pixel starts at j * h * w * c (formed in 64 bits).
 *
 * rt_render_aov_views: slice j of every non-NULL channel is, bit for bit, what rt_render_aov writes for the same p on this
 * context after a camera-only rt_update to cameras[j], with p->seed replaced by seeds[j] (p->seed when seeds is NULL); the
 * pixel index of the RNG stream is local to the view.  NULL channels are not written and shift nothing.
 * rt_render_motion_views: slice j is, bit for bit, rt_render_motion after that update with seeds[j] and
 * prev->camera = &prev->cameras[j] (NULL cameras: last frame's cameras are v->cameras; with a NULL vertex_pos too, every hit
 * has motion (0, 0) exactly).
 * The context's own camera does not change.  A view camera that needs a wider box padding refits once to the widest
 * padding any view needs, which the context keeps, exactly as rt_render_views does — RT_ERR_UNSUPPORTED on RT_NODES_Q8
 * contexts, which otherwise walk their resident 32-byte records as rt_render_aov does.  RT_ACCEL_BRUTE works.
 * Validation comes first; a rejected call writes nothing and leaves the context as it was.  RT_ERR_INVALID: a null ctx, p,
 * v, cameras, prev or output struct; non-zero reserved words; rt_render_aov's size and range checks (mode, max_depth, the
 * photon fields and the wavefront bit do not affect the passes); rt_render_views' checks of v (n_views 1..65535,
 * n_views * width * height < 2^31, the camera rule); a non-finite view camera or previous camera, naming the view in
 * rt_last_error.  RT_ERR_UNSUPPORTED: world > 1.  With valid arguments and no device: RT_ERR_NO_DEVICE.
 * The device forms do not synchronise, except to refit and for the previous call's upload of the view tables, as
 * rt_render_views_device; the context's view scratch serves one call at a time.                                       */
int rt_render_aov_views(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_aov* host_out);
int rt_render_aov_views_device(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_aov* device_out, void* stream);
typedef struct rt_motion_prev_views {
  const float* vertex_pos;        /* as rt_motion_prev: last frame's positions, or NULL = the context's own            */
  const rt_camera* cameras;       /* [n_views] HOST memory: last frame's camera of each view, or NULL = v->cameras     */
  uint32_t reserved[6];           /* zero */
} rt_motion_prev_views;
int rt_render_motion_views(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_motion_prev_views* prev,
                           const rt_motion* host_out);
int rt_render_motion_views_device(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_motion_prev_views* prev,
                                  const rt_motion* device_out, void* stream);
/* rt_denoise over n_frames frames of d->width x d->height: rgb, out and the four guide channels hold [n_frames] slices.
 * Frame j of out is, bit for bit, rt_denoise of slice j: the taps never leave their frame (a stack is not a tall image),
 * and the default sigma_position is computed once, by rt_denoise's reduction.  One packing launch and one launch per
 * iteration over all frames; the context's filter scratch grows to n_frames x a frame's need and serves one call at a
 * time.  rgb may equal out.  RT_ERR_INVALID: rt_denoise's cases, non-zero reserved words, n_frames of 0 or
 * n_frames * width * height of 2^31 or more; with valid arguments and no device: RT_ERR_NO_DEVICE.                    */
int rt_denoise_batch(rt_ctx* ctx, const rt_denoise_params* d, uint32_t n_frames, const float* rgb, const rt_aov* aov, float* out);
int rt_denoise_batch_device(rt_ctx* ctx, const rt_denoise_params* d, uint32_t n_frames, const void* d_rgb, const rt_aov* d_aov,
                            void* d_out, void* stream);

/* ---- vertex colours and textures under the lens, the shutter and many views ---------------------------
 * rt_render_views_shutter_albedo is rt_render_views_shutter with the albedo of every shaded vertex taken from the
 * context's resident vertex colours or texture set.  Since rt_render_views_shutter is the general camera form (one view
 * is a single frame; camera_close == cameras[j], open == close == 0 and aperture > 0 is a pure lens; a record that
 * changes nothing is rt_render_views), this one call gives a coloured or textured scene depth of field, motion blur,
 * many cameras per launch and every mixture of them. */
#define RT_ALBEDO_MATERIAL 0u   /* the meshes' own albedo: the call is the parent form                 */
#define RT_ALBEDO_COLORS   1u   /* the resident vertex colours (rt_set_vertex_colors), rt_render_colors' rule */
#define RT_ALBEDO_TEXTURES 2u   /* the resident texture set (rt_set_textures), rt_render_textured's sampler   */
/* Every sample of view j is generated exactly as rt_render_views_shutter generates it: steps 1 to 6 of the
 * rt_render_shutter contract with seeds[j] (p->seed when seeds is NULL), a pixel index local to the view, and the per-view
 * host-derived constants.  Every ray, the hit selection, both ray counts, the clamp and the accumulation are that form's.
 * The only change is at each shaded vertex: with RT_ALBEDO_COLORS, `albedo` is rt_render_colors' interpolated colour;
 * with RT_ALBEDO_TEXTURES it is rt_render_textured's sample, or the mesh's own albedo on an RT_TEX_NONE mesh; in both
 * cases kdDiffuse = kd * (albedo / float(M_PI)) in the two float32 operations those forms use.
 * Guarantees (all bit for bit: accumulator words and both ray counts):
 *   - X1, slices: slice j is what the same call leaves for n_views == 1, cameras[j], seeds[j], shutters[j].
 *   - X2, no optics: with n_views == 1, cameras[0] equal to the context's camera with no -0 component (the condition V2
 *     and V4 rest on) and a record that changes nothing, the call is rt_render_colors_device / rt_render_textured_device.
 *   - X3, no surface: RT_ALBEDO_MATERIAL is rt_render_views_shutter itself (the same kernels); vertex colours equal to
 *     each mesh's albedo on all of its vertices give that frame too (rt_render_colors' C1), and so do texels all equal to
 *     each mesh's albedo (rt_render_textured's T1).
 *   - X4, faces: on a vertex-split scene with one strip texel per triangle (T2), or per-face colours, the frame is
 *     rt_render_views_shutter of the one-mesh-per-triangle scene under the same views and shutters.
 *   - X5, schedule: sample ranges chain; reserved[0] and reserved[1] bit 0 never change the bits; RT_ACCEL_BRUTE gives the
 *     frame of the tree; an RT_NODES_Q8 context gives the frame of a default context.
 * Validation comes first and a rejected call writes nothing.  The order is rt_render_views_shutter's with two additions:
 * albedo > 2 is RT_ERR_INVALID among the checks the arguments alone decide (after the outputs, before p), ahead of the
 * device; and after the device and rt_render_views_shutter's checks of the context, RT_ERR_STATE when albedo names data the
 * context does not hold (no resident vertex colours, no resident texture set), with rt_render_colors' / rt_render_textured's
 * messages.  world > 1, use_photons, the wavefront bit and the legacy RNG are refused as by rt_render_views_shutter.
 * Buffers, stats and the device form's synchronisation are rt_render_views_shutter's; the resident colours or textures
 * are read in stream order, as by rt_render_colors_device / rt_render_textured_device.  Not combined (each its own form):
 * adaptive passes, light groups, light picks, ray batches, rt_group, textures and colours at once, motion vectors. */
int rt_render_views_shutter_albedo(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_shutter* shutters,
                                   uint32_t albedo, const float* background_rgb, float* out_rgb, float* accum_out,
                                   rt_stats* stats);
int rt_render_views_shutter_albedo_device(rt_ctx* ctx, const rt_params* p, const rt_views* v, const rt_shutter* shutters,
                                          uint32_t albedo, void* d_accum, void* stream, rt_stats* stats);
/* rt_render_aov_views whose albedo channel sums what rt_render_aov_colors / rt_render_aov_textured sum: slice j of every
 * non-NULL channel is, bit for bit, the single-view coloured or textured AOV call for the same p on this context after a
 * camera-only rt_update to cameras[j], with seeds[j].  All other channels are rt_render_aov_views'; RT_ALBEDO_MATERIAL is
 * rt_render_aov_views itself.  Validation is rt_render_aov_views' with albedo > 2 (RT_ERR_INVALID) after the null and
 * reserved-word checks, and RT_ERR_STATE for data the context does not hold after the device and the context's checks. */
int rt_render_aov_views_albedo(rt_ctx* ctx, const rt_params* p, const rt_views* v, uint32_t albedo, const rt_aov* host_out);
int rt_render_aov_views_albedo_device(rt_ctx* ctx, const rt_params* p, const rt_views* v, uint32_t albedo,
                                      const rt_aov* device_out, void* stream);

/* ---- textured material maps: kd, alpha and f0 from the resident textures -------------------------------
 * rt_set_material_maps names, per mesh, two more textures of the RESIDENT texture set (rt_set_textures), and
 * rt_render_material renders rt_render_textured's frame with two more substitutions at every shaded vertex.  The vertex
 * shades with the material {kd, alpha, albedo, f0} in which
 *   albedo      is rt_render_textured's: the sample of texture mesh_texture[mesh], or the mesh's own;
 *   f0          is the rgb sample of texture mesh_f0[mesh];
 *   (kd, alpha) are the r and g of the sample of texture mesh_kd_alpha[mesh] (b is not read: any finite value);
 *   on RT_TEX_NONE, f0 and (kd, alpha) are the mesh's own.
 * All three samples are taken at the same hit coordinate (the one uv per vertex, interpolated as rt_render_textured
 * does), each by rt_render_textured's sampler under its own texture's filter and wraps.  From those eight floats the BSDF
 * is evaluateColorResponse of that material, in exactly the operations rt_create performs on an rt_material: albedo /
 * float(M_PI) then * kd; 1 - kd; alpha * alpha; 1 - f0; k = float(double(alpha) * sqrt(2 / pi)); 1 - k — all float32 but
 * k's product, nothing fused.  No range is imposed on the sampled fields beyond the set's finiteness, as none is on
 * rt_material: an alpha of 0 shades as an rt_material with alpha = 0 does.  The RNG streams, the jitter, every ray, the
 * hit selection, both ray counts, the per-sample clamp and the accumulation are rt_render_textured's: the frame's bounce
 * is drawn from the shading normal alone, so no material field moves a ray.
 * Guarantees, bit for bit on accumulator, image, samples and both ray counts:
 *   - M1: maps that are RT_TEX_NONE on every mesh (or both NULL) give rt_render_textured's frame; so do maps whose texels
 *     equal the mesh's own f0 / (kd, alpha, anything), whatever the uvs, filters and wraps; with T1 that frame is rt_render's.
 *   - M2: on T2's vertex-split scene (triangle k of n with uv ((3k + 1.5) / (3n), 0.5) on its three vertices) and 3n x 1
 *     textures whose texels 3k .. 3k + 2 hold triangle k's albedo, f0 and (kd, alpha, any), the frame under either filter is
 *     rt_render's on the scene of one mesh per triangle whose material k has those four fields.
 *   - M3: sample ranges chain (spp_begin / spp_count), and host and device forms agree.
 *   - M4: reserved[0] (lanes per pixel), reserved[1] bit 0 (no pool), collect_stats, RT_ACCEL_BRUTE and the node format
 *     change the schedule, never the bits.
 * rt_set_material_maps is a host form: it copies the two tables to the context's device, into fresh allocations, and then
 * replaces the ones before, which are freed once the launches that read them have run; NULL releases.  It changes nothing
 * any other entry point reads; the maps stay across every update, refit, rt_rebuild, transform and skin.  The indices
 * refer to the texture set resident AT THE CALL: a later rt_set_textures (replace or release) makes the maps stale until
 * rt_set_material_maps is called again.  Refusals, in this order, with rt_last_error naming the first offender:
 *   RT_ERR_INVALID  a null maps with a null ctx; a non-zero reserved word; a null ctx; n_meshes different from the context's
 *   RT_ERR_STATE    a context that refuses launches
 *   RT_ERR_STATE    no resident texture set
 *   RT_ERR_INVALID  an entry that is neither an index below the resident set's n_textures nor RT_TEX_NONE (mesh_f0 is
 *                   scanned first; the message names the table and the mesh)
 * rt_render_material / rt_render_material_device take rt_render_textured's / rt_render_textured_device's arguments and
 * its checks in its order and with its codes (RT_ERR_UNSUPPORTED: world > 1, use_photons, the wavefront integrator, the
 * legacy RNG); then, last of all, RT_ERR_STATE without a resident texture set, without resident maps, or with stale maps
 * ("the material maps were set for another texture set").  A rejected call writes nothing.  The kernels are
 * rt_render_textured's family (one wave per workgroup, no persistent instances); buffers, stats and the device form's
 * stream order are rt_render_textured_device's.
 * Out of scope: maps under the lens, the shutter or views (rt_render_views_shutter_albedo refuses albedo > 2), under light
 * groups, picks, adaptive passes or ray batches; f0 / roughness AOV channels (rt_aov has no room); a second uv set;
 * rt_group.  (Normal maps, which move the bounce ray, are rt_render_normal_mapped's below.)                            */
typedef struct rt_material_maps {
  uint32_t n_meshes;              /* must be the context's */
  const uint32_t* mesh_f0;        /* [n_meshes] HOST: index into the RESIDENT texture set or RT_TEX_NONE; rgb -> f0.
                                     NULL = RT_TEX_NONE on every mesh */
  const uint32_t* mesh_kd_alpha;  /* [n_meshes] HOST: likewise; r -> kd, g -> alpha, b ignored (any finite value).
                                     NULL = RT_TEX_NONE on every mesh */
  uint32_t reserved[5];           /* zero */
} rt_material_maps;
int rt_set_material_maps(rt_ctx* ctx, const rt_material_maps* maps /* NULL: release */);
/* out_rgb [h][w][3] or NULL, accum_out [h][w][4] or NULL, background_rgb [h][w][3]: as rt_render's */
int rt_render_material(rt_ctx* ctx, const rt_params* p, const float* background_rgb, float* out_rgb, float* accum_out,
                       rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream`, as rt_render_textured_device does. */
int rt_render_material_device(rt_ctx* ctx, const rt_params* p, void* d_accum, void* stream, rt_stats* stats);

/* ---- tangent-space normal maps: the shading normal from the resident textures --------------------------
 * rt_set_normal_maps names, per mesh, one more texture of the RESIDENT texture set (rt_set_textures), and
 * rt_render_normal_mapped renders rt_render_material's frame with one more substitution at every shaded vertex: the
 * interpolated unit shading normal N (Renderer.cpp:42) is replaced by N' BEFORE anything reads it.  From then on the
 * light terms, the BSDF and the hemisphere sample of the bounce all use N', so — unlike every other surface form — the
 * paths differ from rt_render's from depth 1 on, and so do both ray counts.  The reference integrator never looks at a
 * geometric normal, and neither does this frame: no side test, no clamping of N' to the hemisphere of the incoming ray.
 * Material maps are optional: without resident material maps the frame behaves as under maps that are RT_TEX_NONE on
 * every mesh; rt_set_material_maps and rt_set_normal_maps may be called in either order.
 * N' is formed in float32, every operation rounded on its own, nothing fused, in exactly these operations (dot3, cross3
 * and unit3 are Vec3.h's: products summed left to right; a * (1 / sqrt(dot3(a, a))) per component):
 *   p0, p1, p2   the hit triangle's CURRENT vertex positions;  e1 = p1 - p0, e2 = p2 - p0
 *   (s_k, t_k)   its three vertices' uvs;  a1 = s1 - s0, a2 = s2 - s0, b1 = t1 - t0, b2 = t2 - t0
 *   r  = a1 * b2 - a2 * b1
 *   Tr = b2 * e1 - b1 * e2,  Br = a1 * e2 - a2 * e1   (per component; both negated when r < 0)
 *   Tp = Tr - dot3(N, Tr) * N;  T = unit3(Tp)
 *   B  = cross3(N, T), negated when dot3(B, Br) < 0
 *   m  = the sample of texture mesh_normal[mesh] at the hit coordinate the albedo uses (rt_render_textured's (s, t)), by
 *        rt_render_textured's sampler under that texture's own filter and wraps
 *   x = 2 * m.r - 1,  y = 2 * m.g - 1,  z = 2 * m.b - 1
 *   V  = (x * T + y * B) + z * N;  N' = unit3(V)
 * The vertex keeps N, with no arithmetic on it, when the mesh's entry is RT_TEX_NONE; when x == 0 && y == 0; when
 * !(r != 0) (zero or NaN: the uvs span no area); when !(dot3(Tp, Tp) > 0); or when dot3(V, V) is not finite and positive.
 * Nothing of the tangent frame is stored: it is formed at every vertex from the positions and uvs resident then.
 * Guarantees, bit for bit on accumulator, image, samples and both ray counts:
 *   - N1: a table that is RT_TEX_NONE on every mesh (or NULL) gives rt_render_material's frame; so does any map whose
 *     texels are (0.5, 0.5, b) with any b, whatever the uvs, filters and wraps (equal texels sample to that texel exactly,
 *     as M1 argues, and 2 * 0.5 - 1 is 0).  With M1 and T1 that frame is rt_render's.
 *   - N2: the frame follows the geometry: after rt_update, rt_update_transforms or rt_update_skin it is the frame of a
 *     fresh context created on the moved scene with the same sets.
 *   - N3: sample ranges chain (spp_begin / spp_count), and host and device forms agree.
 *   - N4: reserved[0] (lanes per pixel), reserved[1] bit 0 (no pool), collect_stats, RT_ACCEL_BRUTE and the node format
 *     change the schedule, never the bits.
 * rt_set_normal_maps is a host form in rt_set_material_maps' pattern: it copies the table to the context's device, into a
 * fresh allocation, and then replaces the one before, which is freed once the launches that read it have run; NULL
 * releases.  It changes nothing any other entry point reads; the table stays across every update, refit, rt_rebuild,
 * transform and skin.  The indices refer to the texture set resident AT THE CALL: a later rt_set_textures (replace or
 * release) makes the table stale until rt_set_normal_maps is called again.  Refusals, in this order, with rt_last_error
 * naming the first offender:
 *   RT_ERR_INVALID  a null maps with a null ctx; a non-zero reserved word; a null ctx; n_meshes different from the context's
 *   RT_ERR_STATE    a context that refuses launches
 *   RT_ERR_STATE    no resident texture set
 *   RT_ERR_INVALID  an entry that is neither an index below the resident set's n_textures nor RT_TEX_NONE (the message
 *                   names the mesh)
 * rt_render_normal_mapped / rt_render_normal_mapped_device take rt_render_material's / rt_render_material_device's
 * arguments and rt_render_textured's checks in its order and with its codes; then, last of all, RT_ERR_STATE without a
 * resident texture set, without resident normal maps, with stale normal maps ("the normal maps were set for another
 * texture set"), or with resident material maps that are stale.  A rejected call writes nothing.  The kernels are
 * rt_render_material's family (one wave per workgroup, no persistent instances); buffers, stats and the device form's
 * stream order are rt_render_material_device's.
 * Out of scope: normal maps under the lens, the shutter, views, light groups, picks, adaptive passes, ray batches or
 * rt_group; the perturbed normal in the AOV normal channel and the denoisers' guides; object-space maps; a strength
 * factor; height or bump maps; per-vertex tangents supplied by the caller; 8-bit texel storage; a second uv set.       */
typedef struct rt_normal_maps {
  uint32_t n_meshes;            /* must be the context's */
  const uint32_t* mesh_normal;  /* [n_meshes] HOST: index into the RESIDENT texture set or RT_TEX_NONE; rgb -> (x, y, z) of
                                   the tangent-space normal by 2 c - 1.  NULL = RT_TEX_NONE on every mesh */
  uint32_t reserved[6];         /* zero */
} rt_normal_maps;
int rt_set_normal_maps(rt_ctx* ctx, const rt_normal_maps* maps /* NULL: release */);
/* out_rgb [h][w][3] or NULL, accum_out [h][w][4] or NULL, background_rgb [h][w][3]: as rt_render's */
int rt_render_normal_mapped(rt_ctx* ctx, const rt_params* p, const float* background_rgb, float* out_rgb, float* accum_out,
                            rt_stats* stats);
/* Accumulate into caller-zeroed DEVICE d_accum [h][w][4] on `stream`, as rt_render_material_device does. */
int rt_render_normal_mapped_device(rt_ctx* ctx, const rt_params* p, void* d_accum, void* stream, rt_stats* stats);

/* ---- multi-GPU (Renderer.cpp:219-265 sharded by pixel tiles) -------------
 * A tile-sharded frame: rank r of `world` integrates the pixels whose `tile`-pixel granule
 * (tx + ty) mod world == r (rt_params.rank/world/tile) into its own zeroed full-frame
 * accumulator.  Assembly moves only what a rank owns: its 8x8-pixel granules, packed
 * [granule][64] float4 in row-major granule order (n = rt_owned_granules), travel to the
 * assembling rank, which scatters them into its frame.  One process per GPU
 * (torch.distributed / MPI) uses the three calls below around its own collective;
 * one process driving N GPUs uses rt_group_*. */
int rt_owned_granules(const rt_params* p, uint32_t rank, uint32_t* n_out);
int rt_pack_owned_device(rt_ctx* ctx, const rt_params* p, const void* d_accum,
                         void* d_packed /* n*64 float4, device */, void* stream);
int rt_unpack_owned_device(rt_ctx* ctx, const rt_params* p, uint32_t from_rank,
                           const void* d_packed, void* d_accum, void* stream);

/* N devices driven from ONE host thread: the scene is replicated (rt_create per device),
 * every device integrates its tiles concurrently, owned granules go to devices[0] over
 * xGMI — RCCL ncclSend/ncclRecv (librccl.so, loaded on first use) when all devices are
 * distinct, peer copies when ranks share a device — and devices[0] resolves.  The image is
 * bit-identical to rt_render's on one device.  rt_params.rank/world are ignored (set per
 * device); tile = 0 selects 32. */
typedef struct rt_group rt_group;
int rt_group_create(const rt_scene_desc* scene, const int32_t* devices, uint32_t n,
                    const rt_options* opt, rt_group** out);
void rt_group_destroy(rt_group* g);
uint32_t rt_group_size(const rt_group* g);
int rt_group_uses_rccl(const rt_group* g);
rt_ctx* rt_group_ctx(rt_group* g, uint32_t rank); /* borrowed: e.g. rt_emit_photons on rank 0 */
int rt_group_set_photons(rt_group* g, const float* pos3, const float* dir3, uint32_t n);
int rt_group_render(rt_group* g, const rt_params* p, const float* background_rgb,
                    float* out_rgb, float* accum_out, rt_stats* stats);
/* rt_update on every rank, rank 0 first (a rejected update leaves every rank as it was); rep: rank 0's report, total_ms
 * the whole call.  A HIP failure on a later rank leaves the ranks before it updated: destroy the group. */
int rt_group_update(rt_group* g, const rt_scene_update* u, rt_update_report* rep);

/* Ray origins: the BVH's exactness argument (box padding vs the float triangle test's
 * error) covers origins up to 16 x max(|scene coordinate|, |camera|, |light position|);
 * rays that start farther out are answered by the exhaustive loop, transparently. */
int rt_trace(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t accel,
             uint32_t kind, rt_hit* hits);
/* RayTracer::rayTrace over a ray QUEUE resident in HBM (the trace stage of the wavefront
 * integrator; also a device-to-device form of rt_trace): ray_o[i] = origin xyz + kind bits
 * in w (bit 0: any-hit), ray_d[i] = direction xyz (float4 each); res[i] (uint2) = closest
 * hit {t bits, global triangle id} or {~0, ~0}, any-hit {0 / 1, 0}.
 * Unlike rt_trace this form has NO exhaustive-loop fallback for far origins: every ray goes
 * through the BVH, so origins must lie within the range the padding covers (16 x max(|scene
 * coordinate|, |camera|, |light position|)) — true of every ray an integrator generates
 * (camera, surface points); the host cannot check device-resident rays. */
int rt_trace_stream_device(rt_ctx* ctx, const void* d_ray_o, const void* d_ray_d, uint32_t n,
                           void* d_res, void* stream);
/* kdtree::knearest for n queries over the context's photon map (rt_set_photons order):
 * slots of the map in the reference's result order, their float distances, nodes visited.
 * This is the walk photon frames run, on their layout: the same entry width (16-bit stack
 * entries below 65,535 photons) and the same stack rows as a frame whose BVH is shallower
 * than the kd tree (the tightest layout), with the k-slot heap directly above the stack.
 * k in 1..16 (else RT_ERR_UNSUPPORTED); an empty map or k > photons: RT_ERR_STATE.
 * Photon frames with k above 16 run the wide walk: see rt_knn_wide. */
int rt_knn(rt_ctx* ctx, const float* query3, uint32_t n, uint32_t k,
           uint32_t* idx_out /*[n][k]*/, float* dist_out /*[n][k]*/,
           uint32_t* visited_out /*[n] or NULL*/);
/* rt_knn for k in 1..RT_KNN_KMAX (else RT_ERR_UNSUPPORTED; the same RT_ERR_STATE cases).
 * k <= 16 runs rt_knn's instance and returns exactly what it returns; larger k run the
 * walk photon frames with that k run, on their tightest layout (the wide k-heap's LDS
 * layout, DESIGN.md "Photon k up to 256"). */
int rt_knn_wide(rt_ctx* ctx, const float* query3, uint32_t n, uint32_t k,
                uint32_t* idx_out /*[n][k]*/, float* dist_out /*[n][k]*/,
                uint32_t* visited_out /*[n] or NULL*/);

/* Inspection hooks for tests (host copies of the flattened acceleration data). */
int rt_bvh_info_get(rt_ctx* ctx, rt_bvh_info* out);
/* nodes64: the float (64-B) form of the node records — the device traverses the same
 * nodes packed to 32 B (binary16 planes rounded outward). */
int rt_bvh_export(rt_ctx* ctx, void* nodes64 /*n_nodes*64 B*/, void* tris48 /*n_tri_records*48 B*/);
/* The host BVH build alone (no GPU, no context): shape, FNV-1a digest of the node and
 * triangle arrays, and wall seconds.  threads: 0 = one per hardware thread (<= 16); the
 * digest must not depend on it.  (No reference counterpart: BVH.h:100-161 is dead code.) */
int rt_bvh_build_host(const rt_scene_desc* scene, uint32_t leaf_max, uint32_t threads, rt_bvh_info* info,
                      uint64_t* digest, double* seconds);
/* The host-built tree in the given device node format alone (no GPU): builds, packs and CHECKS the
 * result — every node reachable exactly once, every triangle record exactly once, every stored child box
 * containing its padded geometry, the depth as reported and within the cap.  node_format: RT_NODES_F16 or
 * RT_NODES_Q8.  out8 = {nodes, Q8: 16-byte slots of the unified array, Q8: blocks, depth, Q8: nodes the
 * packer had to add (leaf wrappers), 0, 0, 0}; est2 (optional) = surface-area estimate of node visits per
 * random ray from the float boxes / from the decoded boxes of the format.  (No reference counterpart: BVH.h
 * is dead code there.) */
int rt_bvh_check_host(const rt_scene_desc* scene, uint32_t leaf_max, uint32_t node_format, uint32_t* out8,
                      double* est2);
/* The host half of the hybrid builder alone (no GPU): the host builder's top down to parts of <= `cutoff` triangles,
 * CHECKED — the parts and the top's own leaves cover every triangle exactly once, every part is referred to by exactly one
 * child slot whose box contains its padded geometry, part roots lie within the depth cap with room for their subtrees, the
 * order is a permutation.  out8 = {top nodes, parts, largest part, deepest part root, depth cap, top leaves, 0, 0}.        */
int rt_bvh_top_check_host(const rt_scene_desc* scene, uint32_t leaf_max, uint32_t cutoff, uint32_t* out8);
/* Measured-cost tuning of the host-built BVH (no counterpart in the reference, whose rayTrace is the exhaustive
 * loop of RayTracer.h:27-53; this only changes HOW FAST the same hits are found).  Every tree over the same leaves
 * returns the same hits, so a probe frame traces exactly the same rays whatever the tree and its counters are a
 * deterministic cost of the tree for the rays of THIS scene, camera and integrator.  rt_bvh_tune renders `probe`
 * (a small frame: e.g. 128x128, 1-2 spp, the mode of the real render) once per proposed change — a subtree moved to
 * another place in the tree, the two children of a node in the other slot order — and keeps a change only if
 * nodes_visited + 1.5 * tris_tested fell.  Stops after `budget_seconds`, after `max_probes` probe frames (0 = no limit;
 * the counters are deterministic, so a probe limit — unlike a time limit — gives the same tree on every run) or when a
 * whole pass finds nothing; a second
 * probe with another seed referees the result (a tuned tree that is not better on it is dropped: accepted = 0).  Images
 * are unchanged by construction (and tested).  Needs a host-built binary tree (RT_ERR_STATE otherwise); must not run
 * concurrently with a launch on the same context. */
typedef struct rt_tune_report {
  uint32_t probes, accepted;
  double cost_before, cost_after; /* nodes_visited + 1.5 * tris_tested of the probe frame */
  double seconds;
  uint64_t reserved[4];
} rt_tune_report;
int rt_bvh_tune(rt_ctx* ctx, const rt_params* probe, double budget_seconds, uint32_t max_probes, rt_tune_report* out);
/* Device-time bookkeeping: every rt_render_device launch is bracketed by a HIP
 * event pair on its stream.  reset() forgets them; collect() synchronises the
 * device and returns the summed kernel time of the launches since reset
 * (at most 256 are remembered). */
int rt_profile_reset(rt_ctx* ctx);
int rt_profile_collect(rt_ctx* ctx, double* total_kernel_ms, uint32_t* launches);

/* Unit evaluations of single device building blocks on device `device` (parity
 * hooks for the reference's per-function golden vectors; also what the host
 * mirror's Ray::triangleIntersect / Material::evaluateColorResponse forward to).
 * Layouts (per element, 32-bit words unless noted):
 *   RT_UNIT_ASIN         in: double x                     out: double rt_asin(x)
 *   RT_UNIT_SINF/COSF    in: float x                      out: float
 *   RT_UNIT_STREAM_SEED  in: seed,domain,index,sub        out: uint32 state
 *   RT_UNIT_TRIANGLE     in: p0 p1 p2 origin dir (15 f)   out: hit(0/1 as float) u v t
 *                        (out is read first: u,v,t keep their input value where
 *                         Ray.cpp:9-24 leaves them unwritten)
 *   RT_UNIT_BSDF         in: kd alpha albedo3 f03 n3 wi3 wo3 (17 f)  out: rgb
 *   RT_UNIT_RAY_AT       in: camera(12 f) u v             out: origin3 dir3
 *   RT_UNIT_LIGHT_EVAL   in: rt_light(21 f) point3        out: rgb
 *   RT_UNIT_SAMPLERS     in: state idx N pad normal3 rt_light(21 f)  (28 words)
 *                        out: jitter xy, hemisphere dir3, light sample3, end state, pad3 (12 words)
 *   RT_UNIT_LIGHT_SAMPLE in: state rt_light(21 f) (22 words)  out: sample3, end state
 *                        (LightSource.h:46-49 randAreaPosition from a given engine state)
 *   RT_UNIT_POW          in: double x                     out: double x^2, x^5 (Material.h:38,48 pow)
 *   RT_UNIT_RECIP        in: float x                      out: the three-instruction reciprocal, 1.0f / x, the five-
 *                        instruction square root, sqrtf(x) (Ray.cpp:14's inv_det, Vec3.h:170-178's length: each pair
 *                        must agree bit for bit for 2^-100 <= |x| <= 2^100)
 *   RT_UNIT_BSDF_HOISTED in: as RT_UNIT_BSDF (17 f)       out: three rgb (9 f): the form the render kernels run — the
 *                        per-material record rt_create / rt_update make on the host, then the per-vertex and per-light
 *                        halves on the device — with the division and sqrtf, the same with the short reciprocal and
 *                        square root (the render instances' FAST flavour), and RT_UNIT_BSDF's one-piece form FAST.
 *                        FAST is only promised for vectors whose squared length is below 2^100 (rt_create vouches for
 *                        that bound before it picks a FAST instance); all three then equal RT_UNIT_BSDF bit for bit.
 *   RT_UNIT_HEMISPHERE   in: state normal3 (4 words)      out: hemisphere dir3, end state (rt_render_ao's sampler)
 */
enum {
  RT_UNIT_ASIN = 0,
  RT_UNIT_SINF = 1,
  RT_UNIT_COSF = 2,
  RT_UNIT_STREAM_SEED = 3,
  RT_UNIT_TRIANGLE = 4,
  RT_UNIT_BSDF = 5,
  RT_UNIT_RAY_AT = 6,
  RT_UNIT_LIGHT_EVAL = 7,
  RT_UNIT_SAMPLERS = 8,
  RT_UNIT_LIGHT_SAMPLE = 9,
  RT_UNIT_POW = 10,
  RT_UNIT_RECIP = 11,
  RT_UNIT_BSDF_HOISTED = 12,
  RT_UNIT_HEMISPHERE = 13
};
int rt_test_unit(int32_t device, uint32_t which, const void* in, void* out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
