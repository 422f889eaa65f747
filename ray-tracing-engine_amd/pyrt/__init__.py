"""pyrt — thin ctypes view of the C ABI (include/rt_amd.h, include/rt_host.h).

Plumbing for tests and bench.py only: every call goes straight through the
shared libraries built by ray-tracing-engine_amd/Makefile.  There is no Python
implementation of anything and no fallback: if librt_amd.so is missing, or no
gfx950 device is present, the calls raise RtError.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_PKG))
LIB_DIR = os.path.join(os.path.dirname(_PKG), "lib")
MESH_DIR = os.path.join(ROOT, "tests", "golden", "meshes")

RT_OK = 0
MODE_RAY, MODE_PATH = 0, 1
RNG_LEGACY, RNG_PIXEL = 0, 1
ACCEL_BVH, ACCEL_BRUTE = 0, 1
LENS_THIN = 0
BVH_AUTO, BVH_DEVICE, BVH_HYBRID, BVH_HOST = 0, 1, 2, 3
TRACE_CLOSEST, TRACE_ANY = 0, 1
(UNIT_ASIN, UNIT_SINF, UNIT_COSF, UNIT_STREAM_SEED, UNIT_TRIANGLE, UNIT_BSDF, UNIT_RAY_AT, UNIT_LIGHT_EVAL,
 UNIT_SAMPLERS, UNIT_LIGHT_SAMPLE, UNIT_POW, UNIT_RECIP, UNIT_BSDF_HOISTED, UNIT_HEMISPHERE) = range(14)
KMAX = 16  # rt_knn
KMAX_WIDE = 256  # rt_knn_wide and photon frames (RT_KNN_KMAX)


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rt error %d: %s" % (code, msg))
        self.code = code


class Material(C.Structure):
    _fields_ = [("kd", C.c_float), ("alpha", C.c_float), ("albedo", C.c_float * 3), ("f0", C.c_float * 3)]


class Light(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("color", C.c_float * 3), ("vertical", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("normal", C.c_float * 3), ("intensity", C.c_float),
                ("side", C.c_float), ("factor", C.c_float), ("ac", C.c_float), ("al", C.c_float), ("aq", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("lower_left", C.c_float * 3), ("horizontal", C.c_float * 3),
                ("vertical", C.c_float * 3)]


class SceneDesc(C.Structure):
    _fields_ = [("n_meshes", C.c_uint32), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32),
                ("n_lights", C.c_uint32), ("vertex_pos", C.POINTER(C.c_float)), ("vertex_nrm", C.POINTER(C.c_float)),
                ("tri_vtx", C.POINTER(C.c_uint32)), ("mesh_tri_begin", C.POINTER(C.c_uint32)),
                ("mesh_vtx_begin", C.POINTER(C.c_uint32)), ("materials", C.POINTER(Material)),
                ("lights", C.POINTER(Light)), ("camera", Camera)]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("bvh_leaf_max", C.c_uint32), ("bvh_builder", C.c_uint32), ("node_format", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class Params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("width", "height", "spp", "mode", "max_depth", "seed", "rng_mode", "accel", "use_photons", "k",
                 "photons_requested", "spp_begin", "spp_count", "rank", "world", "tile", "collect_stats")] + \
               [("reserved", C.c_uint32 * 7)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("knn_queries", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64),
                ("kd_visited", C.c_uint64), ("frame_fetches", C.c_uint64), ("kernel_ms", C.c_double), ("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class TuneReport(C.Structure):
    _fields_ = [("probes", C.c_uint32), ("accepted", C.c_uint32), ("cost_before", C.c_double), ("cost_after", C.c_double),
                ("seconds", C.c_double), ("reserved", C.c_uint64 * 4)]


class BvhInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_tri_records", C.c_uint32), ("max_depth", C.c_uint32),
                ("leaf_max", C.c_uint32), ("pad", C.c_float), ("build_ms", C.c_float), ("builder", C.c_uint32),
                ("node_format", C.c_uint32), ("flags", C.c_uint32)]


class SceneUpdate(C.Structure):
    _fields_ = [("vertex_pos", C.c_void_p), ("vertex_nrm", C.c_void_p), ("camera", C.POINTER(Camera)),
                ("lights", C.POINTER(Light)), ("n_lights", C.c_uint32), ("materials", C.POINTER(Material)),
                ("reserved", C.c_uint32 * 6)]


class UpdateReport(C.Structure):
    _fields_ = [("refitted", C.c_uint32), ("photons_dropped", C.c_uint32), ("refit_ms", C.c_double),
                ("total_ms", C.c_double), ("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class BvhQuality(C.Structure):
    _fields_ = [("cost", C.c_double), ("nodes", C.c_double), ("tris", C.c_double), ("cost_built", C.c_double),
                ("ratio", C.c_double), ("n_nodes", C.c_uint32), ("refits", C.c_uint32), ("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class RebuildParams(C.Structure):
    _fields_ = [("min_ratio", C.c_float), ("reserved", C.c_uint32 * 7)]


class RebuildReport(C.Structure):
    _fields_ = [("rebuilt", C.c_uint32), ("builder", C.c_uint32), ("ratio_before", C.c_double), ("cost_after", C.c_double),
                ("build_ms", C.c_double), ("total_ms", C.c_double), ("readback_ms", C.c_double), ("plan_ms", C.c_double),
                ("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


XF_STATIC = 1


class MeshTransform(C.Structure):
    """rt_mesh_transform: m [3][4] (positions, last column the translation), n [3][3] (normals), flags (XF_*)."""
    _fields_ = [("m", (C.c_float * 4) * 3), ("n", (C.c_float * 3) * 3), ("flags", C.c_uint32)]


class TransformUpdate(C.Structure):
    _fields_ = [("transforms", C.POINTER(MeshTransform)), ("n_meshes", C.c_uint32), ("n_lights", C.c_uint32),
                ("camera", C.POINTER(Camera)), ("lights", C.POINTER(Light)), ("d_prev_pos", C.c_void_p),
                ("reserved", C.c_uint32 * 6)]


# rt_mesh_transform as a numpy record (make_transforms)
TRANSFORM_DTYPE = np.dtype([("m", "<f4", (3, 4)), ("n", "<f4", (3, 3)), ("flags", "<u4")])


def make_transforms(n_meshes):
    """[n_meshes] rt_mesh_transform records to fill in (fields m, n, flags): identity matrices, every mesh XF_STATIC —
    clear a mesh's flags to move it."""
    t = np.zeros(n_meshes, TRANSFORM_DTYPE)
    t["m"][:, :, :3] = np.eye(3, dtype=np.float32)
    t["n"][:] = np.eye(3, dtype=np.float32)
    t["flags"] = XF_STATIC
    return t


SKIN_INFLUENCES = 4


class Skin(C.Structure):
    """rt_skin: [n_vertices][4] bone indices (uint16) and weights (float32) in host memory."""
    _fields_ = [("n_vertices", C.c_uint32), ("n_bones", C.c_uint32), ("bone", C.POINTER(C.c_uint16)),
                ("weight", C.POINTER(C.c_float)), ("reserved", C.c_uint32 * 6)]


class SkinUpdate(C.Structure):
    _fields_ = [("bones", C.POINTER(MeshTransform)), ("n_bones", C.c_uint32), ("n_lights", C.c_uint32),
                ("camera", C.POINTER(Camera)), ("lights", C.POINTER(Light)), ("d_prev_pos", C.c_void_p),
                ("reserved", C.c_uint32 * 6)]


class Aov(C.Structure):
    """rt_aov: channel pointers (host or device), None = channel not wanted."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p),
                ("hits", C.c_void_p), ("mesh", C.c_void_p), ("tri", C.c_void_p), ("reserved", C.c_uint32 * 4)]


TEX_NONE = 0xffffffff
TEX_REPEAT, TEX_CLAMP = 0, 1
TEX_NEAREST, TEX_BILINEAR = 0, 1
TEX_MAX_SIDE, TEX_MAX_UV, TEX_MAX_TEXELS = 16384, 1024.0, 1 << 28
# the `albedo` argument of the *_albedo forms (rt_amd.h RT_ALBEDO_*): the meshes' own, the resident vertex colours, the
# resident texture set
ALBEDO_MATERIAL, ALBEDO_COLORS, ALBEDO_TEXTURES = 0, 1, 2


class Texture(C.Structure):
    """rt_texture."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("wrap_s", C.c_uint32), ("wrap_t", C.c_uint32),
                ("filter", C.c_uint32), ("reserved", C.c_uint32 * 3), ("texels", C.c_void_p)]


class TextureSet(C.Structure):
    """rt_texture_set."""
    _fields_ = [("n_textures", C.c_uint32), ("n_meshes", C.c_uint32), ("n_vertices", C.c_uint32),
                ("textures", C.POINTER(Texture)), ("mesh_texture", C.c_void_p), ("vertex_uv", C.c_void_p),
                ("reserved", C.c_uint32 * 4)]


class MaterialMaps(C.Structure):
    """rt_material_maps."""
    _fields_ = [("n_meshes", C.c_uint32), ("mesh_f0", C.c_void_p), ("mesh_kd_alpha", C.c_void_p),
                ("reserved", C.c_uint32 * 5)]


def material_maps(n_meshes, mesh_f0=None, mesh_kd_alpha=None):
    """The rt_material_maps of Context.set_material_maps' arguments, and the arrays it points into (keep them alive while
    the structure is in use).  A table that is None is NULL: RT_TEX_NONE on every mesh."""
    m = MaterialMaps()
    keep = []
    m.n_meshes = n_meshes
    for field, table in (("mesh_f0", mesh_f0), ("mesh_kd_alpha", mesh_kd_alpha)):
        if table is not None:
            a = np.ascontiguousarray(table, np.uint32).reshape(-1)
            keep.append(a)
            setattr(m, field, a.ctypes.data)
    return m, keep


class NormalMaps(C.Structure):
    """rt_normal_maps."""
    _fields_ = [("n_meshes", C.c_uint32), ("mesh_normal", C.c_void_p), ("reserved", C.c_uint32 * 6)]


def normal_maps(n_meshes, mesh_normal=None):
    """The rt_normal_maps of Context.set_normal_maps' arguments, and the array it points into (keep it alive while the
    structure is in use).  A table that is None is NULL: RT_TEX_NONE on every mesh."""
    m = NormalMaps()
    keep = []
    m.n_meshes = n_meshes
    if mesh_normal is not None:
        a = np.ascontiguousarray(mesh_normal, np.uint32).reshape(-1)
        keep.append(a)
        m.mesh_normal = a.ctypes.data
    return m, keep


def texture_set(textures, mesh_texture, vertex_uv):
    """The rt_texture_set of Context.set_textures' arguments, and the arrays it points into (keep them alive while the
    structure is in use)."""
    recs = (Texture * max(len(textures), 1))()
    keep = [recs]
    for k, t in enumerate(textures):
        if isinstance(t, dict):
            t = (t["texels"], t.get("wrap_s", TEX_REPEAT), t.get("wrap_t", TEX_REPEAT), t.get("filter", TEX_BILINEAR))
        elif not isinstance(t, tuple):
            t = (t, TEX_REPEAT, TEX_REPEAT, TEX_BILINEAR)
        texels = np.ascontiguousarray(t[0], np.float32)
        if texels.ndim != 3 or texels.shape[2] != 3:
            raise ValueError("texture %d: texels must be [h][w][3], not %r" % (k, texels.shape))
        keep.append(texels)
        recs[k].height, recs[k].width = texels.shape[0], texels.shape[1]
        recs[k].wrap_s, recs[k].wrap_t, recs[k].filter = t[1], t[2], t[3]
        recs[k].texels = texels.ctypes.data
    mt = np.ascontiguousarray(mesh_texture, np.uint32).reshape(-1)
    uv = np.ascontiguousarray(vertex_uv, np.float32).reshape(-1, 2)
    keep += [mt, uv]
    ts = TextureSet()
    ts.n_textures, ts.n_meshes, ts.n_vertices = len(textures), len(mt), len(uv)
    ts.textures = C.cast(recs, C.POINTER(Texture))
    ts.mesh_texture, ts.vertex_uv = mt.ctypes.data, uv.ctypes.data
    return ts, keep


AO_MAX_RAYS = 256


class AoParams(C.Structure):
    """rt_ao_params: occlusion rays per primary hit, the origin bias (0 = 1e-4 of the scene's diagonal) and the distance
    limit (0 = unbounded)."""
    _fields_ = [("n_rays", C.c_uint32), ("bias", C.c_float), ("max_distance", C.c_float), ("reserved", C.c_uint32 * 5)]


class Ao(C.Structure):
    """rt_ao: channel pointers (host or device), None = channel not wanted."""
    _fields_ = [("unoccluded", C.c_void_p), ("hits", C.c_void_p), ("bent", C.c_void_p), ("reserved", C.c_uint32 * 4)]


class RayBatch(C.Structure):
    """rt_ray_batch: n rays (RAY_DTYPE records) and, optionally, the pixel index each ray's RNG stream is keyed by; host
    pointers for rt_render_rays, device pointers for rt_render_rays_device."""
    _fields_ = [("n", C.c_uint32), ("reserved0", C.c_uint32), ("rays", C.c_void_p), ("stream_index", C.c_void_p),
                ("reserved", C.c_uint32 * 6)]


class Lens(C.Structure):
    """rt_lens: the thin lens of rt_render_lens — its radius (0 = pinhole) and the distance of the plane of focus along
    the optical axis."""
    _fields_ = [("model", C.c_uint32), ("aperture", C.c_float), ("focus_distance", C.c_float), ("reserved", C.c_uint32 * 5)]


class Shutter(C.Structure):
    """rt_shutter: the open shutter of rt_render_shutter — the camera when it closes (the context's is the one when it
    opens), the exposure as fractions of the move, and the thin lens on the moving camera (aperture 0 = pinhole)."""
    _fields_ = [("camera_close", Camera), ("open", C.c_float), ("close", C.c_float), ("aperture", C.c_float),
                ("focus_distance", C.c_float), ("reserved", C.c_uint32 * 4)]


LIGHT_GROUPS_MAX = 4


class LightGroups(C.Structure):
    """rt_light_groups: the groups of rt_render_lights — bit l of masks[g] says that light l is lit in group g."""
    _fields_ = [("n_groups", C.c_uint32), ("masks", C.c_uint32 * LIGHT_GROUPS_MAX), ("reserved", C.c_uint32 * 3)]


PICK_SLOTS_MAX = 3


class LightPick(C.Structure):
    """rt_light_pick: `slots` light samples per path vertex, picked by the caller's importance per light (host floats) or,
    without one, by the lights' power."""
    _fields_ = [("slots", C.c_uint32), ("n_importance", C.c_uint32), ("importance", C.c_void_p), ("reserved", C.c_uint32 * 5)]


class DenoiseParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("reserved", C.c_uint32 * 6)]


class MotionPrev(C.Structure):
    """rt_motion_prev: last frame's vertex positions (host or device pointer) and camera (host), None = the context's own."""
    _fields_ = [("vertex_pos", C.c_void_p), ("camera", C.POINTER(Camera)), ("reserved", C.c_uint32 * 6)]


class MotionPrevViews(C.Structure):
    """rt_motion_prev_views: last frame's vertex positions (host or device pointer) and one camera per view (host), None =
    the context's positions / the views' own cameras."""
    _fields_ = [("vertex_pos", C.c_void_p), ("cameras", C.POINTER(Camera)), ("reserved", C.c_uint32 * 6)]


class Motion(C.Structure):
    """rt_motion: channel pointers (host or device), None = channel not wanted."""
    _fields_ = [("motion", C.c_void_p), ("position", C.c_void_p), ("prev_position", C.c_void_p), ("mesh", C.c_void_p),
                ("reserved", C.c_uint32 * 4)]


class TemporalParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_history", C.c_uint32), ("alpha_min", C.c_float),
                ("sigma_position", C.c_float), ("reserved", C.c_uint32 * 6)]


class History(C.Structure):
    """rt_history: one frame's history (host or device pointers), all four required."""
    _fields_ = [("rgb", C.c_void_p), ("position", C.c_void_p), ("mesh", C.c_void_p), ("length", C.c_void_p)]


MOTION_CHANNELS = ("motion", "position", "prev_position", "mesh")
HISTORY_CHANNELS = ("rgb", "position", "mesh", "length")


def make_temporal(width, height, max_history=0, alpha_min=0., sigma_position=0.):
    t = TemporalParams()
    t.width, t.height, t.max_history, t.alpha_min, t.sigma_position = width, height, max_history, alpha_min, sigma_position
    return t


def empty_history(width, height):
    """The history the first frame of a sequence passes: length 0 everywhere."""
    return dict(rgb=np.zeros((height, width, 3), np.float32), position=np.zeros((height, width, 3), np.float32),
                mesh=np.full((height, width), 0xffffffff, np.uint32), length=np.zeros((height, width), np.float32))


class SvgfParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("max_history", C.c_uint32),
                ("alpha_min", C.c_float), ("alpha_min_moments", C.c_float), ("sigma_luminance", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("sigma_reproject", C.c_float),
                ("reserved", C.c_uint32 * 6)]


class SvgfHistory(C.Structure):
    """rt_svgf_history: one frame's history (host or device pointers), all five required."""
    _fields_ = [("color", C.c_void_p), ("moments", C.c_void_p), ("position", C.c_void_p), ("mesh", C.c_void_p),
                ("length", C.c_void_p)]


class SvgfOut(C.Structure):
    """rt_svgf_out: output pointers (host or device); accum and variance may be None."""
    _fields_ = [("rgb", C.c_void_p), ("color", C.c_void_p), ("moments", C.c_void_p), ("length", C.c_void_p),
                ("accum", C.c_void_p), ("variance", C.c_void_p), ("reserved", C.c_uint32 * 4)]


SVGF_HISTORY_CHANNELS = ("color", "moments", "position", "mesh", "length")
SVGF_OUT_CHANNELS = (("rgb", 3), ("color", 3), ("moments", 2), ("length", 1), ("accum", 3), ("variance", 1))
SVGF_FIELDS = ("iterations", "max_history", "alpha_min", "alpha_min_moments", "sigma_luminance", "sigma_normal",
               "sigma_position", "sigma_reproject")


def make_svgf(width, height, **kw):
    """rt_svgf_params: kw of SVGF_FIELDS, 0 (the default of each) = the library's default."""
    s = SvgfParams()
    s.width, s.height = width, height
    for k, v in kw.items():
        assert k in SVGF_FIELDS, k
        setattr(s, k, v)
    return s


def empty_svgf_history(width, height):
    """The history the first frame of a sequence passes to Context.svgf: length 0 everywhere."""
    z = lambda *shape: np.zeros(shape, np.float32)
    return dict(color=z(height, width, 3), moments=z(height, width, 2), position=z(height, width, 3),
                mesh=np.full((height, width), 0xffffffff, np.uint32), length=z(height, width))


class AdaptiveParams(C.Structure):
    _fields_ = [("max_passes", C.c_uint32), ("min_passes", C.c_uint32), ("threshold", C.c_float), ("floor", C.c_float),
                ("reserved", C.c_uint32 * 6)]


class AdaptiveReport(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("granules", C.c_uint32), ("pixel_samples", C.c_uint64),
                ("active", C.c_uint32 * 64), ("render_ms", C.c_double), ("adapt_ms", C.c_double),
                ("total_ms", C.c_double), ("reserved", C.c_uint64 * 4)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("reserved", "active")}
        d["active"] = list(self.active)[:min(self.passes, 64)]
        return d


class Views(C.Structure):
    """rt_views: the cameras (and optional per-view seeds) of a multi-view frame, host memory."""
    _fields_ = [("n_views", C.c_uint32), ("reserved0", C.c_uint32), ("cameras", C.POINTER(Camera)),
                ("seeds", C.POINTER(C.c_uint32)), ("reserved", C.c_uint32 * 6)]


def make_views(cameras, seeds=None):
    """rt_views over cameras [n][4][3] (float32) and seeds [n] (uint32) or None; returns (views, arrays to keep alive)."""
    cams = np.ascontiguousarray(cameras, np.float32).reshape(-1, 12)
    v = Views()
    v.n_views = len(cams)
    v.cameras = C.cast(cams.ctypes.data, C.POINTER(Camera))
    keep = [cams]
    if seeds is not None:
        sd = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        if len(sd) != len(cams):
            raise ValueError("%d seeds for %d cameras" % (len(sd), len(cams)))
        v.seeds = C.cast(sd.ctypes.data, C.POINTER(C.c_uint32))
        keep.append(sd)
    return v, keep


def make_adaptive(threshold, max_passes, min_passes=0, floor=0.):
    a = AdaptiveParams()
    a.max_passes, a.min_passes, a.threshold, a.floor = max_passes, min_passes, threshold, floor
    return a


AOV_FLOAT3 = ("albedo", "normal", "position")
AOV_CHANNELS = ("albedo", "normal", "position", "depth", "hits", "mesh", "tri")


def aov_means(sums):
    """The means of rt_render_aov's sums: sum / hits, and 0 where hits == 0 (hits, mesh and tri as they are)."""
    hits = sums["hits"]
    out = {}
    for k, v in sums.items():
        if k in ("albedo", "normal", "position", "depth"):
            den = hits.astype(np.float32).reshape(hits.shape + (1,) * (v.ndim - 2))
            out[k] = np.where(den > 0, v / np.maximum(den, np.float32(1)), np.float32(0)).astype(np.float32)
        else:
            out[k] = v
    return out


AO_CHANNELS = ("unoccluded", "hits", "bent")


def ao_means(sums, n_rays):
    """The means of rt_render_ao's sums: ao = unoccluded / (hits * n_rays), 1 where hits == 0 (float32 [h][w]), and bent =
    bent / max(unoccluded, 1) (float32 [h][w][3])."""
    un, hits = sums["unoccluded"], sums["hits"]
    den = hits.astype(np.float32) * np.float32(n_rays)
    out = {"ao": np.where(hits > 0, un.astype(np.float32) / np.maximum(den, np.float32(1)), np.float32(1)).astype(np.float32)}
    if "bent" in sums:
        out["bent"] = (sums["bent"] / np.maximum(un, 1).astype(np.float32)[..., None]).astype(np.float32)
    return out


RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3)])
HIT_DTYPE = np.dtype([("hit", "<i4"), ("mesh", "<u4"), ("tri", "<u4"), ("vtx", "<u4", 3), ("u", "<f4"),
                      ("v", "<f4"), ("d", "<f4")])


def pixel_rays(camera, width, height):
    """The pixel-centre primary rays of a pinhole camera ([4][3]: position, lower-left corner, horizontal, vertical) on
    a width x height grid, row-major from the top row, as RAY_DTYPE [height * width]: Camera.h:27-30 in float32 at u =
    (x + 0.5) / width, v = 1 - (y + 0.5) / height, the direction left UN-normalised (rt_render_rays normalises)."""
    f = np.float32
    cam = np.asarray(camera, f).reshape(4, 3)
    u = ((np.arange(width, dtype=f) + f(0.5)) / f(width)).astype(f)
    v = (f(1) - (np.arange(height, dtype=f) + f(0.5)) / f(height)).astype(f)
    d = ((cam[1] + u[None, :, None] * cam[2]) + v[:, None, None] * cam[3]) - cam[0]
    rays = np.zeros(width * height, RAY_DTYPE)
    rays["origin"] = cam[0]
    rays["direction"] = d.astype(f).reshape(-1, 3)
    return rays


# every symbol include/rt_amd.h / include/rt_host.h declares
AMD_SYMBOLS = ["rt_abi_version", "rt_last_error", "rt_create", "rt_destroy", "rt_set_photons", "rt_emit_photons",
               "rt_render", "rt_render_passes", "rt_render_device", "rt_resolve_device", "rt_trace", "rt_knn", "rt_knn_wide", "rt_bvh_info_get",
               "rt_bvh_export", "rt_bvh_build_host", "rt_bvh_check_host", "rt_bvh_top_check_host", "rt_bvh_tune", "rt_profile_reset", "rt_profile_collect", "rt_test_unit",
               "rt_trace_stream_device", "rt_build_photon_map", "rt_get_photons", "rt_test_kd_order", "rt_owned_granules", "rt_pack_owned_device", "rt_unpack_owned_device", "rt_group_create", "rt_group_destroy",
               "rt_group_size", "rt_group_uses_rccl", "rt_group_ctx", "rt_group_set_photons", "rt_group_render",
               "rt_update", "rt_update_vertices_device", "rt_update_transforms", "rt_set_skin", "rt_update_skin", "rt_group_update", "rt_render_aov", "rt_render_aov_device",
               "rt_denoise", "rt_denoise_device", "rt_render_adaptive", "rt_render_adaptive_device", "rt_render_views",
               "rt_render_views_device", "rt_render_motion", "rt_render_motion_device", "rt_temporal_accumulate",
               "rt_temporal_accumulate_device", "rt_svgf", "rt_svgf_device", "rt_bvh_quality_get", "rt_rebuild",
               "rt_render_aov_views", "rt_render_aov_views_device", "rt_render_motion_views", "rt_render_motion_views_device",
               "rt_denoise_batch", "rt_denoise_batch_device", "rt_render_ao", "rt_render_ao_device", "rt_render_rays",
               "rt_render_rays_device", "rt_render_lens", "rt_render_lens_device", "rt_render_shutter",
               "rt_render_shutter_device", "rt_render_views_shutter", "rt_render_views_shutter_device",
               "rt_render_adaptive_shutter", "rt_render_adaptive_shutter_device", "rt_render_lights",
               "rt_render_lights_device", "rt_render_pick", "rt_render_pick_device", "rt_set_vertex_colors",
               "rt_render_colors", "rt_render_colors_device", "rt_render_aov_colors", "rt_render_aov_colors_device",
               "rt_set_textures", "rt_render_textured", "rt_render_textured_device", "rt_render_aov_textured",
               "rt_render_aov_textured_device", "rt_render_views_shutter_albedo", "rt_render_views_shutter_albedo_device",
               "rt_render_aov_views_albedo", "rt_render_aov_views_albedo_device", "rt_set_material_maps",
               "rt_render_material", "rt_render_material_device", "rt_set_normal_maps", "rt_render_normal_mapped",
               "rt_render_normal_mapped_device"]
HOST_SYMBOLS = ["rt_host_scene_build", "rt_host_scene_desc", "rt_host_scene_free", "rt_host_last_error",
                "rt_host_fill_background", "rt_host_save_ppm", "rt_host_kd_order", "rt_host_light_basis"]

_amd = None
_host = None


def make_params(width, height, spp, mode=MODE_PATH, seed=1, accel=ACCEL_BVH, max_depth=3, rng_mode=RNG_PIXEL,
                use_photons=0, k=0, photons_requested=0, spp_begin=0, spp_count=0, rank=0, world=1, tile=8,
                collect_stats=0, lanes_per_pixel=0, no_pool=False, wavefront=False):
    p = Params()
    p.width, p.height, p.spp, p.mode, p.max_depth, p.seed = width, height, spp, mode, max_depth, seed
    p.rng_mode, p.accel, p.use_photons, p.k, p.photons_requested = rng_mode, accel, use_photons, k, photons_requested
    p.spp_begin, p.spp_count, p.rank, p.world, p.tile, p.collect_stats = spp_begin, spp_count, rank, world, tile, collect_stats
    p.reserved[0] = lanes_per_pixel  # 0 = automatic; power of two <= 64: samples of a pixel a wave runs side by side
    p.reserved[1] = 1 if no_pool else 0  # schedule only: sequential shading instead of the wave's ray pool
    p.reserved[2] = 1 if wavefront else 0  # schedule only: the queue-based integrator
    return p


def make_lens(aperture, focus_distance):
    """An rt_lens: a thin lens of radius `aperture` (scene units; 0 = pinhole) focused at `focus_distance` along the
    optical axis."""
    l = Lens()
    l.model, l.aperture, l.focus_distance = LENS_THIN, aperture, focus_distance
    return l


def make_shutter(camera_close, open=0.0, close=1.0, aperture=0.0, focus_distance=0.0):
    """An rt_shutter: the camera moves from the context's to `camera_close` ([4][3]: position, lower_left, horizontal,
    vertical) and the shutter is open over [open, close] of that move; aperture > 0 puts make_lens' lens on it."""
    s = Shutter()
    cam = np.ascontiguousarray(camera_close, np.float32).reshape(12)
    C.memmove(C.byref(s.camera_close), cam.ctypes.data, 48)
    s.open, s.close, s.aperture, s.focus_distance = open, close, aperture, focus_distance
    return s


def make_light_groups(masks):
    """An rt_light_groups: one group per entry of `masks` (bit l: light l is lit in that group), in that order."""
    masks = [int(m) for m in masks]
    if len(masks) > LIGHT_GROUPS_MAX:
        raise ValueError("%d groups: rt_render_lights takes at most %d per call" % (len(masks), LIGHT_GROUPS_MAX))
    g = LightGroups()
    g.n_groups = len(masks)
    for j, m in enumerate(masks):
        g.masks[j] = m
    return g


def make_light_pick(slots, importance=None):
    """An rt_light_pick: `slots` light samples per path vertex; `importance`: one non-negative float per light of the
    context (copied; the record keeps the copy alive), or None for the default, the lights' power."""
    k = LightPick()
    k.slots = int(slots)
    if importance is not None:
        k._importance = np.ascontiguousarray(importance, np.float32).reshape(-1).copy()
        k.n_importance, k.importance = len(k._importance), k._importance.ctypes.data
    return k


def make_shutters(shutters, n):
    """The [n] rt_shutter array rt_render_views_shutter takes, from a sequence of n make_shutter records (copied)."""
    shutters = list(shutters)
    if len(shutters) != n:
        raise ValueError("%d shutter records for %d views" % (len(shutters), n))
    arr = (Shutter * n)()
    for j, s in enumerate(shutters):
        C.memmove(C.byref(arr[j]), C.byref(s), C.sizeof(Shutter))
    return arr


def amd():
    """librt_amd.so (HIP kernels + C ABI).  Loads without a GPU; compute calls then fail."""
    global _amd
    if _amd is None:
        # RT_AMD_LIB: load a diagnostic build of the same library instead (tools/phase_timing.sh)
        path = os.environ.get("RT_AMD_LIB") or os.path.join(LIB_DIR, "librt_amd.so")
        if not os.path.exists(path):
            raise RtError(-1, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        L.rt_last_error.restype = C.c_char_p
        L.rt_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(Options), C.POINTER(C.c_void_p)]
        L.rt_destroy.argtypes = [C.c_void_p]
        L.rt_destroy.restype = None
        L.rt_set_photons.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_emit_photons.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_uint32)]
        L.rt_render.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_passes.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_resolve_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        L.rt_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rt_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_knn_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_bvh_info_get.argtypes = [C.c_void_p, C.POINTER(BvhInfo)]
        L.rt_bvh_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_bvh_tune.argtypes = [C.c_void_p, C.POINTER(Params), C.c_double, C.c_uint32, C.POINTER(TuneReport)]
        L.rt_bvh_build_host.argtypes = [C.POINTER(SceneDesc), C.c_uint32, C.c_uint32, C.POINTER(BvhInfo),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.rt_bvh_check_host.argtypes = [C.POINTER(SceneDesc), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_bvh_top_check_host.argtypes = [C.POINTER(SceneDesc), C.c_uint32, C.c_uint32, C.c_void_p]
        L.rt_profile_reset.argtypes = [C.c_void_p]
        L.rt_profile_collect.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        L.rt_test_unit.argtypes = [C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_trace_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_build_photon_map.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        L.rt_get_photons.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rt_test_kd_order.argtypes = [C.c_int32, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]
        L.rt_owned_granules.argtypes = [C.POINTER(Params), C.c_uint32, C.POINTER(C.c_uint32)]
        L.rt_pack_owned_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_unpack_owned_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_group_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(Options),
                                      C.POINTER(C.c_void_p)]
        L.rt_group_destroy.argtypes = [C.c_void_p]
        L.rt_group_destroy.restype = None
        L.rt_group_size.argtypes = [C.c_void_p]
        L.rt_group_size.restype = C.c_uint32
        L.rt_group_uses_rccl.argtypes = [C.c_void_p]
        L.rt_group_ctx.argtypes = [C.c_void_p, C.c_uint32]
        L.rt_group_ctx.restype = C.c_void_p
        L.rt_group_set_photons.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_group_render.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_update.argtypes = [C.c_void_p, C.POINTER(SceneUpdate), C.POINTER(UpdateReport)]
        L.rt_update_vertices_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(UpdateReport)]
        L.rt_update_transforms.argtypes = [C.c_void_p, C.POINTER(TransformUpdate), C.c_void_p, C.POINTER(UpdateReport)]
        L.rt_set_skin.argtypes = [C.c_void_p, C.POINTER(Skin)]
        L.rt_update_skin.argtypes = [C.c_void_p, C.POINTER(SkinUpdate), C.c_void_p, C.POINTER(UpdateReport)]
        L.rt_group_update.argtypes = [C.c_void_p, C.POINTER(SceneUpdate), C.POINTER(UpdateReport)]
        L.rt_bvh_quality_get.argtypes = [C.c_void_p, C.POINTER(BvhQuality)]
        L.rt_rebuild.argtypes = [C.c_void_p, C.POINTER(RebuildParams), C.POINTER(RebuildReport)]
        L.rt_render_aov.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Aov)]
        L.rt_render_aov_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Aov), C.c_void_p]
        L.rt_render_aov_colors.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Aov)]
        L.rt_render_aov_colors_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Aov), C.c_void_p]
        L.rt_set_vertex_colors.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_render_colors.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_colors_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_aov_textured.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Aov)]
        L.rt_render_aov_textured_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Aov), C.c_void_p]
        L.rt_set_textures.argtypes = [C.c_void_p, C.POINTER(TextureSet)]
        L.rt_render_textured.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_textured_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_ao.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AoParams), C.POINTER(Ao)]
        L.rt_render_ao_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AoParams), C.POINTER(Ao), C.c_void_p]
        L.rt_render_rays.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(RayBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(Stats)]
        L.rt_render_rays_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(RayBatch), C.c_void_p, C.c_void_p,
                                            C.POINTER(Stats)]
        L.rt_render_lens.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Lens), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(Stats)]
        L.rt_render_lens_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Lens), C.c_void_p, C.c_void_p,
                                            C.POINTER(Stats)]
        L.rt_render_shutter.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Shutter), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(Stats)]
        L.rt_render_shutter_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Shutter), C.c_void_p, C.c_void_p,
                                               C.POINTER(Stats)]
        L.rt_render_lights.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(LightGroups), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(Stats)]
        L.rt_render_pick.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(LightPick), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(Stats)]
        L.rt_render_pick_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(LightPick), C.c_void_p, C.c_void_p,
                                            C.POINTER(Stats)]
        L.rt_render_lights_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(LightGroups), C.c_void_p, C.c_void_p,
                                              C.POINTER(Stats)]
        L.rt_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(Aov), C.c_void_p]
        L.rt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AdaptiveParams), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.POINTER(AdaptiveReport), C.POINTER(Stats)]
        L.rt_render_adaptive_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AdaptiveParams), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdaptiveReport),
                                                C.POINTER(Stats)]
        L.rt_render_views.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(Stats)]
        L.rt_render_views_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.c_void_p, C.c_void_p,
                                             C.POINTER(Stats)]
        L.rt_render_views_shutter.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.POINTER(Shutter), C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_views_shutter_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.POINTER(Shutter),
                                                     C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_views_shutter_albedo.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.POINTER(Shutter),
                                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_views_shutter_albedo_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.POINTER(Shutter),
                                                            C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_set_material_maps.argtypes = [C.c_void_p, C.POINTER(MaterialMaps)]
        L.rt_render_material.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_material_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_set_normal_maps.argtypes = [C.c_void_p, C.POINTER(NormalMaps)]
        L.rt_render_normal_mapped.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_normal_mapped_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rt_render_aov_views_albedo.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.c_uint32, C.POINTER(Aov)]
        L.rt_render_aov_views_albedo_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.c_uint32,
                                                        C.POINTER(Aov), C.c_void_p]
        L.rt_render_adaptive_shutter.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AdaptiveParams), C.POINTER(Shutter),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdaptiveReport),
                                                 C.POINTER(Stats)]
        L.rt_render_adaptive_shutter_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(AdaptiveParams),
                                                        C.POINTER(Shutter), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.POINTER(AdaptiveReport), C.POINTER(Stats)]
        L.rt_denoise_device.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(Aov), C.c_void_p,
                                        C.c_void_p]
        L.rt_render_motion.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(MotionPrev), C.POINTER(Motion)]
        L.rt_render_motion_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(MotionPrev), C.POINTER(Motion),
                                              C.c_void_p]
        L.rt_temporal_accumulate.argtypes = [C.c_void_p, C.POINTER(TemporalParams), C.c_void_p, C.POINTER(Motion),
                                             C.POINTER(History), C.c_void_p, C.c_void_p]
        L.rt_temporal_accumulate_device.argtypes = [C.c_void_p, C.POINTER(TemporalParams), C.c_void_p, C.POINTER(Motion),
                                                    C.POINTER(History), C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_svgf.argtypes = [C.c_void_p, C.POINTER(SvgfParams), C.c_void_p, C.POINTER(Aov), C.POINTER(Motion),
                              C.POINTER(SvgfHistory), C.POINTER(SvgfOut)]
        L.rt_svgf_device.argtypes = L.rt_svgf.argtypes + [C.c_void_p]
        views_aov = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.POINTER(Aov)]
        views_motion = [C.c_void_p, C.POINTER(Params), C.POINTER(Views), C.POINTER(MotionPrevViews), C.POINTER(Motion)]
        batch = [C.c_void_p, C.POINTER(DenoiseParams), C.c_uint32, C.c_void_p, C.POINTER(Aov), C.c_void_p]
        for name, types in (("rt_render_aov_views", views_aov), ("rt_render_aov_views_device", views_aov + [C.c_void_p]),
                            ("rt_render_motion_views", views_motion), ("rt_render_motion_views_device", views_motion + [C.c_void_p]),
                            ("rt_denoise_batch", batch), ("rt_denoise_batch_device", batch + [C.c_void_p])):
            # (a library named by RT_AMD_LIB may be an older build without them, as tools/aov_views_bench.py times the
            # per-view loop on; the package's own library must have every one)
            if hasattr(L, name) or not os.environ.get("RT_AMD_LIB"):
                getattr(L, name).argtypes = types
        _amd = L
    return _amd


def host():
    """librt_host.so (scene script, OFF loader, flattener, background, kd order)."""
    global _host
    if _host is None:
        amd()  # dependency, resolved through rpath as well
        path = os.path.join(LIB_DIR, "librt_host.so")
        if not os.path.exists(path):
            raise RtError(-1, "%s not built" % path)
        L = C.CDLL(path)
        L.rt_host_last_error.restype = C.c_char_p
        L.rt_host_scene_build.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.rt_host_scene_desc.argtypes = [C.c_void_p]
        L.rt_host_scene_desc.restype = C.POINTER(SceneDesc)
        L.rt_host_scene_free.argtypes = [C.c_void_p]
        L.rt_host_scene_free.restype = None
        L.rt_host_fill_background.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.rt_host_fill_background.restype = None
        L.rt_host_save_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rt_host_kd_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_host_light_basis.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _host = L
    return _host


def _check(rc):
    if rc != RT_OK:
        raise RtError(rc, amd().rt_last_error().decode())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Scene:
    """A flattened preset scene (host/ScenePresets.h) owned by librt_host."""

    def __init__(self, kind, width, height, mesh_dir=MESH_DIR):
        h = C.c_void_p()
        rc = host().rt_host_scene_build(kind.encode(), mesh_dir.encode(), width, height, C.byref(h))
        if rc != RT_OK:
            raise RtError(rc, host().rt_host_last_error().decode())
        self._h = h
        self.kind, self.width, self.height = kind, width, height
        self.desc_ptr = host().rt_host_scene_desc(h)
        self.desc = self.desc_ptr.contents

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _host is not None:
            _host.rt_host_scene_free(h)

    def __del__(self):
        try:  # at interpreter exit module globals / ctypes may already be torn down
            self.close()
        except Exception:
            pass

    def arrays(self):
        d = self.desc
        nv, nt, nm = d.n_vertices, d.n_triangles, d.n_meshes
        return dict(
            pos=np.ctypeslib.as_array(d.vertex_pos, (nv, 3)).copy(),
            nrm=np.ctypeslib.as_array(d.vertex_nrm, (nv, 3)).copy(),
            tri=np.ctypeslib.as_array(d.tri_vtx, (nt, 3)).copy(),
            tri_begin=np.ctypeslib.as_array(d.mesh_tri_begin, (nm + 1,)).copy(),
            vtx_begin=np.ctypeslib.as_array(d.mesh_vtx_begin, (nm + 1,)).copy(),
            materials=np.frombuffer(C.string_at(d.materials, 32 * nm), dtype="<f4").reshape(nm, 8).copy(),
            lights=np.frombuffer(C.string_at(d.lights, 84 * d.n_lights), dtype="<f4").reshape(d.n_lights, 21).copy(),
            camera=np.frombuffer(bytes(d.camera), dtype="<f4").reshape(4, 3).copy())


def background(width, height):
    bg = np.empty((height, width, 3), np.float32)
    host().rt_host_fill_background(_ptr(bg), width, height)
    return bg


def bvh_build_host(scene, leaf_max=0, threads=0):
    """The host BVH build alone (no GPU): (BvhInfo, digest, seconds)."""
    info, dig, sec = BvhInfo(), C.c_uint64(0), C.c_double(0)
    _check(amd().rt_bvh_build_host(C.byref(scene.desc), leaf_max, threads, C.byref(info), C.byref(dig), C.byref(sec)))
    return info, dig.value, sec.value


NODES_AUTO, NODES_F16, NODES_Q8 = 0, 1, 2


def bvh_check_host(scene, leaf_max=0, node_format=NODES_F16):
    """Host build + packing into the given device node format + structural check (no GPU).  Returns a dict of the
    shape numbers; raises RtError when the packed tree is not a valid tree over the scene's triangles."""
    out = np.zeros(8, np.uint32)
    est = np.zeros(2, np.float64)
    _check(amd().rt_bvh_check_host(C.byref(scene.desc), leaf_max, node_format, _ptr(out), _ptr(est)))
    return dict(nodes=int(out[0]), slots=int(out[1]), blocks=int(out[2]), depth=int(out[3]), added_nodes=int(out[4]),
                visits_float=float(est[0]), visits_packed=float(est[1]))


def bvh_top_check_host(scene, leaf_max=0, cutoff=1024):
    """The hybrid builder's host half (rtbvh::buildTop) alone, validated (no GPU).  Returns a dict of the shape numbers."""
    out = np.zeros(8, np.uint32)
    _check(amd().rt_bvh_top_check_host(C.byref(scene.desc), leaf_max, cutoff, _ptr(out)))
    return dict(top_nodes=int(out[0]), parts=int(out[1]), largest_part=int(out[2]), deepest_part=int(out[3]), depth_cap=int(out[4]),
                top_leaves=int(out[5]))


def kd_order(pos, dir_, weight=None):
    """kdtree::make_tree order (in place on copies); returns (pos, dir, weight)."""
    pos = np.ascontiguousarray(pos, np.float32).copy()
    dir_ = np.ascontiguousarray(dir_, np.float32).copy()
    w = None if weight is None else np.ascontiguousarray(weight, np.float32).copy()
    rc = host().rt_host_kd_order(_ptr(pos), _ptr(dir_), _ptr(w), len(pos))
    if rc != RT_OK:
        raise RtError(rc, host().rt_host_last_error().decode())
    return pos, dir_, w


def light_basis(position, direction):
    """The basis the host's LightSource constructor derives for lights at position [n][3] aimed at direction [n][3]:
    [n][9] = vertical, horizontal, normal (the order of rt_light)."""
    pos = np.ascontiguousarray(position, np.float32).reshape(-1, 3)
    dir_ = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    out = np.zeros((len(pos), 9), np.float32)
    for i in range(len(pos)):
        rc = host().rt_host_light_basis(_ptr(pos[i]), _ptr(dir_[i]), _ptr(out[i]))
        if rc != RT_OK:
            raise RtError(rc, host().rt_host_last_error().decode())
    return out


def _scene_update(pos, nrm, camera, lights, materials):
    """An rt_scene_update over numpy arrays (None = unchanged); returns it and the arrays it points into.
    camera: [4][3] floats (position, lower_left, horizontal, vertical), lights: [n][21], materials: [n_meshes][8]."""
    u = SceneUpdate()
    keep = []

    def arr(a, cols):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, cols)
        keep.append(a)
        return a
    if pos is not None:
        u.vertex_pos = arr(pos, 3).ctypes.data
    if nrm is not None:
        u.vertex_nrm = arr(nrm, 3).ctypes.data
    if camera is not None:
        u.camera = C.cast(arr(camera, 3).ctypes.data, C.POINTER(Camera))
    if lights is not None:
        a = arr(lights, 21)
        # (a non-null pointer even for zero lights: NULL means "unchanged")
        u.lights = C.cast(a.ctypes.data if len(a) else C.addressof(_NO_LIGHT), C.POINTER(Light))
        u.n_lights = len(a)
    if materials is not None:
        u.materials = C.cast(arr(materials, 8).ctypes.data, C.POINTER(Material))
    return u, keep


_NO_LIGHT = Light()


class Context:
    """rt_ctx: the scene resident in HBM on one gfx950 device."""

    def __init__(self, scene, device=0, bvh_leaf_max=0, bvh_builder=0, node_format=0):
        self.scene = scene
        opt = Options()
        opt.device, opt.bvh_leaf_max, opt.bvh_builder, opt.node_format = device, bvh_leaf_max, bvh_builder, node_format
        h = C.c_void_p()
        _check(amd().rt_create(scene.desc_ptr, C.byref(opt), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            amd().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:  # at interpreter exit module globals / ctypes may already be torn down
            self.close()
        except Exception:
            pass

    def bvh_info(self):
        bi = BvhInfo()
        _check(amd().rt_bvh_info_get(self._h, C.byref(bi)))
        return bi

    def tune(self, probe_params, budget_seconds, max_probes=0):
        """rt_bvh_tune: measured-cost tuning of the host-built tree against the rays of `probe_params`."""
        rep = TuneReport()
        _check(amd().rt_bvh_tune(self._h, C.byref(probe_params), float(budget_seconds), int(max_probes), C.byref(rep)))
        return rep

    def update(self, pos=None, nrm=None, camera=None, lights=None, materials=None):
        """rt_update: the resident scene follows the given arrays (None = unchanged; pos / nrm [n_vertices][3],
        camera [4][3], lights [n][21], materials [n_meshes][8]).  Returns the report as a dict."""
        u, _keep = _scene_update(pos, nrm, camera, lights, materials)
        rep = UpdateReport()
        _check(amd().rt_update(self._h, C.byref(u), C.byref(rep)))
        return rep.as_dict()

    def update_vertices_device(self, d_pos, d_nrm, stream=0):
        """rt_update_vertices_device: positions / normals already in device memory (pointers, 0 = unchanged), ordered
        on `stream`.  Returns the report as a dict."""
        rep = UpdateReport()
        _check(amd().rt_update_vertices_device(self._h, C.c_void_p(d_pos or None), C.c_void_p(d_nrm or None),
                                               C.c_void_p(stream or None), C.byref(rep)))
        return rep.as_dict()

    def update_transforms(self, transforms, camera=None, lights=None, d_prev_pos=None, stream=0):
        """rt_update_transforms: the rest pose under one record per mesh (make_transforms' array, or anything of its
        layout), computed on the device; camera / lights as update's.  d_prev_pos: a device pointer [n_vertices][3] that
        receives the positions this call replaces (render_motion_device's d_prev_pos), ordered on `stream`.  Returns the
        report as a dict."""
        t = np.ascontiguousarray(transforms, TRANSFORM_DTYPE).reshape(-1)
        u, _keep = _scene_update(None, None, camera, lights, None)
        x = TransformUpdate()
        x.transforms = C.cast(t.ctypes.data, C.POINTER(MeshTransform))
        x.n_meshes, x.n_lights, x.camera, x.lights = len(t), u.n_lights, u.camera, u.lights
        x.d_prev_pos = int(d_prev_pos) if d_prev_pos else None
        rep = UpdateReport()
        _check(amd().rt_update_transforms(self._h, C.byref(x), C.c_void_p(stream or None), C.byref(rep)))
        return rep.as_dict()

    def set_skin(self, bone, weight, n_bones):
        """rt_set_skin: bone [n_vertices][4] indices below n_bones and weight [n_vertices][4] become the resident skin
        (a zero weight = the slot is unused)."""
        b = np.ascontiguousarray(bone, np.uint16)
        w = np.ascontiguousarray(weight, np.float32)
        if b.ndim != 2 or b.shape[1] != SKIN_INFLUENCES or w.shape != b.shape:
            raise ValueError("bone and weight must both be [n_vertices][%d]" % SKIN_INFLUENCES)
        s = Skin()
        s.n_vertices, s.n_bones = len(b), int(n_bones)
        s.bone, s.weight = C.cast(b.ctypes.data, C.POINTER(C.c_uint16)), C.cast(w.ctypes.data, C.POINTER(C.c_float))
        _check(amd().rt_set_skin(self._h, C.byref(s)))

    def clear_skin(self):
        """rt_set_skin(ctx, NULL): the resident skin is released."""
        _check(amd().rt_set_skin(self._h, None))

    def update_skin(self, bones, camera=None, lights=None, d_prev_pos=None, stream=0):
        """rt_update_skin: the rest pose blended under one record per bone of the resident skin (make_transforms' layout
        with flags 0), computed on the device; camera / lights / d_prev_pos / stream as update_transforms'.  Returns the
        report as a dict."""
        t = np.ascontiguousarray(bones, TRANSFORM_DTYPE).reshape(-1)
        u, _keep = _scene_update(None, None, camera, lights, None)
        x = SkinUpdate()
        x.bones = C.cast(t.ctypes.data, C.POINTER(MeshTransform))
        x.n_bones, x.n_lights, x.camera, x.lights = len(t), u.n_lights, u.camera, u.lights
        x.d_prev_pos = int(d_prev_pos) if d_prev_pos else None
        rep = UpdateReport()
        _check(amd().rt_update_skin(self._h, C.byref(x), C.c_void_p(stream or None), C.byref(rep)))
        return rep.as_dict()

    def bvh_quality(self):
        """rt_bvh_quality_get: the surface-area cost of the resident tree (cost, nodes, tris), the same measure of the tree
        as last built (cost_built), their ratio, n_nodes and the refits since the build, as a dict."""
        q = BvhQuality()
        _check(amd().rt_bvh_quality_get(self._h, C.byref(q)))
        return q.as_dict()

    def rebuild(self, min_ratio=0.0):
        """rt_rebuild: the tree built again from the resident arrays — always (min_ratio 0), or only if bvh_quality's
        ratio has reached min_ratio (>= 1).  Returns the report as a dict."""
        p = RebuildParams()
        p.min_ratio = min_ratio
        rep = RebuildReport()
        _check(amd().rt_rebuild(self._h, C.byref(p), C.byref(rep)))
        return rep.as_dict()

    def bvh_export(self):
        bi = self.bvh_info()
        nodes = np.empty((bi.n_nodes, 16), np.uint32)
        tris = np.empty((bi.n_tri_records, 12), np.uint32)
        _check(amd().rt_bvh_export(self._h, _ptr(nodes), _ptr(tris)))
        return nodes, tris

    def set_photons(self, pos, dir_):
        pos = np.ascontiguousarray(pos, np.float32)
        dir_ = np.ascontiguousarray(dir_, np.float32)
        _check(amd().rt_set_photons(self._h, _ptr(pos), _ptr(dir_), len(pos)))

    def emit_photons(self, n_requested, seed=1):
        pos = np.zeros((max(n_requested, 1), 3), np.float32)
        dir_ = np.zeros_like(pos)
        w = np.zeros(max(n_requested, 1), np.float32)
        n = C.c_uint32()
        _check(amd().rt_emit_photons(self._h, n_requested, seed, _ptr(pos), _ptr(dir_), _ptr(w), C.byref(n)))
        return pos[:n.value].copy(), dir_[:n.value].copy(), w[:n.value].copy()

    def build_photon_map(self, n_requested, seed=1):
        """Emission + compaction + kd order on the device; returns (n_stored, [emit_ms, kd_ms])."""
        n = C.c_uint32()
        ms = (C.c_double * 2)()
        _check(amd().rt_build_photon_map(self._h, n_requested, seed, C.byref(n), ms))
        return n.value, [ms[0], ms[1]]

    def get_photons(self, cap):
        pos = np.zeros((max(cap, 1), 3), np.float32)
        dir_ = np.zeros_like(pos)
        w = np.zeros(max(cap, 1), np.float32)
        n = C.c_uint32()
        _check(amd().rt_get_photons(self._h, _ptr(pos), _ptr(dir_), _ptr(w), cap, C.byref(n)))
        return pos[:n.value].copy(), dir_[:n.value].copy(), w[:n.value].copy()

    def render(self, params, bg=None, want_accum=True):
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render(self._h, C.byref(params), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_passes(self, params, bg, accum_io):
        """rt_render_passes: integrate params.spp_begin/spp_count on top of accum_io (in place)
        and resolve the running estimate; returns (out_rgb, stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32)
        st = Stats()
        bgc = np.ascontiguousarray(bg, np.float32)
        assert accum_io.dtype == np.float32 and accum_io.flags["C_CONTIGUOUS"] and accum_io.shape == (h, w, 4)
        _check(amd().rt_render_passes(self._h, C.byref(params), _ptr(bgc), _ptr(accum_io), _ptr(out), C.byref(st)))
        return out, st

    def render_device(self, params, d_accum_ptr, stream=0, stats=False):
        st = Stats() if stats else None
        _check(amd().rt_render_device(self._h, C.byref(params), C.c_void_p(d_accum_ptr), C.c_void_p(stream),
                                      C.byref(st) if stats else None))
        return st

    def render_views(self, params, cameras, bg=None, seeds=None, want_accum=True):
        """rt_render_views: the frames of cameras [n][4][3] (seeds [n] or None = params.seed) in one launch; returns
        (out [n][h][w][3] or None without bg, accum [n][h][w][4] or None, stats)."""
        v, _keep = make_views(cameras, seeds)
        w, h, n = params.width, params.height, v.n_views
        out = np.empty((n, h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((n, h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_views(self._h, C.byref(params), C.byref(v), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_views_device(self, params, cameras, d_accum_ptr, stream=0, seeds=None, stats=False):
        """rt_render_views_device: accumulate into the caller-zeroed device d_accum [n][h][w][4] on `stream`."""
        v, _keep = make_views(cameras, seeds)
        st = Stats() if stats else None
        _check(amd().rt_render_views_device(self._h, C.byref(params), C.byref(v), C.c_void_p(d_accum_ptr),
                                            C.c_void_p(stream), C.byref(st) if stats else None))
        return st

    def resolve_device(self, width, height, spp, d_accum_ptr, d_bg_ptr, d_out_ptr, stream=0):
        _check(amd().rt_resolve_device(self._h, width, height, spp, C.c_void_p(d_accum_ptr), C.c_void_p(d_bg_ptr),
                                       C.c_void_p(d_out_ptr), C.c_void_p(stream)))

    def trace_stream_device(self, d_ray_o, d_ray_d, n, d_res, stream=0):
        _check(amd().rt_trace_stream_device(self._h, C.c_void_p(d_ray_o), C.c_void_p(d_ray_d), n, C.c_void_p(d_res),
                                            C.c_void_p(stream)))

    def pack_owned(self, params, d_accum_ptr, d_packed_ptr, stream=0):
        _check(amd().rt_pack_owned_device(self._h, C.byref(params), C.c_void_p(d_accum_ptr), C.c_void_p(d_packed_ptr),
                                          C.c_void_p(stream)))

    def unpack_owned(self, params, from_rank, d_packed_ptr, d_accum_ptr, stream=0):
        _check(amd().rt_unpack_owned_device(self._h, C.byref(params), from_rank, C.c_void_p(d_packed_ptr),
                                            C.c_void_p(d_accum_ptr), C.c_void_p(stream)))

    def profile_reset(self):
        _check(amd().rt_profile_reset(self._h))

    def profile_collect(self):
        ms, n = C.c_double(), C.c_uint32()
        _check(amd().rt_profile_collect(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def trace(self, rays, accel=ACCEL_BVH, kind=TRACE_CLOSEST):
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        _check(amd().rt_trace(self._h, _ptr(rays), len(rays), accel, kind, _ptr(hits)))
        return hits

    def render_aov(self, params, raw=False, channels=AOV_CHANNELS, colors=False, textured=False):
        """rt_render_aov: first-hit AOVs of the frame `params` describes, as a dict of numpy arrays ([h][w][3] albedo,
        normal, position; [h][w] depth, hits, mesh, tri).  The means (sum / hits, 0 where hits == 0); raw=True: the
        sums rt_render_aov returns.  `channels`: the ones wanted (the others are not computed).  colors:
        rt_render_aov_colors, whose albedo channel is the interpolated vertex colour; textured: rt_render_aov_textured,
        whose albedo channel is the texture sample."""
        w, h = params.width, params.height
        if not raw and "hits" not in channels:
            channels = tuple(channels) + ("hits",)  # (the means divide by it)
        sums = {}
        a = Aov()
        for k in channels:
            arr = np.zeros((h, w, 3) if k in AOV_FLOAT3 else (h, w), np.float32 if k in AOV_FLOAT3 or k == "depth" else np.uint32)
            sums[k] = arr
            setattr(a, k, arr.ctypes.data)
        f = amd().rt_render_aov_textured if textured else amd().rt_render_aov_colors if colors else amd().rt_render_aov
        _check(f(self._h, C.byref(params), C.byref(a)))
        return sums if raw else aov_means(sums)

    def render_aov_device(self, params, ptrs, stream=0, colors=False, textured=False):
        """rt_render_aov_device: the sums into device buffers; ptrs = {channel: device pointer} (missing = not wanted).
        colors: rt_render_aov_colors_device; textured: rt_render_aov_textured_device."""
        a = Aov()
        for k, v in ptrs.items():
            setattr(a, k, v or None)
        f = (amd().rt_render_aov_textured_device if textured else amd().rt_render_aov_colors_device if colors
             else amd().rt_render_aov_device)
        _check(f(self._h, C.byref(params), C.byref(a), C.c_void_p(stream or None)))

    def render_aov_colors(self, params, raw=False, channels=AOV_CHANNELS):
        """rt_render_aov_colors: render_aov with the albedo channel from the resident vertex colours."""
        return self.render_aov(params, raw, channels, colors=True)

    def render_aov_colors_device(self, params, ptrs, stream=0):
        """rt_render_aov_colors_device: render_aov_device with the albedo channel from the resident vertex colours."""
        self.render_aov_device(params, ptrs, stream, colors=True)

    def set_vertex_colors(self, rgb):
        """rt_set_vertex_colors: rgb [n_vertices][3] floats become the resident per-vertex albedo (copied); None releases
        it."""
        if rgb is None:
            _check(amd().rt_set_vertex_colors(self._h, None, 0))
            return
        rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
        _check(amd().rt_set_vertex_colors(self._h, _ptr(rgb), len(rgb)))

    def render_colors(self, params, bg=None, want_accum=True):
        """rt_render_colors: the frame with the resident per-vertex albedo; returns (out [h][w][3] or None without bg,
        accum [h][w][4] or None, stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_colors(self._h, C.byref(params), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_colors_device(self, params, d_accum, stream=0, stats=False):
        """rt_render_colors_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample ranges
        chain."""
        st = Stats() if stats else None
        _check(amd().rt_render_colors_device(self._h, C.byref(params), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                             C.byref(st) if stats else None))
        return st

    def render_aov_textured(self, params, raw=False, channels=AOV_CHANNELS):
        """rt_render_aov_textured: render_aov with the albedo channel from the resident textures."""
        return self.render_aov(params, raw, channels, textured=True)

    def render_aov_textured_device(self, params, ptrs, stream=0):
        """rt_render_aov_textured_device: render_aov_device with the albedo channel from the resident textures."""
        self.render_aov_device(params, ptrs, stream, textured=True)

    def set_textures(self, textures, mesh_texture=None, vertex_uv=None):
        """rt_set_textures: the set becomes resident (copied); set_textures(None) releases it.  textures: a list whose
        entries are an [h][w][3] float array (repeat, bilinear) or a dict(texels=..., wrap_s=, wrap_t=, filter=) or a tuple
        (texels, wrap_s, wrap_t, filter); mesh_texture [n_meshes]: a texture index or TEX_NONE; vertex_uv
        [n_vertices][2] by global vertex id."""
        if textures is None:
            _check(amd().rt_set_textures(self._h, None))
            return
        ts, keep = texture_set(textures, mesh_texture, vertex_uv)
        _check(amd().rt_set_textures(self._h, C.byref(ts)))

    def render_textured(self, params, bg=None, want_accum=True):
        """rt_render_textured: the frame with the resident textures as albedo; returns (out [h][w][3] or None without
        bg, accum [h][w][4] or None, stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_textured(self._h, C.byref(params), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def set_material_maps(self, mesh_f0=None, mesh_kd_alpha=None, release=False, n_meshes=None):
        """rt_set_material_maps: per mesh, the texture of the RESIDENT set (an index, or TEX_NONE) that gives f0 (rgb) and
        the one that gives kd (r) and alpha (g); either may be None (TEX_NONE on every mesh).  release=True releases the
        maps.  n_meshes: the count the call states (the length of a given table, else the context's)."""
        if release:
            _check(amd().rt_set_material_maps(self._h, None))
            return
        if n_meshes is None:
            given = mesh_f0 if mesh_f0 is not None else mesh_kd_alpha
            n_meshes = len(given) if given is not None else self.scene.desc.n_meshes
        m, keep = material_maps(n_meshes, mesh_f0, mesh_kd_alpha)
        _check(amd().rt_set_material_maps(self._h, C.byref(m)))

    def render_material(self, params, bg=None, want_accum=True):
        """rt_render_material: the textured frame with f0 and (kd, alpha) from the resident material maps; returns (out
        [h][w][3] or None without bg, accum [h][w][4] or None, stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_material(self._h, C.byref(params), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_material_device(self, params, d_accum, stream=0, stats=False):
        """rt_render_material_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample
        ranges chain."""
        st = Stats() if stats else None
        _check(amd().rt_render_material_device(self._h, C.byref(params), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                               C.byref(st) if stats else None))
        return st

    def set_normal_maps(self, mesh_normal=None, release=False, n_meshes=None):
        """rt_set_normal_maps: per mesh, the texture of the RESIDENT set (an index, or TEX_NONE) whose rgb gives the
        tangent-space normal (2 c - 1) that turns the shading normal; None: TEX_NONE on every mesh.  release=True releases
        the maps.  n_meshes: the count the call states (the length of a given table, else the context's)."""
        if release:
            _check(amd().rt_set_normal_maps(self._h, None))
            return
        if n_meshes is None:
            n_meshes = len(mesh_normal) if mesh_normal is not None else self.scene.desc.n_meshes
        m, keep = normal_maps(n_meshes, mesh_normal)
        _check(amd().rt_set_normal_maps(self._h, C.byref(m)))

    def render_normal_mapped(self, params, bg=None, want_accum=True):
        """rt_render_normal_mapped: the material-map frame (with or without resident material maps) with every shaded
        vertex's normal turned by the resident normal maps; returns (out [h][w][3] or None without bg, accum [h][w][4] or
        None, stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_normal_mapped(self._h, C.byref(params), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_normal_mapped_device(self, params, d_accum, stream=0, stats=False):
        """rt_render_normal_mapped_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample
        ranges chain."""
        st = Stats() if stats else None
        _check(amd().rt_render_normal_mapped_device(self._h, C.byref(params), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                                    C.byref(st) if stats else None))
        return st

    def render_textured_device(self, params, d_accum, stream=0, stats=False):
        """rt_render_textured_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample
        ranges chain."""
        st = Stats() if stats else None
        _check(amd().rt_render_textured_device(self._h, C.byref(params), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                               C.byref(st) if stats else None))
        return st

    @staticmethod
    def _ao_params(n_rays, bias, max_distance):
        a = AoParams()
        a.n_rays, a.bias, a.max_distance = n_rays, bias, max_distance
        return a

    def render_ao(self, params, n_rays, bias=0., max_distance=0., channels=AO_CHANNELS):
        """rt_render_ao: n_rays occlusion rays at every primary hit of the frame `params` describes.  The SUMS as a dict
        of numpy arrays: unoccluded, hits [h][w] uint32 and bent [h][w][3] float32 (ao_means turns them into means).
        bias 0: 1e-4 of the scene's diagonal; max_distance 0: unbounded.  `channels`: the ones wanted."""
        w, h = params.width, params.height
        sums, o = {}, Ao()
        for k in channels:
            sums[k] = np.zeros((h, w, 3), np.float32) if k == "bent" else np.zeros((h, w), np.uint32)
            setattr(o, k, sums[k].ctypes.data)
        _check(amd().rt_render_ao(self._h, C.byref(params), C.byref(self._ao_params(n_rays, bias, max_distance)), C.byref(o)))
        return sums

    def render_ao_device(self, params, n_rays, ptrs, bias=0., max_distance=0., stream=0):
        """rt_render_ao_device: the sums into device buffers; ptrs = {channel: device pointer} (missing = not wanted)."""
        o = Ao()
        for k, v in ptrs.items():
            setattr(o, k, v or None)
        _check(amd().rt_render_ao_device(self._h, C.byref(params), C.byref(self._ao_params(n_rays, bias, max_distance)), C.byref(o),
                                         C.c_void_p(stream or None)))

    def render_rays(self, params, rays, bg=None, stream_index=None, want_accum=True):
        """rt_render_rays: the integrator along `rays` (RAY_DTYPE [n], directions of any length) in place of a camera's
        pixel grid; params.width / height are ignored.  stream_index [n] uint32: the pixel index each ray's RNG stream is
        keyed by (None: the ray's own index).  Returns (out [n][3] or None without bg [n][3], accum [n][4] or None, stats)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
        n = len(rays)
        idx = None if stream_index is None else np.ascontiguousarray(stream_index, np.uint32).reshape(-1)
        assert idx is None or len(idx) == n
        b = RayBatch()
        b.n, b.rays, b.stream_index = n, rays.ctypes.data, None if idx is None else idx.ctypes.data
        out = np.empty((n, 3), np.float32) if bg is not None else None
        acc = np.empty((n, 4), np.float32) if want_accum else None
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        assert bgc is None or bgc.size == 3 * n
        st = Stats()
        _check(amd().rt_render_rays(self._h, C.byref(params), C.byref(b), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_rays_device(self, params, d_rays, n, d_accum, d_stream_index=None, stream=0, stats=False):
        """rt_render_rays_device: accumulate the rays at device pointer d_rays ([n] rt_ray) into the caller-zeroed device
        d_accum [n][4] on `stream`; sample ranges chain.  Resolve with resolve_device(n, 1, spp, ...)."""
        b = RayBatch()
        b.n, b.rays, b.stream_index = n, d_rays, d_stream_index or None
        st = Stats() if stats else None
        _check(amd().rt_render_rays_device(self._h, C.byref(params), C.byref(b), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                           C.byref(st) if stats else None))
        return st

    def render_lens(self, params, lens, bg=None, want_accum=True):
        """rt_render_lens: the frame through the thin lens `lens` (make_lens); returns (out or None without bg, accum or
        None, stats) as render does."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_lens(self._h, C.byref(params), C.byref(lens), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_lens_device(self, params, lens, d_accum, stream=0, stats=False):
        """rt_render_lens_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample ranges chain."""
        st = Stats() if stats else None
        _check(amd().rt_render_lens_device(self._h, C.byref(params), C.byref(lens), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                           C.byref(st) if stats else None))
        return st

    def render_shutter(self, params, shutter, bg=None, want_accum=True):
        """rt_render_shutter: the frame under the open shutter `shutter` (make_shutter) while the camera moves; returns
        (out or None without bg, accum or None, stats) as render does."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_shutter(self._h, C.byref(params), C.byref(shutter), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_shutter_device(self, params, shutter, d_accum, stream=0, stats=False):
        """rt_render_shutter_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample ranges chain."""
        st = Stats() if stats else None
        _check(amd().rt_render_shutter_device(self._h, C.byref(params), C.byref(shutter), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                              C.byref(st) if stats else None))
        return st

    def render_lights(self, params, groups, bg=None, want_accum=True):
        """rt_render_lights: the frame split by light group (`groups`: make_light_groups, or a sequence of masks); returns
        (out [G][h][w][3] or None without bg, accum [G][h][w][4] or None, stats): slice g is the frame with only the
        lights of masks[g] lit, and the stats are one frame's."""
        if not isinstance(groups, LightGroups):
            groups = make_light_groups(groups)
        w, h, n = params.width, params.height, max(1, groups.n_groups)
        out = np.empty((n, h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((n, h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_lights(self._h, C.byref(params), C.byref(groups), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_lights_device(self, params, groups, d_accum, stream=0, stats=False):
        """rt_render_lights_device: accumulate into the caller-zeroed device d_accum [G][h][w][4] on `stream`; sample ranges chain."""
        if not isinstance(groups, LightGroups):
            groups = make_light_groups(groups)
        st = Stats() if stats else None
        _check(amd().rt_render_lights_device(self._h, C.byref(params), C.byref(groups), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                             C.byref(st) if stats else None))
        return st

    def render_pick(self, params, pick, bg=None, want_accum=True, importance=None):
        """rt_render_pick: the frame with sampled direct lighting (`pick`: make_light_pick, or the slot count with
        `importance` beside it); returns (out [h][w][3] or None without bg, accum [h][w][4] or None, stats)."""
        if not isinstance(pick, LightPick):
            pick = make_light_pick(pick, importance)
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_pick(self._h, C.byref(params), C.byref(pick), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_pick_device(self, params, pick, d_accum, stream=0, stats=False, importance=None):
        """rt_render_pick_device: accumulate into the caller-zeroed device d_accum [h][w][4] on `stream`; sample ranges chain."""
        if not isinstance(pick, LightPick):
            pick = make_light_pick(pick, importance)
        st = Stats() if stats else None
        _check(amd().rt_render_pick_device(self._h, C.byref(params), C.byref(pick), C.c_void_p(d_accum), C.c_void_p(stream or None),
                                           C.byref(st) if stats else None))
        return st

    def render_views_shutter(self, params, cameras, shutters, bg=None, seeds=None, want_accum=True):
        """rt_render_views_shutter: render_views with view j under the open shutter shutters[j] (a sequence of
        make_shutter records, one per camera: cameras[j] when it opens, its camera_close when it closes); returns
        (out [n][h][w][3] or None without bg, accum [n][h][w][4] or None, stats)."""
        v, _keep = make_views(cameras, seeds)
        sh = make_shutters(shutters, v.n_views)
        w, h, n = params.width, params.height, v.n_views
        out = np.empty((n, h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((n, h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_views_shutter(self._h, C.byref(params), C.byref(v), sh, _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_views_shutter_device(self, params, cameras, shutters, d_accum_ptr, stream=0, seeds=None, stats=False):
        """rt_render_views_shutter_device: accumulate into the caller-zeroed device d_accum [n][h][w][4] on `stream`."""
        v, _keep = make_views(cameras, seeds)
        sh = make_shutters(shutters, v.n_views)
        st = Stats() if stats else None
        _check(amd().rt_render_views_shutter_device(self._h, C.byref(params), C.byref(v), sh, C.c_void_p(d_accum_ptr),
                                                    C.c_void_p(stream or None), C.byref(st) if stats else None))
        return st

    def render_views_shutter_albedo(self, params, cameras, shutters, albedo=ALBEDO_TEXTURES, bg=None, seeds=None, want_accum=True):
        """rt_render_views_shutter_albedo: render_views_shutter with every shaded vertex's albedo from the resident vertex
        colours (ALBEDO_COLORS) or texture set (ALBEDO_TEXTURES); ALBEDO_MATERIAL is render_views_shutter itself.
        Returns (out [n][h][w][3] or None without bg, accum [n][h][w][4] or None, stats)."""
        v, _keep = make_views(cameras, seeds)
        sh = make_shutters(shutters, v.n_views)
        w, h, n = params.width, params.height, v.n_views
        out = np.empty((n, h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((n, h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_render_views_shutter_albedo(self._h, C.byref(params), C.byref(v), sh, albedo, _ptr(bgc), _ptr(out),
                                                    _ptr(acc), C.byref(st)))
        return out, acc, st

    def render_views_shutter_albedo_device(self, params, cameras, shutters, d_accum_ptr, albedo=ALBEDO_TEXTURES, stream=0,
                                           seeds=None, stats=False):
        """rt_render_views_shutter_albedo_device: accumulate into the caller-zeroed device d_accum [n][h][w][4] on `stream`."""
        v, _keep = make_views(cameras, seeds)
        sh = make_shutters(shutters, v.n_views)
        st = Stats() if stats else None
        _check(amd().rt_render_views_shutter_albedo_device(self._h, C.byref(params), C.byref(v), sh, albedo, C.c_void_p(d_accum_ptr),
                                                           C.c_void_p(stream or None), C.byref(st) if stats else None))
        return st

    def render_adaptive_shutter(self, params, shutter, bg, threshold, max_passes, min_passes=0, floor=0.):
        """rt_render_adaptive_shutter: render_adaptive whose passes are render_shutter frames under `shutter`.  Returns
        (out [h][w][3], accum [h][w][4], spp [h][w] uint32, AdaptiveReport, Stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32)
        acc = np.empty((h, w, 4), np.float32)
        spp = np.empty((h, w), np.uint32)
        rep, st = AdaptiveReport(), Stats()
        bgc = np.ascontiguousarray(bg, np.float32)
        a = make_adaptive(threshold, max_passes, min_passes, floor)
        _check(amd().rt_render_adaptive_shutter(self._h, C.byref(params), C.byref(a), C.byref(shutter), _ptr(bgc), _ptr(out),
                                                _ptr(acc), _ptr(spp), C.byref(rep), C.byref(st)))
        return out, acc, spp, rep, st

    def render_adaptive_shutter_device(self, params, shutter, d_bg, d_accum, d_out, threshold, max_passes, min_passes=0,
                                       floor=0., d_spp=None, stream=0, stats=False):
        """rt_render_adaptive_shutter_device on device pointers (d_accum is overwritten; d_spp may be None), on `stream`.
        Returns (AdaptiveReport, Stats or None)."""
        rep = AdaptiveReport()
        st = Stats() if stats else None
        a = make_adaptive(threshold, max_passes, min_passes, floor)
        _check(amd().rt_render_adaptive_shutter_device(self._h, C.byref(params), C.byref(a), C.byref(shutter), C.c_void_p(d_bg),
                                                       C.c_void_p(d_accum), C.c_void_p(d_out), C.c_void_p(d_spp or None),
                                                       C.c_void_p(stream or None), C.byref(rep), C.byref(st) if stats else None))
        return rep, st

    @staticmethod
    def _motion_prev(prev_pos, prev_camera):
        """An rt_motion_prev: prev_pos a numpy array [n_vertices][3] (host form), a device pointer (int) or None;
        prev_camera [4][3] floats or None.  Returns it and the arrays it points into."""
        m, keep = MotionPrev(), []
        if prev_pos is not None:
            if isinstance(prev_pos, int):
                m.vertex_pos = prev_pos
            else:
                keep.append(np.ascontiguousarray(prev_pos, np.float32).reshape(-1, 3))
                m.vertex_pos = keep[-1].ctypes.data
        if prev_camera is not None:
            keep.append(np.ascontiguousarray(prev_camera, np.float32).reshape(4, 3))
            m.camera = C.cast(keep[-1].ctypes.data, C.POINTER(Camera))
        return m, keep

    def render_motion(self, params, prev_pos=None, prev_camera=None, channels=MOTION_CHANNELS):
        """rt_render_motion: per pixel, where the surface point the frame's first primary ray hits was last frame —
        dict of motion [h][w][2], position, prev_position [h][w][3] (float32) and mesh [h][w] (uint32).  prev_pos
        [n_vertices][3] / prev_camera [4][3]: last frame's (None = the context's own)."""
        w, h = params.width, params.height
        shape = dict(motion=(h, w, 2), position=(h, w, 3), prev_position=(h, w, 3), mesh=(h, w))
        out, m = {}, Motion()
        for k in channels:
            out[k] = np.zeros(shape[k], np.uint32 if k == "mesh" else np.float32)
            setattr(m, k, out[k].ctypes.data)
        prev, _keep = self._motion_prev(prev_pos, prev_camera)
        _check(amd().rt_render_motion(self._h, C.byref(params), C.byref(prev), C.byref(m)))
        return out

    def render_motion_device(self, params, ptrs, d_prev_pos=None, prev_camera=None, stream=0):
        """rt_render_motion_device: into device buffers; ptrs = {channel: device pointer} (missing = not wanted),
        d_prev_pos a device pointer or None."""
        m = Motion()
        for k, v in ptrs.items():
            setattr(m, k, v or None)
        prev, _keep = self._motion_prev(int(d_prev_pos) if d_prev_pos else None, prev_camera)
        _check(amd().rt_render_motion_device(self._h, C.byref(params), C.byref(prev), C.byref(m), C.c_void_p(stream or None)))

    def temporal_accumulate(self, cur_rgb, cur, prev, max_history=0, alpha_min=0., sigma_position=0.):
        """rt_temporal_accumulate: cur_rgb [h][w][3] the current frame, cur = render_motion's dict for it, prev = the
        history dict (rgb, position, mesh, length; pyrt.empty_history for the first frame).  Returns (out_rgb,
        out_length); the next frame's history is dict(rgb=out_rgb, position=cur["position"], mesh=cur["mesh"],
        length=out_length)."""
        rgb = np.ascontiguousarray(cur_rgb, np.float32)
        h, w = rgb.shape[:2]
        ck = {k: np.ascontiguousarray(cur[k], np.uint32 if k == "mesh" else np.float32) for k in ("motion", "prev_position", "mesh")}
        hk = {k: np.ascontiguousarray(prev[k], np.uint32 if k == "mesh" else np.float32) for k in HISTORY_CHANNELS}
        m, hs = Motion(), History()
        for k, v in ck.items():
            setattr(m, k, v.ctypes.data)
        for k, v in hk.items():
            setattr(hs, k, v.ctypes.data)
        out, length = np.empty((h, w, 3), np.float32), np.empty((h, w), np.float32)
        t = make_temporal(w, h, max_history, alpha_min, sigma_position)
        _check(amd().rt_temporal_accumulate(self._h, C.byref(t), _ptr(rgb), C.byref(m), C.byref(hs), _ptr(out), _ptr(length)))
        return out, length

    def temporal_accumulate_device(self, width, height, d_cur_rgb, cur_ptrs, prev_ptrs, d_out_rgb, d_out_length, stream=0,
                                   max_history=0, alpha_min=0., sigma_position=0.):
        """rt_temporal_accumulate_device: device pointers (cur_ptrs = {"motion", "prev_position", "mesh"}, prev_ptrs =
        {"rgb", "position", "mesh", "length"}), on `stream`."""
        m, hs = Motion(), History()
        for k, v in cur_ptrs.items():
            setattr(m, k, v or None)
        for k, v in prev_ptrs.items():
            setattr(hs, k, v or None)
        t = make_temporal(width, height, max_history, alpha_min, sigma_position)
        _check(amd().rt_temporal_accumulate_device(self._h, C.byref(t), C.c_void_p(d_cur_rgb), C.byref(m), C.byref(hs),
                                                   C.c_void_p(d_out_rgb), C.c_void_p(d_out_length), C.c_void_p(stream or None)))

    def svgf(self, cur_rgb, aov_sums, cur, prev, want=("accum", "variance"), out_rgb=None, **kw):
        """rt_svgf: cur_rgb [h][w][3] the current frame, aov_sums = render_aov(raw=True)'s sums for it, cur =
        render_motion's dict, prev = the history dict (color, moments, position, mesh, length; pyrt.empty_svgf_history
        for the first frame); kw: make_svgf's.  Returns a dict of rgb, color, moments, length and the optional outputs
        named in `want`; the next frame's history is dict(color=out["color"], moments=out["moments"],
        position=cur["position"], mesh=cur["mesh"], length=out["length"]).  out_rgb may be cur_rgb itself (in place)."""
        rgb = np.ascontiguousarray(cur_rgb, np.float32)
        h, w = rgb.shape[:2]
        u32 = ("hits", "mesh")
        keep = [{k: np.ascontiguousarray(src[k], np.uint32 if k in u32 else np.float32) for k in names}
                for src, names in ((aov_sums, ("albedo", "normal", "position", "hits")),
                                   (cur, ("motion", "prev_position", "mesh")), (prev, SVGF_HISTORY_CHANNELS))]
        a, m, hs, o = Aov(), Motion(), SvgfHistory(), SvgfOut()
        for st, d in zip((a, m, hs), keep):
            for k, v in d.items():
                setattr(st, k, v.ctypes.data)
        out = {k: np.empty((h, w, n) if n > 1 else (h, w), np.float32) for k, n in SVGF_OUT_CHANNELS
               if k in ("rgb", "color", "moments", "length") or k in want}
        if out_rgb is not None:
            assert out_rgb.dtype == np.float32 and out_rgb.flags["C_CONTIGUOUS"] and out_rgb.shape == rgb.shape
            out["rgb"] = out_rgb
        for k, v in out.items():
            setattr(o, k, v.ctypes.data)
        s = make_svgf(w, h, **kw)
        _check(amd().rt_svgf(self._h, C.byref(s), _ptr(rgb), C.byref(a), C.byref(m), C.byref(hs), C.byref(o)))
        return out

    def svgf_device(self, width, height, d_cur_rgb, aov_ptrs, cur_ptrs, prev_ptrs, out_ptrs, stream=0, **kw):
        """rt_svgf_device: device pointers (aov_ptrs = {"albedo", "normal", "position", "hits": sums}, cur_ptrs =
        {"motion", "prev_position", "mesh"}, prev_ptrs = the five history channels, out_ptrs = {"rgb", "color",
        "moments", "length"} and optionally "accum", "variance"), on `stream`; kw: make_svgf's."""
        a, m, hs, o = Aov(), Motion(), SvgfHistory(), SvgfOut()
        for st, d in ((a, aov_ptrs), (m, cur_ptrs), (hs, prev_ptrs), (o, out_ptrs)):
            for k, v in d.items():
                setattr(st, k, v or None)
        s = make_svgf(width, height, **kw)
        _check(amd().rt_svgf_device(self._h, C.byref(s), C.c_void_p(d_cur_rgb), C.byref(a), C.byref(m), C.byref(hs), C.byref(o),
                                    C.c_void_p(stream or None)))

    def render_adaptive(self, params, bg, threshold, max_passes, min_passes=0, floor=0.):
        """rt_render_adaptive: passes of params.spp samples over the granules not yet converged (DESIGN.md "Adaptive
        sampling").  Returns (out [h][w][3], accum [h][w][4], spp [h][w] uint32, AdaptiveReport, Stats)."""
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32)
        acc = np.empty((h, w, 4), np.float32)
        spp = np.empty((h, w), np.uint32)
        rep, st = AdaptiveReport(), Stats()
        bgc = np.ascontiguousarray(bg, np.float32)
        a = make_adaptive(threshold, max_passes, min_passes, floor)
        _check(amd().rt_render_adaptive(self._h, C.byref(params), C.byref(a), _ptr(bgc), _ptr(out), _ptr(acc), _ptr(spp),
                                        C.byref(rep), C.byref(st)))
        return out, acc, spp, rep, st

    def render_adaptive_device(self, params, d_bg, d_accum, d_out, threshold, max_passes, min_passes=0, floor=0.,
                               d_spp=None, stream=0, stats=False):
        """rt_render_adaptive_device on device pointers (d_accum is overwritten; d_spp may be None), on `stream`.
        Returns (AdaptiveReport, Stats or None)."""
        rep = AdaptiveReport()
        st = Stats() if stats else None
        a = make_adaptive(threshold, max_passes, min_passes, floor)
        _check(amd().rt_render_adaptive_device(self._h, C.byref(params), C.byref(a), C.c_void_p(d_bg), C.c_void_p(d_accum),
                                               C.c_void_p(d_out), C.c_void_p(d_spp or None), C.c_void_p(stream or None),
                                               C.byref(rep), C.byref(st) if stats else None))
        return rep, st

    @staticmethod
    def _denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_position):
        d = DenoiseParams()
        d.width, d.height, d.iterations = width, height, iterations
        d.sigma_color, d.sigma_normal, d.sigma_position = sigma_color, sigma_normal, sigma_position
        return d

    def denoise(self, rgb, aov_sums, iterations=0, sigma_color=0., sigma_normal=0., sigma_position=0., out=None):
        """rt_denoise: the a-trous filter of the resolved frame rgb [h][w][3] guided by the SUMS of render_aov
        (raw=True) for the same params.  0 = the defaults.  `out` may be rgb itself (in place)."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        h, w = rgb.shape[:2]
        out = np.empty_like(rgb) if out is None else out
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.shape == rgb.shape
        keep = {k: np.ascontiguousarray(aov_sums[k], np.uint32 if k == "hits" else np.float32)
                for k in ("albedo", "normal", "position", "hits")}
        a = Aov()
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        d = self._denoise_params(w, h, iterations, sigma_color, sigma_normal, sigma_position)
        _check(amd().rt_denoise(self._h, C.byref(d), _ptr(rgb), C.byref(a), _ptr(out)))
        return out

    def denoise_device(self, width, height, d_rgb, ptrs, d_out, stream=0, iterations=0, sigma_color=0., sigma_normal=0.,
                       sigma_position=0.):
        """rt_denoise_device: device pointers (ptrs = {"albedo", "normal", "position", "hits": sums}), on `stream`."""
        a = Aov()
        for k, v in ptrs.items():
            setattr(a, k, v or None)
        d = self._denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_position)
        _check(amd().rt_denoise_device(self._h, C.byref(d), C.c_void_p(d_rgb), C.byref(a), C.c_void_p(d_out),
                                       C.c_void_p(stream or None)))

    def render_aov_views(self, params, cameras, seeds=None, channels=AOV_CHANNELS):
        """rt_render_aov_views: the SUMS of render_aov(raw=True) for every camera of cameras [n][4][3] (seeds [n] or None =
        params.seed) in one launch, as a dict of arrays with a leading view axis ([n][h][w][3] / [n][h][w]).
        `channels`: the ones wanted (the others are not computed)."""
        v, _keep = make_views(cameras, seeds)
        w, h, n = params.width, params.height, v.n_views
        sums, a = {}, Aov()
        for k in channels:
            sums[k] = np.zeros((n, h, w, 3) if k in AOV_FLOAT3 else (n, h, w), np.float32 if k in AOV_FLOAT3 or k == "depth" else np.uint32)
            setattr(a, k, sums[k].ctypes.data)
        _check(amd().rt_render_aov_views(self._h, C.byref(params), C.byref(v), C.byref(a)))
        return sums

    def render_aov_views_device(self, params, cameras, ptrs, stream=0, seeds=None):
        """rt_render_aov_views_device: the sums into device buffers [n][h][w][..]; ptrs = {channel: device pointer}."""
        v, _keep = make_views(cameras, seeds)
        a = Aov()
        for k, p in ptrs.items():
            setattr(a, k, p or None)
        _check(amd().rt_render_aov_views_device(self._h, C.byref(params), C.byref(v), C.byref(a), C.c_void_p(stream or None)))

    def render_aov_views_albedo(self, params, cameras, albedo=ALBEDO_TEXTURES, seeds=None, channels=AOV_CHANNELS):
        """rt_render_aov_views_albedo: render_aov_views whose albedo channel sums the resident vertex colours'
        interpolation (ALBEDO_COLORS) or the resident textures' sample (ALBEDO_TEXTURES)."""
        v, _keep = make_views(cameras, seeds)
        w, h, n = params.width, params.height, v.n_views
        sums, a = {}, Aov()
        for k in channels:
            sums[k] = np.zeros((n, h, w, 3) if k in AOV_FLOAT3 else (n, h, w), np.float32 if k in AOV_FLOAT3 or k == "depth" else np.uint32)
            setattr(a, k, sums[k].ctypes.data)
        _check(amd().rt_render_aov_views_albedo(self._h, C.byref(params), C.byref(v), albedo, C.byref(a)))
        return sums

    def render_aov_views_albedo_device(self, params, cameras, ptrs, albedo=ALBEDO_TEXTURES, stream=0, seeds=None):
        """rt_render_aov_views_albedo_device: the sums into device buffers [n][h][w][..]; ptrs = {channel: device pointer}."""
        v, _keep = make_views(cameras, seeds)
        a = Aov()
        for k, p in ptrs.items():
            setattr(a, k, p or None)
        _check(amd().rt_render_aov_views_albedo_device(self._h, C.byref(params), C.byref(v), albedo, C.byref(a),
                                                       C.c_void_p(stream or None)))

    @staticmethod
    def _motion_prev_views(prev_pos, prev_cameras, n):
        """An rt_motion_prev_views: prev_pos as _motion_prev's; prev_cameras [n][4][3] floats or None."""
        m, keep = MotionPrevViews(), []
        if prev_pos is not None:
            if isinstance(prev_pos, int):
                m.vertex_pos = prev_pos
            else:
                keep.append(np.ascontiguousarray(prev_pos, np.float32).reshape(-1, 3))
                m.vertex_pos = keep[-1].ctypes.data
        if prev_cameras is not None:
            keep.append(np.ascontiguousarray(prev_cameras, np.float32).reshape(-1, 12))
            if len(keep[-1]) != n:
                raise ValueError("%d previous cameras for %d views" % (len(keep[-1]), n))
            m.cameras = C.cast(keep[-1].ctypes.data, C.POINTER(Camera))
        return m, keep

    def render_motion_views(self, params, cameras, prev_pos=None, prev_cameras=None, seeds=None, channels=MOTION_CHANNELS):
        """rt_render_motion_views: render_motion's dict for every camera of cameras [n][4][3] in one launch, each array with
        a leading view axis.  prev_pos [n_vertices][3] / prev_cameras [n][4][3]: last frame's (None = the context's
        positions / the views' own cameras)."""
        v, _keep = make_views(cameras, seeds)
        w, h, n = params.width, params.height, v.n_views
        shape = dict(motion=(n, h, w, 2), position=(n, h, w, 3), prev_position=(n, h, w, 3), mesh=(n, h, w))
        out, m = {}, Motion()
        for k in channels:
            out[k] = np.zeros(shape[k], np.uint32 if k == "mesh" else np.float32)
            setattr(m, k, out[k].ctypes.data)
        prev, _keep2 = self._motion_prev_views(prev_pos, prev_cameras, n)
        _check(amd().rt_render_motion_views(self._h, C.byref(params), C.byref(v), C.byref(prev), C.byref(m)))
        return out

    def render_motion_views_device(self, params, cameras, ptrs, d_prev_pos=None, prev_cameras=None, stream=0, seeds=None):
        """rt_render_motion_views_device: into device buffers [n][h][w][..]; ptrs = {channel: device pointer}, d_prev_pos a
        device pointer or None."""
        v, _keep = make_views(cameras, seeds)
        m = Motion()
        for k, p in ptrs.items():
            setattr(m, k, p or None)
        prev, _keep2 = self._motion_prev_views(int(d_prev_pos) if d_prev_pos else None, prev_cameras, v.n_views)
        _check(amd().rt_render_motion_views_device(self._h, C.byref(params), C.byref(v), C.byref(prev), C.byref(m),
                                                   C.c_void_p(stream or None)))

    def denoise_batch(self, rgb, aov_sums, iterations=0, sigma_color=0., sigma_normal=0., sigma_position=0., out=None):
        """rt_denoise_batch: denoise() of every frame of rgb [n][h][w][3] guided by the stacked SUMS of render_aov_views, in
        one launch per stage.  `out` may be rgb itself (in place)."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        n, h, w = rgb.shape[:3]
        out = np.empty_like(rgb) if out is None else out
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.shape == rgb.shape
        keep = {k: np.ascontiguousarray(aov_sums[k], np.uint32 if k == "hits" else np.float32)
                for k in ("albedo", "normal", "position", "hits")}
        a = Aov()
        for k, x in keep.items():
            assert x.shape[:3] == (n, h, w), k
            setattr(a, k, x.ctypes.data)
        d = self._denoise_params(w, h, iterations, sigma_color, sigma_normal, sigma_position)
        _check(amd().rt_denoise_batch(self._h, C.byref(d), n, _ptr(rgb), C.byref(a), _ptr(out)))
        return out

    def denoise_batch_device(self, width, height, n_frames, d_rgb, ptrs, d_out, stream=0, iterations=0, sigma_color=0.,
                             sigma_normal=0., sigma_position=0.):
        """rt_denoise_batch_device: device pointers to [n_frames] stacked buffers (ptrs = {"albedo", "normal", "position",
        "hits": sums}), on `stream`."""
        a = Aov()
        for k, p in ptrs.items():
            setattr(a, k, p or None)
        d = self._denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_position)
        _check(amd().rt_denoise_batch_device(self._h, C.byref(d), n_frames, C.c_void_p(d_rgb), C.byref(a), C.c_void_p(d_out),
                                             C.c_void_p(stream or None)))

    def knn(self, queries, k):
        q = np.ascontiguousarray(queries, np.float32)
        idx = np.zeros((len(q), k), np.uint32)
        dist = np.zeros((len(q), k), np.float32)
        vis = np.zeros(len(q), np.uint32)
        _check(amd().rt_knn(self._h, _ptr(q), len(q), k, _ptr(idx), _ptr(dist), _ptr(vis)))
        return idx, dist, vis

    def knn_wide(self, queries, k):
        """rt_knn_wide: knn for k in 1..KMAX_WIDE (k <= KMAX: exactly knn; above: the wide frames' walk)."""
        q = np.ascontiguousarray(queries, np.float32)
        idx = np.zeros((len(q), k), np.uint32)
        dist = np.zeros((len(q), k), np.float32)
        vis = np.zeros(len(q), np.uint32)
        _check(amd().rt_knn_wide(self._h, _ptr(q), len(q), k, _ptr(idx), _ptr(dist), _ptr(vis)))
        return idx, dist, vis


def kd_order_device(pos, depth_limit=-1, device=0):
    """rt_test_kd_order: permutation (tree slot -> input index) built on the GPU, and its ms."""
    pos = np.ascontiguousarray(pos, np.float32)
    perm = np.zeros(len(pos), np.uint32)
    ms = C.c_double()
    _check(amd().rt_test_kd_order(device, _ptr(pos), len(pos), depth_limit, _ptr(perm), C.byref(ms)))
    return perm, ms.value


def owned_granules(params, rank):
    """Number of 8x8-pixel granules `rank` owns in the tile-sharded frame `params` describes."""
    n = C.c_uint32()
    _check(amd().rt_owned_granules(C.byref(params), rank, C.byref(n)))
    return n.value


class Group:
    """rt_group: one process driving N devices (RCCL / peer copies inside librt_amd.so)."""

    def __init__(self, scene, devices, bvh_leaf_max=0, node_format=0):
        self.scene = scene
        opt = Options()
        opt.bvh_leaf_max, opt.node_format = bvh_leaf_max, node_format
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        _check(amd().rt_group_create(scene.desc_ptr, devs, len(devices), C.byref(opt), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            amd().rt_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return amd().rt_group_size(self._h)

    @property
    def uses_rccl(self):
        return bool(amd().rt_group_uses_rccl(self._h))

    def set_photons(self, pos, dir_):
        pos = np.ascontiguousarray(pos, np.float32)
        dir_ = np.ascontiguousarray(dir_, np.float32)
        _check(amd().rt_group_set_photons(self._h, _ptr(pos), _ptr(dir_), len(pos)))

    def update(self, pos=None, nrm=None, camera=None, lights=None, materials=None):
        """rt_group_update: Context.update on every rank; rank 0's report."""
        u, _keep = _scene_update(pos, nrm, camera, lights, materials)
        rep = UpdateReport()
        _check(amd().rt_group_update(self._h, C.byref(u), C.byref(rep)))
        return rep.as_dict()

    def render(self, params, bg=None, want_accum=True):
        w, h = params.width, params.height
        out = np.empty((h, w, 3), np.float32) if bg is not None else None
        acc = np.empty((h, w, 4), np.float32) if want_accum else None
        st = Stats()
        bgc = None if bg is None else np.ascontiguousarray(bg, np.float32)
        _check(amd().rt_group_render(self._h, C.byref(params), _ptr(bgc), _ptr(out), _ptr(acc), C.byref(st)))
        return out, acc, st


_UNIT_IO = {UNIT_ASIN: (np.float64, 1, np.float64, 1), UNIT_SINF: (np.float32, 1, np.float32, 1),
            UNIT_COSF: (np.float32, 1, np.float32, 1), UNIT_STREAM_SEED: (np.uint32, 4, np.uint32, 1),
            UNIT_TRIANGLE: (np.float32, 15, np.float32, 4), UNIT_BSDF: (np.float32, 17, np.float32, 3),
            UNIT_RAY_AT: (np.float32, 14, np.float32, 6), UNIT_LIGHT_EVAL: (np.float32, 24, np.float32, 3),
            UNIT_SAMPLERS: (np.uint32, 28, np.uint32, 12), UNIT_LIGHT_SAMPLE: (np.uint32, 22, np.uint32, 4),
            UNIT_POW: (np.float64, 1, np.float64, 2), UNIT_RECIP: (np.float32, 1, np.float32, 4),
            UNIT_BSDF_HOISTED: (np.float32, 17, np.float32, 9), UNIT_HEMISPHERE: (np.uint32, 4, np.uint32, 4)}


def unit(which, inp, out_init=None, device=0):
    """rt_test_unit: evaluate one device building block on n packed inputs."""
    it, iw, ot, ow = _UNIT_IO[which]
    a = np.ascontiguousarray(inp, it).reshape(-1, iw)
    out = np.zeros((len(a), ow), ot) if out_init is None else np.ascontiguousarray(out_init, ot).reshape(len(a), ow).copy()
    _check(amd().rt_test_unit(device, which, _ptr(a), _ptr(out), len(a)))
    return out


class ArrayScene:
    """A scene assembled from numpy arrays (tests: scaled / synthetic geometry)."""

    def __init__(self, pos, nrm, tri, tri_begin, vtx_begin, materials, lights, camera):
        self._keep = [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32),
                      np.ascontiguousarray(tri, np.uint32), np.ascontiguousarray(tri_begin, np.uint32),
                      np.ascontiguousarray(vtx_begin, np.uint32), np.ascontiguousarray(materials, np.float32),
                      np.ascontiguousarray(lights, np.float32), np.ascontiguousarray(camera, np.float32)]
        k = self._keep
        d = SceneDesc()
        d.n_meshes, d.n_vertices, d.n_triangles, d.n_lights = len(k[3]) - 1, len(k[0]), len(k[2]), len(k[6])
        d.vertex_pos = k[0].ctypes.data_as(C.POINTER(C.c_float))
        d.vertex_nrm = k[1].ctypes.data_as(C.POINTER(C.c_float))
        d.tri_vtx = k[2].ctypes.data_as(C.POINTER(C.c_uint32))
        d.mesh_tri_begin = k[3].ctypes.data_as(C.POINTER(C.c_uint32))
        d.mesh_vtx_begin = k[4].ctypes.data_as(C.POINTER(C.c_uint32))
        d.materials = k[5].ctypes.data_as(C.POINTER(Material))
        d.lights = k[6].ctypes.data_as(C.POINTER(Light))
        C.memmove(C.byref(d.camera), k[7].ctypes.data, 48)
        self.desc = d
        self.desc_ptr = C.pointer(d)

    def arrays(self):
        k = self._keep
        return dict(pos=k[0], nrm=k[1], tri=k[2], tri_begin=k[3], vtx_begin=k[4], materials=k[5], lights=k[6], camera=k[7])
