"""Scenes and (scene, request, seed) cases for the device's photon pipeline: emission (k_emit), the one-workgroup
compaction (k_photon_compact), the gather after the kd order (k_photon_gather) and the host code around them in
rt_emit_photons / rt_build_photon_map.  numpy + pyrt only; no GPU.

What the cases are chosen to reach (tests/test_photon_cases_cpu.py establishes each with the oracle, so a drifting
preset fails there and does not hollow out tests/test_gpu_photon_pipeline.py):

* light counts 1..5: k_emit takes the light from j / perLight and the weight from 1 / n_lights, and the slot count is
  (int)((float)n * (1.f / n_lights)) * n_lights: requests on both sides of a perLight step and requests below the
  light count (zero slots) for every light count;
* slot counts around the compaction's chunk edges: it is ONE workgroup of 1,024 threads, each scanning
  ceil(n / 1024) consecutive slots, so n < 1,024 leaves tail threads idle, n = 1,025 gives the first 512 threads two
  slots, thread 512 one and the rest none, and 1,024 m - 1, 1,024 m, 1,024 m + 1 change the chunk length (with ONE
  light the slot count is the request);
* emission's four exits: a miss on the first cast (nothing stored: aimed_away_scene), a miss after a bounce (the last
  hit stored: the open room), the roulette exit (the hit stored: closed_box_scene(DARK) takes it on every photon) and
  the 20-cast cap (nothing stored: in the watertight closed_box_scene(BRIGHT) an unstored photon can be nothing else);
* maps of exactly 1, 2 and 3 stored photons built by the device (TINY)."""
import numpy as np

import pyrt

LIGHT_COUNTS = (1, 2, 3, 4, 5)
# 1..7: single live lanes of k_emit's first wave and perLight == 0 / 1; 63..65: its wave; 1,023..1,026, 2,047..2,049,
# 3,073: the compaction's chunk edges (with one light) and perLight steps of the other light counts
REQUESTS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 3073)
# slot counts 1,024 m - 1, 1,024 m, 1,024 m + 1 for m = 1, 2, 3; reached with one light, where slots == request
COMPACT_EDGES = tuple(1024 * m + d for m in (1, 2, 3) for d in (-1, 0, 1))
SEEDS = (5, 11)
DARK, BRIGHT = 0.05, 3.0  # closed_box_scene albedos: roulette exit at the first hit / the 20-cast cap
EXIT_SLOTS = (1025, 3000)
EXIT_SCENES = ("aimed_away", "box_dark", "box_bright")
# one-light requests (seed 5) that store exactly 1, 2 and 3 photons: {n_stored: (request, seed)}
TINY = {1: (1, 5), 2: (4, 5), 3: (7, 5)}


def slots(n_requested, n_lights):
    """photons_per_light (rt_api.cpp; PhotonMap.h:19-20) times the light count, restated in float32: the number of
    photons emitted, each of which owns one slot."""
    if n_requested == 0 or n_lights == 0:
        return 0
    light_pdf = np.float32(1) / np.float32(n_lights)
    return int(np.float32(n_requested) * light_pdf) * n_lights


def requests_for(n_lights):
    """The emission requests of a light count: REQUESTS, and with one light the compaction edges among them."""
    r = set(REQUESTS)
    if n_lights == 1:
        r |= set(COMPACT_EDGES)
    return tuple(sorted(r))


def _array_scene(a, lights, pos=None, nrm=None, tri=None, tri_begin=None, vtx_begin=None, materials=None):
    pick = lambda v, k: a[k] if v is None else v
    lights = np.ascontiguousarray(lights, np.float32).reshape(-1, 21)
    return pyrt.ArrayScene(pick(pos, "pos"), pick(nrm, "nrm"), pick(tri, "tri"), pick(tri_begin, "tri_begin"),
                           pick(vtx_begin, "vtx_begin"), pick(materials, "materials"),
                           lights if len(lights) else np.zeros((0, 21), np.float32), a["camera"])


def light_rows(n_lights, w=40, h=32):
    """The rt_light rows [n_lights][21] of lights_scene."""
    L = pyrt.Scene("cubes", w, h).arrays()["lights"]
    if n_lights > 3:  # two more lights: copies of light 2 moved inside the box
        extra = np.repeat(L[2:3], n_lights - 3, axis=0).copy()
        extra[:, 0] += np.linspace(-0.6, 0.7, n_lights - 3).astype(np.float32)
        extra[:, 1] += 0.9
        L = np.concatenate([L, extra])
    else:
        L = L[:n_lights]
    return np.ascontiguousarray(L, np.float32)


def lights_scene(n_lights, w=40, h=32):
    """The cubes preset (34 triangles, an open room) with 0..5 lights: the first n of its three, or its three and
    copies of the third moved inside the room."""
    return _array_scene(pyrt.Scene("cubes", w, h).arrays(), light_rows(n_lights, w, h))


def aimed_away_scene(w=40, h=32):
    """The cubes preset with ONE light, the preset's first, moved to (0, 0, -100) and looking along -z, away from the
    room: every photon misses on its first cast and stores nothing."""
    a = pyrt.Scene("cubes", w, h).arrays()
    L = a["lights"][:1].copy()
    at = np.array([[0.0, 0.0, -100.0]], np.float32)
    L[:, 0:3] = at
    L[:, 6:15] = pyrt.light_basis(at, at + np.array([[0.0, 0.0, -1.0]], np.float32))
    return _array_scene(a, L)


def closed_box_scene(albedo, w=40, h=32):
    """A watertight box: 12 triangles with inward normals (four vertices of their own per face), half-size 2 around
    the origin, one mesh with the preset's material 0 at a uniform albedo, the preset's first light at the centre.
    No photon can leave it, so an emitted photon either stores (the roulette exit) or runs into the 20-cast cap."""
    a = pyrt.Scene("cubes", w, h).arrays()
    pos, nrm, tri = [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            base = len(pos)
            for cu, cv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[axis], p[u], p[v] = 2.0 * sign, 2.0 * cu, 2.0 * cv
                n = np.zeros(3)
                n[axis] = -sign
                pos.append(p)
                nrm.append(n)
            # (e_u x e_v = e_axis: this winding faces +axis, what the -axis wall needs; the other one is turned)
            quad = (0, 1, 2, 0, 2, 3) if sign < 0 else (0, 2, 1, 0, 3, 2)
            tri += [[base + quad[0], base + quad[1], base + quad[2]], [base + quad[3], base + quad[4], base + quad[5]]]
    mats = a["materials"][:1].copy()
    mats[0, 2:5] = albedo  # (rt_material: kd, alpha, albedo[3], f0[3])
    L = a["lights"][:1].copy()
    L[:, 0:3] = 0.0
    return _array_scene(a, L, pos=np.array(pos, np.float32), nrm=np.array(nrm, np.float32), tri=np.array(tri, np.uint32),
                        tri_begin=np.array([0, 12], np.uint32), vtx_begin=np.array([0, 24], np.uint32), materials=mats)


def scene(name, w=40, h=32):
    """A scene of the case lists by name: "lights1" .. "lights5", "aimed_away", "box_dark", "box_bright"."""
    if name.startswith("lights"):
        return lights_scene(int(name[6:]), w, h)
    if name == "aimed_away":
        return aimed_away_scene(w, h)
    return closed_box_scene({"box_dark": DARK, "box_bright": BRIGHT}[name], w, h)


def emission_cases(n_lights):
    """(scene name, request, seed) of the emission / compaction sweep of one light count."""
    return [("lights%d" % n_lights, n, seed) for n in requests_for(n_lights) for seed in SEEDS]


def exit_cases():
    """(scene name, request, seed) of the exits: one light each, so the request is the slot count."""
    return [(name, n, SEEDS[0]) for name in EXIT_SCENES for n in EXIT_SLOTS]


CASES = [c for n in LIGHT_COUNTS for c in emission_cases(n)] + exit_cases() + \
        [("lights1", req, seed) for req, seed in TINY.values()]
