"""The surface-area cost of rt_bvh_quality_get restated in numpy over an rt_bvh_export pair (include/rt_amd.h, "rebuilding a
refit tree").  Node i has two slots k with a box lo, hi (float32) and a ref child[k]: >= 0 an inner node, < 0 a leaf of
cnt = ((~ref) & 7) + 1 triangle records.  With A(lo, hi) = dx*dy + dy*dz + dz*dx in float64 from the float32 planes and
A_root = max(A(union of node 0's two slots), 1e-300):
    nodes = 1 + sum over inner slots of A / A_root,  tris = sum over leaf slots of cnt * A / A_root,  cost = nodes + 1.5 * tris.
The sums are exact sums (math.fsum) of the float64 terms."""
import math

import numpy as np


def area(lo, hi):
    """A of boxes lo, hi [..., 3] (float32 planes), in float64."""
    d = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return dx * dy + dy * dz + dz * dx


def cost(nodes):
    """nodes: [n][16] uint32, the rt_bvh_export node records (lo0 hi0 lo1 hi1 child[2] pad[2]).  Returns a dict of cost,
    nodes, tris (float64) and n_slots."""
    nodes = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 16)
    f = nodes.view(np.float32)
    lo = np.stack([f[:, 0:3], f[:, 6:9]], 1)   # [n][2][3]
    hi = np.stack([f[:, 3:6], f[:, 9:12]], 1)
    ref = nodes[:, 12:14].view(np.int32)       # [n][2]
    a_root = max(float(area(np.minimum(lo[0, 0], lo[0, 1]), np.maximum(hi[0, 0], hi[0, 1]))), 1e-300)
    a = area(lo, hi)
    inner = ref >= 0
    cnt = ((~ref) & 7) + 1
    node_terms = a[inner] / a_root
    tri_terms = (cnt[~inner].astype(np.float64) * a[~inner]) / a_root
    n, t = 1.0 + math.fsum(node_terms), math.fsum(tri_terms)
    return dict(cost=n + 1.5 * t, nodes=n, tris=t, n_slots=2 * len(nodes))
