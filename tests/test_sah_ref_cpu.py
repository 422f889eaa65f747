"""tests/sah_ref.py on hand-written trees whose cost is worked out below (no GPU)."""
import numpy as np

import sah_ref


def node(lo0, hi0, lo1, hi1, c0, c1):
    r = np.zeros(16, np.uint32)
    r.view(np.float32)[0:12] = np.concatenate([lo0, hi0, lo1, hi1]).astype(np.float32)
    r.view(np.int32)[12:14] = [c0, c1]
    return r


def leaf(first, count):
    return ~((first << 3) | (count - 1))


def test_three_node_tree():
    """Root slots: [0,2]x[0,1]x[0,1] -> node 1 and [2,4]x[0,1]x[0,1] -> node 2: A = 2 + 1 + 2 = 5 each; their union is
    [0,4]x[0,1]x[0,1]: A_root = 4 + 1 + 4 = 9.  Node 1: two unit-cube leaves of 1 record (A = 3 each).  Node 2: a leaf of
    2 records in [2,3]x[0,1]x[0,1] (A = 3) and a leaf of 1 record in the flat box [3,4]x[0,1]x[0,0] (A = 1 + 0 + 0 = 1).
    nodes = 1 + (5 + 5) / 9 = 19 / 9; tris = (3 + 3 + 2 * 3 + 1) / 9 = 13 / 9; cost = 19 / 9 + 1.5 * 13 / 9 = 38.5 / 9."""
    t = np.stack([
        node([0, 0, 0], [2, 1, 1], [2, 0, 0], [4, 1, 1], 1, 2),
        node([0, 0, 0], [1, 1, 1], [1, 0, 0], [2, 1, 1], leaf(0, 1), leaf(1, 1)),
        node([2, 0, 0], [3, 1, 1], [3, 0, 0], [4, 1, 0], leaf(2, 2), leaf(4, 1))])
    c = sah_ref.cost(t)
    assert c["n_slots"] == 6
    assert abs(c["nodes"] - 19.0 / 9.0) <= 4e-16 and abs(c["tris"] - 13.0 / 9.0) <= 4e-16
    assert abs(c["cost"] - 38.5 / 9.0) <= 1e-15


def test_single_node_power_of_two_boxes_is_exact():
    """One node, two leaves: 8 records in [0,2]^3 (A = 12) and 1 record in [2,4]x[0,2]x[0,2] (A = 12); union [0,4]x[0,2]x[0,2]:
    A_root = 8 + 4 + 8 = 20.  nodes = 1 (no inner slot); tris = (8 * 12 + 12) / 20 = 5.4; cost = 1 + 1.5 * 5.4 = 9.1."""
    t = node([0, 0, 0], [2, 2, 2], [2, 0, 0], [4, 2, 2], leaf(0, 8), leaf(8, 1))[None]
    c = sah_ref.cost(t)
    assert c["nodes"] == 1.0 and c["n_slots"] == 2
    assert abs(c["tris"] - 5.4) <= 1e-15 and abs(c["cost"] - 9.1) <= 2e-15


def test_degenerate_root_box_hits_the_guard():
    """Every box is the point (1, 2, 3): all areas are 0 and A_root is the guard 1e-300, so every term is 0 / 1e-300 = 0:
    nodes = 1 + 0 (one inner slot), tris = 0, cost = 1 — finite, no division by zero.  The area function itself on flat
    boxes: a segment of length 1e-30 has A = 0, a flat square of that side A ~ 1e-60 (float64 holds it), and twice that
    over the guard is a finite number."""
    p = [1, 2, 3]
    t = np.stack([node(p, p, p, p, 1, leaf(0, 1)), node(p, p, p, p, leaf(1, 1), leaf(2, 1))])
    c = sah_ref.cost(t)
    assert (c["nodes"], c["tris"], c["cost"]) == (1.0, 0.0, 1.0)
    assert sah_ref.area(np.float32([0, 0, 0]), np.float32([1e-30, 0, 0])) == 0.0
    a = float(sah_ref.area(np.float32([0, 0, 0]), np.float32([1e-30, 1e-30, 0])))
    assert 0.0 < a < 1.1e-60 and np.isfinite(2 * a / max(0.0, 1e-300))
