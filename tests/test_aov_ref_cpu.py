"""CPU checks of the restatements in tests/aov_ref.py (no GPU): the primary rays it reads from the oracle's ray dump are
the frame's own (their hit count is the oracle frame's primary-hit count), and the a-trous restatement keeps a constant
image and passes pixels without a hit through."""
import numpy as np
import pytest

import aov_ref
import orc
import pyrt


@pytest.mark.parametrize("kind,rng", [("cubes", dict(spp=7)), ("lowres", dict(spp=7, spp_begin=3, spp_count=4))])
def test_restated_hits_are_the_oracle_frames_primary_hits(kind, rng):
    w, h = 37, 23
    s = pyrt.Scene(kind, w, h)
    p = pyrt.make_params(w, h, mode=pyrt.MODE_PATH, seed=4, **rng)
    a = aov_ref.aov_sums(s, p)
    _, acc, _ = orc.render(s, p, math_mode=orc.MATH_DET)
    assert np.array_equal(a["hits"].astype(np.float32), acc[..., 3])
    hit = a["hits"] > 0
    n = np.linalg.norm(a["normal"][hit] / a["hits"][hit][:, None], axis=1)
    assert (n <= 1.0001).all()  # (a mean of unit normals)
    assert (a["mesh"][hit] < s.desc.n_meshes).all() and (a["mesh"][~hit] == aov_ref.MISS).all()


def test_atrous_restatement_identities():
    h, w = 20, 30
    rng = np.random.default_rng(1)
    hits = np.full((h, w), 2, np.uint32)
    sums = dict(hits=hits, albedo=np.full((h, w, 3), 1.0, np.float32), normal=np.tile(np.float32([0, 2, 0]), (h, w, 1)),
                position=np.tile(np.float32([1, 2, 3]), (h, w, 1)))
    rgb = np.tile(np.float32([0.2, 0.4, 0.6]), (h, w, 1))
    assert np.abs(aov_ref.atrous(rgb, sums, 5, 1.0, 1.0, 1.0) - rgb).max() < 1e-6
    hits[rng.random((h, w)) < 0.4] = 0
    noisy = rng.random((h, w, 3), dtype=np.float32)
    out = aov_ref.atrous(noisy, sums, 5, 1.0, 1.0, 1.0)
    assert np.array_equal(out[hits == 0], noisy[hits == 0])
    assert np.var(out[hits > 0]) < np.var(noisy[hits > 0])
