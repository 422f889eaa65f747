"""bench.py --dump-outputs without a GPU: whole frames below 64 MB, and above it the same seeded sample of pixels
from every array, with their indices."""
import os

import numpy as np

import bench


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_whole_frames_below_the_limit(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.random((48, 64, 3), dtype=np.float32)
    acc = rng.random((48, 64, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"image": img, "accum": acc})
    assert sorted(os.listdir(tmp_path / "d")) == ["accum.npy", "image.npy"]
    got_img, got_acc = np.load(tmp_path / "d" / "image.npy"), np.load(tmp_path / "d" / "accum.npy")
    assert got_img.dtype == got_acc.dtype == np.float32
    assert np.array_equal(got_img, img) and np.array_equal(got_acc, acc)


def test_dump_samples_frames_above_the_limit_the_same_way_every_time(tmp_path):
    # C4's frame: 2048 x 2048 x (3 + 4) float32 = 117 MB; every pixel holds its own flat index
    h = w = 2048
    pix = np.arange(h * w, dtype=np.float32).reshape(h, w, 1)
    arrays = {"image": np.repeat(pix, 3, axis=2), "accum": np.repeat(pix, 4, axis=2)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    assert sorted(os.listdir(a)) == ["accum.npy", "image.npy", "pixel_index.npy"]
    assert _sizes(a) <= bench.DUMP_LIMIT_BYTES
    idx = np.load(a / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < h * w
    assert len(idx) > (h * w) // 3  # (most of the budget is used)
    img, acc = np.load(a / "image.npy"), np.load(a / "accum.npy")
    assert img.shape == (len(idx), 3) and acc.shape == (len(idx), 4) and img.dtype == acc.dtype == np.float32
    assert np.array_equal(img, np.repeat(idx[:, None], 3, axis=1)) and np.array_equal(acc, np.repeat(idx[:, None], 4, axis=1))
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f))
