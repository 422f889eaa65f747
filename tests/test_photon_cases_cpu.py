"""The inputs of tests/test_gpu_photon_pipeline.py reach what they are meant to reach, established with the oracle
alone (no GPU): which exit of the emission each scene takes, the stored counts of the tiny maps, the perLight steps
and the zero-slot requests of every light count, and the float32 slot count itself.  These are conditions, not
measurements: a preset that drifts fails here instead of hollowing out the GPU tests."""
import numpy as np

import orc
import photon_cases as pc
import pyrt


def emit(scene, n, seed=pc.SEEDS[0]):
    """(photons [m][7] in emission order, emission rays) of the oracle in the mode the GPU tests compare with."""
    ph, _, rays = orc.emit_photons(scene, n, pyrt.RNG_PIXEL, seed=seed, math_mode=orc.MATH_DET)
    return ph, rays


def test_case_scenes_have_the_geometry_they_claim():
    for n in (0,) + pc.LIGHT_COUNTS:
        assert pc.lights_scene(n).desc.n_lights == n and pc.lights_scene(n).desc.n_triangles == 34
    a = pc.aimed_away_scene().arrays()
    assert len(a["lights"]) == 1 and a["lights"][0, 0:3].tolist() == [0.0, 0.0, -100.0]
    assert a["lights"][0, 12:15].tolist() == [0.0, 0.0, -1.0]  # its normal: away from the room around the origin
    b = pc.closed_box_scene(pc.BRIGHT).arrays()
    assert b["tri"].shape == (12, 3) and len(b["pos"]) == 24 and (np.abs(b["pos"]) == 2).all()
    assert b["materials"][0, 2:5].tolist() == [np.float32(pc.BRIGHT)] * 3 and b["lights"][0, 0:3].tolist() == [0, 0, 0]
    # inward: every vertex normal and every triangle's geometric normal points at the centre
    p = b["pos"][b["tri"]]
    g = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", g, -p[:, 0]) > 0).all() and (np.einsum("ij,ij->i", b["nrm"], -b["pos"]) > 0).all()


def test_aimed_away_stores_nothing_and_casts_once_per_slot():
    s = pc.aimed_away_scene()
    for n in pc.EXIT_SLOTS:
        ph, rays = emit(s, n)
        assert n >= 1025 and len(ph) == 0 and rays == n == pc.slots(n, 1)


def test_dark_box_stores_every_slot():
    s = pc.closed_box_scene(pc.DARK)
    for n in pc.EXIT_SLOTS:
        ph, rays = emit(s, n)
        assert len(ph) == n and rays >= n


def test_bright_box_mostly_ends_at_the_cast_cap():
    """Watertight box: no photon misses, so one that is not stored ran into the 20-cast cap."""
    s = pc.closed_box_scene(pc.BRIGHT)
    for n in pc.EXIT_SLOTS:
        ph, rays = emit(s, n)
        assert 0 < len(ph) <= 3 * n // 4 and rays > 10 * n  # both exits occur; the cap is the common one
        # the cap itself: were every unstored photon to cast 20 times, the stored ones would cast the rest
        assert 20 * (n - len(ph)) + len(ph) <= rays <= 20 * n


def test_open_room_reaches_the_miss_after_a_bounce_and_the_other_exits():
    """One light, the open room.  Photon j's stream depends on j alone, so the emission of j + 1 photons minus the
    emission of j gives photon j's casts and whether it stored.  Stored after ONE cast: the roulette exit at the
    first hit.  Unstored after one cast: the miss on the first cast.  Stored after TWO casts whose stored hit is
    the FIRST one (the line back along its income direction meets the light's own square): a miss after one
    bounce; where the stored hit is not the first one: the roulette exit at the second hit."""
    s = pc.lights_scene(1)
    L = s.arrays()["lights"][0]
    at, vert, horiz, nrm, side = L[0:3], L[6:9], L[9:12], L[12:15], L[16]
    n = 256
    runs = [emit(s, j) for j in range(n + 1)]
    kinds = {"first_miss": 0, "roulette_first": 0, "miss_after_bounce": 0, "roulette_second": 0, "other": 0}
    for j in range(n):
        casts, stored = runs[j + 1][1] - runs[j][1], len(runs[j + 1][0]) - len(runs[j][0])
        assert np.array_equal(runs[j + 1][0][:len(runs[j][0])], runs[j][0])  # (a prefix: streams keyed by j)
        if casts == 1:
            kinds["roulette_first" if stored else "first_miss"] += 1
        elif casts == 2 and stored:
            ph = runs[j + 1][0][-1].astype(np.float64)
            p, back = ph[0:3], ph[3:6]
            t = np.dot(at - p, nrm) / np.dot(back, nrm)
            q = p + t * back - at  # where the line back meets the light's plane, from its centre
            on_light = t > 0 and abs(np.dot(q, vert)) <= 1.01 * side * np.dot(vert, vert) and \
                abs(np.dot(q, horiz)) <= 1.01 * side * np.dot(horiz, horiz)
            kinds["miss_after_bounce" if on_light else "roulette_second"] += 1
        else:
            kinds["other"] += 1
    assert min(kinds[k] for k in ("first_miss", "roulette_first", "miss_after_bounce", "roulette_second")) >= 5, kinds


def test_tiny_requests_store_exactly_one_two_and_three():
    s = pc.lights_scene(1, 16, 12)
    assert sorted(pc.TINY) == [1, 2, 3]
    for want, (req, seed) in pc.TINY.items():
        assert len(emit(s, req, seed)[0]) == want and ("lights1", req, seed) in pc.CASES


def test_requests_straddle_a_per_light_step_and_fall_below_the_light_count():
    for nl in pc.LIGHT_COUNTS:
        reqs = sorted({n for name, n, _ in pc.CASES if name == "lights%d" % nl})
        per = [pc.slots(n, nl) // nl for n in reqs]
        steps = [(a, b) for a, b, pa, pb in zip(reqs, reqs[1:], per, per[1:]) if b == a + 1 and pb == pa + 1]
        assert steps, nl
        if nl > 1:  # consecutive requests with the SAME perLight too: the step is not at every request
            assert any(b == a + 1 and pb == pa for a, b, pa, pb in zip(reqs, reqs[1:], per, per[1:])), nl
            assert any(0 < n < nl and pc.slots(n, nl) == 0 for n in reqs), nl
        # idle lanes and threads: a single slot, fewer than a wave, fewer than the compaction's 1,024 threads
        assert pc.slots(reqs[0], nl) <= 1 and any(0 < pc.slots(n, nl) < 64 for n in reqs)
    one = {pc.slots(n, 1) for name, n, _ in pc.CASES if name == "lights1"}
    assert set(pc.COMPACT_EDGES) <= one and {1, 2, 3} <= one
    assert (pc.slots(1024, 5), pc.slots(1025, 5)) == (1020, 1025)


def test_slots_is_the_oracles_count_of_emitted_photons():
    """On lights that all look away from the room every emitted photon casts exactly once, so the oracle's emission
    ray count IS the number of photons it emitted: every request up to 1,100, every request of the case lists and a
    few of the sizes the other photon tests use, for every light count."""
    a = pc.closed_box_scene(pc.DARK).arrays()  # (12 triangles, all of them behind the lights)
    away = pc.aimed_away_scene().arrays()["lights"]
    for nl in pc.LIGHT_COUNTS:
        s = pc._array_scene(a, np.repeat(away, nl, axis=0))
        for n in sorted(set(range(0, 1101)) | set(pc.requests_for(1)) | {29999, 30000, 49999, 50000, 50001}):
            ph, rays = emit(s, n)
            assert len(ph) == 0 and rays == pc.slots(n, nl), (nl, n)
    assert pc.slots(0, 3) == 0 and pc.slots(7, 0) == 0
