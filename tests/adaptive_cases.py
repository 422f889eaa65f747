"""What the rt_render_adaptive tests share (test_gpu_adaptive.py, test_gpu_adaptive_shapes.py): the reference chain of
rt_render_passes calls, the bit-for-bit comparison of an adaptive frame with the numpy rule over that chain
(tests/adaptive_ref.py), and the threshold picks."""
import numpy as np

import adaptive_ref
import pyrt

# rt_adaptive_report.active holds the first 64 passes (include/rt_amd.h)
REPORT_ACTIVE = 64

# thresholds tried by pick_threshold, coarse to fine
LADDER = (0.5, 0.3, 0.2, 0.15, 0.1, 0.07, 0.05, 0.03, 0.02, 0.01)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def chain_of(ctx, p, bg, passes):
    """accumulators after passes 0..passes-1 of the reference chain (rt_render_passes, seed + j, full ranges)."""
    acc = np.zeros((p.height, p.width, 4), np.float32)
    out = []
    for j in range(passes):
        q = pyrt.Params.from_buffer_copy(p)
        q.seed = (p.seed + j) & 0xffffffff
        ctx.render_passes(q, bg, acc)
        out.append(acc.copy())
    return out


def check_result(p, bg, chain, K, active, result):
    """An adaptive frame's (out, acc, spp, rep, st) against the rule's (K, active) over the chain, bit for bit."""
    out, acc, spp, rep, st = result
    w, h = p.width, p.height
    Kp = adaptive_ref.per_pixel(K, w, h)
    assert np.array_equal(spp, (Kp * p.spp).astype(np.uint32)), "per-pixel sample counts differ from the rule's"
    exp_acc = adaptive_ref.assemble(chain, K, w, h)
    assert np.array_equal(bits(acc), bits(exp_acc)), "accumulator differs from the chain at %d pixels" % int(
        np.any(bits(acc) != bits(exp_acc), axis=2).sum())
    exp_out = adaptive_ref.resolve(exp_acc, bg, Kp * p.spp)
    assert np.array_equal(bits(out), bits(exp_out)), "image differs from the per-pixel resolve"
    # the report stores the first 64 passes' counts; the entries after them stay zero
    n = min(len(active), REPORT_ACTIVE)
    assert rep.passes == len(active) and list(rep.active)[:n] == active[:n]
    assert not any(list(rep.active)[n:])
    assert rep.granules == K.size and rep.pixel_samples == int(spp.astype(np.uint64).sum())
    assert st.samples == rep.pixel_samples and st.rays_closest > 0
    assert rep.render_ms > 0 and rep.adapt_ms > 0 and rep.total_ms >= rep.render_ms


def check_frame(ctx, p, bg, chain, threshold, max_passes, min_passes=0, floor=0.):
    """Run the adaptive frame and compare everything with the restatement; returns K per granule."""
    K, active = adaptive_ref.run_rule(chain, bg, p.spp, threshold, max_passes, min_passes, floor)
    out, acc, spp, rep, st = ctx.render_adaptive(p, bg, threshold, max_passes, min_passes, floor)
    check_result(p, bg, chain, K, active, (out, acc, spp, rep, st))
    return K, out, acc, spp, rep


def pick_threshold(chain, bg, max_passes, P_):
    """A threshold at which granules retire after at least three different pass counts."""
    for t in LADDER:
        K, _ = adaptive_ref.run_rule(chain, bg, P_, t, max_passes)
        if len(np.unique(K)) >= 3:
            return t, K
    raise AssertionError("no threshold retires granules at three different passes")


# thresholds tried by pick_chunk_threshold: 0.5 down to 0.005 in steps of 10 %.  The chunk conditions need the fifth pass
# (the first one after the default min_passes) above CHUNK active granules and the sixth below, a window that is a few
# per cent of the threshold wide at some samples-per-pass.
CHUNK_LADDER = tuple(float(np.float32(0.5 * 0.9 ** i)) for i in range(45))

CHUNK = 1024  # granules per iteration of the list kernels' loops (one workgroup of 1,024 threads: csrc/adaptive.hip)


def chunk_conditions(K, active):
    """The passes of a frame of more than CHUNK granules, from the rule's output alone, that take the list kernels
    through their second loop iteration with a carried offset.  Returns (mid, full, short):

    mid    passes in which a granule past the first CHUNK is active while one of the first CHUNK (row-major) is
           retired: k_adapt_compact enters its second iteration with 0 < base < CHUNK and writes list[base + off]
    full   those of mid with more than CHUNK active granules: k_adapt_expand runs a second iteration as well, over
           a list whose first CHUNK entries are not the first CHUNK granules
    short  passes after one of mid with 1..CHUNK-1 active granules: one iteration again, and a list shorter than the
           stale tail the pass before left in list and tiles

    A granule is active in pass k (0-based) when K > k: it ran K passes, 0..K-1."""
    Kf = K.reshape(-1)
    assert Kf.size > CHUNK
    mid, full, short = [], [], []
    for k, n in enumerate(active):
        act = Kf > k
        assert int(act.sum()) == n
        if mid and 1 <= n < CHUNK:
            short.append(k)
        if act[CHUNK:].any() and not act[:CHUNK].all():
            mid.append(k)
            if n > CHUNK:
                full.append(k)
    return mid, full, short


def pick_chunk_threshold(chain, bg, max_passes, P_, need_full, ladder=CHUNK_LADDER):
    """A threshold whose rule output has a `mid` pass (a `full` one if need_full) and a later `short` pass."""
    for t in ladder:
        K, active = adaptive_ref.run_rule(chain, bg, P_, t, max_passes)
        if K.size <= CHUNK:
            break
        mid, full, short = chunk_conditions(K, active)
        first = full if need_full else mid
        if first and short and short[-1] > first[0]:
            return t, K, active
    raise AssertionError("no threshold of the ladder gives the chunk conditions")
