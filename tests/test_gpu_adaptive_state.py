"""rt_adaptive_state: a resumable, refinable adaptive frame (include/rt/rt_abi.h).

The header's consequences are the tests, and all of them are bit-for-bit identities against code
already held to the oracle: a fresh state run to completion is rt_render_adaptive(_halves); staged
thresholds, split advances, a raised cap and a checkpoint restored into a second state all land on
the one-shot frame; and a tile at count n always holds rt_render's pixels at spp = n. The tile
counts after every call are predicted from oracle-derived samples by the numpy restatement of the
rule (tests/adaptive_state_reference.py), never from the library; the thresholds keep every
compared reference E_t at least 0.5 % away.
"""
import ctypes

import numpy as np
import pytest

from tests import adaptive_reference as ar
from tests import adaptive_state_reference as asr

pytestmark = pytest.mark.gpu

SPP, MIN, STEP, CHUNK = 96, 16, 16, 16
# the frames of the issue's table: (scene, W, H, chain of thresholds)
FRAMES = [(0, 40, 24, (0.06, 0.029, 0.02)), (0, 36, 20, (0.030, 0.02)), (4, 40, 24, (0.06, 0.045, 0.029))]


def _setup(rt, renderer, scene, W, H):
    renderer.upload(rt.World(1).build_scene(scene))
    return rt.scene_camera(scene, W, H)


def _params(rt, bg, W, H, spp, chunk=CHUNK, fmt=None, **kw):
    return rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk,
                              out_format=rt.RT_OUT_F64 if fmt is None else fmt, **kw)


def _same(a, b):
    """Every output of two frames bit for bit (mean, tile_spp, tile_error, stderr_map, half means)."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, i
        assert x.tobytes() == y.tobytes(), i


def _one_shot(rt, renderer, cam, p, thr, halves, min_spp=MIN, step_spp=STEP):
    fn = renderer.render_adaptive_halves if halves else renderer.render_adaptive
    return fn(cam, p, min_spp, step_spp, thr)


def _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, frame, chunk=CHUNK, cache=None):
    """Consequence 6: the pixels of a tile at count n are rt_render's at spp = n, same chunk."""
    mean, tile_spp = frame[0], frame[1]
    n_px = ar.tile_map(tile_spp, W, H)
    cache = {} if cache is None else cache
    for n in sorted(set(tile_spp.reshape(-1).tolist())):
        if n not in cache:
            cache[n] = renderer.render(cam, _params(rt, bg, W, H, n, chunk))
        sel = n_px == n
        assert np.array_equal(mean[sel], cache[n][sel]), n


@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("scene,W,H,chain", FRAMES)
def test_fresh_state_is_render_adaptive(rt, renderer, scene, W, H, chain, halves, fmt):
    """Consequence 1, at each frame's last threshold."""
    out_format = rt.RT_OUT_F64 if fmt == "f64" else rt.RT_OUT_F32
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, SPP, fmt=out_format)
    ref = _one_shot(rt, renderer, cam, p, chain[-1], halves)
    passes = renderer.adaptive_stats().passes
    st = renderer.adaptive_state(cam, p, MIN, STEP, halves=halves)
    try:
        assert st.advance(chain[-1], SPP) == 0
        _same(st.resolve(out_format), ref)
        s = st.stats()
        assert s.groups == passes and s.samples_traced == 64 * int(ref[1].sum())   # the groups are its passes
        assert len(set(ref[1].reshape(-1).tolist())) >= 2
    finally:
        st.close()


@pytest.mark.parametrize("min_spp,step_spp", [(20, 4), (16, 4)])
def test_fresh_state_across_buffer_batches(rt, renderer, min_spp, step_spp):
    """Consequence 1 where a group takes several buffer batches off the 2-sample chunk's grid
    (test_threshold_zero_across_buffer_batches' set-up): the carried sums give the same bits."""
    scene, W, H, spp = 7, 72, 40, 20
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, spp, chunk=0)
    renderer.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 1 << 20)
    try:
        ref = renderer.render_adaptive_halves(cam, p, min_spp, step_spp, 0.0)
        assert renderer.adaptive_stats().max_pass_batches > 1
        st = renderer.adaptive_state(cam, p, min_spp, step_spp, halves=True)
        try:
            assert st.advance(0.0, spp) == 0
            assert renderer.stats().n_batches > st.stats().groups
            _same(st.resolve(rt.RT_OUT_F64), ref)
        finally:
            st.close()
    finally:
        renderer.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 0)
    assert (ref[1] == spp).all() and np.array_equal(ref[0], renderer.render(cam, _params(rt, bg, W, H, spp, chunk=0)))


@pytest.mark.parametrize("scene,W,H,chain", FRAMES)
def test_staged_thresholds_and_split_advances(rt, renderer, scene, W, H, chain):
    """Consequences 2 and 3: each stage of the chain once whole (state a) and once as
    max_launches = 1 calls (state b). After every call the counts are the CPU simulation's and the
    pixels rt_render's (consequence 6); after every stage the two states hold the same bits, and at
    the end those of one rt_render_adaptive_halves at the last threshold."""
    samples = ar.oracle_samples(scene, W, H, SPP)
    sim_a, sim_b = (asr.SimState(samples, W, H, MIN, STEP) for _ in range(2))
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, SPP)
    a = renderer.adaptive_state(cam, p, MIN, STEP, halves=True)
    b = renderer.adaptive_state(cam, p, MIN, STEP, halves=True)
    renders = {}
    try:
        for thr in chain:
            assert a.advance(thr, SPP) == sim_a.advance(thr, SPP) == 0
            fa = a.resolve(rt.RT_OUT_F64)
            assert np.array_equal(fa[1], sim_a.tile_spp)
            _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, fa, cache=renders)
            calls = 0
            while True:
                left, exp_left = b.advance(thr, SPP, max_launches=1), sim_b.advance(thr, SPP, max_launches=1)
                assert left == exp_left and b.stats().groups == sim_b.groups <= 1
                fb = b.resolve(rt.RT_OUT_F64)
                assert np.array_equal(fb[1], sim_b.tile_spp)
                _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, fb, cache=renders)
                calls += 1
                if left == 0:
                    break
                assert calls <= 16
            _same(fa, fb)
            assert a.stats().groups_total == b.stats().groups_total == sim_a.groups_total
        print(f"margin {min(sim_a.margin(), sim_b.margin()):.4f}, counts {sorted(set(fa[1].reshape(-1).tolist()))}")
        assert min(sim_a.margin(), sim_b.margin()) >= 0.005
        _same(fa, _one_shot(rt, renderer, cam, p, chain[-1], True))
        _same(a.resolve(rt.RT_OUT_F32), _one_shot(rt, renderer, cam, _params(rt, bg, W, H, SPP, fmt=rt.RT_OUT_F32),
                                                  chain[-1], True))
    finally:
        a.close()
        b.close()


def test_raising_the_cap(rt, renderer):
    """Consequence 4: cap 48 (on the schedule, a multiple of the chunk), then 96, at 0.029."""
    scene, W, H, thr = 0, 40, 24, 0.029
    samples = ar.oracle_samples(scene, W, H, SPP)
    sim = asr.SimState(samples, W, H, MIN, STEP)
    cam, bg = _setup(rt, renderer, scene, W, H)
    st = renderer.adaptive_state(cam, _params(rt, bg, W, H, SPP), MIN, STEP, halves=True)
    try:
        assert st.advance(thr, 48) == sim.advance(thr, 48) == 0
        f48 = st.resolve(rt.RT_OUT_F64)
        assert np.array_equal(f48[1], sim.tile_spp) and sorted(set(f48[1].reshape(-1).tolist())) == [16, 32, 48]
        _same(f48, _one_shot(rt, renderer, cam, _params(rt, bg, W, H, 48), thr, True))
        assert st.advance(thr, 96) == sim.advance(thr, 96) == 0
        f96 = st.resolve(rt.RT_OUT_F64)
        assert np.array_equal(f96[1], sim.tile_spp)
        assert sim.margin() >= 0.005
        _same(f96, _one_shot(rt, renderer, cam, _params(rt, bg, W, H, 96), thr, True))
        assert st.advance(thr, 32) == 0 and st.stats().groups == 0     # a cap below the counts: nothing active
        _same(st.resolve(rt.RT_OUT_F64), f96)
    finally:
        st.close()


def test_ragged_cap_closes_a_partial_chunk(rt, renderer):
    """Cap 40 under chunk 16 closes a partial chunk: the run is rt_render_adaptive's at spp 40, a
    later cap 96 is RT_ERR_INVALID before anything is launched, and the state still resolves to the
    cap-40 frame (and still advances under caps up to 40)."""
    scene, W, H, thr = 0, 40, 24, 0.029
    cam, bg = _setup(rt, renderer, scene, W, H)
    st = renderer.adaptive_state(cam, _params(rt, bg, W, H, SPP), MIN, STEP, halves=True)
    try:
        assert st.advance(thr, 40) == 0
        f40 = st.resolve(rt.RT_OUT_F64)
        assert f40[1].max() == 40
        _same(f40, _one_shot(rt, renderer, cam, _params(rt, bg, W, H, 40), thr, True))
        _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, f40)
        total = st.stats().groups_total
        for cap in (96, 41):
            with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
                st.advance(thr, cap)
        assert st.stats().groups_total == total
        _same(st.resolve(rt.RT_OUT_F64), f40)
        assert st.checkpoint()[0].ragged_cap == 40
        assert st.advance(0.0, 40) == 0                    # the same cap, threshold off: every tile to 40
        f = st.resolve(rt.RT_OUT_F64)
        assert (f[1] == 40).all() and np.array_equal(f[0], renderer.render(cam, _params(rt, bg, W, H, 40)))
    finally:
        st.close()


def test_checkpoint_restored_into_a_second_state(rt, renderer):
    """Consequence 5, with halves, on one context."""
    scene, W, H = 0, 40, 24
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, SPP)
    a = renderer.adaptive_state(cam, p, MIN, STEP, halves=True)
    b = renderer.adaptive_state(cam, p, MIN, STEP, halves=True)
    try:
        a.advance(0.06, SPP)
        hdr, arrays = a.checkpoint()
        assert (hdr.width, hdr.height, hdr.spp_chunk, hdr.min_spp, hdr.step_spp, hdr.with_halves) == (W, H, 16, 16, 16, 1)
        assert hdr.groups_total == a.stats().groups_total > 0 and hdr.ragged_cap == 0
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            b.resolve(rt.RT_OUT_F64)                       # nothing traced yet
        b.restore(hdr, arrays)
        _same(b.resolve(rt.RT_OUT_F64), a.resolve(rt.RT_OUT_F64))
        assert b.stats().groups_total == hdr.groups_total and b.stats().min_count == 16
        assert a.advance(0.02, SPP) == b.advance(0.02, SPP) == 0
        assert a.stats().groups == b.stats().groups > 0
        fa = a.resolve(rt.RT_OUT_F64)
        _same(fa, b.resolve(rt.RT_OUT_F64))
        _same(fa, _one_shot(rt, renderer, cam, p, 0.02, True))
    finally:
        a.close()
        b.close()


def _checkerboard(ty, tx):
    j, i = np.mgrid[0:ty, 0:tx]
    return ((i + j) & 1).astype(np.float64)


def _map_round(rt, renderer, st, cam, bg, W, H, chunk, step, cap, device):
    """One caller's-map round with a 0/1 checkerboard at threshold 0.5; returns (before, after,
    stepped mask per tile). Checks the counts, consequence 6 and that unstepped tiles keep their bits."""
    before = st.resolve(rt.RT_OUT_F64)
    ty, tx = before[1].shape
    board = _checkerboard(ty, tx)
    total = st.stats().groups_total
    if device:
        import torch
        dev = torch.from_numpy(board.copy()).to("cuda:0")
        torch.cuda.synchronize()
        left = st.advance(0.5, cap, tile_error_ptr=dev.data_ptr())
    else:
        left = st.advance(0.5, cap, tile_error=board)
    after = st.resolve(rt.RT_OUT_F64)
    stepped = (board == 1) & (before[1] < cap)
    assert left == 0 and stepped.any() and not stepped.all()
    exp = np.where(stepped, np.minimum(cap, before[1].astype(np.int64) + step), before[1])
    assert np.array_equal(after[1], exp)
    assert st.stats().groups == len(set(before[1][stepped].tolist())) == st.stats().groups_total - total
    assert st.stats().samples_traced == 64 * int((exp - before[1]).sum())
    _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, after, chunk)
    keep_px = ar.tile_map(~stepped, W, H)
    assert np.array_equal(after[2][~stepped], before[2][~stepped])          # tile_error
    assert np.array_equal(after[3][keep_px], before[3][keep_px])            # stderr_map
    for k in (0, 4, 5):                                                     # mean, mean_a, mean_b
        assert np.array_equal(after[k][keep_px], before[k][keep_px])
        assert not np.array_equal(after[k][~keep_px], before[k][~keep_px])
    return before, after, stepped


@pytest.mark.parametrize("device", [False, True])
def test_a_callers_error_map_steps_the_selected_tiles_once(rt, renderer, device):
    """After advance(0.06) on scene 0, a checkerboard map (the test never looks inside it) steps
    the 1-tiles below the cap by one step each, whatever their own E_t; their refreshed tile_error
    and stderr_map are the numpy criterion's on the oracle's samples."""
    scene, W, H = 0, 40, 24
    samples = ar.oracle_samples(scene, W, H, SPP)
    cam, bg = _setup(rt, renderer, scene, W, H)
    st = renderer.adaptive_state(cam, _params(rt, bg, W, H, SPP), MIN, STEP, halves=True)
    try:
        st.advance(0.06, SPP)
        before, after, stepped = _map_round(rt, renderer, st, cam, bg, W, H, CHUNK, STEP, SPP, device)
        assert len(set(before[1][stepped].tolist())) >= 2                   # more than one group
        sim = asr.SimState(samples, W, H, MIN, STEP)
        sim.tile_spp = after[1].astype(np.int64)
        S, Q, se = sim.frame()
        _, E, _ = ar.criterion(S, Q, sim.tile_spp, W, H)
        px = ar.tile_map(stepped, W, H)
        assert ar.close(after[2][stepped], E[stepped]) and ar.close(after[3][px], se[px])
    finally:
        st.close()


def _stepwise(rt, st, thr, cap, min_r, step_r, most):
    """Drives a state to (thr, cap) one launch per call. Before each launch the CPU-tested host rule
    (rt_adaptive_next_group_host) names the group from the checkpoint's own tile_spp and tile_error
    (the E bits the device reads, so no margin is needed); the launch must move exactly that group
    to n_next, leave every other count, and return the host rule's active count on the new arrays.
    Returns the launches it took (at most `most`)."""
    launches = 0
    while True:
        _, arrays = st.checkpoint()
        n = arrays["tile_spp"].reshape(-1)
        group, n_star, n_next, _ = rt.adaptive_next_group_host(n, thr, cap, min_r, step_r,
                                                               tile_error=arrays["tile_error"].reshape(-1))
        assert group.size > 0 and (n[group] == n_star).all()
        left = st.advance(thr, cap, max_launches=1)
        assert st.stats().groups == 1
        launches += 1
        _, arrays = st.checkpoint()
        exp = n.copy()
        exp[group] = n_next
        assert np.array_equal(arrays["tile_spp"].reshape(-1), exp), launches
        assert left == rt.adaptive_next_group_host(exp, thr, cap, min_r, step_r,
                                                   tile_error=arrays["tile_error"].reshape(-1))[3], launches
        if left == 0:
            return launches
        assert launches < most


def test_regroup_beyond_one_round(rt, renderer):
    """1089 tiles: the regroup's partition loop runs twice. The state is driven one launch per call
    and every launch held to the host rule on the state's own checkpoint (_stepwise), the final
    frame to rt_render per count; the one-shot call, on the same driver, must land on the same
    bits. Then a checkerboard round on it."""
    scene, W, H, chunk, mn, step, cap, thr = 4, 264, 264, 2, 2, 2, 6, 0.05
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, cap, chunk)
    ref = renderer.render_adaptive_halves(cam, p, mn, step, thr)
    passes = renderer.adaptive_stats().passes
    assert ref[1].size == 1089 and len(set(ref[1].reshape(-1).tolist())) >= 2
    st = renderer.adaptive_state(cam, p, mn, step, halves=True)
    one = renderer.adaptive_state(cam, p, mn, step, halves=True)
    try:
        assert _stepwise(rt, one, thr, cap, mn, step, 3) == one.stats().groups_total == passes   # 2 -> 4 -> 6
        f = one.resolve(rt.RT_OUT_F64)
        _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, f, chunk)
        _same(f, ref)
        assert st.advance(thr, cap) == 0
        _same(st.resolve(rt.RT_OUT_F64), ref)
        assert st.stats().groups == passes
        before, after, stepped = _map_round(rt, renderer, st, cam, bg, W, H, chunk, step, 8, False)
        _, arrays = st.checkpoint()
        E, se = rt.adaptive_tile_errors_host(arrays["sums"], arrays["q"], arrays["tile_spp"], W, H)
        assert ar.close(after[2], E.reshape(after[2].shape)) and ar.close(after[3], se)
    finally:
        st.close()
        one.close()


def test_one_tile_frame(rt, renderer):
    scene, W, H, chunk, mn, step, cap, thr = 0, 5, 3, 2, 2, 2, 6, 0.05
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, cap, chunk)
    st = renderer.adaptive_state(cam, p, mn, step, halves=True)
    one = renderer.adaptive_state(cam, p, mn, step, halves=True)
    try:
        assert st.advance(thr, cap, max_launches=1) in (0, 1)
        assert st.advance(thr, cap) == 0
        f = st.resolve(rt.RT_OUT_F64)
        _same(f, renderer.render_adaptive_halves(cam, p, mn, step, thr))
        _check_counts_hold_rt_render(rt, renderer, cam, bg, W, H, f, chunk)
        assert _stepwise(rt, one, thr, cap, mn, step, 3) == st.stats().groups_total
        _same(one.resolve(rt.RT_OUT_F64), f)
    finally:
        st.close()
        one.close()


def test_context_is_untouched_and_sequences_repeat(rt, renderer):
    """test_context_state_is_untouched_and_call_is_deterministic's pattern around state calls; an
    rt_render_adaptive between two advances of a live state leaves its continuation unchanged; a
    second run of the sequence repeats the first."""
    scene, W, H, spp = 0, 40, 24, 48
    cam, bg = _setup(rt, renderer, scene, W, H)
    full = renderer.render(cam, _params(rt, bg, W, H, spp))
    order = np.random.default_rng(3).permutation(15)
    shard = dict(row_begin=1, row_stride=3, tile_shard=1)
    raster = renderer.render(cam, _params(rt, bg, W, H, spp, **shard))

    def sequence(interleave):
        st = renderer.adaptive_state(cam, _params(rt, bg, W, H, spp), MIN, STEP, halves=True)
        try:
            st.advance(0.06, spp, max_launches=1)
            assert renderer.stats().schedule == rt.RT_SCHED_POOL
            if interleave:
                renderer.render_adaptive(cam, _params(rt, bg, W, H, spp), MIN, STEP, 0.04)
                assert np.array_equal(renderer.render(cam, _params(rt, bg, W, H, spp, **shard)), before)
                assert renderer.stats().schedule == rt.RT_SCHED_ITEMS
            preview = st.resolve(rt.RT_OUT_F64)
            st.advance(0.04, spp)
            return preview, st.resolve(rt.RT_OUT_F64)
        finally:
            st.close()

    renderer.set_tile_order(order)
    renderer.set_schedule(rt.RT_SCHED_ITEMS)
    try:
        before = renderer.render(cam, _params(rt, bg, W, H, spp, **shard))
        ast = renderer.adaptive_stats().as_dict()
        runs = [sequence(False), sequence(True), sequence(False)]
        after = renderer.render(cam, _params(rt, bg, W, H, spp, **shard))
        assert renderer.stats().schedule == rt.RT_SCHED_ITEMS
        assert np.array_equal(renderer.render(cam, _params(rt, bg, W, H, spp)), full)
        one_shot = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, spp), MIN, STEP, 0.04)
    finally:
        renderer.set_tile_order(None)
        renderer.set_schedule(rt.RT_SCHED_AUTO)
    assert np.array_equal(before, after) and not np.array_equal(before, raster)
    assert runs[0][0][1].max() == 16 and len(set(runs[0][1][1].reshape(-1).tolist())) > 1
    for r in runs[1:]:
        _same(r[0], runs[0][0])
        _same(r[1], runs[0][1])
    _same(runs[0][1], one_shot)
    assert ast["passes"] >= 0
    assert np.array_equal(renderer.render(cam, _params(rt, bg, W, H, spp)), full)


def test_stats(rt, renderer):
    """Groups and samples of each advance and in total are the CPU simulation's; the three timings
    are measured; rt_adaptive_last_stats is not touched by state calls."""
    scene, W, H = 0, 36, 20
    samples = ar.oracle_samples(scene, W, H, SPP)
    sim = asr.SimState(samples, W, H, MIN, STEP)
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = _params(rt, bg, W, H, SPP, chunk=0)     # the automatic chunk for spp 96: 6
    renderer.render_adaptive(cam, p, MIN, STEP, 0.030)
    ast = renderer.adaptive_stats().as_dict()
    st = renderer.adaptive_state(cam, _params(rt, bg, W, H, SPP), 12, 10)
    try:
        s = st.stats()
        assert (s.spp_chunk, s.min_spp, s.step_spp, s.tiles) == (16, 16, 16, 15)
        assert (s.groups, s.groups_total, s.min_count, s.max_count, s.active_left) == (0, 0, 0, 0, 15)
        for thr in (0.030, 0.02):
            left = st.advance(thr, SPP)
            assert left == sim.advance(thr, SPP) == 0
            s = st.stats()
            assert (s.groups, s.samples_traced) == (sim.groups, sim.samples_traced) and s.groups > 0
            assert (s.groups_total, s.samples_total) == (sim.groups_total, sim.samples_total)
            assert (s.min_count, s.max_count) == (sim.tile_spp.min(), sim.tile_spp.max()) and s.active_left == 0
            assert s.trace_ms > 0 and s.moments_ms > 0 and s.classify_ms > 0
            rs = renderer.stats()
            assert rs.samples == s.samples_traced and rs.kernel_ms == s.trace_ms and rs.schedule == rt.RT_SCHED_POOL
        assert sim.margin() >= 0.005
        assert s.samples_total == 64 * int(sim.tile_spp.sum())
        st.resolve(rt.RT_OUT_F64)
        st.checkpoint()
    finally:
        st.close()
    assert renderer.adaptive_stats().as_dict() == ast


def test_errors(rt, renderer):
    W, H = 32, 24
    cam, bg = _setup(rt, renderer, 0, W, H)
    ok = lambda **kw: _params(rt, bg, W, H, 16, 4, **kw)   # noqa: E731
    ref = renderer.render(cam, ok())

    def refused(code, fn):
        with pytest.raises(rt.RTError, match=code):
            fn()
        assert np.array_equal(renderer.render(cam, ok()), ref)   # and the context still renders rt_render's bits

    lib = renderer.lib
    h = ctypes.c_void_p()
    ap, adv = rt.AdaptiveParams(4, 4, 0.0), rt.AdaptiveAdvanceParams()
    adv.threshold, adv.spp_cap = 0.05, 16
    out = rt.AdaptiveOut()
    p = ok()
    assert lib.rt_adaptive_state_create(None, ctypes.byref(cam), ctypes.byref(p), ctypes.byref(ap), 0, ctypes.byref(h)) == -1
    assert lib.rt_adaptive_state_create(renderer.h, None, ctypes.byref(p), ctypes.byref(ap), 0, ctypes.byref(h)) == -1
    assert lib.rt_adaptive_state_create(renderer.h, ctypes.byref(cam), None, ctypes.byref(ap), 0, ctypes.byref(h)) == -1
    assert lib.rt_adaptive_state_create(renderer.h, ctypes.byref(cam), ctypes.byref(p), None, 0, ctypes.byref(h)) == -1
    assert lib.rt_adaptive_state_create(renderer.h, ctypes.byref(cam), ctypes.byref(p), ctypes.byref(ap), 0, None) == -1
    assert lib.rt_adaptive_state_advance(None, ctypes.byref(adv), None) == -1
    assert lib.rt_adaptive_state_resolve(None, rt.RT_OUT_F64, 0, ctypes.byref(out), None) == -1
    assert lib.rt_adaptive_state_get(None, None, None) == -1 and lib.rt_adaptive_state_set(None, None, None) == -1
    assert lib.rt_adaptive_state_last_stats(None, None) == -1
    lib.rt_adaptive_state_destroy(None)

    for shard in (dict(row_begin=1), dict(row_stride=2), dict(tile_shard=1), dict(row_block=8)):
        refused("RT_ERR_INVALID", lambda: renderer.adaptive_state(cam, ok(**shard), 4, 4))
    refused("RT_ERR_INVALID", lambda: renderer.adaptive_state(cam, ok(), 1, 4))       # min_spp < 2
    refused("RT_ERR_INVALID", lambda: renderer.adaptive_state(cam, ok(), 4, 0))       # step_spp < 1

    st = renderer.adaptive_state(cam, ok(), 4, 4)
    other = renderer.adaptive_state(cam, _params(rt, bg, 40, 24, 16, 4), 4, 4)
    try:
        assert lib.rt_adaptive_state_advance(st.h, None, None) == -1
        assert lib.rt_adaptive_state_resolve(st.h, rt.RT_OUT_F64, 0, None, None) == -1
        assert lib.rt_adaptive_state_resolve(st.h, rt.RT_OUT_F64, 0, ctypes.byref(out), None) == -1   # mean is null
        refused("RT_ERR_INVALID", lambda: st.advance(0.05, 1))                        # spp_cap < 2
        refused("RT_ERR_INVALID", lambda: st.advance(float("nan"), 16))
        refused("RT_ERR_INVALID", lambda: st.resolve(rt.RT_OUT_F64))                  # before the first launch
        refused("RT_ERR_INVALID", lambda: st.advance(0.5, 16, tile_error=np.ones((3, 4))))   # a map on a fresh state
        assert st.advance(0.05, 16, max_launches=1) >= 0
        refused("RT_ERR_INVALID", lambda: st.advance(0.5, 16, max_launches=1, tile_error=np.ones((3, 4))))
        refused("RT_ERR_INVALID", lambda: st.resolve(7))                              # out_format
        mean = np.empty((H, W, 3))
        hv = rt.AdaptiveHalves(mean.ctypes.data, mean.ctypes.data)
        o2 = rt.AdaptiveOut(mean.ctypes.data, None, None, None)
        assert lib.rt_adaptive_state_resolve(st.h, rt.RT_OUT_F64, 0, ctypes.byref(o2), ctypes.byref(hv)) == -1   # no halves
        renderer.set_precision(rt.RT_PREC_F32)
        try:
            for fn in (lambda: st.advance(0.05, 16), lambda: renderer.adaptive_state(cam, ok(), 4, 4)):
                with pytest.raises(rt.RTError, match="RT_ERR_UNSUPPORTED"):
                    fn()
        finally:
            renderer.set_precision(rt.RT_PREC_F64)
        assert np.array_equal(renderer.render(cam, ok()), ref)
        hdr, arrays = st.checkpoint()
        o_hdr, o_arrays = other.checkpoint()
        data = rt.AdaptiveStateData(**{k: v.ctypes.data for k, v in o_arrays.items()})
        assert lib.rt_adaptive_state_set(other.h, ctypes.byref(hdr), ctypes.byref(data)) == -1       # another geometry
        assert "frame size" in lib.rt_last_error().decode()
        bad = {k: v.copy() for k, v in arrays.items()}
        bad["tile_spp"][0, 0] = 5                                                     # off the chunk grid
        refused("RT_ERR_INVALID", lambda: st.restore(hdr, bad))
        st.restore(hdr, arrays)
        preview = st.resolve(rt.RT_OUT_F64)
        renderer.upload(rt.World(1).build_scene(0))                                   # a new upload
        refused("RT_ERR_INVALID", lambda: st.advance(0.05, 16))
        _same(st.resolve(rt.RT_OUT_F64), preview)
        st.checkpoint()
        assert st.stats().max_count == 4
    finally:
        st.close()
        other.close()
    fresh = rt.Renderer(0)
    try:
        with pytest.raises(rt.RTError, match="RT_ERR_NO_SCENE"):
            fresh.adaptive_state(cam, ok(), 4, 4)
    finally:
        fresh.close()
    assert np.array_equal(renderer.render(cam, ok()), ref)
