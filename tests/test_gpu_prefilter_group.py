"""k_wvm_prefilter_group against k_wvm_prefilter at every patch size the group kernel is built for.  The two kernels call one copy of
the fold, the level bounds and the queue push (wvm_dense.hpp); this pins that a grouped batch and the same batch with
FD_WVM_GROUP=0 queue the same number of windows and return the same bytes, per member, on a small frame -- 20x20, 24x24, 16x24 and
32x16, members of different dense depth (L = 16 and L = 8), a group of two and, for 24x24, a full group of WVD_GMAX = 8 (issued by
the worker pool: six jobs and more).  The batch entry point takes single-frame pyramids only, so the kernels' frame-to-XCD split
(eight frames and more) is not reachable from here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(octave_layers=4, min_scale=0.3, max_scale=0.8)
WVD_GMAX = 8
CASES = ((20, 20, 2), (24, 24, 2), (16, 24, 2), (32, 16, 2), (24, 24, WVD_GMAX))


@pytest.fixture(scope="module")
def scene(oracle, capi, ctx, synth):
    frame = synth.make_frame(320, 240, seed=5)
    pg = capi.Pyramid(ctx, **KW)
    pg.update(frame)
    po = oracle.Pyramid(**KW)
    po.update(frame)
    yield frame, pg, po
    pg.close()


def _members(synth, oracle, frame, pw, ph, n):
    """n (wvm, svm) models on a pw x ph patch, dense depths alternating: n_per = 20 (L = 16) and n_per = 8 (L = 8)"""
    gray = oracle.bgr2gray(frame)
    calib = synth.random_patches(gray, pw, ph, 3000, np.random.default_rng(9))
    eq = synth.histeq64_np(synth.random_patches(gray, pw, ph, 264, np.random.default_rng(10)))
    sm = synth.make_svm_u8(73, eq, nsv=64, calib=eq[64:], positive_fraction=0.5)
    out = []
    for i in range(n):
        n_per, n_levels = ((20, 4), (8, 6))[i & 1]
        out.append((synth.make_wvm(71 + i, fw=pw, fh=ph, n_per=n_per, n_levels=n_levels, calib_patches=calib, min_survivors=24), sm))
    return out


@pytest.mark.parametrize("pw,ph,n", CASES)
def test_grouped_prefilter_equals_single_launches(oracle, capi, ctx, synth, scene, monkeypatch, pw, ph, n):
    frame, pg, po = scene
    total = pg.window_count(pw, ph, 1, 1)
    assert total >= 512 and sum(1 for l in po.layers() if l["h"] >= ph and l["w"] >= pw) >= 3   # the dense kernels run, on several layers
    models = _members(synth, oracle, frame, pw, ph, n)
    hs = [(capi.Wvm(ctx, wm), capi.Svm(ctx, sm)) for wm, sm in models]
    jobs = [(pg, w, s) for w, s in hs]
    try:
        monkeypatch.setenv("FD_WVM_GROUP", "0")
        r0 = capi.detect_five_stage_batch(ctx, jobs, cap=1 << 14)
        q0 = [w.last_queue_length() for w, _ in hs]
        monkeypatch.delenv("FD_WVM_GROUP")
        ctx.set_kernel_timing(2)   # the group launch leaves its member count
        try:
            r1 = capi.detect_five_stage_batch(ctx, jobs, cap=1 << 14)
            members = ctx.last_group_prefilter_ms()[1]
        finally:
            ctx.set_kernel_timing(0)
        q1 = [w.last_queue_length() for w, _ in hs]
        assert members == n, "the batch did not launch k_wvm_prefilter_group over all members"
        npos = 0
        for i, ((d0, s0), (d1, s1)) in enumerate(zip(r0, r1)):
            print("%dx%d member %d/%d: windows %d queued %d / %d stages %s" % (pw, ph, i, n, total, q0[i], q1[i], s1.tolist()))
            assert np.array_equal(s0, s1), (i, s0, s1)
            assert d0.tobytes() == d1.tobytes(), i
            assert q0[i] == q1[i], (i, q0[i], q1[i])
            assert 0 < q1[i] < total, (i, q1[i], total)   # the pre-filter rejected some windows and let some through
            npos += int(s1[0])
        assert npos > 0
        # the reference: the first two members' complete result (the others repeat their two shapes with other seeds)
        for i in range(2):
            do, so = oracle.five_stage(po, oracle.Wvm(models[i][0]), oracle.Svm(models[i][1]), cap=1 << 14)
            assert np.array_equal(r1[i][1], so), (i, r1[i][1], so)
            for f in ("cx", "cy", "w", "h"):
                assert np.array_equal(r1[i][0][f], do[f]), (i, f)
    finally:
        for w, s in hs:
            w.close(); s.close()
