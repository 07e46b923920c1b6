"""OpticalFlowTransitionModel::predict for a resident particle set (fd_flow_track_fb_resident, fd_particles_sample_flow, _state_flow;
DESIGN.md 4.7): the sampler with the motion block forced both ways against tests/resident_model.py, and a six-frame chain update ->
track_fb_resident -> sample_flow -> evaluate_integral (ihog, linear SVM) -> weigh_classifier -> state_flow in which every step is
compared with the model fed the device's previous generation.  Integer outputs and float bit patterns are compared exactly, weights
in units in the last place (WEIGHT_ULP_BOUND of tests/test_gpu_condensation.py)."""
import math

import numpy as np
import pytest

import condensation_model as cm
import integral_hog_model
import resident_model as model
from test_gpu_condensation import WEIGHT_ULP_BOUND, _draws, _old_generation, _same_generation
from test_integral_hog_model import capi_params

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def forced(capi, ctx):
    """a flow handle and the crafted tracks that leave a usable motion in it, and an unusable one"""
    flow = capi.Flow(ctx, 64, 48)
    yield flow, {True: model.crafted_tracks(16, 41), False: model.crafted_tracks(16, 42, 16, 3)}
    flow.close()


@pytest.mark.parametrize("n_fresh", [0, 3], ids=["no-fresh", "fresh"])
@pytest.mark.parametrize("copies", [0, 1, 256, 257, 8192])
@pytest.mark.parametrize("n_old", [1, 3, 257])
def test_sample_flow_equals_the_model(capi, ctx, forced, n_old, copies, n_fresh):
    flow, tracks = forced
    copies = min(copies, capi.FD_PARTICLES_MAX - n_fresh)   # a full set: 8189 copies beside three fresh samples
    count = copies + n_fresh
    particles = capi.Particles.unbound(ctx, max(n_old, count, 1))
    old = _old_generation(n_old, n_old * 7 + copies)
    flow_d, fresh = _draws(count, copies, count + 1)
    fall_d, _ = _draws(count, copies, count + 2)
    for ok in (True, False):
        motion = flow.debug_motion(*tracks[ok])
        assert motion["ok"] == ok and model.same_motion(motion, model.motion(*tracks[ok]))
        particles.set(**old)
        particles.sample_flow(flow, count, copies, 0.37, flow_d, fall_d, fresh, 1000)
        want, source = model.sample_flow(old, motion, count, copies, 0.37, flow_d, fall_d, fresh, 1000)
        got = particles.get()
        assert len(particles) == len(want["x"]) == count
        _same_generation(got, want)
        assert np.array_equal(particles.trace(windows=False)[0], source)
        if copies:
            if ok:   # the copies carry the flow, not their parent's velocity
                assert np.abs(got["vx"][:copies] - float(motion["median_x"])).max() <= 20 and (got["vsize"][:copies] != old["vsize"][source[:copies]]).any()
            plain, _ = cm.sample(old, count, copies, 0.37, fall_d, fresh, 1000)
            assert all(np.array_equal(got[k], plain[k]) for k in cm.FIELDS) == (not ok)
        info, back = particles.state_flow(flow)
        assert model.same_motion(back, motion) and info["count"] == count
    particles.close()


def test_sample_flow_arguments(capi, ctx, forced):
    flow, tracks = forced
    particles = capi.Particles.unbound(ctx, 16)
    old = _old_generation(16, 3)
    particles.set(**old)
    fresh = capi.Flow(ctx, 64, 48)   # holds no motion

    def refused(call, code):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == code, e.value

    refused(lambda: particles.sample_flow(fresh, 8, 8, 0.5, np.ones((8, 3)), np.ones((8, 3)), np.zeros((0, 3), np.int32), 0), capi.FD_ERR_RUNTIME)
    refused(lambda: particles.state_flow(fresh), capi.FD_ERR_RUNTIME)
    fresh.close()
    flow.debug_motion(*tracks[True])
    for count, n_resampled in ((17, 4), (8, 9), (8, -1)):
        refused(lambda: particles.sample_flow(flow, count, n_resampled, 0.5, np.ones((16, 3)), np.ones((16, 3)), np.ones((17, 3), np.int32), 0),
                capi.FD_ERR_INVALID_ARGUMENT)
    _same_generation(particles.get(), old)   # refused calls change nothing
    particles.close()


W, H = model.CHAIN_W, model.CHAIN_H
ASPECT = 1.0
MAPS = [("resize", float(F(1.1))), ("integral",)]
HOG_CASE = dict(grid=(8, 8), bins=9, filter=integral_hog_model.HIST_HOG, cell=4, block=1)
POSITION_DEVIATION, SIZE_DEVIATION = 2.0, 0.04


@pytest.mark.parametrize("n", [65, 300])
def test_six_frame_chain(capi, ctx, n):
    frames = model.chain_frames()
    flow, integral = capi.Flow(ctx, W, H), capi.Integral(ctx)
    hp = capi_params(capi, HOG_CASE)
    x, y, size = model.CHAIN_TARGET
    # a linear model that answers to the target: its own features in frame 0, centred; the threshold at half its own score
    integral.update(frames[0])
    box = model.apply_maps(MAPS, [(x, y, size, model.cv_round(ASPECT * size))])
    feat, valid = integral.extract_hog(hp, box)
    assert valid[0]
    w = feat[0] - feat[0].mean()
    svm = capi.Svm(ctx, dict(kernel=0, dtype=1, sv=w[None, :].astype(np.float32), coeff=np.ones(1, np.float32), bias=np.float32(0)))
    own = float(svm.distance(feat)[0])
    assert own > 0
    threshold, logistic_a, logistic_b = 0.5 * own, 2.0, -4.0 / own
    particles = capi.Particles.unbound(ctx, n)
    particles.set(x=np.full(n, x), y=np.full(n, y), size=np.full(n, size), cluster_id=np.full(n, 1))
    rng = np.random.default_rng(n)
    n_resampled = cm.resampled_count(n, 0.2)
    next_id, found, worst, oks, target = 2, 0, 0, [], (x, y, size)
    for k, frame in enumerate(frames):
        flow.update(frame)
        integral.update(frame)
        old = particles.get()
        draws = []
        for _ in range(2):   # the flow model's block, then the fallback's
            z = rng.standard_normal((n_resampled, 3))
            draws.append(np.stack([POSITION_DEVIATION * z[:, 0], POSITION_DEVIATION * z[:, 1], [math.pow(2, SIZE_DEVIATION * v) for v in z[:, 2]]], 1))
        fresh = np.array([cm.fresh_sample(rng.random(), 0, 0, 12, 60, W, H) for _ in range(n - n_resampled)])
        fresh[:, 0] += rng.integers(0, W - fresh[:, 2] + 1)
        fresh[:, 1] += rng.integers(0, H - fresh[:, 2] + 1)
        u = rng.random()
        tracked = k > 0   # no previous pyramid in the first frame: the host knows, and takes the fallback itself
        if tracked:
            pts = model.chain_points(target[0], target[1], target[2], ASPECT)
            flow.track_fb_resident(pts)
            particles.sample_flow(flow, n, n_resampled, u, draws[0], draws[1], fresh, next_id)
        else:
            particles.sample(n, n_resampled, u, draws[1], fresh, next_id)
        sampled = particles.get()
        sampled_source = particles.trace(windows=False)[0]
        particles.evaluate_integral(integral, svm, ASPECT, MAPS, hog=hp)
        _, windows, valid = particles.trace()
        scores = particles.get()["score"]
        particles.weigh_classifier(logistic_a, logistic_b, threshold)
        device = particles.get()
        if tracked:
            info, motion = particles.state_flow(flow)   # the frame's one read-back
            tracks = flow.get_tracks()
            host = capi.flow_median(pts, tracks["fwd"], tracks["bwd"], tracks["fstatus"], tracks["bstatus"])
            assert model.same_motion(motion, host) and tracks["n_valid"] == host["n_valid"] and tracks["n_correct"] == host["n_correct"]
            assert np.array_equal(tracks["order"], host["order"])
            fwd, bwd, fst, bst = flow.track_fb(pts)     # the generic route's call: the same kernels
            assert fwd.tobytes() == tracks["fwd"].tobytes() and bwd.tobytes() == tracks["bwd"].tobytes()
            assert np.array_equal(fst, tracks["fstatus"]) and np.array_equal(bst, tracks["bstatus"])
            oks.append(bool(motion["ok"]))
            want, source = model.sample_flow(old, motion, n, n_resampled, u, draws[0], draws[1], fresh, next_id)
            print("frame %d: motion ok %d, %d of %d correct, flow (%.3f, %.3f) x %.4f" % (k, motion["ok"], motion["n_correct"], len(pts), motion["median_x"],
                                                                                          motion["median_y"], motion["median_ratio"]))
        else:
            info = particles.state()
            want, source = cm.sample(old, n, n_resampled, u, draws[1], fresh, next_id)
        next_id += n - n_resampled
        _same_generation(sampled, want)
        assert np.array_equal(sampled_source, source)
        xywh = model.apply_maps(MAPS, model.sample_xywh(want, ASPECT))
        assert np.array_equal(windows, xywh)
        feats, host_valid = integral.extract_hog(hp, xywh)
        assert np.array_equal(valid.astype(bool), host_valid) and scores.tobytes() == svm.distance(feats).tobytes()
        weighed, best = model.weigh_classifier(want, valid, scores, logistic_a, logistic_b, threshold)
        _same_generation(device, weighed, [f for f in cm.FIELDS if f != "weight"])
        worst = max(worst, max(cm.ulp_distance(device["weight"], weighed["weight"])))
        state = cm.filtered_state(device)
        assert info["best_score"] == best and info["weight_sum"] == cm.weight_sum(device["weight"]) and info["n_valid"] == int(valid.sum())
        assert (info["found"] == 1) == (state is not None)
        if state is not None:
            found += 1
            assert (info["x"], info["y"], info["size"], info["vx"], info["vy"]) == state[:5] and np.float32(info["vsize"]) == state[5]
            target = (info["x"], info["y"], info["size"])
            print("frame %d: state (%d, %d, %d), the texture is at (%d, %d)" % (k, info["x"], info["y"], info["size"], x + 2 * k, y + k))
    print("chain of %d: max %d ulp between the device's weights and the model's; motion ok per tracked frame: %s" % (n, worst, oks))
    assert worst <= WEIGHT_ULP_BOUND and found >= 1
    assert any(oks) and not all(oks)
    particles.close()
    flow.close()
    integral.close()
