"""SingleClassifierModel on the integral family for a resident particle set (fd_particles_create_unbound, _evaluate_integral,
_weigh_classifier) on a 64 x 48 seeded image.  The sample list k_particles_xywh writes is read back through the trace
and compared with tests/resident_model.py; validity and scores with the host entry points on the mapped list (the scores bit for
bit: the same kernels on the same rows); the weights with the model in units in the last place (the device's exp against libm's,
WEIGHT_ULP_BOUND of tests/test_gpu_condensation.py)."""
import numpy as np
import pytest

import condensation_model as cm
import integral_hog_model
import resident_model as model
from test_gpu_condensation import WEIGHT_ULP_BOUND, _same_generation
from test_integral_hog_model import capi_params

pytestmark = pytest.mark.gpu

W, H, ASPECT = 64, 48, 1.25
SCALE = float(np.float32(1.1))   # the apps read the scale as a float
MAPS = {"none": [], "integral": [("integral",)], "resize+integral": [("resize", SCALE), ("integral",)]}
HOG_CASE = dict(grid=(8, 8), bins=9, filter=integral_hog_model.HIST_HOG, cell=4, block=1)
LOGISTIC_A, LOGISTIC_B = 0.3, -1.7


def _samples(n=257):
    """{x, y, size}: a regular one first, then off-image, empty, negative and huge ones, then border-flush ones (size 20 is 20 x 25,
    23 x 29 behind the default chain: its patch starts at (0, 0) for x = 11, y = 14 and ends on the last row and column of the
    integral image for x = 53, y = 34) with their neighbours one pixel outside, then seeded ones that hang over every border"""
    rng = np.random.default_rng(11)
    rows = [(30, 24, 16), (-40, 20, 30), (W + 40, 20, 30), (30, -60, 30), (30, 24, 0), (30, 24, -3), (30, 24, 4000), (11, 14, 20), (53, 34, 20),
            (10, 14, 20), (54, 34, 20), (32, 24, 38), (32, 24, 39), (31, 23, 15), (32, 24, 1), (32, 24, 2)]
    rest = np.stack([rng.integers(-5, W + 5, n), rng.integers(-5, H + 5, n), rng.integers(3, 40, n)], 1).tolist()
    return np.array((rows + rest)[:n], np.int64)


@pytest.fixture(scope="module")
def scene(capi, ctx, synth):
    """the image's integral image, and per feature kind its parameters (as keyword of evaluate_integral), the rows of every sample of
    the mapped default list and a linear SVM on them"""
    rng = np.random.default_rng(20261020)
    image = np.clip(np.kron(rng.integers(40, 216, (H // 4, W // 4)), np.ones((4, 4))) + rng.integers(-30, 30, (H, W)), 0, 255).astype(np.uint8)
    integral = capi.Integral(ctx)
    integral.update(image)
    s = _samples()
    gen = cm.generation(len(s), x=s[:, 0], y=s[:, 1], size=s[:, 2])
    mapped = model.apply_maps(MAPS["resize+integral"], model.sample_xywh(gen, ASPECT))
    kinds = {"haar": dict(haar=capi.haar_params()), "surf": dict(surf=(12, 4)), "hog": dict(hog=capi_params(capi, HOG_CASE))}
    extract = {"haar": lambda q: integral.extract_haar(kinds["haar"]["haar"], q), "surf": lambda q: integral.extract_surf(12, 4, q),
               "hog": lambda q: integral.extract_hog(kinds["hog"]["hog"], q)}
    out = dict(integral=integral, gen=gen, mapped=mapped, kinds=kinds, extract=extract, svm={}, model={})
    for name in kinds:
        feats, valid = extract[name](mapped)
        assert 20 <= valid.sum() <= len(s) - 7, (name, valid.sum())
        m = synth.make_svm_f32(5, feats[valid], nsv=12, positive_fraction=0.4, kernel=0)
        m["logistic_a"], m["logistic_b"] = LOGISTIC_A, LOGISTIC_B
        out["model"][name], out["svm"][name] = m, capi.Svm(ctx, m)
    yield out
    integral.close()


@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("maps", sorted(MAPS))
def test_sample_list_equals_the_model(capi, ctx, scene, maps, n):
    s = _samples(n)
    particles = capi.Particles.unbound(ctx, n)
    gen = cm.generation(n, x=s[:, 0], y=s[:, 1], size=s[:, 2])
    particles.set(**gen)
    particles.evaluate_integral(scene["integral"], scene["svm"]["hog"], ASPECT, MAPS[maps], **scene["kinds"]["hog"])
    _, windows, valid = particles.trace()
    want = model.apply_maps(MAPS[maps], model.sample_xywh(gen, ASPECT))
    assert np.array_equal(windows, want), np.flatnonzero((windows != want).any(1))[:5]
    assert np.array_equal(valid.astype(bool), scene["extract"]["hog"](want)[1])
    if n == 257:
        assert (want[:, 2] != want[:, 3]).any() and 0 < valid.sum() < n
        if maps == "resize+integral":   # halves were rounded: 1.1f * 15 = 16.5000004 -> 17 where 1.1 gives 16
            assert want[13].tolist() == [32, 24, 18, 22] and want[7].tolist() == [11, 14, 23, 29]
    particles.close()


@pytest.mark.parametrize("kind", ["haar", "surf", "hog"])
def test_evaluate_and_weigh(capi, ctx, scene, kind):
    integral, svm, m, mapped = scene["integral"], scene["svm"][kind], scene["model"][kind], scene["mapped"]
    n = len(mapped)
    rng = np.random.default_rng(4)
    gen = {k: v.copy() for k, v in scene["gen"].items()}
    gen["weight"] = rng.random(n) * 3          # weights other than 1: the classifier sets the weight, it does not multiply
    gen["cluster_id"] = rng.integers(0, 4, n).astype(np.int32)
    particles = capi.Particles.unbound(ctx, n)
    particles.set(**gen)
    particles.evaluate_integral(integral, svm, ASPECT, MAPS["resize+integral"], **scene["kinds"][kind])
    _, windows, valid = particles.trace()
    got = particles.get()
    assert np.array_equal(windows, mapped)
    feats, host_valid = scene["extract"][kind](mapped)
    assert np.array_equal(valid.astype(bool), host_valid) and not valid[[1, 2, 3, 5, 6, 9, 10]].any() and valid[0]
    assert got["score"].tobytes() == svm.distance(feats).astype(np.float64).tobytes()    # the same kernel on the same rows
    _same_generation(got, gen, [k for k in cm.FIELDS if k != "score"])                    # evaluate changes the scores only
    host_target, host_weight = integral.svm_evaluate_samples(svm, mapped, **scene["kinds"][kind])
    scores = got["score"]
    threshold = float(scores[np.flatnonzero(valid)[5]])                                   # a score exactly on the threshold
    for thr in (float(np.float32(m["threshold"])), threshold):
        particles.set(**gen)
        particles.evaluate_integral(integral, svm, ASPECT, MAPS["resize+integral"], **scene["kinds"][kind])
        particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, thr)
        device = particles.get()
        want, best = model.weigh_classifier(gen, valid, scores, LOGISTIC_A, LOGISTIC_B, thr)
        _same_generation(device, want, [k for k in cm.FIELDS if k != "weight"])
        ulps = cm.ulp_distance(device["weight"], want["weight"])
        print("%s, threshold %r: max %d ulp over %d weights" % (kind, thr, max(ulps), n))
        assert max(ulps) <= WEIGHT_ULP_BOUND
        assert not device["weight"][valid == 0].any()
        if thr == threshold:
            assert device["target"][np.flatnonzero(valid)[5]] == 1 and scores[np.flatnonzero(valid)[5]] == thr
        info = particles.state()
        assert info["best_score"] == best and info["n_valid"] == int(valid.sum()) and info["n_target"] == int(device["target"].sum())
        assert 0 < info["n_target"] <= info["n_valid"]
        if thr != threshold:   # the host's SingleClassifierModel on the same list
            assert np.array_equal(device["target"].astype(bool), host_target)
            assert max(cm.ulp_distance(device["weight"], host_weight)) <= WEIGHT_ULP_BOUND
    particles.close()


def test_arguments(capi, ctx, synth, scene):
    integral, hog, svm = scene["integral"], scene["kinds"]["hog"], scene["svm"]["hog"]
    particles = capi.Particles.unbound(ctx, 8)
    s = _samples(8)
    particles.set(x=s[:, 0], y=s[:, 1], size=s[:, 2])
    before = particles.get()

    def refused(call, code, match=""):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == code and match in str(e.value), e.value

    refused(lambda: particles.evaluate(0, ASPECT), capi.FD_ERR_RUNTIME, "no tracker")
    refused(lambda: particles.weigh_classifier(0.0, -1.0, 0.0), capi.FD_ERR_RUNTIME, "not been evaluated")
    u8 = np.random.default_rng(1).integers(0, 256, (16, 36)).astype(np.uint8)
    refused(lambda: particles.evaluate_integral(integral, capi.Svm(ctx, synth.make_svm_u8(3, u8, nsv=8, calib=u8, positive_fraction=0.5)), ASPECT, [], **hog),
            capi.FD_ERR_INVALID_ARGUMENT, "f32")
    refused(lambda: particles.evaluate_integral(integral, scene["svm"]["surf"], ASPECT, [], **hog), capi.FD_ERR_INVALID_ARGUMENT, "f32 vectors of length 36")
    refused(lambda: particles.evaluate_integral(integral, svm, ASPECT, [("integral",)] * 5, **hog), capi.FD_ERR_INVALID_ARGUMENT, "sample maps")
    refused(lambda: particles.evaluate_integral(integral, svm, ASPECT, [(9,)], **hog), capi.FD_ERR_INVALID_ARGUMENT, "map kind")
    fresh = capi.Integral(ctx)   # never updated
    refused(lambda: particles.evaluate_integral(fresh, svm, ASPECT, [], **hog), capi.FD_ERR_RUNTIME, "has not been updated with an image")
    fresh.close()
    refused(lambda: particles.weigh_classifier(0.0, -1.0, 0.0), capi.FD_ERR_RUNTIME, "not been evaluated")   # refused calls evaluate nothing
    _same_generation(particles.get(), before)
    for capacity in (0, capi.FD_PARTICLES_MAX + 1):
        refused(lambda: capi.Particles.unbound(ctx, capacity), capi.FD_ERR_INVALID_ARGUMENT)
    # every other call works on an unbound set: sample, state, an empty generation through the whole chain
    particles.sample(8, 4, 0.5, np.ones((4, 3)), np.full((4, 3), 20, np.int32), 7)
    assert len(particles) == 8 and particles.state()["count"] == 8
    particles.sample(0, 0, 0.5, np.zeros((0, 3)), np.zeros((0, 3), np.int32), 0)
    particles.evaluate_integral(integral, svm, ASPECT, MAPS["integral"], **hog)
    particles.weigh_classifier(0.0, -1.0, 0.0)
    info = particles.state()
    assert info["count"] == 0 and info["found"] == 0 and info["n_valid"] == 0
    particles.close()
