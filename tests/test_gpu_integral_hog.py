"""The integral HOG family on the device (capi.Integral.extract_hog, svm_evaluate_samples(hog=...)): the fused launch against the
three stand-alone calls it replaces (fd_integral_gradient_patches -> fd_gradient_binning_image -> fd_hist_patch_batch /
fd_ehog_patch_batch), bit for bit, and against the CPU model of tests/integral_hog_model.py.

Everything is integer arithmetic or float arithmetic in the reference's order, so the comparisons are equalities -- with the one
exception the histogram kernels document (hog.hip, hist_normalize_wave): SpatialHistogramFilter with 1 x 1 blocks normalises the
whole vector with fp64 partial sums combined across lanes, compared at 1e-6 relative against the CPU model as in
tests/test_gpu_parity.py.  Fused and composed run the same device function and are equal there too."""
import numpy as np
import pytest

import integral_hog_model as model
import integral_model
from test_integral_hog_model import capi_params

pytestmark = pytest.mark.gpu

W, H = 200, 150


@pytest.fixture(scope="module")
def frame():
    return model.make_frame(W, H, 20261020)


@pytest.fixture(scope="module")
def reference(frame):
    """the model's integral image of the frame, the 664 samples and the model's validity per gradient grid, computed once"""
    I = integral_model.integral_fast(frame)
    I.setflags(write=False)
    samples = integral_model.make_samples(W, H)
    samples.setflags(write=False)
    valid = {}

    def valid_for(grid):
        if grid not in valid:
            v = integral_model.gradient_patches(I, grid[0], grid[1], samples)[1]
            assert v.sum() >= 500 and (~v).sum() >= 30
            v.setflags(write=False)
            valid[grid] = v
        return valid[grid]
    return I, samples, valid_for


@pytest.fixture(scope="module")
def integral(capi, ctx, frame):
    g = capi.Integral(ctx)
    g.update(frame)
    yield g
    g.close()


def composed(capi, ctx, integral, case, samples):
    """the three stand-alone calls: rows of the valid samples, and the validity"""
    rows, cols = case["grid"]
    grad, valid = integral.gradient_patches(rows, cols, samples)
    grad = grad[valid]
    nv = len(grad)
    ch = 4 if case.get("interpolate_bins") else 2
    bins = capi.gradient_binning_image(ctx, grad.reshape(nv * rows, cols, 2), case["bins"], signed_gradients=bool(case.get("signed")),
                                       interpolate=bool(case.get("interpolate_bins"))).reshape(nv, rows, cols, ch)
    hp = capi_params(capi, case)
    if case["filter"] == "ehog":
        out = capi.ehog_patch_batch(ctx, bins, hp.ehog)
    else:
        out = capi.hist_patch_batch(ctx, bins, hp.hist)
    return out.reshape(nv, -1), valid


@pytest.mark.parametrize("name", sorted(model.CASES))
def test_fused_equals_composed(capi, ctx, integral, reference, name):
    case = model.CASES[name]
    _, samples, valid_for = reference
    want_valid = valid_for(case["grid"])
    got, valid = integral.extract_hog(capi_params(capi, case), samples)
    assert got.dtype == np.float32 and got.shape == (len(samples), model.feature_length(case))
    assert np.array_equal(valid, want_valid)
    assert not got[~valid].any() and got[valid].any()
    want, cvalid = composed(capi, ctx, integral, case, samples)
    assert np.array_equal(cvalid, want_valid)
    assert np.array_equal(got[valid].view(np.uint32), want.view(np.uint32)), "%d values differ" % int((got[valid] != want).sum())


@pytest.mark.parametrize("name", ["default", model.EHOG_MODEL_CASE])
def test_against_the_cpu_model(oracle, capi, integral, reference, name):
    """every sixth sample (the ehog descriptors of the model are Python loops)"""
    case = model.CASES[name]
    I, samples, _ = reference
    samples = samples[::6]
    want, want_valid = model.features(oracle, I, case, samples)
    got, valid = integral.extract_hog(capi_params(capi, case), samples)
    assert np.array_equal(valid, want_valid) and valid.sum() > 80 and (~valid).sum() >= 5
    assert not got[~valid].any()
    if name == "default":   # one block of 1 x 1 cells: the wave-order L2 normalisation
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
        print("largest relative difference to the CPU model: %.3g" % err[want != 0].max())
        assert np.allclose(got, want, rtol=1e-6, atol=1e-9)
        assert len(np.unique(got[valid].reshape(-1, 9).argmax(1))) == 9   # the bins vary
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d values differ" % int((got != want).sum())


def test_invalid_samples(capi, integral, reference):
    _, samples, valid_for = reference
    for name in ("default", "hog2x2", "hog64", "ehog20x12"):
        case = model.CASES[name]
        want_valid = valid_for(case["grid"])
        assert want_valid.sum() >= 500 and (~want_valid).sum() >= 30
        got, valid = integral.extract_hog(capi_params(capi, case), samples)
        assert np.array_equal(valid, want_valid) and not got[~valid].any()
        assert np.array_equal(valid, capi.integral_gradient_samples_valid(W, H, case["grid"][0], case["grid"][1], samples))
        lost, vl = integral.extract_hog(capi_params(capi, case), samples[~want_valid])   # a call without a single valid sample
        assert not vl.any() and not lost.any()


def test_sample_counts(capi, integral, reference):
    """n = 0, a partial workgroup (n = 1, n = 5) and more samples than the grid holds (4 * 32 * CUs + 3: the grid stride wraps)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _, samples, valid_for = reference
    case = dict(grid=(8, 8), bins=9, filter=model.HIST_HOG, cell=4, block=1)
    hp = capi_params(capi, case)
    ok = valid_for((8, 8))
    base, v = integral.extract_hog(hp, samples[ok])
    assert v.all() and base.shape == (ok.sum(), 36)
    none, v0 = integral.extract_hog(hp, np.zeros((0, 4), np.int32))
    assert none.shape == (0, 36) and len(v0) == 0
    for n in (1, 5):
        part, vp = integral.extract_hog(hp, samples[ok][7:7 + n])
        assert vp.all() and np.array_equal(part, base[7:7 + n])
    n = 4 * 32 * cus + 3
    rep = np.resize(np.arange(ok.sum()), n)
    feats, valid = integral.extract_hog(hp, samples[ok][rep])
    assert len(feats) == n and valid.all() and np.array_equal(feats, base[rep])
    assert integral.extract_hog(hp, samples[ok][:5], download=False) is None   # rows stay on the device


def probability(m, d):
    """ProbabilisticSvmClassifier.cpp:54-58"""
    f = m["logistic_a"] + m["logistic_b"] * d
    return np.where(f >= 0, np.exp(-f) / (1.0 + np.exp(-f)), 1.0 / (1.0 + np.exp(f)))


@pytest.mark.parametrize("kernel", [2, 0], ids=["rbf", "linear"])
@pytest.mark.parametrize("name", ["default", "ehog20x12"])
def test_scoring(capi, ctx, synth, integral, reference, name, kernel):
    case = model.CASES[name]
    _, samples, valid_for = reference
    ok = valid_for(case["grid"])
    hp = capi_params(capi, case)
    feats, valid = integral.extract_hog(hp, samples)
    assert np.array_equal(valid, ok)
    m = synth.make_svm_f32(5, feats[ok], nsv=40, gamma=0.5, positive_fraction=0.4, kernel=kernel)
    m["logistic_a"], m["logistic_b"] = 0.3, -1.7
    svm = capi.Svm(ctx, m)
    target, weight = integral.svm_evaluate_samples(svm, samples, kind="hog", hog=hp)
    ref = svm.distance(feats[ok])   # the same kernel on the same vectors
    assert np.array_equal(target[ok], ref >= np.float64(np.float32(m["threshold"])))
    assert target[ok].any() and not target[ok].all()
    assert np.allclose(weight[ok], probability(m, ref), rtol=1e-14, atol=0)
    assert not target[~ok].any() and not weight[~ok].any() and (~ok).sum() >= 30   # no valid patch: (0, 0.0)
    t0, w0 = integral.svm_evaluate_samples(svm, samples[:0], hog=hp)
    assert len(t0) == 0 and len(w0) == 0
    k = int(np.nonzero(ok)[0][3])
    t1, w1 = integral.svm_evaluate_samples(svm, samples[k:k + 1], hog=hp)
    assert t1[0] == target[k] and w1[0] == weight[k]


def test_cached_binning_table(capi, integral, reference):
    """the look-up table is kept per handle for one (bins, signed, interpolate) triple: alternate two, then a fresh handle"""
    _, samples, _ = reference
    s = samples[::5]
    a, b = model.CASES["default"], model.CASES["hog30-bins2-plain-sau"]   # (9, unsigned, interpolated) and (8, signed, plain)
    ra = integral.extract_hog(capi_params(capi, a), s)[0]
    rb = integral.extract_hog(capi_params(capi, b), s)[0]
    assert np.array_equal(integral.extract_hog(capi_params(capi, a), s)[0], ra)
    assert np.array_equal(integral.extract_hog(capi_params(capi, b), s)[0], rb)
    assert np.array_equal(integral.extract_hog(capi_params(capi, b), s)[0], rb)   # the kept table
    assert ra.any() and rb.any() and ra.shape != rb.shape


def test_errors(capi, ctx, synth, integral, reference):
    _, samples, _ = reference
    s = samples[:8]
    hp = capi_params(capi, model.DEFAULT)
    feats, _ = integral.extract_hog(hp, samples[:64])
    good = capi.Svm(ctx, synth.make_svm_f32(5, feats, nsv=8, kernel=0))
    fresh = capi.Integral(ctx)   # never updated
    for call in (lambda: fresh.extract_hog(hp, s), lambda: fresh.svm_evaluate_samples(good, s, hog=hp)):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_RUNTIME and "has not been updated with an image" in str(e.value)
    fresh.close()

    def rejected(call, match):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and match in str(e.value), e.value

    u8 = np.random.default_rng(1).integers(0, 256, (16, feats.shape[1])).astype(np.uint8)
    rejected(lambda: integral.svm_evaluate_samples(capi.Svm(ctx, synth.make_svm_u8(3, u8, nsv=8, calib=u8, positive_fraction=0.5)), s, hog=hp), "f32")
    rejected(lambda: integral.svm_evaluate_samples(capi.Svm(ctx, synth.make_svm_f32(5, feats[:, :-1], nsv=8, kernel=0)), s, hog=hp),
             "f32 vectors of length 225")
    broken = {"patch": dict(model.DEFAULT, patch=(29, 30)), "bins": dict(model.DEFAULT, filter_bins=8), "2..64": dict(model.DEFAULT, grid=(65, 30), patch=(30, 65)),
              "1..255": dict(model.DEFAULT, bins=0)}
    for match, case in broken.items():
        bad = capi_params(capi, case)
        rejected(lambda: integral.extract_hog(bad, s), match)
        rejected(lambda: integral.svm_evaluate_samples(good, s, hog=bad), match)
    # four samples of a workgroup must fit the LDS: 64 x 64 with 2 x 2 blocks of 4-pixel cells does not, and the message names the way out
    big = dict(grid=(64, 64), bins=9, interpolate_bins=True, filter=model.HIST_HOG, cell=4, block=2)
    assert capi.integral_hog_feature_length(capi_params(capi, big)) == -1
    with pytest.raises(capi.FdError) as e:
        integral.extract_hog(capi_params(capi, big), s)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    for word in ("bytes of LDS", "fd_integral_gradient_patches", "fd_gradient_binning_image", "fd_hist_patch_batch"):
        assert word in str(e.value)
    # the handle still works
    again, valid = integral.extract_hog(hp, samples[:64])
    assert np.array_equal(again, feats) and valid.any()
