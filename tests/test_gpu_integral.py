"""Integral-image features on the device (capi.Integral, capi.integral_image, capi.gradient_sum_batch) against the CPU model of
tests/integral_model.py.

The family is integer arithmetic plus a few float operations per feature in the reference's order, so everything up to the
unnormalised SURF sums is compared bit for bit.  The normalised SURF descriptor is bit-identical to fd_unit_norm_batch(NORM_L2) of
the stand-alone stages and within 4 ulp of float32 of the model's float64 normalisation (one division and one square root on
values in [-1, 1]; the existing fd_unit_norm_batch test states no other bound, it compares with its own float32 formula).
SVM distances: the bound of test_svm_distance_batch for f32 RBF models, 1e-4 |d| + 1e-5 max(sum |coeff|, 1)."""
import math

import numpy as np
import pytest

import integral_model as model
from test_integral_host import HAAR_CASES, capi_params, model_features

pytestmark = pytest.mark.gpu

W, H = 160, 120
# seeds of the synthetic SVMs: with them no valid sample's distance (oracle SVM on the model's features) lies within 1e-3 of the
# threshold, which test_measurement_model asserts before it compares targets
SVM_SEEDS = {"haar": 14, "surf": 13}   # smallest gaps on the CPU model: 5.2e-3 and 3.0e-3


@pytest.fixture(scope="module")
def frame(synth):
    return synth.make_frame(W, H, seed=20261018)


@pytest.fixture(scope="module")
def reference(frame):
    """the model's integral image of the 160 x 120 frame and the sample set, computed once"""
    I = model.integral(model.bgr2gray(frame))
    I.setflags(write=False)
    samples = model.make_samples(W, H)
    samples.setflags(write=False)
    return I, samples


@pytest.fixture(scope="module")
def integral(capi, ctx, frame):
    g = capi.Integral(ctx)
    g.update(frame)
    yield g
    g.close()


def _device_copy(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


# ---- integral image ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (67, 1), (1, 67), (67, 45)], ids=lambda s: "%dx%d" % s)
def test_integral_image_small(capi, ctx, synth, size):
    w, h = size
    bgr = synth.make_frame(max(w, 8), max(h, 8), seed=w * 131 + h)[:h, :w].copy()
    gray = model.bgr2gray(bgr)
    want = model.integral(gray)
    assert np.array_equal(want, model.integral_fast(gray))
    g = capi.Integral(ctx)
    assert g.size() == (0, 0)
    for name, image in (("bgr", bgr), ("gray", gray)):
        g.update(image)
        assert g.size() == (w + 1, h + 1)
        assert np.array_equal(g.download(), want), name + " host"
        dev = _device_copy(image)
        g.update_device(dev.data_ptr(), w, h, 3 if image.ndim == 3 else 1)
        assert np.array_equal(g.download(), want), name + " device"
    assert np.array_equal(capi.integral_image(ctx, gray), want)
    g.close()


@pytest.mark.parametrize("content", ["random", "all255"])
def test_integral_image_across_tiles(capi, ctx, content):
    """1031 x 517: more than four 256-pixel row steps with a ragged tail, seventeen 32-row bands with a ragged last one"""
    w, h = 1031, 517
    gray = np.random.default_rng(5).integers(0, 256, (h, w)).astype(np.uint8) if content == "random" else np.full((h, w), 255, np.uint8)
    want = model.integral_fast(gray)
    g = capi.Integral(ctx)
    g.update(gray)
    got = g.download()
    assert got.dtype == np.int32 and got.shape == (h + 1, w + 1)
    assert np.array_equal(got, want)
    assert np.array_equal(capi.integral_image(ctx, gray), want)
    g.close()


def test_integral_matches_the_model_on_the_frame(integral, reference):
    assert np.array_equal(integral.download(), reference[0])


# ---- Haar features ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAAR_CASES))
def test_haar_features(capi, integral, reference, name):
    I, samples = reference
    case = HAAR_CASES[name]
    want, want_valid = model.haar_extract(I, model_features(case), samples)
    got, valid = integral.extract_haar(capi_params(capi, case), samples)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[~valid].any() and valid.sum() > 500
    exists = np.array([model.patch_origin(s, W + 1, H + 1)[2] for s in samples])
    x0 = samples[:, 0] - samples[:, 2] // 2
    y0 = samples[:, 1] - samples[:, 3] // 2
    right, bottom = exists & (x0 + samples[:, 2] == W + 1), exists & (y0 + samples[:, 3] == H + 1)
    assert right.sum() >= 10 and bottom.sum() >= 10
    # the one deviation: a rectangle edge that rounds to the patch size (an edge at 1.0; 0.9333 on patches up to 7 pixels) reads one
    # past the patch, which on a patch flush with the last column / row is outside the integral image.  cvRound(edge * size) is
    # monotonic in the edge, so the table's largest edges decide.
    rects = model.haar_table(model_features(case))[0]
    max_x, max_y = (rects[:, :, 0] + rects[:, :, 2]).max(), (rects[:, :, 1] + rects[:, :, 3]).max()
    past_x = np.rint((max_x * samples[:, 2].astype(np.float32)).astype(np.float64)) >= samples[:, 2]
    past_y = np.rint((max_y * samples[:, 3].astype(np.float32)).astype(np.float64)) >= samples[:, 3]
    assert np.array_equal(valid, exists & ~(right & past_x) & ~(bottom & past_y))
    if name == "edge-at-one":
        assert not valid[right | bottom].any()
    else:
        assert valid[right | bottom].any()


# ---- integral gradients, gradient sums, the SURF chain ----------------------------------------------------------------------------------
GRADIENT_GRIDS = [(2, 2), (4, 4), (12, 12), (8, 12)]


@pytest.mark.parametrize("grid", GRADIENT_GRIDS, ids=lambda g: "%dx%d" % g)
def test_integral_gradients(integral, reference, grid):
    I, samples = reference
    rows, cols = grid
    want, want_valid = model.gradient_patches(I, rows, cols, samples)
    got, valid = integral.gradient_patches(rows, cols, samples)
    assert np.array_equal(valid, want_valid) and valid.sum() > 500 and (~valid).sum() >= 30
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # with width and height >= 4 every read stays inside the patch: valid iff the patch exists
    exists = np.array([model.patch_origin(s, W + 1, H + 1)[2] for s in samples])
    big = (samples[:, 2] >= 4) & (samples[:, 3] >= 4)
    assert np.array_equal(valid[big], exists[big])


@pytest.mark.parametrize("content", ["flat", "checkerboard"])
def test_integral_gradients_extreme_content(capi, ctx, reference, content):
    """a flat image gives the code 127 everywhere; a saturated checkerboard of 8 x 8 blocks reaches the codes 0 and 254"""
    if content == "flat":
        gray = np.full((H, W), 200, np.uint8)
    else:
        y, x = np.mgrid[0:H, 0:W]
        gray = (((x // 8 + y // 8) & 1) * 255).astype(np.uint8)
    I = model.integral_fast(gray)
    samples = reference[1]
    g = capi.Integral(ctx)
    g.update(gray)
    extremes = set()
    for rows, cols in GRADIENT_GRIDS:
        want, want_valid = model.gradient_patches(I, rows, cols, samples)
        got, valid = g.gradient_patches(rows, cols, samples)
        assert np.array_equal(valid, want_valid) and np.array_equal(got, want)
        extremes |= {int(got[valid].min()), int(got[valid].max())}
        if content == "flat":
            assert (got[valid] == 127).all()
    if content == "checkerboard":
        assert 0 in extremes and 254 in extremes
    g.close()


@pytest.mark.parametrize("shape", [((12, 12), (4, 4)), ((12, 12), (12, 12)), ((8, 12), (2, 3))], ids=["12x12-4x4", "12x12-12x12", "8x12-2x3"])
def test_gradient_sums(capi, ctx, integral, reference, shape):
    (rows, cols), (cr, cc) = shape
    I, samples = reference
    grad, _ = model.gradient_patches(I, rows, cols, samples)
    rng = np.random.default_rng(rows * cols + cr)
    grad = np.concatenate([grad, rng.integers(0, 256, (40, rows, cols, 2)).astype(np.uint8)])   # every code, 255 included
    want = model.gradient_sums(grad, cr, cc)
    got = capi.gradient_sum_batch(ctx, grad, cr, cc)
    assert got.dtype == np.float32 and got.shape == (len(grad), cr * cc * 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(capi.gradient_sum_batch(ctx, grad[7:8], cr, cc), got[7:8])   # the per-Mat form: n = 1


def test_gradient_sum_divisibility_errors(capi, ctx):
    grad = np.zeros((2, 12, 12, 2), np.uint8)
    with pytest.raises(capi.FdError) as e:
        capi.gradient_sum_batch(ctx, grad, 5, 4)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert "GradientSumFilter: image row count (12) is not divisible by cell count (5)" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        capi.gradient_sum_batch(ctx, grad, 4, 5)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert "GradientSumFilter: image column count (12) is not divisible by cell count (5)" in str(e.value)


@pytest.mark.parametrize("gc", [(12, 4), (8, 2)], ids=["12-4", "8-2"])
def test_surf_descriptor(capi, ctx, integral, reference, gc):
    I, samples = reference
    _check_surf(capi, ctx, integral, I, samples, *gc)


@pytest.mark.parametrize("gc", [(64, 32), (47, 47), (64, 1)], ids=["64-32", "47-47", "64-1"])
def test_surf_descriptor_at_the_lds_limit(capi, ctx, integral, reference, gc):
    """the largest accepted (gradient count, cell count) pairs: 96 KB and 155 KB of the 160 KB of LDS of a workgroup, the longest
    descriptor (8836 floats) and the largest cells (64 x 64); every sixth sample"""
    I, samples = reference
    assert capi.surf_feature_length(*gc) == 4 * gc[1] ** 2
    _check_surf(capi, ctx, integral, I, samples[::6], *gc)


@pytest.mark.parametrize("gc", [(48, 48), (56, 56), (64, 64)], ids=["48-48", "56-56", "64-64"])
def test_surf_descriptor_beyond_the_lds_limit(synth, capi, ctx, integral, reference, gc):
    """the first rejected pair with cell count == gradient count, and the largest one: a readable error from both entry points,
    and the stand-alone calls still serve them"""
    samples = reference[1][:8]
    with pytest.raises(capi.FdError) as e:
        integral.extract_surf(gc[0], gc[1], samples)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "bytes of LDS per workgroup" in str(e.value) and "fd_gradient_sum_batch" in str(e.value)
    svm = capi.Svm(ctx, synth.make_svm_f32(3, np.random.default_rng(2).random((8, 64)).astype(np.float32), nsv=4))   # the pair is checked first
    with pytest.raises(capi.FdError) as e:
        integral.svm_evaluate_samples(svm, samples, surf=gc)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "bytes of LDS per workgroup" in str(e.value)
    grad, valid = integral.gradient_patches(gc[0], gc[0], samples)
    want_grad, want_valid = model.gradient_patches(reference[0], gc[0], gc[0], samples)
    assert np.array_equal(valid, want_valid) and np.array_equal(grad, want_grad)
    staged = capi.gradient_sum_batch(ctx, grad, gc[1], gc[1])
    assert np.array_equal(staged.view(np.uint32), model.gradient_sums(want_grad, gc[1], gc[1]).view(np.uint32))
    assert integral.extract_surf(12, 4, samples)[1].all()   # the handle still works


def _check_surf(capi, ctx, integral, I, samples, G, Cn):
    sums, exact, want_valid = model.surf_extract(I, G, Cn, samples)
    got, valid = integral.extract_surf(G, Cn, samples)
    assert got.dtype == np.float32 and got.shape == (len(samples), 4 * Cn * Cn)
    assert np.array_equal(valid, want_valid) and not got[~valid].any()
    # the fused launch equals the three stand-alone calls in a row, bit for bit
    grad, gvalid = integral.gradient_patches(G, G, samples)
    assert np.array_equal(gvalid, valid)
    staged = capi.gradient_sum_batch(ctx, grad, Cn, Cn)
    assert np.array_equal(staged.view(np.uint32)[valid], sums.view(np.uint32)[valid])
    normed = capi.unit_norm_batch(ctx, staged, 4)
    assert np.array_equal(got.view(np.uint32)[valid], normed.view(np.uint32)[valid])
    # and the model's float64 normalisation to 4 ulp of float32
    ulps = model.ulp_distance(got[valid], exact[valid])
    print("largest distance to the float64 normalisation: %.3f ulp" % ulps.max())
    assert ulps.max() <= 4.0


# ---- the measurement model --------------------------------------------------------------------------------------------------------
def _probability(m, d):
    f = m["logistic_a"] + m["logistic_b"] * d
    return math.exp(-f) / (1.0 + math.exp(-f)) if f >= 0 else 1.0 / (1.0 + math.exp(f))


def measurement_case(synth, I, samples, kind):
    """model features, the synthetic f32 RBF SVM over them, and the extraction arguments of `kind`"""
    if kind == "haar":
        feats, valid = model.haar_extract(I, model_features(HAAR_CASES["default"]), samples)
    else:
        _, exact, valid = model.surf_extract(I, 12, 4, samples)
        feats = exact.astype(np.float32)
    # about 30 % positives; the fraction puts the bias half way between two neighbouring distances of the calibration vectors
    nv = int(valid.sum())
    m = synth.make_svm_f32(SVM_SEEDS[kind], feats[valid], nsv=96, gamma=0.5, positive_fraction=(round(0.3 * (nv - 1)) + 0.5) / (nv - 1))
    return feats, valid, m


@pytest.mark.parametrize("kind", ["haar", "surf"])
def test_measurement_model(oracle, capi, ctx, synth, integral, reference, kind):
    I, samples = reference
    feats, want_valid, m = measurement_case(synth, I, samples, kind)
    threshold = float(np.float32(m["threshold"]))
    do = oracle.Svm(m).distance(feats)
    assert np.abs(do[want_valid] - threshold).min() > 1e-3, "seed %d leaves a sample at the threshold" % SVM_SEEDS[kind]
    svm = capi.Svm(ctx, m)
    if kind == "haar":
        kw = dict(haar=capi.haar_params())
        got_feats, valid = integral.extract_haar(kw["haar"], samples)
    else:
        kw = dict(surf=(12, 4))
        got_feats, valid = integral.extract_surf(12, 4, samples)
    assert np.array_equal(valid, want_valid)
    target, weight = integral.svm_evaluate_samples(svm, samples, **kw)
    # the same kernel as fd_svm_distance_batch on the extracted features: equal
    dg = svm.distance(got_feats)
    assert np.array_equal(target, valid & (dg >= threshold))
    assert np.array_equal(weight, np.where(valid, [_probability(m, d) for d in dg], 0.0))
    assert not target[~valid].any() and not weight[~valid].any() and (~valid).sum() >= 30
    # distances against the oracle's SVM on the model's features
    bound = 1e-4 * np.abs(do) + 1e-5 * max(float(np.abs(m["coeff"]).sum()), 1.0)
    print("largest distance error / bound: %.3g" % (np.abs(dg - do)[valid] / bound[valid]).max())
    assert np.all(np.abs(dg - do)[valid] <= bound[valid])
    assert np.array_equal(target[valid], do[valid] >= threshold) and 0 < target.sum() < valid.sum()
    # n = 0 and n = 1
    t0, w0 = integral.svm_evaluate_samples(svm, samples[:0], **kw)
    assert len(t0) == 0 and len(w0) == 0
    k = int(np.nonzero(valid)[0][3])
    t1, w1 = integral.svm_evaluate_samples(svm, samples[k:k + 1], **kw)
    assert t1[0] == target[k] and w1[0] == weight[k]


# ---- composition: hog with `gradients integral` ----------------------------------------------------------------------------------------
def test_hog_on_integral_gradients(oracle, capi, ctx, integral, reference):
    """IntegralGradientFilter -> GradientBinningFilter -> HogFilter through fd_integral_gradient_patches, fd_gradient_binning_image
    on the n * rows x cols stack of patches (the filter is per pixel) and fd_hist_patch_batch, against the oracle's binning and
    HOG filter on the model's gradient patches; equality, as in the existing fd_hist_patch_batch test"""
    I, samples = reference
    rows = cols = 20
    want_grad, want_valid = model.gradient_patches(I, rows, cols, samples)
    grad, valid = integral.gradient_patches(rows, cols, samples)
    assert np.array_equal(valid, want_valid)
    keep = np.nonzero(valid)[0][::9]
    grad, want_grad = grad[keep], want_grad[keep]
    bins = capi.gradient_binning_image(ctx, grad.reshape(len(keep) * rows, cols, 2), 9).reshape(len(keep), rows, cols, 2)
    hp = capi.hist_params(kind=capi.HIST_HOG, pw=cols, ph=rows, sx=1, sy=1, bins=9, cell=5, block=2)
    got = capi.hist_patch_batch(ctx, bins, hp)
    want = np.stack([np.asarray(oracle.hog_filter(oracle.gradient_binning(np.ascontiguousarray(p), 9), 9, 5, 2), np.float32).ravel() for p in want_grad])
    assert got.shape == want.shape and len(keep) > 50
    assert np.array_equal(got, want)


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(capi, ctx, synth, integral, reference):
    samples = reference[1][:4]
    fresh = capi.Integral(ctx)
    for call in (lambda: fresh.extract_haar(capi.haar_params(), samples), lambda: fresh.extract_surf(12, 4, samples),
                 lambda: fresh.gradient_patches(4, 4, samples), lambda: fresh.download()):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_RUNTIME and "has not been updated with an image" in str(e.value)
    # the overflow bound comes before the data is touched: a one-byte buffer is enough
    with pytest.raises(capi.FdError) as e:
        ctx.check(capi.lib().fd_integral_update(fresh.h, np.zeros(1, np.uint8).ctypes.data, 4000, 3000, 1, 0))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "255 * width * height > 2^31 - 1" in str(e.value)
    assert fresh.size() == (0, 0)
    fresh.close()
    with pytest.raises(capi.FdError) as e:
        integral.gradient_patches(1, 4, samples)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "rows and cols must be at least 2" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        integral.extract_surf(12, 5, samples)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "not divisible" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        integral.update(np.zeros((4, 4, 2), np.uint8))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "channels" in str(e.value)
    # dimension mismatch between the feature length and the SVM
    rng = np.random.default_rng(1)
    m = synth.make_svm_f32(3, rng.random((64, 60)).astype(np.float32), nsv=16)
    svm = capi.Svm(ctx, m)
    with pytest.raises(capi.FdError) as e:
        integral.svm_evaluate_samples(svm, samples, haar=capi.haar_params())
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "f32 vectors of length 204" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        integral.svm_evaluate_samples(svm, samples, surf=(12, 4))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "f32 vectors of length 64" in str(e.value)
    # the handle still works
    assert integral.extract_surf(12, 4, samples)[1].all()
