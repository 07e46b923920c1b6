"""Sampled pyramid features on the device: the glbp layer filter (FD_LAYER_GRADMAG_LBP) and the stand-alone magnitude filter byte for
byte against tests/pyramid_samples_model.py, the sampled histogram / extended-HOG features bit for bit against the patch and the
strided entry points, and SingleClassifierModel::evaluate on top of them (fd_hist_svm_evaluate_samples)."""
import itertools

import numpy as np
import pytest

import pyramid_samples_model as model

pytestmark = pytest.mark.gpu

PYR = dict(octave_layers=3, min_scale=0.3, max_scale=1.0)
LBP_TYPES = (0, 1, 2, 3)
GRAD_KERNELS = (1, 3, -1)   # -1: CV_SCHARR
BLURS = (0, 3)


def make_image(w, h, seed):
    """noise plus a smooth ramp, BGR"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 40.0 + 120.0 * xx / max(w - 1, 1) + 50.0 * yy / max(h - 1, 1)
    img = ramp[:, :, None] + rng.normal(0, 25, (h, w, 3)) + np.array([0.0, 10.0, -10.0])
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def image():
    return make_image(120, 96, 20261020)


@pytest.fixture(scope="module")
def gray_layers(capi, ctx):
    """the gray layers of an image under PYR (the input of the layer filters), computed once per image size"""
    cache = {}

    def get(img):
        key = img.tobytes()
        if key not in cache:
            p = capi.Pyramid(ctx, **PYR)
            p.update(img)
            cache[key] = [p.layer(i) for i in range(len(p.layers()))]
        return cache[key]
    return get


def layer_pyramid(capi, ctx, img, kind, **kw):
    p = capi.Pyramid(ctx, **PYR)
    p.set_layer_filter(kind, **kw)
    p.update(img)
    return p


# ---- the glbp layer filter
@pytest.mark.parametrize("size", [(120, 96), (9, 7), (70, 50)], ids=lambda s: "%dx%d" % s)
def test_glbp_layers_equal_the_model(capi, ctx, gray_layers, size):
    """every kept layer byte for byte, all LBP types x gradient kernels x blurs; 9 x 7: layers of a few pixels a side; 70 x 50:
    more than one tile in both directions"""
    img = make_image(size[0], size[1], 7 + size[0])
    grays = gray_layers(img)
    assert len(grays) >= 4
    if size == (9, 7):
        assert min(g.shape[0] for g in grays) <= 3
    if size == (70, 50):
        assert grays[0].shape == (50, 70)   # wider than one 64-pixel tile, higher than one 16-row tile
    p = capi.Pyramid(ctx, **PYR)
    for lbp_type, ksize, blur in itertools.product(LBP_TYPES, GRAD_KERNELS, BLURS):
        p.set_layer_filter(capi.FD_LAYER_GRADMAG_LBP, grad_kernel=ksize, lbp_type=lbp_type, blur_kernel=blur)
        p.update(img)
        infos = p.layers()
        assert len(infos) == len(grays) and all(i["ch"] == 1 for i in infos)
        for i, g in enumerate(grays):
            got = p.layer(i)
            want = model.glbp_layer(g, ksize, blur, lbp_type)
            assert got.shape == want.shape and np.array_equal(got, want), (lbp_type, ksize, blur, i, g.shape)


def test_glbp_rejects_bad_parameters(capi, ctx):
    p = capi.Pyramid(ctx, **PYR)
    for kw in (dict(grad_kernel=2), dict(lbp_type=4), dict(lbp_type=-1)):
        with pytest.raises(capi.FdError) as e:
            p.set_layer_filter(capi.FD_LAYER_GRADMAG_LBP, **kw)
        assert e.value.args and ("GradientFilter" in str(e.value) or "LbpFilter" in str(e.value))


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (33, 17)], ids=lambda s: "%dx%d" % s)
def test_gradient_magnitude_image(capi, ctx, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    grad = rng.integers(0, 256, shape + (2,)).astype(np.uint8)
    grad.reshape(-1, 2)[0] = (255, 255)
    got = capi.gradient_magnitude_image(ctx, grad)
    assert got.dtype == np.uint8 and got.shape == shape and np.array_equal(got, model.gradient_magnitude(grad))


# ---- sampled features
LAYER_CONFIGS = {
    "gradbin2": dict(kind="GRADBIN", kw=dict(bins=9, interpolate=False), bins=9, sau=False),
    "gradbin4": dict(kind="GRADBIN", kw=dict(bins=8, signed_gradients=True, interpolate=True, grad_kernel=3), bins=8, sau=True),
    "lbp": dict(kind="LBP", kw=dict(lbp_type=2), bins=16, sau=False),
    "glbp": dict(kind="GRADMAG_LBP", kw=dict(lbp_type=1, grad_kernel=3, blur_kernel=3), bins=59, sau=False),
}
PATCHES = {(16, 16): dict(cell=8, cell_h=0), (12, 20): dict(cell=6, cell_h=5)}


def hist_cases(capi, cfg, pw, ph):
    """the four FD_HIST_* kinds, interpolating and not, that the layer kind admits"""
    geo = PATCHES[(pw, ph)]
    hog_ok = cfg["kind"] == "GRADBIN"
    for interpolate in (False, True):
        if hog_ok:
            yield capi.hist_params(0, pw, ph, 1, 1, bins=cfg["bins"], cell=geo["cell"], block=2, interpolate=interpolate,
                                   signed_and_unsigned=cfg["sau"], cell_h=geo["cell_h"])
            yield capi.hist_params(2, pw, ph, 1, 1, bins=cfg["bins"], levels=2, interpolate=interpolate, signed_and_unsigned=cfg["sau"])
        yield capi.hist_params(1, pw, ph, 1, 1, bins=cfg["bins"], cell=geo["cell"], block=1, interpolate=interpolate, normalization=2,
                               cell_h=geo["cell_h"])
        yield capi.hist_params(1, pw, ph, 1, 1, bins=cfg["bins"], cell=geo["cell"], block=2, interpolate=interpolate, concatenate=True,
                               normalization=1, cell_h=geo["cell_h"])
        yield capi.hist_params(3, pw, ph, 1, 1, bins=cfg["bins"], levels=2, interpolate=interpolate, normalization=3)


def samples_for(p, pw, ph):
    layers = p.layers()
    s = model.make_samples(layers, p.inc, pw, ph)
    want = model.sample_windows(layers, p.inc, pw, ph, s)
    ok = want[:, 3] == 1
    assert 2 * ok.sum() >= len(s) and (~ok).sum() >= 8 and set(want[ok, 0].tolist()) == set(range(len(layers)))
    return s, want, ok


def crop(layer_images, windows, pw, ph):
    return np.stack([layer_images[l][by:by + ph, bx:bx + pw] for l, bx, by, _ in windows.tolist()])


@pytest.mark.parametrize("name", sorted(LAYER_CONFIGS))
def test_sampled_hist_features_equal_the_pinned_paths(capi, ctx, image, name):
    cfg = LAYER_CONFIGS[name]
    p = layer_pyramid(capi, ctx, image, getattr(capi, "FD_LAYER_" + cfg["kind"]), **cfg["kw"])
    limg = [p.layer(i) for i in range(len(p.layers()))]
    assert len(limg) == 6
    ncases = 0
    for (pw, ph) in PATCHES:
        s, want, ok = samples_for(p, pw, ph)
        assert np.array_equal(p.sample_windows(pw, ph, s), want)
        patches = crop(limg, want[ok], pw, ph)
        allw = p.windows(pw, ph, 1, 1)
        row_of = {(int(r[0]), int(r[1]), int(r[2])): i for i, r in enumerate(allw)}
        # the strided scan stops one short of the right and the bottom border (x + pw < width, DirectPyramidFeatureExtractor.cpp:
        # 108-121): those windows exist only as samples, every other one is compared with its row of the scan
        keys = [(l, bx, by) for l, bx, by, _ in want[ok].tolist()]
        scanned = np.array([k in row_of for k in keys])
        lw = np.array([limg[l].shape[1] for l, _, _ in keys])
        lh = np.array([limg[l].shape[0] for l, _, _ in keys])
        flush = (want[ok, 1] + pw == lw) | (want[ok, 2] + ph == lh)
        assert np.array_equal(~scanned, flush) and {k[0] for k, there in zip(keys, scanned) if there} == set(range(len(limg)))
        rows = np.array([row_of[k] for k, there in zip(keys, scanned) if there])
        for hp in hist_cases(capi, cfg, pw, ph):
            feats, valid = capi.hist_extract_samples(ctx, p, hp, s)
            assert np.array_equal(valid, ok)
            assert feats.shape[1] > 0 and not feats[~ok].any()            # invalid rows are zero
            assert feats[ok].any()
            a = capi.hist_patch_batch(ctx, patches, hp)
            assert np.array_equal(feats[ok], a), (name, pw, ph, hp.kind, hp.interpolate)
            b = capi.extract_hist(ctx, p, hp)
            assert len(b) == len(allw) and np.array_equal(feats[ok][scanned], b[rows]), (name, pw, ph, hp.kind, hp.interpolate)
            ncases += 1
    assert ncases == (20 if cfg["kind"] == "GRADBIN" else 12)


@pytest.mark.parametrize("name", ["gradbin2", "gradbin4"])
def test_sampled_ehog_features_equal_the_patch_filter(capi, ctx, image, name):
    cfg = LAYER_CONFIGS[name]
    p = layer_pyramid(capi, ctx, image, capi.FD_LAYER_GRADBIN, **cfg["kw"])
    limg = [p.layer(i) for i in range(len(p.layers()))]
    for (pw, ph), geo in PATCHES.items():
        s, want, ok = samples_for(p, pw, ph)
        patches = crop(limg, want[ok], pw, ph)
        for interpolate in (False, True):
            ep = capi.ehog_patch_params(pw, ph, bins=cfg["bins"], cell_w=geo["cell"], cell_h=geo["cell_h"], interpolate=interpolate,
                                        signed_and_unsigned=cfg["sau"])
            feats, valid = capi.ehog_extract_samples(ctx, p, ep, s)
            assert np.array_equal(valid, ok) and not feats[~ok].any() and feats[ok].any()
            a = capi.ehog_patch_batch(ctx, patches, ep)
            assert np.array_equal(feats[ok], a.reshape(len(a), -1)), (name, pw, ph, interpolate)


def test_more_samples_than_workgroups_and_the_small_counts(capi, ctx, image):
    """n = CUs * 32 + 3: the grid-stride loop of k_hist_features wraps; n = 1, n = 0 and a list without a single window"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = layer_pyramid(capi, ctx, image, capi.FD_LAYER_GRADBIN, bins=9)
    hp = capi.hist_params(0, 16, 16, 1, 1, bins=9, cell=8, block=2)
    s, want, ok = samples_for(p, 16, 16)
    base, _ = capi.hist_extract_samples(ctx, p, hp, s[ok])
    n = cus * 32 + 3
    rep = np.resize(np.arange(ok.sum()), n)
    feats, valid = capi.hist_extract_samples(ctx, p, hp, s[ok][rep])
    assert len(feats) == n > cus * 32 and valid.all() and np.array_equal(feats, base[rep])
    one, v1 = capi.hist_extract_samples(ctx, p, hp, s[ok][3:4])
    assert v1.tolist() == [True] and np.array_equal(one, base[3:4])
    none, v0 = capi.hist_extract_samples(ctx, p, hp, np.zeros((0, 4), np.int32))
    assert none.shape == (0, base.shape[1]) and len(v0) == 0
    lost, vl = capi.hist_extract_samples(ctx, p, hp, s[~ok])
    assert len(lost) == (~ok).sum() and not vl.any() and not lost.any()
    svm = capi.Svm(ctx, dict(kernel=0, dtype=1, sv=base[:1], coeff=np.ones(1, np.float32), bias=0.0))
    t, w = capi.hist_svm_evaluate_samples(ctx, p, hp, svm, s[~ok])
    assert not t.any() and not w.any()
    t, w = capi.hist_svm_evaluate_samples(ctx, p, hp, svm, np.zeros((0, 4), np.int32))
    assert len(t) == 0 and len(w) == 0


# ---- SingleClassifierModel::evaluate
def probability(m, d):
    """ProbabilisticSvmClassifier.cpp:54-58"""
    f = m["logistic_a"] + m["logistic_b"] * d
    return np.where(f >= 0, np.exp(-f) / (1.0 + np.exp(-f)), 1.0 / (1.0 + np.exp(f)))


@pytest.mark.parametrize("kernel", [2, 0], ids=["rbf", "linear"])
@pytest.mark.parametrize("chain", ["hist", "ehog"])
def test_svm_evaluate_samples(capi, ctx, synth, image, kernel, chain):
    p = layer_pyramid(capi, ctx, image, capi.FD_LAYER_GRADBIN, bins=9)
    if chain == "hist":
        prm = capi.hist_params(0, 16, 16, 1, 1, bins=9, cell=8, block=2)
        extract = capi.hist_extract_samples
    else:
        prm = capi.ehog_patch_params(16, 16, bins=9, cell_w=4)
        extract = capi.ehog_extract_samples
    s, want, ok = samples_for(p, 16, 16)
    feats, valid = extract(ctx, p, prm, s)
    m = synth.make_svm_f32(5, feats[ok], nsv=40, gamma=0.5, positive_fraction=0.4, kernel=kernel)
    m["logistic_a"], m["logistic_b"] = 0.3, -1.7
    svm = capi.Svm(ctx, m)
    target, weight, dist = capi.hist_svm_evaluate_samples(ctx, p, prm, svm, s, want_distance=True)
    ref = svm.distance(feats[ok])
    assert np.array_equal(dist[ok], ref) and not dist[~ok].any()           # the same kernel on the same vectors: the same bits
    assert np.array_equal(target[ok], ref >= np.float64(np.float32(m["threshold"])))
    assert target[ok].any() and not target[ok].all()
    assert np.allclose(weight[ok], probability(m, ref), rtol=1e-14, atol=0)
    assert not target[~ok].any() and not weight[~ok].any()                 # no window: 0 / 0
    t2, w2 = capi.hist_svm_evaluate_samples(ctx, p, prm, svm, s)
    assert np.array_equal(t2, target) and np.array_equal(w2, weight)


def test_svm_evaluate_samples_argument_rules(capi, ctx, synth, image):
    """argument checks only: each is FD_ERR_INVALID_ARGUMENT with a message, before anything is launched"""
    p = layer_pyramid(capi, ctx, image, capi.FD_LAYER_GRADBIN, bins=9)
    hp = capi.hist_params(0, 16, 16, 1, 1, bins=9, cell=8, block=2)
    s, want, ok = samples_for(p, 16, 16)
    feats, _ = capi.hist_extract_samples(ctx, p, hp, s[ok])
    good = capi.Svm(ctx, synth.make_svm_f32(5, feats, nsv=8, kernel=0))
    capi.hist_svm_evaluate_samples(ctx, p, hp, good, s)

    def rejected(pyr, prm, svm, samples=s, match=None):
        with pytest.raises(capi.FdError) as e:
            capi.hist_svm_evaluate_samples(ctx, pyr, prm, svm, samples)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and str(e.value), e.value
        if match:
            assert match in str(e.value), e.value

    rejected(p, hp, capi.Svm(ctx, synth.make_svm_f32(5, feats[:, :-1], nsv=8, kernel=0)), match="length")      # wrong dimension
    u8 = np.random.default_rng(1).integers(0, 256, (16, feats.shape[1])).astype(np.uint8)
    rejected(p, hp, capi.Svm(ctx, synth.make_svm_u8(3, u8, nsv=8, calib=u8, positive_fraction=0.5)), match="f32")   # u8 vectors
    multi = capi.Pyramid(ctx, **PYR)
    multi.set_frames(2)
    multi.update_frames(images=[image, image])
    rejected(multi, hp, good, match="frames")
    gray = capi.Pyramid(ctx, **PYR)
    gray.update(image)
    rejected(gray, hp, good, match="bin images")
    fresh = capi.Pyramid(ctx, **PYR)
    fresh.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9)
    rejected(fresh, hp, good, match="not been updated")
    rejected(p, capi.hist_params(0, 16, 16, 1, 1, bins=8, cell=8, block=2), good, match="bins")
    lbp = layer_pyramid(capi, ctx, image, capi.FD_LAYER_LBP, lbp_type=2)
    rejected(lbp, hp, good, match="gradient bin image")                     # HOG on codes
    rejected(lbp, capi.ehog_patch_params(16, 16, bins=9, cell_w=4), good, match="FD_LAYER_GRADBIN")
    import ctypes as C
    lib = capi.lib()
    t, w = np.zeros(4, np.uint8), np.zeros(4, np.float64)
    for n in (-1, capi.FD_HIST_SAMPLES_MAX + 1):
        rc = lib.fd_hist_svm_evaluate_samples(ctx.h, p.h, capi.FD_SAMPLES_HIST, C.byref(hp), good.h, n, s.ctypes.data_as(C.c_void_p),
                                              t.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
        assert rc == capi.FD_ERR_INVALID_ARGUMENT and "sample count" in lib.fd_last_error(ctx.h).decode()
    rc = lib.fd_hist_svm_evaluate_samples(ctx.h, p.h, 7, C.byref(hp), good.h, 1, s.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                          w.ctypes.data_as(C.c_void_p))
    assert rc == capi.FD_ERR_INVALID_ARGUMENT and "kind" in lib.fd_last_error(ctx.h).decode()
