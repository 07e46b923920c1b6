"""Gray-patch features and the RVM cascade on sampled windows of a gray pyramid (csrc/patch_samples.hpp): fd_patch_extract_samples bit
for bit against the per-patch entry points and the strided whi scan, fd_patch_rvm_evaluate_samples on both of its routes (the fused
k_rvm_samples, FD_PATCH_FUSED=1, and the composed one, FD_PATCH_FUSED=0) against tests/rvm_score_model.py and against each other,
fd_patch_svm_evaluate_samples against fd_svm_distance_batch, the small and the wrapping sample counts, and every argument rule.

Image, pyramid and the sample categories are those of tests/test_gpu_pyramid_samples.py.  A 32 x 32 patch does not fit the smallest of the
six layers (38 x 30), so for that patch "every layer is named" reads "every layer that can hold the patch".  The RVM cases need a row that
leaves at each of up to 129 levels, more rows than make_samples gives: they add a grid of windows of every layer (more_samples, built with
the same pyramid_samples_model.window_sample) behind make_samples' list."""
import ctypes as C

import numpy as np
import pytest

import pyramid_samples_model as model
import rvm_score_model as M

pytestmark = pytest.mark.gpu

PYR = dict(octave_layers=3, min_scale=0.3, max_scale=1.0)
PATCHES = ((20, 20), (12, 20), (5, 5), (32, 32))
CONVS = ((1.0 / 255.0, 0.0), (1.0 / 127.5, -1.0))
NUM_USED = (1, 2, 63, 64, 65, 128, 129)
FILTERS = 129
# kernel -> (feature space, patch, conversion): each u8 space and each patch shape meets the cascade once
RVM_SPACES = {"rbf": ("HQ64", (20, 20), (1.0 / 255.0, 0.0)), "hik": ("HISTEQ", (12, 20), (1.0 / 255.0, 0.0)),
              "linear": ("GRAY", (5, 5), (1.0 / 127.5, -1.0)), "poly": ("GRAY", (32, 32), (1.0, 0.0))}


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
def pyr(capi, ctx, image):
    p = capi.Pyramid(ctx, **PYR)
    p.update(image)
    yield p
    p.close()


@pytest.fixture(scope="module")
def layer_images(pyr):
    limg = [pyr.layer(i) for i in range(len(pyr.layers()))]
    assert len(limg) == 6 and all(l.ndim == 2 for l in limg)
    return limg


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def samples_for(p, pw, ph):
    layers = p.layers()
    s = model.make_samples(layers, p.inc, pw, ph)
    want = model.sample_windows(layers, p.inc, pw, ph, s)
    ok = want[:, 3] == 1
    fits = {i for i, l in enumerate(layers) if l["w"] >= pw and l["h"] >= ph}
    assert 2 * ok.sum() >= len(s) and (~ok).sum() >= 8 and set(want[ok, 0].tolist()) == fits and len(fits) >= 5
    return s, want, ok


def more_samples(p, pw, ph, per_side=8):
    """make_samples' list and, behind it, a per_side x per_side grid of windows in every layer that holds the patch"""
    layers = p.layers()
    s = model.make_samples(layers, p.inc, pw, ph).tolist()
    for L in layers:
        W, H = L["w"] - pw, L["h"] - ph
        if W < 0 or H < 0:
            continue
        for by in np.linspace(0, H, per_side).astype(int):
            for bx in np.linspace(0, W, per_side).astype(int):
                v = model.window_sample(L, pw, int(bx), int(by))
                if v is not None:
                    s.append(v)
    s = np.array(s, np.int32)
    want = model.sample_windows(layers, p.inc, pw, ph, s)
    return s, want, want[:, 3] == 1


def crop(layer_images, windows, pw, ph):
    return np.stack([layer_images[l][by:by + ph, bx:bx + pw] for l, bx, by, _ in windows.tolist()])


def space_of(capi, name):
    return getattr(capi, "FD_FEATURE_" + name)


# ---- features
@pytest.mark.parametrize("patch", PATCHES, ids=lambda s: "%dx%d" % s)
def test_features_equal_the_per_patch_entry_points(capi, ctx, pyr, layer_images, patch):
    pw, ph = patch
    s, want, ok = samples_for(pyr, pw, ph)
    assert np.array_equal(pyr.sample_windows(pw, ph, s), want)
    patches = crop(layer_images, want[ok], pw, ph)
    u8 = {"GRAY": patches, "HQ64": ctx.histeq64(patches), "HISTEQ": capi.equalize_hist_batch(ctx, patches)}
    assert not np.array_equal(u8["HQ64"], patches) and not np.array_equal(u8["HISTEQ"], u8["HQ64"])
    for name, src in u8.items():
        for scale, shift in CONVS:
            pp = capi.patch_samples_params(pw, ph, space_of(capi, name), scale, shift)
            feats, valid = capi.patch_extract_samples(ctx, pyr, pp, s)
            assert feats.shape == (len(s), pw * ph) and np.array_equal(valid, ok)
            assert not feats[~ok].any() and feats[ok].any()
            ref = src.reshape(len(src), -1).astype(np.float32) * np.float32(scale) + np.float32(shift)
            assert ref.dtype == np.float32 and feats[ok].tobytes() == ref.tobytes(), (name, pw, ph, scale, shift)
    # the whi chain ignores scale and shift
    ref = capi.whi_batch(ctx, patches).reshape(len(patches), -1)
    for scale, shift in CONVS:
        pp = capi.patch_samples_params(pw, ph, capi.FD_FEATURE_WHI, scale, shift)
        feats, valid = capi.patch_extract_samples(ctx, pyr, pp, s)
        assert np.array_equal(valid, ok) and not feats[~ok].any()
        assert feats[ok].tobytes() == ref.tobytes(), (pw, ph)
    # where the strided scan has the window: its row (the scan stops one short of the right and the bottom border)
    allw = pyr.windows(pw, ph, 1, 1)
    row_of = {(int(r[0]), int(r[1]), int(r[2])): i for i, r in enumerate(allw)}
    keys = [(l, bx, by) for l, bx, by, _ in want[ok].tolist()]
    scanned = np.array([k in row_of for k in keys])
    assert scanned.any() and not scanned.all()
    rows = np.array([row_of[k] for k, there in zip(keys, scanned) if there])
    scan = capi.extract_whi(ctx, pyr, capi.whi_params(pw, ph, 1, 1))
    assert len(scan) == len(allw) and feats[ok][scanned].tobytes() == scan[rows].tobytes()
    other = capi.patch_extract_samples(ctx, pyr, capi.patch_samples_params(pw, ph, capi.FD_FEATURE_WHI, whi_alpha=0.5, whi_cutoff=0.25), s)[0]
    assert other[ok].tobytes() == capi.whi_batch(ctx, patches, alpha=0.5, cutoff=0.25).tobytes() != ref.tobytes()


# ---- the RVM cascade
_RVM_CASES = {}   # (kernel, feature space) -> samples, rows, base model and the model's tables: built once, left unchanged


def rvm_case(capi, ctx, pyr, kname, space=None):
    sp, (pw, ph), conv = RVM_SPACES[kname]
    sp = space or sp
    c = _RVM_CASES.setdefault((kname, sp), {})
    if not c:
        s, want, ok = more_samples(pyr, pw, ph)
        assert ok.sum() >= 2 * FILTERS and (~ok).sum() >= 8
        pp = capi.patch_samples_params(pw, ph, space_of(capi, sp), *conv)
        feats, valid = capi.patch_extract_samples(ctx, pyr, pp, s)
        assert np.array_equal(valid, ok)
        rows = np.ascontiguousarray(feats[ok])
        base = M.make_model("patch-samples-%s-%s" % (kname, sp), M.KERNELS[kname], rows, pw, ph, FILTERS)
        K = M.kernel_values(base, rows)
        c.update(s=s, ok=ok, rows=rows, base=base, pp=pp, D=M.distances(base, K), B=M.bounds(base, K))
    return c


def check_rvm(capi, ctx, pyr, monkeypatch, c, m, what, routes=("1", "0", None)):
    """every route of the device against the model and against each other"""
    r = M.run(m, c["D"], c["B"])
    assert r.sure.all(), what          # no row's level may depend on the last bits of an exp: every row is compared
    h = capi.Rvm(ctx, m)
    try:
        lv_rows, d_rows = h.eval(c["rows"])
        ok = c["ok"]
        for route in routes:
            if route is None:
                monkeypatch.delenv("FD_PATCH_FUSED", raising=False)
            else:
                monkeypatch.setenv("FD_PATCH_FUSED", route)
            valid, level, dist, target = capi.patch_rvm_evaluate_samples(ctx, pyr, c["pp"], h, c["s"])
            w = "%s route %s" % (what, route)
            assert np.array_equal(valid, ok), w
            assert np.all(level[~ok] == -1) and not dist[~ok].any() and not target[~ok].any(), w
            assert np.array_equal(level[ok], r.level), (w, np.nonzero(level[ok] != r.level)[0][:5])
            assert np.array_equal(target[ok], r.positive), w
            if m["kernel"] == M.RBF:
                err = np.abs(dist[ok] - r.dist)
                i = int(np.argmax(err / r.bound))
                print("%s: max err / bound = %.3g (level %d)" % (w, err[i] / r.bound[i], r.level[i]))
                assert np.all(err <= r.bound), (w, i, err[i], r.bound[i])
            else:
                assert dist[ok].tobytes() == r.dist.tobytes(), w
            # the routes and Rvm.eval on the extracted rows: identical levels, identical distance bits
            assert np.array_equal(level[ok], lv_rows) and dist[ok].tobytes() == d_rows.tobytes(), w
    finally:
        monkeypatch.delenv("FD_PATCH_FUSED", raising=False)
        h.close()
    return r


@pytest.mark.parametrize("nu", NUM_USED)
@pytest.mark.parametrize("kname", sorted(RVM_SPACES))
def test_rvm_levels(capi, ctx, pyr, monkeypatch, kname, nu):
    """one lane, two, a block less one, a full block, the hand-over to the second block, that block's last lane less one and one lane of
    a third; a row leaves at every level"""
    c = rvm_case(capi, ctx, pyr, kname)
    m = dict(c["base"], num_used=nu)
    m["thresholds"] = M.calibrate(m, c["rows"], 0.995, D=c["D"])
    r = check_rvm(capi, ctx, pyr, monkeypatch, c, m, "%s num_used=%d" % (kname, nu))
    assert set(r.level.tolist()) == set(range(nu)), "a row leaves at every level"
    assert r.positive.any() and not r.positive.all()


@pytest.mark.parametrize("value,level", [(np.inf, 0), (-1e30, FILTERS - 1)], ids=["+inf", "-1e30"])
@pytest.mark.parametrize("kname", sorted(RVM_SPACES))
def test_rvm_constant_thresholds(capi, ctx, pyr, monkeypatch, kname, value, level):
    c = rvm_case(capi, ctx, pyr, kname)
    m = dict(c["base"], num_used=0, thresholds=np.full(FILTERS, value, np.float32))
    r = check_rvm(capi, ctx, pyr, monkeypatch, c, m, "%s thresholds %g" % (kname, value))
    assert np.all(r.level == level) and r.positive.all() == (level > 0) and r.positive.any() == (level > 0)


def test_rvm_on_the_whi_chain(capi, ctx, pyr, monkeypatch):
    """FD_FEATURE_WHI takes the composed route whatever the knob says"""
    c = rvm_case(capi, ctx, pyr, "rbf", "WHI")
    m = dict(c["base"], num_used=65)
    m["thresholds"] = M.calibrate(m, c["rows"], 0.99, D=c["D"])
    r = check_rvm(capi, ctx, pyr, monkeypatch, c, m, "rbf whi num_used=65")
    assert set(r.level.tolist()) == set(range(65))


# ---- the SVM call
def probability(m, d):
    """ProbabilisticSvmClassifier.cpp:54-58"""
    f = m["logistic_a"] + m["logistic_b"] * d
    with np.errstate(over="ignore"):   # the branch that is not taken may overflow
        return np.where(f >= 0, np.exp(-f) / (1.0 + np.exp(-f)), 1.0 / (1.0 + np.exp(f)))


@pytest.mark.parametrize("kernel", [2, 0], ids=["rbf", "linear"])
@pytest.mark.parametrize("space", ["GRAY", "WHI"])
def test_svm_evaluate_samples(capi, ctx, synth, pyr, kernel, space):
    pp = capi.patch_samples_params(20, 20, space_of(capi, space), 1.0 / 255.0, 0.0)
    s, want, ok = samples_for(pyr, 20, 20)
    feats, valid = capi.patch_extract_samples(ctx, pyr, pp, s)
    m = synth.make_svm_f32(5, feats[ok], nsv=40, gamma=0.5, positive_fraction=0.4, kernel=kernel)
    m["logistic_a"], m["logistic_b"] = 0.3, -1.7
    svm = capi.Svm(ctx, m)
    target, weight, dist = capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s, want_distance=True)
    ref = svm.distance(feats[ok])
    assert dist[ok].tobytes() == ref.tobytes() and not dist[~ok].any()      # the same kernel on the same vectors: the same bits
    assert np.array_equal(target[ok], ref >= np.float64(np.float32(m["threshold"])))
    assert target[ok].any() and not target[ok].all()
    assert np.allclose(weight[ok], probability(m, ref), rtol=1e-14, atol=0)
    assert not target[~ok].any() and not weight[~ok].any()                  # no window: 0 / 0
    t2, w2 = capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s)
    assert np.array_equal(t2, target) and np.array_equal(w2, weight)
    svm.close()


# ---- counts
def test_counts(capi, ctx, synth, pyr, monkeypatch, num_cus):
    """n = 0, 1, 5 (a partial workgroup of k_rvm_samples), a list without one window, and one sample more than the fused kernel's grid
    (num_cus * 8 workgroups of four windows) covers in one trip"""
    pp = capi.patch_samples_params(20, 20, capi.FD_FEATURE_HQ64, 1.0 / 255.0, 0.0)
    s, want, ok = samples_for(pyr, 20, 20)
    base, _ = capi.patch_extract_samples(ctx, pyr, pp, s[ok])
    m = dict(M.make_model("patch-samples-counts", M.RBF, base, 20, 20, 24), num_used=0)
    m["thresholds"] = M.calibrate(m, base, 0.97)
    r = M.evaluate(m, base)
    assert r.sure.all() and len(set(r.level.tolist())) >= 20
    rvm = capi.Rvm(ctx, m)
    svm = capi.Svm(ctx, synth.make_svm_f32(5, base, nsv=8, kernel=0))
    empty = np.zeros((0, 4), np.int32)
    for route in ("1", "0", None):
        if route is None:
            monkeypatch.delenv("FD_PATCH_FUSED", raising=False)
        else:
            monkeypatch.setenv("FD_PATCH_FUSED", route)
        v, lv0, d0, t0 = capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s[ok])
        assert v.all() and np.array_equal(lv0, r.level) and np.array_equal(t0, r.positive)
        for n in (1, 5):
            v, lv, d, t = capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s[ok][3:3 + n])
            assert v.all() and np.array_equal(lv, lv0[3:3 + n]) and d.tobytes() == d0[3:3 + n].tobytes() and np.array_equal(t, t0[3:3 + n])
        v, lv, d, t = capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, empty)
        assert len(v) == len(lv) == len(d) == len(t) == 0
        v, lv, d, t = capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s[~ok])
        assert not v.any() and np.all(lv == -1) and not d.any() and not t.any()
        n = num_cus * 32 + 1
        rep = np.resize(np.arange(ok.sum()), n)
        v, lv, d, t = capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s[ok][rep])
        assert len(lv) == n and v.all() and np.array_equal(lv, lv0[rep]) and d.tobytes() == d0[rep].tobytes() and np.array_equal(t, t0[rep])
    monkeypatch.delenv("FD_PATCH_FUSED", raising=False)
    feats, valid = capi.patch_extract_samples(ctx, pyr, pp, s[ok][rep])
    assert valid.all() and feats.tobytes() == base[rep].tobytes()
    for n in (1, 5):
        one, v1 = capi.patch_extract_samples(ctx, pyr, pp, s[ok][3:3 + n])
        assert v1.all() and one.tobytes() == base[3:3 + n].tobytes()
    none, v0 = capi.patch_extract_samples(ctx, pyr, pp, empty)
    assert none.shape == (0, 400) and len(v0) == 0
    lost, vl = capi.patch_extract_samples(ctx, pyr, pp, s[~ok])
    assert len(lost) == (~ok).sum() and not vl.any() and not lost.any()
    t, w = capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s[~ok])
    assert not t.any() and not w.any()
    t, w = capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, empty)
    assert len(t) == 0 and len(w) == 0
    t0, w0, d0 = capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s[ok], want_distance=True)
    t, w, d = capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s[ok][rep], want_distance=True)
    assert d.tobytes() == d0[rep].tobytes() and np.array_equal(t, t0[rep])
    rvm.close()
    svm.close()


# ---- argument rules
def test_argument_rules(capi, ctx, synth, image, pyr):
    """each is FD_ERR_INVALID_ARGUMENT with a message, before anything is queued; pyramid and models stay usable"""
    pp = capi.patch_samples_params(20, 20, capi.FD_FEATURE_HQ64, 1.0 / 255.0, 0.0)
    s, want, ok = samples_for(pyr, 20, 20)
    feats, _ = capi.patch_extract_samples(ctx, pyr, pp, s)
    base = feats[ok]
    m = dict(M.make_model("patch-samples-rules", M.RBF, base, 20, 20, 8), num_used=0)
    m["thresholds"] = M.calibrate(m, base, 0.9)
    rvm = capi.Rvm(ctx, m)
    svm = capi.Svm(ctx, synth.make_svm_f32(5, base, nsv=8, kernel=0))
    before = (capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s), capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s, want_distance=True))

    def rejected(match, p=pyr, prm=pp, r=rvm, v=svm, calls="esr", c=ctx):
        for call in calls:
            with pytest.raises(capi.FdError) as e:
                if call == "e":
                    capi.patch_extract_samples(c, p, prm, s)
                elif call == "s":
                    capi.patch_svm_evaluate_samples(c, p, prm, v, s)
                else:
                    capi.patch_rvm_evaluate_samples(c, p, prm, r, s)
            assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and match in str(e.value), (call, e.value)

    other = capi.Context(0)
    foreign = capi.Pyramid(other, **PYR)
    foreign.update(image)
    rejected("different contexts", p=foreign)
    rejected("different contexts", r=capi.Rvm(other, m), calls="r")
    multi = capi.Pyramid(ctx, **PYR)
    multi.set_frames(2)
    multi.update_frames(images=[image, image])
    rejected("frames", p=multi)
    rejected("not been updated", p=capi.Pyramid(ctx, **PYR))
    filtered = capi.Pyramid(ctx, **PYR)
    filtered.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9)
    filtered.update(image)
    rejected("gray pyramid", p=filtered)
    for side in (0, 33):
        rejected("patch size", prm=capi.patch_samples_params(side, 20, capi.FD_FEATURE_HQ64))
        rejected("patch size", prm=capi.patch_samples_params(20, side, capi.FD_FEATURE_GRAY))
    for space in (4, -1):
        rejected("feature space", prm=capi.patch_samples_params(20, 20, space))
    rejected("filter size", prm=capi.patch_samples_params(12, 20, capi.FD_FEATURE_HQ64), calls="r")
    rejected("filter size", prm=capi.patch_samples_params(20, 12, capi.FD_FEATURE_WHI), calls="r")
    rejected("length", prm=capi.patch_samples_params(12, 20, capi.FD_FEATURE_HQ64), calls="s")
    u8 = np.random.default_rng(1).integers(0, 256, (16, 400)).astype(np.uint8)
    rejected("f32", v=capi.Svm(ctx, synth.make_svm_u8(3, u8, nsv=8, calib=u8, positive_fraction=0.5)), calls="s")
    lib = capi.lib()
    buf = np.zeros(64, np.float64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for n in (-1, capi.FD_HIST_SAMPLES_MAX + 1):
        assert lib.fd_patch_extract_samples(ctx.h, pyr.h, C.byref(pp), n, ptr(s), None, None) == capi.FD_ERR_INVALID_ARGUMENT
        assert "sample count" in lib.fd_last_error(ctx.h).decode()
        assert lib.fd_patch_svm_evaluate_samples(ctx.h, pyr.h, C.byref(pp), svm.h, n, ptr(s), ptr(buf), ptr(buf), None) == capi.FD_ERR_INVALID_ARGUMENT
        assert "sample count" in lib.fd_last_error(ctx.h).decode()
        assert lib.fd_patch_rvm_evaluate_samples(ctx.h, pyr.h, C.byref(pp), rvm.h, n, ptr(s), None, None, None, None) == capi.FD_ERR_INVALID_ARGUMENT
        assert "sample count" in lib.fd_last_error(ctx.h).decode()
    # fd_detect_rvm keeps refusing the whi space
    with pytest.raises(capi.FdError) as e:
        capi.detect_rvm(ctx, pyr, rvm, feature_space=capi.FD_FEATURE_WHI)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "feature space" in str(e.value)
    after = (capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s), capi.patch_svm_evaluate_samples(ctx, pyr, pp, svm, s, want_distance=True))
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert a.tobytes() == b.tobytes()
    assert capi.patch_extract_samples(ctx, pyr, pp, s)[0].tobytes() == feats.tobytes()
    foreign.close()
    other.close()
