"""fd_ehog_tracker (feature pyramid, heat pyramid, samples, patches, heat peak, local maxima) against tests/ehog_model.py, bit for bit.
96 x 80 frame, cell 4, windows of 3 x 4 and 4 x 3 cells (the second has an even kernel width: the anchor rule), two layers per octave."""
import numpy as np
import pytest

import ehog_model as model

pytestmark = pytest.mark.gpu

W, H, CELL, OLC, MAXW = 96, 80, 4, 2, 60
BINS, SIGNED, UNSIGNED, ALPHA = 18, True, True, 0.2
INTERP_BINS, INTERP_CELLS = False, True
BIAS = 0.3
GEOMS = {"3x4": (3, 4), "4x3": (4, 3)}   # (cell_cols, cell_rows)


def _fp(capi):
    return capi.cehog_params(cell_size=CELL, bin_count=BINS, signed_gradients=SIGNED, unsigned_gradients=UNSIGNED, interpolate_bins=INTERP_BINS,
                             interpolate_cells=INTERP_CELLS, alpha=ALPHA)


def _prm(capi, cols, rows):
    return capi.ehog_tracker_params(_fp(capi), cols, rows, OLC, cols * CELL, MAXW)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r != %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


class Scene:
    """one tracker per window geometry, updated with the frame, and the model's view of the same frame -- built once"""

    def __init__(self, capi, ctx, synth, cols, rows):
        self.cols, self.rows = cols, rows
        self.frame = synth.make_frame(W, H, seed=31)
        self.prm = _prm(capi, cols, rows)
        self.tracker = capi.EhogTracker(ctx, self.prm)
        self.tracker.update(self.frame)
        D = self.tracker.channels
        self.weights = (np.random.default_rng(cols * 10 + rows).standard_normal((rows, cols, D)) * 0.5).astype(np.float32)
        self.tracker.set_svm(self.weights, BIAS)
        self.layers = model.plan_layers(W, H, cols, CELL, cols * CELL, MAXW, OLC)
        mn, mx = model.pyramid_limits(cols, CELL, cols * CELL, MAXW, OLC)
        pyr = capi.Pyramid(ctx, octave_layers=OLC, min_scale=mn, max_scale=mx)
        pyr.update(self.frame)
        self.gray = [pyr.layer(i) for i in range(len(pyr.layers()))]
        self.features = [model.cehog(g, CELL, BINS, SIGNED, UNSIGNED, INTERP_BINS, INTERP_CELLS, ALPHA) for g in self.gray]
        self.heats = [model.heat_layer(f, self.weights, BIAS) for f in self.features]

    def window(self, s):
        return model.sample_window(s[0], s[1], s[2], s[3], self.layers, self.cols, self.rows, CELL, OLC)

    def patch(self, s):
        return model.patch_window(s[0], s[1], s[2], s[3], self.layers, self.cols, self.rows, CELL, OLC)


@pytest.fixture(scope="module")
def scenes(capi, ctx, synth):
    return {k: Scene(capi, ctx, synth, *g) for k, g in GEOMS.items()}


@pytest.fixture(params=list(GEOMS))
def scene(request, scenes):
    return scenes[request.param]


def test_layers(scene):
    got = scene.tracker.layers()
    assert len(got) == len(scene.layers) >= 3
    for g, (index, w, h, rows, cols, scale) in zip(got, scene.layers):
        assert (g["index"], g["width"], g["height"], g["rows"], g["cols"], g["scale"]) == (index, w, h, rows, cols, scale)
    assert [g.shape for g in scene.gray] == [(l[2], l[1]) for l in scene.layers]


def test_feature_and_heat_layers(scene):
    for li in range(len(scene.layers)):
        _same(scene.tracker.feature_layer(li), scene.features[li], "feature layer %d" % li)
        _same(scene.tracker.heat_layer(li), scene.heats[li], "heat layer %d" % li)


def test_heat_rim_has_the_zero_border(scene):
    """the corner of a heat layer sees only the taps that fall into the layer"""
    f, k = scene.features[0], scene.weights
    ay, ax = scene.rows // 2, scene.cols // 2
    window = np.zeros_like(k)
    window[ay:, ax:] = f[:scene.rows - ay, :scene.cols - ax]
    assert scene.tracker.heat_layer(0)[0, 0] == model.ordered_dot(window, k, BIAS)


def _edge_samples(scene):
    """windows exactly fitting and one cell past each of the four edges of the first layer, odd sizes, widths with no layer on either side"""
    cols, rows = scene.cols, scene.rows
    w, h = cols * CELL, rows * CELL   # layer 0, scale 1
    out = []
    for (bx, by) in [(0, 0), (W // CELL - cols, H // CELL - rows), (-1, 0), (0, -1), (W // CELL - cols + 1, 0), (0, H // CELL - rows + 1)]:
        out.append((bx * CELL + w // 2, by * CELL + h // 2, w, h))
    out += [(40, 40, w + 1, h + 1), (41, 39, w + 3, h - 1), (37, 33, 2 * w + 1, 2 * h + 1), (50, 40, 2 * w - 1, 2 * h + 3)]
    out += [(40, 40, 2, 3), (40, 40, 1, 1), (40, 40, 400, 400), (40, 40, 0, 10), (40, 40, 10, 0), (40, 40, -5, 10)]
    return out


def _random_samples(n, seed, scene):
    rng = np.random.default_rng(seed)
    width = rng.integers(scene.cols * CELL // 2, 90, n)
    height = np.maximum(1, width * scene.rows // scene.cols + rng.integers(-2, 3, n))
    return np.stack([rng.integers(-5, W + 5, n), rng.integers(-5, H + 5, n), width, height], 1).astype(np.int32)


def _check_samples(scene, samples):
    samples = np.asarray(samples, np.int32).reshape(-1, 4)
    valid, score = scene.tracker.evaluate_samples(samples)
    valid2, cells = scene.tracker.extract_cells(samples)
    assert np.array_equal(valid, valid2) and len(valid) == len(samples)
    for i, s in enumerate(samples):
        win = scene.window(s)
        assert bool(valid[i]) == (win is not None), (i, s)
        if win is None:
            assert score[i] == 0 and not cells[i].any()
            continue
        li, bx, by = win
        assert score[i] == scene.heats[li][by + scene.rows // 2, bx + scene.cols // 2], (i, s)
        _same(cells[i], scene.features[li][by:by + scene.rows, bx:bx + scene.cols], "cells of sample %d" % i)
        assert score[i] == model.ordered_dot(cells[i], scene.weights, BIAS), (i, s)
    return valid


def test_edge_samples(scene):
    samples = _edge_samples(scene)
    valid = _check_samples(scene, samples)
    assert valid[:6].tolist() == [1, 1, 0, 0, 0, 0]
    assert not valid[-6:].any()


@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_seeded_samples(scene, n):
    valid = _check_samples(scene, _random_samples(n, 7 + n, scene))
    if n == 1000:
        assert 100 < int(valid.sum()) < 900


def _patch_samples(scene):
    """on layer 0 (a sample of cols * CELL x rows * CELL widens to exactly the patch): inside, up to one cell outside on each side
    (mirrored), just beyond (invalid)"""
    cols, rows = scene.cols, scene.rows
    w, h = cols * CELL, rows * CELL
    pw, ph = (cols + 2) * CELL, (rows + 2) * CELL
    out = []
    for (bx, by) in [(10, 9), (0, 0), (W - pw, H - ph), (-1, 5), (-CELL, 5), (5, -CELL), (W - pw + CELL, 3), (3, H - ph + CELL), (-CELL, -CELL),
                     (W - pw + CELL, H - ph + CELL), (-CELL - 1, 5), (5, -CELL - 1), (W - pw + CELL + 1, 3), (3, H - ph + CELL + 1)]:
        out.append((bx + pw // 2, by + ph // 2, w, h))
    return out


def test_extract_patches(capi, ctx, scene):
    rng = np.random.default_rng(3)
    samples = np.array(_patch_samples(scene) + _random_samples(50, 11, scene).tolist(), np.int32)
    valid, feat, score = scene.tracker.extract_patches(samples, want_score=True)
    valid2, feat2 = scene.tracker.extract_patches(samples)
    assert np.array_equal(valid, valid2) and feat.tobytes() == feat2.tobytes()
    pw, ph = (scene.cols + 2) * CELL, (scene.rows + 2) * CELL
    assert valid[:14].tolist() == [1] * 10 + [0] * 4
    seen_outside = 0
    for i, s in enumerate(samples):
        win = scene.patch(s)
        assert bool(valid[i]) == (win is not None), (i, s)
        if win is None:
            assert score[i] == 0 and not feat[i].any()
            continue
        li, bx, by = win
        g = scene.gray[li]
        seen_outside += bx < 0 or by < 0 or bx + pw > g.shape[1] or by + ph > g.shape[0]
        patch = model.mirrored_patch(g, bx, by, pw, ph)
        want = capi.cehog_image(ctx, _fp(capi), gray=patch)[1:-1, 1:-1]
        _same(feat[i], want, "patch features of sample %d" % i)
        dot = 0.0
        for a, b in zip(feat[i].ravel().tolist(), scene.weights.ravel().tolist()):
            dot = dot + a * b
        assert score[i] == -float(np.float32(BIAS)) + dot, (i, s)
    assert seen_outside >= 7
    # the dense filter on one mirrored patch equals the model, so the chain above ends at the model
    li, bx, by = scene.patch(samples[4])
    patch = model.mirrored_patch(scene.gray[li], bx, by, pw, ph)
    _same(feat[4], model.cehog(patch, CELL, BINS, SIGNED, UNSIGNED, INTERP_BINS, INTERP_CELLS, ALPHA)[1:-1, 1:-1], "sample 4 against the model")


def test_patch_lds_limit(capi, ctx):
    """the largest geometry a workgroup's LDS (64 KB) holds is stated by fd_ehog_tracker_patch_lds_bytes; beyond it the call is refused"""
    small = _prm(capi, 3, 4)
    assert 0 < capi.ehog_tracker_patch_lds_bytes(small) < 8192
    big = capi.ehog_tracker_params(_fp(capi), 30, 30, OLC, 30 * CELL, 200)
    assert capi.ehog_tracker_patch_lds_bytes(big) > 65536
    t = capi.EhogTracker(ctx, big)
    t.update(np.zeros((300, 300), np.uint8))
    with pytest.raises(capi.FdError) as e:
        t.extract_patches([(150, 150, 120, 120)])
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    t.close()


def test_peak_on_noise(scene):
    found, box = scene.tracker.heat_peak()
    mfound, mscore, mbounds = model.heat_peak(scene.heats, scene.layers, scene.cols, scene.rows, CELL)
    assert found and mfound
    assert box["score"] == mscore and (box["x"], box["y"], box["w"], box["h"]) == mbounds


def test_maxima_on_noise(capi, scene):
    for thr in (-1e30, 0.0, 0.5):
        got = scene.tracker.heat_maxima(thr)
        want = model.heat_maxima(scene.heats, scene.layers, scene.cols, scene.rows, CELL, thr)
        assert [(g["score"], g["x"], g["y"], g["w"], g["h"]) for g in got] == want
    assert len(scene.tracker.heat_maxima(-1e30)) >= 3
    total = len(scene.tracker.heat_maxima(-1e30))
    with pytest.raises(capi.FdError) as e:
        scene.tracker.heat_maxima(-1e30, cap=total - 1)
    assert e.value.code == capi.FD_ERR_CAPACITY and e.value.count == total


@pytest.mark.parametrize("geom", list(GEOMS))
def test_flat_frame_peak_and_plateau(capi, ctx, geom):
    """a flat frame has no gradients: every feature is 0, every heat value is delta.  The first offered position of the first layer
    wins the peak (strict >), every offered position is a local maximum (>=), and the threshold test is strict"""
    cols, rows = GEOMS[geom]
    t = capi.EhogTracker(ctx, _prm(capi, cols, rows))
    t.update(np.full((H, W, 3), 90, np.uint8))
    D = t.channels
    t.set_svm(np.ones((rows, cols, D), np.float32), -1.25)
    layers = model.plan_layers(W, H, cols, CELL, cols * CELL, MAXW, OLC)
    heats = [np.full((l[3], l[4]), np.float32(1.25), np.float32) for l in layers]
    for li in range(len(layers)):
        _same(t.heat_layer(li), heats[li], "flat heat layer %d" % li)
    found, box = t.heat_peak()
    assert found and box["score"] == np.float32(1.25)
    assert (box["x"], box["y"], box["w"], box["h"]) == (0, 0, cols * CELL, rows * CELL)
    want = model.heat_maxima(heats, layers, cols, rows, CELL, 1.0)
    offered = sum(len(r) * len(c) for r, c in (model.offered_positions(l[3], l[4], rows, cols) for l in layers))
    assert len(want) == offered > 50
    got = t.heat_maxima(1.0)
    assert [(g["score"], g["x"], g["y"], g["w"], g["h"]) for g in got] == want
    assert len(t.heat_maxima(1.25)) == 0                                   # score > threshold is strict
    assert len(t.heat_maxima(float(np.nextafter(np.float32(1.25), np.float32(0))))) == offered
    t.close()


def test_calls_before_an_svm_is_set_are_errors(capi, ctx, synth):
    t = capi.EhogTracker(ctx, _prm(capi, 3, 4))
    for call in (lambda: t.evaluate_samples([(40, 40, 12, 16)]), lambda: t.extract_cells([(40, 40, 12, 16)]), lambda: t.feature_layer(0)):
        with pytest.raises(capi.FdError) as e:   # not updated yet
            call()
        assert e.value.code == capi.FD_ERR_RUNTIME
    assert len(t.layers()) == 0
    t.update(synth.make_frame(W, H, seed=2))
    assert t.extract_cells([(40, 40, 12, 16)])[0].tolist() == [1]
    for call in (lambda: t.evaluate_samples([(40, 40, 12, 16)]), t.heat_peak, lambda: t.heat_maxima(0.0), lambda: t.heat_layer(0),
                 lambda: t.extract_patches([(40, 40, 12, 16)], want_score=True)):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_RUNTIME
    assert t.extract_patches([(40, 40, 12, 16)])[0].tolist() == [1]   # features alone need no SVM
    t.close()


def test_invalid_parameters(capi, ctx):
    fp = _fp(capi)
    for prm in (capi.ehog_tracker_params(fp, 0, 4, 2, 12, 60), capi.ehog_tracker_params(fp, 3, 0, 2, 12, 60), capi.ehog_tracker_params(fp, 3, 4, 0, 12, 60),
                capi.ehog_tracker_params(fp, 3, 4, 2, 0, 60), capi.ehog_tracker_params(fp, 3, 4, 2, 30, 20),
                capi.ehog_tracker_params(capi.cehog_params(cell_size=4, bin_count=9), 3, 4, 2, 12, 60)):
        with pytest.raises(capi.FdError) as e:
            capi.EhogTracker(ctx, prm)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    t = capi.EhogTracker(ctx, capi.ehog_tracker_params(fp, 1, 4, 2, 4, 60))
    t.update(np.zeros((H, W), np.uint8))
    t.set_svm(np.zeros((4, 1, t.channels), np.float32), 0.0)
    with pytest.raises(capi.FdError) as e:
        t.heat_maxima(0.0)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    t.close()


def test_too_few_layers_is_a_runtime_error(capi, ctx):
    """min_width == max_width leaves one layer: the feature pyramid (an ImagePyramid built on another) needs two"""
    t = capi.EhogTracker(ctx, capi.ehog_tracker_params(_fp(capi), 3, 4, 2, 12, 12))
    with pytest.raises(capi.FdError) as e:
        t.update(np.zeros((H, W), np.uint8))
    assert e.value.code == capi.FD_ERR_RUNTIME
    t.close()


def test_second_update_with_another_size_rebuilds_the_layers(capi, ctx, synth):
    cols, rows = 3, 4
    t = capi.EhogTracker(ctx, _prm(capi, cols, rows))
    weights = (np.random.default_rng(1).standard_normal((rows, cols, t.channels)) * 0.5).astype(np.float32)
    t.set_svm(weights, BIAS)
    mn, mx = model.pyramid_limits(cols, CELL, cols * CELL, MAXW, OLC)
    for (w, h, seed) in [(W, H, 4), (77, 90, 5), (W, H, 6)]:
        frame = synth.make_frame(w, h, seed=seed)
        t.update(frame)
        layers = model.plan_layers(w, h, cols, CELL, cols * CELL, MAXW, OLC)
        got = t.layers()
        assert [(g["index"], g["width"], g["height"], g["rows"], g["cols"]) for g in got] == [l[:5] for l in layers]
        pyr = capi.Pyramid(ctx, octave_layers=OLC, min_scale=mn, max_scale=mx)
        pyr.update(frame)
        li = len(layers) - 1
        f = model.cehog(pyr.layer(li), CELL, BINS, SIGNED, UNSIGNED, INTERP_BINS, INTERP_CELLS, ALPHA)
        _same(t.feature_layer(li), f, "last feature layer at %d x %d" % (w, h))
        _same(t.heat_layer(li), model.heat_layer(f, weights, BIAS), "last heat layer at %d x %d" % (w, h))
    t.close()
