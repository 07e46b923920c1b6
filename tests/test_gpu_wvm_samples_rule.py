"""fd_wvm_svm_evaluate_samples resolves its samples by the shared sample -> window rule (fd_sample_window): the samples it scores are
exactly the ones fd_sample_windows gives a window, on every edge of the rule and for samples whose arithmetic does not fit an int."""
import numpy as np
import pytest

import pyramid_samples_model as model

pytestmark = pytest.mark.gpu

PW = PH = 20
PYR = dict(octave_layers=3, min_scale=0.5, max_scale=0.8)   # of the layers 1, 0.794, 0.63, 0.5, ... the kept ones are 0.794, 0.63, 0.5
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
EXTREMES = (I32_MIN, I32_MAX, I32_MAX - 1)


def make_models(synth, gray):
    rng = np.random.default_rng(96)
    calib = synth.random_patches(gray, PW, PH, 2000, rng)
    wvm = synth.make_wvm(21, n_per=5, n_levels=4, calib_patches=calib, min_survivors=48)
    eq = synth.histeq64_np(synth.random_patches(gray, PW, PH, 300, rng))
    svm = synth.make_svm_u8(22, eq, nsv=64, calib=eq[64:], positive_fraction=0.5)
    return wvm, svm


def smallest_probabilities(wvm, svm):
    """lower bounds of the two logistic outputs.  A WVM output is sum_p hk[k][p] * K_p - bias with 0 < K_p <= 1, an SVM distance
    sum_i coeff[i] * K_i - bias likewise, so |output| <= the largest absolute row sum + |bias|"""
    wvm_bound = np.abs(wvm["hk_weights"].astype(np.float64)).sum(1).max() + abs(wvm["bias"])
    svm_bound = np.abs(svm["coeff"].astype(np.float64)).sum() + abs(float(svm["bias"]))
    low = lambda m, bound: 1.0 / (1.0 + np.exp(abs(m["logistic_a"]) + abs(m["logistic_b"]) * bound))
    return low(wvm, wvm_bound), low(svm, svm_bound)


def width_for(layers, inc, index):
    """a sample width that the rule maps to the pyramid layer `index`"""
    w = int(round(PW / inc ** index))
    assert model.lround(np.log(PW / w) / np.log(inc)) == index
    return w


def make_samples(layers, inc):
    """(samples, number of leading samples that are not extreme)"""
    first, last = layers[0], layers[-1]
    assert last["scale"] == 0.5 and (first["w"], first["h"]) == (76, 57) and (last["w"], last["h"]) == (48, 36)
    s = []
    # the layer choice: one before the first kept layer, the first, the last, one behind the last
    for index in (first["index"] - 1, first["index"], last["index"], last["index"] + 1):
        w = width_for(layers, inc, index)
        s.append((48, 36, w, w))
    # the first layer's borders: bx, by of -1, 0, lw - pw, lw - pw + 1
    W, H = first["w"] - PW, first["h"] - PH
    for bx, by in ((-1, H // 2), (0, 0), (W, H), (W + 1, H // 2), (W // 2, -1), (0, H), (W, 0), (W // 2, H + 1)):
        v = model.window_sample(first, PW, bx, by)
        assert v is not None
        s.append(v)
    # the last layer has scale 0.5 and width 40: (x - 20) * 0.5 is half-way for every odd x - 20, and cvRound takes it to the even
    # neighbour.  x - 20 = -3, -2, -1, 0 -> -1.5 (-2), -1, -0.5 (0: a window), 0; 56 .. 59 -> 28 = lw - pw, 28.5 (28: a window), 29, 29.5 (30)
    w = width_for(layers, inc, last["index"])
    assert w == 40 and last["w"] - PW == 28 and last["h"] - PH == 16
    for d in (-3, -2, -1, 0, 56, 57, 58, 59):
        s.append((20 + d, 20 + 16, w, w))
    for d in (-3, -2, -1, 0, 32, 33, 34, 35):   # y: 16 = lh - ph, 16.5 (16: a window), 17, 17.5 (18)
        s.append((20 + 28, 20 + d, w, w))
    for L in layers:   # one window inside every kept layer
        v = model.window_sample(L, PW, (L["w"] - PW) // 2, (L["h"] - PH) // 3)
        assert v is not None
        s.append(v)
    s.append((48, 36, 0, 10))
    s.append((48, 36, -5, -5))
    regular = len(s)
    # positions no int arithmetic holds, with widths that select no layer (1, 2, INT32_MAX) and widths that select one (25, 40)
    for v in EXTREMES:
        for w in (1, 2, I32_MAX, 25, 40):
            s += [(v, v, w, w), (v, 36, w, w), (48, v, w, w)]
    return np.array(s, np.int32), regular


def test_wvm_svm_samples_follow_the_shared_rule(oracle, capi, ctx, synth):
    frame = synth.make_frame(96, 72, seed=33)
    wvm, svm = make_models(synth, oracle.bgr2gray(frame))
    # no valid window's weight can underflow to 0: weight is 0.5 * p_wvm, or p_wvm * p_svm behind the SVM
    p_wvm, p_svm = smallest_probabilities(wvm, svm)
    assert p_wvm > 1e-100 and p_svm > 1e-100 and 0.5 * p_wvm > 0 and p_wvm * p_svm > 0
    pyr = capi.Pyramid(ctx, **PYR)
    pyr.update(frame)
    layers = pyr.layers()
    assert [L["index"] for L in layers] == [1, 2, 3]
    samples, regular = make_samples(layers, pyr.inc)
    assert 50 <= len(samples) <= 100
    want = capi.sample_windows(layers, pyr.inc, PW, PH, samples)
    valid = want[:, 3] == 1
    assert np.array_equal(want, model.sample_windows(layers, pyr.inc, PW, PH, samples))
    assert np.array_equal(want, pyr.sample_windows(PW, PH, samples))
    # the categories are all there: both verdicts of the layer choice, of every border, of the half-way cases
    assert valid[:4].tolist() == [False, True, True, False]
    assert valid[4:12].tolist() == [False, True, True, False, False, True, True, False]
    assert valid[12:20].tolist() == [False, False, True, True, True, True, False, False]
    assert valid[20:28].tolist() == [False, False, True, True, True, True, False, False]
    assert want[14].tolist() == [2, 0, 8, 1] and want[17].tolist() == [2, 28, 8, 1] and want[25].tolist() == [2, 14, 16, 1]
    assert valid[28:31].all() and not valid[31:].any() and regular == 33
    wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)
    target, weight = capi.wvm_svm_evaluate(ctx, pyr, wg, sg, samples)
    print("valid %d of %d, targets %d, weights %s" % (valid.sum(), len(samples), target.sum(), weight[valid].tolist()))
    assert np.array_equal(weight != 0, valid)
    assert not target[~valid].any()
    assert not target[regular:].any() and np.all(weight[regular:] == 0.0)
    # a valid sample alone gives what it gives in the set.  The set re-scores only its 8 most probable WVM positives with the SVM and
    # a sample alone is always re-scored, so the set must not hold more than 8: a sample the WVM rejects has weight 0.5 * p_wvm of
    # its window's WVM output, a positive has p_wvm * p_svm
    layer_images = [pyr.layer(i) for i in range(len(layers))]
    crops = np.stack([layer_images[l][by:by + PH, bx:bx + PW] for l, bx, by, _ in want[valid].tolist()])
    _, fout = capi.wvm_eval(ctx, wg, synth.histeq64_np(crops))
    rejected = np.array([0.5 * oracle.Wvm(wvm).probability(f) for f in fout])
    alone = [capi.wvm_svm_evaluate(ctx, pyr, wg, sg, samples[i:i + 1]) for i in np.flatnonzero(valid)]
    positives = ~np.isclose([w1[0] for _, w1 in alone], rejected, rtol=1e-9, atol=0)
    assert positives.sum() <= 8, positives.sum()
    for i, (t1, w1) in zip(np.flatnonzero(valid), alone):
        assert t1[0] == target[i] and w1[0] == weight[i], (i, samples[i].tolist())
    for i in np.flatnonzero(~valid)[::5]:   # and so does a sample without a window
        t1, w1 = capi.wvm_svm_evaluate(ctx, pyr, wg, sg, samples[i:i + 1])
        assert not t1[0] and w1[0] == 0.0
    wg.close(); sg.close(); pyr.close()
