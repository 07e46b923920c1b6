"""condensation::WvmSvmModel on the resident particle set, the parts that need no device: tests/wvm_svm_resident_model.py against the
oracle's WvmSvmModel::evaluate on one 96 x 72 scene (targets equal, weights bit-equal: both sides use libm), the tie rule of the
selection, and the three new symbols."""
import os
import re

import numpy as np
import pytest

import wvm_svm_resident_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PW, PH = 96, 72, 20, 20
PYR = dict(octave_layers=3, min_scale=0.5, max_scale=0.8)   # tests/test_gpu_wvm_samples_rule.py: the kept layers are 0.794, 0.63, 0.5
NEW_SYMBOLS = ("fd_particles_evaluate_wvm_svm", "fd_particles_weigh_wvm_svm", "fd_particles_get_wvm_svm_trace")
FRAME_SEED, WVM_SEED, SVM_SEED, MIN_SURVIVORS = 33, 21, 22, 200
# (seed, count) of the sample sets: the first keeps at most 8 WVM positives, the second more than 8
SETS = {"few": (1, 40), "many": (2, 300)}


def make_scene(synth, oracle, min_survivors=MIN_SURVIVORS, n_levels=4):
    """(frame, wvm, svm): a seeded 96 x 72 frame and 20 x 20 models calibrated on its patches; n_levels * 5 filters"""
    frame = synth.make_frame(W, H, seed=FRAME_SEED)
    gray = oracle.bgr2gray(frame)
    rng = np.random.default_rng(96)
    calib = synth.random_patches(gray, PW, PH, 2000, rng)
    wvm = synth.make_wvm(WVM_SEED, n_per=5, n_levels=n_levels, calib_patches=calib, min_survivors=min_survivors)
    eq = synth.histeq64_np(synth.random_patches(gray, PW, PH, 300, rng))
    svm = synth.make_svm_u8(SVM_SEED, eq, nsv=64, calib=eq[64:], positive_fraction=0.5)
    return frame, wvm, svm


def make_particles(seed, n):
    """{x, y, size} int32 (n, 3): centres over the frame and a little outside, sizes around the widths the kept layers take (25 .. 40)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(8, W - 8, n), rng.integers(8, H - 8, n), rng.integers(22, 44, n)], 1).astype(np.int32)


def oracle_outputs(oracle, pyr, wvm, svm, samples):
    """per sample {x, y, width, height}: (valid, level, fout, the SVM distance of its equalised patch) from the oracle's own pieces"""
    ow, os_ = oracle.Wvm(wvm), oracle.Svm(svm)
    layers = [pyr.layer(i) for i in range(len(pyr.layers()))]
    n = len(samples)
    valid, level, fout, dist = np.zeros(n, bool), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64)
    for i, (x, y, w, h) in enumerate(np.asarray(samples).tolist()):
        win = oracle.extract_single(pyr, PW, PH, x, y, w, h)
        if win is None:
            continue
        eq = oracle.histeq64(layers[win[0]][win[2]:win[2] + PH, win[1]:win[1] + PW].copy())
        valid[i] = True
        level[i], fout[i] = ow.eval(eq)
        dist[i] = os_.distance(eq.reshape(1, -1))[0]
    return valid, level, fout, dist


def as_samples(particles):
    """Sample::aspectRatio 1: {x, y, size, size}"""
    return np.concatenate([particles, particles[:, 2:3]], 1).astype(np.int32)


@pytest.mark.parametrize("name", sorted(SETS))
def test_model_equals_the_oracle(oracle, synth, name):
    frame, wvm, svm = make_scene(synth, oracle)
    pyr = oracle.Pyramid(**PYR)
    pyr.update(frame)
    samples = as_samples(make_particles(*SETS[name]))
    valid, level, fout, dist = oracle_outputs(oracle, pyr, wvm, svm, samples)
    free, n_pos = model.tie_free(wvm, valid, level, fout)
    print("%s: %d samples, %d valid, %d WVM positives" % (name, len(samples), valid.sum(), n_pos))
    # the precondition, asserted: where the 8th and 9th most probable positives tie, the reference's choice is an accident of its sort
    assert free
    assert (1 <= n_pos <= model.RESCORED) if name == "few" else n_pos > model.RESCORED
    assert 0 < valid.sum() and (name == "few" or valid.sum() < len(samples))
    selected = model.select(wvm, valid, level, fout)
    assert len(selected) == min(n_pos, model.RESCORED)
    target, weight, score, best, n_valid = model.weigh(wvm, svm, valid, level, fout, selected, dist[selected])
    want_target, want_weight = oracle.wvm_svm_evaluate(pyr, oracle.Wvm(wvm), oracle.Svm(svm), samples)
    assert np.array_equal(target.astype(bool), want_target)
    assert weight.tobytes() == want_weight.tobytes()
    assert n_valid == int(valid.sum()) and best == max(0.0 if not valid.all() else model.LOWEST, float(fout[valid].max()))
    assert not weight[~valid].any() and not score[~valid].any() and np.array_equal(score[valid], fout[valid].astype(np.float64))
    pyr.close()


def all_positive(wvm):
    out = dict(wvm)
    out["thresholds"] = np.full(len(wvm["thresholds"]), -np.inf, np.float32)
    return out


def test_equal_keys_go_to_the_lower_index(oracle, synth):
    frame, wvm, svm = make_scene(synth, oracle)
    wvm = all_positive(wvm)
    pyr = oracle.Pyramid(**PYR)
    pyr.update(frame)
    samples = as_samples(np.tile(np.array([[48, 36, 30]], np.int32), (12, 1)))   # the same window 12 times
    valid, level, fout, dist = oracle_outputs(oracle, pyr, wvm, svm, samples)
    assert valid.all() and np.unique(fout).size == 1 and model.positives(wvm, level, fout).all()
    assert model.tie_free(wvm, valid, level, fout) == (False, 12)
    assert model.select(wvm, valid, level, fout) == list(range(8))
    target, weight, _, _, _ = model.weigh(wvm, svm, valid, level, fout, list(range(8)), dist[:8])
    assert np.unique(weight[:8]).size == 1 and np.unique(weight[8:]).size == 1 and not target[8:].any()
    assert weight[8] == 0.5 * model.p_wvm(model.key(wvm["logistic_a"], wvm["logistic_b"], fout[0]))
    pyr.close()


def test_selection_order():
    wvm = dict(num_filters=3, thresholds=np.array([0, 0, 1.0], np.float32), logistic_a=0.5, logistic_b=-2.0)
    last = 2
    #            0     1     2     3      4       5     6     7     8     9     10    11
    fout = np.array([3.0, 5.0, 5.0, 9.0, np.nan, 0.5, 4.0, 4.5, 2.0, 1.0, 6.0, 7.0], np.float32)
    level = np.full(12, last, np.int32)
    level[6] = 1                      # did not reach the last filter
    valid = np.ones(12, bool)
    valid[3] = False                  # the most probable positive belongs to an invalid particle: its spare window is never selected
    # 5 fails the last threshold; logistic_b < 0: the larger output is the more probable; 1 and 2 tie and keep their order;
    # a NaN output is no positive at all (NaN >= threshold is false)
    assert model.positives(wvm, level, fout).tolist() == [True, True, True, True, False, False, False, True, True, True, True, True]
    assert model.select(wvm, valid, level, fout) == [11, 10, 1, 2, 7, 0, 8, 9]
    valid[9] = False
    assert model.select(wvm, valid, level, fout) == [11, 10, 1, 2, 7, 0, 8]
    # a NaN key (a logistic parameter that is not a number) ranks behind every number, and then the index decides; -0 equals +0
    assert sorted([model.order(float("nan"), 0), model.order(1e300, 5), model.order(-0.0, 4), model.order(0.0, 3)]) == \
        [(0, 0.0, 3), (0, 0.0, 4), (0, 1e300, 5), (1, 0.0, 0)]
    assert model.key(0.5, -2.0, np.float32(0.1)) == 0.5 + -2.0 * float(np.float32(0.1))
    assert model.p_wvm(1e6) == 0.0 and model.p_wvm(-1e6) == 1.0 and model.p_svm(0.0, -1.0, 1e6) == 1.0 and model.p_svm(0.0, -1.0, -1e6) == 0.0


def test_symbols_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi._SIGS and getattr(lib, name).argtypes is not None, name
    for name in ("evaluate_wvm_svm", "weigh_wvm_svm", "wvm_svm_trace"):
        assert callable(getattr(capi.Particles, name)), name
    bad = capi.FD_ERR_INVALID_ARGUMENT   # NULL handles are refused before anything is touched
    assert lib.fd_particles_evaluate_wvm_svm(None, None, None, None, None, 1.0, None, 0) == bad
    assert lib.fd_particles_weigh_wvm_svm(None, None, None, None) == bad
    assert lib.fd_particles_get_wvm_svm_trace(None, None, None, None, None) == bad
