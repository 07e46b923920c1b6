"""condensation::ExtendedHogBasedMeasurementModel (evaluation half) through ehog_eval_app against tests/ehog_model.py: sample scores
bit for bit, weights through the logistic, the heat peak, the good negative examples, the re-initialisation branches of a lost
target, and the fused-call counter (one fd_ehog_tracker_evaluate_samples per batched evaluate)."""
import math
import os
import subprocess

import numpy as np
import pytest

import ehog_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "ehog_eval_app")
W, H = 160, 120
TARGET = (80, 60, 30, 42)          # x, y, width, height: aspect 1.4 -> 5 x 7 cells
CELL, OLC, BINS, ALPHA, D = 5, 5, 9, 0.48, 13
BIAS, LOGISTIC_A, LOGISTIC_B = 0.2, 0.3, -1.7
REJECTION = -0.1


def _probability(d):
    f = LOGISTIC_A + LOGISTIC_B * d
    return math.exp(-f) / (1.0 + math.exp(-f)) if f >= 0 else 1.0 / (1.0 + math.exp(f))


class Scene:
    def __init__(self, capi, ctx, synth):
        self.cols, self.rows = model.cell_grid(TARGET[2], TARGET[3], 35)
        assert (self.cols, self.rows) == (5, 7)
        self.frame = synth.make_frame(W, H, seed=77)
        self.min_w, self.max_w = CELL * self.cols, model.max_width(W, H, TARGET[2], TARGET[3])
        self.layers = model.plan_layers(W, H, self.cols, CELL, self.min_w, self.max_w, OLC)
        mn, mx = model.pyramid_limits(self.cols, CELL, self.min_w, self.max_w, OLC)
        pyr = capi.Pyramid(ctx, octave_layers=OLC, min_scale=mn, max_scale=mx)
        pyr.update(self.frame)
        gray = [pyr.layer(i) for i in range(len(pyr.layers()))]
        self.weights = (np.random.default_rng(8).standard_normal((self.rows, self.cols, D)) * 0.4).astype(np.float32)
        self.features = [model.cehog(g, CELL, BINS, False, True, False, True, ALPHA) for g in gray]
        self.heats = [model.heat_layer(f, self.weights, BIAS) for f in self.features]
        self.svm = dict(kernel=0, p0=0.0, p1=0.0, p2=0.0, dtype=1, sv=self.weights.reshape(1, -1), coeff=np.ones(1, np.float32), bias=np.float32(BIAS),
                        threshold=0.0, logistic_a=LOGISTIC_A, logistic_b=LOGISTIC_B)

    def score(self, x, y, size):
        height = model.cv_round(self.rows / self.cols * size)
        win = model.sample_window(x, y, size, height, self.layers, self.cols, self.rows, CELL, OLC)
        if win is None:
            return None
        li, bx, by = win
        return self.heats[li][by + self.rows // 2, bx + self.cols // 2]


@pytest.fixture(scope="module")
def scene(capi, ctx, synth):
    return Scene(capi, ctx, synth)


def _samples():
    rng = np.random.default_rng(21)
    size = rng.integers(20, 90, 80)
    return np.stack([rng.integers(0, W, 80), rng.integers(0, H, 80), size], 1).astype(np.int32)


def _run(tmp_path, synth, scene, threshold, extra=""):
    if not os.path.exists(APP):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    synth.save_svm_text(str(tmp_path / "svm.txt"), scene.svm, rows=scene.rows, cols=scene.cols * D)
    synth.save_pnm(str(tmp_path / "frame.ppm"), scene.frame)
    (tmp_path / "eval.cfg").write_text(
        "target\n{\n    x %d\n    y %d\n    width %d\n    height %d\n}\n" % TARGET +
        "classifier\n{\n    classifierFile %s\n    threshold %.9g\n}\nrejectionThreshold %s\n%s" % (tmp_path / "svm.txt", threshold, REJECTION, extra))
    samples = _samples()
    (tmp_path / "samples.txt").write_text("".join("%d %d %d\n" % tuple(r) for r in samples))
    r = subprocess.run([APP, str(tmp_path / "eval.cfg"), str(tmp_path / "frame.ppm"), str(tmp_path / "samples.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "grid %d %d" % (scene.cols, scene.rows)
    rows = [l.split() for l in lines[1:1 + len(samples)]]
    peak = lines[1 + len(samples)].split()
    assert peak[0] == "peak"
    neg = lines[2 + len(samples)].split()
    assert neg[0] == "negatives"
    boxes = [tuple(int(v) for v in l.split()) for l in lines[3 + len(samples):]]
    assert len(boxes) == int(neg[1])
    return samples, rows, peak, boxes, r.stderr


def _check_peak_and_negatives(scene, peak, boxes, threshold=-1.0):
    found, score, bounds = model.heat_peak(scene.heats, scene.layers, scene.cols, scene.rows, CELL)
    assert found and np.float32(float(peak[1])) == score and tuple(int(v) for v in peak[2:]) == bounds
    maxima = model.heat_maxima(scene.heats, scene.layers, scene.cols, scene.rows, CELL, threshold)
    target_bounds = (TARGET[0] - TARGET[2] // 2, TARGET[1] - TARGET[3] // 2, TARGET[2], TARGET[3])
    want = model.good_negative_boxes(maxima, target_bounds)
    assert boxes == want
    return want


def test_tracked_target(tmp_path, synth, scene):
    """the target is not lost and the peak does not classify (threshold above every score): every sample is scored where it is"""
    samples, rows, peak, boxes, err = _run(tmp_path, synth, scene, 1e6)
    assert "80 samples: 1 fused device call(s)" in err
    nvalid = 0
    for s, r in zip(samples, rows):
        want = scene.score(*s)
        assert (int(r[3]), int(r[4]), int(r[5])) == tuple(s)
        if want is None:
            assert r[:3] == ["0", "0", "0"]
            continue
        nvalid += 1
        assert np.float32(float(r[1])) == want
        assert int(r[0]) == int(want > REJECTION)
        assert math.isclose(float(r[2]), _probability(float(want)), rel_tol=1e-14)
    assert 15 < nvalid < 75
    assert len({r[6] for r in rows}) == len(rows)   # nobody was re-initialised: the cluster ids are the samples' own
    want = _check_peak_and_negatives(scene, peak, boxes)
    assert len(want) >= 2


def test_lost_target_is_reinitialised_at_the_peak(tmp_path, synth, scene):
    """targetLost and a peak that classifies: the samples are redrawn around the peak, share a new cluster id and are scored there"""
    samples, rows, peak, boxes, err = _run(tmp_path, synth, scene, -1e6, "targetLost 1\n")
    assert "80 samples: 1 fused device call(s)" in err
    _check_peak_and_negatives(scene, peak, boxes)
    px, py, pw, ph = (int(v) for v in peak[2:])
    assert len({r[6] for r in rows}) == 1
    moved = 0
    for s, r in zip(samples, rows):
        x, y, size = int(r[3]), int(r[4]), int(r[5])
        moved += (x, y, size) != tuple(s)
        assert abs(x - (px + pw // 2)) <= 0.2 * pw * 6 + 1 and abs(y - (py + ph // 2)) <= 0.2 * pw * 6 + 1 and abs(size - pw) <= 0.2 * pw * 6 + 1
        want = scene.score(x, y, size)
        if want is None:
            assert r[:3] == ["0", "0", "0"]
            continue
        assert np.float32(float(r[1])) == want and r[0] == "1"   # a lost target: the classifier's verdict, score >= threshold
        assert math.isclose(float(r[2]), _probability(float(want)), rel_tol=1e-14)
    assert moved >= 78


def test_lost_target_without_a_classifying_peak(tmp_path, synth, scene):
    samples, rows, peak, boxes, err = _run(tmp_path, synth, scene, 1e6, "targetLost 1\n")
    assert "80 samples: 0 fused device call(s)" in err
    for s, r in zip(samples, rows):
        assert r[:3] == ["0", "0", "0"] and (int(r[3]), int(r[4]), int(r[5])) == tuple(s)
    _check_peak_and_negatives(scene, peak, boxes)
