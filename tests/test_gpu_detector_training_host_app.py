"""detector_training_app end to end: six synthetic 128 x 96 images (a textured square on noise each, one with an `ignore` region),
FHOG with cell 8, window 4 x 4, two layers per octave, 4 random negatives and at most 8 hard negatives per image, two rounds,
mirroring -- once with unlimited negatives, once with maxNegatives = 60, where HardNegativeExampleManagement drops examples.

The app's trace is replayed in Python: tests/detector_training_model.py's training loop, features through
capi.Aggregated.update / extract, hard negatives through capi.Aggregated.set_svm / detect, training through svm_train_model on the
device's Q.  The replay must reproduce every record of the trace bit for bit, and the stored SVM file.

The held-out image's square is found with IoU >= 0.5 at threshold 0.  That is a condition on the inputs: it was checked on the
CPU, with the oracle's FHOG and aggregated detector and svm_train_model in place of the device (random negatives drawn from
numpy's generator, seed 1; unlimited and 60 negatives), where the one detection left by the non-maximum suppression has IoU
0.71 with the square."""
import os
import subprocess

import numpy as np
import pytest

import detector_training_model as T
import svm_train_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "featuredetection_amd")
CFG = dict(window_w=4, window_h=4, cell=8, n=2)
SEED = 1
FEATURES = "type fhog\nwindowWidthInCells 4\nwindowHeightInCells 4\ncellSizeInPixels 8\noctaveLayerCount 2\nwidthScaleFactor 1\nheightScaleFactor 1\n"
TRAINING = ("mirrorTrainingData true\nmaxNegatives %d\nrandomNegativesPerImage 4\nmaxHardNegativesPerImage 8\nbootstrappingRounds 2\n"
            "negativeScoreThreshold -1\noverlapThreshold %s\nC 1\ncompensateImbalance false\nprobabilistic %s\n")
DETECTION = ("features {\n type fhog\n windowWidthInCells 4\n windowHeightInCells 4\n cellSizeInPixels 8\n widthScaleFactor 1\n heightScaleFactor 1\n}\n"
             "detection {\n minWindowWidthInPixels 0\n minWindowHeightInPixels 0\n octaveLayerCount 2\n approximatePyramid false\n"
             " nmsOverlapThreshold 0.3\n threshold 0\n}\n")


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    d = tmp_path_factory.mktemp("detector_training_app")
    data = T.make_training_set(SEED)
    lines = []
    for k, (img, boxes) in enumerate(data):
        _write_pgm(str(d / ("image%d.pgm" % k)), img)
        if k < len(data) - 1:
            lines.append(" ".join([str(d / ("image%d.pgm" % k))] + ["%s %d %d %d %d" % b for b in boxes]))
    (d / "images.lst").write_text("\n".join(lines) + "\n")
    (d / "features.cfg").write_text(FEATURES)
    (d / "detection.cfg").write_text(DETECTION)
    return d, data


def _run_app(d, name, max_negatives, overlap="0.3", probabilistic="false", images="images.lst"):
    (d / (name + ".cfg")).write_text(TRAINING % (max_negatives, overlap, probabilistic))
    return subprocess.run([os.path.join(PKG, "detector_training_app"), "train", str(d / images), str(d / "features.cfg"), str(d / (name + ".cfg")),
                           str(d / (name + ".svm")), "--seed", "3", "--trace", str(d / (name + ".trace"))], capture_output=True, text=True)


class DeviceBackend:
    def __init__(self, capi, ctx):
        self.det = capi.Aggregated(ctx, np.zeros((4, 4, 31), np.float32), 0.0, 0.0, cell_size=8, octave_layers=2, nms_overlap=1.0)

    def update(self, image):
        self.image = image
        self.det.update(image)

    def extract(self, box):
        feats, bounds, valid = self.det.extract([box])
        if not valid[0]:
            return None
        b = bounds[0]
        return feats[0].copy(), (int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]))

    def detect(self, weights, bias, threshold):
        self.det.set_svm(weights, float(bias), threshold)
        _, cand = self.det.detect(self.image)
        return [(int(c["x"]), int(c["y"]), int(c["w"]), int(c["h"])) for c in cand]


def _replay(capi, ctx, data, draws, max_negatives):
    params = dict(mirror=True, random_per_image=4, max_hard_per_image=8, rounds=2, negative_threshold=-1.0, overlap=0.3,
                  max_negatives=max_negatives, C=1.0)

    def train_fn(x, n_pos, C):
        q, qd = capi.linear_svm_gram(ctx, x, n_pos)
        r = M.train(x, n_pos, C, q=q, qd=qd)
        assert r["converged"] == 1
        return r["weights"], r["rho"], r["iterations"]

    return T.replay_training(data[:-1], CFG, params, DeviceBackend(capi, ctx), train_fn, draws=draws)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_records(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (k, g[0], w[0])
        if g[0] != "training":
            assert g == w, (k, g, w)
            continue
        assert g[1:7] == w[1:7], (k, g[1:7], w[1:7])   # initial, n_pos, n_neg, new_pos, new_neg, iterations
        assert _bits(np.float64(g[7])) == _bits(np.float64(w[7])), (k, g[7], w[7])
        assert _bits(g[8].reshape(-1)) == _bits(w[8].reshape(-1)), (k, np.abs(g[8].reshape(-1) - w[8].reshape(-1)).max())


def _read_svm(path):
    """(bias, weights) of the text format of SvmClassifier::store, which prints nine significant digits: exact for float32"""
    tokens = open(path).read().split()
    assert tokens[:2] == ["Kernel", "Linear"] and tokens[2] == "Bias" and tokens[4:7] == ["Coefficients", "1", "1"]
    assert tokens[7:13] == ["SupportVectors", "1", "4", "4", "31", "5"]
    return np.float32(tokens[3]), np.array(tokens[13:], np.float32)


@pytest.fixture(scope="module")
def unlimited(capi, ctx, scene):
    d, data = scene
    run = _run_app(d, "unlimited", 0)
    assert run.returncode == 0, run.stderr
    trace, draws = T.parse_trace((d / "unlimited.trace").read_text())
    return trace, _replay(capi, ctx, data, draws, 0)


def test_replay_equals_the_trace(unlimited, scene):
    trace, replay = unlimited
    _same_records(replay, trace)
    trainings = [r for r in trace if r[0] == "training"]
    assert len(trainings) == 3 and [r[1] for r in trainings] == [True, False, False]
    assert (trainings[0][2], trainings[0][3]) == (12, 48) and trainings[1][3] > 48 and trainings[2][3] > trainings[1][3]
    # the random draws are valid draws, the hard negatives were looked at in the detector's order and some were refused
    blocks = [r for r in trace if r[0] == "image"]
    assert len(blocks) == 3 * 12 and [b[1:] for b in blocks[:3]] == [(0, 0, -1), (0, 1, -1), (1, 0, -1)]
    assert all(T.is_random_bounds(r[1], 128, 96, 4, 4, 8) for r in trace if r[0] == "random")
    hard = [r for r in trace if r[0] == "hard"]
    assert any(not r[2] for r in hard) and any(r[2] for r in hard)
    assert any(not r[2] for r in trace if r[0] == "random")   # a draw on the square or the ignore region
    # the stored file holds the last training's numbers
    bias, weights = _read_svm(str(scene[0] / "unlimited.svm"))
    assert _bits(weights) == _bits(replay[-1][8].reshape(-1)) and _bits(bias) == _bits(np.float32(replay[-1][7]))
    assert _bits(trace[-1][9]) == _bits(bias)


def test_replay_with_dropped_negatives(capi, ctx, scene):
    d, data = scene
    run = _run_app(d, "bounded", 60)
    assert run.returncode == 0, run.stderr
    trace, draws = T.parse_trace((d / "bounded.trace").read_text())
    replay = _replay(capi, ctx, data, draws, 60)
    _same_records(replay, trace)
    trainings = [r for r in trace if r[0] == "training"]
    assert [r[3] for r in trainings] == [48, 60, 60] and trainings[1][5] > 12 and trainings[2][5] > 0   # more came in than fit
    bias, weights = _read_svm(str(d / "bounded.svm"))
    assert _bits(weights) == _bits(replay[-1][8].reshape(-1)) and _bits(bias) == _bits(np.float32(replay[-1][7]))


def test_trained_detector_finds_the_held_out_square(capi, ctx, unlimited, scene):
    d, data = scene
    _, replay = unlimited
    img, boxes = data[-1]
    w, bias = replay[-1][8], float(np.float32(replay[-1][7]))
    det = capi.Aggregated(ctx, w, bias, 0.0, cell_size=8, octave_layers=2, nms_overlap=0.3)
    found, _ = det.detect(img)
    ious = [T.overlap((int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])), boxes[0][1:]) for b in found]
    print("held-out detections:", [(int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]), float(b["score"])) for b in found], "IoU", ious)
    assert ious and max(ious) >= 0.5
    # aggregated_detect_app with the stored file returns the same detections
    run = subprocess.run([os.path.join(PKG, "aggregated_detect_app"), str(d / "detection.cfg"), str(d / "unlimited.svm"),
                          str(d / ("image%d.pgm" % (len(data) - 1)))], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = [ln.split() for ln in run.stdout.splitlines()]
    assert [tuple(int(v) for v in r[1:5]) for r in rows] == [(int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])) for b in found]
    assert [np.float32(r[5]) for r in rows] == [np.float32(b["score"]) for b in found]
    det.close()


def test_documented_exceptions(scene):
    d, data = scene
    run = _run_app(d, "probabilistic", 0, probabilistic="true")
    assert run.returncode == 1 and "invalid argument" in run.stderr and "probabilistic" in run.stderr
    # an image its annotations cover: with an overlap threshold of 0 every draw touches the ignore region
    (d / "covered.lst").write_text("%s ignore-all 0 0 128 96\n" % (d / "image0.pgm"))
    run = _run_app(d, "covered", 0, overlap="0", images="covered.lst")
    assert run.returncode == 1 and "runtime error" in run.stderr and "no random negative found" in run.stderr
