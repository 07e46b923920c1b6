"""ehog_eval_app in training mode: condensation::ExtendedHogBasedMeasurementModel built on a TrainableProbabilisticSvmClassifier
(libsvm::LibSvmClassifier, unlimited positives, age-based negatives) runs initialize -> evaluate -> adapt over three 160 x 120
frames.  Per frame the printed rho and weights must equal a Python replay: the examples are extracted with capi.EhogTracker at
the sample / bounds the app reports for every retraining, pass through a restatement of the two stores and are trained with
capi.linear_svm_train.  initialize leaves isUsable() true; an adapt whose target scores at or below adaptationThreshold leaves
the weights unchanged."""
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
CELL, OLC, D, COLS, ROWS = 5, 5, 13, 5, 7
CAPACITY, NEGATIVES, INITIAL = 12, 10, 50


@pytest.fixture(scope="module")
def frames(synth):
    base = synth.make_frame(W, H, seed=77)
    noise = np.random.default_rng(3).integers(-2, 3, base.shape)
    return [base, np.clip(base.astype(np.int32) + noise, 0, 255).astype(np.uint8), np.roll(base, 1, axis=1)]


@pytest.fixture(scope="module")
def trackers(capi, ctx, frames):
    """one tracker handle per frame with the model's parameters: the replay's feature extractor"""
    assert model.cell_grid(TARGET[2], TARGET[3], 35) == (COLS, ROWS)
    fp = capi.cehog_params(cell_size=CELL, bin_count=9, signed_gradients=False, unsigned_gradients=True, interpolate_bins=False,
                           interpolate_cells=True, alpha=0.48)
    prm = capi.ehog_tracker_params(fp, COLS, ROWS, OLC, CELL * COLS, model.max_width(W, H, TARGET[2], TARGET[3]))
    out = []
    for f in frames:
        t = capi.EhogTracker(ctx, prm)
        t.update(f)
        out.append(t)
    return out


def _run(tmp_path, synth, frames, adaptation_threshold):
    if not os.path.exists(APP):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / ("frame%d.ppm" % i)))
        synth.save_pnm(paths[-1], f)
    (tmp_path / "train.cfg").write_text(
        "target\n{\n    x %d\n    y %d\n    width %d\n    height %d\n}\n" % TARGET +
        "classifier\n{\n    training\n    {\n        c 1\n        compensateImbalance 0\n        negativeCapacity %d\n    }\n}\n" % CAPACITY +
        "adaptation position\nadaptationThreshold %.9g\n" % adaptation_threshold)
    rng = np.random.default_rng(21)
    size = rng.integers(20, 90, 30)
    samples = np.stack([rng.integers(0, W, 30), rng.integers(0, H, 30), size], 1)
    (tmp_path / "samples.txt").write_text("".join("%d %d %d\n" % tuple(r) for r in samples))
    r = subprocess.run([APP, str(tmp_path / "train.cfg"), paths[0], str(tmp_path / "samples.txt")] + paths[1:], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "grid %d %d" % (COLS, ROWS)
    out, k = [], 1
    while k < len(lines) and lines[k].startswith("frame "):
        t = lines[k].split()
        rec = dict(frame=int(t[1]), usable=int(t[3]), adapted=int(t[5]), trainings=[])
        k += 1
        while lines[k].startswith("train "):
            t = lines[k].split()
            npos, nneg = int(t[2]), int(t[4])
            boxes = [l.split() for l in lines[k + 1:k + 1 + npos + nneg]]
            assert [b[0] for b in boxes] == ["p"] * npos + ["n"] * nneg
            boxes = [tuple(int(v) for v in b[1:]) for b in boxes]
            rec["trainings"].append((boxes[:npos], boxes[npos:]))
            k += 1 + npos + nneg
        t = lines[k].split()
        assert t[0] == "info"
        rec["info"] = [int(v) for v in t[1:5]] + [float(t[5])]
        assert lines[k + 1].startswith("w")
        rec["w"] = np.array([float(v) for v in lines[k + 1].split()[1:]], np.float32)
        k += 2
        out.append(rec)
    return out


def _overlap(a, b):
    x0, y0 = max(a[0], b[0]), max(a[1], b[1])
    x1, y1 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = float(max(0, x1 - x0) * max(0, y1 - y0)) if x1 > x0 and y1 > y0 else 0.0
    return inter / (a[2] * a[3] + b[2] * b[3] - inter)


class Replay:
    """the classifier's side: unlimited positives, age-based negatives (AgeBasedExampleManagement.cpp:18-30), one training per
    retraining that brings something new"""

    def __init__(self, capi, ctx):
        self.capi, self.ctx = capi, ctx
        self.pos, self.neg, self.insert = [], [], 0
        self.w = self.rho = self.info = None

    def retrain(self, tracker, pos_samples, neg_bounds):
        if not pos_samples and not neg_bounds:
            return
        if pos_samples:
            valid, feats = tracker.extract_patches(pos_samples)
            assert valid.all()
            self.pos += [f.reshape(-1) for f in feats]
        if neg_bounds:
            valid, feats = tracker.extract_cells([(x + w // 2, y + h // 2, w, h) for (x, y, w, h) in neg_bounds])
            assert valid.all()
            for f in feats:
                if len(self.neg) < CAPACITY:
                    self.neg.append(f.reshape(-1))
                else:
                    self.neg[self.insert] = f.reshape(-1)
                    self.insert = (self.insert + 1) % len(self.neg)
        x = np.stack(self.pos + self.neg)
        self.w, _, _, self.info = self.capi.linear_svm_train(self.ctx, x, len(self.pos), C=1.0, eps=1e-4)

    def check(self, rec):
        i = self.info
        assert rec["info"] == [i["iterations"], i["converged"], i["n_sv"], i["n_bounded"], i["rho"]]
        assert rec["w"].shape == (ROWS * COLS * D,) and rec["w"].tobytes() == self.w.tobytes()


def test_initialize_evaluate_adapt_equal_the_replay(capi, ctx, synth, frames, trackers, tmp_path):
    recs = _run(tmp_path, synth, frames, 0.5)
    assert [r["frame"] for r in recs] == [0, 1, 2] and all(r["usable"] == 1 for r in recs)   # initialize leaves isUsable() true
    target_bounds = (TARGET[0] - TARGET[2] // 2, TARGET[1] - TARGET[3] // 2, TARGET[2], TARGET[3])
    # initialize: the target against 50 random windows, then the good negatives of the first model (at most negativeExampleCount)
    first, second = recs[0]["trainings"]
    assert first[0] == [TARGET] and len(first[1]) == INITIAL and second[0] == [] and 1 <= len(second[1]) <= NEGATIVES
    max_w = model.max_width(W, H, TARGET[2], TARGET[3])
    for (x, y, w, h) in first[1]:
        assert CELL * COLS <= w < max_w and h == w * ROWS // COLS and 0 <= x <= W - w and 0 <= y <= H - h
    assert len(set(first[1])) > INITIAL // 2
    for b in first[1] + second[1]:
        assert _overlap(target_bounds, b) < 0.5
    replay = Replay(capi, ctx)
    adapted = 0
    for rec in recs:
        for pos, neg in rec["trainings"]:
            replay.retrain(trackers[rec["frame"]], pos, neg)
        replay.check(rec)
        if rec["frame"] > 0 and rec["adapted"]:
            adapted += 1
            (pos, neg), = rec["trainings"]
            assert pos == [TARGET] and len(neg) <= NEGATIVES
    assert adapted >= 1 and len(replay.neg) == CAPACITY and len(replay.pos) == 1 + adapted
    assert recs[-1]["w"].tobytes() != recs[0]["w"].tobytes()


def test_adapt_below_the_threshold_leaves_the_weights(synth, frames, tmp_path):
    recs = _run(tmp_path, synth, frames, 1e9)
    assert len(recs) == 3 and len(recs[0]["trainings"]) == 2
    for rec in recs[1:]:
        assert rec["usable"] == 1 and rec["adapted"] == 0 and rec["trainings"] == []
        assert rec["w"].tobytes() == recs[0]["w"].tobytes() and rec["info"] == recs[0]["info"]
