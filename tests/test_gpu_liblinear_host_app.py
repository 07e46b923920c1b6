"""svm_train_app with `training liblinear`: a liblinear::LibLinearClassifier from a feature matrix and a config with headTrackingApp's
keys, against capi.liblinear_train on the same rows (the static negatives behind the matrix's)."""
import os
import subprocess

import numpy as np
import pytest

import liblinear_cases as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "svm_train_app")


def _run(tmp_path, x, n_pos, config):
    feats, cfg, out = tmp_path / "features.txt", tmp_path / "classifier.cfg", tmp_path / "svm.txt"
    with open(feats, "w") as f:
        f.write("%d %d %d\n" % (n_pos, len(x) - n_pos, x.shape[1]))
        for row in x:
            f.write(" ".join("%.9g" % v for v in row) + "\n")
    cfg.write_text(config)
    return subprocess.run([APP, str(feats), str(cfg), str(out)], capture_output=True, text=True, timeout=120), out


def _read_linear_svm(path, d):
    """the text format of SvmClassifier::store as a capi.Svm model dict"""
    tokens = open(path).read().split()
    assert tokens[:3] == ["Kernel", "Linear", "Bias"] and tokens[4] == "Coefficients" and tokens[5] == "1"
    bias, coeff = np.float32(tokens[3]), np.array(tokens[6:7], np.float32)
    assert tokens[7:13] == ["SupportVectors", "1", "1", str(d), "1", "5"]
    sv = np.array(tokens[13:13 + d], np.float32).reshape(1, d)
    assert len(tokens) == 13 + d
    return dict(kernel=0, p0=0.0, p1=0.0, p2=0.0, dtype=1, sv=sv, coeff=coeff, bias=bias)


@pytest.mark.parametrize("bias", [False, True])
def test_training_liblinear(capi, ctx, tmp_path, bias):
    x, n_pos, n_neg, c, _ = L.case("bias39")
    static = L.make_x(91, 1, 5, x.shape[1])[1:]
    negatives = tmp_path / "negatives.txt"
    negatives.write_text("".join(";".join("%.9g" % (4 * v) for v in row) + "\n" for row in static))
    run, out = _run(tmp_path, x, n_pos, "kernel linear\ntraining liblinear\n{\n\tC 0.5\n\tbias %s\n\tstaticNegativeExamples true\n\t{\n"
                    "\t\tfilename %s\n\t\tamount 4\n\t\tscale 0.25\n\t}\n}\n" % ("true" if bias else "false", negatives))
    assert run.returncode == 0, run.stderr
    printed = dict(line.split() for line in run.stdout.strip().splitlines())
    rows = np.concatenate([x, static[:4]])
    w, b, _, _, info = capi.liblinear_train(ctx, rows, n_pos, C=0.5, bias=bias)
    assert int(printed["iterations"]) == info["iterations"] and int(printed["cg_steps"]) == info["cg_steps"]
    assert int(printed["negatives"]) == n_neg + 4
    model = _read_linear_svm(out, x.shape[1])
    assert model["sv"].tobytes() == w.tobytes() and model["coeff"][0] == 1.0
    assert np.float32(model["bias"]).tobytes() == np.float32(b).tobytes() == np.float32(printed["bias"]).tobytes()
    want = rows.astype(np.float64) @ w.astype(np.float64) - float(b)
    got = capi.Svm(ctx, model).distance(rows)
    clear = np.abs(want) > 1e-4 * (1 + np.abs(rows).astype(np.float64) @ np.abs(w).astype(np.float64))   # float32 scoring
    assert np.array_equal(np.sign(got[clear]), np.sign(want[clear])) and clear.sum() > len(rows) // 2


def test_without_static_negatives_and_with_defaults(capi, ctx, tmp_path):
    x, n_pos, n_neg, c, _ = L.case("c100")
    run, out = _run(tmp_path, x, n_pos, "kernel linear\ntraining liblinear\n")
    assert run.returncode == 0, run.stderr
    w, b, _, _, info = capi.liblinear_train(ctx, x, n_pos)
    model = _read_linear_svm(out, x.shape[1])
    assert model["sv"].tobytes() == w.tobytes() and model["bias"] == 0 and b == 0


def test_another_kernel_is_refused(tmp_path):
    x, n_pos, _, _, _ = L.case("tiny")
    run, out = _run(tmp_path, x, n_pos, "kernel rbf\n{\n\tgamma 0.5\n}\ntraining liblinear\n{\n\tC 1\n}\n")
    assert run.returncode != 0 and "training liblinear needs kernel linear" in run.stderr and not os.path.exists(out)


# ---- tracker_app: training { type libLinear } ----

STATIC = [(60, 40)] * 9   # the first frame initialises the tracker, eight are processed


def _track(tmp_path, training):
    import test_gpu_condensation_host_app as T
    settings = dict(count=120, rate="0.25", seed=5, sliding=1, adaptation="position", threshold="0")
    text = (T.CONFIG % settings).replace("training { c 1 compensateImbalance 0 negativeCapacity 100 }", training)
    assert training in text
    config = tmp_path / "tracking.cfg"
    config.write_text(text)
    paths = T._write_frames(tmp_path, STATIC)
    x0, y0 = STATIC[0]
    return subprocess.run([T.APP, "--dump", str(config), str(x0), str(y0), "30", "40"] + paths, capture_output=True, text=True, timeout=120), T


@pytest.mark.parametrize("bias", [0, 1])
def test_tracker_app_trains_a_liblinear_classifier(tmp_path, bias):
    """The model goes retrain -> weights -> fd_ehog_tracker_set_svm, the route of a trainable that does not train on the tracker
    handle.  The target stands still, so the window the classifier was trained on as its one positive is there in every frame:
    the tracker has to find it within two cells (8 pixels; the samples scatter with a deviation of 3) and to adapt on it, and the
    samples' scores have to differ, which they do not while the heat pyramid's weights are zero."""
    run, T = _track(tmp_path, "training { type libLinear c 1 bias %d negativeCapacity 100 }" % bias)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.startswith("init 1 %d %d 30 40" % STATIC[0])
    frames = T._parse(run.stdout)
    assert len(frames) == 8
    for f, fr in enumerate(frames):
        scores = fr["gen"]["score"]
        print(f, fr["found"], fr["box"], fr["adapted"], float(scores.min()), float(scores.max()))
        assert fr["found"] == 1 and fr["adapted"] == 1, f
        x, y, w, h = fr["box"]
        assert abs(x + w / 2 - (STATIC[0][0] + 15)) <= 8 and abs(y + h / 2 - (STATIC[0][1] + 20)) <= 8, (f, fr["box"])
        assert scores.max() > scores.min(), f


def test_tracker_app_refuses_an_unknown_training_type(tmp_path):
    run, _ = _track(tmp_path, "training { type libFoo c 1 negativeCapacity 100 }")
    assert run.returncode != 0 and "invalid training type: libFoo" in run.stdout + run.stderr
