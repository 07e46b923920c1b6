"""aggregated_detect_app with `features.type fpdw` (no image filter, ChainedFilter(FpdwFeaturesFilter, AggregationFilter) as layer
filter, through the host layer's classes), on exact feature layers and on the approximated pyramid with explicit lambdas: the
printed detections are the CPU model's (tests/fpdw_model.py), with the threshold in the largest gap of the model's top scores."""
import os
import subprocess

import numpy as np
import pytest

import aggregated_approx_model as approx
import fpdw_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "featuredetection_amd")
D = model.CHANNELS
CFG = dict(n=2, size=(320, 240), window_w=4, window_h=5, cell=4, min_window_width=0)
LAMBDAS = np.concatenate([np.linspace(0.05, 0.3, 6), [0.11, 0.0, 0.02, -0.03]])
SEEDS = {False: 5, True: 16}   # of the SVM weights, by `approximatePyramid`: the model's largest gap clears the score bound, >= 2 detections

CONFIG = """features
{
    type fpdw
    windowWidthInCells %(window_w)d
    windowHeightInCells %(window_h)d
    cellSizeInPixels %(cell)d
    widthScaleFactor 1.25
    heightScaleFactor 0.8
%(lambdas)s}
detection
{
    minWindowWidthInPixels %(min_window_width)d
    minWindowHeightInPixels 0
    octaveLayerCount %(n)d
    approximatePyramid %(approximate)s
    nmsOverlapThreshold 0.3
    threshold %(threshold)s
}
"""


def _run(args, ok=True):
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr)
    return r.stdout, r.stderr


def _app():
    app = os.path.join(PKG, "aggregated_detect_app")
    if not os.path.exists(app):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    return app


def _svm(tmp_path, synth, name, weights, bias):
    svm = dict(kernel=0, sv=weights.reshape(1, -1), coeff=np.ones(1, np.float32), bias=bias)
    synth.save_svm_text(str(tmp_path / name), svm, rows=weights.shape[0], cols=weights.shape[1] * D)
    return str(tmp_path / name)


def _config(tmp_path, name, approximate, threshold, lambdas=None):
    lam = "" if lambdas is None else '    lambdas "%s"\n' % " ".join("%.17g" % v for v in lambdas)
    (tmp_path / name).write_text(CONFIG % dict(CFG, approximate="true" if approximate else "false", threshold="%.9g" % threshold, lambdas=lam))
    return str(tmp_path / name)


def _weights(seed):
    return np.random.default_rng(seed).normal(0, 0.05, (CFG["window_h"], CFG["window_w"], D)).astype(np.float32)


@pytest.mark.parametrize("approximate", [False, True], ids=["exact", "approximated"])
def test_aggregated_detect_app_fpdw(tmp_path, oracle, synth, approximate):
    W, H = CFG["size"]
    frame = synth.make_frame(W, H, seed=77)
    path = str(tmp_path / "frame.ppm")
    synth.save_pnm(path, frame)
    weights, bias = _weights(SEEDS[approximate]), float(np.float32(0.1))
    ws, hs = float(np.float32(1.0) / np.float32(1.25)), float(np.float32(1.0) / np.float32(0.8))
    p = model.params(CFG["cell"])
    layers, feats, _ = model.feature_layers(oracle, frame, CFG, p, approximate, LAMBDAS if approximate else None)
    thr, scores, bounds = model.gap_threshold(layers, feats, weights, bias, p)
    sc, bx, _ = approx.candidates(layers, scores, thr, CFG, ws, hs)
    bd = np.concatenate([b[s > np.float32(thr)] for s, b in zip(scores, bounds)])
    assert len(sc) >= 2
    keep_s, keep_b = oracle.nms_iou(sc.astype(np.float32), bx, 0.3, 0)
    out, _ = _run([_app(), _config(tmp_path, "fpdw.cfg", approximate, thr, LAMBDAS if approximate else None),
                   _svm(tmp_path, synth, "window.svm.txt", weights, bias), path])
    lines = [l.split() for l in out.strip().splitlines()]
    assert len(lines) == len(keep_s) > 0
    for g, s, b in zip(lines, keep_s, keep_b):
        assert int(g[0]) == 0 and [int(v) for v in g[1:5]] == [int(v) for v in b]
        k = int(np.argmin(np.abs(sc.astype(np.float32) - s)))   # MAX_SCORE keeps a candidate's own score
        assert abs(float(g[5]) - float(sc[k])) <= bd[k]


def test_aggregated_detect_app_fpdw_errors(tmp_path, oracle, synth):
    app = _app()
    svm = _svm(tmp_path, synth, "zero.svm.txt", np.zeros((CFG["window_h"], CFG["window_w"], D), np.float32), 0.0)
    gray = str(tmp_path / "frame.pgm")
    synth.save_pnm(gray, oracle.bgr2gray(synth.make_frame(320, 240, seed=1)))
    for approximate in (False, True):
        _, err = _run([app, _config(tmp_path, "gray.cfg", approximate, 0.0, LAMBDAS if approximate else None), svm, gray], ok=False)
        assert "the gradient image type must be CV_8UC3" in err
    frame = str(tmp_path / "frame.ppm")
    synth.save_pnm(frame, synth.make_frame(320, 240, seed=1))
    _, err = _run([app, _config(tmp_path, "count.cfg", True, 0.0, np.zeros(31)), svm, frame], ok=False)
    assert "the number of lambdas does not match the number of channels" in err
    _, err = _run([app, _config(tmp_path, "exactlam.cfg", False, 0.0, LAMBDAS), svm, frame], ok=False)
    assert "features.lambdas belong to approximatePyramid true" in err
