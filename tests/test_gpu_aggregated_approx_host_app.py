"""aggregated_detect_app (the host layer's two ways to an AggregatedFeaturesDetector, chosen by the config key `approximatePyramid`)
with `approximatePyramid true` and `false` on a synthetic frame and a written SVM file: the printed detections equal the CPU
model's (tests/aggregated_approx_model.py), respectively the frozen oracle's exact detector."""
import os
import subprocess

import numpy as np
import pytest

import aggregated_approx_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "featuredetection_amd")
D = 31
CFG = dict(n=4, size=(640, 480), window_w=8, window_h=10, cell=8, min_window_width=0, unsigned_bins=9)
LAMBDAS = np.linspace(0.02, 0.3, D)

CONFIG = """features
{
    type fhog
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
    approximatePyramid %(approximate)s ; exact feature layers or the approximated pyramid
    nmsOverlapThreshold 0.3
    threshold %(threshold)s
}
"""


def _run(args, ok=True):
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr)
    return r.stdout, r.stderr


def _setup(tmp_path, synth, weights, bias):
    app = os.path.join(PKG, "aggregated_detect_app")
    if not os.path.exists(app):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    svm = dict(kernel=0, sv=weights.reshape(1, -1), coeff=np.ones(1, np.float32), bias=bias)
    synth.save_svm_text(str(tmp_path / "window.svm.txt"), svm, rows=weights.shape[0], cols=weights.shape[1] * D)
    return app


def _config(tmp_path, name, approximate, threshold, lambdas=None, **over):
    lam = "" if lambdas is None else '    lambdas "%s"\n' % " ".join("%.17g" % v for v in lambdas)
    (tmp_path / name).write_text(CONFIG % dict(CFG, approximate=approximate, threshold="%.9g" % threshold, lambdas=lam, **over))
    return str(tmp_path / name)


def _same_lines(out, image_index, score, xywh):
    lines = [l.split() for l in out.strip().splitlines() if int(l.split()[0]) == image_index]
    assert len(lines) == len(score) > 0
    for g, s, b in zip(lines, score, xywh):
        assert [int(v) for v in g[1:5]] == [int(v) for v in b]
        assert np.float32(float(g[5])) == s


def test_aggregated_detect_app_both_pyramids(tmp_path, oracle, synth):
    W, H = CFG["size"]
    frames = [synth.make_frame(W, H, seed=77), oracle.bgr2gray(synth.make_frame(W, H, seed=78))]
    weights = np.random.default_rng(5).normal(0, 0.05, (CFG["window_h"], CFG["window_w"], D)).astype(np.float32)
    bias = float(np.float32(0.1))
    ws, hs = float(np.float32(1.0) / np.float32(1.25)), float(np.float32(1.0) / np.float32(0.8))
    app = _setup(tmp_path, synth, weights, bias)
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / ("frame%d.%s" % (i, "ppm" if f.ndim == 3 else "pgm"))))
        synth.save_pnm(paths[-1], f)
    layers = model.plan(CFG["window_w"], CFG["window_h"], CFG["cell"], CFG["n"], 0, W, H)
    # approximated, explicit lambdas: everything is fixed by the model
    feats = [model.feature_layers(oracle, f, layers, CFG, LAMBDAS)[0] for f in frames]
    scores = [model.all_scores(layers, ft, weights, bias) for ft in feats]
    thr = float(np.float32(np.quantile(np.concatenate([s.ravel() for s in scores[0]]), 0.995)))
    out, _ = _run([app, _config(tmp_path, "approx.cfg", "true", thr, LAMBDAS), str(tmp_path / "window.svm.txt")] + paths)
    approx_first = None
    for i in range(len(frames)):
        sc, bx, where = model.candidates(layers, scores[i], thr, CFG, ws, hs)
        assert {layers[k]["approximated"] for k in where.tolist()} == {0, 1}
        fs, fb = oracle.nms_iou(sc, bx, 0.3, 0)
        _same_lines(out, i, fs, fb)
        approx_first = approx_first if approx_first is not None else fs
    # exact: the frozen oracle's detector
    out, _ = _run([app, _config(tmp_path, "exact.cfg", "false", thr), str(tmp_path / "window.svm.txt")] + paths)
    for i, f in enumerate(frames):
        so, bo = oracle.aggregated_candidates(f, weights, bias, thr, cell_size=CFG["cell"], octave_layers=CFG["n"], width_scale=ws, height_scale=hs)
        fs, fb = oracle.nms_iou(so, bo, 0.3, 0)
        _same_lines(out, i, fs, fb)
        if i == 0:
            assert len(fs) != len(approx_first) or not np.array_equal(fs, approx_first)   # the two configs are told apart
    # approximated, estimated lambdas: runs, and prints detections
    out, _ = _run([app, _config(tmp_path, "estimate.cfg", "true", thr), str(tmp_path / "window.svm.txt")] + paths)
    assert len(out.strip().splitlines()) > 0


def test_aggregated_detect_app_errors(tmp_path, oracle, synth):
    weights = np.zeros((CFG["window_h"], CFG["window_w"], D), np.float32)
    app = _setup(tmp_path, synth, weights, 0.0)
    frame = str(tmp_path / "frame.ppm")
    synth.save_pnm(frame, synth.make_frame(640, 480, seed=1))
    small = str(tmp_path / "small.pgm")
    synth.save_pnm(small, np.zeros((100, 100), np.uint8))
    svm = str(tmp_path / "window.svm.txt")
    _, err = _run([app, _config(tmp_path, "count.cfg", "true", 0.0, np.zeros(30)), svm, frame], ok=False)
    assert "the number of lambdas does not match the number of channels" in err
    _, err = _run([app, _config(tmp_path, "ok.cfg", "true", 0.0), svm, small], ok=False)
    assert "at least two pyramid layers are needed to estimate the lambdas" in err
    _run([app, _config(tmp_path, "bad.cfg", "maybe", 0.0), svm, frame], ok=False)


def test_approximated_pyramid_boundary():
    """an approximated pyramid used for anything but the aggregated detector, and the extractor on anything but such a pyramid,
    throw logic_error (aggregated_boundary_app)"""
    app = os.path.join(PKG, "aggregated_boundary_app")
    if not os.path.exists(app):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    out, _ = _run([app])
    lines = dict(l.split() for l in out.strip().splitlines())
    assert set(lines) == {"approximate_a_source_pyramid", "update", "get_layers", "layer_scales", "other_layer_filter", "second_layer_filter",
                          "sliding_window_extractor", "extractor_on_exact_pyramid", "fixed_min_scale"}
    assert all(v == "logic_error" for v in lines.values()), lines
