"""The ihog / iehog feature types through the C++ host layer: condensation::SingleClassifierModel on IntegralFeatureExtractor and
PatchResizingFeatureExtractor wrappers (integral_eval_app), condensation::PositionDependentMeasurementModel on the reference's default
`feature ihog` block (position_dependent_eval_app, every choice of adapt against the restatement of tests/pyramid_samples_model.py
with the integral extractor's window rule and features), and tracker_app on `measurement positionDependent` with integral features.
The Python side maps the samples through the two wrappers (tests/integral_hog_model.py) and calls capi.Integral."""
import os
import subprocess

import numpy as np
import pytest

import integral_hog_model as hog_model
import pyramid_samples_model as selection_model
from test_gpu_integral_host_app import ASPECT, _samples
from test_integral_hog_model import capi_params
from test_position_dependent_host import W as PW, H as PH, make_frames, run_app, tracker_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_APP = os.path.join(ROOT, "featuredetection_amd", "integral_eval_app")
W, H = 160, 120

# the `feature ihog` block of the reference's default tracker configurations (headTrackingApp/default.cfg:94)
DEFAULT_IHOG = """feature ihog { scale 1.1  signed false  interpolate true  bins 9  gradientCount 30
               histogram spatial { cellSize 6  blockSize 1  interpolate false  normalization l2norm } }"""
IEHOG = dict(grid=(30, 30), bins=18, signed=True, interpolate_bins=False, filter="ehog", cell=6, interpolate=False, sau=True, alpha=0.2)
EVAL_FEATURES = {
    "ihog": ("feature ihog\n{\n    scale %s\n    signed false\n    interpolate true\n    bins 9\n    gradientCount 30\n    histogram spatial\n    {\n"
             "        cellSize 6\n        blockSize 1\n        interpolate false\n        normalization l2norm\n    }\n}\n", hog_model.DEFAULT),
    "iehog": ("feature iehog\n{\n    scale %s\n    signed true\n    interpolate false\n    bins 18\n    gradientCount 30\n    histogram\n    {\n"
              "        cellSize 6\n        interpolate 0\n        signedAndUnsigned 1\n        alpha 0.2\n    }\n}\n", IEHOG),
}


@pytest.mark.parametrize("kind,scale", [("ihog", 1.1), ("iehog", 1.1), ("ihog", 1)], ids=["ihog-1.1", "iehog-1.1", "ihog-1"])
def test_integral_eval_app_equals_the_capi_pipeline(tmp_path, capi, ctx, synth, kind, scale):
    if not os.path.exists(EVAL_APP):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    text, case = EVAL_FEATURES[kind]
    frame = synth.make_frame(W, H, seed=20261020)
    s3 = _samples()
    samples = np.stack([s3[:, 0], s3[:, 1], s3[:, 2], np.rint(ASPECT * s3[:, 2]).astype(np.int32)], 1)
    mapped = hog_model.map_samples(samples, scale=float(scale))   # PatchResizingFeatureExtractor (scale != 1), then IntegralFeatureExtractor
    assert np.array_equal(mapped[:, 2:] > samples[:, 2:], np.ones((64, 2), bool))
    integral = capi.Integral(ctx)
    integral.update(frame)
    hp = capi_params(capi, case)
    feats, valid = integral.extract_hog(hp, mapped)
    nv = int(valid.sum())
    assert 30 <= nv < 64   # 52 at scale 1, 33 at scale 1.1: with and without a valid patch
    m = synth.make_svm_f32(3, feats[valid], nsv=48, gamma=0.5, positive_fraction=0.4)
    m["logistic_a"], m["logistic_b"] = 0.3, -1.7
    want_target, want_weight = integral.svm_evaluate_samples(capi.Svm(ctx, m), mapped, kind="hog", hog=hp)
    assert 0 < want_target.sum() < nv
    synth.save_svm_text(str(tmp_path / "svm.txt"), m)
    synth.save_pnm(str(tmp_path / "frame.ppm"), frame)
    (tmp_path / "eval.cfg").write_text(text % scale + "classifier\n{\n    classifierFile %s\n}\naspectRatio %s\n" % (tmp_path / "svm.txt", ASPECT))
    (tmp_path / "samples.txt").write_text("".join("%d %d %d\n" % tuple(r) for r in s3))
    r = subprocess.run([EVAL_APP, str(tmp_path / "eval.cfg"), str(tmp_path / "frame.ppm"), str(tmp_path / "samples.txt")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    # the wrappers are walked: one fd_integral_svm_evaluate_samples, no per-sample loop
    assert "64 samples: one fused device call" in r.stderr and "per-sample loop" not in r.stderr
    got = np.array([[float(v) for v in l.split()] for l in r.stdout.strip().splitlines()])
    assert got.shape == (64, 2)
    assert np.array_equal(got[:, 0].astype(bool), want_target)
    print("largest weight difference between the app and the capi pipeline: %.3g" % np.abs(got[:, 1] - want_weight).max())
    assert np.array_equal(got[:, 1], want_weight)
    assert not got[~valid].any()
    integral.close()


def pd_config(feature, around, symmetry, start=2):
    return """tracking {
  seed 7
  transition simple { positionDeviation 4 sizeDeviation 0.05 }
  adaptive { resampling { particleCount 60 randomRate 0.3 minSize 16 maxSize 60 } }
  initialCount 60
  measurement positionDependent {
    %s
    filter none  startFrameCount %d  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget %d  sampleAdditionalNegatives 6  sampleTestNegatives 5
    exploitSymmetry %d
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
}
""" % (feature, start, around, symmetry)


@pytest.mark.parametrize("around,symmetry", [(0, 0), (2, 1)], ids=["around0-sym0", "around2-sym1"])
def test_adapt_follows_the_restatement_on_the_default_ihog_block(capi, ctx, tmp_path, around, symmetry):
    paths, targets = make_frames(tmp_path)
    frames, particles = run_app(tmp_path, pd_config(DEFAULT_IHOG, around, symmetry), paths, targets)
    assert len(frames) == 4
    sel = selection_model.Selection(seed=7, start_frame_count=2, target_threshold=0.1, confidence_threshold=0.95, negatives_around_target=around,
                                    additional_negatives=6, test_negatives=5)
    hp = capi_params(capi, hog_model.DEFAULT)
    integral = capi.Integral(ctx)
    svm_model, retrainings = None, 0
    for f, (fr, path, target, ps) in enumerate(zip(frames, paths, targets, particles)):
        with open(path, "rb") as fh:
            integral.update(np.frombuffer(fh.read()[-PW * PH:], np.uint8).reshape(PH, PW))
        assert fr["usable_before"] == int(sel.usable)

        def has_window(x, y, w, h):
            return bool(capi.integral_gradient_samples_valid(PW, PH, 30, 30, hog_model.map_samples([(x, y, w, h)], scale=1.1))[0])

        def probability(x, y, w, h):
            return float(integral.svm_evaluate_samples(capi.Svm(ctx, svm_model), hog_model.map_samples([(x, y, w, h)], scale=1.1), hog=hp)[1][0])

        if sel.usable:   # the particle weights: one fused call on the classifier of the frame before
            mapped = hog_model.map_samples([(x, y, s, s) for x, y, s in ps], scale=1.1)
            target_flags, weights = integral.svm_evaluate_samples(capi.Svm(ctx, svm_model), mapped, hog=hp)
            assert [e[1] for e in fr["e"]] == weights.tolist() and [bool(e[0]) for e in fr["e"]] == target_flags.tolist()
            assert fr["fused"] > 0 and fr["loop"] == 0
            assert (weights > 0).any() and (weights == 0).any()   # particles with and without a valid patch
        else:
            assert all(e == (0, 1.0) for e in fr["e"])
        weighted = [(x, y, s, e[1]) for (x, y, s), e in zip(ps, fr["e"])]
        chosen = sel.adapt(PW, PH, weighted, target, has_window, probability)
        assert fr["adapt"] == int(chosen is not None) == fr["retrained"], (f, fr["adapt"])
        if chosen is not None:
            pos, neg, test = chosen
            assert fr["positives"] == pos and fr["negatives"] == neg and fr["tests"] == test, f
            assert len(pos) == 5 and len(neg) == {0: 0, 2: 18}[around] + 6 and len(test) == 5
            assert fr["vectors"] == sel.training_vectors(pos, neg, has_window, probability, bool(symmetry)), f
            retrainings += 1
        sel.usable = bool(fr["usable"])
        if fr["svm"]:
            svm_model = fr["svm"]
            assert svm_model["sv"].shape[1] == svm_model["dim"] == capi.integral_hog_feature_length(hp) == 225
    assert frames[0]["adapt"] == 0 and frames[1]["adapt"] == 1 and frames[1]["usable"] == 1   # startFrameCount 2
    assert retrainings >= 2 and frames[2]["usable_before"] == 1
    integral.close()


HAAR = 'feature haar { sizes "0.2 0.4" gridRows 5 gridCols 5 types "2rect 3rect 4rect center-surround" scale 1 }'


@pytest.mark.parametrize("feature", [DEFAULT_IHOG, HAAR], ids=["ihog", "haar"])
def test_tracker_app_runs_integral_features(tmp_path, feature):
    paths, targets = make_frames(tmp_path)
    out = tracker_run(tmp_path, pd_config(feature, 2, 0, start=1), paths, targets[0])
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("init 1 ")
    assert len([l for l in lines if l.startswith("frame ")]) == 3
