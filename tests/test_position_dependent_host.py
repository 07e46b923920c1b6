"""condensation::PositionDependentMeasurementModel through position_dependent_eval_app and tracker_app: the samples every adapt
chooses, the retrain counts and the usable flags against the restatement in tests/pyramid_samples_model.py, the particle weights
against capi.hist_svm_evaluate_samples on the classifier the app reports, and which route SingleClassifierModel took."""
import math
import os
import subprocess

import numpy as np
import pytest

import pyramid_samples_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "position_dependent_eval_app")
TRACKER = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
W, H = 96, 80
PATCH = 16

FEATURES = {
    "hog": """feature hog { pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }
                gradientKernel 3 blurKernel 0 bins 9 signed 0 interpolate 0
                histogram spatial { cellSize 8 blockSize 2 interpolate 0 signedAndUnsigned 0 concatenate 0 normalization l2hys } }""",
    "glbp": """feature glbp { pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }
                gradientKernel 3 blurKernel 3 type lbp8uniform
                histogram spatial { cellSize 8 blockSize 1 interpolate 0 concatenate 0 normalization l2hys } }""",
    "ehog": """feature ehog { pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }
                gradientKernel 3 blurKernel 0 bins 8 signed 1 interpolate 0
                histogram { cellSize 4 interpolate 0 signedAndUnsigned 1 alpha 0.2 } }""",
}


def config_text(feature, around, symmetry, start=2, wrapped=0, filter_="none", print_vectors=0):
    return """tracking {
  seed 7
  transition simple { positionDeviation 4 sizeDeviation 0.05 }
  adaptive { resampling { particleCount 60 randomRate 0.3 minSize 16 maxSize 60 } }
  initialCount 60
  measurement positionDependent {
    %s
    filter %s  wrapped %d  printVectors %d  startFrameCount %d  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget %d  sampleAdditionalNegatives 6  sampleTestNegatives 5
    exploitSymmetry %d
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
}
""" % (FEATURES[feature], filter_, wrapped, print_vectors, start, around, symmetry)


def make_frames(tmp_path):
    """four 96 x 80 gray frames: noise plus a ramp, and a striped blob that moves two pixels a frame"""
    rng = np.random.default_rng(20261020)
    yy, xx = np.mgrid[0:H, 0:W]
    back = 60.0 + 0.8 * xx + 0.5 * yy + rng.normal(0, 12, (H, W))
    paths, targets = [], []
    for f in range(4):
        cx, cy, size = 44 + 2 * f, 38 + f, 26
        img = back + rng.normal(0, 4, (H, W))
        inside = (np.abs(xx - cx) <= size // 2) & (np.abs(yy - cy) <= size // 2)
        img[inside] = 120 + 90 * np.sin((xx[inside] - cx) * 0.9) * np.cos((yy[inside] - cy) * 0.5)
        img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        p = tmp_path / ("frame%d.pgm" % f)
        with open(p, "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H))
            fh.write(img.tobytes())
        paths.append(str(p))
        targets.append((cx, cy, size))
    return paths, targets


def make_particles(target, rng):
    tx, ty, ts = target
    near = [(tx + int(dx), ty + int(dy), max(14, ts + int(ds))) for dx, dy, ds in rng.integers(-6, 7, (24, 3))]
    far = [(int(x), int(y), int(s)) for x, y, s in zip(rng.integers(12, W - 12, 20), rng.integers(12, H - 12, 20), rng.integers(14, 48, 20))]
    return near + far + [(tx, ty, ts), (3, 3, 20), (W - 2, H - 2, 30)]


def run_app(tmp_path, cfg, paths, targets):
    rng = np.random.default_rng(5)
    cfg_path = tmp_path / "pd.cfg"
    cfg_path.write_text(cfg)
    particles = [make_particles(t, rng) for t in targets]
    lines = []
    for path, t, ps in zip(paths, targets, particles):
        lines.append("frame %s %d %d %d %d" % (path, t[0], t[1], t[2], len(ps)))
        lines += ["%d %d %d" % p for p in ps]
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    out = subprocess.run([APP, str(cfg_path), str(script)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return parse(out.stdout), particles


def parse(text):
    frames, cur, group = [], None, None
    for line in text.splitlines():
        t = line.split()
        if t[0] == "frame":
            cur = dict(usable_before=int(t[3]), fused=int(t[7]), loop=int(t[9]), e=[], svm=None, pv=[])
            frames.append(cur)
        elif t[0] == "e":
            cur["e"].append((int(t[1]), float(t[2])))
        elif t[0] == "adapt":
            cur.update(adapt=int(t[1]), usable=int(t[3]), retrained=int(t[5]))
        elif t[0] in ("positives", "negatives", "tests"):
            group = cur[t[0]] = []
        elif t[0] == "s":
            group.append((int(t[1]), int(t[2]), int(t[3])))
        elif t[0] == "vectors":
            cur["vectors"] = (int(t[1]), int(t[2]))
        elif t[0] == "pv":
            cur["pv"].append(np.array(t[3:], np.float32).reshape(int(t[1]), int(t[2])))
        elif t[0] == "svm":
            cur["svm"] = dict(kernel=0, dtype=1, sv=[], coeff=[], bias=np.float32(t[4]), threshold=float(t[6]), logistic_a=float(t[8]),
                              logistic_b=float(t[9]), dim=int(t[2]))
        elif t[0] == "sv":
            cur["svm"]["coeff"].append(np.float32(t[1]))
            cur["svm"]["sv"].append(np.array(t[2:], np.float32))
    for f in frames:
        if f["svm"]:
            f["svm"]["sv"] = np.stack(f["svm"]["sv"])
            f["svm"]["coeff"] = np.array(f["svm"]["coeff"], np.float32)
    return frames


def python_side(capi, ctx, feature, frame_path):
    """the app's pyramid and patch filter through capi (createPyramidExtractor's scale range, HeadTracking's filter choice)"""
    inc = math.pow(0.5, 1.0 / 3)
    lo, hi = 16.0 / 64, 16.0 / 16
    max_index, min_index = model.cv_round(math.log(lo) / math.log(inc)), model.cv_round(math.log(hi) / math.log(inc))
    p = capi.Pyramid(ctx, 3, math.pow(inc, max_index), math.pow(inc, min_index))
    if feature == "hog":
        p.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9, grad_kernel=3)
        hp = capi.hist_params(0, PATCH, PATCH, 1, 1, bins=9, cell=8, block=2, normalization=2)
    else:
        p.set_layer_filter(capi.FD_LAYER_GRADMAG_LBP, grad_kernel=3, lbp_type=1, blur_kernel=3)
        hp = capi.hist_params(1, PATCH, PATCH, 1, 1, bins=59, cell=8, block=1, normalization=2)
    with open(frame_path, "rb") as fh:
        data = fh.read()
    p.update(np.frombuffer(data[-W * H:], np.uint8).reshape(H, W))
    return p, hp


CASES = [("hog", 0, 0), ("hog", 1, 1), ("glbp", 2, 0), ("glbp", 3, 1)]


@pytest.mark.parametrize("feature,around,symmetry", CASES, ids=["%s-around%d-sym%d" % c for c in CASES])
def test_adapt_follows_the_restatement(capi, ctx, tmp_path, feature, around, symmetry):
    paths, targets = make_frames(tmp_path)
    frames, particles = run_app(tmp_path, config_text(feature, around, symmetry), paths, targets)
    assert len(frames) == 4
    sel = model.Selection(seed=7, start_frame_count=2, target_threshold=0.1, confidence_threshold=0.95, negatives_around_target=around,
                          additional_negatives=6, test_negatives=5)
    svm_model, retrainings = None, 0
    for f, (fr, path, target, ps) in enumerate(zip(frames, paths, targets, particles)):
        pyr, hp = python_side(capi, ctx, feature, path)
        layers = pyr.layers()
        assert fr["usable_before"] == int(sel.usable)

        def has_window(x, y, w, h):
            return bool(model.sample_windows(layers, pyr.inc, PATCH, PATCH, [(x, y, w, h)])[0, 3])

        def probability(x, y, w, h):
            return float(capi.hist_svm_evaluate_samples(ctx, pyr, hp, capi.Svm(ctx, svm_model), [(x, y, w, h)])[1][0])

        # the particle weights: one fused call on the classifier of the frame before
        if sel.usable:
            xywh = [(x, y, s, s) for x, y, s in ps]
            target_flags, weights = capi.hist_svm_evaluate_samples(ctx, pyr, hp, capi.Svm(ctx, svm_model), xywh)
            assert [e[1] for e in fr["e"]] == weights.tolist() and [bool(e[0]) for e in fr["e"]] == target_flags.tolist()
            assert fr["fused"] > 0 and fr["loop"] == 0
            assert (weights > 0).any() and (weights == 0).any()   # particles with and without a window
        else:
            assert all(e == (0, 1.0) for e in fr["e"])
        weighted = [(x, y, s, e[1]) for (x, y, s), e in zip(ps, fr["e"])]
        chosen = sel.adapt(W, H, weighted, target, has_window, probability)
        assert fr["adapt"] == int(chosen is not None) == fr["retrained"], (f, fr["adapt"])
        if chosen is not None:
            pos, neg, test = chosen
            assert fr["positives"] == pos and fr["negatives"] == neg and fr["tests"] == test, f
            assert len(pos) == 5 and len(neg) == {0: 0, 1: 6, 2: 18, 3: 26}[around] + 6 and len(test) == 5
            assert fr["vectors"] == sel.training_vectors(pos, neg, has_window, probability, bool(symmetry)), f
            retrainings += 1
        sel.usable = bool(fr["usable"])
        if fr["svm"]:
            svm_model = fr["svm"]
            assert svm_model["sv"].shape[1] == svm_model["dim"] == capi.lib().fd_hist_feature_length(hp, 2 if feature == "hog" else 1)
    assert frames[0]["adapt"] == 0 and frames[1]["adapt"] == 1 and frames[1]["usable"] == 1   # startFrameCount 2
    assert retrainings >= 2 and frames[2]["usable_before"] == 1


def test_wrapped_extractor_keeps_the_loop(capi, ctx, tmp_path):
    """behind a PatchResizingFeatureExtractor SingleClassifierModel scores sample by sample: same choices, same weights up to the
    last bits of a one-row scoring launch"""
    paths, targets = make_frames(tmp_path)
    fused, particles = run_app(tmp_path, config_text("hog", 1, 0), paths, targets)
    loop, _ = run_app(tmp_path, config_text("hog", 1, 0, wrapped=1), paths, targets)
    assert any(f["usable_before"] for f in loop)
    for a, b in zip(fused, loop):
        assert b["fused"] == 0 and a["loop"] == 0
        assert b["usable_before"] == a["usable_before"] and (not b["usable_before"] or b["loop"] > 0)
        assert [e[0] for e in a["e"]] == [e[0] for e in b["e"]]
        assert np.allclose([e[1] for e in a["e"]], [e[1] for e in b["e"]], rtol=1e-9, atol=0)
        for key in ("positives", "negatives", "tests", "vectors", "adapt", "usable"):
            assert a.get(key) == b.get(key), key
    assert fused[-1]["fused"] > 0


@pytest.mark.parametrize("wrapped", [0, 1], ids=["direct", "wrapped"])
def test_ehog_symmetry_mirrors_cells_not_floats(capi, ctx, tmp_path, wrapped):
    """exploitSymmetry on the ehog feature type: the reference flips a rows x cols Mat of 8 + 4 + 4 channels, so the mirrored vector has
    the cells of every row in reverse order and each cell's 16 values as they were (bins, unsigned halves, energies stay in place)"""
    paths, targets = make_frames(tmp_path)
    frames, _ = run_app(tmp_path, config_text("ehog", 1, 1, start=1, wrapped=wrapped, print_vectors=1), paths[:2], targets[:2])
    fr = frames[0]
    assert fr["adapt"] == 1 and fr["vectors"][0] == 10 == len(fr["pv"])
    # the unmirrored vectors are the extractor's: ehog_extract_samples on the same layers
    inc = math.pow(0.5, 1.0 / 3)
    p = capi.Pyramid(ctx, 3, math.pow(inc, 6), math.pow(inc, 0))
    p.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=8, signed_gradients=True, grad_kernel=3)
    with open(paths[0], "rb") as fh:
        p.update(np.frombuffer(fh.read()[-W * H:], np.uint8).reshape(H, W))
    ep = capi.ehog_patch_params(PATCH, PATCH, bins=8, cell_w=4, signed_and_unsigned=True, alpha=0.2)
    feats, valid = capi.ehog_extract_samples(ctx, p, ep, [(x, y, s, s) for x, y, s in fr["positives"]])
    assert valid.all()
    D, rows, cols = 8 + 4 + 4, 4, 4
    for k in range(5):
        plain, mirrored = fr["pv"][2 * k], fr["pv"][2 * k + 1]
        assert plain.shape == mirrored.shape == (rows, cols * D)
        assert np.array_equal(plain.reshape(-1), feats[k])
        cells = plain.reshape(rows, cols, D)
        assert np.array_equal(mirrored.reshape(rows, cols, D), cells[:, ::-1, :])
        assert not np.array_equal(mirrored, plain[:, ::-1])   # not the float-by-float flip


def tracker_run(tmp_path, cfg, paths, target):
    cfg_path = tmp_path / "tracker.cfg"
    cfg_path.write_text(cfg)
    x, y, s = target
    return subprocess.run([TRACKER, str(cfg_path), str(x - s // 2), str(y - s // 2), str(s), str(s)] + paths, capture_output=True, text=True, timeout=120)


def test_tracker_app_runs_a_position_dependent_config(tmp_path):
    paths, targets = make_frames(tmp_path)
    out = tracker_run(tmp_path, config_text("hog", 2, 0, start=1), paths, targets[0])
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("init 1 ")
    frames = [l for l in lines if l.startswith("frame ")]
    assert len(frames) == 3 and all(" route generic " in l for l in frames)


def test_tracker_app_names_what_is_not_built(tmp_path):
    paths, targets = make_frames(tmp_path)
    out = tracker_run(tmp_path, config_text("hog", 0, 0, start=1, filter_="before"), paths, targets[0])
    assert out.returncode == 1 and "filter before" in out.stderr and "FilteringClassifierModel" in out.stderr
