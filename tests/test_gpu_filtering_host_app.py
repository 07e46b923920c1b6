"""condensation::FilteringClassifierModel and ClassificationBasedStateValidator through filtering_eval_app and tracker_app: targets and
weights of `filter before`, `filter after` and `filter none` against a restatement composed from capi.patch_rvm_evaluate_samples and
capi.hist_svm_evaluate_samples, the routes the counters report, the validator's candidates and verdicts, and the tracker configs that
use them."""
import math
import os
import subprocess

import numpy as np
import pytest

import pyramid_samples_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "filtering_eval_app")
TRACKER = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
W, H = 96, 80
PATCH = 16
SIZES, DISPLACEMENTS = (0.9, 1.0, 1.1), (-0.1, 0.0, 0.1)

PYRAMID = "pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }"
HOG = """feature hog { %s
                gradientKernel 3 blurKernel 0 bins 9 signed 0 interpolate 0
                histogram spatial { cellSize 8 blockSize 2 interpolate 0 signedAndUnsigned 0 concatenate 0 normalization l2hys } }""" % PYRAMID


def make_frames(tmp_path):
    """four 96 x 80 gray frames: noise plus a ramp, and a striped blob that moves two pixels a frame (the generator of
    tests/test_position_dependent_host.py)"""
    rng = np.random.default_rng(20261020)
    yy, xx = np.mgrid[0:H, 0:W]
    back = 60.0 + 0.8 * xx + 0.5 * yy + rng.normal(0, 12, (H, W))
    paths, targets, images = [], [], []
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
        images.append(img)
    return paths, targets, images


def make_particles(target, rng):
    tx, ty, ts = target
    near = [(tx + int(dx), ty + int(dy), max(14, ts + int(ds))) for dx, dy, ds in rng.integers(-6, 7, (24, 3))]
    far = [(int(x), int(y), int(s)) for x, y, s in zip(rng.integers(12, W - 12, 20), rng.integers(12, H - 12, 20), rng.integers(14, 48, 20))]
    return near + far + [(tx, ty, ts), (3, 3, 20), (W - 2, H - 2, 30)]


def pyramids(capi, ctx):
    """the app's two pyramids through capi (createPyramidExtractor's scale range): gray for the filter and the validator (feature h),
    gradient bins for the inner model (feature hog)"""
    inc = math.pow(0.5, 1.0 / 3)
    lo, hi = 16.0 / 64, 16.0 / 16
    max_index, min_index = model.cv_round(math.log(lo) / math.log(inc)), model.cv_round(math.log(hi) / math.log(inc))
    gray = capi.Pyramid(ctx, 3, math.pow(inc, max_index), math.pow(inc, min_index))
    bins = capi.Pyramid(ctx, 3, math.pow(inc, max_index), math.pow(inc, min_index))
    bins.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9, grad_kernel=3)
    return gray, bins


def candidates(target):
    """ClassificationBasedStateValidator.cpp:28-45: sizes x displacements x displacements, std::round"""
    tx, ty, ts = target
    out = []
    for factor in SIZES:
        size = model.lround(factor * ts)
        for dx in DISPLACEMENTS:
            x = tx + model.lround(dx * size)
            for dy in DISPLACEMENTS:
                out.append((x, ty + model.lround(dy * size), size))
    return out


@pytest.fixture(scope="module")
def scene(capi, ctx, synth, tmp_path_factory):
    """frames, particles, the two classifiers of the measurement model and the validator's RVM, built once"""
    tmp = tmp_path_factory.mktemp("filtering")
    paths, targets, images = make_frames(tmp)
    rng = np.random.default_rng(5)
    particles = [make_particles(t, rng) for t in targets]
    gray, bins = pyramids(capi, ctx)
    pp = capi.patch_samples_params(PATCH, PATCH, capi.FD_FEATURE_HISTEQ, 1.0 / 127.5, -1.0)     # feature h
    hp = capi.hist_params(0, PATCH, PATCH, 1, 1, bins=9, cell=8, block=2, normalization=2)
    # training vectors: a grid of square samples over frame 0
    grid = [(x, y, s, s) for s in (16, 20, 26, 32, 40) for y in range(s // 2, H - s // 2, 7) for x in range(s // 2, W - s // 2, 7)]
    gray.update(images[0])
    bins.update(images[0])
    hfeats, hvalid = capi.patch_extract_samples(ctx, gray, pp, grid)
    gfeats, gvalid = capi.hist_extract_samples(ctx, bins, hp, grid)
    assert hvalid.sum() > 200 and gvalid.sum() > 200
    rvm = synth.make_rvm(21, hfeats[hvalid], PATCH, PATCH, n_filters=12, kernel=2, pass_rate=0.8, min_survivors=40)
    synth.save_rvm(str(tmp / "filter.rvm"), rvm)
    svm = synth.make_svm_f32(9, gfeats[gvalid], nsv=24, gamma=0.5, positive_fraction=0.5, kernel=2)
    svm["logistic_a"], svm["logistic_b"] = 0.3, -1.7
    synth.save_svm_text(str(tmp / "svm.txt"), svm)
    # the validator's RVM: three levels, the first two pass everything, the last threshold chosen on the candidates' distances so that
    # one frame is valid through a single candidate and another frame through none
    vrvm = synth.make_rvm(22, hfeats[hvalid], PATCH, PATCH, n_filters=3, kernel=2, pass_rate=0.8, min_survivors=40)
    vrvm["thresholds"] = np.full(3, -1e30, np.float32)
    open_rvm = capi.Rvm(ctx, vrvm)
    tops = []
    for img, t in zip(images, targets):
        gray.update(img)
        valid, level, dist, _ = capi.patch_rvm_evaluate_samples(ctx, gray, pp, open_rvm, [(x, y, s, s) for x, y, s in candidates(t)])
        assert valid.sum() >= 9 and np.all(level[valid] == 2)
        tops.append(np.sort(dist[valid])[::-1][:2])
    open_rvm.close()
    best = int(np.argmax([t[0] for t in tops]))
    lowest = min(t[0] for i, t in enumerate(tops) if i != best)
    floor = max(tops[best][1], lowest)
    assert floor < tops[best][0]
    vrvm["thresholds"][2] = np.float32(0.5 * (floor + tops[best][0]))
    assert floor < np.float64(vrvm["thresholds"][2]) < tops[best][0]
    synth.save_rvm(str(tmp / "validator.rvm"), vrvm)
    return dict(tmp=tmp, paths=paths, targets=targets, images=images, particles=particles, gray=gray, bins=bins, pp=pp, hp=hp, rvm=rvm, svm=svm, vrvm=vrvm,
                best=best)


def eval_config(scene, wrapped):
    tmp = scene["tmp"]
    return """tracking {
  measurement positionDependent {
    %s
    classifier { classifierFile %s }
    filter before { classifierFile %s feature h { %s } }
    wrapped %d
  }
  validator rvm { classifierFile %s feature h { %s } sizes "0.9 1 1.1" displacements "-0.1 0 0.1" }
}
""" % (HOG, tmp / "svm.txt", tmp / "filter.rvm", PYRAMID, wrapped, tmp / "validator.rvm", PYRAMID)


def run_app(scene, wrapped):
    tmp = scene["tmp"]
    cfg = tmp / ("eval%d.cfg" % wrapped)
    cfg.write_text(eval_config(scene, wrapped))
    lines = []
    for path, t, ps in zip(scene["paths"], scene["targets"], scene["particles"]):
        lines.append("frame %s %d %d %d %d" % (path, t[0], t[1], t[2], len(ps)))
        lines += ["%d %d %d" % p for p in ps]
    script = tmp / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    out = subprocess.run([APP, str(cfg), str(script)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    frames, counters = [], None
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "frame":
            frames.append(dict(e=[], c=[], valid=None))
        elif t[0] == "e":
            frames[-1]["e"].append((int(t[1]), float(t[2]), int(t[3]), float(t[4]), int(t[5]), float(t[6])))
        elif t[0] == "validator":
            frames[-1]["valid"] = int(t[1])
            frames[-1]["n"] = int(t[3])
        elif t[0] == "c":
            frames[-1]["c"].append((int(t[1]), int(t[2]), int(t[3])))
        elif t[0] == "counters":
            counters = dict(before=(int(t[3]), int(t[5])), after=(int(t[8]), int(t[10])), validator=(int(t[13]), int(t[15])))
    return frames, counters


def restatement(capi, ctx, scene):
    """per frame: (before target, before weight, after target, after weight, none target, none weight), validator verdict, candidates"""
    rvm, svm, vrvm = capi.Rvm(ctx, scene["rvm"]), capi.Svm(ctx, scene["svm"]), capi.Rvm(ctx, scene["vrvm"])
    gray, bins, pp, hp = scene["gray"], scene["bins"], scene["pp"], scene["hp"]
    out = []
    for img, t, ps in zip(scene["images"], scene["targets"], scene["particles"]):
        gray.update(img)
        bins.update(img)
        xywh = np.array([(x, y, s, s) for x, y, s in ps], np.int32)
        _, _, _, passes = capi.patch_rvm_evaluate_samples(ctx, gray, pp, rvm, xywh)
        none_t, none_w = capi.hist_svm_evaluate_samples(ctx, bins, hp, svm, xywh)
        # before: the inner model sees the passing samples only (one call on that subset, as the app makes it)
        before_t, before_w = np.zeros(len(ps), bool), np.zeros(len(ps))
        if passes.any():
            before_t[passes], before_w[passes] = capi.hist_svm_evaluate_samples(ctx, bins, hp, svm, xywh[passes])
        # after: the inner model on all samples, the filter on those it marked
        after_t = none_t.copy()
        if none_t.any():
            after_t[none_t] = capi.patch_rvm_evaluate_samples(ctx, gray, pp, rvm, xywh[none_t])[3]
        cand = candidates(t)
        accepted = capi.patch_rvm_evaluate_samples(ctx, gray, pp, vrvm, [(x, y, s, s) for x, y, s in cand])[3]
        out.append(dict(e=(before_t, before_w, after_t, none_w, none_t, none_w), passes=passes, accepted=accepted, c=cand))
    for h in (rvm, svm, vrvm):
        h.close()
    return out


def test_filter_and_validator_follow_the_restatement(capi, ctx, scene):
    frames, counters = run_app(scene, 0)
    want = restatement(capi, ctx, scene)
    assert len(frames) == len(want) == 4
    verdicts = []
    for fr, w in zip(frames, want):
        got = list(zip(*fr["e"]))
        for k in (0, 2, 4):
            assert [bool(v) for v in got[k]] == w["e"][k].tolist(), k
            assert list(got[k + 1]) == w["e"][k + 1].tolist(), k
        assert fr["c"] == w["c"] and fr["n"] == 27
        assert fr["valid"] == int(w["accepted"].any())
        verdicts.append(int(w["accepted"].sum()))
    # the filter bites: it rejects samples the inner model accepts, and passes others
    passes = np.concatenate([w["passes"] for w in want])
    none_t = np.concatenate([w["e"][4] for w in want])
    assert (passes & none_t).any() and (~passes & none_t).any() and (passes & ~none_t).any()
    assert verdicts[scene["best"]] == 1 and 0 in verdicts     # valid through a single candidate; invalid
    assert counters["before"] == (4, 0) and counters["after"] == (4, 0) and counters["validator"] == (4, 0)


def test_wrapped_extractors_take_the_loops(capi, ctx, scene):
    """behind PatchResizingFeatureExtractor(.., 1) every route is the per-sample one: the same verdicts, the same weights up to the last
    bits of a one-row scoring launch"""
    fused, _ = run_app(scene, 0)
    loop, counters = run_app(scene, 1)
    assert counters["before"] == (0, 4) and counters["after"] == (0, 4) and counters["validator"] == (0, 4)
    for a, b in zip(fused, loop):
        ga, gb = list(zip(*a["e"])), list(zip(*b["e"]))
        for k in (0, 2, 4):
            assert ga[k] == gb[k]
            assert np.allclose(ga[k + 1], gb[k + 1], rtol=1e-9, atol=0)
        assert a["valid"] == b["valid"] and a["c"] == b["c"]


# ---- tracker_app
def tracker_config(scene, feature=HOG, filter_="filter none", validator=""):
    return """tracking {
  seed 7
  transition simple { positionDeviation 4 sizeDeviation 0.05 }
  adaptive { resampling { particleCount 60 randomRate 0.3 minSize 16 maxSize 60 } }
  initialCount 60
  measurement positionDependent {
    %s
    %s  startFrameCount 1  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget 2  sampleAdditionalNegatives 6  sampleTestNegatives 5
    exploitSymmetry 0
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
  %s
}
""" % (feature, filter_, validator)


def tracker_run(scene, cfg, name):
    cfg_path = scene["tmp"] / name
    cfg_path.write_text(cfg)
    x, y, s = scene["targets"][0]
    return subprocess.run([TRACKER, str(cfg_path), str(x - s // 2), str(y - s // 2), str(s), str(s)] + scene["paths"], capture_output=True, text=True,
                          timeout=120)


def tracker_cases(scene):
    tmp = scene["tmp"]
    block = "{ classifierFile %s feature h { %s } }" % (tmp / "filter.rvm", PYRAMID)
    open_validator = 'validator rvm { classifierFile %s numFiltersToUse 2 feature h { %s } sizes "0.9 1 1.1" displacements "-0.1 0 0.1" }' % (
        tmp / "validator.rvm", PYRAMID)
    return {"before": dict(filter_="filter before " + block), "after": dict(filter_="filter after " + block),
            "validator": dict(validator=open_validator), "grayscale": dict(feature="feature grayscale { %s }" % PYRAMID),
            "whi": dict(feature="feature whi { %s }" % PYRAMID, filter_="filter before " + block)}


@pytest.mark.parametrize("name", ["before", "after", "validator", "grayscale", "whi"])
def test_tracker_app_runs(scene, name):
    out = tracker_run(scene, tracker_config(scene, **tracker_cases(scene)[name]), name + ".cfg")
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("init 1 ")
    assert len([l for l in lines if l.startswith("frame ")]) == 3


@pytest.mark.parametrize("feature,names", [("feature histeq { %s }" % PYRAMID, ("histeq",)),
                                            ("feature h { pyramid derived { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 } }",
                                             ("pyramid derived",))], ids=["histeq", "derived"])
def test_tracker_app_names_what_it_refuses(scene, feature, names):
    out = tracker_run(scene, tracker_config(scene, feature=feature), "refused.cfg")
    assert out.returncode == 1 and all(n in out.stderr for n in names), out.stderr
