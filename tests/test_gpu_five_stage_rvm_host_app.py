"""ffp_detect_app with a fiveStageCascade node whose firstClassifier / secondClassifier values select other loaders than pwvm / psvm
(FaceFrontal.cfg:5: "pwvm | prvm | psvm"): FiveStageSlidingWindowDetector's fused RVM path (fd_detect_five_stage_rvm), the reference's own
per-patch composition for what no fused path serves, and the unchanged default.  Expected boxes: the oracle composition of
test_gpu_five_stage_rvm.py."""
import os

import numpy as np
import pytest

import test_gpu_five_stage_rvm as T
from test_gpu_host_apps import FACE_CFG, PKG, _read_patches, _run

pytestmark = pytest.mark.gpu

PW = PH = 20
CONV = 0.25   # conversionFilter "5 0.25": CV_32F, scaling 0.25
CFG = """detectors
{
    Face
    {
        landmark "face"
        type fiveStageCascade
        feature hq64
        patchFilter
        {
            conversionFilter "5 0.25"
        }
        firstClassifier %s
        {
            classifierFile %s
            logisticA 0.4
            logisticB -2.0
        }
        secondClassifier %s
        {
            classifierFile %s
        }
        pyramid
        {
            minScaleFactor %s
            maxScaleFactor 0.4
            incrementalScaleFactor 0.7071
            patch
            {
                width 20
                height 20
            }
        }
        overlapElimination
        {
            dist 5.0
            ratio 0.0
        }
    }
}
"""


def app_path():
    app = os.path.join(PKG, "ffp_detect_app")
    if not os.path.exists(app):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    return app


def app_scene(oracle, frame640, min_scale):
    """windows (step 1, as the app's SlidingWindowDetector) and hq64 * 0.25 feature rows of the 320 x 240 crop"""
    small = np.ascontiguousarray(frame640[:240, :320])
    po = oracle.Pyramid(inc=float(np.float32(0.7071)), min_scale=float(np.float32(min_scale)), max_scale=float(np.float32(0.4)))
    po.update(small)
    layers = [po.layer(i) for i in range(len(po.layers()))]
    wins = po.windows(PW, PH, 1, 1)
    pat = np.stack([oracle.histeq64(np.ascontiguousarray(layers[lp][ly:ly + PH, lx:lx + PW])) for lp, lx, ly, *_ in wins])
    feats = pat.reshape(len(pat), -1).astype(np.float32) * np.float32(CONV)
    return small, po, wins, feats


def boxes(out):
    got = [l.split() for l in out.strip().splitlines()]
    assert all(g[0] == "Face" and g[1] == "face" and float(g[6]) == 0.5 for g in got)
    return sorted(tuple(int(v) for v in g[2:6]) for g in got)


def box_of(q):   # Patch::getBounds (Patch.hpp:28-35)
    return (int(q["cx"]) - int(q["w"]) // 2, int(q["cy"]) - int(q["h"]) // 2, int(q["w"]), int(q["h"]))


def expected_boxes(exp):
    """the printed boxes: one second-stage positive per maximum (any of those that share its centre: all have probability 0.5)"""
    by_centre = {}
    for q in exp["pos2"]:
        by_centre.setdefault((int(q["cx"]), int(q["cy"])), set()).add(box_of(q))
    if exp["maxima"] is None:
        return None, by_centre
    return exp["maxima"], by_centre


def check_boxes(got, exp):
    maxima, by_centre = expected_boxes(exp)
    assert len(got) == exp["stages"][3] > 0
    if maxima is None:
        assert got == sorted(b for s in by_centre.values() for b in s)
        return
    centres = sorted((x + w // 2, y + h // 2) for x, y, w, h in got)
    assert centres == maxima
    for b in got:
        assert b in by_centre[(b[0] + b[2] // 2, b[1] + b[3] // 2)]


@pytest.mark.parametrize("second", ["psvm", "prvm"])
def test_first_classifier_prvm_runs_the_fused_path(tmp_path, oracle, synth, frame640, second):
    app = app_path()
    small, po, wins, feats = app_scene(oracle, frame640, 0.2)
    rvm = synth.make_rvm(12, feats[::4], PW, PH, n_filters=20, kernel=2)
    rvm["logistic_a"], rvm["logistic_b"] = 0.4, -2.0
    synth.save_rvm(str(tmp_path / "first.fdrvm"), rvm)
    if second == "psvm":
        m2 = synth.make_svm_f32(PRVM_PSVM_SEED, feats[1::4], nsv=128, gamma=rvm["p0"], positive_fraction=0.3, kernel=2)
        synth.save_svm_text(str(tmp_path / "second.model"), m2, rows=PH, cols=PW)
    else:
        m2 = synth.make_rvm(PRVM_PRVM_SEED, feats[2::4], PW, PH, n_filters=12, pass_rate=PRVM_PRVM_PASS)
        synth.save_rvm(str(tmp_path / "second.model"), m2)
    exp = T.expected(oracle, rvm, m2, wins, feats, po.img_w, po.img_h)
    synth.save_pnm(str(tmp_path / "frame.ppm"), small)
    (tmp_path / "c.cfg").write_text(CFG % ("prvm", tmp_path / "first.fdrvm", second, tmp_path / "second.model", "0.2"))
    out = _run([app, str(tmp_path / "c.cfg"), str(tmp_path / "frame.ppm")])
    got = boxes(out)
    check_boxes(got, exp)
    # keepPatchData(true) works on this path as on the WVM path: every returned patch carries the converted HistEq64 cut
    out2 = _run([app, "--patches", str(tmp_path / "patches.bin"), str(tmp_path / "c.cfg"), str(tmp_path / "frame.ppm")])
    assert out2 == out
    patches = _read_patches(str(tmp_path / "patches.bin"))
    lines = [tuple(int(v) for v in l.split()[2:6]) for l in out.strip().splitlines()]
    assert len(patches) == len(lines)
    rows = {box_of(dict(zip(("layer", "lx", "ly", "cx", "cy", "w", "h"), w))): i for i, w in enumerate(wins)}
    for pt, b in zip(patches, lines):
        assert pt.dtype == np.float32 and np.array_equal(pt, feats[rows[b]].reshape(PH, PW))
    po.close()


# chosen on the CPU so that every stage is thinner than the one before and no survivor lies within the tolerance of the second threshold
PRVM_PSVM_SEED = 9
PRVM_PRVM_SEED, PRVM_PRVM_PASS = 22, 0.9


def first_svm_model(synth, feats, seed):
    """A small f32 RBF SVM as first stage: eight support vectors keep sum |coefficient|, hence the tolerance test_svm_distance_batch grants
    its distances, small against the gaps between the few positives' probabilities."""
    gamma = float(np.float32(1.0 / np.median(((feats[:200, None, :].astype(np.float64) - feats[None, 200:208, :]) ** 2).sum(-1))))
    m = synth.make_svm_f32(seed, feats[::4], nsv=8, gamma=gamma, positive_fraction=0.006, kernel=2)
    m["logistic_a"], m["logistic_b"] = 0.4, -2.0
    return m


def test_a_composition_without_a_fused_path_is_composed_per_patch(tmp_path, oracle, synth, frame640):
    """firstClassifier psvm (f32, on the converted HistEq64 patch) with secondClassifier prvm: no fused path serves it, so the detector runs
    SlidingWindowDetector::detect with patch data, OverlapElimination::eliminate and one classify() per survivor, then the block NMS."""
    app = app_path()
    small, po, wins, feats = app_scene(oracle, frame640, 0.3)
    m1 = first_svm_model(synth, feats, PSVM_FIRST_SEED)
    so = oracle.Svm(m1)
    d1 = so.distance(feats)
    tol1 = T.svm_tolerance(m1, d1)
    assert np.all(np.abs(d1 - m1["threshold"]) > tol1), "a window lies within the f32 tolerance of the first threshold: choose another seed"
    pos = np.nonzero(d1 >= m1["threshold"])[0]
    dets = np.zeros(len(pos), oracle.DET_DTYPE)
    for q, i in zip(dets, pos):
        q["layer"], q["lx"], q["ly"], q["cx"], q["cy"], q["w"], q["h"] = (int(v) for v in wins[i])
        q["positive"], q["fout"], q["prob"] = 1, np.float32(d1[i]), so.probability(d1[i])
    # the device's probabilities follow its distances: |dp| <= |logisticB| / 4 * |dd|; the order of the overlap elimination is fixed when
    # the oracle's probabilities are further apart than twice that
    perr = abs(m1["logistic_b"]) / 4 * tol1[pos].max()
    assert np.diff(np.sort(dets["prob"])).min() > 2 * perr + 1e-9, "two first-stage probabilities too close: choose another seed"
    keep = oracle.overlap_elimination(dets, 5.0, 0.0)
    m2 = synth.make_rvm(21, feats[2::4], PW, PH, n_filters=12, pass_rate=PSVM_PRVM_PASS)
    passes, d2, tol2, thr2, reached = T.second_stage(oracle, m2, feats[pos[keep]])
    assert np.all(~reached | (np.abs(d2 - thr2) > tol2))
    pos2 = dets[keep][passes]
    maxima = T.final_stage(oracle, pos2, po.img_w, po.img_h, None)
    stages = [len(pos), len(keep), int(passes.sum()), len(pos2) if maxima is None else len(maxima)]
    assert len(wins) > stages[0] > stages[1] > stages[2] > stages[3] > 0, stages
    exp = dict(stages=stages, pos2=pos2, maxima=maxima)
    synth.save_svm_text(str(tmp_path / "first.model"), m1, rows=PH, cols=PW)
    synth.save_rvm(str(tmp_path / "second.fdrvm"), m2)
    synth.save_pnm(str(tmp_path / "frame.ppm"), small)
    (tmp_path / "c.cfg").write_text(CFG % ("psvm", tmp_path / "first.model", "prvm", tmp_path / "second.fdrvm", "0.3"))
    out = _run([app, str(tmp_path / "c.cfg"), str(tmp_path / "frame.ppm")])
    check_boxes(boxes(out), exp)
    po.close()


PSVM_FIRST_SEED = 17   # the first seed from 9 on that meets the two conditions on the first stage
PSVM_PRVM_PASS = 0.85


def test_default_classifier_values_behave_as_before(tmp_path, oracle, synth, frame640, small_models):
    """firstClassifier / secondClassifier without a value load a WVM and an SVM as "pwvm" / "psvm" do, and print the oracle's five-stage result"""
    app = app_path()
    wvm, svm = small_models
    synth.save_wvm(str(tmp_path / "face.fdwvm"), wvm)
    synth.save_svm_text(str(tmp_path / "face.svm.txt"), svm, rows=20, cols=20)
    synth.save_pnm(str(tmp_path / "frame.ppm"), frame640)
    cfg = FACE_CFG % (tmp_path / "face.fdwvm", tmp_path / "face.svm.txt")
    (tmp_path / "face.cfg").write_text(cfg)
    assert "firstClassifier pwvm" in cfg and "secondClassifier psvm" in cfg
    (tmp_path / "bare.cfg").write_text(cfg.replace("firstClassifier pwvm", "firstClassifier").replace("secondClassifier psvm", "secondClassifier"))
    out = _run([app, str(tmp_path / "face.cfg"), str(tmp_path / "frame.ppm")])
    assert _run([app, str(tmp_path / "bare.cfg"), str(tmp_path / "frame.ppm")]) == out
    got = [l.split() for l in out.strip().splitlines()]
    po = oracle.Pyramid(inc=float(np.float32(0.92)), min_scale=float(np.float32(0.05)), max_scale=float(np.float32(0.16)))
    po.update(frame640)
    dets, _ = oracle.five_stage(po, oracle.Wvm(wvm), oracle.Svm(svm), 5.0, 0.0, 1, 1, None)
    assert len(got) == len(dets) > 0
    for g, d in zip(got, dets):
        assert g[0] == "FaceFrontal" and g[1] == "face"
        assert [int(v) for v in g[2:6]] == [d["cx"] - d["w"] // 2, d["cy"] - d["h"] // 2, d["w"], d["h"]]
        assert float(g[6]) == d["prob"]
    # an unknown value is refused
    (tmp_path / "bad.cfg").write_text(cfg.replace("firstClassifier pwvm", "firstClassifier pxvm"))
    import subprocess
    r = subprocess.run([app, str(tmp_path / "bad.cfg"), str(tmp_path / "frame.ppm")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LD_LIBRARY_PATH=PKG + ":" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert r.returncode != 0 and "unknown classifier type pxvm" in r.stderr
    po.close()


def frame_lines(out, n):
    """the app's sequence output, 'frame k Name landmark x y w h p', as one single-image text per frame"""
    per = [""] * n
    for l in out.strip().splitlines():
        w = l.split()
        assert w[0] == "frame"
        per[int(w[1])] += " ".join(w[2:]) + "\n"
    return per


@pytest.mark.parametrize("first,second", [("prvm", "psvm"), ("psvm", "prvm")])
def test_detect_frames_runs_other_compositions_one_image_at_a_time(tmp_path, oracle, synth, frame640, first, second):
    """Several images go through FiveStageSlidingWindowDetector::detectFrames.  The multi-frame pyramid is the WVM pair's; the fused RVM path
    and the per-patch composition give for every frame of a same-size sequence what detect(image) gives for it (the models are those of the
    two tests above, whose single-image output is compared with the oracle there)."""
    app = app_path()
    min_scale = "0.2" if first == "prvm" else "0.3"
    small, po, wins, feats = app_scene(oracle, frame640, float(min_scale))
    po.close()
    if first == "prvm":
        m1 = synth.make_rvm(12, feats[::4], PW, PH, n_filters=20, kernel=2)
        m1["logistic_a"], m1["logistic_b"] = 0.4, -2.0
        synth.save_rvm(str(tmp_path / "first.model"), m1)
        m2 = synth.make_svm_f32(PRVM_PSVM_SEED, feats[1::4], nsv=128, gamma=m1["p0"], positive_fraction=0.3, kernel=2)
        synth.save_svm_text(str(tmp_path / "second.model"), m2, rows=PH, cols=PW)
    else:
        synth.save_svm_text(str(tmp_path / "first.model"), first_svm_model(synth, feats, PSVM_FIRST_SEED), rows=PH, cols=PW)
        synth.save_rvm(str(tmp_path / "second.model"), synth.make_rvm(21, feats[2::4], PW, PH, n_filters=12, pass_rate=PSVM_PRVM_PASS))
    images = [small, np.ascontiguousarray(small[:, ::-1]), small]
    names = []
    for i, im in enumerate(images):
        names.append(str(tmp_path / ("frame%d.ppm" % i)))
        synth.save_pnm(names[-1], im)
    (tmp_path / "c.cfg").write_text(CFG % (first, tmp_path / "first.model", second, tmp_path / "second.model", min_scale))
    single = [_run([app, str(tmp_path / "c.cfg"), n]) for n in names]
    assert len(single[0].strip().splitlines()) > 0 and single[0] == single[2] and single[1] != single[0]
    seq = _run([app, str(tmp_path / "c.cfg")] + names)
    assert frame_lines(seq, len(names)) == single


def test_wvm_with_an_f32_svm_is_the_same_for_one_image_and_for_a_sequence(tmp_path, synth, frame640, small_models):
    """A WVM on HistEq64 patches in front of an SVM with f32 support vectors is no case of the fused WVM path (its SVM works on the u8
    patch): detect and detectFrames both compose it per patch, where the SVM refuses the u8 patch as the reference's kernels refuse
    arguments of two types -- the same refusal for one image and for two, not an error from the multi-frame entry point."""
    import subprocess
    app = app_path()
    wvm, _ = small_models
    rng = np.random.default_rng(4)
    svm = synth.make_svm_f32(9, rng.random((400, 400)).astype(np.float32) * 255, nsv=32, gamma=1e-6, positive_fraction=0.3)
    synth.save_wvm(str(tmp_path / "face.fdwvm"), wvm)
    synth.save_svm_text(str(tmp_path / "face.svm.txt"), svm, rows=20, cols=20)
    synth.save_pnm(str(tmp_path / "frame.ppm"), frame640)
    (tmp_path / "face.cfg").write_text(FACE_CFG % (tmp_path / "face.fdwvm", tmp_path / "face.svm.txt"))
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    errs = []
    for imgs in (1, 2):
        r = subprocess.run([app, str(tmp_path / "face.cfg")] + [str(tmp_path / "frame.ppm")] * imgs, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode != 0
        errs.append(r.stderr.strip())
    assert errs[0] == errs[1] and errs[0].startswith("invalid argument: SvmClassifier: feature vector and support vectors")
