"""ffp_detect_app with the `imageFilter greyworld` key of this backend: ImagePyramid::addImageFilter(GreyWorldNormalizationFilter) in
front of the GrayscaleFilter, through detect(image) and detectFrames(images).  Printed results equal the oracle chain's."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "featuredetection_amd")
FF = dict(inc=float(np.float32(0.92)), min_scale=float(np.float32(0.05)), max_scale=float(np.float32(0.16)))

# the config of test_gpu_host_apps.py with one more line in the pyramid node
FACE_CFG = """detectors
{
    FaceFrontal
    {
        landmark "face"
        type fiveStageCascade ; same keys as ffpDetectApp/FaceFrontal.cfg
        firstClassifier pwvm
        {
            classifierFile %s
        }
        secondClassifier psvm
        {
            classifierFile %s
        }
        pyramid
        {
            minScaleFactor 0.05
            maxScaleFactor 0.16
            incrementalScaleFactor 0.92
%s            patch
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
KEY = "            imageFilter greyworld\n"


def variant(frame, kind):
    """cast: channel gains 0.55, 0.8, 1.0 on B, G, R; sat: red gain 1.9, clipped to 255 (as in test_gpu_greyworld_pyramid.py)"""
    gains = {"cast": (0.55, 0.8, 1.0), "sat": (1.0, 1.0, 1.9)}[kind]
    return np.clip(np.rint(frame.astype(np.float64) * np.array(gains)), 0, 255).astype(np.uint8)


def oracle_chain(oracle, frame, **kw):
    po = oracle.Pyramid(**kw)
    po.update(oracle.greyworld(frame))
    return po


def _run(args, ok=True):
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr)
    return r.stdout


def _setup(tmp_path, synth, small_models, frames):
    app = os.path.join(PKG, "ffp_detect_app")
    if not os.path.exists(app):
        pytest.fail("host apps not built (make -C featuredetection_amd/host)")
    wvm, svm = small_models
    synth.save_wvm(str(tmp_path / "face.fdwvm"), wvm)
    synth.save_svm_text(str(tmp_path / "face.svm.txt"), svm, rows=20, cols=20)
    for name, key in (("greyworld.cfg", KEY), ("plain.cfg", "")):
        (tmp_path / name).write_text(FACE_CFG % (tmp_path / "face.fdwvm", tmp_path / "face.svm.txt", key))
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / ("frame%d.ppm" % i)))
        synth.save_pnm(paths[-1], f)
    return app, paths


def _expected(oracle, small_models, frame, greyworld):
    wvm, svm = small_models
    if greyworld:
        po = oracle_chain(oracle, frame, **FF)
    else:
        po = oracle.Pyramid(**FF)
        po.update(frame)
    dets, stages = oracle.five_stage(po, oracle.Wvm(wvm), oracle.Svm(svm), 5.0, 0.0, 1, 1, None)
    po.close()
    return dets, stages


def _same_lines(lines, dets):
    assert len(lines) == len(dets)
    for g, d in zip(lines, dets):
        assert g[0] == "FaceFrontal" and g[1] == "face"
        assert [int(v) for v in g[2:6]] == [d["cx"] - d["w"] // 2, d["cy"] - d["h"] // 2, d["w"], d["h"]]   # Patch::getBounds
        assert float(g[6]) == d["prob"]


def test_ffp_detect_app_greyworld_one_image(tmp_path, oracle, synth, frame640, small_models):
    frame = variant(frame640, "sat")
    app, paths = _setup(tmp_path, synth, small_models, [frame])
    want, st = _expected(oracle, small_models, frame, True)
    plain, st_plain = _expected(oracle, small_models, frame, False)
    assert len(want) > 0 and len(plain) > 0 and not np.array_equal(st, st_plain)
    assert len(want) != len(plain) or not np.array_equal(want["prob"], plain["prob"])   # the printed lines tell the two apart
    got = [l.split() for l in _run([app, str(tmp_path / "greyworld.cfg"), paths[0]]).strip().splitlines()]
    _same_lines(got, want)
    # the same config without the key prints the plain result
    got = [l.split() for l in _run([app, str(tmp_path / "plain.cfg"), paths[0]]).strip().splitlines()]
    _same_lines(got, plain)
    # an unknown filter name is an error, not a silent plain run
    (tmp_path / "bad.cfg").write_text((tmp_path / "greyworld.cfg").read_text().replace("imageFilter greyworld", "imageFilter sepia"))
    _run([app, str(tmp_path / "bad.cfg"), paths[0]], ok=False)


def test_ffp_detect_app_greyworld_image_sequence(tmp_path, oracle, synth, frame640, small_models):
    """three images: FiveStageSlidingWindowDetector::detectFrames, whose multi-frame pyramid takes the setting over"""
    frames = [frame640, variant(synth.make_frame(640, 480, seed=31), "cast"), variant(synth.make_frame(640, 480, seed=32), "sat")]
    app, paths = _setup(tmp_path, synth, small_models, frames)
    for cfg, greyworld in (("greyworld.cfg", True), ("plain.cfg", False)):
        got = [l.split() for l in _run([app, str(tmp_path / cfg)] + paths).strip().splitlines()]
        total = 0
        for fi, f in enumerate(frames):
            dets, _ = _expected(oracle, small_models, f, greyworld)
            mine = [g for g in got if g[0] == "frame" and int(g[1]) == fi]
            _same_lines([g[2:] for g in mine], dets)
            total += len(dets)
        assert total > 0 and len(got) == total
