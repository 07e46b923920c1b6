"""tracker_app with `tracker partiallyAdaptive` (the reference's partiallyAdaptiveTrackingApp: condensation::WvmSvmModel until a
condensation::SelfLearningMeasurementModel, bootstrapped from the static model's most and least confident samples, is usable) over
twelve 96 x 72 frames of tests/test_gpu_resident_wvm_svm_host.py's scene and models, 100 particles, once per route: FD_COND_DEVICE=0
keeps the particles in Sample objects and picks the examples with fd_particles_examples_select, FD_COND_DEVICE=1 keeps them on the device
and reads the examples and their rows with the state (fd_particles_state_examples_pyramid).  Both routes must print the
same boxes, models, flags, draws, integer sample fields and `sp` / `sn` records; the weights go through exp on the host or on the device
and are compared in units in the last place.

The thresholds come from the weights a first generic run prints (one in which no sample is ever an example): the positive one lies
half way between two neighbouring weights of the second frame, so that more than 10 samples lie above it, the negative one below the
smallest positive weight, so that the samples of weight 0 are the negatives.  The generic run alone must then show a bootstrap frame with
both lists non-empty, a frame evaluated by the adaptive model and a frame with more than 10 candidates on a side."""
import os
import subprocess

import numpy as np
import pytest

import condensation_model as cm
from test_gpu_resident_tracker_host import APP, _parse
from test_gpu_resident_wvm_svm_host import MAX_WIDTH, MIN_WIDTH, OCTAVE_LAYERS, SHIFT
from test_wvm_svm_resident_model import H, PH, PW, W, make_scene

pytestmark = pytest.mark.gpu

FRAMES = 12
WEIGHT_ULPS = 8     # the bound of tests/test_gpu_resident_wvm_svm_host.py for this static model; the adaptive model's one logistic stays inside it
SEED = 7

CONFIG = """tracking {
  seed %(seed)d
  tracker partiallyAdaptive
  transition simple { positionDeviation 3 sizeDeviation 0.05 }
  measurement wvmSvm {
    firstClassifier pwvm { classifierFile %(wvm)s }
    secondClassifier psvm { classifierFile %(svm)s threshold %(threshold)s }
    patch { width %(pw)d height %(ph)d minWidth %(min_width)d maxWidth %(max_width)d octaveLayerCount %(layers)d }
  }
  adaptive selfLearning {
    resampling { particleCount 100 randomRate 0.25 }
    positiveThreshold %(positive)s
    negativeThreshold %(negative)s
    subclass %(subclass)d
    feature hog { pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }
                  gradientKernel 3 blurKernel 0 bins 9 signed 0 interpolate 0
                  histogram spatial { cellSize 8 blockSize 2 interpolate 0 signedAndUnsigned 0 concatenate 0 normalization l2hys } }
    classifier {
      kernel rbf { gamma 0.5 }
      training { c 10 examples fixedsize positiveExamples 10 negativeExamples 50 minPositiveExamples %(min_positives)d }
      probabilistic fixed { logisticA 0.0 logisticB -2.0 }
    }
  }
}
"""


@pytest.fixture(scope="module")
def scene(synth, oracle):
    frame, wvm, svm = make_scene(synth, oracle, min_survivors=400)
    assert frame.shape[:2] == (H, W)
    return [np.roll(frame, (SHIFT[1] * k, SHIFT[0] * k), axis=(0, 1)) for k in range(FRAMES)], wvm, svm


def run(tmp_path, synth, scene, device, positive, negative, dump=True, subclass=0, min_positives=3, frames=FRAMES):
    images, wvm, svm = scene
    synth.save_wvm(str(tmp_path / "face.fdwvm"), wvm)
    synth.save_svm_text(str(tmp_path / "face.svm.txt"), svm, rows=20, cols=20)
    config = tmp_path / "tracking.cfg"
    config.write_text(CONFIG % dict(seed=SEED, wvm=tmp_path / "face.fdwvm", svm=tmp_path / "face.svm.txt", threshold=repr(float(svm["threshold"])), pw=PW, ph=PH,
                                    min_width=MIN_WIDTH, max_width=MAX_WIDTH, layers=OCTAVE_LAYERS, positive=repr(float(positive)),
                                    negative=repr(float(negative)), subclass=subclass, min_positives=min_positives))
    paths = []
    for k, image in enumerate(images[:frames]):
        paths.append(str(tmp_path / ("frame%d.ppm" % k)))
        synth.save_pnm(paths[-1], image)
    env = dict(os.environ, FD_COND_DEVICE="1" if device else "0")
    done = subprocess.run([APP, "--adaptation"] + (["--dump"] if dump else []) + [str(config), "0", "0", "0", "0"] + paths, capture_output=True, text=True,
                          env=env, timeout=120)
    assert done.returncode == 0, done.stdout[-1500:] + done.stderr[-1500:]
    parsed = _parse(done.stdout)
    assert len(parsed) == frames
    k = -1
    for line in done.stdout.split("\n"):   # what _parse does not know: the model, the adaptation line and the example records
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            k += 1
            parsed[k].update(model=t[13], sp=[], sn=[])
        elif t[0] == "adaptation":
            parsed[k].update(was_usable=int(t[1]), materialized=int(t[3]), usable=int(t[5]))
        elif t[0] in ("sp", "sn"):
            parsed[k][t[0]].append(tuple(int(v) for v in t[1:]))
    return parsed


def thresholds(tmp_path, synth, scene):
    """from a generic run in which nothing is ever an example (the static model weighs every frame)"""
    probe = run(tmp_path, synth, scene, False, 2.0, -1.0, frames=3)
    assert all(fr["model"] == "static" and not fr["sp"] and not fr["sn"] for fr in probe)
    seen = np.unique(probe[1]["gen"]["weight"])
    seen = seen[seen > 0]
    assert len(seen) >= 24, len(seen)
    return float((seen[-14] + seen[-15]) / 2), float(seen[0] / 2)


def same_lines(generic, device, first_device_frame=1):
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert g["route"] == "generic" and d["route"] == ("device" if f >= first_device_frame else "generic"), (f, g["route"], d["route"])
        for k in ("found", "box", "adapted", "model", "was_usable", "usable", "sp", "sn"):
            assert g[k] == d[k], (f, k, g[k], d[k])
    return worst


def test_routes_agree(tmp_path, synth, scene):
    positive, negative = thresholds(tmp_path, synth, scene)
    generic = run(tmp_path, synth, scene, False, positive, negative)
    # the run is not vacuous, on the generic route's own output
    bootstrap = [f for f, fr in enumerate(generic) if not fr["was_usable"] and fr["sp"] and fr["sn"]]
    adaptive = [f for f, fr in enumerate(generic) if fr["model"] == "adaptive"]
    crowded = [f for f, fr in enumerate(generic) if (fr["gen"]["weight"] > positive).sum() > 10 or (fr["gen"]["weight"] < negative).sum() > 10]
    print("bootstrap frames %s, adaptive frames %s, frames with more than 10 candidates %s" % (bootstrap, adaptive, crowded))
    assert bootstrap and adaptive and crowded
    assert all(fr["materialized"] == 1 for fr in generic)
    device = run(tmp_path, synth, scene, True, positive, negative)
    same_lines(generic, device)
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert g["draws"] == d["draws"] and g["t"] == d["t"] and g["f"] == d["f"], f
        for k in ("x", "y", "size", "vx", "vy", "vsize", "target", "cluster_id"):
            assert g["gen"][k].tobytes() == d["gen"][k].tobytes(), (f, k)
        worst = max(worst, max(cm.ulp_distance(g["gen"]["weight"], d["gen"]["weight"])))
    print("weights of the two routes at most %d ulp apart" % worst)
    assert worst <= WEIGHT_ULPS
    # without --dump nothing asks for the samples: no device frame builds them (the first frame has no adaptive pyramid yet: generic)
    quiet = run(tmp_path, synth, scene, True, positive, negative, dump=False)
    same_lines(generic, quiet)
    assert [fr["materialized"] for fr in quiet] == [1] + [0] * (FRAMES - 1)


def test_a_failed_retraining_falls_back_to_the_static_model(tmp_path, synth, scene):
    """more positive examples required than the frames offer: every retraining fails, and the next frame is the static model's"""
    positive, negative = thresholds(tmp_path, synth, scene)
    generic = run(tmp_path, synth, scene, False, positive, negative, min_positives=1000, frames=5)
    assert any(fr["sp"] and fr["sn"] for fr in generic)
    assert all(fr["model"] == "static" and fr["usable"] == 0 for fr in generic)
    device = run(tmp_path, synth, scene, True, positive, negative, dump=False, min_positives=1000, frames=5)
    same_lines(generic, device)
    assert [fr["materialized"] for fr in device] == [1, 0, 0, 0, 0]


def test_a_subclass_keeps_the_generic_route(tmp_path, synth, scene):
    positive, negative = thresholds(tmp_path, synth, scene)
    generic = run(tmp_path, synth, scene, False, positive, negative, frames=5)
    subclassed = run(tmp_path, synth, scene, True, positive, negative, subclass=1, frames=5)
    same_lines(generic, subclassed, first_device_frame=5)
    assert all(fr["materialized"] == 1 for fr in subclassed)


def test_what_is_not_built_is_refused_by_name(tmp_path):
    for text, match in (("tracker other", "adaptive and partiallyAdaptive are supported"),
                        ("tracker partiallyAdaptive measurement ehog { }", "needs `measurement wvmSvm`"),
                        ("tracker partiallyAdaptive measurement wvmSvm { } adaptive other { }", "needs `adaptive selfLearning")):
        config = tmp_path / "tracking.cfg"
        config.write_text("tracking { %s }\n" % text)
        done = subprocess.run([APP, str(config), "0", "0", "0", "0", "none.pgm"], capture_output=True, text=True, timeout=60)
        assert done.returncode == 1 and match in done.stderr, done.stderr
