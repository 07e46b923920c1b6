"""tracker_app with `measurement wvmSvm` (the reference's face tracker: a CondensationTracker on condensation::WvmSvmModel) over eight
96 x 72 frames after the first one, 100 particles, once per route: FD_COND_DEVICE=0 keeps the particles in Sample objects and scores them
with fd_wvm_svm_evaluate_samples, FD_COND_DEVICE=1 keeps them on the device (fd_particles_evaluate_wvm_svm / _weigh_wvm_svm, DESIGN.md
4.7).  Both routes draw the same random numbers in the same order, so boxes, flags, the dumped draws and every integer field of every
sample must agree; the weights go through exp on the host (libm) or on the device: at most 8 ulp apart, as
tests/test_gpu_particles_wvm_svm.py derives.  The scores are not compared: WvmSvmModel does not store them in its samples, the device
route reports the WVM's outputs.

Two preconditions are asserted on the generic run's own dump.  Per frame, the 8th and 9th most probable WVM positives of its samples
differ in probability (with a tie the reference's choice is an accident of its sort; the device takes the lower index): the samples go
through the oracle's pieces for that.  And moving every weight by +-8 ulp changes no selected index and no state."""
import os
import subprocess

import numpy as np
import pytest

import condensation_model as cm
import resident_model
import wvm_svm_resident_model as model
from test_gpu_resident_tracker_host import APP, _parse
from test_wvm_svm_resident_model import H, PH, PW, W, make_scene, oracle_outputs

pytestmark = pytest.mark.gpu

FRAMES = 9          # the first one starts the tracker ("init"), eight are compared
WEIGHT_ULPS = 8
SEED = 7
SHIFT = (2, 1)      # the scene moves by this much per frame
MIN_WIDTH, MAX_WIDTH, OCTAVE_LAYERS = 25, 50, 3

CONFIG = """tracking {
  seed %(seed)d
  transition simple { positionDeviation 3 sizeDeviation 0.05 }
  adaptive { resampling { particleCount 100 randomRate 0.25 } }
  measurement wvmSvm {
    firstClassifier pwvm { classifierFile %(wvm)s }
    secondClassifier psvm { classifierFile %(svm)s threshold %(threshold)s }
    patch { width %(pw)d height %(ph)d minWidth %(min_width)d maxWidth %(max_width)d octaveLayerCount %(layers)d }
  }
}
"""


def scene_frames(synth, oracle):
    """the models of tests/test_wvm_svm_resident_model.py with a cascade that lets more windows through, and their frame rolled by SHIFT
    per frame"""
    frame, wvm, svm = make_scene(synth, oracle, min_survivors=400)
    return [np.roll(frame, (SHIFT[1] * k, SHIFT[0] * k), axis=(0, 1)) for k in range(FRAMES)], wvm, svm


def run(tmp_path, synth, frames, wvm, svm, device, seed=SEED):
    synth.save_wvm(str(tmp_path / "face.fdwvm"), wvm)
    synth.save_svm_text(str(tmp_path / "face.svm.txt"), svm, rows=20, cols=20)
    config = tmp_path / "tracking.cfg"
    config.write_text(CONFIG % dict(seed=seed, wvm=tmp_path / "face.fdwvm", svm=tmp_path / "face.svm.txt", threshold=repr(float(svm["threshold"])),
                                    pw=PW, ph=PH, min_width=MIN_WIDTH, max_width=MAX_WIDTH, layers=OCTAVE_LAYERS))
    paths = []
    for k, frame in enumerate(frames):
        paths.append(str(tmp_path / ("frame%d.ppm" % k)))
        synth.save_pnm(paths[-1], frame)
    env = dict(os.environ, FD_COND_DEVICE="1" if device else "0")
    done = subprocess.run([APP, "--counts", "--dump", str(config), "0", "0", "0", "0"] + paths, capture_output=True, text=True, env=env, timeout=120)
    assert done.returncode == 0, done.stdout[-1500:] + done.stderr[-1500:]
    assert done.stdout.startswith("init "), done.stdout[:200]
    parsed = _parse(done.stdout)
    assert len(parsed) == FRAMES - 1
    last = done.stdout.strip().split("\n")[-1].split()
    assert last[0] == "evaluations" and last[1] == "fused" and last[3] == "loop", last
    return parsed, int(last[2]), int(last[4])


def app_pyramid(oracle):
    """the pyramid DirectPyramidFeatureExtractor(width, height, minWidth, maxWidth, octaveLayerCount) builds (.cpp:27-36): the scale limits
    are powers of the incremental scale, as the app computes them"""
    inc = 0.5 ** (1.0 / OCTAVE_LAYERS)
    index = lambda width: int(np.rint(np.log(PW / width) / np.log(inc)))
    return oracle.Pyramid(octave_layers=OCTAVE_LAYERS, min_scale=inc ** index(MAX_WIDTH), max_scale=inc ** index(MIN_WIDTH))


def positives_per_frame(oracle, frames, wvm, svm, generic):
    """per compared frame (tie-free, number of WVM positives) of the generic run's samples, through the oracle's pieces"""
    out = []
    pyr = app_pyramid(oracle)
    for k, fr in enumerate(generic):
        pyr.update(frames[k + 1])
        assert [(l["w"], l["h"]) for l in pyr.layers()][:2] == [(76, 57), (60, 45)]
        samples = resident_model.sample_xywh(fr["gen"], 1.0)
        valid, level, fout, _ = oracle_outputs(oracle, pyr, wvm, svm, samples)
        assert np.array_equal(valid, fr["gen"]["weight"] != 0)   # no valid sample's weight underflows: the dump tells the valid ones
        out.append(model.tie_free(wvm, valid, level, fout))
    pyr.close()
    return out


def stable_under(frames, ulps):
    """+-ulps on every weight changes no selection and no state"""
    for f in range(1, len(frames)):
        old, fr = frames[f - 1]["gen"], frames[f]
        has_u, u, copies, fresh = fr["draws"]
        want = cm.low_variance_indices(old["weight"], copies, u) if has_u else []
        state = cm.filtered_state(old)
        for nudge in (-ulps, ulps):
            moved = dict(old)
            moved["weight"] = cm.nudge(old["weight"], nudge)
            assert cm.low_variance_indices(moved["weight"], copies, u) == want or not has_u, (f, nudge)
            assert cm.filtered_state(moved) == state, (f, nudge)


def test_routes_agree(tmp_path, synth, oracle):
    frames, wvm, svm = scene_frames(synth, oracle)
    assert frames[0].shape[:2] == (H, W)
    generic, generic_fused, generic_loop = run(tmp_path, synth, frames, wvm, svm, device=False)
    device, fused, loop = run(tmp_path, synth, frames, wvm, svm, device=True)
    # one batched evaluation per frame, the first included, and no per-sample evaluation on either route
    assert (generic_fused, generic_loop) == (FRAMES, 0) and (fused, loop) == (FRAMES, 0), (generic_fused, generic_loop, fused, loop)
    conditions = positives_per_frame(oracle, frames, wvm, svm, generic)
    print("WVM positives per frame:", [n for _, n in conditions])
    assert all(free for free, _ in conditions), conditions
    assert max(n for _, n in conditions) > model.RESCORED, conditions
    stable_under(generic, WEIGHT_ULPS)
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert g["route"] == "generic" and d["route"] == "device", (f, g["route"], d["route"])
        assert (g["found"], g["box"], g["adapted"]) == (d["found"], d["box"], 0), (f, g["found"], g["box"], d["found"], d["box"])
        assert g["draws"] == d["draws"] and g["t"] == d["t"] and g["f"] == d["f"], f
        assert len(g["gen"]["x"]) == 100
        for k in ("x", "y", "size", "vx", "vy", "vsize", "target", "cluster_id"):
            assert g["gen"][k].tobytes() == d["gen"][k].tobytes(), (f, k)
        ulps = max(cm.ulp_distance(g["gen"]["weight"], d["gen"]["weight"]))
        assert ulps <= WEIGHT_ULPS, (f, ulps)
        worst = max(worst, ulps)
    assert sum(fr["found"] for fr in generic) >= 3 and sum(int(fr["gen"]["target"].sum()) for fr in generic) >= 8
    print("found in %d of %d frames, weights of the two routes at most %d ulp apart" % (sum(fr["found"] for fr in generic), len(generic), worst))


def test_the_unknown_model_message_names_all_three(tmp_path):
    config = tmp_path / "tracking.cfg"
    config.write_text("tracking { measurement other { classifier { } } }\n")
    done = subprocess.run([APP, str(config), "0", "0", "0", "0", "none.pgm"], capture_output=True, text=True, timeout=60)
    assert done.returncode == 1 and "ehog, positionDependent and wvmSvm are supported" in done.stderr, done.stderr
