"""tracker_app on the reference's default-like configuration -- `transition opticalFlow` with `fallback simple`, `measurement
positionDependent` on `feature ihog` with scale 1.1 -- over seven 96 x 80 frames after the one it is initialised on, once per route:
FD_COND_DEVICE=0 keeps the particles in Sample objects, FD_COND_DEVICE=1 on the device.  Both routes draw the same
random numbers in the same order -- the device route draws the blocks of both transition models and puts back the one the device's
branch did not use -- so boxes, flags, the flow line of every frame (used or not, counts, median motion), the dumped draws and every
integer field of every sample must agree; the weights go through exp on the host (libm) or on the device (WEIGHT_ULP_BOUND).  The
scores are not compared: SingleClassifierModel does not store them in its samples, the device route reports the SVM's distances.

The precondition -- moving every weight by +-4 ulp changes no selected index and no state -- is asserted on the generic run's own
weights, as tests/test_gpu_condensation_host_app.py asserts it (they are SVM scores of the frames and exist only after a device run).

The frames are tests/resident_model.chain_frames: a texture moved by (2, 1) per frame with one unrelated frame, so the flow predicts in
some frames and the fallback in others (tests/test_resident_model.py pins both on the CPU)."""
import os
import subprocess

import numpy as np
import pytest

import condensation_model as model
import resident_model
from test_condensation_host import _dumped_generation
from test_gpu_condensation import WEIGHT_ULP_BOUND
from test_gpu_condensation_host_app import _stable_under_four_ulp
from test_gpu_integral_hog_host_app import DEFAULT_IHOG
from test_position_dependent_host import FEATURES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
FRAMES = 8

CONFIG = """tracking {
  seed 7
  transition opticalFlow { positionDeviation 2 sizeDeviation 0.04 %(transition)s fallback simple { positionDeviation 3 sizeDeviation 0.05 } }
  adaptive { resampling { particleCount 80 randomRate 0.25 minSize 16 maxSize 60 } }
  initialCount 80
  measurement positionDependent {
    %(feature)s
    filter none  startFrameCount 1  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget 2  sampleAdditionalNegatives 6  sampleTestNegatives 5
    exploitSymmetry 0
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
}
"""


def _parse(text):
    frames, cur = [], None
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            cur = dict(found=int(t[3]), box=tuple(int(v) for v in t[4:8]), adapted=int(t[9]), route=t[11], draws=None, flow=None, t=[], f=[], s=[])
            frames.append(cur)
        elif t[0] == "flow":
            cur["flow"] = (int(t[1]), int(t[3]), int(t[5]), int(t[7])) + tuple(float(v) for v in t[9:12])
        elif t[0] == "draws":
            cur["draws"] = (int(t[2]), float(t[3]), int(t[5]), int(t[7]))
        elif t[0] in ("d", "z"):
            cur["t"].append((t[0],) + tuple(float(v) for v in t[1:4]))
        elif t[0] == "f":
            cur["f"].append(tuple(int(v) for v in t[1:4]))
        elif t[0] == "s":
            cur["s"].append(t[1:])
    for fr in frames:
        fr["gen"] = _dumped_generation(fr["s"])
    return frames


def _run(tmp_path, device, feature=DEFAULT_IHOG, transition=""):
    config = tmp_path / "tracking.cfg"
    config.write_text(CONFIG % dict(feature=feature, transition=transition))
    paths = []
    for k, frame in enumerate(resident_model.chain_frames(FRAMES)):
        path = tmp_path / ("frame%d.pgm" % k)
        with open(path, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (resident_model.CHAIN_W, resident_model.CHAIN_H))
            f.write(frame.tobytes())
        paths.append(str(path))
    x, y, size = resident_model.CHAIN_TARGET
    env = dict(os.environ, FD_COND_DEVICE="1" if device else "0")
    run = subprocess.run([APP, "--dump", str(config), str(x - size // 2), str(y - size // 2), str(size), str(size)] + paths, capture_output=True, text=True,
                         env=env, timeout=120)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.startswith("init 1 "), run.stdout[:200]
    frames = _parse(run.stdout)
    assert len(frames) == FRAMES - 1
    return frames


def test_routes_agree(tmp_path):
    generic = _run(tmp_path, device=False)
    device = _run(tmp_path, device=True)
    _stable_under_four_ulp(generic)
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert g["route"] == "generic" and d["route"] == "device", (f, g["route"], d["route"])
        assert (g["found"], g["box"], g["adapted"]) == (d["found"], d["box"], d["adapted"]), (f, g["found"], g["box"], d["found"], d["box"])
        assert g["flow"] == d["flow"], (f, g["flow"], d["flow"])
        assert g["draws"] == d["draws"] and g["t"] == d["t"] and g["f"] == d["f"], f
        for k in ("x", "y", "size", "vx", "vy", "vsize", "target", "cluster_id"):
            assert g["gen"][k].tobytes() == d["gen"][k].tobytes(), (f, k)
        ulps = max(model.ulp_distance(g["gen"]["weight"], d["gen"]["weight"]))
        print("frame %d: flow %s, found %d, weights at most %d ulp apart" % (f, g["flow"][:4], g["found"], ulps))
        assert ulps <= WEIGHT_ULP_BOUND, (f, ulps)
        worst = max(worst, ulps)
    used = [fr["flow"][0] for fr in generic]
    assert 1 in used and 0 in used, used                       # both transition models predicted, on the same frames on both routes
    assert any(kind == "z" for fr in device for kind, *_ in fr["t"]) and any(kind == "d" for fr in device for kind, *_ in fr["t"])
    assert sum(fr["found"] for fr in generic) >= 3
    print("weights of the two routes: at most %d ulp apart" % worst)


@pytest.mark.parametrize("name,settings", [("subclassed-transition", dict(transition="subclass 1")), ("grid-40x40", dict(transition="gridSize 40")),
                                           ("pyramid-feature", dict(feature=FEATURES["hog"]))])
def test_other_configurations_keep_the_generic_route(tmp_path, name, settings):
    frames = _run(tmp_path, device=True, **settings)
    assert [fr["route"] for fr in frames] == ["generic"] * (FRAMES - 1), name
