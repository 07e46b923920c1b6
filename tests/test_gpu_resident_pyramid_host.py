"""tracker_app with `measurement positionDependent` on the pyramid feature types (hog, ehog, glbp, grayscale, whi; hog also behind the
`scale 1.1` wrapper) over six 96 x 80 frames after the one it is initialised on, once per route: FD_COND_DEVICE unset keeps the particles
in Sample objects, FD_COND_DEVICE=1 on the device, where fd_particles_evaluate_pyramid resolves and scores them.  With
`transition opticalFlow` a pyramid feature type keeps the generic route under FD_COND_DEVICE=1 (tests/test_gpu_resident_tracker_host.py pins
that; the library's own flow frame on a pyramid chain is in tests/test_gpu_particles_pyramid.py): that case asserts the route and equal output.  Both
routes draw the same random numbers in the same order, so boxes, flags, flow lines, the dumped draws and every integer field of every
sample must agree; the weights go through exp on the host (libm) or on the device (WEIGHT_ULP_BOUND).  The scores are not compared:
SingleClassifierModel does not store them in its samples, the device route reports the SVM's distances.

The precondition -- moving every weight by +-4 ulp changes no selected index and no state -- is asserted on the generic run's own
weights, as tests/test_gpu_resident_tracker_host.py asserts it.  The frames are tests/resident_model.chain_frames."""
import os
import subprocess

import pytest

import condensation_model as model
import resident_model
from test_gpu_condensation import WEIGHT_ULP_BOUND
from test_gpu_condensation_host_app import _stable_under_four_ulp
from test_gpu_resident_tracker_host import APP, _parse
from test_position_dependent_host import FEATURES

pytestmark = pytest.mark.gpu

FRAMES = 7
PYRAMID = "pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }"
FLOW = "opticalFlow { positionDeviation 2 sizeDeviation 0.04 fallback simple { positionDeviation 3 sizeDeviation 0.05 } }"
SIMPLE = "simple { positionDeviation 3 sizeDeviation 0.05 }"
# the blocks of tests/test_position_dependent_host.py with the cells (hog) and the normalization (glbp) at which the tracker finds its
# target on these frames in most of them, so that the states and the adaptation are compared too
HOG = FEATURES["hog"].replace("cellSize 8", "cellSize 4")
GLBP = FEATURES["glbp"].replace("normalization l2hys", "normalization none")
assert HOG != FEATURES["hog"] and GLBP != FEATURES["glbp"]
CASES = {
    "hog": (HOG, SIMPLE),
    "ehog": (FEATURES["ehog"], SIMPLE),
    "glbp": (GLBP, SIMPLE),
    "grayscale": ("feature grayscale { %s }" % PYRAMID, SIMPLE),
    "whi": ("feature whi { %s }" % PYRAMID, SIMPLE),
    "hog-scale-1.1": (HOG.replace("gradientKernel 3", "scale 1.1 gradientKernel 3"), SIMPLE),
    "hog-optical-flow": (HOG, FLOW),
}

CONFIG = """tracking {
  seed 7
  transition %(transition)s
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


def _run(tmp_path, device, feature, transition):
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
    env = dict(os.environ)
    env.pop("FD_COND_DEVICE", None)
    if device:
        env["FD_COND_DEVICE"] = "1"
    run = subprocess.run([APP, "--counts", "--dump", str(config), str(x - size // 2), str(y - size // 2), str(size), str(size)] + paths, capture_output=True,
                         text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.startswith("init 1 "), run.stdout[:200]
    frames = _parse(run.stdout)
    assert len(frames) == FRAMES - 1
    last = run.stdout.strip().split("\n")[-1].split()
    assert last[0] == "evaluations" and last[1] == "fused" and last[3] == "loop", last
    return frames, int(last[2]), int(last[4])


@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_agree(tmp_path, name):
    feature, transition = CASES[name]
    generic, generic_fused, generic_loop = _run(tmp_path, False, feature, transition)
    device, fused, loop = _run(tmp_path, True, feature, transition)
    resident = transition == SIMPLE
    assert (fused, loop) == (FRAMES - 1, 0), (fused, loop)
    # the generic route scores a wrapped pyramid extractor sample by sample, any other in one call
    assert (generic_fused, generic_loop) == ((0, FRAMES - 1) if name == "hog-scale-1.1" else (FRAMES - 1, 0)), (generic_fused, generic_loop)
    _stable_under_four_ulp(generic)
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert g["route"] == "generic" and d["route"] == ("device" if resident else "generic"), (f, g["route"], d["route"])
        assert (g["found"], g["box"], g["adapted"]) == (d["found"], d["box"], d["adapted"]), (f, g["found"], g["box"], d["found"], d["box"])
        assert g["flow"] == d["flow"] and (g["flow"] is not None) == (name == "hog-optical-flow"), (f, g["flow"], d["flow"])
        assert g["draws"] == d["draws"] and g["t"] == d["t"] and g["f"] == d["f"], f
        for k in ("x", "y", "size", "vx", "vy", "vsize", "target", "cluster_id"):
            assert g["gen"][k].tobytes() == d["gen"][k].tobytes(), (f, k)
        ulps = max(model.ulp_distance(g["gen"]["weight"], d["gen"]["weight"]))
        assert ulps <= WEIGHT_ULP_BOUND, (f, ulps)
        worst = max(worst, ulps)
    assert sum(fr["found"] for fr in generic) >= 3
    print("%s: found in %d of %d frames, weights of the two routes at most %d ulp apart" % (name, sum(fr["found"] for fr in generic), len(generic), worst))
