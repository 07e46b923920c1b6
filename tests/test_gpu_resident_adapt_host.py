"""tracker_app --adaptation --dump on `measurement positionDependent`, once per route, on the frame chain of
tests/test_gpu_resident_tracker_host.py: with FD_COND_DEVICE=1 the additional negatives of PositionDependentMeasurementModel::adapt are
chosen on the device behind the state (fd_particles_state_negatives), so process() never builds the Sample objects of
its generation -- every device frame reports `materialized 0` -- and still adapts on the same samples: the boxes, the flags, the
rectangles of every adaptation record (positives, negatives with the chosen ones among them, test negatives: the random fill-ins and
test samples are drawn behind the choice, so they agree only when the choice does), the dumped draws and every integer field of every
sample are those of the generic route; the weights go through exp on the host or on the device (WEIGHT_ULP_BOUND).  Run with
`transition opticalFlow` on `feature ihog` (the reference's default-like configuration) and with `transition simple` on a pyramid
feature type.  A subclassed model keeps the generic route, and 65 additional negatives are more than the device chooses: both report
`materialized 1` and the generic route's output."""
import os
import subprocess

import pytest

import condensation_model as model
import resident_model
from test_gpu_condensation import WEIGHT_ULP_BOUND
from test_gpu_condensation_host_app import _stable_under_four_ulp
from test_gpu_integral_hog_host_app import DEFAULT_IHOG
from test_gpu_resident_pyramid_host import HOG
from test_gpu_resident_tracker_host import APP, FRAMES, _parse

pytestmark = pytest.mark.gpu

FLOW = "opticalFlow { positionDeviation 2 sizeDeviation 0.04 fallback simple { positionDeviation 3 sizeDeviation 0.05 } }"
SIMPLE = "simple { positionDeviation 3 sizeDeviation 0.05 }"
CASES = {"ihog-optical-flow": (DEFAULT_IHOG, FLOW), "hog-simple": (HOG, SIMPLE)}

CONFIG = """tracking {
  seed 7
  transition %(transition)s
  adaptive { resampling { particleCount 80 randomRate 0.25 minSize 16 maxSize 60 } }
  initialCount 80
  measurement positionDependent {
    %(feature)s
    filter none  startFrameCount 1  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget 2  sampleAdditionalNegatives %(additional)d  sampleTestNegatives 5
    exploitSymmetry 0  subclass %(subclass)d
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
}
"""


def _adaptations(text):
    """per frame dict(adaptation, materialized, ap, an, at): the lines --adaptation adds"""
    frames, cur = [], None
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            cur = dict(adaptation=None, materialized=None, counts={}, ap=[], an=[], at=[])
            frames.append(cur)
        elif t[0] == "adaptation":
            assert t[2] == "materialized"
            cur["adaptation"], cur["materialized"] = int(t[1]), int(t[3])
        elif t[0] in ("positives", "negatives", "testNegatives"):
            cur["counts"][t[0]] = int(t[1])
        elif t[0] in ("ap", "an", "at"):
            cur[t[0]].append(tuple(int(v) for v in t[1:4]))
    return frames


def _run(tmp_path, device, case, additional=6, subclass=0):
    feature, transition = CASES[case]
    config = tmp_path / "tracking.cfg"
    config.write_text(CONFIG % dict(feature=feature, transition=transition, additional=additional, subclass=subclass))
    paths = []
    for k, frame in enumerate(resident_model.chain_frames(FRAMES)):
        path = tmp_path / ("frame%d.pgm" % k)
        with open(path, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (resident_model.CHAIN_W, resident_model.CHAIN_H))
            f.write(frame.tobytes())
        paths.append(str(path))
    x, y, size = resident_model.CHAIN_TARGET
    env = dict(os.environ, FD_COND_DEVICE="1" if device else "0")
    run = subprocess.run([APP, "--adaptation", "--dump", str(config), str(x - size // 2), str(y - size // 2), str(size), str(size)] + paths,
                         capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.startswith("init 1 "), run.stdout[:200]
    frames, extra = _parse(run.stdout), _adaptations(run.stdout)
    assert len(frames) == len(extra) == FRAMES - 1
    for fr, ex in zip(frames, extra):
        assert ex["adaptation"] == fr["adapted"] and ex["materialized"] in (0, 1)
        if ex["adaptation"]:
            assert ex["counts"] == dict(positives=len(ex["ap"]), negatives=len(ex["an"]), testNegatives=len(ex["at"]))
            assert len(ex["an"]) == 18 + additional and len(ex["at"]) == 5 and len(ex["ap"]) == 5   # sampleNegativesAroundTarget 2: 18
        else:
            assert not ex["counts"] and not ex["ap"] and not ex["an"] and not ex["at"]
        fr.update(ex)
    return frames


def _same_output(generic, device, routes, materialized):
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert (g["route"], d["route"]) == routes, (f, g["route"], d["route"])
        assert (g["found"], g["box"], g["adapted"]) == (d["found"], d["box"], d["adapted"]), (f, g["found"], g["box"], d["found"], d["box"])
        assert g["flow"] == d["flow"], (f, g["flow"], d["flow"])
        for k in ("ap", "an", "at"):
            assert g[k] == d[k], (f, k, g[k], d[k])
        assert g["draws"] == d["draws"] and g["t"] == d["t"] and g["f"] == d["f"], f
        for k in ("x", "y", "size", "vx", "vy", "vsize", "target", "cluster_id"):
            assert g["gen"][k].tobytes() == d["gen"][k].tobytes(), (f, k)
        ulps = max(model.ulp_distance(g["gen"]["weight"], d["gen"]["weight"]))
        assert ulps <= WEIGHT_ULP_BOUND, (f, ulps)
        worst = max(worst, ulps)
        assert g["materialized"] == 1 and d["materialized"] == materialized, (f, g["materialized"], d["materialized"])
    return worst


@pytest.mark.parametrize("case", sorted(CASES))
def test_routes_agree_and_nothing_is_materialized(tmp_path, case):
    generic = _run(tmp_path, False, case)
    device = _run(tmp_path, True, case)
    _stable_under_four_ulp(generic)
    worst = _same_output(generic, device, ("generic", "device"), 0)
    adapted = sum(fr["adapted"] for fr in generic)
    assert adapted >= 3 and sum(fr["found"] for fr in generic) >= 3
    # the chosen samples are real ones: among the negatives of an adaptation, behind the 18 around the target, samples of that frame's generation
    chosen = [s for fr in device if fr["adapted"] for s in fr["an"][18:]]
    print("%s: %d adaptations, %d chosen negatives, weights of the two routes at most %d ulp apart" % (case, adapted, len(chosen), worst))


def test_a_subclassed_model_keeps_the_generic_route(tmp_path):
    generic = _run(tmp_path, False, "ihog-optical-flow")
    subclassed = _run(tmp_path, True, "ihog-optical-flow", subclass=1)
    _same_output(generic, subclassed, ("generic", "generic"), 1)


def test_more_negatives_than_the_device_chooses(tmp_path):
    generic = _run(tmp_path, False, "ihog-optical-flow", additional=65)
    device = _run(tmp_path, True, "ihog-optical-flow", additional=65)
    _stable_under_four_ulp(generic)
    _same_output(generic, device, ("generic", "device"), 1)
