"""tracker_app (AdaptiveCondensationTracker on an ExtendedHogBasedMeasurementModel that trains its SVM on the device) over eight
176 x 144 frames after the one it is initialised on, once per route: FD_COND_DEVICE=0 keeps the particles in Sample objects on the host, FD_COND_DEVICE=1 on the device.
Both routes draw the same random numbers in the same order, so boxes, flags and every integer field of every sample must agree;
the weights go through exp on the host (libm) or on the device and may differ in the last places (WEIGHT_ULP_BOUND, on every frame).

The precondition of that comparison -- moving every weight by +-4 ulp changes no selected index and no state -- is asserted here, on each
run's own dumped weights (_stable_under_four_ulp), and not in the CPU tests: these weights come from the extended-HOG scores of the
frames and exist only after a device run.  tests/test_condensation_host.py asserts the same property on the CPU for the seeds and frames
of tracker_app's self-test, whose weights need no device."""
import os
import subprocess

import numpy as np
import pytest

import condensation_model as model
from test_condensation_host import _dumped_generation
from test_gpu_condensation import WEIGHT_ULP_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
W, H = 176, 144

CONFIG = """tracking {
    transition simple { positionDeviation 3 sizeDeviation 0.04 }
    adaptive { resampling { particleCount %(count)d randomRate %(rate)s minSize 20 maxSize 80 } }
    initialCount %(count)d
    seed %(seed)d
    measurement ehog {
        cellSize 4 cellCount 12 signedAndUnsigned 1 interpolateBins 0 interpolateCells 1 octaveLayerCount 2
        rejectionThreshold -0.5 useSlidingWindow %(sliding)d conservativeReInit 0
        negativeExampleCount 10 initialNegativeExampleCount 40 randomExampleCount 40 negativeScoreThreshold -1.0
        adaptation %(adaptation)s adaptationThreshold 0.25 exclusionThreshold 0.0
        classifier { training { c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.0 logisticB -2.0 threshold %(threshold)s }
    }
}
"""


def _frame(x0, y0):
    rng = np.random.default_rng(99)
    frame = rng.integers(90, 130, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:40, 0:30]
    blob = (128 + 100 * np.sin(xx / 2.5) * np.cos(yy / 3.5)).astype(np.uint8)
    if x0 is not None:   # None: the target is out of sight
        frame[y0:y0 + 40, x0:x0 + 30] = blob[:, :, None]
    return frame


def _write_frames(tmp_path, positions):
    paths = []
    for k, (x0, y0) in enumerate(positions):
        path = tmp_path / ("frame%d.ppm" % k)
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (W, H))
            f.write(_frame(x0, y0).tobytes())
        paths.append(str(path))
    return paths


def _parse(text):
    frames, cur = [], None
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            cur = dict(found=int(t[3]), box=tuple(int(v) for v in t[4:8]), adapted=int(t[9]), route=t[11], draws=None, d=[], f=[], s=[])
            frames.append(cur)
        elif t[0] == "draws":
            cur["draws"] = (int(t[2]), float(t[3]), int(t[5]), int(t[7]))
        elif t[0] == "d":
            cur["d"].append(tuple(float(v) for v in t[1:4]))
        elif t[0] == "f":
            cur["f"].append(tuple(int(v) for v in t[1:4]))
        elif t[0] == "s":
            cur["s"].append(t[1:])
    for fr in frames:
        fr["gen"] = _dumped_generation(fr["s"])
    return frames


def _run(tmp_path, positions, device, **cfg):
    settings = dict(count=120, rate="0.25", seed=5, sliding=1, adaptation="position", threshold="0")
    settings.update(cfg)
    config = tmp_path / "tracking.cfg"
    config.write_text(CONFIG % settings)
    paths = _write_frames(tmp_path, positions)
    x0, y0 = positions[0]
    env = dict(os.environ, FD_COND_DEVICE="1" if device else "0")
    run = subprocess.run([APP, "--dump", str(config), str(x0), str(y0), "30", "40"] + paths, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.startswith("init 1 %d %d 30 40" % (x0, y0)), run.stdout[:200]
    return _parse(run.stdout)


def _compare_routes(generic, device):
    assert len(generic) == len(device) == 8
    worst = 0
    for f, (g, d) in enumerate(zip(generic, device)):
        assert g["route"] == "generic" and d["route"] == "device", (f, g["route"], d["route"])
        assert (g["found"], g["box"], g["adapted"]) == (d["found"], d["box"], d["adapted"]), (f, g["found"], g["box"], d["found"], d["box"])
        assert g["draws"] == d["draws"] and g["d"] == d["d"] and g["f"] == d["f"], f
        for k in ("x", "y", "size", "vx", "vy", "vsize", "score", "target", "cluster_id"):
            assert g["gen"][k].tobytes() == d["gen"][k].tobytes(), (f, k)
        ulps = max(model.ulp_distance(g["gen"]["weight"], d["gen"]["weight"]))
        assert ulps <= WEIGHT_ULP_BOUND, (f, ulps)
        worst = max(worst, ulps)
    print("weights of the two routes: at most %d ulp apart" % worst)


def _stable_under_four_ulp(frames):
    """the precondition of the comparison, on the run's own weights: +-4 ulp on every weight changes no selection and no state"""
    for f in range(1, len(frames)):
        old, fr = frames[f - 1]["gen"], frames[f]
        has_u, u, copies, fresh = fr["draws"]
        want = model.low_variance_indices(old["weight"], copies, u) if has_u else []
        state = model.filtered_state(old)
        for nudge in (-4, 4):
            moved = dict(old)
            moved["weight"] = model.nudge(old["weight"], nudge)
            assert model.low_variance_indices(moved["weight"], copies, u) == want or not has_u, (f, nudge)
            assert model.filtered_state(moved) == state, (f, nudge)


MOVING = [(60 + 3 * k, 40 + 2 * k) for k in range(9)]   # the first frame initialises the tracker, eight are processed
JUMPING = [(32, 32), (32, 32), (34, 32), (36, 33), (120, 88), (120, 88), (121, 88), (122, 89), (123, 89)]


@pytest.mark.parametrize("sliding", [1, 0], ids=["heat", "patches"])
def test_routes_agree(tmp_path, sliding):
    generic = _run(tmp_path, MOVING, device=False, sliding=sliding)
    device = _run(tmp_path, MOVING, device=True, sliding=sliding)
    _stable_under_four_ulp(generic)
    reinit = [f for f, fr in enumerate(generic) if len(set(fr["gen"]["cluster_id"].tolist())) == 1 and fr["draws"][3] > 0]
    _compare_routes(generic, device)
    assert sum(fr["found"] for fr in generic) >= 4
    for f, fr in enumerate(generic):   # every frame replays from the dumped draws: the device route's samples are the model's
        if f == 0 or f in reinit or (f - 1) in reinit:
            continue
        has_u, u, copies, fresh = fr["draws"]
        old = device[f - 1]["gen"]
        first = int(fr["gen"]["cluster_id"][copies]) if fresh else 0
        new, _ = model.sample(old, copies + fresh, copies, u, fr["d"], fr["f"], first)
        for k in ("x", "y", "size", "vx", "vy", "vsize", "cluster_id"):
            assert new[k].tobytes() == device[f]["gen"][k].tobytes(), (f, k)


def test_reinitialisation_on_both_routes(tmp_path):
    """the target jumps across the image: no sample scores above the rejection threshold, the target is lost, and with an SVM threshold
    that every heat peak passes evaluate re-initialises the samples around the peak (one new cluster for all of them) -- with the same
    draws on both routes"""
    generic = _run(tmp_path, JUMPING, device=False, rate="0.0", threshold="-100")
    device = _run(tmp_path, JUMPING, device=True, rate="0.0", threshold="-100")
    reinit = [f for f, fr in enumerate(generic) if f >= 4 and len(set(fr["gen"]["cluster_id"].tolist())) == 1 and
              fr["gen"]["cluster_id"][0] != generic[0]["gen"]["cluster_id"][0]]
    assert reinit, [sorted(set(fr["gen"]["cluster_id"].tolist()))[:4] for fr in generic]
    _compare_routes(generic, device)


def test_trajectory_adaptation_takes_the_generic_route(tmp_path):
    frames = _run(tmp_path, MOVING, device=True, adaptation="trajectory")
    assert [fr["route"] for fr in frames] == ["generic"] * 8
