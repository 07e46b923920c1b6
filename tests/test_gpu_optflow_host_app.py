"""tracker_app with `transition opticalFlow` (condensation::OpticalFlowTransitionModel on fd_flow) over eight 176 x 144 frames after the
one it is initialised on.  A textured scene that moves by integer steps: the flow predicts every frame, its traced motion is the
model's (tests/optflow_model.py) on the same frames and target, and the samples are a replay of the dumped draws.  A flat target on a
flat scene: no window has a gradient, the fallback predicts every frame, and the run equals `transition simple` with the fallback's
deviations line by line."""
import os
import subprocess

import numpy as np
import pytest

import condensation_model as cmodel
import optflow_model as M
from test_condensation_host import _dumped_generation

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
W, H = 176, 144
POSITION_DEVIATION, SIZE_DEVIATION = 2.0, 0.03

CONFIG = """tracking {
    transition %(transition)s
    adaptive { resampling { particleCount 120 randomRate 0.25 minSize 20 maxSize 80 } }
    initialCount 120
    seed 5
    measurement ehog {
        cellSize 4 cellCount 12 signedAndUnsigned 1 interpolateBins 0 interpolateCells 1 octaveLayerCount 2
        rejectionThreshold -0.5 useSlidingWindow 1 conservativeReInit 0
        negativeExampleCount 10 initialNegativeExampleCount 40 randomExampleCount 40 negativeScoreThreshold -1.0
        adaptation position adaptationThreshold 0.25 exclusionThreshold 0.0
        classifier { training { c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.0 logisticB -2.0 threshold 0 }
    }
}
"""
FLOW = "opticalFlow { positionDeviation %s sizeDeviation %s fallback simple { positionDeviation 3 sizeDeviation 0.04 } }" % (POSITION_DEVIATION, SIZE_DEVIATION)
SIMPLE = "simple { positionDeviation 3 sizeDeviation 0.04 }"


def _textured_frame(k):
    """a blurred-noise scene with a high-contrast blob in it, everything moved by (3 k, 2 k)"""
    base = (M.textured(W, H, seed=21).astype(np.int32) - 128) // 2 + 128
    yy, xx = np.mgrid[0:40, 0:30]
    blob = (128 + 100 * np.sin(xx / 2.5) * np.cos(yy / 3.5)).astype(np.uint8)
    base[40:80, 60:90] = blob
    gray = np.roll(base.astype(np.uint8), (2 * k, 3 * k), axis=(0, 1))
    return np.repeat(gray[:, :, None], 3, axis=2)


def _flat_frame(k):
    """a flat bright rectangle of 60 x 80 on a flat scene, moved by (2 k, k): an edge for the HOG cells, no gradient for the flow windows"""
    frame = np.full((H, W, 3), 90, np.uint8)
    frame[30 + k:110 + k, 50 + 2 * k:110 + 2 * k] = 200
    return frame


def _run(tmp_path, frames, box, transition, device=False):
    config = tmp_path / ("tracking_%s.cfg" % transition.split()[0])
    config.write_text(CONFIG % dict(transition=transition))
    paths = []
    for k, frame in enumerate(frames):
        path = tmp_path / ("frame%d.ppm" % k)
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (W, H))
            f.write(frame.tobytes())
        paths.append(str(path))
    env = dict(os.environ, FD_COND_DEVICE="1" if device else "0")
    run = subprocess.run([APP, "--dump", str(config)] + [str(v) for v in box] + paths, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.startswith("init 1 %d %d %d %d" % tuple(box)), run.stdout[:200]
    return run.stdout


def _parse(text):
    frames, cur = [], None
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            cur = dict(found=int(t[3]), box=tuple(int(v) for v in t[4:8]), route=t[11], flow=None, draws=None, z=[], d=[], f=[], s=[])
            frames.append(cur)
        elif t[0] == "flow":
            cur["flow"] = dict(used=int(t[1]), tracked=int(t[3]), valid=int(t[5]), correct=int(t[7]), motion=tuple(np.float32(v) for v in t[9:12]))
        elif t[0] == "draws":
            cur["draws"] = (int(t[2]), float(t[3]), int(t[5]), int(t[7]))
        elif t[0] in ("z", "d"):
            cur[t[0]].append(tuple(float(v) for v in t[1:4]))
        elif t[0] == "f":
            cur["f"].append(tuple(int(v) for v in t[1:4]))
        elif t[0] == "s":
            cur["s"].append(t[1:])
    for fr in frames:
        fr["gen"] = _dumped_generation(fr["s"])
    return frames


def _state_of(box):
    """the Sample behind a printed box: (x, y, width, height)"""
    x, y, w, h = box
    return x + w // 2, y + h // 2, w, h


def test_flow_predicts_every_frame(tmp_path):
    images = [_textured_frame(k) for k in range(9)]
    # the resident particle set is asked for, and the route stays the generic one: that set knows SimpleTransitionModel only
    frames = _parse(_run(tmp_path, images, (60, 40, 30, 40), FLOW, device=True))
    assert len(frames) == 8 and all(fr["route"] == "generic" for fr in frames)
    assert [fr["flow"]["used"] for fr in frames] == [1] * 8, [(fr["found"], fr["flow"]) for fr in frames]
    template = M.grid(10, 10, True)
    pyramids = [M.build_pyramid(img, 15, 15, 2) for img in images]
    target = (60 + 15, 40 + 20, 30, 40)   # the state AdaptiveCondensationTracker::initialize makes of the box
    previous = None                        # the generation before the frame: initialCount copies of the state
    for f, fr in enumerate(frames):
        # the traced motion is the model's, from the frames and the target the tracker had
        pts = M.target_points(template, *target)
        fwd, fst, _ = M.track(pyramids[f], pyramids[f + 1], pts, 15, 15)
        bwd, bst, _ = M.track(pyramids[f + 1], pyramids[f], fwd, 15, 15)
        m = M.median(pts, fwd, bwd, fst, bst)
        assert m["ok"] and (fr["flow"]["valid"], fr["flow"]["correct"]) == (m["n_valid"], m["n_correct"]), (f, fr["flow"], m)
        assert [v.view(np.uint32) for v in fr["flow"]["motion"]] == [np.float32(m[k]).view(np.uint32) for k in ("median_x", "median_y", "median_ratio")], (f, fr["flow"], m)
        assert abs(m["median_x"] - 3) < 0.5 and abs(m["median_y"] - 2) < 0.5   # and it is the motion of the scene
        # the samples are a replay of the draws
        has_u, u, copies, fresh = fr["draws"]
        gen = fr["gen"]
        assert copies + fresh == len(gen["x"]) == 120 and len(fr["z"]) == copies and not fr["d"] and len(fr["f"]) == fresh
        if previous is None:
            old = cmodel.generation(120, x=[target[0]] * 120, y=[target[1]] * 120, size=[target[2]] * 120)
        else:
            old = previous
        picks = cmodel.low_variance_indices(old["weight"], copies, u)
        assert len(picks) == copies == 90
        for i, k in enumerate(picks):
            want = M.apply_motion((int(old["x"][k]), int(old["y"][k]), int(old["size"][k])), m, POSITION_DEVIATION, SIZE_DEVIATION, fr["z"][i])
            got = (int(gen["x"][i]), int(gen["y"][i]), int(gen["size"][i]), int(gen["vx"][i]), int(gen["vy"][i]), np.float32(gen["vsize"][i]))
            assert got == want, (f, i, got, want)
        for j, (x, y, size) in enumerate(fr["f"]):
            assert (int(gen["x"][copies + j]), int(gen["y"][copies + j]), int(gen["size"][copies + j])) == (x, y, size)
        # the box is the state of the dumped generation
        state = cmodel.filtered_state(gen)
        assert fr["found"] == (state is not None), f
        assert fr["found"], "frame %d lost the target: the next frame would fall back" % f
        height = cmodel.cv_round(40.0 / 30.0 * state[2])
        assert fr["box"] == (state[0] - state[2] // 2, state[1] - height // 2, state[2], height), (f, fr["box"], state)
        target = _state_of(fr["box"])
        previous = gen


def test_flat_frames_fall_back_and_equal_the_simple_model(tmp_path):
    images = [_flat_frame(k) for k in range(9)]
    flow_text = _run(tmp_path, images, (50, 30, 60, 80), FLOW)
    simple_text = _run(tmp_path, images, (50, 30, 60, 80), SIMPLE)
    frames = _parse(flow_text)
    assert len(frames) == 8
    assert [fr["flow"]["used"] for fr in frames] == [0] * 8
    with_target = [fr for fr in frames if fr["flow"]["tracked"]]
    assert with_target, "no frame had a target: the flow was never asked"
    assert all(fr["flow"]["valid"] < 40 for fr in with_target)   # tracked, and too few of the 80 points came back

    def comparable(text):
        out = []
        for line in text.split("\n"):
            if line.startswith("flow "):
                continue
            out.append(line.split(" ms ")[0] if line.startswith("frame ") else line)
        return out
    assert comparable(flow_text) == comparable(simple_text)
