"""The numpy model of the pyramidal Lucas-Kanade flow (tests/optflow_model.py) against a known motion, against the
project's oracle where the two overlap, and over the cases of the GPU test: every exit of the tracker must occur in them.  No GPU."""
import numpy as np
import pytest

import optflow_model as M


@pytest.fixture(scope="module")
def rolled():
    """the 10 x 10 circle grid on a 64 x 64 target, tracked forward and back between a frame and its roll by (3, -2)"""
    base = M.textured()
    moved = np.roll(base, (-2, 3), axis=(0, 1))
    prev, cur = M.build_pyramid(base, 15, 15, 2), M.build_pyramid(moved, 15, 15, 2)
    pts = M.grid_points()
    fwd, fst, ftrace = M.track(prev, cur, pts, 15, 15)
    bwd, bst, _ = M.track(cur, prev, fwd, 15, 15)
    return pts, fwd, fst, bwd, bst, ftrace, prev


def test_known_motion(rolled):
    pts, fwd, fst, bwd, bst, ftrace, prev = rolled
    assert len(prev) == 3 and [(l["w"], l["h"]) for l in prev] == [(160, 128), (80, 64), (40, 32)]
    assert len(pts) == 80   # the 10 x 10 grid without the 20 points outside the circle
    assert fst.all() and bst.all()
    flow = fwd - pts
    print("largest deviation from (3, -2): %.6f px" % np.abs(flow - np.array([3, -2], np.float32)).max())
    assert np.abs(flow - np.array([3, -2], np.float32)).max() < 0.1   # steps stop at 0.01 px
    back = bwd - pts
    d2 = back[:, 0] * back[:, 0] + back[:, 1] * back[:, 1]
    print("largest squared forward-backward distance: %.3g" % d2.max())
    assert d2.max() < 0.01
    assert (ftrace[:, :3, 0] > 0).all()   # every level iterated


def test_median_of_the_known_motion(rolled):
    pts, fwd, fst, bwd, bst, _, _ = rolled
    m = M.median(pts, fwd, bwd, fst, bst)
    assert m["ok"] and m["n_valid"] == len(pts) and m["n_correct"] == len(pts)
    flow = fwd - pts
    assert m["median_x"] == np.sort(flow[:, 0])[len(pts) // 2] and m["median_y"] == np.sort(flow[:, 1])[len(pts) // 2]
    ratios = []
    order = m["order"]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            before, after = pts[order[a]] - pts[order[b]], fwd[order[a]] - fwd[order[b]]
            ratios.append((after[0] * after[0] + after[1] * after[1]) / (before[0] * before[0] + before[1] * before[1]))
    assert m["median_ratio"] == np.sqrt(np.sort(np.array(ratios, np.float32))[len(ratios) // 2])
    back = bwd - pts
    d2 = back[:, 0] * back[:, 0] + back[:, 1] * back[:, 1]
    assert np.array_equal(order, np.lexsort((np.arange(len(pts)), d2)))


def test_pyramid_primitives_equal_the_oracle(oracle):
    rng = np.random.default_rng(3)
    for shape in ((128, 160), (17, 33), (5, 9), (48, 64), (3, 4)):
        a = rng.integers(0, 256, shape).astype(np.uint8)
        assert np.array_equal(M.pyr_down(a), oracle.pyrdown(a)), shape
    bgr = rng.integers(0, 256, (20, 30, 3)).astype(np.uint8)
    assert np.array_equal(M.bgr2gray(bgr), oracle.bgr2gray(bgr))


def test_truncation_rule():
    img = M.textured(64, 48, seed=2)
    assert [(l["w"], l["h"]) for l in M.build_pyramid(img, 15, 15, 2)] == [(64, 48), (32, 24)]   # 16 x 12 does not exceed the window
    assert [(l["w"], l["h"]) for l in M.build_pyramid(img[:17, :33], 5, 7, 2)] == [(33, 17), (17, 9)]
    level = M.build_pyramid(img, 15, 15, 0)[0]
    assert level["img"].shape == (48 + 30, 64 + 30) and level["der"].shape == (78, 94, 2)
    assert (level["img"][:15, :15] == img[0, 0]).all() and (level["der"][-15:, -15:] == level["der"][-16, -16]).all()


def test_scharr_of_a_ramp():
    ramp = np.tile(np.arange(0, 60, 3, dtype=np.uint8), (8, 1))   # dx = 3 per pixel: (3 + 10 + 3) * 2 * 3 inside, 0 at the reflected ends
    d = M.scharr(ramp)
    assert (d[:, 1:-1, 0] == 96).all() and (d[:, [0, -1], 0] == 0).all() and (d[..., 1] == 0).all()


def test_every_exit_occurs_in_the_gpu_cases():
    """keeps the GPU comparison from passing on a kernel that never iterates: over the cases it compares, the model itself takes
    every exit, the count exit in a case with max_count 2, and iterates on every level"""
    seen = {}
    for name in M.CASES:
        _, _, trace = M.reference(name)
        nlev = len(M.pyramids(*M.CASES[name][:4])[0])
        assert (trace[:, nlev:, 1] == M.EXIT_NONE).all() and (trace[:, :nlev, 1] != M.EXIT_NONE).all()
        for level in range(nlev):
            for reason in np.unique(trace[:, level, 1]):
                seen.setdefault(int(reason), set()).add(name)
    print({M.EXIT_NAMES[r]: sorted(names) for r, names in seen.items()})
    for reason in (M.EXIT_SKIP_RANGE, M.EXIT_SKIP_EIGEN, M.EXIT_EPS, M.EXIT_OSCILLATION, M.EXIT_COUNT, M.EXIT_LEFT_RANGE):
        assert reason in seen, M.EXIT_NAMES[reason]
    _, _, trace = M.reference("zoom-15x15-count2-n64")
    assert (trace[..., 1] == M.EXIT_COUNT).any() and trace[..., 0].max() == 2
    _, status, trace = M.reference("roll-15x15-mixed")
    assert trace[..., 0].max() > 2 and 0 < status.sum() < len(status)
