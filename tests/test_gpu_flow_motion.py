"""k_flow_motion (the median flow of a resident track) through fd_debug_flow_motion against the host's fd_flow_median on
the same arrays: the counts and the bit patterns of the three medians are compared exactly (a median that is a NaN is any NaN: the
device reports the default one).  The cases sit on both sides of every threshold of the rule -- n / 2 valid pairs, n / 2 correct
pairs, two correct pairs, a distance of exactly 0.5f -- and on odd and even counts, ties and NaN."""
import numpy as np
import pytest

import resident_model as model

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [0, 1, 2, 3, 4, 5, 64, 65, 257, 1024]


@pytest.fixture(scope="module")
def flow(capi, ctx):
    f = capi.Flow(ctx, 64, 48)
    yield f
    f.close()


def _check(capi, flow, tracks):
    """the device, the host's fd_flow_median and the sort-free model agree; returns the device's motion"""
    got = flow.debug_motion(*tracks)
    want = capi.flow_median(*tracks)
    assert model.same_motion(got, want), (got, {k: v for k, v in want.items() if k != "order"})
    assert model.same_motion(got, model.motion(*tracks))
    return got


@pytest.mark.parametrize("n", SIZES)
def test_seeded_tracks(capi, flow, n):
    got = _check(capi, flow, model.crafted_tracks(n, 100 + n))
    assert got["ok"] == (n >= 2) and got["n_valid"] == got["n_correct"] == n
    if n >= 64:
        assert abs(got["median_ratio"] - 1.03) < 0.02


@pytest.mark.parametrize("n", SIZES)
def test_both_sides_of_the_counts(capi, flow, n):
    """exactly n / 2 valid pairs and one fewer; exactly n / 2 correct pairs and one fewer; odd and even numbers of correct pairs"""
    half = n // 2
    for n_valid, n_correct in ((half, half), (half - 1, half - 1), (n, half), (n, half - 1), (n, max(n - 1, 0)), (max(n - 1, 0), max(n - 2, 0))):
        if n_correct < 0:
            continue
        got = _check(capi, flow, model.crafted_tracks(n, 200 + n, n_valid, n_correct))
        enough = n_valid >= half
        assert got["n_valid"] == n_valid and got["n_correct"] == (n_correct if enough else 0)
        assert got["ok"] == (enough and n_correct >= half and n_correct >= 2)


@pytest.mark.parametrize("n", [2, 3])
def test_one_correct_pair(capi, flow, n):
    got = _check(capi, flow, model.crafted_tracks(n, 9, n, 1))
    assert got["n_correct"] == 1 and not got["ok"] and got["median_ratio"] == 1


def test_distance_on_the_threshold(capi, flow):
    pts, fwd, bwd, fst, bst = model.crafted_tracks(9, 5)
    pts[1], pts[2] = (64, 32), (0, 0)             # adding 0.5 and its successor is exact there
    bwd[:] = pts
    bwd[1] = pts[1] + np.array([0.5, 0.5], F)     # d = 0.5f: correct
    bwd[2] = pts[2] + np.array([0.5, np.nextafter(F(0.5), F(1))], F)   # d = the successor of 0.5f: not correct
    got = _check(capi, flow, (pts, fwd, bwd, fst, bst))
    assert got["n_valid"] == 9 and got["n_correct"] == 8 and got["ok"]
    bwd[2, 1] = F(0.5)                            # back on the threshold
    assert _check(capi, flow, (pts, fwd, bwd, fst, bst))["n_correct"] == 9


@pytest.mark.parametrize("n", [5, 64, 257, 1024])
def test_ties_and_nan(capi, flow, n):
    pts, fwd, bwd, fst, bst = model.crafted_tracks(n, 300 + n)
    fwd[:] = pts + np.array([2, -1], F)           # equal flows: every ratio of a pair is 1 up to the rounding of the sums
    got = _check(capi, flow, (pts, fwd, bwd, fst, bst))
    assert got["ok"] and abs(got["median_x"] - 2) < 1e-4 and abs(got["median_y"] + 1) < 1e-4 and abs(got["median_ratio"] - 1) < 1e-4
    grid = np.stack(np.meshgrid(np.arange(32, dtype=F), np.arange(32, dtype=F)), -1).reshape(-1, 2)[:n] * F(4)
    got = _check(capi, flow, (grid, grid + np.array([3, 5], F), grid.copy(), fst, bst))   # exact arithmetic: all flows and ratios tie
    assert got["median_x"] == 3 and got["median_y"] == 5 and got["median_ratio"] == 1
    fwd[n // 3, 0] = np.nan                       # a NaN in fwd with both status bytes set: its flow and its ratios sort last
    got = _check(capi, flow, (pts, fwd, bwd, fst, bst))
    assert got["ok"] and got["n_correct"] == n and got["median_x"] == got["median_x"]
    fwd[:, 1] = np.nan                            # more than half of the y flows and of the ratios are NaN: so are their medians
    got = _check(capi, flow, (pts, fwd, bwd, fst, bst))
    assert got["ok"] and got["median_y"] != got["median_y"] and got["median_ratio"] != got["median_ratio"] and got["median_x"] == got["median_x"]
    bwd[n // 2, 1] = np.nan                       # a NaN distance: the pair is not tracked
    assert _check(capi, flow, (pts, fwd, bwd, fst, bst))["n_valid"] == n - 1
    same = np.tile(np.array([[64, 32]], F), (n, 1))   # coinciding points: every ratio is 0 / 0
    got = _check(capi, flow, (same, same + F(1), same.copy(), fst, bst))
    assert got["ok"] and got["median_x"] == 1 and got["median_ratio"] != got["median_ratio"]


def test_zero_flows_of_both_signs(capi, flow):
    """the host's comparison does not order -0 and +0, so fd_flow_median may report either; the device's key puts -0 first (DESIGN.md
    4.7): the median is the same number, and its sign is the one that order gives"""
    pts = np.array([[0, 0], [0, 8], [0, 16], [0, 24], [0, 32]], F)
    for negative, sign in ((3, True), (2, False)):      # rank 5 / 2 = 2 of [-0 x negative, +0 ...]
        fwd = pts + np.array([0, 1], F)
        fwd[:negative, 0] = -0.0
        assert np.signbit(fwd[:negative, 0] - pts[:negative, 0]).all() and not np.signbit(fwd[negative:, 0] - pts[negative:, 0]).any()
        tracks = (pts, fwd, pts.copy(), np.ones(5, np.uint8), np.ones(5, np.uint8))
        got, want = flow.debug_motion(*tracks), capi.flow_median(*tracks)
        assert got["ok"] and want["ok"] and got["median_x"] == want["median_x"] == 0 and bool(np.signbit(got["median_x"])) == sign
        assert got["median_y"].tobytes() == want["median_y"].tobytes() and got["median_ratio"].tobytes() == want["median_ratio"].tobytes()


def test_too_many_points_are_refused_before_a_launch(capi, ctx, flow):
    n = capi.FD_FLOW_RESIDENT_MAX_POINTS + 1
    z, s = np.zeros((n, 2), F), np.ones(n, np.uint8)
    with pytest.raises(capi.FdError) as e:
        flow.debug_motion(z, z, z, s, s)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError) as e:
        flow.track_fb_resident(z)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        flow.debug_motion(z, z[:5], z, s, s)
    fresh = capi.Flow(ctx, 64, 48)
    with pytest.raises(capi.FdError) as e:        # no frames yet: nothing to track between
        fresh.track_fb_resident(z[:4])
    assert e.value.code == capi.FD_ERR_RUNTIME
    with pytest.raises(capi.FdError) as e:        # and no resident track to report
        fresh.get_tracks()
    assert e.value.code == capi.FD_ERR_RUNTIME
    fresh.close()
