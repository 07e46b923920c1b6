"""The resident frame of the integral-feature models with an optical-flow transition, the parts that need no device:
tests/resident_model.py against hand-computed cases and against tests/optflow_model.py, the host-only fd_sample_maps_apply against the
Python maps, the declarations of the C ABI, and the two frame pairs of the GPU chain test under the flow model (so that the chain
cannot lose one of its branches without this file noticing)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import condensation_model as cm
import optflow_model as fm
import resident_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_map_arithmetic():
    assert model.map_integral((10, 20, 30, 41)) == (10, 21, 31, 42)
    assert model.map_integral((-3, -4, 7, 8)) == (-2, -4, 8, 9)
    assert model.map_integral((0, 0, 0, -1)) == (0, 1, 1, 0)            # C++: -1 % 2 == -1, which is not 0
    # halves go to the even neighbour: 0.5 * 5 = 2.5 -> 2, 0.5 * 7 = 3.5 -> 4, 1.5 * 3 = 4.5 -> 4, 1.5 * 5 = 7.5 -> 8
    assert model.map_resize((0, 0, 5, 7), 0.5) == (0, 0, 2, 4)
    assert model.map_resize((0, 0, 3, 5), 1.5) == (0, 0, 4, 8)
    assert model.map_resize((10, -10, 5, 7), 1.0, 0.5, -0.5) == (12, -14, 5, 7)   # 12.5 -> 12, -13.5 -> -14
    # the apps read the scale as a float: 15 * 1.1f = 16.5000004 -> 17, the double 1.1 gives 16.5 -> 16
    assert model.map_resize((0, 0, 15, 15), float(F(1.1)))[2] == 17 and model.map_resize((0, 0, 15, 15), 1.1)[2] == 16
    chain = [(model.RESIZE, float(F(1.1))), (model.INTEGRAL,)]
    assert model.apply_maps(chain, [(40, 30, 15, 20)]).tolist() == [[41, 30, 18, 23]]   # (40, 30, 17, 22) -> odd width moves x
    assert model.apply_maps([], [(1, 2, 3, 4)]).tolist() == [[1, 2, 3, 4]]
    gen = cm.generation(2, x=[5, 6], y=[7, 8], size=[10, 15])
    assert model.sample_xywh(gen, 1.5).tolist() == [[5, 7, 10, 15], [6, 8, 15, 22]]   # 22.5 -> 22


def _map_cases():
    rng = np.random.default_rng(3)
    s = np.stack([rng.integers(-50, 200, 300), rng.integers(-50, 200, 300), rng.integers(0, 120, 300), rng.integers(0, 120, 300)], 1)
    # factor * width on k + 0.5 for even and odd k, negative coordinates, odd and even sizes, empty and negative sizes
    halves = [(0, 0, 5, 7), (0, 0, 1, 3), (-7, -9, 9, 11), (3, -4, 13, 15), (-1, -1, 0, 0), (5, 5, -3, -4), (2, 2, 2, 4)]
    return np.concatenate([s, np.array(halves)]).astype(np.int32)


@pytest.mark.parametrize("maps", [[], [("integral",)], [("resize", 0.5)], [("resize", 1.5, 0.5, -0.5)], [("resize", float(F(1.1))), ("integral",)],
                                  [("integral",), ("resize", 2.5, -0.25, 0.75), ("integral",), ("resize", 0.5)]],
                         ids=["none", "integral", "half", "offsets", "default-chain", "four"])
def test_sample_maps_apply_equals_the_model(capi, maps):
    s = _map_cases()
    got = capi.sample_maps_apply(maps, s)
    want = model.apply_maps(maps, s)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:5]
    if maps and maps[0] == ("resize", 0.5):
        assert got[300].tolist() == [0, 0, 2, 4] and got[301].tolist() == [0, 0, 0, 2]   # 2.5 -> 2, 3.5 -> 4, 0.5 -> 0, 1.5 -> 2


def test_sample_maps_saturate_alike(capi):
    """a product that leaves the int range: the library saturates where a plain conversion would wrap, as the device's conversion does"""
    s = np.array([(5, -7, 100, 300), (2 ** 30, -2 ** 30, 2 ** 30, 3)], np.int32)
    for maps in ([("resize", 1e9)], [("resize", -1e9, 4.0, -4.0)], [("resize", float("nan"), float("inf"), 0.5)]):
        got, want = capi.sample_maps_apply(maps, s), model.apply_maps(maps, s)
        assert np.array_equal(got, want), (maps, got, want)
    assert capi.sample_maps_apply([("resize", 1e9)], s)[0].tolist() == [5, -7, 2 ** 31 - 1, 2 ** 31 - 1]
    assert capi.sample_maps_apply([("resize", -1e9, 4.0, -4.0)], s)[1].tolist() == [2 ** 31 - 1, -2 ** 30 - 12, -2 ** 31, -2 ** 31]


def test_sample_maps_apply_arguments(capi):
    lib = capi.lib()
    s = np.zeros((2, 4), np.int32)
    bad = capi.FD_ERR_INVALID_ARGUMENT
    five = capi.sample_maps([("integral",)] * 5)
    assert lib.fd_sample_maps_apply(five, 5, 2, s.ctypes.data_as(ctypes.c_void_p)) == bad
    assert lib.fd_sample_maps_apply(capi.sample_maps([(7,)]), 1, 2, s.ctypes.data_as(ctypes.c_void_p)) == bad
    assert lib.fd_sample_maps_apply(None, 1, 0, None) == bad and lib.fd_sample_maps_apply(None, 0, 1, None) == bad
    assert lib.fd_sample_maps_apply(None, 0, 0, None) == capi.FD_OK and not s.any()


def test_classifier_weighing_sets_the_weight():
    gen = cm.generation(4, weight=[2.0, 5.0, 0.25, 1.0])
    out, best = model.weigh_classifier(gen, [1, 0, 1, 1], [0.5, 9.0, 0.25, -3.0], 0.0, -2.0, 0.25)
    assert out["weight"][0] == 1.0 / (1.0 + np.exp(-1.0)) and out["weight"][1] == 0 and out["score"][1] == 0   # set, not 2.0 * p
    assert out["target"].tolist() == [1, 0, 1, 0] and best == 0.5                                              # 0.25 >= 0.25
    assert out["weight"][3] == np.exp(-6.0) / (1.0 + np.exp(-6.0))
    out, best = model.weigh_classifier(gen, [0, 0, 0, 0], [1.0] * 4, 0.0, -2.0, 0.25)
    assert not out["weight"].any() and not out["target"].any() and best == 0.0


def _check_motion(tracks):
    got, want = model.motion(*tracks), fm.median(*tracks)
    assert model.same_motion(got, want), (got, {k: v for k, v in want.items() if k != "order"})
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 64, 65, 257])
def test_motion_equals_the_sorting_model(n):
    got = _check_motion(model.crafted_tracks(n, 100 + n))
    assert got["ok"] == (n >= 2)
    if n >= 64:
        # the shift plus the zoom's share at the median point (0.03 * up to +-100 px, about +-0.5 px at these counts), and the zoom
        assert abs(got["median_x"] - 1.5) < 1.0 and abs(got["median_y"] + 0.75) < 1.0 and abs(got["median_ratio"] - 1.03) < 0.02
    for n_valid, n_correct in ((n // 2, n // 2), (n // 2 - 1, n // 2 - 1), (n, n // 2), (n, n // 2 - 1)):
        if n_correct >= 0:
            got = _check_motion(model.crafted_tracks(n, 200 + n, n_valid, n_correct))
            assert got["ok"] == (n_valid >= n // 2 and n_correct >= n // 2 and n_correct >= 2)


def test_motion_edge_cases():
    pts, fwd, bwd, fst, bst = model.crafted_tracks(8, 5)
    pts[1], pts[2] = (64, 32), (0, 0)             # so that adding 0.5 and its successor is exact
    bwd[:] = pts
    bwd[0, 0] = pts[0, 0] + np.sqrt(F(0.5))       # may or may not exceed 0.5f after squaring: both models use the same float product
    bwd[1] = pts[1] + np.array([0.5, 0.5], F)     # d = 0.5f exactly: correct
    bwd[2] = pts[2] + np.array([0.5, np.nextafter(F(0.5), F(1))], F)   # d = the successor of 0.5f: not correct
    assert (bwd[1] - pts[1]).tolist() == [0.5, 0.5] and float(F(0.25) + (bwd[2, 1] - pts[2, 1]) ** 2) == float(np.nextafter(F(0.5), F(1)))
    got = _check_motion((pts, fwd, bwd, fst, bst))
    assert got["n_valid"] == 8 and got["n_correct"] in (6, 7)
    fwd[3, 0] = np.nan                            # a NaN flow of a correct pair sorts last
    _check_motion((pts, fwd, bwd, fst, bst))
    fwd[:] = pts + np.array([2, -1], F)           # equal flows: every ratio is 1
    got = _check_motion((pts, fwd, bwd, fst, bst))
    assert got["ok"] and got["median_x"] == 2 and got["median_y"] == -1 and got["median_ratio"] == 1
    bwd[4, 1] = np.nan                            # a NaN distance: not tracked
    assert _check_motion((pts, fwd, bwd, fst, bst))["n_valid"] == 7
    for n in (2, 3):                              # one correct pair of two or three: enough pairs, no ratio
        t = model.crafted_tracks(n, 9, n, 1)
        got = _check_motion(t)
        assert got["n_correct"] == 1 and not got["ok"]


def test_flow_prediction():
    mot = dict(ok=True, median_x=F(2.5), median_y=F(-1.25), median_ratio=F(1.05))
    # the sample's own velocity is replaced: 2.5 + 0 -> 3 (away from zero), -1.25 - 0.25 = -1.5 -> -2; 10 * 1.05f = 10.5f -> 11
    assert model.predict_flow(10, 20, 10, mot["median_x"], mot["median_y"], mot["median_ratio"], 0.0, -0.25, 1.0) == (13, 18, 11, 3, -2, F(1.05))
    old = cm.generation(3, x=[10, 20, 30], y=[5, 6, 7], size=[10, 20, 30], vx=[9, 9, 9], vy=[-9, -9, -9], vsize=[2, 2, 2], weight=[1, 1, 1], cluster_id=[4, 5, 6])
    flow_d, fall_d = np.array([[0.0, 0.0, 1.0]] * 3), np.array([[1.0, 1.0, 1.0]] * 3)
    fresh = np.array([[1, 2, 3]], np.int32)
    new, source = model.sample_flow(old, mot, 4, 3, 0.5, flow_d, fall_d, fresh, 50)
    assert source.tolist() == [0, 1, 2, -1] and new["x"].tolist() == [13, 23, 33, 1] and new["vx"].tolist() == [3, 3, 3, 0]
    assert new["size"].tolist() == [11, 21, 31, 3] and new["cluster_id"].tolist() == [4, 5, 6, 50]   # 10.5f -> 11; 30 * 1.05f = 31.499998f -> 31
    mot["ok"] = False
    new2, source2 = model.sample_flow(old, mot, 4, 3, 0.5, flow_d, fall_d, fresh, 50)
    want, _ = cm.sample(old, 4, 3, 0.5, fall_d, fresh, 50)
    assert all(np.array_equal(new2[k], want[k]) for k in cm.FIELDS) and new2["vx"].tolist() == [10, 10, 10, 0]


def test_header_declares_the_resident_calls():
    hdr = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    for name in ("fd_particles_create_unbound", "fd_sample_maps_apply", "fd_particles_evaluate_integral", "fd_particles_weigh_classifier",
                 "fd_flow_track_fb_resident", "fd_flow_get_tracks", "fd_debug_flow_motion", "fd_particles_sample_flow", "fd_particles_state_flow"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    src = ('#include "fd_hip.h"\n'
           'typedef char info_is_64[sizeof(fd_particles_info) == 64 ? 1 : -1];\n'
           'typedef char motion_is_24[sizeof(fd_flow_motion_info) == 24 ? 1 : -1];\n'
           'typedef char map_is_32[sizeof(fd_sample_map) == 32 ? 1 : -1];\n'
           'int main(void) { fd_sample_map m; fd_flow_motion_info i; m.kind = FD_SAMPLE_MAP_INTEGRAL; m.factor = m.x_offset = m.y_offset = 0; i.ok = 0;\n'
           '  i.median_ratio = 1.f; return m.kind - FD_SAMPLE_MAP_RESIZE - 1 + i.ok + (FD_FLOW_RESIDENT_MAX_POINTS - 1024) + (FD_SAMPLE_MAPS_MAX - 4); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)


def test_binding_matches_the_structs(capi):
    assert ctypes.sizeof(capi.fd_particles_info) == 64 and capi.fd_particles_info.best_score.offset == 48
    assert ctypes.sizeof(capi.fd_flow_motion_info) == 24 and capi.fd_flow_motion_info.median_x.offset == 12
    assert ctypes.sizeof(capi.fd_sample_map) == 32 and capi.fd_sample_map.factor.offset == 8
    assert (capi.FD_SAMPLE_MAP_RESIZE, capi.FD_SAMPLE_MAP_INTEGRAL, capi.FD_SAMPLE_MAPS_MAX, capi.FD_FLOW_RESIDENT_MAX_POINTS) == (0, 1, 4, 1024)
    assert capi.FD_SAMPLE_MAPS_MAX == model.MAX_MAPS and capi.FD_FLOW_RESIDENT_MAX_POINTS == model.MAX_POINTS
    lib = capi.lib()
    bad = capi.FD_ERR_INVALID_ARGUMENT
    # NULL handles are refused before anything is touched
    assert lib.fd_particles_create_unbound(None, 4, None) == bad
    assert lib.fd_particles_evaluate_integral(None, None, None, 0, None, None, 1.0, None, 0) == bad
    assert lib.fd_particles_weigh_classifier(None, None, 0.0, 0.0, 0.0) == bad
    assert lib.fd_flow_track_fb_resident(None, None, None, 0) == bad
    assert lib.fd_flow_get_tracks(None, None, 0, None, None, None, None, None, None, None, None) == bad
    assert lib.fd_debug_flow_motion(None, None, None, None, None, None, None, 0, None) == bad
    assert lib.fd_particles_sample_flow(None, None, None, 0, 0, 0.0, None, None, None, 0) == bad
    assert lib.fd_particles_state_flow(None, None, None, None, None) == bad


@pytest.fixture(scope="module")
def chain_pairs():
    """the model's tracks of the 10 x 10 grid on the chain's target over its shifted pair (frames 0 -> 1) and its unrelated pair (2 -> 3)"""
    frames = model.chain_frames()
    out = {}
    for name, (a, b) in (("shifted", (0, 1)), ("unrelated", (2, 3))):
        x, y, size = model.CHAIN_TARGET
        x, y = x + model.CHAIN_SHIFT[0] * a, y + model.CHAIN_SHIFT[1] * a
        pts = model.chain_points(x, y, size)
        prev, cur = fm.build_pyramid(frames[a], 15, 15, 2), fm.build_pyramid(frames[b], 15, 15, 2)
        fwd, fst, _ = fm.track(prev, cur, pts, 15, 15)
        bwd, bst, _ = fm.track(cur, prev, fwd, 15, 15)
        out[name] = (pts, fwd, bwd, fst, bst)
    return out


def test_chain_frames_take_both_branches(chain_pairs):
    shifted = _check_motion(chain_pairs["shifted"])
    assert shifted["ok"] and abs(shifted["median_x"] - 2) < 0.1 and abs(shifted["median_y"] - 1) < 0.1 and abs(shifted["median_ratio"] - 1) < 0.01
    assert len(chain_pairs["shifted"][0]) <= 100
    unrelated = _check_motion(chain_pairs["unrelated"])
    assert not unrelated["ok"]
