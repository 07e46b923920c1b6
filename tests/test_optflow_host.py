"""The host-only half of the optical-flow transition model: fd_flow_grid and fd_flow_median bit for bit against the model
(tests/optflow_model.py), condensation::OpticalFlowTransitionModel on a stub that injects the tracked points, and the declarations
of the C ABI.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import optflow_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW_SYMBOLS = ("fd_flow_default_params", "fd_flow_limits", "fd_flow_create", "fd_flow_destroy", "fd_flow_levels", "fd_flow_update", "fd_flow_track",
                "fd_flow_track_fb", "fd_debug_flow_level", "fd_flow_grid", "fd_flow_median")


def test_symbols_are_declared_exported_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    for name in FLOW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, hdr) and name in capi._SIGS and hasattr(capi.lib(), name), name
    src = ('#include "fd_hip.h"\nint main(void) { fd_flow_params p; fd_flow_motion m; int a = 0, b = 0, c = 0; fd_flow_default_params(&p); m.ok = 0;'
           ' fd_flow_limits(&a, &b, &c); return p.win_w - 15 + m.ok + FD_FLOW_EXIT_LEFT_RANGE - 6 + FD_FLOW_MAX_LEVELS - 8; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)
    for cls in ("Flow",):
        for method in ("update", "track", "track_fb", "level", "levels"):
            assert hasattr(getattr(capi, cls), method)
    assert callable(capi.flow_grid) and callable(capi.flow_median)


def test_defaults_and_limits(capi):
    p = capi.flow_params()
    assert (p.win_w, p.win_h, p.max_level, p.max_count, p.epsilon, p.min_eig_threshold) == (15, 15, 2, 30, 0.01, 1e-4)
    max_points, lo, hi = capi.flow_limits()
    assert max_points >= 4096 and max_points == capi.FD_FLOW_MAX_POINTS and (lo, hi) == (3, 31)
    assert capi.FD_FLOW_MAX_LEVELS == M.MAX_LEVELS
    assert (capi.FD_FLOW_EXIT_SKIP_RANGE, capi.FD_FLOW_EXIT_SKIP_EIGEN, capi.FD_FLOW_EXIT_EPS, capi.FD_FLOW_EXIT_OSCILLATION, capi.FD_FLOW_EXIT_COUNT,
            capi.FD_FLOW_EXIT_LEFT_RANGE) == (M.EXIT_SKIP_RANGE, M.EXIT_SKIP_EIGEN, M.EXIT_EPS, M.EXIT_OSCILLATION, M.EXIT_COUNT, M.EXIT_LEFT_RANGE)


@pytest.mark.parametrize("gw,gh,circle,count", [(10, 10, True, 80), (10, 10, False, 100), (1, 1, True, 1), (3, 7, True, None), (3, 7, False, 21)])
def test_grid_equals_the_model(capi, gw, gh, circle, count):
    got, want = capi.flow_grid(gw, gh, circle), M.grid(gw, gh, circle)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if count is not None:
        assert len(got) == count


def test_grid_rejects_and_reports_capacity(capi):
    import ctypes as C
    n = C.c_int()
    out = np.zeros((4, 2), np.float32)
    assert capi.lib().fd_flow_grid(0, 3, 1, out.ctypes.data, 4, C.byref(n)) == 1            # FD_ERR_INVALID_ARGUMENT
    assert capi.lib().fd_flow_grid(10, 10, 1, out.ctypes.data, 4, C.byref(n)) == 5 and n.value == 80   # FD_ERR_CAPACITY, the count still reported
    assert np.array_equal(out, M.grid(10, 10)[:4])


def _tracked(n, seed, valid=1.0, error=0.05, flow=(2.25, -1.5), zoom=1.0625):
    """n points around (80, 64), their forward points (zoomed and moved, with noise) and backward points (off by about `error`)"""
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-30, 30, (n, 2)) + (80, 64)).astype(np.float32)
    fwd = ((pts - (80, 64)) * zoom + (80, 64) + flow + rng.normal(0, 0.2, (n, 2))).astype(np.float32)
    bwd = (pts + rng.normal(0, error, (n, 2))).astype(np.float32)
    fst = (rng.uniform(0, 1, n) < valid).astype(np.uint8)
    bst = (rng.uniform(0, 1, n) < valid).astype(np.uint8)
    return pts, fwd, bwd, fst, bst


def _median_cases():
    cases = {}
    cases["even-all-good"] = _tracked(80, 1)
    cases["odd-all-good"] = _tracked(81, 2)
    cases["some-lost-some-wrong"] = _tracked(80, 3, valid=0.9, error=0.45)
    cases["too-few-valid"] = _tracked(80, 4, valid=0.5)           # about a quarter of the pairs have both flags
    cases["too-few-correct"] = _tracked(80, 5, error=2.0)
    cases["exactly-half-valid"] = _tracked(10, 6)
    cases["exactly-half-valid"][3][:5] = 0
    cases["one-less-than-half-valid"] = _tracked(10, 7)
    cases["one-less-than-half-valid"][3][:6] = 0
    pts, fwd, bwd, fst, bst = _tracked(40, 8)                      # ties: the same offset for groups of points, in an order that is not the index order
    pts = np.rint(pts).astype(np.float32)                          # so that the offsets survive the subtraction exactly
    offsets = np.array([[0.25, 0.0], [0.0, 0.25], [-0.25, 0.0], [0.125, 0.125]], np.float32)
    bwd = pts + offsets[(np.arange(40) * 7) % 4]
    cases["ties"] = (pts, fwd, bwd.astype(np.float32), fst, bst)
    pts, fwd, bwd, fst, bst = _tracked(12, 9)                      # the cut falls on a value: 0.5 * 0.5 + 0.5 * 0.5 is exactly 0.5f and stays
    pts = np.rint(pts).astype(np.float32)
    bwd = pts + np.array([[0.5, 0.5]] * 3 + [[0.5, 0.515625]] * 3 + [[0.75, 0.0]] * 3 + [[0.0, 0.0]] * 3, np.float32)
    cases["cut-on-a-value"] = (pts, fwd, bwd.astype(np.float32), fst, bst)
    cases["two-points"] = _tracked(2, 10)
    cases["one-point"] = _tracked(1, 11)
    cases["no-point"] = _tracked(0, 12)
    pts, fwd, bwd, fst, bst = _tracked(9, 13)
    pts[4] = pts[2]                                                # two points that coincide: a 0 / 0 or x / 0 ratio
    bwd[4] = pts[4]
    cases["coincident-points"] = (pts, fwd, bwd, fst, bst)
    return cases


MEDIAN_CASES = _median_cases()


@pytest.mark.parametrize("name", sorted(MEDIAN_CASES))
def test_median_equals_the_model(capi, name):
    args = MEDIAN_CASES[name]
    got, want = capi.flow_median(*args), M.median(*args)
    assert got["ok"] == want["ok"] and got["n_valid"] == want["n_valid"] and got["n_correct"] == want["n_correct"], (got, want)
    assert np.array_equal(got["order"], want["order"])
    for field in ("median_x", "median_y", "median_ratio"):
        assert np.float32(got[field]).view(np.uint32) == np.float32(want[field]).view(np.uint32), (field, got[field], want[field])


def test_median_cases_cover_what_they_claim():
    res = {name: M.median(*args) for name, args in MEDIAN_CASES.items()}
    assert res["even-all-good"]["ok"] and res["odd-all-good"]["ok"] and res["some-lost-some-wrong"]["ok"]
    assert 0 < res["some-lost-some-wrong"]["n_correct"] < res["some-lost-some-wrong"]["n_valid"] < 80
    assert not res["too-few-valid"]["ok"] and res["too-few-valid"]["n_valid"] < 40 and res["too-few-valid"]["n_correct"] == 0
    assert not res["too-few-correct"]["ok"] and res["too-few-correct"]["n_valid"] == 80 and res["too-few-correct"]["n_correct"] < 40
    assert res["exactly-half-valid"]["ok"] and res["exactly-half-valid"]["n_valid"] == 5
    assert not res["one-less-than-half-valid"]["ok"] and res["one-less-than-half-valid"]["n_valid"] == 4
    ties = res["ties"]["order"]
    assert ties.tolist() != sorted(ties.tolist()) and all(ties[k] < ties[k + 1] for k in range(9))   # the first group of ten: one distance, index order
    cut = res["cut-on-a-value"]
    assert cut["n_valid"] == 12 and cut["n_correct"] == 6 and set(cut["order"][:6].tolist()) == {0, 1, 2, 9, 10, 11}
    assert res["two-points"]["ok"] and not res["one-point"]["ok"] and not res["no-point"]["ok"]
    assert res["coincident-points"]["ok"]


def test_median_of_the_known_motion(capi):
    """the issue's sanity case through the library: exactly the medians of the model's arrays"""
    base = M.textured()
    prev, cur = M.build_pyramid(base, 15, 15, 2), M.build_pyramid(np.roll(base, (-2, 3), axis=(0, 1)), 15, 15, 2)
    pts = M.grid_points()
    fwd, fst, _ = M.track(prev, cur, pts, 15, 15)
    bwd, bst, _ = M.track(cur, prev, fwd, 15, 15)
    m = capi.flow_median(pts, fwd, bwd, fst, bst)
    flow = fwd - pts
    assert m["ok"] and m["n_correct"] == len(pts)
    assert m["median_x"] == np.sort(flow[:, 0])[len(pts) // 2] and m["median_y"] == np.sort(flow[:, 1])[len(pts) // 2]
    assert abs(m["median_x"] - 3) < 0.1 and abs(m["median_y"] + 2) < 0.1 and abs(m["median_ratio"] - 1) < 0.01


# condensation::OpticalFlowTransitionModel with the tracking replaced: six frames that take, in order, the fallback (no previous frame), the
# fallback (no target), the flow, the fallback (too few points tracked), the fallback (too few correct), the flow.  The program prints
# what the model was given and what it did; the test replays it with the model.
HOST_PROGRAM = r'''
#include <cstdio>
#include "condensation/OpticalFlowTransitionModel.hpp"
#include "condensation/SimpleTransitionModel.hpp"
using namespace condensation;
using std::make_shared;
using std::shared_ptr;
using std::vector;

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }

struct Injected : public OpticalFlowTransitionModel {
    using OpticalFlowTransitionModel::OpticalFlowTransitionModel;
    int frame = -1, updates = 0, tracked = 0;
    void updatePyramid(const cv::Mat&) override { ++updates; }
    void trackPoints(const vector<cv::Point2f>& points, vector<cv::Point2f>& fwd, vector<cv::Point2f>& bwd, vector<cv::uchar>& fst, vector<cv::uchar>& bst) override {
        ++tracked;
        const size_t n = points.size();
        fwd.resize(n); bwd.resize(n); fst.assign(n, 1); bst.assign(n, 1);
        for (size_t i = 0; i < n; ++i) {
            fwd[i] = cv::Point2f((points[i].x - 80.f) * 1.0625f + 80.f + 2.25f + 0.03125f * (float)(i % 5), (points[i].y - 64.f) * 1.0625f + 64.f - 1.5f - 0.0625f * (float)(i % 3));
            bwd[i] = cv::Point2f(points[i].x + 0.015625f * (float)(i % 7), points[i].y - 0.03125f * (float)(i % 2));
            if (frame == 3 && i % 5 != 0) (i % 2 ? fst : bst)[i] = 0;           // a fifth of the points keep both flags
            if (frame == 4 && i % 3 != 0) bwd[i].x += 1.f;                     // a third of the points stay correct
        }
    }
};

int main() {
    const unsigned flowSeed = 77, fallbackSeed = 78;
    Sample::setAspectRatio(1.5);
    auto fallback = make_shared<SimpleTransitionModel>(4.0, 0.05, fallbackSeed);
    SimpleTransitionModel fallbackTwin(4.0, 0.05, fallbackSeed);
    Injected model(fallback, 3.0, 0.1, cv::Size(10, 10), true, cv::Size(15, 15), 2, flowSeed);
    std::mt19937 twin(flowSeed);
    std::normal_distribution<> normal;
    expect(model.getTemplatePoints().size() == 80, "80 template points");
    expect(model.getPositionDeviation() == 3.0 && model.getSizeDeviation() == 0.1, "deviations");
    model.setPositionDeviation(2.5);
    model.setSizeDeviation(0.125);
    expect(model.getPositionDeviation() == 2.5 && model.getSizeDeviation() == 0.125, "set deviations");
    cv::Mat image = cv::Mat::zeros(128, 160, CV_8UC1);
    vector<shared_ptr<Sample>> samples;
    for (int i = 0; i < 7; ++i) samples.push_back(make_shared<Sample>(60 + 5 * i, 50 + 3 * i, 30 + 2 * i, i - 3, 2 - i, 1.f + 0.01f * i));
    auto target = make_shared<Sample>(80, 64, 40);
    const bool wantFlow[6] = {false, false, true, false, false, true};
    for (int f = 0; f < 6; ++f) {
        model.frame = f;
        vector<int> before;
        for (auto& s : samples) { before.push_back(s->getX()); before.push_back(s->getY()); before.push_back(s->getSize()); }
        model.predict(samples, image, f == 1 ? shared_ptr<Sample>() : target);
        expect(model.usedFlow() == wantFlow[f], "flow or fallback");
        expect(model.updates == f + 1, "one pyramid per frame");
        std::printf("frame %d flow %d tracked %d valid %d correct %d motion %.9g %.9g %.9g\n", f, model.usedFlow() ? 1 : 0, model.tracked, model.getLastMotion().n_valid,
                    model.getLastMotion().n_correct, model.getLastMotion().median_x, model.getLastMotion().median_y, model.getLastMotion().median_ratio);
        if (model.usedFlow()) {
            expect(model.getLastDraws().size() == 3 * samples.size(), "three draws per sample");
            for (double z : model.getLastDraws()) expect(z == normal(twin), "the flow model's generator, in order, untouched by fallback frames");
        } else {
            expect(model.getLastDraws().empty(), "no draw of the flow model on a fallback frame");
            expect(fallback->getLastDiffusion().size() == 3 * samples.size(), "the fallback drew");
            for (size_t i = 0; i < samples.size(); ++i) {
                double d[3];
                fallbackTwin.drawDiffusion(d);
                expect(d[0] == fallback->getLastDiffusion()[3 * i] && d[1] == fallback->getLastDiffusion()[3 * i + 1] && d[2] == fallback->getLastDiffusion()[3 * i + 2],
                       "the fallback's generator advances on fallback frames");
            }
        }
        for (size_t i = 0; i < model.getPoints().size(); ++i)
            std::printf("p %.9g %.9g %.9g %.9g %.9g %.9g\n", model.getPoints()[i].x, model.getPoints()[i].y, model.getForwardPoints()[i].x, model.getForwardPoints()[i].y,
                        model.getBackwardPoints()[i].x, model.getBackwardPoints()[i].y);
        std::printf("correct");
        for (int i : model.getCorrectFlowIndices()) std::printf(" %d", i);
        std::printf("\n");
        for (size_t i = 0; i < samples.size(); ++i) {
            const double* z = model.usedFlow() ? &model.getLastDraws()[3 * i] : &fallback->getLastDiffusion()[3 * i];
            std::printf("s %d %d %d -> %d %d %d %d %d %.9g z %.17g %.17g %.17g\n", before[3 * i], before[3 * i + 1], before[3 * i + 2], samples[i]->getX(), samples[i]->getY(),
                        samples[i]->getSize(), samples[i]->getVx(), samples[i]->getVy(), samples[i]->getVSize(), z[0], z[1], z[2]);
        }
    }
    expect(model.tracked == 4, "tracked on the four frames with a previous frame and a target");
    // init makes the first predict a tracking one
    Injected second(make_shared<SimpleTransitionModel>(1.0, 0.1), 1.0, 0.1);
    second.frame = 2;
    second.init(image);
    second.predict(samples, image, target);
    expect(second.usedFlow() && second.updates == 2, "init gives the previous frame");
    // the size is a float product: 5 * 0.9f is 4.5f and rounds to 5; the double product 4.49999988 would give 4
    Sample five(0, 0, 5);
    const double zero[3] = {0.0, 0.0, 0.0};
    OpticalFlowTransitionModel::apply(five, 0.f, 0.f, 0.9f, 1.0, 0.0, zero);
    expect(five.getSize() == 5 && five.getVSize() == 0.9f, "5 * 0.9f -> 5");
    Sample half(10, 10, 20);
    OpticalFlowTransitionModel::apply(half, -2.5f, 2.5f, 1.f, 1.0, 0.0, zero);
    expect(half.getVx() == -3 && half.getVy() == 3 && half.getX() == 7 && half.getY() == 13, "halves round away from zero");
    bool threw = false;
    try { OpticalFlowTransitionModel bad(make_shared<SimpleTransitionModel>(1.0, 0.1), 1.0, 0.1, cv::Size(10, 10), true, cv::Size(33, 15)); } catch (const std::invalid_argument&) { threw = true; }
    expect(threw, "a window of 33 is refused");
    threw = false;
    try { OpticalFlowTransitionModel bad(shared_ptr<TransitionModel>(), 1.0, 0.1); } catch (const std::invalid_argument&) { threw = true; }
    expect(threw, "a missing fallback is refused");
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("optflow_host")
    src, exe = tmp / "optflow_host.cpp", tmp / "optflow_host"
    src.write_text(HOST_PROGRAM)
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    return run


def test_host_class_contracts(host_run):
    assert host_run.returncode == 0 and "0 failures" in host_run.stdout, host_run.stdout[-3000:] + host_run.stderr


def test_host_class_equals_the_model(host_run):
    assert host_run.returncode == 0, host_run.stdout[-3000:] + host_run.stderr
    frames = []
    for line in host_run.stdout.splitlines():
        t = line.split()
        if t[0] == "frame":
            frames.append(dict(flow=int(t[3]), tracked=int(t[5]), valid=int(t[7]), correct=int(t[9]), motion=[np.float32(v) for v in t[11:14]], p=[], s=[]))
        elif t[0] == "p":
            frames[-1]["p"].append([np.float32(v) for v in t[1:]])
        elif t[0] == "correct":
            frames[-1]["indices"] = [int(v) for v in t[1:]]
        elif t[0] == "s":
            frames[-1]["s"].append(([int(v) for v in t[1:4]], [int(v) for v in t[5:10]] + [np.float32(t[10])], [float(v) for v in t[12:15]]))
    assert [f["flow"] for f in frames] == [0, 0, 1, 0, 0, 1]
    assert [f["tracked"] for f in frames] == [0, 0, 1, 2, 3, 4]   # the two early fallbacks do not track
    template = M.grid(10, 10, True)
    for number, f in enumerate(frames):
        if number < 2:
            assert not f["p"] and f["valid"] == 0 and f["correct"] == 0
        else:
            p = np.array(f["p"], np.float32)
            assert np.array_equal(p[:, :2], M.target_points(template, 80, 64, 40, 60))   # height = cvRound(1.5 * 40)
            fst, bst = np.ones(80, np.uint8), np.ones(80, np.uint8)
            if number == 3:
                for i in range(80):
                    if i % 5:
                        (fst if i % 2 else bst)[i] = 0
            m = M.median(p[:, :2], p[:, 2:4], p[:, 4:6], fst, bst)
            assert bool(f["flow"]) == m["ok"] and f["valid"] == m["n_valid"] and f["correct"] == m["n_correct"]
            assert f["indices"] == m["order"][:m["n_correct"]].tolist()
            if m["ok"]:
                assert [v.view(np.uint32) for v in f["motion"]] == [np.float32(m[k]).view(np.uint32) for k in ("median_x", "median_y", "median_ratio")]
        assert len(f["s"]) == 7
        for before, after, z in f["s"]:
            if f["flow"]:
                want = M.apply_motion(before, m, 2.5, 0.125, z)
                assert tuple(after[:5]) == tuple(want[:5]) and after[5] == want[5], (number, before, after, want)
    assert frames[3]["valid"] == 16 and frames[4]["valid"] == 80 and frames[4]["correct"] == 27   # under 40 each: the two late fallbacks
