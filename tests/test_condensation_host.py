"""The Condensation tracker's frame loop, the parts that need no device: tests/condensation_model.py against hand-computed cases, the
host classes (ResamplingSampler on LowVarianceSampling + SimpleTransitionModel, GridSampler, the state extractors, CondensationTracker)
against the model through `tracker_app --selftest`, which dumps its draws, and the declarations of the C ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import condensation_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
F32 = np.float32


def test_equal_weights_take_the_first_sample_twice():
    """count = N, u = 0: the pointers 0, 1, 2 ... land on the cumulative sums 1, 2, 3 ...; `>` is strict, so 0 and 1 both stay at sample 0"""
    assert model.low_variance_indices([1.0] * 6, 6, 0.0) == [0, 0, 1, 2, 3, 4]
    assert model.low_variance_indices([1.0] * 6, 6, 0.5) == [0, 1, 2, 3, 4, 5]
    assert model.low_variance_indices([1.0] * 4, 2, 0.25) == [0, 2]   # step 2, pointers 0.5 and 2.5
    assert model.low_variance_indices([1.0], 3, 0.9) == [0, 0, 0]


def test_dominant_and_zero_weights():
    # sum 100.002, step 25.0005: every pointer lies inside the one large weight
    assert model.low_variance_indices([0.001, 100.0, 0.001], 4, 0.5) == [1, 1, 1, 1]
    # zero weights at both ends: the pointer 0 does not exceed the sum 0, so the first (weightless) sample is taken
    assert model.low_variance_indices([0, 0, 1, 1, 0, 0], 4, 0.0) == [0, 2, 2, 3]
    assert model.low_variance_indices([0, 0, 1, 1, 0, 0], 4, 0.5) == [2, 2, 3, 3]
    # all weights zero: the step is not positive, nothing is produced; no samples: nothing either
    assert model.low_variance_indices([0.0, 0.0, 0.0], 5, 0.3) == []
    assert model.low_variance_indices([], 5, 0.3) == []
    assert model.low_variance_indices([1.0, 2.0], 0, 0.3) == []
    # a pointer that rounding leaves above the total stops at the last sample
    w = [0.1] * 10
    assert max(model.low_variance_indices(w, 10, 1.0)) == 9


def test_prediction_arithmetic():
    # velocities: double, rounded half away from zero; position moves by the new velocity
    assert model.predict(10, 20, 30, 1, -1, F32(1), 0.5, -0.5, 1.0)[:5] == (12, 18, 30, 2, -2)
    assert model.predict(10, 20, 30, 0, 0, F32(1), 0.49, -0.49, 1.0)[:5] == (10, 20, 30, 0, 0)
    assert model.predict(0, 0, 30, 2, -3, F32(1), 0.5, 0.5, 1.0)[3:5] == (3, -3)   # 2.5 -> 3, -2.5 -> -3
    # the size factor is stored as a float, and size * factor is a float product: 5 * 0.9f = 4.5f exactly, which rounds to 5;
    # in double 5 * 0.89999997615814209 = 4.4999998807907104 would round to 4
    assert float(F32(5) * F32(0.9)) == 4.5 and 5 * float(F32(0.9)) < 4.5
    assert model.predict(0, 0, 5, 0, 0, F32(0.9), 0.0, 0.0, 1.0)[2] == 5
    assert model.predict(0, 0, 10, 0, 0, F32(1.05), 0.0, 0.0, 1.0)[2] == 11   # 10.5f against 10.499999523162842
    x, y, size, vx, vy, vs = model.predict(0, 0, 100, 0, 0, F32(1), 0.0, 0.0, 2 ** 0.1)
    assert vs == F32(2 ** 0.1) and vs.dtype == np.float32 and size == 107


def test_prediction_rounds_negative_halves_away_from_zero():
    assert model.predict(0, 0, 30, -3, 0, F32(1), 0.5, 0.0, 1.0)[3] == -3   # -2.5 -> -3
    assert model.predict(0, 0, 30, 2, 0, F32(1), 0.5, 0.0, 1.0)[3] == 3     #  2.5 ->  3


def test_weighted_mean_truncates_the_size_factor():
    gen = model.generation(5, x=[10, 11, 12, 13, 14], y=[7] * 5, size=[20] * 5, vsize=[0.4] * 5, target=[1] * 5)
    assert model.filtered_state(gen) == (12, 7, 20, 0, 0, F32(0))        # a mean size factor of 0.4 becomes (int)0.9 = 0
    gen["vsize"][:] = 1.6
    assert model.filtered_state(gen)[5] == F32(2)
    gen["vx"][:] = -1
    assert model.filtered_state(gen)[3] == 0                             # (int)(-1 + 0.5) truncates towards zero
    gen["weight"][:] = 0
    assert model.filtered_state(gen) is None
    gen["weight"][:] = 1
    gen["target"][:] = 0
    assert model.filtered_state(gen) is None


def test_cluster_tie_goes_to_the_first_member():
    gen = model.generation(4, x=[10, 20, 30, 40], cluster_id=[7, 3, 3, 7], target=[1] * 4)
    assert model.largest_cluster(gen["cluster_id"], range(4)) == 7
    assert model.filtered_state(gen)[0] == 25
    gen["target"][0] = 0   # without its first member cluster 7 is smaller
    assert model.filtered_state(gen)[0] == 25 and model.largest_cluster(gen["cluster_id"], [1, 2, 3]) == 3
    assert model.max_weight_state(model.generation(3, weight=[0.2, 0.7, 0.7], x=[1, 2, 3], target=[1, 1, 1]))[0] == 2
    assert model.max_weight_state(model.generation(3, weight=[0.2, 0.7, 0.1], x=[1, 2, 3], target=[1, 0, 1])) is None
    assert model.max_weight_state(model.generation(2, weight=[0, 0], target=[1, 1])) is None


def test_weighing():
    gen = model.generation(3, weight=[2.0, 1.0, 1.0])
    out, best = model.weigh(gen, [1, 0, 1], [0.5, 9.0, -3.0], 0.0, -2.0, 0.25, model.TARGET_LOST, -1.0)
    assert out["weight"][0] == 2.0 * (1.0 / (1.0 + np.exp(-1.0))) and out["weight"][1] == 0 and out["score"][1] == 0
    assert out["target"].tolist() == [1, 0, 0] and best == 0.5
    out, best = model.weigh(gen, [0, 0, 1], [0.5, 9.0, -3.0], 0.0, -2.0, 0.25, model.SLIDING_WINDOW, -3.0)
    assert out["target"].tolist() == [0, 0, 0] and best == 0.0          # -3 > -3 is false; the samples without a window count with 0
    assert model.weigh(gen, [1, 1, 1], [0.5, 9.0, -3.0], 0.0, -2.0, 0.25, model.ALL_TARGETS, 0.0)[0]["target"].tolist() == [1, 1, 1]
    assert model.probability(800.0, 0.0, 1.0) == 0.0 and model.probability(-800.0, 0.0, 1.0) == 1.0   # neither branch overflows


def test_grid_sampler_counts():
    """64 x 48, sizes 10 .. 40 with factor 1.5: 10, 15, 22 (int * float, truncated), 33; steps (int)(0.25 * size + 0.5)"""
    samples = model.grid_samples(64, 48, 10, 40, 1.5, 0.25)
    sizes = sorted(set(s[2] for s in samples))
    assert sizes == [10, 15, 22, 33]
    per = {size: sum(1 for s in samples if s[2] == size) for size in sizes}
    # size 10: step 3 (2.5 + 0.5), x in [5, 59) -> 18, y in [5, 43) -> 13; size 15: step 4, x [7, 56) -> 13, y [7, 40) -> 9;
    # size 22: step 6, x [11, 53) -> 7, y [11, 37) -> 5; size 33: step 8 (8.75), x [16, 47) -> 4, y [16, 31) -> 2
    assert per == {10: 18 * 13, 15: 13 * 9, 22: 7 * 5, 33: 4 * 2}


def _parse_selftest(text):
    frames, grid, cur = [], [], None
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            cur = dict(found=int(t[3]), state=None, draws=None, d=[], f=[], s=[], max=None)
            if cur["found"]:
                cur["state"] = tuple(int(v) for v in t[4:9]) + (F32(t[9]),)
            frames.append(cur)
        elif t[0] == "max":
            cur["max"] = tuple(int(v) for v in t[2:5]) if t[1] == "1" else None
        elif t[0] == "draws":
            cur["draws"] = dict(has_u=int(t[2]), u=float(t[3]), copies=int(t[5]), fresh=int(t[7]))
        elif t[0] == "d":
            cur["d"].append(tuple(float(v) for v in t[1:4]))
        elif t[0] == "f":
            cur["f"].append(tuple(int(v) for v in t[1:4]))
        elif t[0] == "s":
            cur["s"].append(t[1:])
        elif t[0] == "g":
            grid.append(tuple(int(v) for v in t[1:4]))
    return frames, grid


def _dumped_generation(rows):
    cols = list(zip(*rows)) if rows else [[]] * 10
    conv = (int, int, int, int, int, F32, float, float, int, int)
    return {k: np.array([c(v) for v in cols[i]], model.DTYPES[k]) for i, (k, c) in enumerate(zip(model.FIELDS, conv))}


def _stub_weigh(gen, frame_number):
    """StubModel of tracker_app: weight *= 1 / (1 + d^2), score = -d^2, target when d^2 < 144, d the distance to (20 + 2 f, 16 + f)"""
    out = {k: v.copy() for k, v in gen.items()}
    for i in range(len(gen["x"])):
        dx, dy = float(int(gen["x"][i]) - (20 + 2 * frame_number)), float(int(gen["y"][i]) - (16 + frame_number))
        d2 = dx * dx + dy * dy
        out["score"][i] = -d2
        out["weight"][i] = float(gen["weight"][i]) * (1.0 / (1.0 + d2))
        out["target"][i] = d2 < 144
    return out


SELFTEST_CASES = [(1, 6, 40, 0.25), (7, 5, 65, 0.0), (3, 4, 9, 0.5), (11, 3, 300, 0.35)]


@pytest.fixture(scope="module", params=SELFTEST_CASES, ids=lambda c: "seed%d-%dx%d" % c[:3])
def selftest(request):
    seed, frames, count, rate = request.param
    run = subprocess.run([APP, "--selftest", str(seed), str(frames), str(count), str(rate)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return request.param, _parse_selftest(run.stdout)


def _replay(case, frames, nudge=0):
    """steps the model through the dumped draws; with nudge the weights of every old generation are moved by that many ulp first.
    Returns per frame (generation after weighing, source indices, state)."""
    seed, n_frames, count, rate = case
    old = model.generation(0)
    out = []
    for f, fr in enumerate(frames):
        d = fr["draws"]
        dumped = _dumped_generation(fr["s"])
        first_id = int(dumped["cluster_id"][d["copies"]]) if d["fresh"] else 0
        stepped = dict(old)
        if nudge:
            stepped["weight"] = model.nudge(old["weight"], nudge)
        new, source = model.sample(stepped, d["copies"] + d["fresh"], d["copies"], d["u"], fr["d"], fr["f"], first_id)
        weighed = _stub_weigh(new, f + 1)
        out.append((weighed, source, model.filtered_state(weighed), dumped))
        old = weighed
    return out


def test_host_classes_equal_the_model(selftest):
    case, (frames, grid) = selftest
    seed, n_frames, count, rate = case
    assert len(frames) == n_frames
    next_fresh = None
    for f, (fr, (weighed, source, state, dumped)) in enumerate(zip(frames, _replay(case, frames))):
        d = fr["draws"]
        assert len(fr["d"]) == d["copies"] and len(fr["f"]) == d["fresh"] and d["copies"] + d["fresh"] == count
        assert d["copies"] == (model.resampled_count(count, rate) if f > 0 and d["has_u"] else 0)
        assert all(0 <= u < 1 for u in [d["u"]])
        for k in model.FIELDS:
            assert weighed[k].tobytes() == dumped[k].tobytes(), (f, k, weighed[k][:5], dumped[k][:5])
        assert fr["state"] == state, (f, fr["state"], state)
        mw = model.max_weight_state(weighed)
        assert fr["max"] == (None if mw is None else tuple(int(v) for v in mw[:3]))
        if d["fresh"]:   # consecutive cluster ids, in order, continuing over the frames (the extracted state takes one as well)
            ids = dumped["cluster_id"][d["copies"]:]
            assert np.array_equal(ids, ids[0] + np.arange(len(ids)))
            if next_fresh is not None:
                assert ids[0] == next_fresh
            next_fresh = int(ids[-1]) + 1 + (1 if state is not None else 0)
        for x, y, size in fr["f"]:   # ResamplingSampler::sampleValues: inside the image, sizes 8 .. 48 (maxSize clamped to the image by init)
            assert 8 <= size <= 48 and size // 2 <= x <= 64 - size + size // 2 and size // 2 <= y <= 48 - size + size // 2
    assert any(fr["found"] for fr in frames)
    assert grid == model.grid_samples(64, 48, 10, 40, 1.5, 0.25)


def test_integer_outputs_survive_four_ulp(selftest):
    """the precondition of comparing two routes whose weights differ in the last places: moving every weight by +-4 ulp changes no
    selected index, no sample field and no state on these seeds and frames.  These are the self-test's seeds and stub weights; the
    route test's own weights are extended-HOG scores that exist only after a device run, so
    tests/test_gpu_condensation_host_app.py asserts the same property on each run's dumped weights before it compares the routes."""
    case, (frames, _) = selftest
    base = _replay(case, frames)
    for nudge in (-4, 4):
        for f, ((w0, s0, st0, _), (w1, s1, st1, _)) in enumerate(zip(base, _replay(case, frames, nudge))):
            assert np.array_equal(s0, s1), (f, nudge)
            for k in ("x", "y", "size", "vx", "vy", "vsize", "target", "cluster_id"):
                assert w0[k].tobytes() == w1[k].tobytes(), (f, nudge, k)
            assert st0 == st1, (f, nudge)


def test_header_declares_the_particle_set():
    hdr = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    for name in ("create", "destroy", "capacity", "set", "get", "get_trace", "sample", "evaluate", "weigh", "state", "route_enabled"):
        assert re.search(r"\bfd_particles_%s\s*\(" % name, hdr), name
    assert "int fd_particles_sample(fd_ctx* ctx, fd_particles* p, int count, int n_resampled, double u, const double* diffusion, const int32_t* fresh," in hdr
    src = ('#include "fd_hip.h"\nint main(void) { fd_particles_info i; fd_particles_arrays a; a.x = 0; i.found = FD_PARTICLES_MAX - 8192;'
           ' return i.found + (a.x != 0) + FD_PARTICLES_TARGET_LOST; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)


def test_binding_matches_the_structs(capi):
    import ctypes
    assert ctypes.sizeof(capi.fd_particles_info) == 64 and capi.fd_particles_info.best_score.offset == 48
    assert ctypes.sizeof(capi.fd_particles_arrays) == 10 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in capi.PARTICLE_FIELDS] == list(model.FIELDS) == [n for n, _ in capi.fd_particles_arrays._fields_]
    assert capi.lib().fd_particles_capacity(None) == 0
    old = os.environ.pop("FD_COND_DEVICE", None)
    try:
        assert capi.lib().fd_particles_route_enabled() == 0
        os.environ["FD_COND_DEVICE"] = "1"
        assert capi.lib().fd_particles_route_enabled() == 1
        os.environ["FD_COND_DEVICE"] = "0"
        assert capi.lib().fd_particles_route_enabled() == 0
    finally:
        os.environ.pop("FD_COND_DEVICE", None)
        if old is not None:
            os.environ["FD_COND_DEVICE"] = old


HOST_PROGRAM = r'''
#include "condensation/AdaptiveCondensationTracker.hpp"
#include "condensation/GridSampler.hpp"
#include "condensation/ResamplingSampler.hpp"
#include <cstdio>
#include <functional>
#include <type_traits>
using namespace condensation;
static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static bool invalid(const std::function<void()>& f) {
    try { f(); } catch (const std::invalid_argument&) { return true; } catch (...) { return false; }
    return false;
}
int main() {
    static_assert(std::is_base_of<AdaptiveMeasurementModel, ExtendedHogBasedMeasurementModel>::value, "the model adapts");
    static_assert(std::is_base_of<StateValidator, ExtendedHogBasedMeasurementModel>::value, "the model validates");
    static_assert(std::is_base_of<MeasurementModel, AdaptiveMeasurementModel>::value, "an adaptive model measures");
    auto lv = std::make_shared<LowVarianceSampling>();
    auto tm = std::make_shared<SimpleTransitionModel>(10.0, 0.1);
    expect(invalid([&] { ResamplingSampler s(10, 0.5, lv, tm, 0, 10); }), "minSize 0");
    expect(invalid([&] { ResamplingSampler s(10, 0.5, lv, tm, 20, 10); }), "maxSize < minSize");
    expect(invalid([] { GridSampler g(0, 10, 1.5f, 0.1f); }), "grid minSize 0");
    expect(invalid([] { GridSampler g(10, 5, 1.5f, 0.1f); }), "grid maxSize < minSize");
    expect(invalid([] { GridSampler g(10, 20, 1.0f, 0.1f); }), "grid scale 1");
    ResamplingSampler s(10, 1.5, lv, tm, 8, 200);
    expect(s.getRandomRate() == 1.0 && s.getCount() == 10, "the random rate is clamped");
    cv::Mat tiny(4, 4, CV_8UC1);
    expect(invalid([&] { s.init(tiny); }), "minSize larger than the image");
    // a descendant: the parent's values and cluster, weight 1, score 0, no target flag, the parent as ancestor
    auto parent = std::make_shared<Sample>(3, 4, 5, 1, -1, 1.25f);
    parent->setWeight(0.5); parent->setScore(2.0); parent->setTarget(true);
    Sample child(parent);
    expect(child.getX() == 3 && child.getVSize() == 1.25f && child.getClusterId() == parent->getClusterId(), "descendant values");
    expect(child.getWeight() == 1 && child.getScore() == 0 && !child.isTarget() && child.getAncestor() == parent, "descendant state");
    // same seed, same stream; the default is the engine's default seed
    LowVarianceSampling a(5), b(5), c, d(std::mt19937::default_seed);
    expect(a.draw() == b.draw() && c.draw() == d.draw(), "seeded generators");
    expect(tm->getPositionDeviation() == 10.0 && tm->getSizeDeviation() == 0.1, "deviations");
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
'''


def test_host_class_contracts(tmp_path):
    src = tmp_path / "cond_host.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "cond_host"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
