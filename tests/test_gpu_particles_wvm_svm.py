"""condensation::WvmSvmModel on a resident particle set (fd_particles_evaluate_wvm_svm, _weigh_wvm_svm, _get_wvm_svm_trace; DESIGN.md
4.7) on a 96 x 72 frame with 20 x 20 models.  The windows are compared with the host's rule, the scores bit for bit with fd_wvm_eval_batch
on the windows' equalised crops, the selection, targets, n_valid and best_score with tests/wvm_svm_resident_model.py, the SVM distances
with capi.Svm.distance on the same rows, and the weights with the model in units in the last place: each device logistic is within the 3
ulp of libm that DESIGN.md 4.7 states, and a weight is at most the product of two of them: 3 + 3 + 2 for the roundings of the products."""
import numpy as np
import pytest

import condensation_model as cm
import resident_model as rm
import wvm_svm_resident_model as model
from test_wvm_svm_resident_model import PH, PW, PYR, SETS, all_positive, as_samples, make_particles, make_scene

pytestmark = pytest.mark.gpu

WEIGHT_ULPS = 8
CAPACITY = 8192                                  # FD_PARTICLES_MAX
MAPS = [("resize", float(np.float32(1.1)), 0.05, -0.05)]
# (seed, count) of the sets compared with the host route, per scene: at most 8 WVM positives, and more than 8; the 8th and 9th most probable
# differ (asserted where they are used)
HOST_SETS = {"stage-a": {"few": (5, 120), "many": SETS["many"]}, "stage-b": SETS}


class Scene:
    def __init__(self, capi, ctx, synth, oracle, n_levels, positive=False, name=None):
        self.capi, self.ctx, self.name = capi, ctx, name
        self.frame, self.wvm, self.svm = make_scene(synth, oracle, n_levels=n_levels)
        if positive:
            # every window is a positive, and the smaller output is the more probable one: the first kept layer's window at (0, 0), on
            # which particles without a window are scored, has one of the smallest outputs of this frame
            self.wvm = all_positive(self.wvm)
            self.wvm["logistic_b"] = 2.95
        self.pyr = capi.Pyramid(ctx, **PYR)
        self.pyr.update(self.frame)
        self.wg, self.sg = capi.Wvm(ctx, self.wvm), capi.Svm(ctx, self.svm)
        self.reference = capi.Wvm(ctx, self.wvm)   # fd_wvm_eval_batch for the expected scores: not the handle the set runs on
        self.images = [self.pyr.layer(i) for i in range(len(self.pyr.layers()))]
        self.synth = synth

    def crops(self, windows):
        """the equalised patches of (k, 4) windows {layer, bx, by, valid}"""
        raw = np.stack([self.images[l][by:by + PH, bx:bx + PW] for l, bx, by, _ in np.asarray(windows).tolist()])
        return self.synth.histeq64_np(raw)

    def outputs(self, windows):
        """(level, fout, equalised patches) per particle; zeros for a particle without a window"""
        n = len(windows)
        level, fout, eq = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, PH, PW), np.uint8)
        ok = windows[:, 3] == 1
        if ok.any():
            eq[ok] = self.crops(windows[ok])
            level[ok], fout[ok] = self.capi.wvm_eval(self.ctx, self.reference, eq[ok])
        return level, fout, eq

    def close(self):
        for h in (self.wg, self.sg, self.reference, self.pyr):
            h.close()


@pytest.fixture(scope="module", params=["stage-a", "stage-b"])
def scene(request, capi, ctx, synth, oracle):
    """15 filters: at most WVM_LCAP (16), every positive comes from the first cascade stage; 20 filters: from the second"""
    s = Scene(capi, ctx, synth, oracle, 3 if request.param == "stage-a" else 4, name=request.param)
    assert (s.wvm["num_filters"] <= 16) == (request.param == "stage-a")
    yield s
    s.close()


@pytest.fixture(scope="module")
def positive_scene(capi, ctx, synth, oracle):
    s = Scene(capi, ctx, synth, oracle, 4, positive=True)
    yield s
    s.close()


def run_and_check(s, rows, maps=(), aspect=1.0, capacity=None):
    """one evaluate + weigh of the particles {x, y, size} on the scene's handles, everything compared; returns what the callers look at"""
    capi, ctx = s.capi, s.ctx
    n = len(rows)
    gen = cm.generation(n, x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    gen["weight"] = np.random.default_rng(n).random(n) * 3       # the model sets the weight, it does not multiply
    particles = capi.Particles.unbound(ctx, capacity or n)
    particles.set(**gen)
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, aspect, maps)
    _, windows, valid = particles.trace()
    evaluated = particles.get()
    mapped = capi.sample_maps_apply(maps, rm.sample_xywh(gen, aspect))
    want = s.pyr.sample_windows(PW, PH, mapped)
    assert np.array_equal(windows, want) and np.array_equal(valid, want[:, 3].astype(np.uint8))
    ok = valid.astype(bool)
    level, fout, eq = s.outputs(want)
    assert evaluated["score"][ok].tobytes() == fout[ok].astype(np.float64).tobytes()
    for f in cm.FIELDS:
        if f != "score":
            assert np.array_equal(evaluated[f], gen[f]), f          # evaluate changes the scores only
    particles.weigh_wvm_svm(s.wg, s.sg)
    index, distance = particles.wvm_svm_trace()
    selected = model.select(s.wvm, ok, level, fout)
    assert index.tolist() == selected, (index.tolist(), selected)
    if selected:
        host = s.sg.distance(eq[selected].reshape(len(selected), -1))
        assert np.max(np.abs(distance - host)) <= 1e-4 * np.abs(s.svm["coeff"]).sum()   # the bound of tests/test_gpu_parity.py for u8 distances
    target, weight, score, best, n_valid = model.weigh(s.wvm, s.svm, ok, level, fout, selected, distance)
    device = particles.get()
    assert np.array_equal(device["target"], target)
    assert device["score"].tobytes() == score.tobytes()
    ulps = cm.ulp_distance(device["weight"], weight)
    print("n %d: %d valid, %d positives, %d selected, max %d ulp" % (n, ok.sum(), model.positives(s.wvm, level, fout)[ok].sum(), len(selected),
                                                                    max(ulps) if n else 0))
    assert n == 0 or max(ulps) <= WEIGHT_ULPS
    assert not device["weight"][~ok].any() and not device["target"][~ok].any()
    info = particles.state()
    assert info["best_score"] == best and info["n_valid"] == n_valid and info["n_target"] == int(target.sum()) and info["count"] == n
    out = dict(particles=particles, gen=device, valid=ok, level=level, fout=fout, selected=selected, windows=want, info=info)
    return out


# ---- 1. against the model
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 257, CAPACITY])
def test_against_the_model(scene, n):
    rows = make_particles(5, CAPACITY)
    if n < CAPACITY:
        # WVM positives are rare: put them in front, every other place, so that the small sets hold some and the sets from 64 on more
        # than 8 (asserted below).  The expected values come from the windows' crops either way.
        windows = scene.pyr.sample_windows(PW, PH, as_samples(rows[:1000]))
        level, fout, _ = scene.outputs(windows)
        pos = (windows[:, 3] == 1) & model.positives(scene.wvm, level, fout)
        first, rest = np.flatnonzero(pos), np.flatnonzero(~pos)
        assert len(first) >= 16, len(first)
        order = np.empty(2 * len(first), np.int64)
        order[0::2], order[1::2] = first, rest[:len(first)]
        rows = np.concatenate([rows[order], rows[rest[len(first):]]])
    out = run_and_check(scene, rows[:n], capacity=CAPACITY if n == CAPACITY else None)
    want = {1: 1, 7: 4, 8: 4, 9: 5}.get(n, 8)
    assert len(out["selected"]) == want and (n < 64 or 0 < out["valid"].sum() < n)
    out["particles"].close()


def test_with_a_wrapper_and_an_aspect_ratio(scene):
    out = run_and_check(scene, make_particles(6, 257), MAPS, 1.25)
    assert out["valid"].sum() >= 20 and out["selected"]
    out["particles"].close()


# ---- 2. everything positive: invalid particles, duplicates, the spare window, ties
def test_everything_positive(positive_scene):
    s = positive_scene
    rows = make_particles(7, 120)
    windows = s.pyr.sample_windows(PW, PH, as_samples(rows))
    ok = windows[:, 3] == 1
    # invalid ones: widths that select no layer, windows off a border
    invalid = np.array([(48, 36, 5), (48, 36, 400), (1, 36, 30), (48, 71, 30), (95, 2, 26)], np.int32)
    assert not (s.pyr.sample_windows(PW, PH, as_samples(invalid))[:, 3] == 1).any()
    # The spare window (the first kept layer's window at 0, 0) is what an invalid particle is scored on, and here it is a positive.
    # Keep only valid particles that are less probable than it: the best candidate of the run is then a spare window.
    spare = np.array([[0, 0, 0, 1]], np.int32)
    _, spare_fout, _ = s.outputs(spare)
    _, fout, _ = s.outputs(windows)
    a, b = s.wvm["logistic_a"], s.wvm["logistic_b"]
    worse = ok & np.array([model.key(a, b, f) > model.key(a, b, spare_fout[0]) for f in fout])
    assert worse.sum() >= 20, worse.sum()
    keep = rows[worse][:20]
    mixed = np.concatenate([invalid[:2], keep[:6], keep[3:4], invalid[2:], keep[6:], keep[3:4], keep[3:4]])   # duplicates of one window
    out = run_and_check(s, mixed)
    assert len(out["selected"]) == 8 and (~out["valid"]).sum() == len(invalid)
    assert out["valid"][out["selected"]].all()
    assert model.positives(s.wvm, out["level"], out["fout"])[out["valid"]].all()
    out["particles"].close()


def test_ties_go_to_the_lower_index(positive_scene):
    s = positive_scene
    same = np.tile(np.array([[48, 36, 30]], np.int32), (12, 1))
    out = run_and_check(s, same)
    assert out["selected"] == list(range(8)) and np.unique(out["fout"]).size == 1
    assert np.unique(out["gen"]["weight"][:8]).size == 1 and np.unique(out["gen"]["weight"][8:]).size == 1
    out["particles"].close()
    # two windows, interleaved with an invalid particle: the more probable window's copies first, each group by index
    other = np.array([[40, 30, 26]], np.int32)
    rows = np.concatenate([same[:3], other, np.array([[48, 36, 5]], np.int32), same[:3], other, other, same[:4]])
    out = run_and_check(s, rows)
    f = out["fout"]
    first = 0 if model.key(s.wvm["logistic_a"], s.wvm["logistic_b"], f[0]) < model.key(s.wvm["logistic_a"], s.wvm["logistic_b"], f[3]) else 3
    groups = [[i for i in range(len(rows)) if out["valid"][i] and f[i] == f[first]], [i for i in range(len(rows)) if out["valid"][i] and f[i] != f[first]]]
    assert f[0] != f[3] and out["selected"] == (groups[0] + groups[1])[:8]
    out["particles"].close()


# ---- 3. against fd_wvm_svm_evaluate_samples
@pytest.mark.parametrize("name", sorted(SETS))
def test_against_the_host_route(scene, name):
    s = scene
    out = run_and_check(s, make_particles(*HOST_SETS[s.name][name]))
    free, n_pos = model.tie_free(s.wvm, out["valid"], out["level"], out["fout"])
    assert free and n_pos >= 1 and (name == "few" or n_pos > 8)   # the precondition: the 8th and 9th most probable positives differ
    gen = out["gen"]
    target, weight = s.capi.wvm_svm_evaluate(s.ctx, s.pyr, s.wg, s.sg, rm.sample_xywh(gen, 1.0))
    assert np.array_equal(gen["target"].astype(bool), target.astype(bool))
    assert max(cm.ulp_distance(gen["weight"], weight)) <= WEIGHT_ULPS
    out["particles"].close()


# ---- 4. the handle between five-stage calls
def test_five_stage_calls_around_the_resident_ones(scene):
    s = scene
    before, stages_before = s.capi.detect_five_stage(s.ctx, s.pyr, s.wg, s.sg)
    out = run_and_check(s, make_particles(8, 64))
    out["particles"].close()
    after, stages_after = s.capi.detect_five_stage(s.ctx, s.pyr, s.wg, s.sg)
    assert np.array_equal(stages_before, stages_after) and before.tobytes() == after.tobytes() and stages_before[0] > 0
    again, _ = s.capi.detect_five_stage(s.ctx, s.pyr, s.wg, s.sg)
    assert again.tobytes() == before.tobytes()


# ---- 5. arguments
def test_arguments(scene, capi, ctx, synth):
    s = scene
    rows = make_particles(9, 8)
    particles = capi.Particles.unbound(ctx, 8)
    particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    before = particles.get()

    def refused(call, code, match=""):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == code and match in str(e.value), e.value
        for later in (lambda: particles.weigh_wvm_svm(s.wg, s.sg), particles.wvm_svm_trace, lambda: particles.weigh_classifier(0.0, -1.0, 0.0)):
            with pytest.raises(capi.FdError) as e:   # a refused call leaves the generation "not evaluated"
                later()
            assert e.value.code == capi.FD_ERR_RUNTIME and "not been evaluated" in str(e.value)
        got = particles.get()
        assert all(np.array_equal(got[f], before[f]) for f in cm.FIELDS)

    bad = capi.FD_ERR_INVALID_ARGUMENT
    refused(lambda: particles.weigh_wvm_svm(s.wg, s.sg), capi.FD_ERR_RUNTIME, "not been evaluated")
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)    # evaluated: every refusal below has to take that back
    before = particles.get()                              # with the scores this evaluate left
    refused(lambda: particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0, [("integral",)]), bad, "FD_SAMPLE_MAP_RESIZE")
    refused(lambda: particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0, [("resize", 1.1)] * 5), bad, "sample maps")
    f32 = synth.make_svm_f32(5, np.random.default_rng(1).random((16, PW * PH)).astype(np.float32), nsv=8, kernel=0)
    refused(lambda: particles.evaluate_wvm_svm(s.pyr, s.wg, capi.Svm(ctx, f32), 1.0), bad, "HistEq64 patch")
    short = np.random.default_rng(1).integers(0, 256, (16, 16 * 16)).astype(np.uint8)
    refused(lambda: particles.evaluate_wvm_svm(s.pyr, s.wg, capi.Svm(ctx, synth.make_svm_u8(3, short, nsv=8, calib=short, positive_fraction=0.5)), 1.0),
            bad, "HistEq64 patch")
    filtered = capi.Pyramid(ctx, **PYR)
    filtered.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9, interpolate=False)
    filtered.update(s.frame)
    refused(lambda: particles.evaluate_wvm_svm(filtered, s.wg, s.sg, 1.0), bad, "gray pyramid")
    multi = capi.Pyramid(ctx, **PYR)
    multi.set_frames(2)
    multi.update_frames(images=[s.frame, s.frame])
    refused(lambda: particles.evaluate_wvm_svm(multi, s.wg, s.sg, 1.0), bad, "frames")
    other = capi.Context(0)
    foreign = capi.Pyramid(other, **PYR)
    foreign.update(s.frame)
    foreign_wvm, foreign_svm = capi.Wvm(other, s.wvm), capi.Svm(other, s.svm)
    refused(lambda: particles.evaluate_wvm_svm(foreign, s.wg, s.sg, 1.0), bad, "different contexts")
    refused(lambda: particles.evaluate_wvm_svm(s.pyr, foreign_wvm, s.sg, 1.0), bad, "different contexts")
    refused(lambda: particles.evaluate_wvm_svm(s.pyr, s.wg, foreign_svm, 1.0), bad, "different contexts")
    # a width -> layer table longer than FD_SAMPLE_TABLE_MAX: one layer of scale 2^-12 (1 x 1 pixel of a 2200 x 2200 frame); widths up to
    # 20 * 2^12.5 = 115852 map to it (the estimate of tests/test_sample_layer_table.py)
    tiny = capi.Pyramid(ctx, octave_layers=1, min_scale=2.0 ** -12, max_scale=2.0 ** -12)
    tiny.update(np.full((2200, 2200), 128, np.uint8))
    assert [(l["index"], l["w"], l["h"]) for l in tiny.layers()] == [(12, 1, 1)] and PW / 0.5 ** 12.5 > capi.FD_SAMPLE_TABLE_MAX + 2
    refused(lambda: particles.evaluate_wvm_svm(tiny, s.wg, s.sg, 1.0), bad, "width -> layer table")
    deep = capi.Pyramid(ctx, octave_layers=30, min_scale=0.21, max_scale=1.0)   # 68 kept layers: more than the cascade's table holds
    deep.update(s.frame)
    assert len(deep.layers()) > 64
    refused(lambda: particles.evaluate_wvm_svm(deep, s.wg, s.sg, 1.0), bad, "layers")
    fresh = capi.Pyramid(ctx, **PYR)   # never updated
    refused(lambda: particles.evaluate_wvm_svm(fresh, s.wg, s.sg, 1.0), capi.FD_ERR_RUNTIME, "not been updated with an image")
    # The weigh call checks the SVM it is given: the rows it reads hold the WVM's dimension in bytes.  A refused weighing launches nothing
    # and the generation stays evaluated
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)
    evaluated = particles.get()
    short_svm = capi.Svm(ctx, synth.make_svm_u8(3, short, nsv=8, calib=short, positive_fraction=0.5))
    for wrong, match in ((capi.Svm(ctx, f32), "HistEq64 patch"), (short_svm, "HistEq64 patch"), (foreign_svm, "different contexts")):
        with pytest.raises(capi.FdError) as e:
            particles.weigh_wvm_svm(s.wg, wrong)
        assert e.value.code == bad and match in str(e.value), e.value
        got = particles.get()
        assert all(got[f].tobytes() == evaluated[f].tobytes() for f in cm.FIELDS)
    with pytest.raises(capi.FdError) as e:
        particles.weigh_wvm_svm(foreign_wvm, s.sg)
    assert e.value.code == bad and "different contexts" in str(e.value)
    particles.weigh_wvm_svm(s.wg, s.sg)
    assert particles.state()["n_valid"] == int(s.pyr.sample_windows(PW, PH, as_samples(rows))[:, 3].sum())
    # another run on the WVM handle between the two calls takes the positives away: the weighing is refused, nothing is read
    particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)
    capi.detect_five_stage(ctx, s.pyr, s.wg, s.sg)
    with pytest.raises(capi.FdError) as e:
        particles.weigh_wvm_svm(s.wg, s.sg)
    assert e.value.code == capi.FD_ERR_RUNTIME and "has run again" in str(e.value)
    # evaluated with one WVM, weighed with another
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)
    with pytest.raises(capi.FdError) as e:
        particles.weigh_wvm_svm(s.reference, s.sg)
    assert e.value.code == capi.FD_ERR_RUNTIME
    with pytest.raises(capi.FdError) as e:   # the trace needs the weighing
        particles.wvm_svm_trace()
    assert e.value.code == capi.FD_ERR_RUNTIME
    # another kind of evaluate is no evaluate of this kind
    pp = capi.patch_samples_params(PW, PH, capi.FD_FEATURE_GRAY, 1.0 / 127.5, -1.0)
    particles.evaluate_pyramid(s.pyr, capi.Svm(ctx, f32), 1.0, [], patch=pp)
    with pytest.raises(capi.FdError) as e:
        particles.weigh_wvm_svm(s.wg, s.sg)
    assert e.value.code == capi.FD_ERR_RUNTIME and "not been evaluated" in str(e.value)
    # an empty generation goes through the whole chain
    particles.sample(0, 0, 0.5, np.zeros((0, 3)), np.zeros((0, 3), np.int32), 0)
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)
    particles.weigh_wvm_svm(s.wg, s.sg)
    index, distance = particles.wvm_svm_trace()
    info = particles.state()
    assert len(index) == 0 and info["count"] == 0 and info["found"] == 0 and info["n_valid"] == 0
    # no layer holds a window: every particle is invalid, nothing is selected
    small = capi.Pyramid(ctx, octave_layers=3, min_scale=0.1, max_scale=0.2)
    small.update(s.frame)
    assert small.layers() and all(l["h"] < PH for l in small.layers())
    particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    particles.evaluate_wvm_svm(small, s.wg, s.sg, 1.0)
    particles.weigh_wvm_svm(s.wg, s.sg)
    got = particles.get()
    assert len(particles.wvm_svm_trace()[0]) == 0 and not got["weight"].any() and not got["target"].any() and not got["score"].any()
    assert particles.state()["n_valid"] == 0
    for p in (filtered, multi, foreign, deep, fresh, small, tiny, foreign_wvm, foreign_svm):
        p.close()
    other.close()
    particles.close()
    # the set works after every refusal
    run_and_check(s, rows)["particles"].close()


def test_a_fixed_stage_b_state_below_the_particle_count_is_refused(scene, monkeypatch):
    """FD_WVM_DEEP_CAP (read per call) fixes the second cascade stage's state; nobody reads an overflow of this run back, so the call is
    refused before anything is queued.  A model whose cascade ends in the first stage has no such state"""
    s = scene
    rows = make_particles(10, 100)
    particles = s.capi.Particles.unbound(s.ctx, 100)
    particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    monkeypatch.setenv("FD_WVM_DEEP_CAP", "64")
    if s.name == "stage-b":
        with pytest.raises(s.capi.FdError) as e:
            particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)
        assert e.value.code == s.capi.FD_ERR_DEVICE_CAPACITY and "FD_WVM_DEEP_CAP" in str(e.value)
        with pytest.raises(s.capi.FdError) as e:
            particles.weigh_wvm_svm(s.wg, s.sg)
        assert e.value.code == s.capi.FD_ERR_RUNTIME and "not been evaluated" in str(e.value)
        monkeypatch.setenv("FD_WVM_DEEP_CAP", "100")   # exactly the count: accepted
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0)
    particles.weigh_wvm_svm(s.wg, s.sg)
    with_cap = particles.get()
    monkeypatch.delenv("FD_WVM_DEEP_CAP")
    particles.close()
    out = run_and_check(s, rows)
    assert all(out["gen"][f].tobytes() == with_cap[f].tobytes() for f in ("x", "y", "size", "weight", "score", "target"))
    out["particles"].close()
