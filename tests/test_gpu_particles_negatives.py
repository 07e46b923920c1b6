"""fd_particles_state_negatives (k_particles_negatives behind k_particles_state) against tests/negatives_model.py: the
count and every record bit for bit, the info -- and the motion when a flow is given -- equal to what fd_particles_state /
fd_particles_state_flow report on the same generation.  The generations are placed with fd_particles_set (weights with few distinct
values, zeros and -0 among them, so ties are everywhere; all equal; all zero; all distinct), at every size around the selection's
paths: empty, below and at max_count, one and several steps of 64 per wavefront, the largest set.  The model's box is taken around the
state the device reports, which is the one fd_particles_state reports.  One generation comes out of a real sample -> evaluate_integral
-> weigh_classifier chain; there the model is fed the device's own weights."""
import ctypes as C

import numpy as np
import pytest

import condensation_model as cm
import negatives_model as model
import resident_model
from test_gpu_particles_integral import ASPECT, HOG_CASE, MAPS, _samples
from test_integral_hog_model import capi_params
from test_negatives_model import TARGET, generation

pytestmark = pytest.mark.gpu

COUNTS = (1, 10, 64)


def _sizes(max_count):
    return sorted({0, 1, 2, max(max_count - 1, 0), max_count, max_count + 1, 64, 65, 257, 1000, 8192})


@pytest.fixture(scope="module")
def particles(capi, ctx):
    p = capi.Particles.unbound(ctx, capi.FD_PARTICLES_MAX)
    yield p
    p.close()


@pytest.fixture(scope="module")
def flow(capi, ctx):
    f = capi.Flow(ctx, 64, 48)
    f.debug_motion(*resident_model.crafted_tracks(16, 41))
    yield f
    f.close()


def _with_state(gen, seed, clusters=3):
    """target flags and cluster ids of the test's choosing: a third of the samples targets in `clusters` clusters; sample 0 is a target
    with a positive weight, so that with one cluster a state exists whatever the other weights are"""
    rng = np.random.default_rng(seed)
    n = len(gen["x"])
    gen["target"] = (rng.random(n) < 0.34).astype(np.uint8)
    gen["cluster_id"] = rng.integers(5, 5 + clusters, n).astype(np.int32)
    if n:
        gen["target"][0] = 1
        if not gen["weight"][0] > 0:
            gen["weight"][0] = 0.5
    return gen


def _same_info(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array(a[k]).tobytes() == np.array(b[k]).tobytes(), (k, a[k], b[k])


def _check(capi, particles, gen, max_count, offset_factor, flow=None):
    """the call on `gen` against the plain state calls and the model; returns (info, chosen)"""
    particles.set(**gen)
    if flow is None:
        plain, plain_motion = particles.state(), None
    else:
        plain, plain_motion = particles.state_flow(flow)
    info, motion, chosen = particles.state_negatives(capi.negatives_params(max_count, offset_factor), flow)
    _same_info(info, plain)
    assert (motion is None) == (flow is None) and (flow is None or resident_model.same_motion(motion, plain_motion))
    if not info["found"]:
        assert len(chosen["index"]) == 0
        return info, chosen
    want = model.records(gen, model.choose(gen, max_count, offset_factor, (info["x"], info["y"], info["size"])))
    assert chosen["index"].tolist() == want["index"].tolist(), (chosen["index"][:8], want["index"][:8])
    for k in ("x", "y", "size", "weight"):
        assert chosen[k].tobytes() == want[k].tobytes(), k
    _same_info(particles.state(), plain)   # the generation is untouched
    return info, chosen


@pytest.mark.parametrize("max_count", COUNTS)
def test_every_size(capi, particles, max_count):
    for n in _sizes(max_count):
        for weights in ("random", "distinct", "equal", "zero"):
            if n > 1000 and weights == "zero":
                continue
            gen = _with_state(generation(n, 7 * n + max_count, weights, spread=40 if n < 1000 else 120), n, clusters=1 if n < 64 or weights == "zero" else 3)
            info, chosen = _check(capi, particles, gen, max_count, 0.5)
            assert info["count"] == n and info["found"] == (1 if n else 0)
            if n >= 257:   # about half of the samples lie outside the box: the list is full and the cut real
                assert len(chosen["index"]) == max_count
    print("max_count %d: sizes %s" % (max_count, _sizes(max_count)))


@pytest.mark.parametrize("offset_factor", [0.0, 0.3, 0.5])
def test_offset_factors_and_flow(capi, particles, flow, offset_factor):
    gen = _with_state(generation(300, 5, "random"), 2)
    for max_count in COUNTS:
        _check(capi, particles, gen, max_count, offset_factor)
        info, chosen = _check(capi, particles, gen, max_count, offset_factor, flow)
        assert info["found"] == 1 and len(chosen["index"]) > 0


def test_samples_on_the_bounds_and_few_outside(capi, particles):
    # the state of a generation whose targets all sit on one point is that point: the box is known beforehand
    for offset_factor in (0.3, 0.5):
        b = model.bounds(offset_factor, *TARGET)
        rows = [list(TARGET)] * 4
        for k in range(6):
            for d in (-1, 0, 1):
                s = list(TARGET)
                s[k // 2] = b[k] + d
                rows.append(s)
        rows = np.array(rows)
        n = len(rows)
        gen = cm.generation(n, x=rows[:, 0], y=rows[:, 1], size=rows[:, 2], weight=np.linspace(0.9, 0.1, n))
        gen["target"][:4] = 1
        info, chosen = _check(capi, particles, gen, 64, offset_factor)
        assert (info["x"], info["y"], info["size"]) == TARGET
        assert sorted(chosen["index"].tolist()) == [4 + 3 * k + d for k in range(6) for d in ((0, 1) if k % 2 == 0 else (1, 2))]   # 12 < 64 outside
        info, chosen = _check(capi, particles, gen, 10, offset_factor)
        assert len(chosen["index"]) == 10 and (np.diff(chosen["weight"]) >= 0).all()
    # none outside
    gen = cm.generation(70, x=np.full(70, TARGET[0]), y=np.full(70, TARGET[1]), size=np.full(70, TARGET[2]), weight=np.linspace(0.1, 1, 70))
    gen["target"][:] = 1
    info, chosen = _check(capi, particles, gen, 10, 0.5)
    assert info["found"] == 1 and len(chosen["index"]) == 0


def test_no_state_and_bad_weight(capi, particles, flow):
    gen = generation(200, 1, "random")                      # no target flag: no state
    info, chosen = _check(capi, particles, gen, 10, 0.5)
    assert info["found"] == 0 and info["count"] == 200 and len(chosen["index"]) == 0
    gen = _with_state(generation(200, 1, "random"), 3)
    gen["weight"][:] = 0                                    # targets, but their weights add up to 0: no state either
    info, chosen = _check(capi, particles, gen, 10, 0.5)
    assert info["found"] == 0 and len(chosen["index"]) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        gen = _with_state(generation(200, 1, "random"), 3)
        gen["weight"][150] = bad
        particles.set(**gen)
        with pytest.raises(capi.FdError) as plain:
            particles.state()
        for f in (None, flow):
            with pytest.raises(capi.FdError) as e:
                particles.state_negatives(capi.negatives_params(10, 0.5), f)
            assert e.value.code == capi.FD_ERR_RUNTIME == plain.value.code and e.value.count == 0
            _same_info({k: v for k, v in e.value.info.items() if k != "weight_sum"}, {k: v for k, v in plain.value.info.items() if k != "weight_sum"})
            assert e.value.info["bad_weight"] == 1 and e.value.info["found"] == 0


def test_arguments(capi, ctx, particles, flow):
    gen = _with_state(generation(50, 1, "random"), 3)
    particles.set(**gen)
    before = particles.state()
    for params in (capi.fd_particles_negatives_params(0, 0.5, 0.5, 2.0), capi.fd_particles_negatives_params(65, 0.5, 0.5, 2.0),
                   capi.fd_particles_negatives_params(10, float("nan"), 0.5, 2.0), capi.negatives_params(10, 1.0)):
        with pytest.raises(capi.FdError) as e:
            particles.state_negatives(params)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    other = capi.Context(0)
    foreign = capi.Flow(other, 64, 48)
    foreign.debug_motion(*resident_model.crafted_tracks(16, 41))
    with pytest.raises(capi.FdError) as e:
        particles.state_negatives(capi.negatives_params(10, 0.5), foreign)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    info, motion, count = capi.fd_particles_info(), capi.fd_flow_motion_info(), C.c_int()
    records = (capi.fd_particles_negative * capi.FD_PARTICLES_NEGATIVES_MAX)()
    params = capi.negatives_params(10, 0.5)
    assert capi.lib().fd_particles_state_negatives(other.h, particles.h, None, C.byref(params), C.byref(info), None, C.byref(count),
                                                   records) == capi.FD_ERR_INVALID_ARGUMENT
    assert capi.lib().fd_particles_state_negatives(ctx.h, particles.h, flow.h, C.byref(params), C.byref(info), None, C.byref(count),
                                                   records) == capi.FD_ERR_INVALID_ARGUMENT   # a flow without room for its motion
    foreign.close()
    other.close()
    _same_info(particles.state(), before)


def test_behind_a_real_chain(capi, ctx, synth, particles):
    """sample -> evaluate_integral (ihog, linear SVM) -> weigh_classifier -> state_negatives on a 64 x 48 seeded image: the weights are the
    device's own (its exp), the choice is the model's on them"""
    W, H = 64, 48
    rng = np.random.default_rng(20261021)
    image = np.clip(np.kron(rng.integers(40, 216, (H // 4, W // 4)), np.ones((4, 4))) + rng.integers(-30, 30, (H, W)), 0, 255).astype(np.uint8)
    integral = capi.Integral(ctx)
    integral.update(image)
    hog = capi_params(capi, HOG_CASE)
    s = _samples(257)
    old = cm.generation(len(s), x=s[:, 0], y=s[:, 1], size=s[:, 2], weight=rng.random(len(s)), cluster_id=rng.integers(0, 3, len(s)))
    feats, valid = integral.extract_hog(hog, resident_model.apply_maps(MAPS["resize+integral"], resident_model.sample_xywh(old, ASPECT)))
    m = synth.make_svm_f32(5, feats[valid], nsv=12, positive_fraction=0.4, kernel=0)
    svm = capi.Svm(ctx, m)
    n, copies = 300, 200
    z = rng.standard_normal((copies, 3))
    diffusion = np.stack([2.0 * z[:, 0], 2.0 * z[:, 1], np.exp2(0.05 * z[:, 2])], 1)
    fresh = np.stack([rng.integers(5, W - 5, n - copies), rng.integers(5, H - 5, n - copies), rng.integers(8, 30, n - copies)], 1).astype(np.int32)
    particles.set(**old)
    particles.sample(n, copies, 0.41, diffusion, fresh, 100)
    particles.evaluate_integral(integral, svm, ASPECT, MAPS["resize+integral"], hog=hog)
    particles.weigh_classifier(0.3, -1.7, float(np.float32(m["threshold"])))
    device = particles.get()
    plain = particles.state()
    assert plain["found"] == 1 and 0 < plain["n_valid"] < n and (device["weight"] == 0).any()
    for max_count in COUNTS:
        info, motion, chosen = particles.state_negatives(capi.negatives_params(max_count, 0.3))
        _same_info(info, plain)
        want = model.records(device, model.choose(device, max_count, 0.3, (info["x"], info["y"], info["size"])))
        assert len(want["index"]) == max_count and chosen["index"].tolist() == want["index"].tolist()
        for k in ("x", "y", "size", "weight"):
            assert chosen[k].tobytes() == want[k].tobytes(), k
    _same_generation = {k: device[k].tobytes() for k in cm.FIELDS}
    assert {k: v.tobytes() for k, v in particles.get().items()} == _same_generation
    integral.close()
