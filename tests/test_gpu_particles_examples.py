"""fd_particles_state_examples_integral (k_particles_examples behind k_particles_state, the chosen samples' rows behind that; DESIGN.md
4.7) against tests/self_learning_model.py: both counts and every record bit for bit, the info -- and the motion when a flow is
given -- equal to what fd_particles_state / fd_particles_state_flow report on the same generation, every valid flag and every row bit
for bit what fd_integral_extract_* returns for the chosen samples behind the same chain.  The generations are placed with
fd_particles_set at the sizes around the selection's paths (a partial wavefront, partial quarters of the workgroup, several steps of
64 per wavefront) with 0, max_count - 1, max_count, max_count + 1 and n candidates per side, weights of few distinct values (ties
across the cut), weights exactly on the thresholds, and positions that partly have no patch.  Two generations come out of real chains:
evaluate_integral -> weigh_classifier (the usable branch: require_window on the evaluate's flags) and evaluate_wvm_svm -> weigh_wvm_svm
on a pyramid (the bootstrap branch: the rows come from another extractor than the one that made the weights)."""
import ctypes as C

import numpy as np
import pytest

import condensation_model as cm
import resident_model
import self_learning_model as model
from test_gpu_particles_integral import ASPECT, LOGISTIC_A, LOGISTIC_B, MAPS, _samples, scene   # noqa: F401  (scene: the fixture)
from test_self_learning_model import NEGATIVE, POSITIVE

pytestmark = pytest.mark.gpu

COUNTS = (1, 10, 32)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
CHAIN = MAPS["resize+integral"]
HIGH = np.array([0.75, 0.75, 0.875, 1.0, np.nextafter(POSITIVE, 1)])      # above the positive threshold, with a tie
LOW = np.array([0.0, -0.0, 0.125, 0.125, np.nextafter(NEGATIVE, 0)])      # below the negative one
NEITHER = np.array([POSITIVE, NEGATIVE, 0.5])                               # on either threshold: not chosen


@pytest.fixture(scope="module")
def particles(capi, ctx):
    p = capi.Particles.unbound(ctx, 1024)
    yield p
    p.close()


@pytest.fixture(scope="module")
def flow(capi, ctx):
    f = capi.Flow(ctx, 64, 48)
    f.debug_motion(*resident_model.crafted_tracks(16, 41))
    yield f
    f.close()


def generation(n, n_pos, n_neg, seed, targets=True):
    """n samples at _samples' positions (some without a patch) of which exactly n_pos lie above POSITIVE and n_neg below NEGATIVE"""
    rng = np.random.default_rng(seed)
    s = _samples(n)
    weight = rng.choice(NEITHER, n)
    order = rng.permutation(n)
    weight[order[:n_pos]] = rng.choice(HIGH, n_pos)
    weight[order[n_pos:n_pos + n_neg]] = rng.choice(LOW, n_neg)
    gen = cm.generation(n, x=s[:, 0], y=s[:, 1], size=s[:, 2], weight=weight, cluster_id=rng.integers(5, 8, n).astype(np.int32))
    if targets:
        gen["target"] = (rng.random(n) < 0.4).astype(np.uint8)
    return gen


def _same_info(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array(a[k]).tobytes() == np.array(b[k]).tobytes(), (k, a[k], b[k])


def check(capi, particles, scene, gen, params, kind="hog", maps=CHAIN, flow=None, valid=None, plain=None, integral=None, extract=None):
    """the call on the set's current generation (`gen`: what the device holds) against the plain state call, the model and the
    extract call; returns (info, positives, negatives, rows)"""
    integral = integral or scene["integral"]
    extract = extract or scene["extract"][kind]
    if plain is None:
        plain = particles.state() if flow is None else particles.state_flow(flow)[0]
    info, motion, pos, neg, rows = particles.state_examples(params, integral, ASPECT, maps, flow=flow, **scene["kinds"][kind])
    _same_info(info, plain)
    assert (motion is None) == (flow is None)
    want_pos, want_neg = model.select(gen["weight"], valid, params.positive_threshold, params.negative_threshold, params.max_count, params.require_window)
    chosen = np.concatenate([want_pos, want_neg]).astype(np.int64)
    sub = {k: gen[k][chosen] for k in ("x", "y", "size")}
    want_rows, want_valid = (extract(resident_model.apply_maps(maps, resident_model.sample_xywh(sub, ASPECT))) if len(chosen)
                            else (np.zeros((0, rows.shape[1]), np.float32), np.zeros(0, bool)))
    for got, index, ok in ((pos, want_pos, want_valid[:len(want_pos)]), (neg, want_neg, want_valid[len(want_pos):])):
        want = model.records(gen, index, ok)
        assert got["index"].tolist() == want["index"].tolist(), (got["index"][:12], want["index"][:12])
        for k in ("x", "y", "size", "valid", "weight"):
            assert got[k].tobytes() == want[k].tobytes(), k
    assert rows.shape == want_rows.shape
    want_rows = np.where(want_valid[:, None], want_rows, np.float32(0))   # the row of a record without a patch is not written
    assert rows.tobytes() == want_rows.astype(np.float32).tobytes()
    return info, pos, neg, rows


@pytest.mark.parametrize("max_count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_candidate_count(capi, particles, scene, n, max_count):
    counts = sorted({c for c in (0, max_count - 1, max_count, max_count + 1) if c <= n})
    cases = [(a, b) for a in counts for b in counts if a + b <= n] + [(n, 0), (0, n)]
    params = capi.examples_params(POSITIVE, NEGATIVE, max_count, 0)
    full = 0
    for k, (n_pos, n_neg) in enumerate(cases):
        gen = generation(n, n_pos, n_neg, 100 * n + k)
        particles.set(**gen)
        info, pos, neg, rows = check(capi, particles, scene, gen, params)
        assert len(pos["index"]) == min(n_pos, max_count) and len(neg["index"]) == min(n_neg, max_count) and info["count"] == n
        full += n_pos > max_count or n_neg > max_count
        _same_info(particles.state(), info)   # the generation is untouched
    assert full or n <= max_count


def test_ties_across_the_cut(capi, particles, scene):
    n = 257
    s = _samples(n)
    for value, side in ((0.75, "pos"), (0.125, "neg"), (0.0, "neg")):
        gen = cm.generation(n, x=s[:, 0], y=s[:, 1], size=s[:, 2], weight=np.full(n, value))
        particles.set(**gen)
        info, pos, neg, _ = check(capi, particles, scene, gen, capi.examples_params(POSITIVE, NEGATIVE, 10, 0))
        got = pos if side == "pos" else neg
        assert got["index"].tolist() == list(range(10)) and len((neg if side == "pos" else pos)["index"]) == 0
    # two weights around the cut: 7 of the better one anywhere, then the lowest indices of the tied one
    gen = cm.generation(n, x=s[:, 0], y=s[:, 1], size=s[:, 2], weight=np.full(n, 0.75))
    best = [250, 200, 129, 128, 64, 63, 5]
    gen["weight"][best] = 1.0
    particles.set(**gen)
    _, pos, _, _ = check(capi, particles, scene, gen, capi.examples_params(POSITIVE, NEGATIVE, 10, 0))
    assert pos["index"].tolist() == sorted(best) + [0, 1, 2]


def test_weights_on_the_thresholds(capi, particles, scene):
    n = 70
    s = _samples(n)
    weight = np.where(np.arange(n) % 2 == 0, POSITIVE, NEGATIVE).astype(np.float64)
    weight[[3, 40]] = np.nextafter(NEGATIVE, 0)
    weight[[8, 66]] = np.nextafter(POSITIVE, 1)
    gen = cm.generation(n, x=s[:, 0], y=s[:, 1], size=s[:, 2], weight=weight)
    particles.set(**gen)
    _, pos, neg, _ = check(capi, particles, scene, gen, capi.examples_params(POSITIVE, NEGATIVE, 10, 0))
    assert pos["index"].tolist() == [8, 66] and neg["index"].tolist() == [3, 40]


@pytest.mark.parametrize("kind", ["haar", "surf", "hog"])
def test_rows_of_every_family_behind_a_real_chain(capi, ctx, scene, particles, flow, kind):
    """the usable branch: evaluate_integral -> weigh_classifier, the thresholds taken from the device's own weights, require_window 0
    and 1 on a generation of which a part has no patch; then a generation without any patch"""
    svm, m = scene["svm"][kind], scene["model"][kind]
    gen = {k: v.copy() for k, v in scene["gen"].items()}
    gen["cluster_id"][:] = 3
    particles.set(**gen)
    particles.evaluate_integral(scene["integral"], svm, ASPECT, CHAIN, **scene["kinds"][kind])
    particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, float(np.float32(m["threshold"])))
    device = particles.get()
    valid = particles.trace()[2]
    seen = np.sort(device["weight"][valid == 1])
    assert 0 < valid.sum() < len(valid) and len(seen) > 40
    unique = np.unique(seen)   # the thresholds are weights the device made: more than 10 candidates on either side where the weights allow
    assert len(unique) >= 3
    high = float(max([u for u in unique[:-1] if (seen > u).sum() >= 12] or [unique[-2]]))
    low = float(min([u for u in unique[1:] if (seen < u).sum() >= 12] or [unique[1]]))
    n_high, n_low, n_invalid = int((seen > high).sum()), int((seen < low).sum()), int((valid == 0).sum())
    print("%s: %d valid of %d, %d distinct weights, %d above %r, %d below %r" % (kind, valid.sum(), len(valid), len(unique), n_high, high, n_low, low))
    assert n_high > 0 and n_low > 0
    plain = particles.state()
    for max_count in COUNTS:
        for require_window in (0, 1):
            params = capi.examples_params(high, low, max_count, require_window)
            info, pos, neg, rows = check(capi, particles, scene, device, params, kind, valid=valid, plain=plain)
            assert len(pos["index"]) == min(n_high, max_count) and pos["valid"].all() and rows.shape[1] > 0
            if require_window:
                assert neg["valid"].all() and len(neg["index"]) == min(n_low, max_count)
            else:   # the weight 0 of the samples without a patch comes first
                assert len(neg["index"]) == min(n_invalid + n_low, max_count)
                if n_invalid + n_low > max_count and (seen > 0).all():
                    first = min(n_invalid, max_count)
                    assert not neg["valid"][:first].any() and neg["valid"][first:].all()
    check(capi, particles, scene, device, capi.examples_params(high, low, 10, 1), kind, valid=valid, flow=flow)
    info, motion, _, _, _ = particles.state_examples(capi.examples_params(high, low, 10, 1), scene["integral"], ASPECT, CHAIN, flow=flow, **scene["kinds"][kind])
    assert resident_model.same_motion(motion, particles.state_flow(flow)[1])
    # no sample has a patch
    n = 70
    off = cm.generation(n, x=np.full(n, -100), y=np.arange(n), size=np.full(n, 20))
    particles.set(**off)
    particles.evaluate_integral(scene["integral"], svm, ASPECT, CHAIN, **scene["kinds"][kind])
    particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, 0.0)
    device, valid = particles.get(), particles.trace()[2]
    assert not valid.any() and not device["weight"].any()
    _, pos, neg, _ = check(capi, particles, scene, device, capi.examples_params(high, low, 10, 1), kind, valid=valid)
    assert len(pos["index"]) == 0 and len(neg["index"]) == 0
    _, pos, neg, rows = check(capi, particles, scene, device, capi.examples_params(high, low, 10, 0), kind, valid=valid)
    assert neg["index"].tolist() == list(range(10)) and not neg["valid"].any() and not rows.any()


def test_bootstrap_form_behind_wvm_svm(capi, ctx, synth, oracle):
    """the bootstrap branch: the generation was evaluated by evaluate_wvm_svm on a pyramid chain; the rows come from an integral chain
    on the same frame, in which some of the chosen samples have no patch"""
    from test_gpu_particles_wvm_svm import Scene
    from test_integral_hog_model import capi_params
    from test_gpu_particles_integral import HOG_CASE
    from test_wvm_svm_resident_model import make_particles
    s = Scene(capi, ctx, synth, oracle, 4, positive=True)
    integral = capi.Integral(ctx)
    integral.update(s.frame)
    hog = capi_params(capi, HOG_CASE)
    rows = make_particles(5, 8192)[:300]
    particles = capi.Particles.unbound(ctx, 300)
    particles.set(**cm.generation(len(rows), x=rows[:, 0], y=rows[:, 1], size=rows[:, 2]))
    particles.evaluate_wvm_svm(s.pyr, s.wg, s.sg, 1.0, [("resize", float(np.float32(1.1)), 0.05, -0.05)])
    particles.weigh_wvm_svm(s.wg, s.sg)
    device = particles.get()
    seen = np.sort(device["weight"][device["weight"] > 0])
    assert len(seen) > 30
    fake = dict(kinds={"hog": dict(hog=hog)})
    extract = lambda q: integral.extract_hog(hog, q)   # noqa: E731
    hi, lo = float(seen[-12]), float(seen[15])
    # a chain other than the evaluation's in which some of the chosen positives (all of which had a window there) have no patch
    best = model.select(device["weight"], None, hi, lo, 32, 0)[0]
    sub = {k: device[k][best] for k in ("x", "y", "size")}
    chain = None
    for factor in (1.0, 1.15, 1.3, 1.45, 0.9, 0.75):
        for offset in (0.0, 0.3, -0.3, 0.6):
            candidate = [("resize", factor, offset, 0.0), ("integral",)]
            ok = extract(resident_model.apply_maps(candidate, resident_model.sample_xywh(sub, ASPECT)))[1]
            if chain is None and ok.any() and not ok.all():
                chain = candidate
    assert chain is not None
    print("chain %s" % (chain,))
    some_invalid = False
    for max_count in COUNTS:
        params = capi.examples_params(hi, lo, max_count, 0)
        info, pos, neg, got = check(capi, particles, fake, device, params, "hog", maps=chain, integral=integral, extract=extract)
        assert len(pos["index"]) == min(int((device["weight"] > hi).sum()), max_count) > 0
        assert len(neg["index"]) == min(int((device["weight"] < lo).sum()), max_count) > 0
        print("max_count %d: valid flags %s | %s" % (max_count, pos["valid"].tolist(), neg["valid"].tolist()))
        both = np.concatenate([pos["valid"], neg["valid"]])
        some_invalid |= bool((pos["valid"] == 0).any() and (pos["valid"] == 1).any())
        assert not got[both == 0].any()
    assert some_invalid
    for h in (particles, integral):
        h.close()
    s.close()


def test_no_state_and_bad_weight(capi, particles, scene):
    gen = generation(200, 30, 30, 1, targets=False)   # no target flag: no state; the lists are what they are with one
    particles.set(**gen)
    params = capi.examples_params(POSITIVE, NEGATIVE, 10, 0)
    info, pos, neg, _ = check(capi, particles, scene, gen, params)
    assert info["found"] == 0 and len(pos["index"]) == 10 and len(neg["index"]) == 10
    with_state = dict(gen, target=np.ones(200, np.uint8))
    particles.set(**with_state)
    info, pos2, neg2, _ = check(capi, particles, scene, with_state, params)
    assert info["found"] == 1 and pos2["index"].tolist() == pos["index"].tolist() and neg2["index"].tolist() == neg["index"].tolist()
    for bad in (-1.0, float("nan")):
        gen = generation(200, 30, 30, 1)
        gen["weight"][150] = bad
        particles.set(**gen)
        with pytest.raises(capi.FdError) as plain:
            particles.state()
        with pytest.raises(capi.FdError) as e:
            particles.state_examples(params, scene["integral"], ASPECT, CHAIN, **scene["kinds"]["hog"])
        assert e.value.code == capi.FD_ERR_RUNTIME == plain.value.code and e.value.counts == (0, 0)
        assert str(e.value).split(": ", 2)[-1] == str(plain.value).split(": ", 2)[-1]   # the existing message behind the entry point's name
        assert e.value.info["bad_weight"] == 1 and e.value.info["found"] == 0


def test_arguments(capi, ctx, particles, scene, flow):
    gen = generation(50, 12, 12, 1)
    particles.set(**gen)
    before = particles.state()
    hog = scene["kinds"]["hog"]
    length, capacity = capi.particles_examples_bounds(10, **hog)

    def refused(params, code=None, match="", **kw):
        with pytest.raises(capi.FdError) as e:
            particles.state_examples(params, scene["integral"], ASPECT, kw.pop("maps", CHAIN), **hog, **kw)
        assert e.value.code == (code or capi.FD_ERR_INVALID_ARGUMENT) and match in str(e.value), e.value

    refused(capi.examples_params(POSITIVE, NEGATIVE, 0), match="max_count 0")
    refused(capi.examples_params(POSITIVE, NEGATIVE, 33), match="max_count 33")
    refused(capi.examples_params(float("nan"), NEGATIVE), match="nan")
    refused(capi.examples_params(POSITIVE, float("-inf")), match="-inf")
    refused(capi.fd_particles_examples_params(POSITIVE, NEGATIVE, 10, 2), match="require_window 2")
    refused(capi.examples_params(NEGATIVE, POSITIVE), match="lies above positive_threshold")
    refused(capi.examples_params(POSITIVE, NEGATIVE), match="row_capacity %d" % (capacity - 1), row_capacity=capacity - 1)
    refused(capi.examples_params(POSITIVE, NEGATIVE), match="sample maps", maps=[("integral",)] * 5)
    refused(capi.examples_params(POSITIVE, NEGATIVE, 10, 1), code=capi.FD_ERR_RUNTIME, match="not been evaluated")
    info, motion, n_pos, n_neg, row_length = capi.fd_particles_info(), capi.fd_flow_motion_info(), C.c_int(), C.c_int(), C.c_int()
    pos, neg = (capi.fd_particles_example * 32)(), (capi.fd_particles_example * 32)()
    rows = np.zeros(capacity, np.float32)
    params = capi.examples_params(POSITIVE, NEGATIVE)

    def raw(context, flow_handle, motion_ref):
        return capi.lib().fd_particles_state_examples_integral(context.h, particles.h, flow_handle, scene["integral"].h, capi.INTEGRAL_HOG, C.byref(hog["hog"]),
                                                               ASPECT, None, 0, C.byref(params), C.byref(info), motion_ref, C.byref(n_pos), pos,
                                                               C.byref(n_neg), neg, rows.ctypes.data_as(C.c_void_p), capacity, C.byref(row_length))
    other = capi.Context(0)
    assert raw(other, None, None) == capi.FD_ERR_INVALID_ARGUMENT                 # another context
    assert raw(ctx, flow.h, None) == capi.FD_ERR_INVALID_ARGUMENT                 # a flow without room for its motion
    assert raw(ctx, None, None) == capi.FD_OK and row_length.value == length and n_pos.value == 10 and n_neg.value == 10
    other.close()
    _same_info(particles.state(), before)
