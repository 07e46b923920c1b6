"""tests/self_learning_model.py, the rule of SelfLearningMeasurementModel::adapt's examples, against an independent
restatement that uses no sort -- a repeated arg-max / arg-min with the index tie-break written out -- against its own properties, and
against the library's host half, fd_particles_examples_select, which runs the comparisons k_particles_examples runs.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

import self_learning_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 10, 32)
SIZES = (0, 1, 2, 9, 10, 11, 31, 32, 33, 63, 64, 65, 257)
POSITIVE, NEGATIVE = 0.625, 0.25   # both exact in binary and among the weights below


def weights(n, seed, kind="random"):
    """random: few distinct values, the thresholds themselves, zeros and -0 among them, so ties are everywhere; distinct; equal"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.choice(np.array([0.0, -0.0, 0.125, NEGATIVE, 0.2, 0.5, POSITIVE, 0.75, 0.75, 0.875, 1.0]), n)
    if kind == "distinct":
        return rng.permutation(n) / float(max(n, 1))
    return np.full(n, 0.75 if kind == "high" else 0.125)


def restated(weight, valid, positive_threshold, negative_threshold, max_count, require_window):
    """no sort: the candidates in index order; where there are too many, max_count times the best remaining one, of equal ones the lowest index"""
    out = []
    for positive, threshold in ((True, positive_threshold), (False, negative_threshold)):
        left = [i for i in range(len(weight)) if (weight[i] > threshold if positive else weight[i] < threshold) and (not require_window or valid[i])]
        if len(left) > max_count:
            chosen = []
            for _ in range(max_count):
                best = left[0]
                for i in left[1:]:   # ascending indices: only a strictly better weight replaces
                    if (weight[i] > weight[best]) if positive else (weight[i] < weight[best]):
                        best = i
                chosen.append(best)
                left.remove(best)
            left = chosen
        out.append(np.array(left, np.int32))
    return out


def cases():
    for kind in ("random", "distinct", "high", "low"):
        for n in SIZES:
            for seed in range(3):
                w = weights(n, 1000 * n + seed, kind)
                valid = (np.random.default_rng(seed + 7).random(n) < 0.7).astype(np.uint8)
                yield kind, n, seed, w, valid


@pytest.mark.parametrize("require_window", [0, 1])
@pytest.mark.parametrize("max_count", COUNTS)
def test_model_equals_the_restatement_and_the_library(capi, max_count, require_window):
    sorted_sides = 0
    for kind, n, seed, w, valid in cases():
        want = restated(w, valid, POSITIVE, NEGATIVE, max_count, require_window)
        got = model.select(w, valid, POSITIVE, NEGATIVE, max_count, require_window)
        native = capi.particles_examples_select(w, capi.examples_params(POSITIVE, NEGATIVE, max_count, require_window), valid)
        for side in range(2):
            assert got[side].tolist() == want[side].tolist(), (kind, n, seed, side)
            assert native[side].tolist() == want[side].tolist(), (kind, n, seed, side)
            sorted_sides += len(want[side]) == max_count and n > max_count
    assert sorted_sides > 0


@pytest.mark.parametrize("max_count", COUNTS)
def test_properties(max_count):
    for kind, n, seed, w, valid in cases():
        for require_window in (0, 1):
            pos, neg = model.select(w, valid, POSITIVE, NEGATIVE, max_count, require_window)
            usable = np.ones(n, bool) if not require_window else valid.astype(bool)
            for positive, chosen in ((True, pos), (False, neg)):
                candidates = np.flatnonzero(((w > POSITIVE) if positive else (w < NEGATIVE)) & usable)
                assert all((w[i] > POSITIVE) if positive else (w[i] < NEGATIVE) for i in chosen)   # strict: a weight on the threshold is no example
                assert all(usable[i] for i in chosen)
                assert len(chosen) == min(len(candidates), max_count)
                if len(candidates) <= max_count:
                    assert chosen.tolist() == candidates.tolist()   # index order, unsorted
                else:
                    key = [((-w[i] if positive else w[i]) + 0.0, i) for i in chosen]
                    assert key == sorted(key)
                    rest = [i for i in candidates if i not in set(chosen.tolist())]
                    assert all((((-w[i] if positive else w[i]) + 0.0, i) > key[-1]) for i in rest)


def test_weights_on_the_thresholds_are_not_chosen():
    w = np.array([POSITIVE, np.nextafter(POSITIVE, 1), NEGATIVE, np.nextafter(NEGATIVE, 0), 0.5])
    pos, neg = model.select(w, None, POSITIVE, NEGATIVE, 10, 0)
    assert pos.tolist() == [1] and neg.tolist() == [3]


@pytest.mark.parametrize("max_count", COUNTS)
def test_a_duplicated_particle_is_a_duplicated_example(max_count):
    """resampling copies particles; the reference keeps both copies"""
    for n in (3, max_count + 5, 100):
        w = weights(n, n, "distinct")
        best, worst = int(np.argmax(w)), int(np.argmin(w))
        w2 = np.concatenate([w, [w[best], w[worst]]])
        pos = model.select(w2, None, -1.0, -1.0, max_count, 0)[0]   # every sample a positive candidate
        neg = model.select(w2, None, 2.0, 2.0, max_count, 0)[1]     # every sample a negative one
        if n + 2 > max_count and max_count >= 2:
            assert pos[:2].tolist() == [best, n] and neg[:2].tolist() == [worst, n + 1]
        elif n + 2 <= max_count:
            assert best in pos and n in pos and worst in neg and n + 1 in neg


def test_bad_weights():
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            model.select(np.array([0.5, bad]), None, POSITIVE, NEGATIVE, 10, 0)


def test_library_arguments_and_declarations(capi):
    w = weights(40, 3)
    for params in (capi.examples_params(POSITIVE, NEGATIVE, 0), capi.examples_params(POSITIVE, NEGATIVE, 33),
                   capi.examples_params(float("nan"), NEGATIVE), capi.examples_params(POSITIVE, float("inf")),
                   capi.fd_particles_examples_params(POSITIVE, NEGATIVE, 10, 2), capi.examples_params(NEGATIVE, POSITIVE)):   # the last: inverted
        with pytest.raises(capi.FdError) as e:
            capi.particles_examples_select(w, params)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError) as e:   # require_window without the flags
        capi.particles_examples_select(w, capi.examples_params(POSITIVE, NEGATIVE, 10, 1))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    for bad in (-1.0, float("nan"), float("inf")):
        w2 = w.copy()
        w2[7] = bad
        with pytest.raises(capi.FdError) as e:
            capi.particles_examples_select(w2, capi.examples_params(POSITIVE, NEGATIVE))
        assert e.value.code == capi.FD_ERR_RUNTIME
    header = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    for name in ("fd_particles_examples_select", "fd_particles_examples_bounds", "fd_particles_state_examples_integral",
                 "fd_particles_state_examples_pyramid"):
        assert name in header and hasattr(capi.lib(), name)
    assert "#define FD_PARTICLES_EXAMPLES_MAX %d" % capi.FD_PARTICLES_EXAMPLES_MAX in header
    assert C.sizeof(capi.fd_particles_example) == 32 and C.sizeof(capi.fd_particles_examples_params) == 24


def test_row_bounds(capi):
    from test_gpu_particles_integral import HOG_CASE
    from test_integral_hog_model import capi_params
    hog = capi_params(capi, HOG_CASE)
    length, capacity = capi.particles_examples_bounds(10, hog=hog)
    assert length == capi.lib().fd_integral_hog_feature_length(C.byref(hog)) > 0 and capacity == 20 * length
    assert capi.particles_examples_bounds(1, surf=(12, 4)) == (64, 128)
    for count in (0, 33):
        with pytest.raises(capi.FdError):
            capi.particles_examples_bounds(count, hog=hog)
