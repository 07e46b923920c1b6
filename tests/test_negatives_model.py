"""tests/negatives_model.py against itself -- the closed form of the additional negatives (the max_count largest under (weight
descending, index ascending), listed by (weight ascending, index descending)) against a literal restatement of the reference's loop
(PositionDependentMeasurementModel.cpp:172-192) -- and against the library's host half: fd_particles_negatives_bounds, the function
k_particles_negatives itself calls, on the model's bounds; the declaration, the export and the binding of
fd_particles_state_negatives, and its argument rules, which need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import condensation_model as cm
import negatives_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = (100, 80, 40)   # x, y, size
COUNTS = (1, 10, 64)
FACTORS = (0.0, 0.3, 0.5)


def generation(n, seed, weights="random", target=TARGET, spread=40):
    """n samples around the target, about half of them inside the box of factor 0.5.  weights: random (few distinct values, so ties
    are everywhere, zeros among them), equal, zero"""
    rng = np.random.default_rng(seed)
    x = target[0] + rng.integers(-spread, spread + 1, n)
    y = target[1] + rng.integers(-spread, spread + 1, n)
    size = np.maximum(1, target[2] + rng.integers(-spread // 2, 2 * spread + 1, n))
    if weights == "random":
        weight = rng.choice(np.concatenate([[0.0, 0.0, 0.0, -0.0], rng.random(6)]), n)
    elif weights == "distinct":
        weight = rng.permutation(n) / float(max(n, 1))
    else:
        weight = np.full(n, 0.25 if weights == "equal" else 0.0)
    return cm.generation(n, x=x, y=y, size=size, weight=weight)


def on_the_bounds(offset_factor, target=TARGET):
    """per bound a sample exactly on it and its two neighbours, everything else at the target: on the bound and beyond it is outside"""
    b = model.bounds(offset_factor, *target)
    rows = []
    for k in range(6):
        for d in (-1, 0, 1):
            s = list(target)
            s[k // 2] = b[k] + d
            rows.append(s)
    rows = np.array(rows)
    return cm.generation(len(rows), x=rows[:, 0], y=rows[:, 1], size=rows[:, 2], weight=np.linspace(0.1, 0.9, len(rows)))


@pytest.mark.parametrize("offset_factor", FACTORS)
@pytest.mark.parametrize("max_count", COUNTS)
def test_closed_form_equals_the_loop(max_count, offset_factor):
    seen_short, seen_full = False, False
    for weights in ("random", "distinct", "equal", "zero"):
        for n in (0, 1, 2, max_count - 1, max_count, max_count + 1, 64, 65, 257):
            for seed in range(4):
                gen = generation(n, 100 * n + seed, weights)
                want = model.reference_loop(gen, max_count, offset_factor, TARGET)
                got = model.choose(gen, max_count, offset_factor, TARGET)
                assert np.array_equal(got, want), (weights, n, seed, got, want)
                candidates = int(model.outside(model.bounds(offset_factor, *TARGET), gen["x"], gen["y"], gen["size"]).sum())
                assert len(got) == min(candidates, max_count)
                seen_short |= 0 < candidates < max_count
                seen_full |= candidates > max_count
    assert seen_full and (seen_short or max_count == 1)


@pytest.mark.parametrize("max_count", COUNTS)
def test_ties_across_the_cut(max_count):
    """max_count + 5 candidates: three above, the rest equal -- the cut falls among the equal ones and takes the lowest indices"""
    n = max_count + 5
    gen = cm.generation(n, x=np.full(n, 0), y=np.full(n, 0), size=np.full(n, 40), weight=np.full(n, 0.5))
    gen["weight"][[1, n - 1, 4]] = [0.75, 0.75, 0.9]
    got = model.choose(gen, max_count, 0.5, TARGET)
    assert np.array_equal(got, model.reference_loop(gen, max_count, 0.5, TARGET))
    equal = [i for i in range(n) if gen["weight"][i] == 0.5][:max(0, max_count - 3)]
    assert got.tolist() == (equal[::-1] + [n - 1, 1, 4])[-max_count:]


@pytest.mark.parametrize("offset_factor", FACTORS)
def test_samples_on_the_bounds(offset_factor):
    gen = on_the_bounds(offset_factor)
    b = model.bounds(offset_factor, *TARGET)
    out = model.outside(b, gen["x"], gen["y"], gen["size"])
    if offset_factor > 0:   # low bounds: below and on the bound outside, above inside; high bounds the other way round
        assert out.reshape(6, 3).tolist() == [[True, True, False], [False, True, True]] * 3
    else:                   # the box is a point: everything is outside
        assert b[0] == b[1] == TARGET[0] and out.all()
    for max_count in COUNTS:
        assert np.array_equal(model.choose(gen, max_count, offset_factor, TARGET), model.reference_loop(gen, max_count, offset_factor, TARGET))


def test_none_outside():
    gen = cm.generation(50, x=np.full(50, TARGET[0]), y=np.full(50, TARGET[1]), size=np.full(50, TARGET[2]), weight=np.linspace(0, 1, 50))
    assert len(model.choose(gen, 10, 0.5, TARGET)) == 0 and len(model.reference_loop(gen, 10, 0.5, TARGET)) == 0


def test_bounds_are_float_arithmetic():
    assert model.bounds(0.5, 100, 80, 40) == [80, 120, 60, 100, 20, 80]
    assert model.bounds(0.3, 100, 80, 40) == [88, 112, 68, 92, 28, 57]      # 1 / 0.7f * 40 = 57.14
    assert model.bounds(0.3, 0, 0, 70)[4:] == [49, 100]                     # 0.7f * 70 = 49.0000008 as a float product: 48.99... in double
    assert model.bounds(0.0, 5, 6, 7) == [5, 5, 6, 6, 7, 7]
    assert model.bounds(1.0, 0, 0, 10)[4:] == [0, model.INT32_MAX]          # an infinite factor saturates
    assert model.bounds(0.5, model.INT32_MAX, 0, 16)[:2] == [model.INT32_MAX - 8, model.INT32_MIN + 7]   # the sums wrap


def test_library_bounds_equal_the_model(capi):
    rng = np.random.default_rng(3)
    for offset_factor in FACTORS + (0.05, 0.9, 0.999, 1.0, 1.5):
        params = capi.negatives_params(10, offset_factor)
        f, down, up = model.scales(offset_factor)
        assert (np.float32(params.offset_factor), np.float32(params.down_scale)) == (f, down)
        assert np.float32(params.up_scale) == up or (np.isinf(up) and np.isinf(params.up_scale))
        cases = [TARGET, (0, 0, 0), (-5, 7, 1), (model.INT32_MAX, model.INT32_MIN, model.INT32_MAX), (3, 4, 16777217), (1, 2, -40)]
        cases += [tuple(int(v) for v in rng.integers(-2000, 2000, 3)) for _ in range(200)]
        for x, y, size in cases:
            assert capi.particles_negatives_bounds(params, x, y, size).tolist() == model.bounds(offset_factor, x, y, size), (offset_factor, x, y, size)


def test_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    for name in ("fd_particles_state_negatives(", "fd_particles_negatives_bounds(", "fd_particles_negatives_params;", "fd_particles_negative;",
                 "#define FD_PARTICLES_NEGATIVES_MAX 64"):
        assert name in header, name
    lib = capi.lib()
    assert lib.fd_particles_state_negatives.restype is C.c_int and len(lib.fd_particles_state_negatives.argtypes) == 8
    assert callable(capi.Particles.state_negatives) and capi.FD_PARTICLES_NEGATIVES_MAX == model.NEGATIVES_MAX
    assert C.sizeof(capi.fd_particles_negative) == 24 and C.sizeof(capi.fd_particles_negatives_params) == 16


def test_bad_arguments_need_no_device(capi):
    lib = capi.lib()
    info, motion, count = capi.fd_particles_info(), capi.fd_flow_motion_info(), C.c_int(7)
    records = (capi.fd_particles_negative * capi.FD_PARTICLES_NEGATIVES_MAX)()

    def call(params, ctx=None, particles=None, flow=None, with_motion=False, with_info=True):
        return lib.fd_particles_state_negatives(ctx, particles, flow, C.byref(params) if params is not None else None, C.byref(info) if with_info else None,
                                                C.byref(motion) if with_motion else None, C.byref(count), records)

    good = capi.negatives_params(10, 0.5)
    for max_count in (0, -1, 65, 1 << 20):
        assert call(capi.fd_particles_negatives_params(max_count, 0.5, 0.5, 2.0)) == capi.FD_ERR_INVALID_ARGUMENT
    for floats in ((float("nan"), 0.5, 2.0), (0.5, float("inf"), 2.0), (1.0, 0.0, float("inf")), (0.5, 0.5, float("-inf"))):
        assert call(capi.fd_particles_negatives_params(10, *floats)) == capi.FD_ERR_INVALID_ARGUMENT
    assert call(capi.negatives_params(10, 1.0)) == capi.FD_ERR_INVALID_ARGUMENT      # 1 / (1 - 1)
    assert call(good) == capi.FD_ERR_INVALID_ARGUMENT                                  # no context, no set
    assert call(None) == capi.FD_ERR_INVALID_ARGUMENT
    assert call(good, with_info=False) == capi.FD_ERR_INVALID_ARGUMENT
    assert call(good, with_motion=True) == capi.FD_ERR_INVALID_ARGUMENT                # a motion without a flow
    assert count.value == 0                                                           # a refused call reports no records
    assert lib.fd_particles_negatives_bounds(None, 0, 0, 0, None) == capi.FD_ERR_INVALID_ARGUMENT
