"""fd_aggregated_plan_layers (host only, no GPU): the layer list of the approximated feature pyramid
(ImagePyramid::createApproximated, ImagePyramid.cpp:51-63,200-235 behind AggregatedFeaturesExtractor's scale limits) against the
Python model of tests/aggregated_approx_model.py -- index, approximated flag, parent, the three scales as exact doubles, rows and
columns -- including the cases that hang on rounding: the dropped smallest layer at n = 2 / 3 and maxScale < 1."""
import itertools
import math

import pytest

import aggregated_approx_model as model

SIZES = [(640, 480), (1280, 720), (1920, 1080), (333, 517)]
WINDOWS = [(8, 8), (10, 12)]
CELLS = [4, 8]
NS = [1, 2, 3, 4, 8]


def _grid():
    for n, (w, h), (ww, wh), cell, wide in itertools.product(NS, SIZES, WINDOWS, CELLS, (False, True)):
        yield n, w, h, ww, wh, cell, (int(1.5 * ww * cell) if wide else 0)


def _check(capi, n, w, h, ww, wh, cell, min_width):
    want = model.plan(ww, wh, cell, n, min_width, w, h)
    if want is None:
        with pytest.raises(capi.FdError) as e:
            capi.aggregated_plan_layers(ww, wh, cell, n, min_width, w, h)
        assert e.value.code == capi.FD_ERR_RUNTIME
        return None
    got = capi.aggregated_plan_layers(ww, wh, cell, n, min_width, w, h)
    assert len(got) == len(want)
    for g, m in zip(got, want):
        for key in ("index", "approximated", "parent", "rows", "cols"):
            assert int(g[key]) == m[key], (key, g, m)
        for key in ("scale", "scale_x", "scale_y"):
            assert float(g[key]) == m[key], (key, g, m)   # exact doubles
    return want


@pytest.mark.parametrize("n", NS)
def test_plan_matches_model_on_the_grid(capi, n):
    cases = [c for c in _grid() if c[0] == n]
    assert len(cases) == 32
    checked = 0
    for c in cases:
        checked += _check(capi, *c) is not None
    assert checked > 16


def test_plan_exact_layers_only_for_one_layer_per_octave(capi):
    got = capi.aggregated_plan_layers(8, 8, 8, 1, 0, 640, 480)
    assert len(got) >= 2 and not got["approximated"].any() and (got["parent"] == -1).all()
    assert [float(s) for s in got["scale"]] == [0.5 ** j for j in range(len(got))]


def test_plan_drops_the_smallest_layer_where_rounding_says_so(capi):
    """0.5^j * pow(inc, i) >= pow(inc, L) fails in double at many L for n = 2 and n = 3 (the smallest approximated layer is then
    absent) and holds for n = 4 and 8: the grid must contain both, and the library must agree with the model on each."""
    dropped, present = {}, {}
    for n, w, h, ww, wh, cell, min_width in _grid():
        if n == 1:
            continue
        want = _check(capi, n, w, h, ww, wh, cell, min_width)
        if want is None:
            continue
        min_scale, _ = model.limits(ww, wh, cell, n, min_width, w, h)
        inc = math.pow(0.5, 1.0 / n)
        L = round(math.log(min_scale) / math.log(inc))
        if L % n == 0:
            continue   # the smallest layer is an exact one
        has = abs(want[-1]["scale"] - min_scale) < 1e-12
        (present if has else dropped).setdefault(n, []).append((w, h, ww, wh, cell, min_width))
    assert dropped.get(2) and dropped.get(3), "the grid lost its n = 2 / 3 cases with a dropped smallest layer"
    assert not dropped.get(4) and not dropped.get(8)
    assert present.get(4) and present.get(8)


def test_plan_has_no_layers_between_half_and_max_scale(capi):
    """maxScale < 1: the scale-1 source layer is not kept, so nothing exists in (0.5, maxScale] although maxScale > 0.5"""
    seen = 0
    for n, w, h, ww, wh, cell, min_width in _grid():
        if not min_width or n == 1:
            continue
        _, max_scale = model.limits(ww, wh, cell, n, min_width, w, h)
        assert 0.5 < max_scale < 1.0
        if model.plan(ww, wh, cell, n, min_width, w, h) is None:
            continue   # a single octave left: the error case
        got = capi.aggregated_plan_layers(ww, wh, cell, n, min_width, w, h)
        assert float(got["scale"].max()) == 0.5 and int(got[0]["index"]) == n and not got[0]["approximated"]
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("w,h,ww,wh,cell", [(100, 100, 8, 8, 8), (70, 90, 10, 12, 4), (64, 64, 8, 8, 8)])
def test_plan_too_small_image_is_an_error(capi, w, h, ww, wh, cell):
    """fewer than two source layers: ImagePyramid::estimateLambdas throws runtime_error (ImagePyramid.cpp:238-239)"""
    assert model.plan(ww, wh, cell, 8, 0, w, h) is None
    with pytest.raises(capi.FdError) as e:
        capi.aggregated_plan_layers(ww, wh, cell, 8, 0, w, h)
    assert e.value.code == capi.FD_ERR_RUNTIME


def test_plan_rejects_bad_arguments(capi):
    for args in [(0, 8, 8, 8, 0, 640, 480), (8, 8, 0, 8, 0, 640, 480), (8, 8, 8, 0, 0, 640, 480), (8, 8, 8, 8, 0, 0, 480)]:
        with pytest.raises(capi.FdError) as e:
            capi.aggregated_plan_layers(*args)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
