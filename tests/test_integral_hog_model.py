"""Host-only rules of the integral HOG family against tests/integral_hog_model.py: which samples IntegralGradientFilter can serve
(fd_integral_gradient_samples_valid runs the statements of the kernels on the host) and the feature lengths / argument rules of
fd_integral_hog_params (fd_integral_hog_feature_length).  No device is touched."""
import numpy as np
import pytest

import integral_hog_model as model
import integral_model

W, H = 200, 150


def capi_params(capi, case):
    """a case of model.CASES (or a broken variant of one) as fd_integral_hog_params"""
    rows, cols = case["grid"]
    pw, ph = case.get("patch", (cols, rows))
    fbins = case.get("filter_bins", case["bins"])
    if case["filter"] == "ehog":
        flt = dict(ehog=capi.ehog_patch_params(pw, ph, bins=fbins, cell_w=case["cell"], cell_h=case.get("cell_h", 0), interpolate=bool(case.get("interpolate")),
                                               signed_and_unsigned=bool(case.get("sau")), alpha=case.get("alpha", 0.2)))
    else:
        flt = dict(hist=capi.hist_params(case["filter"], pw, ph, 1, 1, bins=fbins, cell=case.get("cell", 0), block=case.get("block", 1),
                                         levels=case.get("levels", 0), interpolate=bool(case.get("interpolate")),
                                         signed_and_unsigned=bool(case.get("sau")), concatenate=bool(case.get("concatenate")),
                                         normalization=case.get("normalization", 0)))
    return capi.integral_hog_params(rows, cols, bins=case["bins"], signed_gradients=bool(case.get("signed")),
                                    interpolate_bins=bool(case.get("interpolate_bins")), **flt)


@pytest.mark.parametrize("grid", [(2, 2), (7, 5), (30, 30), (64, 64)], ids=lambda g: "%dx%d" % g)
def test_gradient_samples_valid(capi, grid):
    samples = integral_model.make_samples(W, H)
    assert len(samples) == 664
    I = integral_model.integral_fast(model.make_frame(W, H, 3))
    _, want = integral_model.gradient_patches(I, grid[0], grid[1], samples)
    assert want.sum() >= 500 and (~want).sum() >= 30   # 624 and 40 for each of the four grids
    got = capi.integral_gradient_samples_valid(W, H, grid[0], grid[1], samples)
    assert got.dtype == bool and np.array_equal(got, want)
    assert len(capi.integral_gradient_samples_valid(W, H, grid[0], grid[1], samples[:0])) == 0


def test_gradient_samples_valid_argument_rules(capi):
    s = integral_model.make_samples(W, H)[:4]
    for args in ((0, H, 4, 4), (W, 0, 4, 4), (W, H, 1, 4), (W, H, 4, 1), (W, H, 16385, 4)):
        with pytest.raises(capi.FdError) as e:
            capi.integral_gradient_samples_valid(*args, s)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", sorted(model.CASES))
def test_feature_length(capi, name):
    case = model.CASES[name]
    want = model.feature_length(case)
    assert want > 0
    assert capi.integral_hog_feature_length(capi_params(capi, case)) == want


BROKEN = {
    "grid-below-2": dict(model.DEFAULT, grid=(1, 30), patch=(30, 1)),
    "grid-cols-below-2": dict(model.DEFAULT, grid=(30, 1), patch=(1, 30)),
    "grid-above-64": dict(model.DEFAULT, grid=(65, 30), patch=(30, 65)),
    "grid-cols-above-64": dict(model.DEFAULT, grid=(30, 65), patch=(65, 30)),
    "patch-width": dict(model.DEFAULT, patch=(29, 30)),
    "patch-height": dict(model.DEFAULT, patch=(30, 31)),
    "patch-swapped": dict(model.DEFAULT, grid=(7, 5), patch=(7, 5)),
    "bins-mismatch": dict(model.DEFAULT, filter_bins=8),
    "bins-zero": dict(model.DEFAULT, bins=0),
    "bins-above-256": dict(model.DEFAULT, bins=257),
    "zero-cell-rows": dict(model.DEFAULT, grid=(2, 30), cell=6),   # cvRound(2 / 6) = 0 rows of cells
    "ehog-patch": dict(model.CASES["ehog20x12"], patch=(20, 12)),
    "ehog-bins-mismatch": dict(model.CASES["ehog20x12"], filter_bins=18),
    "ehog-zero-cell-rows": dict(model.CASES["ehog20x12"], grid=(2, 12), cell=6),
}


@pytest.mark.parametrize("name", sorted(BROKEN))
def test_feature_length_refusals(capi, name):
    case = BROKEN[name]
    assert model.feature_length(case) == -1
    assert capi.integral_hog_feature_length(capi_params(capi, case)) == -1


def test_feature_length_null_and_kind(capi):
    assert capi.integral_hog_feature_length(None) == -1
    hp = capi_params(capi, model.DEFAULT)
    hp.kind = 2
    assert capi.integral_hog_feature_length(hp) == -1


def test_wrapper_maps():
    """IntegralFeatureExtractor.hpp:36-47 and PatchResizingFeatureExtractor.hpp:41-52 on a few hand-computed samples"""
    assert model.integral_extractor_map((10, 20, 30, 40)) == (10, 20, 31, 41)
    assert model.integral_extractor_map((10, 20, 31, 40)) == (11, 20, 32, 41)
    assert model.integral_extractor_map((10, 20, 30, 41)) == (10, 21, 31, 42)
    assert model.patch_resizing_map((10, 20, 30, 45), 1.1) == (10, 20, 33, 50)        # 49.5 rounds to the even 50
    assert model.patch_resizing_map((10, 20, 25, 35), 1.1) == (10, 20, 28, 38)        # 27.5 -> 28, 38.5 -> 38
    assert model.patch_resizing_map((10, 20, 30, 40), 1.0, 0.25, -0.5) == (18, 0, 30, 40)   # 17.5 -> 18
    got = model.map_samples([(10, 20, 30, 45)], scale=1.1)
    assert got.tolist() == [[11, 20, 34, 51]]                                        # resized to 33 x 50, then the odd width moves x
